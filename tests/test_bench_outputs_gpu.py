"""-m gpu: a plain `bench.py --gpus 1 --steps K --warmup W` run prints the headline line and nothing of `--full`, honours --steps,
and `--dump-outputs DIR` writes the predictions of the last timed step — the same numbers the CPU oracle computes for the bench's
seeded batch and weights, and the same bytes in a second run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import parity_util as PU

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("cold", "sequential", "overlap_mode", "sustained", "device", "strict_mode", "layer_path", "protocol_8d", "roofline",
             "kernels", "all_eigenvectors", "pipelined", "cpu_baseline", "vs_cpu_baseline", "scatter_roofline")


def _bench(dump, steps=7, warmup=3):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    d = _bench(tmp_path / "a")
    assert d["steps"] == 7 and d["warmup"] == 3 and d["full"] is False
    assert d["metric"] == "graphs/sec SignNet+GINE forward, ZINC batch=128 k=16"
    assert d["unit"] == "graphs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and abs(d["value"] - 128 * 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d], [k for k in FULL_ONLY if k in d]
    y = np.load(tmp_path / "a" / "y.npy")
    assert y.dtype == np.float32 and y.shape == (128, 1) and np.isfinite(y).all()

    # the bench's own batch and weights (seeded) through the CPU oracle, fp32 and float64
    sys.path.insert(0, ROOT)
    import bench
    from oracle import pyg_signnet as O
    from signnet_basisnet_amd import synth
    w = bench.WORKLOADS[1]
    host = synth.make_batch(w["B"], seed=1234 + 2, n_lo=w["n_lo"], n_hi=w["n_hi"], features=w["features"])
    sd = {k: v.detach().clone() for k, v in bench.build_model("cpu").state_dict().items()}
    cfg = O.make_cfg(w["variant"], w["node_feat"], w["edge_feat"], w["hidden"], w["n_out"], w["nl_signnet"], w["nl_gnn"])
    with torch.no_grad():
        ref = O.signnet_gnn(sd, cfg, host, training=False, max_k=w["k"])
        sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
        ref64 = O.signnet_gnn(sd64, cfg, PU.data_f64(host), training=False, max_k=w["k"])
    PU.close(torch.from_numpy(y), ref, "bench --dump-outputs y vs the CPU oracle", ref64=ref64)

    # same arguments, same inputs: the same outputs (other step counts time other loops of the same forward)
    _bench(tmp_path / "b", steps=2, warmup=1)
    assert np.array_equal(np.load(tmp_path / "b" / "y.npy"), y)
