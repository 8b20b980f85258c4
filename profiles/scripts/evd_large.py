"""Timing of the eigendecomposition pre-transform on batches with graphs of 65 .. 128 nodes -> profiles/evd_large.json.

One process, every shape warmed up, the routes alternating in >= 5 rounds, host wall clock around synchronised windows (the library
route is host-bound: device events alone would flatter it), median [min - max] per route.
  W1  128 graphs with sizes uniform in 65 .. 128 (seeded)
  W2  the bench's 128 ZINC-like graphs plus one 70-node graph
      routes: "kernel"  = transform.evd_laplacian_batch as it stands (sn_laplacian_evd_f32 + sn_laplacian_evd_large_f32),
              "library" = the route before the mid-size kernel: sn_laplacian_evd_f32, a status read, then dense Laplacian +
                          torch.linalg.eigh per graph above 64 nodes (transform._dense_eigh_on_device, still in the file)
  W3  the bench's 128 ZINC-like graphs alone: this tree against a build of the parent commit (--parent DIR: a checkout of it with its
      library built), loaded side by side under another module name — the kernels of that path are untouched, so the readings must
      interleave.
Run from the repository root:  python profiles/scripts/evd_large.py [--parent DIR] [--rounds 7] [--out profiles/evd_large.json]
"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from signnet_basisnet_amd import ops, synth              # noqa: E402
from signnet_basisnet_amd import transform as T          # noqa: E402

DEV = "cuda:0"


def load_parent(path):
    """The parent commit's package under the name signnet_basisnet_amd_parent (its own libsignnet_hip.so, its own ctypes handle)."""
    pkg = os.path.join(path, "signnet_basisnet_amd")
    spec = importlib.util.spec_from_file_location("signnet_basisnet_amd_parent", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["signnet_basisnet_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("signnet_basisnet_amd_parent.transform")


def library_route(edge_index, gp, sizes, norm):
    """What evd_laplacian_batch did before the mid-size kernel existed."""
    N, total = sum(sizes), sum(v * v for v in sizes)
    val, vec, evoff, pe, status = ops.laplacian_evd(edge_index, gp, N, total, norm)
    st = int(status[0].item())
    assert st & ~2 == 0
    if st & 2:
        n0 = off = 0
        for n in sizes:
            if n > 64:
                D, V = T._dense_eigh_on_device(edge_index, n0, n, norm)
                val[n0:n0 + n] = D
                vec[off:off + n * n] = V.reshape(-1)
            n0 += n
            off += n * n
    return val, vec


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def summary(xs):
    return {"median_ms": statistics.median(xs), "min_ms": min(xs), "max_ms": max(xs), "rounds_ms": xs}


def alternate(routes, rounds, iters):
    for fn in routes.values():
        for _ in range(3):
            fn()                                   # warm-up: every shape, every route
    out = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            out[k].append(window(fn, iters))
    return {k: summary(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evd_large.json"))
    a = ap.parse_args()
    norm = "sym"
    res = {"device": torch.cuda.get_device_name(0), "norm": norm, "rounds": a.rounds}

    def gptr(sizes):
        return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)

    # W1
    rng = np.random.default_rng(2024)
    sizes1 = [int(v) for v in rng.integers(65, 129, size=128)]
    b1 = synth.make_batch(128, seed=2024, sizes=sizes1)
    e1, g1 = b1.edge_index.to(DEV), gptr(sizes1)
    # W2 / W3: the bench's batch (bench.py: synth.make_batch(128, seed=1236)) and the same plus one 70-node graph
    b3 = synth.make_batch(128, seed=1236)
    sizes3 = list(b3.sizes)
    e3, g3 = b3.edge_index.to(DEV), gptr(sizes3)
    b70 = synth.make_batch(1, seed=170, sizes=[70])
    sizes2 = sizes3 + [70]
    e2 = torch.cat([b3.edge_index, b70.edge_index + sum(sizes3)], 1).contiguous().to(DEV)
    g2 = gptr(sizes2)

    # the two routes agree (eigenvalues; the vectors are checked by tests/test_evd_large_gpu.py)
    for e, g, s in ((e1, g1, sizes1), (e2, g2, sizes2)):
        dk = T.evd_laplacian_batch(e, ptr=g, sizes=s, norm=norm)[0]
        dl = library_route(e, g, s, norm)[0]
        assert float((dk - dl).abs().max()) < 1e-5

    res["W1"] = alternate({"kernel": lambda: T.evd_laplacian_batch(e1, ptr=g1, sizes=sizes1, norm=norm),
                           "library": lambda: library_route(e1, g1, sizes1, norm)}, a.rounds, 5)
    res["W2"] = alternate({"kernel": lambda: T.evd_laplacian_batch(e2, ptr=g2, sizes=sizes2, norm=norm),
                           "library": lambda: library_route(e2, g2, sizes2, norm)}, a.rounds, 20)
    routes3 = {"this": lambda: T.evd_laplacian_batch(e3, ptr=g3, sizes=sizes3, norm=norm)}
    if a.parent:
        TP = load_parent(a.parent)
        routes3["parent"] = lambda: TP.evd_laplacian_batch(e3, ptr=g3, sizes=sizes3, norm=norm)
    routes3["this_again"] = routes3["this"]
    res["W3"] = alternate(routes3, a.rounds, 50)

    # the mid-size launch alone (W1), device time, and its cost per rotation step
    N, total = sum(sizes1), sum(v * v for v in sizes1)
    val, vec, evoff, pe, st = ops.laplacian_evd(e1, g1, N, total, norm)
    t = []
    for _ in range(a.rounds + 2):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        stl = ops.laplacian_evd_large(e1, g1, N, total, evoff, val, vec, None, norm)
        ev1.record()
        torch.cuda.synchronize()
        t.append(ev0.elapsed_time(ev1))
    sweeps = int(stl[1])
    res["W1_large_call_alone"] = {**summary(t[2:]), "status": int(stl[0]), "largest_sweep_count": sweeps,
                                  "us_per_step": statistics.median(t[2:]) * 1e3 / (sweeps * 127)}
    one = synth.make_batch(1, seed=228, sizes=[128])
    eo, go = one.edge_index.to(DEV), gptr([128])
    val, vec, evoff, pe, st = ops.laplacian_evd(eo, go, 128, 128 * 128, norm)
    t = []
    for _ in range(a.rounds + 2):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        stl = ops.laplacian_evd_large(eo, go, 128, 128 * 128, evoff, val, vec, None, norm)
        ev1.record()
        torch.cuda.synchronize()
        t.append(ev0.elapsed_time(ev1))
    sweeps = int(stl[1])
    res["one_128_node_graph"] = {**summary(t[2:]), "sweeps": sweeps, "us_per_step": statistics.median(t[2:]) * 1e3 / (sweeps * 127)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: ({r: (round(v["median_ms"], 4), round(v["min_ms"], 4), round(v["max_ms"], 4)) for r, v in w.items()}
                          if k in ("W1", "W2", "W3") else w) for k, w in res.items()}, default=str))


if __name__ == "__main__":
    main()
