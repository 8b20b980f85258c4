"""What train-mode dropout costs: the sn_dropout_f32 launch next to sn_pointwise_f32 with a residual at the same shape (the same traffic, no
generator; its code is the parent's), and a GatedGCN NoPE training step (GatedGCN_ZINC_NoPE.json: hidden 77, 16 layers) at dropout 0 and
0.1, eager and through train_graph.DGLBucketedStep.

Launch time: [3001, 128] (vector path) and [E, 77] (scalar path) of the headline batch, HIP events around 200 back-to-back launches, the
three candidates alternating pass by pass in one process, median and range over five passes.  torch's F.dropout + add on the device
is there as context only (two launches, a stored mask).
Training time: the protocol of profiles/scripts/pe_baselines.py (16 shuffled batches of 128 ZINC-like molecules, whole passes timed on the
host, five passes, the four loops alternating).  The p = 0 rows are checked against the pass-to-pass range profiles/pe_baselines.json
records for the parent.

    python profiles/scripts/dropout.py [out.json]        (default: profiles/dropout.json)
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
import dgl_bucketed_train as base  # noqa: E402
from signnet_basisnet_amd import dgl_configs, dropout_models, ops, optim  # noqa: E402
from signnet_basisnet_amd.train_graph import DGLBucketedStep  # noqa: E402

DEV = base.DEV
P = 0.1
REPS = 200
CONFIG = "gatedgcn_nope"


def _summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), passes=v)


def launch_times():
    E = base._batches(8)[0]["E"]
    snap = ops.DropoutState(seed=1, device=DEV).snapshot()
    out = []
    for R, C in ((3001, 128), (E, 77)):
        x, r = torch.randn(R, C, device=DEV), torch.randn(R, C, device=DEV)
        cands = {"sn_dropout_f32": lambda: ops.dropout(x, P, snap, 0, residual=r),
                 "sn_pointwise_f32": lambda: ops.pointwise(x, residual=r),
                 "torch_dropout_add": lambda: F.dropout(x, P, True) + r}
        us = {k: [] for k in cands}
        for fn in cands.values():
            for _ in range(20):
                fn()
        for _ in range(base.PASSES):
            for k, fn in cands.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / REPS)      # (back-to-back launches: includes the host's issue rate)
        out.append(dict(rows=R, cols=C, path="vector" if C % 4 == 0 else "scalar", p=P, launches=REPS, bytes=3 * R * C * 4,
                        us_per_launch={k: _summary(v) for k, v in us.items()}))
    return out


def _net(p):
    cls, cfg = dgl_configs.net_params(CONFIG, DEV)
    cfg = dict(cfg, dropout=p)
    torch.manual_seed(0)
    net = dropout_models.NETS[cls](cfg).to(DEV).train()      # (at p = 0: dgl_nets' class with one class attribute changed)
    return net, optim.FlatAdam(net.parameters(), lr=1e-4)


def train_times():
    loops, keep = {}, []
    batches = None
    for p in (0.0, P):
        net2, o2 = _net(p)
        if batches is None:
            batches = base._batches(net2.pos_enc_dim)
        step = DGLBucketedStep(net2, o2, max_graphs=base.GRAPHS, granule=base.GRANULE, max_captures=4)
        net, o = _net(p)

        def eager(b, net=net, o=o):          # train_ZINC_graph_regression.py:66-81 (the per-step loss.item() of :82 left out)
            o.zero_grad()
            y, _ = net(b["g"], b["h"], None, b["e"], None)
            net.loss(y, b["t"]).backward()
            o.step()

        loops[f"eager_p{p:g}"] = eager
        loops[f"bucketed_p{p:g}"] = lambda b, step=step: step.step(b["g"], b["h"], None, b["e"], None, b["t"])
        keep.append((step, net, o, net2, o2))
    first = {k: base._pass(fn, batches) for k, fn in loops.items()}          # captures, lazy setup
    ms = {k: [] for k in loops}
    for _ in range(base.PASSES):
        for k, fn in loops.items():
            ms[k].append(base._pass(fn, batches))
    res = dict(config=CONFIG, hidden=keep[0][1].embedding_h.weight.shape[1], layers=len(keep[0][1].layers), batches=len(batches),
               graphs=base.GRAPHS, p=P, first_pass_ms_per_step=first, ms_per_step={k: _summary(v) for k, v in ms.items()})
    for step, *_ in keep:
        step.check()
        res.setdefault("captures", []).append(step.captures)
        step.release()
    return res


def regression_check(train):
    """The p = 0 rows against the parent's pass-to-pass range of the same config in profiles/pe_baselines.json."""
    path = os.path.join(ROOT, "profiles", "pe_baselines.json")
    ref = next(r for r in json.load(open(path))["runs"] if r["config"] == CONFIG)
    out = {}
    for kind in ("eager", "bucketed"):
        lo, hi = min(ref[f"{kind}_passes_ms"]), max(ref[f"{kind}_passes_ms"])
        got = train["ms_per_step"][f"{kind}_p0"]["median"]
        out[kind] = dict(parent_range_ms=[lo, hi], p0_median_ms=got, inside=bool(lo <= got <= hi))
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dropout.json")
    res = dict(device=bench.device_block(DEV), launch=launch_times())
    res["train"] = train_times()
    res["regression_check"] = regression_check(res["train"])
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["launch"]:
        print(f"[{r['rows']}, {r['cols']}] ({r['path']}): " + ", ".join(
            f"{k} {v['median']:.2f} us [{v['min']:.2f}, {v['max']:.2f}]" for k, v in r["us_per_launch"].items()))
    for k, v in res["train"]["ms_per_step"].items():
        print(f"{k}: {v['median']:.2f} ms/step [{v['min']:.2f}, {v['max']:.2f}]")
    print("regression check", json.dumps(res["regression_check"]))


if __name__ == "__main__":
    main()
