"""What dropout in the sign-invariant encoders costs, on the protocol of profiles/scripts/dropout.py.

  launch   sn_affine_dropout_f32 against the two launches it replaces (sn_masked_affine_f32 with scale / shift, then sn_dropout_f32) at
           [24 008, 68] (row-vector path), [24 008, 95] and [111 037, 67] (flat-vector path) and a strided view of [24 008, 72] with 67
           columns (scalar path, through the C ABI): HIP events around 200 back-to-back launches, the candidates alternating pass by pass
           in one process, median and range over five passes
  train    train_graph.DGLBucketedStep ms/step of `gatedgcn` (k = 8) and `gatedgcn_mask` (k = 37) at their shipped sizes with the classes of
           dropout_signinv.py at dropout 0 and 0.1: the batches and the pass protocol of profiles/scripts/dgl_bucketed_train.py, the two
           loops alternating pass by pass
  p0       the regression check's unit: the same two configs at dropout 0 with the classes of dgl_nets in the tree given by --tree — run
           once per process for the parent commit's tree and for this tree, alternating, three rounds (profiles/dropout.json's
           `parent_ab_same_box`)
  merge    the partial results (one JSON file per run above) into profiles/signinv_dropout.json

    python profiles/scripts/signinv_dropout.py launch|train OUT.json
    python profiles/scripts/signinv_dropout.py p0 OUT.json --tree PATH
    python profiles/scripts/signinv_dropout.py merge OUT.json COMMIT LAUNCH.json TRAIN.json P0_parent_1.json P0_this_1.json ...
"""
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if "--tree" in sys.argv:
    i = sys.argv.index("--tree")
    ROOT = os.path.abspath(sys.argv[i + 1])
    del sys.argv[i:i + 2]
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles", "scripts"))

P = 0.1
REPS = 200
CONFIGS = ("gatedgcn", "gatedgcn_mask")


def _summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), passes=v)


def launch_times():
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import _lib as L
    from signnet_basisnet_amd import ops
    DEV = base.DEV
    snap = ops.DropoutState(seed=1, device=DEV).snapshot()
    thr, ps = ops.dropout_threshold(P)
    out = []
    for R, C, ld in ((24008, 68, 68), (24008, 95, 95), (111037, 67, 67), (24008, 67, 72)):
        xb, yb, mb = (torch.randn(R, ld, device=DEV) for _ in range(3))
        x, y, mid = xb[:, :C], yb[:, :C], mb[:, :C]
        sc, sh = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
        path = "row-vector" if C % 4 == 0 else ("flat-vector" if ld == C else "scalar")

        def fused():
            L.check(L.lib().sn_affine_dropout_f32(L.ptr(x), ld, R, C, None, 0, L.ptr(sc), L.ptr(sh), thr, ps, L.ptr(snap), ops.SIGNINV_DROP_SITE,
                                                  0, L.ptr(y), ld, L.stream()), "sn_affine_dropout_f32")

        def composed():
            L.check(L.lib().sn_masked_affine_f32(L.ptr(x), ld, R, C, None, 0, ops.EPI_AFFINE, L.ptr(sc), L.ptr(sh), None, 0, L.ptr(mid), ld,
                                                 L.stream()), "sn_masked_affine_f32")
            L.check(L.lib().sn_dropout_f32(L.ptr(mid), ld, R, C, thr, ps, L.ptr(snap), ops.SIGNINV_DROP_SITE, 0, None, 0, L.ptr(y), ld,
                                           L.stream()), "sn_dropout_f32")

        def affine_only():
            L.check(L.lib().sn_masked_affine_f32(L.ptr(x), ld, R, C, None, 0, ops.EPI_AFFINE, L.ptr(sc), L.ptr(sh), None, 0, L.ptr(mid), ld,
                                                 L.stream()), "sn_masked_affine_f32")

        cands = {"sn_affine_dropout_f32": fused, "masked_affine_then_dropout": composed, "sn_masked_affine_f32_alone": affine_only}
        composed()
        ref = y.clone()
        fused()
        same = bool(torch.equal(y.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)))
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
        r = dict(rows=R, cols=C, ld=ld, path=path, p=P, launches=REPS, bytes_fused=2 * R * C * 4, bytes_composed=4 * R * C * 4,
                 bit_equal=same, us_per_launch={k: _summary(v) for k, v in us.items()})
        f, c = r["us_per_launch"]["sn_affine_dropout_f32"]["median"], r["us_per_launch"]["masked_affine_then_dropout"]["median"]
        r["fused_over_composed"] = f / c
        r["fused_GBps"] = r["bytes_fused"] / f / 1e3
        out.append(r)
        print(f"[{R}, {C}] ld {ld} ({path}): " + ", ".join(f"{k} {v['median']:.2f} us [{v['min']:.2f}, {v['max']:.2f}]"
                                                              for k, v in r["us_per_launch"].items()) + f"  bit-equal {same}", flush=True)
    return out


def _step(name, nets, p):
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import dgl_configs, optim
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    cls, cfg = dgl_configs.net_params(name, base.DEV)
    torch.manual_seed(0)
    net = getattr(nets, cls)(dict(cfg, dropout=p)).to(base.DEV).train()
    o = optim.FlatAdam(net.parameters(), lr=1e-4)
    return net, o, DGLBucketedStep(net, o, max_graphs=base.GRAPHS, granule=base.GRANULE, max_captures=4)


def train_times(ps, module):
    import importlib
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import dgl_configs
    nets = importlib.import_module("signnet_basisnet_amd." + module)
    runs = []
    for name in CONFIGS:
        batches = base._batches(dgl_configs.SHIPPED[name]["pos_enc_dim"])
        keep = {p: _step(name, nets, p) for p in ps}
        loops = {f"bucketed_p{p:g}": (lambda b, s=keep[p][2]: s.step(b["g"], b["h"], b["p"], b["e"], None, b["t"])) for p in ps}
        first = {k: base._pass(fn, batches) for k, fn in loops.items()}          # captures, lazy setup
        ms = {k: [] for k in loops}
        for _ in range(base.PASSES):
            for k, fn in loops.items():
                ms[k].append(base._pass(fn, batches))
        enc = keep[ps[0]][0].sign_inv_net
        r = dict(config=name, k=enc.k, sign_inv_layers=len(enc.enc.layers), classes=module, batches=len(batches), graphs=base.GRAPHS,
                 first_pass_ms_per_step=first, ms_per_step={k: _summary(v) for k, v in ms.items()}, captures=[])
        for net, o, step in keep.values():
            step.check()
            r["captures"].append(step.captures)
            step.release()
        del keep, loops
        torch.cuda.empty_cache()
        runs.append(r)
        for k, v in r["ms_per_step"].items():
            print(f"{name} {k}: {v['median']:.2f} ms/step [{v['min']:.2f}, {v['max']:.2f}]", flush=True)
    return runs


def merge(out, commit, launch, train, p0_files):
    res = dict(commit=commit, device=json.load(open(launch))["device"], launch=json.load(open(launch))["launch"],
               train=json.load(open(train))["train"])
    runs = [json.load(open(f)) for f in p0_files]
    ab = dict(note="dropout 0, classes of dgl_nets, bucketed ms/step (median of five passes) of the parent commit's tree and of this tree, "
                   "separate processes alternating three times on one device in one session", runs=[])
    for r in runs:
        ab["runs"].append(dict(tree=r["tree"], **{t["config"]: t["ms_per_step"]["bucketed_p0"] for t in r["train"]}))
    verdict = {}
    for name in CONFIGS:
        par = [p for r in ab["runs"] if r["tree"] == "parent" for p in r[name]["passes"]]
        med = [r[name]["median"] for r in ab["runs"] if r["tree"] == "this"]
        if par and med:
            verdict[name] = dict(parent_pass_range_ms=[min(par), max(par)], this_medians_ms=med,
                                 inside=bool(all(min(par) <= m <= max(par) for m in med)))
    ab["verdict"] = verdict
    res["parent_ab_same_box"] = ab
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(verdict))


def main():
    mode, out = sys.argv[1], sys.argv[2]
    if mode == "merge":
        return merge(out, sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6:])
    import bench
    import dgl_bucketed_train as base
    res = dict(device=bench.device_block(base.DEV))
    if mode == "launch":
        res["launch"] = launch_times()
    elif mode == "train":
        res["train"] = train_times((0.0, P), "dropout_signinv")
    elif mode == "p0":
        res["tree"] = "this" if os.path.samefile(ROOT, os.path.dirname(os.path.dirname(HERE))) else "parent"
        res["train"] = train_times((0.0,), "dgl_nets")
    else:
        raise SystemExit(__doc__)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
