"""What `--sign_inv_activation tanh | elu` costs, on the protocol of profiles/scripts/signinv_dropout.py.

  launch   sn_act_affine_f32 (with scale / shift) and sn_act_affine_bwd_f32 for tanh and elu at [24 008, 68] (row-vector path),
           [24 008, 95] and [111 037, 67] (flat-vector path), next to sn_masked_affine_f32 with SN_EPI_RELU_PRE | SN_EPI_AFFINE at the same
           shapes (the same traffic, no transcendental): HIP events around 200 back-to-back launches, the candidates alternating pass by
           pass in one process, median and range over five passes.  Report only: the transcendental costs what it costs.
  encoder  GINDeepSigns eval forward at the shipped `gatedgcn` shape (hidden 95, k = 8, 8 layers, 128 graphs): relu on the fused
           three-launch path, relu on the layer path, tanh on the layer path, with the recorded launch counts — the difference between
           the first and the third is the fused forward, not the activation
  train    train_graph.DGLBucketedStep ms/step of `gatedgcn` (k = 8) with the classes of activation_signinv.py, relu vs tanh: batches
           and pass protocol of profiles/scripts/dgl_bucketed_train.py, the two loops alternating pass by pass
  relu     the regression check's unit: the relu encoder forward (fused) and the relu bucketed step with the classes of dgl_nets in the
           tree given by --tree — run once per process for the parent commit's tree and for this tree, alternating, three rounds
  merge    the partial results (one JSON file per run above) into profiles/signinv_activation.json

    python profiles/scripts/signinv_activation.py launch|encoder|train OUT.json
    python profiles/scripts/signinv_activation.py relu OUT.json --tree PATH
    python profiles/scripts/signinv_activation.py merge OUT.json COMMIT LAUNCH.json ENCODER.json TRAIN.json RELU_parent_1.json RELU_this_1.json ...
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

REPS = 200
CONFIG = "gatedgcn"


def _summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), passes=v)


def _timed(cands, passes, reps, unit=1e3):
    import torch
    out = {k: [] for k in cands}
    for fn in cands.values():
        for _ in range(max(3, reps // 10)):
            fn()
    for _ in range(passes):
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) * unit / reps)      # (back-to-back launches: includes the host's issue rate)
    return {k: _summary(v) for k, v in out.items()}


def launch_times():
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import _lib as L
    from signnet_basisnet_amd import ops
    DEV = base.DEV
    out = []
    for R, C in ((24008, 68), (24008, 95), (111037, 67)):
        x, y, dy = (torch.randn(R, C, device=DEV) for _ in range(3))
        a = torch.tanh(x)
        sc, sh = torch.rand(C, device=DEV) + 0.5, torch.randn(C, device=DEV)
        path = "row-vector" if C % 4 == 0 else "flat-vector"

        def relu_affine():
            L.check(L.lib().sn_masked_affine_f32(L.ptr(x), C, R, C, None, 0, ops.EPI_RELU_PRE | ops.EPI_AFFINE, L.ptr(sc), L.ptr(sh), None, 0,
                                                 L.ptr(y), C, L.stream()), "sn_masked_affine_f32")

        def fwd(code):
            return lambda: L.check(L.lib().sn_act_affine_f32(L.ptr(x), C, R, C, None, 0, code, L.ptr(sc), L.ptr(sh), L.ptr(y), C, L.stream()),
                                   "sn_act_affine_f32")

        def bwd(code):
            return lambda: L.check(L.lib().sn_act_affine_bwd_f32(L.ptr(dy), C, L.ptr(a), C, R, C, None, 0, code, L.ptr(y), C, L.stream()),
                                   "sn_act_affine_bwd_f32")

        cands = {"sn_masked_affine_f32_relu_pre_affine": relu_affine, "sn_act_affine_f32_tanh": fwd(ops.ACT_TANH),
                 "sn_act_affine_f32_elu": fwd(ops.ACT_ELU), "sn_act_affine_bwd_f32_tanh": bwd(ops.ACT_TANH),
                 "sn_act_affine_bwd_f32_elu": bwd(ops.ACT_ELU)}
        us = _timed(cands, base.PASSES, REPS)
        r = dict(rows=R, cols=C, path=path, launches=REPS, bytes_forward=2 * R * C * 4, bytes_adjoint=3 * R * C * 4, us_per_launch=us)
        r["GBps"] = {k: (r["bytes_adjoint"] if "bwd" in k else r["bytes_forward"]) / v["median"] / 1e3 for k, v in us.items()}
        out.append(r)
        print(f"[{R}, {C}] ({path}): " + ", ".join(f"{k} {v['median']:.2f} us [{v['min']:.2f}, {v['max']:.2f}]" for k, v in us.items()), flush=True)
    return out


def _encoder(module, act, fused=True):
    import importlib
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import dgl_configs
    mod = importlib.import_module("signnet_basisnet_amd." + module)
    _, cfg = dgl_configs.net_params(CONFIG, base.DEV)
    torch.manual_seed(0)
    enc = mod.get_sign_inv_net(dict(cfg, sign_inv_activation=act)).to(base.DEV).eval()
    enc.fused_stages = fused
    return enc


def encoder_times(variants):
    """variants: {label: (module, activation, fused_stages)}."""
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import dgl_configs, ops
    b = base._batches(dgl_configs.SHIPPED[CONFIG]["pos_enc_dim"])[0]
    x = b["p"].unsqueeze(-1).contiguous()
    encs = {k: _encoder(*v) for k, v in variants.items()}
    launches = {}
    cands = {}
    for k, enc in encs.items():
        def run(enc=enc):
            with torch.no_grad():
                return enc(b["g"], x)
        run()
        rec = ops.KernelTimer()
        with rec:
            run()
        names = [s[0] for s in rec.spans]
        launches[k] = dict(recorded=len(names), by_entry_point={n: names.count(n) for n in sorted(set(names))})
        cands[k] = run
    ms = _timed(cands, base.PASSES, 50, unit=1.0)
    enc = next(iter(encs.values()))
    r = dict(config=CONFIG, k=enc.k, sign_inv_layers=len(enc.enc.layers), nodes=int(x.shape[0]), graphs=base.GRAPHS, launches=launches,
             ms_per_forward=ms)
    for k, v in ms.items():
        print(f"encoder {k}: {v['median']:.3f} ms [{v['min']:.3f}, {v['max']:.3f}]  {launches[k]['recorded']} recorded launches", flush=True)
    return r


def _step(nets, act):
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import dgl_configs, optim
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    cls, cfg = dgl_configs.net_params(CONFIG, base.DEV)
    torch.manual_seed(0)
    net = getattr(nets, cls)(dict(cfg, sign_inv_activation=act)).to(base.DEV).train()
    o = optim.FlatAdam(net.parameters(), lr=1e-4)
    return net, o, DGLBucketedStep(net, o, max_graphs=base.GRAPHS, granule=base.GRANULE, max_captures=4)


def train_times(acts, module):
    import importlib
    import torch
    import dgl_bucketed_train as base
    from signnet_basisnet_amd import dgl_configs
    nets = importlib.import_module("signnet_basisnet_amd." + module)
    batches = base._batches(dgl_configs.SHIPPED[CONFIG]["pos_enc_dim"])
    keep = {a: _step(nets, a) for a in acts}
    loops = {f"bucketed_{a}": (lambda b, s=keep[a][2]: s.step(b["g"], b["h"], b["p"], b["e"], None, b["t"])) for a in acts}
    first = {k: base._pass(fn, batches) for k, fn in loops.items()}          # captures, lazy setup
    ms = {k: [] for k in loops}
    for _ in range(base.PASSES):
        for k, fn in loops.items():
            ms[k].append(base._pass(fn, batches))
    enc = keep[acts[0]][0].sign_inv_net
    r = dict(config=CONFIG, k=enc.k, sign_inv_layers=len(enc.enc.layers), classes=module, batches=len(batches), graphs=base.GRAPHS,
             first_pass_ms_per_step=first, ms_per_step={k: _summary(v) for k, v in ms.items()}, captures=[])
    for net, o, step in keep.values():
        step.check()
        r["captures"].append(step.captures)
        step.release()
    del keep, loops
    torch.cuda.empty_cache()
    for k, v in r["ms_per_step"].items():
        print(f"{CONFIG} {k}: {v['median']:.2f} ms/step [{v['min']:.2f}, {v['max']:.2f}]", flush=True)
    return r


def merge(out, commit, launch, encoder, train, relu_files):
    res = dict(commit=commit, device=json.load(open(launch))["device"], launch=json.load(open(launch))["launch"],
               encoder=json.load(open(encoder))["encoder"], train=json.load(open(train))["train"])
    runs = [json.load(open(f)) for f in relu_files]
    ab = dict(note="activation relu, classes of dgl_deepsigns / dgl_nets: encoder eval forward (fused three-launch path, ms) and bucketed "
                   "ms/step, median of five passes, of the parent commit's tree and of this tree, separate processes alternating on one "
                   "device in one session", runs=[])
    for r in runs:
        ab["runs"].append(dict(tree=r["tree"], encoder=r["encoder"]["ms_per_forward"]["relu_fused"], train=r["train"]["ms_per_step"]["bucketed_relu"]))
    verdict = {}
    for what in ("encoder", "train"):
        par = [p for r in ab["runs"] if r["tree"] == "parent" for p in r[what]["passes"]]
        med = [r[what]["median"] for r in ab["runs"] if r["tree"] == "this"]
        if par and med:
            verdict[what] = dict(parent_pass_range_ms=[min(par), max(par)], this_medians_ms=med,
                                 inside=bool(all(min(par) <= m <= max(par) for m in med)))
    ab["verdict"] = verdict
    res["parent_ab_same_box"] = ab
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(verdict))


def main():
    mode, out = sys.argv[1], sys.argv[2]
    if mode == "merge":
        return merge(out, sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6], sys.argv[7:])
    import bench
    import dgl_bucketed_train as base
    res = dict(device=bench.device_block(base.DEV))
    if mode == "launch":
        res["launch"] = launch_times()
    elif mode == "encoder":
        res["encoder"] = encoder_times({"relu_fused": ("activation_signinv", "relu", True), "relu_layer_path": ("activation_signinv", "relu", False),
                                        "tanh_layer_path": ("activation_signinv", "tanh", True)})
    elif mode == "train":
        res["train"] = train_times(("relu", "tanh"), "activation_signinv")
    elif mode == "relu":
        res["tree"] = "this" if os.path.samefile(ROOT, os.path.dirname(os.path.dirname(HERE))) else "parent"
        res["encoder"] = encoder_times({"relu_fused": ("dgl_deepsigns", "relu", True)})
        res["train"] = train_times(("relu",), "dgl_nets")
    else:
        raise SystemExit(__doc__)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
