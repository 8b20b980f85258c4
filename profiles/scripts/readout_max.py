"""What readout='max' costs next to 'mean' (DESIGN.md §4.6a), and whether 'sum' / 'mean' moved.

  kernels     sn_segment_max_f32 (with arg) against sn_segment_pool_f32 (mean), and sn_segment_max_bwd_f32 against
              sn_segment_broadcast_f32, at [N of 128 ZINC-like graphs, C in {64, 77, 95}]: device events over 200 back-to-back launches,
              the variants alternating pass by pass, median and range of five passes
  gatedgcn    GatedGCN NoPE (configs/gatedgcn/GatedGCN_ZINC_NoPE.json: hidden 77, 16 layers): the one-launch eval forward and
              train_graph.DGLBucketedStep, readout 'mean' against 'max', over the 16 shuffled batches of
              profiles/scripts/dgl_bucketed_train.py, alternating pass by pass, five passes

    python profiles/scripts/readout_max.py [out.json]        (default: profiles/readout_max.json)

  regression  `--regression [--root TREE] out.json`: 'sum' / 'mean' eval and the bucketed step of GatedGCN NoPE and the GIN net with the
              classes of dgl_nets alone, so the same file runs against another checkout (`--root`: the tree whose package and bench.py
              are imported).  Run it in alternating processes on this tree and on the parent commit, three rounds; `--compare a.json
              b.json ...` prints, per workload, each tree's medians and the parent's own pass-to-pass range.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ARGV = sys.argv[1:]
if "--root" in ARGV:
    i = ARGV.index("--root")
    ROOT = os.path.abspath(ARGV[i + 1])
    del ARGV[i:i + 2]
if "--compare" not in ARGV:
    sys.path.insert(0, ROOT)
    sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

    import torch  # noqa: E402

    import bench  # noqa: E402
    from signnet_basisnet_amd import dgl_configs, dgl_nets, optim, synth  # noqa: E402
    from signnet_basisnet_amd._lib import check, lib, ptr, stream  # noqa: E402
    from signnet_basisnet_amd.dgl_deepsigns import Graph  # noqa: E402
    from signnet_basisnet_amd.train_graph import DGLBucketedStep  # noqa: E402

DEV = "cuda:0"
SEEDS = range(1, 17)
GRAPHS = 128
PASSES = 5
REPS = 200
GRANULE = dict(N=256, E=512)


def _batches(k):
    """The 16 shuffled batches of profiles/scripts/dgl_bucketed_train.py."""
    out = []
    g = torch.Generator().manual_seed(0)
    for s in SEEDS:
        d = synth.make_batch(GRAPHS, seed=s)
        src, dst = d.edge_index
        out.append(dict(g=Graph(src.to(DEV), dst.to(DEV), torch.tensor(d.sizes).to(DEV)), h=d.x.squeeze(-1).to(DEV),
                        p=synth.dgl_pos_enc(d, k).to(DEV), e=d.edge_attr.to(DEV), t=torch.randn(GRAPHS, 1, generator=g).to(DEV),
                        N=d.batch.numel(), E=d.edge_index.shape[1], sizes=list(d.sizes)))
    return out


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _alternate(variants, reps):
    """{name: fn} -> {name: {median, passes}} in the unit of _events_ms (ms per call): one warm-up pass each, then PASSES passes, the
    variants alternating pass by pass (a drift of the clock or of the host load hits all of them)."""
    for fn in variants.values():
        _events_ms(fn, max(reps // 10, 1))
    passes = {n: [] for n in variants}
    for _ in range(PASSES):
        for n, fn in variants.items():
            passes[n].append(_events_ms(fn, reps))
    return {n: dict(median=statistics.median(v), min=min(v), max=max(v), passes=v) for n, v in passes.items()}


def kernels():
    d = synth.make_batch(GRAPHS, seed=1)
    N, B = int(d.batch.numel()), GRAPHS
    gp = torch.tensor([0] + list(d.sizes), dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)
    rows = []
    for C in (64, 77, 95):
        x = torch.randn(N, C, device=DEV)
        dy = torch.randn(B, C, device=DEV)
        out, dx = torch.empty(B, C, device=DEV), torch.empty(N, C, device=DEV)
        arg = torch.empty(B, C, dtype=torch.int32, device=DEV)
        L, st = lib(), stream()
        fwd = _alternate({
            "segment_pool_mean": lambda: check(L.sn_segment_pool_f32(ptr(x), B, C, ptr(gp), 1, ptr(out), st), "pool"),
            "segment_max_arg": lambda: check(L.sn_segment_max_f32(ptr(x), B, C, ptr(gp), ptr(out), ptr(arg), st), "max"),
        }, REPS)
        bwd = _alternate({
            "segment_broadcast_mean": lambda: check(L.sn_segment_broadcast_f32(ptr(dy), B, C, ptr(gp), 1, ptr(dx), st), "bcast"),
            "segment_max_bwd": lambda: check(L.sn_segment_max_bwd_f32(ptr(dy), ptr(arg), B, C, ptr(gp), ptr(dx), st), "max_bwd"),
        }, REPS)
        # what each launch moves (bytes the algorithm needs): forward reads x and writes out (+ arg); the adjoint reads dy (+ arg), writes dx
        rows.append(dict(N=N, B=B, C=C, launches_per_pass=REPS, unit="us per launch, back to back (launch-bound: includes the host's issue rate)",
                         bytes=dict(segment_pool_mean=4 * (N * C + B * C), segment_max_arg=4 * (N * C + 2 * B * C),
                                    segment_broadcast_mean=4 * (N * C + B * C), segment_max_bwd=4 * (N * C + 2 * B * C)),
                         **{n: {k: ([t * 1e3 for t in v] if k == "passes" else v * 1e3) for k, v in r.items()} for n, r in {**fwd, **bwd}.items()}))
    return rows


def _net(module, name, readout, train):
    cls, p = dgl_configs.net_params(name, DEV)
    p = dict(p, readout=readout)
    torch.manual_seed(0)
    net = getattr(module, cls)(p).to(DEV)
    return net.train(train)


def _eval_pass(net, batches):
    def run():
        with torch.no_grad():
            for b in batches:
                net(b["g"], b["h"], None, b["e"], None)
    return run


def _workloads(module, name, readouts):
    """{label: fn over one pass of the 16 batches} for the eval forward and the bucketed step of `name` at every readout, + cleanup."""
    batches = _batches(8)
    fns, steps = {}, []
    for r in readouts:
        net = _net(module, name, r, False)
        fns[f"{name}/eval/{r}"] = _eval_pass(net, batches)
        tnet = _net(module, name, r, True)
        step = DGLBucketedStep(tnet, optim.FlatAdam(tnet.parameters(), lr=1e-4), max_graphs=GRAPHS, granule=GRANULE, max_captures=4)
        steps.append(step)

        def bucketed(step=step):
            for b in batches:
                step.step(b["g"], b["h"], None, b["e"], None, b["t"])
        fns[f"{name}/bucketed_step/{r}"] = bucketed
    return fns, steps, len(batches)


def _measure(module, name, readouts):
    fns, steps, n = _workloads(module, name, readouts)
    res = _alternate(fns, 1)
    for s in steps:
        s.check()
        s.release()
    torch.cuda.empty_cache()
    return {k: dict(unit="ms per batch (eval) / ms per step", median=v["median"] / n, min=v["min"] / n, max=v["max"] / n,
                    passes=[t / n for t in v["passes"]]) for k, v in res.items()}


def compare(paths):
    runs = [json.load(open(p)) for p in paths]
    trees = sorted({r["tree"] for r in runs})
    keys = sorted(runs[0]["workloads"])
    for k in keys:
        line = [k]
        for t in trees:
            passes = [v for r in runs if r["tree"] == t for v in r["workloads"][k]["passes"]]
            meds = [r["workloads"][k]["median"] for r in runs if r["tree"] == t]
            line.append(f"{t}: medians {[round(m, 4) for m in meds]} passes [{min(passes):.4f}, {max(passes):.4f}]")
        print("  ".join(line))


def main():
    if "--compare" in ARGV:
        return compare([a for a in ARGV if a != "--compare"])
    if "--regression" in ARGV:
        out = [a for a in ARGV if a != "--regression"][0]
        res = dict(tree=os.path.basename(ROOT), device=bench.device_block(DEV), workloads={})
        for name in ("gatedgcn_nope", "gin_nope"):
            res["workloads"].update(_measure(dgl_nets, name, ("mean", "sum")))
    else:
        from signnet_basisnet_amd import readout_models
        out = ARGV[0] if ARGV else os.path.join(ROOT, "profiles", "readout_max.json")
        res = dict(device=bench.device_block(DEV), kernels=kernels(), gatedgcn_nope=_measure(readout_models, "gatedgcn_nope", ("mean", "max")))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for row in res.get("kernels", []):
        print(f"C={row['C']} N={row['N']}: " + ", ".join(f"{n} {row[n]['median']:.2f} us [{row[n]['min']:.2f}, {row[n]['max']:.2f}]"
                                                          for n in ("segment_pool_mean", "segment_max_arg", "segment_broadcast_mean", "segment_max_bwd")))
    for k, v in {**res.get("gatedgcn_nope", {}), **res.get("workloads", {})}.items():
        print(f"{k}: {v['median']:.4f} ms [{v['min']:.4f}, {v['max']:.4f}]")


if __name__ == "__main__":
    main()
