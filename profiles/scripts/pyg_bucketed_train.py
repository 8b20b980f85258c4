"""The baselines of the two PyG trees on SHUFFLED batch shapes: the eager step vs train_graph.BucketedStep (one capture per capacity
bucket) — the protocol of profiles/scripts/dgl_bucketed_train.py.

16 batches of 128 ZINC-like molecules (synth.make_batch, seeds 1-16: every batch has its own N and E) for pyg_gnn_types.GNN at hidden 128
and 4 layers with each of the five gnn_type values, and 16 Alchemy-like batches ([128, 12] targets) for pyg_baselines.NetGINE(64).  For
each: eager ms/step over the sequence and bucketed ms/step (after the first pass, which captures), PASSES passes each, alternating in
one process; captures, hits, padding fraction.  The two launches the captured step added — ops.csr_drop_loops and the masked
SimplifiedPNAConv statistics / adjoint — alone, by device events, on the largest bucket of the sequence.

Regression check of pyg.SignNetGNN's own bucketed step (k = 16, the workload of profiles/scripts/bucketed_train.py): with
`--parent DIR` (a checkout of the parent commit with its library built) this tree and DIR are measured in ALTERNATING child processes,
ROUNDS each, before this process opens the device; this tree's median must lie inside the parent's own pass-to-pass range.

    python profiles/scripts/pyg_bucketed_train.py [--parent DIR] [out.json]        (default: profiles/pyg_bucketed_train.json)
    python profiles/scripts/pyg_bucketed_train.py --signnet-child TREE             (one child: prints a JSON line)
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"
SEEDS = range(1, 17)
GRAPHS = 128
PASSES = 5
ROUNDS = 3
GRANULE = dict(N=256, E=512)
HIDDEN, LAYERS = 128, 4
NOT_MEASURED = [
    "pooling='mean' (the rows are pooling='add', core/config.py's default)",
    "dropout_models.GNN with dropout > 0",
    "step_from on a data.GraphStore (the gather launch in place of the pack launch)",
    "other widths / depths than hidden 128, 4 layers and NetGINE(64)",
    "memory reserved per capture",
]


def _pass(fn, batches):
    """ms per step over one whole pass of the sequence."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for b in batches:
        fn(*b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


# ----------------------------------------------------------------------------- one child of the regression check
def signnet_child(tree):
    sys.path.insert(0, os.path.abspath(tree))
    sys.path.insert(1, ROOT)                # bench.py (the workload and the model builder) is this tree's in both
    import torch
    import signnet_basisnet_amd             # (before bench, which puts its own directory in front of sys.path)
    if os.path.dirname(os.path.dirname(os.path.abspath(signnet_basisnet_amd.__file__))) != os.path.abspath(tree):
        raise RuntimeError(f"the package was imported from {signnet_basisnet_amd.__file__}, not from {tree}")
    import bench
    from signnet_basisnet_amd import optim, synth
    from signnet_basisnet_amd.train_graph import BucketedStep
    W = bench.WORKLOAD
    hosts = [synth.make_batch(W["B"], seed=s, n_lo=W["n_lo"], n_hi=W["n_hi"], features=W["features"]) for s in SEEDS]
    g = torch.Generator().manual_seed(0)
    batches = [(synth.batch_to(h, DEV), torch.randn(h.num_graphs, W["n_out"], generator=g).to(DEV)) for h in hosts]
    m = bench.build_model(DEV, k=W["k"]).train()
    o = optim.FlatAdam(m.parameters(), lr=1e-4)
    step = BucketedStep(m, o, max_graphs=W["B"], granule=dict(N=256, E=512, S=16384, K=8), max_captures=4)
    _pass(step.step, batches)               # captures
    passes = [_pass(step.step, batches) for _ in range(PASSES)]
    step.check()
    print("CHILD " + json.dumps(dict(passes_ms=passes, median_ms=statistics.median(passes), captures=step.captures)))


def signnet_regression(parent):
    out = dict(workload="pyg.SignNetGNN k = 16 through BucketedStep (profiles/scripts/bucketed_train.py), 16 shuffled batches",
               rounds=ROUNDS, passes_per_round=PASSES, parent=[], tree=[])
    for _ in range(ROUNDS):
        for name, tree in (("parent", parent), ("tree", ROOT)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--signnet-child", tree], capture_output=True, text=True,
                               timeout=300)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                raise RuntimeError(f"signnet child ({name}) failed: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            out[name].append(json.loads(line[0][6:]))
    pp = [v for c in out["parent"] for v in c["passes_ms"]]
    tp = [v for c in out["tree"] for v in c["passes_ms"]]
    out["parent_median_ms"], out["parent_range_ms"] = statistics.median(pp), [min(pp), max(pp)]
    out["tree_median_ms"], out["tree_range_ms"] = statistics.median(tp), [min(tp), max(tp)]
    out["tree_median_inside_parent_range"] = min(pp) <= out["tree_median_ms"] <= max(pp)
    return out


# ----------------------------------------------------------------------------- eager vs bucketed
def _batches(features, n_out):
    import torch
    from signnet_basisnet_amd import synth
    g = torch.Generator().manual_seed(0)
    out, sizes = [], []
    for s in SEEDS:
        h = synth.make_batch(GRAPHS, seed=s, features=features)
        sizes.append((h.batch.numel(), h.edge_index.shape[1]))
        del h.eigen_values, h.eigen_vectors            # these models read no eigen data: the loader delivers none
        out.append((synth.batch_to(h, DEV), torch.randn(GRAPHS, n_out, generator=g).to(DEV)))
    return out, sizes


def _build(kind):
    import torch
    from signnet_basisnet_amd import optim, pyg_baselines, pyg_gnn_types
    torch.manual_seed(0)
    m = pyg_baselines.NetGINE(64) if kind == "NetGINE(64)" else pyg_gnn_types.GNN(None, None, HIDDEN, 1, LAYERS, kind)
    m = m.to(DEV).train()
    return m, optim.FlatAdam(m.parameters(), lr=1e-4)


def run(kind, batches, sizes):
    import torch
    from signnet_basisnet_amd.train_graph import BucketedStep
    res = dict(model=kind, batches=len(batches), graphs=GRAPHS, nodes=[n for n, _ in sizes], edges=[e for _, e in sizes])
    m2, o2 = _build(kind)
    step = BucketedStep(m2, o2, max_graphs=GRAPHS, granule=GRANULE, max_captures=4)
    res["first_pass_ms_per_step"] = _pass(step.step, batches)          # captures every bucket
    m, o = _build(kind)

    def eager(d, t):          # core/train.py:55-66 / main_alchemy.py:99-110 (the per-step loss.item() left out)
        o.zero_grad()
        (m(d) - t).abs().mean().backward()
        o.step()

    _pass(eager, batches)                     # warm-up pass (lazy setup, allocator)
    # the two loops alternate pass by pass on the same box: a drift of the clock or of the host load hits both
    eager_ms, bucketed_ms = [], []
    for _ in range(PASSES):
        eager_ms.append(_pass(eager, batches))
        bucketed_ms.append(_pass(step.step, batches))
    step.check()
    res["eager_ms_per_step"], res["eager_passes_ms"] = statistics.median(eager_ms), eager_ms
    res["bucketed_ms_per_step"], res["bucketed_passes_ms"] = statistics.median(bucketed_ms), bucketed_ms
    res["speedup"] = res["eager_ms_per_step"] / res["bucketed_ms_per_step"]
    res["captures"], res["hits"] = step.captures, step.hits
    res["buckets"] = [dict(N=b.N, E=b.E) for b in step.buckets]
    rows = dict(nodes=[0, 0], edges=[0, 0])
    for (d, _), (n, e) in zip(batches, sizes):
        b = step.bucket_of(d)
        for key, v, cap in (("nodes", n, b.N), ("edges", e, b.E)):
            rows[key][0] += cap - v
            rows[key][1] += cap
    res["padding_fraction"] = {key: v[0] / v[1] for key, v in rows.items()}
    step.release()
    del step, m, o, m2, o2
    torch.cuda.empty_cache()
    return res


# ----------------------------------------------------------------------------- the two new launches alone
def _events(fn, reps=50):
    import torch
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(5):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return dict(median_us=statistics.median(out), range_us=[min(out), max(out)], launches_per_sample=reps)


def new_launches(batches, sizes):
    import torch
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import Bucket, PaddedBatch
    i = max(range(len(sizes)), key=lambda j: sizes[j][0])
    d, t = batches[i]
    N, E = sizes[i]
    bucket = Bucket(-(-(N + 1) // GRANULE["N"]) * GRANULE["N"], -(-E // GRANULE["E"]) * GRANULE["E"], 1, 1)
    pad = PaddedBatch(bucket, GRAPHS + 1, d, t, DEV)
    ops.bucket_pack(d, t, pad)
    plan = ops.build_plan(pad.batch, pad.edge_index, pad.B_cap, 0)
    rplan = ops.build_plan(pad.batch, pad.edge_index.flip(0).contiguous(), pad.B_cap, 0)
    Cc = 3 * HIDDEN
    a, b, dr = (torch.randn(bucket.N, Cc, device=DEV) for _ in range(3))
    q = torch.randn(bucket.E, Cc, device=DEV)
    bn = torch.nn.BatchNorm1d(Cc).to(DEV).train()
    state, _ = ops.spna_stats(a, b, q, plan, bn, pad.node_valid, pad.counts)
    gamma = bn.weight.detach()
    return dict(
        batch=dict(N=N, E=E, N_cap=bucket.N, E_cap=bucket.E, C=Cc),
        csr_drop_loops_both_operators_three_launches=_events(lambda: ops.csr_drop_loops(plan, rplan)),
        spna_stats_masked=_events(lambda: ops.spna_stats(a, b, q, plan, bn, pad.node_valid, pad.counts)),
        spna_stats_unmasked_same_buffers=_events(lambda: ops.spna_stats(a, b, q, plan, bn)),
        spna_bwd_masked=_events(lambda: ops.spna_bwd(a, b, q, plan, rplan, dr, state=state, gamma=gamma, node_valid=pad.node_valid,
                                                     counts=pad.counts)),
        spna_bwd_unmasked_same_buffers=_events(lambda: ops.spna_bwd(a, b, q, plan, rplan, dr, state=state, gamma=gamma)),
        note="device events around 50 back-to-back calls (host allocation of the outputs included); the unmasked rows run the eager "
             "step's launches over the same capacity buffers, for scale",
    )


def main():
    args = sys.argv[1:]
    if args[:1] == ["--signnet-child"]:
        return signnet_child(args[1])
    parent = None
    if args[:1] == ["--parent"]:
        parent, args = args[1], args[2:]
    out = args[0] if args else os.path.join(ROOT, "profiles", "pyg_bucketed_train.json")
    res = dict(protocol="16 shuffled 128-graph batches, eager and bucketed passes alternating in one process, median and range over "
                        f"{PASSES} passes; pyg_gnn_types.GNN(None, None, {HIDDEN}, 1, {LAYERS}, gnn_type) and NetGINE(64)")
    not_measured = list(NOT_MEASURED)
    if parent is not None:                   # (children first: this process has not opened the device yet)
        res["signnet_regression"] = signnet_regression(parent)
    else:
        not_measured.append("the SignNetGNN regression check (no --parent checkout given)")
    sys.path.insert(0, ROOT)
    import bench
    from signnet_basisnet_amd import pyg_gnn_types
    res["device"] = bench.device_block(DEV)
    zinc, zs = _batches("zinc", 1)
    res["runs"] = [run(kind, zinc, zs) for kind in pyg_gnn_types.GNN_TYPES]
    res["new_launches"] = new_launches(zinc, zs)
    del zinc
    alch, as_ = _batches("alchemy", 12)
    res["runs"].append(run("NetGINE(64)", alch, as_))
    res["not_measured"] = not_measured
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["runs"]:
        print(f"{r['model']}: eager {r['eager_ms_per_step']:.2f} ms/step {[round(v, 2) for v in r['eager_passes_ms']]}, "
              f"bucketed {r['bucketed_ms_per_step']:.2f} ms/step {[round(v, 2) for v in r['bucketed_passes_ms']]}, "
              f"captures {r['captures']}, hits {r['hits']}")
    print(json.dumps(res["new_launches"]))
    if parent is not None:
        s = res["signnet_regression"]
        print(f"SignNetGNN k=16 bucketed: parent {s['parent_median_ms']:.3f} ms {s['parent_range_ms']}, tree {s['tree_median_ms']:.3f} ms "
              f"{s['tree_range_ms']}, inside the parent's range: {s['tree_median_inside_parent_range']}")


if __name__ == "__main__":
    main()
