"""What full-graph attention from the bond graph costs and buys (TransformerNet.full_graph_input = "bonds").

One process, contenders alternating pass by pass, median and range of five passes.

 (a) kernel alone, the headline ZINC-like batch (synth.make_batch, 128 graphs; 8 heads, dk = 8, C = 4): sn_bond_full_attention_f32 /
     _bwd_f32 on the bond graph against sn_full_attention_f32 / _bwd_f32 on ops.make_full_graph of the same batch; device events over
     back-to-back launches into preallocated outputs.
 (b) the shipped NoPE Transformer shape (dgl_configs 'transformer_nope') with full_graph=True over 16 shuffled batches, whole passes
     timed on the host: the eager edge-form step, the eager bond-form step and the bond-form DGLBucketedStep (ms/step); the eval
     forward in both forms; and on ONE batch shape serving.GraphedDGLForward against the eager bond-form eval forward.
 (c) with --parent TREE: the full_graph=False eval forward and the "edges" full-graph eval forward of this tree and of the parent
     commit's tree (its package, built), in alternating child processes; whether this tree's median lies inside the parent's own
     pass-to-pass range.

    python profiles/scripts/bond_full_attention.py [--parent TREE] [out.json]        (default: profiles/bond_full_attention.json)
"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TREE = None
if "--tree" in sys.argv:                      # (child of (c): import the package of another tree)
    TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
if TREE:
    sys.path.insert(0, TREE)

import torch  # noqa: E402

import signnet_basisnet_amd  # noqa: E402,F401  (first: the helper module below puts ROOT in front of the path again)
import dgl_bucketed_train as base  # noqa: E402
from signnet_basisnet_amd import dgl_configs, dgl_nets, ops, optim, synth  # noqa: E402
from signnet_basisnet_amd._lib import check, lib, ptr, stream  # noqa: E402
from signnet_basisnet_amd.dgl_deepsigns import Graph  # noqa: E402

DEV = base.DEV
REPS = 50
PASSES = base.PASSES
CONFIG = "transformer_nope"
H, DK, NC = 8, 8, 4


def _summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), passes=v)


def _alternate(cands, reps=REPS):
    """us per launch of every candidate: PASSES passes, the candidates alternating pass by pass."""
    for fn in cands.values():
        for _ in range(5):
            fn()
    us = {k: [] for k in cands}
    for _ in range(PASSES):
        for k, fn in cands.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {k: _summary(v) for k, v in us.items()}


def kernel_times():
    d = synth.make_batch(base.GRAPHS, seed=1)
    src, dst = d.edge_index
    sizes = torch.tensor(d.sizes)
    g = Graph(src.to(DEV), dst.to(DEV), sizes)
    e = d.edge_attr.reshape(-1).long().to(DEV)
    full, ef = ops.make_full_graph(g, e)
    N, D, B = d.batch.numel(), H * DK, len(d.sizes)
    batch = torch.repeat_interleave(torch.arange(B), sizes).to(DEV)
    fs, fd = full.edges()
    E_full = fs.numel()
    ei = torch.stack([fs, fd])
    fplan, frplan = ops.build_plan(batch, ei, B, 0), ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)
    bplan = ops.build_plan(batch, torch.stack([src, dst]).to(DEV), B, 0)
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    Q, K, V, Q2, K2, dout = (rnd(N, D) for _ in range(6))
    Tr, Tf = rnd(NC, D), rnd(NC, D)
    gamma = torch.tensor([0.5], device=DEV)
    codes = ops.full_graph_codes(ef, full.edata["real"])
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)
    out, den, bout, bden = new(N, D), new(N, H), new(N, D), new(N, H)
    status = torch.zeros(2, dtype=torch.int32, device=DEV)
    L = lib()
    st = stream()

    def full_fwd():
        check(L.sn_full_attention_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), D, ptr(Tr), ptr(Tf), NC, ptr(codes), ptr(gamma), N, H, DK,
                                      ptr(fplan.rowptr), ptr(fplan.col), ptr(fplan.eperm), ptr(out), ptr(den), ptr(status), st), "fwd")

    def bond_fwd():
        check(L.sn_bond_full_attention_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), D, ptr(Tr), ptr(Tf), NC, ptr(e), ptr(gamma), N, B, bplan.E, H,
                                           DK, ptr(bplan.graph_ptr), ptr(bplan.rowptr), ptr(bplan.col), ptr(bplan.eperm), None, None, ptr(bout),
                                           ptr(bden), ptr(status), st), "bond fwd")

    gq = [new(N, D) for _ in range(5)] + [new(NC, D), new(NC, D), new(1)]
    bq = [new(N, D) for _ in range(5)] + [new(NC, D), new(NC, D), new(1)]
    scratch = new(int(L.sn_full_attention_bwd_scratch_floats(N, E_full, H, DK, NC)))
    bscratch = new(int(L.sn_bond_full_attention_bwd_scratch_floats(N, B, H, DK, NC)))

    def full_bwd():
        check(L.sn_full_attention_bwd_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), D, ptr(Tr), ptr(Tf), NC, ptr(codes), ptr(gamma), ptr(out),
                                          ptr(den), ptr(dout), N, E_full, H, DK, ptr(fplan.rowptr), ptr(fplan.col), ptr(fplan.eperm),
                                          ptr(frplan.rowptr), ptr(frplan.col), ptr(frplan.eperm), *(ptr(t) for t in gq), ptr(scratch), st), "bwd")

    def bond_bwd():
        check(L.sn_bond_full_attention_bwd_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), D, ptr(Tr), ptr(Tf), NC, ptr(e), ptr(gamma), ptr(bout),
                                               ptr(bden), ptr(dout), N, B, bplan.E, H, DK, ptr(bplan.graph_ptr), ptr(bplan.rowptr),
                                               ptr(bplan.col), ptr(bplan.eperm), None, None, *(ptr(t) for t in bq), ptr(bscratch), st), "bond bwd")

    full_fwd()
    bond_fwd()
    t = _alternate({"sn_full_attention_f32": full_fwd, "sn_bond_full_attention_f32": bond_fwd, "sn_full_attention_bwd_f32": full_bwd,
                    "sn_bond_full_attention_bwd_f32": bond_bwd})
    assert status.tolist() == [0, 0]
    agree = float((bout - out).abs().max() / out.abs().max())
    return dict(graphs=B, nodes=N, bonds=int(src.numel()), full_edges=E_full, heads=H, dk=DK, classes=NC, launches=REPS,
                largest_graph=int(max(d.sizes)), staged_nodes=dict(forward=ops.bond_attention_staged_nodes(DK), adjoint=ops.bond_attention_staged_nodes(DK, True)),
                scratch_floats=dict(edge_list=int(scratch.numel()), bonds=int(bscratch.numel())),
                per_pair_index_bytes=dict(edge_list=int(20 * E_full), bonds=0),      # (int32 codes; col and eperm of two plans)
                max_rel_difference_of_the_outputs=agree, us_per_launch=t)


def _net(full, form="edges"):
    cls, cfg = dgl_configs.net_params(CONFIG, DEV)
    torch.manual_seed(0)
    net = getattr(dgl_nets, cls)(dict(cfg, full_graph=full)).to(DEV)
    if form != "edges":
        net.full_graph_input = form
    return net, optim.FlatAdam(net.parameters(), lr=1e-4)


def _eval_fn(net, gkey, ekey):
    net.eval()

    def fwd(b):
        with torch.no_grad():
            net(b[gkey], b["h"], None, b[ekey], None)
    return fwd


def _step_fn(net, o, gkey, ekey):
    net.train()

    def step(b):          # train_ZINC_graph_regression.py:66-81 (the per-step loss.item() of :82 left out)
        o.zero_grad()
        y, _ = net(b[gkey], b["h"], None, b[ekey], None)
        net.loss(y, b["t"]).backward()
        o.step()
    return step


def step_times():
    from signnet_basisnet_amd import serving
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    batches = base._batches(16)
    for b in batches:
        b["e"] = b["e"].reshape(-1).long()
        b["gf"], b["ef"] = ops.make_full_graph(b["g"], b["e"])
    nets = dict(edges_eval=_net(True), bonds_eval=_net(True, "bonds"), edges_step=_net(True), bonds_step=_net(True, "bonds"),
                bonds_bucketed=_net(True, "bonds"), bonds_graphed=_net(True, "bonds"))
    cap = DGLBucketedStep(nets["bonds_bucketed"][0].train(), nets["bonds_bucketed"][1], max_graphs=base.GRAPHS, granule=base.GRANULE, max_captures=4)
    one = batches[0]
    served = nets["bonds_graphed"][0].eval()
    graphed = serving.GraphedDGLForward(served, one["g"], one["h"], None, one["e"])
    fixed = _eval_fn(nets["bonds_eval"][0], "g", "e")
    loops = {
        "eager_step_edges": _step_fn(*nets["edges_step"], "gf", "ef"),
        "eager_step_bonds": _step_fn(*nets["bonds_step"], "g", "e"),
        "bucketed_step_bonds": lambda b: cap.step(b["g"], b["h"], None, b["e"], None, b["t"]),
        "eval_forward_edges": _eval_fn(nets["edges_eval"][0], "gf", "ef"),
        "eval_forward_bonds": fixed,
        "eval_forward_bonds_one_shape": lambda b: fixed(one),
        "graphed_forward_bonds_one_shape": lambda b: graphed(one["g"], one["h"], None, one["e"]),
    }
    first = {k: base._pass(fn, batches) for k, fn in loops.items()}
    ms = {k: [] for k in loops}
    for _ in range(PASSES):
        for k, fn in loops.items():
            ms[k].append(base._pass(fn, batches))
    cap.check()
    graphed.check()
    with torch.no_grad():
        same = bool(torch.equal(graphed(one["g"], one["h"], None, one["e"]), served(one["g"], one["h"], None, one["e"])[0]))
    net0 = nets["bonds_eval"][0]
    res = dict(config=CONFIG, hidden=net0.embedding_h.weight.shape[1], layers=len(net0.layers), batches=len(batches), graphs=base.GRAPHS,
               first_pass_ms=first, ms={k: _summary(v) for k, v in ms.items()}, captures=cap.captures, hits=cap.hits,
               buckets=[dict(N=bk.N, E=bk.E) for bk in cap.buckets], graphed_replay_equals_eager_bits=same,
               edges=dict(bonds=[b["E"] for b in batches], full=[int(b["ef"].numel()) for b in batches]))
    cap.release()
    return res


def child():
    """(c): the two forwards that exist in the parent too — the sparse net and the edge form of the full-graph net."""
    batches = base._batches(16)
    for b in batches:
        b["e"] = b["e"].reshape(-1).long()
        b["gf"], b["ef"] = ops.make_full_graph(b["g"], b["e"])
    loops = {"eval_forward_sparse": _eval_fn(_net(False)[0], "g", "e"), "eval_forward_edges": _eval_fn(_net(True)[0], "gf", "ef")}
    for fn in loops.values():
        base._pass(fn, batches)
    ms = {k: [] for k in loops}
    for _ in range(PASSES):
        for k, fn in loops.items():
            ms[k].append(base._pass(fn, batches))
    print(json.dumps(dict(package=os.path.dirname(signnet_basisnet_amd.__file__), **{k: _summary(v) for k, v in ms.items()})))


def regression(parent, out):
    """(c): child processes alternating parent tree / this tree, three of the parent and two of this one."""
    runs = []
    for tree in (parent, ROOT, parent, ROOT, parent):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--child"], capture_output=True, text=True, timeout=300)
        if p.returncode != 0:
            raise RuntimeError(f"child for {tree} failed:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        if os.path.realpath(r["package"]) != os.path.realpath(os.path.join(tree, "signnet_basisnet_amd")):
            raise RuntimeError(f"the child for {tree} imported {r['package']}")
        r["package"] = os.path.relpath(r["package"], ROOT)
        runs.append(dict(tree=os.path.relpath(tree, ROOT), **r))
    chk = {}
    for k in ("eval_forward_sparse", "eval_forward_edges"):
        par = [v for r in runs if r["tree"] != "." for v in r[k]["passes"]]
        mine = statistics.median([v for r in runs if r["tree"] == "." for v in r[k]["passes"]])
        chk[k] = dict(parent_range_ms=[min(par), max(par)], this_tree_median_ms=mine, inside=bool(min(par) <= mine <= max(par)),
                      not_slower=bool(mine <= max(par)))
    out["parent_ab_same_box"] = dict(note="alternating child processes", runs=runs)
    out["regression_check"] = chk


def main():
    args = [a for a in sys.argv[1:]]
    if "--child" in args:
        child()
        return
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "bond_full_attention.json")
    import bench
    res = dict(device=bench.device_block(DEV))
    res["kernel"] = kernel_times()
    res["net"] = step_times()
    if parent:
        regression(parent, res)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for k, v in res["kernel"]["us_per_launch"].items():
        print(f"{k}: {v['median']:.2f} us [{v['min']:.2f}, {v['max']:.2f}]")
    for k, v in res["net"]["ms"].items():
        print(f"{k}: {v['median']:.3f} ms [{v['min']:.3f}, {v['max']:.3f}]")
    if parent:
        print("regression check", json.dumps(res["regression_check"]))


if __name__ == "__main__":
    main()
