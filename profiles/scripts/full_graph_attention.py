"""What full-graph attention costs (TransformerNet with full_graph=True).

One process on the headline ZINC-like batch (synth.make_batch, 128 graphs) made full with ops.make_full_graph; 8 heads, dk = 8, C = 4;
median and range of five alternating passes, device events over back-to-back launches into preallocated outputs.

 (a) sn_full_attention_f32 and sn_full_attention_bwd_f32; beside them, as context, the sparse kernel's formulation of the same thing:
     sn_edge_attention_f32 / _bwd_f32 over the same full edge list with a materialised [E_full, 64] edge projection, and the two
     [E_full, 64] x [64, 64] Linears that formulation needs per layer.
 (b) sn_make_full_graph per launch.
 (c) the shipped Transformer shape (dgl_configs 'transformer_nope') at full_graph False and True: eval forward and eager training step
     with FlatAdam, 16 shuffled batches, whole passes timed on the host.
 (d) with --parent TREE: the full_graph=False eval forward and eager step of this tree and of the parent commit's tree (its package,
     built), in alternating child processes; this tree's median must lie inside the parent's own pass-to-pass range.

    python profiles/scripts/full_graph_attention.py [--parent TREE] [out.json]        (default: profiles/full_graph_attention.json)
"""
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TREE = None
if "--tree" in sys.argv:                      # (child of (d): import the package of another tree)
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


def _alternate(cands, reps=REPS, unit=1e3):
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
            us[k].append(e0.elapsed_time(e1) * unit / reps)
    return {k: _summary(v) for k, v in us.items()}


def op_times():
    d = synth.make_batch(base.GRAPHS, seed=1)
    src, dst = d.edge_index
    g = Graph(src.to(DEV), dst.to(DEV), torch.tensor(d.sizes))
    e = d.edge_attr.reshape(-1).long().to(DEV)
    full, ef = ops.make_full_graph(g, e)
    N, D = d.batch.numel(), H * DK
    fs, fd = full.edges()
    E = fs.numel()
    batch = torch.repeat_interleave(torch.arange(len(d.sizes)), torch.tensor(d.sizes)).to(DEV)
    ei = torch.stack([fs, fd])
    plan, rplan = ops.build_plan(batch, ei, len(d.sizes), 0), ops.build_plan(batch, ei.flip(0).contiguous(), len(d.sizes), 0)
    gen = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    Q, K, V, Q2, K2, dout = (rnd(N, D) for _ in range(6))
    Tr, Tf = rnd(NC, D), rnd(NC, D)
    gamma = torch.tensor([0.5], device=DEV)
    codes = ops.full_graph_codes(ef, full.edata["real"])
    new = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)
    out, den = new(N, D), new(N, H)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    L = lib()
    st = stream()

    def full_fwd():
        check(L.sn_full_attention_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), D, ptr(Tr), ptr(Tf), NC, ptr(codes), ptr(gamma), N, H, DK,
                                      ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(out), ptr(den), ptr(status), st), "fwd")

    gq = [new(N, D) for _ in range(5)] + [new(NC, D), new(NC, D), new(1)]
    scratch = new(int(L.sn_full_attention_bwd_scratch_floats(N, E, H, DK, NC)))

    def full_bwd():
        check(L.sn_full_attention_bwd_f32(ptr(Q), ptr(K), ptr(V), ptr(Q2), ptr(K2), D, ptr(Tr), ptr(Tf), NC, ptr(codes), ptr(gamma), ptr(out),
                                          ptr(den), ptr(dout), N, E, H, DK, ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(rplan.rowptr),
                                          ptr(rplan.col), ptr(rplan.eperm), *(ptr(t) for t in gq), ptr(scratch), st), "bwd")

    # the sparse kernel's formulation over the same pairs: a materialised edge projection (one class table here: context, not parity)
    emb = rnd(NC, D)
    edge_emb = emb[ef].contiguous()                                  # [E_full, 64]: the edge embedding that formulation projects
    WE, WE2 = (ops.PackedLinear(ops.pack_weight(rnd(D, D)), D, D, None) for _ in range(2))
    Ee = ops.masked_linear(edge_emb, WE)
    out_p = new(N, D)
    dQ, dK, dV, dE = new(N, D), new(N, D), new(N, D), new(E, D)
    scr_p = new(2 * E * H)

    def sparse_fwd():
        check(L.sn_edge_attention_f32(ptr(Q), ptr(K), ptr(V), ptr(Ee), N, H, DK, ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(out_p), st),
              "sparse fwd")

    def sparse_bwd():
        check(L.sn_edge_attention_bwd_f32(ptr(Q), ptr(K), ptr(V), ptr(Ee), ptr(out_p), ptr(dout), N, E, H, DK, ptr(plan.rowptr), ptr(plan.col),
                                          ptr(plan.eperm), ptr(rplan.rowptr), ptr(rplan.col), ptr(rplan.eperm), ptr(dQ), ptr(dK), ptr(dV),
                                          ptr(dE), ptr(scr_p), st), "sparse bwd")

    def edge_gemms():
        ops.masked_linear(edge_emb, WE)
        ops.masked_linear(edge_emb, WE2)

    full_fwd()
    sparse_fwd()
    t = _alternate({"sn_full_attention_f32": full_fwd, "sn_edge_attention_f32_on_full_list": sparse_fwd,
                    "sn_full_attention_bwd_f32": full_bwd, "sn_edge_attention_bwd_f32_on_full_list": sparse_bwd,
                    "two_edge_projection_linears": edge_gemms})
    mk = _alternate({"sn_make_full_graph": lambda: ops.make_full_graph(g, e, status=status)})
    assert int(status.item()) == 0
    return dict(graphs=len(d.sizes), nodes=N, sparse_edges=int(src.numel()), full_edges=E, heads=H, dk=DK, classes=NC, launches=REPS,
                bytes_per_edge=dict(full=4, sparse_formulation=4 * D), edge_projection_bytes=E * D * 4, us_per_launch=t), \
        dict(graphs=len(d.sizes), nodes=N, full_edges=E, launches=REPS, us_per_launch=mk, note="includes the four output allocations")


def _net(full):
    cls, cfg = dgl_configs.net_params(CONFIG, DEV)
    cfg = dict(cfg, full_graph=full)
    torch.manual_seed(0)
    net = getattr(dgl_nets, cls)(cfg).to(DEV)
    return net, optim.FlatAdam(net.parameters(), lr=1e-4)


def _loops(full, batches):
    """(eval forward, eager training step) closures of one net over the batch sequence."""
    ev, _ = _net(full)
    ev.eval()
    tr, o = _net(full)
    tr.train()
    key = "gf" if full else "g"
    ekey = "ef" if full else "e"

    def fwd(b):
        with torch.no_grad():
            ev(b[key], b["h"], None, b[ekey], None)

    def step(b):          # train_ZINC_graph_regression.py:66-81 (the per-step loss.item() of :82 left out)
        o.zero_grad()
        y, _ = tr(b[key], b["h"], None, b[ekey], None)
        tr.loss(y, b["t"]).backward()
        o.step()
    return fwd, step, (ev, tr, o)


def net_times(with_full=True):
    batches = base._batches(16)
    if with_full:
        for b in batches:
            b["gf"], b["ef"] = ops.make_full_graph(b["g"], b["e"].reshape(-1).long())
    loops, keep = {}, []
    for full in ((False, True) if with_full else (False,)):
        fwd, step, k = _loops(full, batches)
        tag = "full" if full else "sparse"
        loops[f"eval_forward_{tag}"], loops[f"eager_step_{tag}"] = fwd, step
        keep.append(k)
    first = {k: base._pass(fn, batches) for k, fn in loops.items()}
    ms = {k: [] for k in loops}
    for _ in range(PASSES):
        for k, fn in loops.items():
            ms[k].append(base._pass(fn, batches))
    res = dict(config=CONFIG, hidden=keep[0][0].embedding_h.weight.shape[1], layers=len(keep[0][0].layers), batches=len(batches),
               graphs=base.GRAPHS, first_pass_ms=first, ms={k: _summary(v) for k, v in ms.items()})
    if with_full:
        res["edges"] = dict(sparse=[b["E"] for b in batches], full=[int(b["ef"].numel()) for b in batches])
    return res


def regression(parent, out):
    """(d): child processes alternating parent tree / this tree, three of the parent and two of this one."""
    runs = []
    for tree in (parent, ROOT, parent, ROOT, parent):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--child"], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError(f"child for {tree} failed:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        if os.path.realpath(r["package"]) != os.path.realpath(os.path.join(tree, "signnet_basisnet_amd")):
            raise RuntimeError(f"the child for {tree} imported {r['package']}")
        r["package"] = os.path.relpath(r["package"], ROOT)
        runs.append(dict(tree=os.path.relpath(tree, ROOT), **r))
    chk = {}
    for k in ("eval_forward_sparse", "eager_step_sparse"):
        par = [v for r in runs if r["tree"] != "." for v in r[k]["passes"]]
        mine = statistics.median([v for r in runs if r["tree"] == "." for v in r[k]["passes"]])
        chk[k] = dict(parent_range_ms=[min(par), max(par)], this_tree_median_ms=mine, inside=bool(min(par) <= mine <= max(par)),
                      not_slower=bool(mine <= max(par)))
    out["parent_ab_same_box"] = dict(note="full_graph=False, alternating child processes", runs=runs)
    out["regression_check"] = chk


def main():
    args = [a for a in sys.argv[1:]]
    if "--child" in args:
        r = net_times(with_full=False)
        import signnet_basisnet_amd
        print(json.dumps(dict(package=os.path.dirname(signnet_basisnet_amd.__file__), **r["ms"])))
        return
    parent = None
    if "--parent" in args:
        i = args.index("--parent")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "full_graph_attention.json")
    import bench
    res = dict(device=bench.device_block(DEV))
    res["attention"], res["make_full_graph"] = op_times()
    res["net"] = net_times()
    if parent:
        regression(parent, res)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for k, v in {**res["attention"]["us_per_launch"], **res["make_full_graph"]["us_per_launch"]}.items():
        print(f"{k}: {v['median']:.2f} us [{v['min']:.2f}, {v['max']:.2f}]")
    for k, v in res["net"]["ms"].items():
        print(f"{k}: {v['median']:.3f} ms [{v['min']:.3f}, {v['max']:.3f}]")
    if parent:
        print("regression check", json.dumps(res["regression_check"]))


if __name__ == "__main__":
    main()
