"""GatNet and ARMANet, the last two rows of the LearningFilters table, next to BernNet on the reference's graph (32 x 32 grid, N = 1024)
at its defaults (hidden 32, 2 layers, 4 heads): eval ms per forward, captured ms per epoch (learning_filters.GraphedEpoch) and the
recorded entry-point launches of one eager epoch, in one process, the three alternating pass by pass (PASSES passes; median and range).
BernNet is the check that the box agrees with profiles/filter_baselines.json.

The attention launch alone (one GATConv layer behind its Linear: [1024, 4 * 8], ELU) by device events, forward and adjoint, beside the
same layer COMPOSED from torch ops on the device (gather, leaky_relu, scatter_reduce amax, exp, index_add; autograd for the adjoint) —
context only: composed ops, not an earlier implementation.

    python profiles/scripts/filter_attention.py [out.json]        (default: profiles/filter_attention.json)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from signnet_basisnet_amd import learning_filters as LF  # noqa: E402
from signnet_basisnet_amd import ops, optim, synth  # noqa: E402
from signnet_basisnet_amd.filter_baselines import FilterGraph  # noqa: E402

DEV = "cuda:0"
SIDE, PASSES = 32, 5
EVAL_ITERS, TRAIN_ITERS = 1000, 150     # the model rows: about 0.1 s (GatNet's forward) or more of device work per timed pass
LAYER_ITERS = 1000                      # the single-layer rows: 13 ms or more per pass, host enqueue included — context, not kernel times
LAUNCHES = {"sn_gat_conv_bwd_f32": 2}                       # launches behind one recorded entry point, where it is not one


def _pass(fn, iters):
    """ms per call over one pass of `iters` calls (host clock around work that ends in a device synchronise)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _events(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), passes=v)


def _subjects(ei, N):
    """name -> (eval forward, captured epoch, recorded launches of one eager epoch)"""
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(N, 1, generator=g).to(DEV), torch.randn(N, 1, generator=g).to(DEV)
    m = torch.ones(N, 1, device=DEV)
    graph = FilterGraph(ei.to(DEV), N)
    zero = torch.zeros(N, device=DEV)
    out = {}
    for name in ("GatNet", "ARMANet", "BernNet"):
        args = LF.FilterArgs(net=name)
        eig = LF.GridEigen(zero, torch.zeros(N, N, device=DEV), args)          # no eigenvector features (training.py's defaults)
        torch.manual_seed(0)
        m_eval, m_eager, m_graph = (LF.gen_model(args, eig, DEV, baselines="all") for _ in range(3))
        m_eval.eval()
        o_eager, o_graph = (optim.FlatAdam(n.parameters(), lr=args.lr) for n in (m_eager, m_graph))
        ge = LF.GraphedEpoch(m_graph, o_graph, args, eig, x, y, m, graph=graph)

        def fwd(mod=m_eval):
            with torch.no_grad():
                return mod(x, graph)

        LF.train_step(m_eager, o_eager, args, eig, x, y, m, graph)
        rec = ops.KernelTimer()
        with rec:
            LF.train_step(m_eager, o_eager, args, eig, x, y, m, graph)
        names = [n for n, _, _ in rec.spans]
        out[name] = (fwd, ge.step, dict(recorded=sum(LAUNCHES.get(n, 1) for n in names),
                                        by_entry_point={n: names.count(n) * LAUNCHES.get(n, 1) for n in sorted(set(names))}))
    return out


def _attention_alone(ei, N):
    heads, C = 4, 8
    graph = FilterGraph(ei.to(DEV), N)
    op = graph.lap
    g = torch.Generator().manual_seed(0)
    feat, al, ar, b, cot = (torch.randn(*s, generator=g).to(DEV) for s in ((N, heads * C), (heads * C,), (heads * C,), (heads * C,), (N, heads * C)))
    dst = torch.repeat_interleave(torch.arange(N, device=DEV), (op.rowptr[1:] - op.rowptr[:-1]).long())
    loop = torch.arange(N, device=DEV)
    src, dst = torch.cat([op.col.long(), loop]), torch.cat([dst, loop])
    idx = dst.view(-1, 1).expand(-1, heads)

    def composed(f):
        fh = f.view(N, heads, C)
        e = torch.nn.functional.leaky_relu((fh * al.view(1, heads, C)).sum(-1)[src] + (fh * ar.view(1, heads, C)).sum(-1)[dst], 0.2)
        top = torch.full((N, heads), float("-inf"), device=DEV).scatter_reduce(0, idx, e.detach(), "amax")
        p = (e - top[dst]).exp()
        a = p / torch.zeros(N, heads, device=DEV).index_add(0, dst, p)[dst]
        return torch.nn.functional.elu(torch.zeros(N, heads, C, device=DEV).index_add(0, dst, a.unsqueeze(-1) * fh[src]).view(N, -1) + b)

    out, lse = ops.gat_conv(feat, al, ar, b, op, heads, "elu")
    fr = feat.clone().requires_grad_(True)
    ref = composed(fr)
    err = float((out - ref).abs().max() / ref.abs().max())
    ref.backward(cot)
    dfeat = ops.gat_conv_bwd(feat, al, ar, out, lse, cot, op, heads, "elu")[0]
    err_b = float((dfeat - fr.grad).abs().max() / fr.grad.abs().max())

    @torch.no_grad()
    def k_fwd():
        return ops.gat_conv(feat, al, ar, b, op, heads, "elu")

    @torch.no_grad()
    def k_bwd():
        return ops.gat_conv_bwd(feat, al, ar, out, lse, cot, op, heads, "elu")

    @torch.no_grad()
    def c_fwd():
        return composed(feat)

    def c_both():
        f = feat.detach().requires_grad_(True)
        composed(f).backward(cot)

    fns = dict(kernel_forward_ms=k_fwd, kernel_adjoint_ms=k_bwd, composed_forward_ms=c_fwd, composed_forward_and_adjoint_ms=c_both)
    for fn in fns.values():
        _events(fn, 20)
    res = {k: [] for k in fns}
    for _ in range(PASSES):
        for k, fn in fns.items():
            res[k].append(_events(fn, LAYER_ITERS))
    doc = dict(nodes=N, heads=heads, channels=C, edges=int(op.nnz), max_rel_diff_forward_vs_composed=err, max_rel_diff_dfeat_vs_composed=err_b,
               note="device events over back-to-back calls; kernel_adjoint is sn_gat_conv_bwd_f32 (two launches) and the reduction of the "
                    "parameter partials; composed_* is the same layer from torch ops on the device, context only")
    doc.update({k: _stat(v) for k, v in res.items()})
    return doc


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "filter_attention.json")
    ei, N = synth.grid_graph(SIDE)
    ei = torch.as_tensor(np.asarray(ei))
    subjects = _subjects(ei, N)
    for fwd, step, _ in subjects.values():           # warm-up: lazy setup, allocator, packed weights
        _pass(fwd, 5)
        _pass(step, 5)
    res = {n: ([], []) for n in subjects}
    for _ in range(PASSES):                          # the subjects alternate pass by pass: a drift of the clock or the host hits all
        for col, iters in ((0, EVAL_ITERS), (1, TRAIN_ITERS)):
            for n, fns in subjects.items():
                res[n][col].append(_pass(fns[col], iters))
    doc = dict(device=bench.device_block(DEV), passes=PASSES, grid=f"{SIDE} x {SIDE}", nodes=N, hidden=32, layers=2, heads=4,
               models=[dict(model=n, eval_ms_per_forward=_stat(r[0]), graphed_train_ms_per_epoch=_stat(r[1]),
                            eager_epoch_launches=subjects[n][2]) for n, r in res.items()],
               launches_note="entry points recorded by ops.KernelTimer over one eager epoch (sn_gat_conv_bwd_f32 counted as its two "
                             "launches); weight packing, the ReLU adjoint, the optimiser and torch's own kernels (loss, cat, "
                             "gradient accumulation) are not recorded",
               attention_layer=_attention_alone(ei, N))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    for mm in doc["models"]:
        e, gq = mm["eval_ms_per_forward"], mm["graphed_train_ms_per_epoch"]
        print(f"{mm['model']}: eval {e['median']:.3f} ms [{e['min']:.3f}, {e['max']:.3f}], graphed {gq['median']:.3f} ms/epoch "
              f"[{gq['min']:.3f}, {gq['max']:.3f}], recorded launches per eager epoch {mm['eager_epoch_launches']['recorded']}")
    s = doc["attention_layer"]
    print(f"attention layer: kernel forward {s['kernel_forward_ms']['median']:.4f} ms, adjoint {s['kernel_adjoint_ms']['median']:.4f} ms; composed "
          f"forward {s['composed_forward_ms']['median']:.4f} ms, forward + adjoint {s['composed_forward_and_adjoint_ms']['median']:.4f} ms "
          f"(max rel diff {s['max_rel_diff_forward_vs_composed']:.1e} / {s['max_rel_diff_dfeat_vs_composed']:.1e})")


if __name__ == "__main__":
    main()
