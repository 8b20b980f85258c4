"""The LearningFilters table's baseline rows next to a sign / basis invariant row on one stack, on the reference's graph (32 x 32 grid,
N = 1024) at its defaults (hidden 32, 2 layers, K = 10): eval ms per forward, eager training ms per epoch (learning_filters.train_step)
and captured ms per epoch (learning_filters.GraphedEpoch) of

  BernNet, GPRNet            filter_baselines.py (csrc/poly_filter.hip), no eigenvector features (training.py's defaults)
  DS + BasisNet              --net DS --use_eig --lap_method basis_inv  (the existing row of the table)

in one process, the three alternating pass by pass (PASSES passes; median and range), and BernConv's propagation at width 32 alone by
device events: the two launches (sn_poly_basis_f32 + sn_poly_combine_f32) beside the same 65 propagations COMPOSED from torch.sparse.mm
on the device (context only: composed ops, not an earlier implementation).

    python profiles/scripts/filter_baselines.py [out.json]        (default: profiles/filter_baselines.json)
"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from signnet_basisnet_amd import autograd as AG  # noqa: E402
from signnet_basisnet_amd import learning_filters as LF  # noqa: E402
from signnet_basisnet_amd import optim, synth  # noqa: E402
from signnet_basisnet_amd.filter_baselines import FilterGraph  # noqa: E402

DEV = "cuda:0"
SIDE, PASSES = 32, 5
EVAL_ITERS, TRAIN_ITERS, PROP_ITERS = 1000, 150, 1000      # >= 0.1 s of device work per timed pass for the fastest subject


def _pass(fn, iters):
    """ms per call over one pass of `iters` calls (host clock around work that ends in a device synchronise)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def _stat(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), passes=v)


def _grid():
    """utils.py:67-78 + training.py:42-43: dense sym-normalised Laplacian and eigh in float64, then .float()."""
    ei, N = synth.grid_graph(SIDE)
    A = np.zeros((N, N))
    A[ei[0], ei[1]] = 1.0
    dis = 1.0 / np.sqrt(A.sum(1))
    w, V = np.linalg.eigh(np.eye(N) - dis[:, None] * A * dis[None, :])
    return torch.as_tensor(np.asarray(ei)), N, torch.from_numpy(w).float().to(DEV), torch.from_numpy(V).float().to(DEV)


def _subjects(ei, N, D, V):
    """name -> (eval forward, eager epoch, captured epoch)"""
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(N, 1, generator=g).to(DEV), torch.randn(N, 1, generator=g).to(DEV)
    m = torch.ones(N, 1, device=DEV)
    graph = FilterGraph(ei.to(DEV), N)
    out = {}
    for name, a, gr in (("BernNet", dict(net="BernNet"), graph), ("GPRNet", dict(net="GPRNet"), graph),
                        ("DS + BasisNet (basis_inv, IGN)", dict(net="DS", use_eig=True, lap_method="basis_inv"), None)):
        args = LF.FilterArgs(**a)
        eig = LF.GridEigen(D, V, args)
        torch.manual_seed(0)
        np.random.seed(0)
        nets = [LF.gen_model(args, eig, DEV, baselines=gr is not None) for _ in range(3)]
        m_eval, m_eager, m_graph = nets
        m_eval.eval()
        o_eager, o_graph = (optim.FlatAdam(n.parameters(), lr=args.lr) for n in (m_eager, m_graph))
        ge = LF.GraphedEpoch(m_graph, o_graph, args, eig, x, y, m, graph=gr)

        def fwd(mod=m_eval, args=args, eig=eig, gr=gr):
            with torch.no_grad():
                return mod(LF.get_lap_feat(args.use_eig, eig, x, args.lap_method, mod), gr)

        def eager(mod=m_eager, o=o_eager, args=args, eig=eig, gr=gr):
            return LF.train_step(mod, o, args, eig, x, y, m, gr)

        out[name] = (fwd, eager, ge.step)
    return out


def _bernstein_alone(ei, N):
    """BernConv's propagation of one [N, 32] block, K = 10: two launches vs models.py:326-340 composed from torch.sparse.mm."""
    K, d = 10, 32
    graph = FilterGraph(ei.to(DEV), N)
    op = graph.lap
    rows = torch.repeat_interleave(torch.arange(N, device=DEV), (op.rowptr[1:] - op.rowptr[:-1]).long())
    A = torch.sparse_coo_tensor(torch.stack([rows, op.col.long()]), op.w, (N, N)).coalesce()
    eye = torch.sparse_coo_tensor(torch.stack([torch.arange(N, device=DEV)] * 2), torch.ones(N, device=DEV), (N, N))
    L, M = (eye - A).coalesce(), (eye + A).coalesce()
    x = torch.randn(N, d, generator=torch.Generator().manual_seed(0)).to(DEV)
    c = torch.tensor([math.comb(K, i) / 2.0 ** K for i in range(K + 1)], device=DEV)
    crev = c.flip(0).contiguous()

    @torch.no_grad()
    def kernel():
        return AG.bern_prop(x, c, crev, op, K)

    @torch.no_grad()
    def composed():
        h, tmp = x, [x]
        for _ in range(K):
            h = torch.sparse.mm(M, h)
            tmp.append(h)
        out = c[0] * tmp[K]
        for i in range(K):
            h = torch.sparse.mm(L, tmp[K - i - 1])
            for _ in range(i):
                h = torch.sparse.mm(L, h)
            out = out + c[i + 1] * h
        return out

    err = float((kernel() - composed()).abs().max() / composed().abs().max())

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(PROP_ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / PROP_ITERS

    for fn in (kernel, composed):
        events(fn)                       # warm-up
    k_ms, c_ms = [], []
    for _ in range(PASSES):
        k_ms.append(events(kernel))
        c_ms.append(events(composed))
    return dict(nodes=N, width=d, K=K, max_rel_diff_vs_composed=err, two_launches_ms=_stat(k_ms), composed_65_sparse_mm_ms=_stat(c_ms),
                note="device events over back-to-back calls; composed_65_sparse_mm is BernConv's original 65 propagations from "
                     "torch.sparse.mm on the device, context only")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "filter_baselines.json")
    ei, N, D, V = _grid()
    subjects = _subjects(ei, N, D, V)
    for fns in subjects.values():                    # warm-up: lazy setup, allocator, packed weights
        for fn in fns:
            _pass(fn, 5)
    res = {n: ([], [], []) for n in subjects}
    for _ in range(PASSES):                          # the subjects alternate pass by pass: a drift of the clock or the host hits all
        for col, iters in ((0, EVAL_ITERS), (1, TRAIN_ITERS), (2, TRAIN_ITERS)):
            for n, fns in subjects.items():
                res[n][col].append(_pass(fns[col], iters))
    doc = dict(device=bench.device_block(DEV), passes=PASSES, grid=f"{SIDE} x {SIDE}", nodes=N, hidden=32, layers=2, K=10,
               models=[dict(model=n, eval_ms_per_forward=_stat(r[0]), eager_train_ms_per_epoch=_stat(r[1]),
                            graphed_train_ms_per_epoch=_stat(r[2])) for n, r in res.items()],
               bernstein_propagation=_bernstein_alone(ei, N))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    for mm in doc["models"]:
        e, t, gq = mm["eval_ms_per_forward"], mm["eager_train_ms_per_epoch"], mm["graphed_train_ms_per_epoch"]
        print(f"{mm['model']}: eval {e['median']:.3f} ms [{e['min']:.3f}, {e['max']:.3f}], eager {t['median']:.3f} ms/epoch "
              f"[{t['min']:.3f}, {t['max']:.3f}], graphed {gq['median']:.3f} ms/epoch [{gq['min']:.3f}, {gq['max']:.3f}]")
    s = doc["bernstein_propagation"]
    print(f"Bernstein propagation: two launches {s['two_launches_ms']['median']:.4f} ms vs 65 composed torch.sparse.mm "
          f"{s['composed_65_sparse_mm_ms']['median']:.4f} ms (max rel diff {s['max_rel_diff_vs_composed']:.1e})")


if __name__ == "__main__":
    main()
