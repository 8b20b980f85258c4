"""The plain GNN of GINESignNetPyG for every model.gnn_type on one stack: eval ms per forward and eager training ms per step (FlatAdam) of

  GNN(None, None, 128, 1, 4, gnn_type, 0, 'add')   gnn_type in GINEConv, GINConv, GCNConv, GATConv, SimplifiedPNAConv

on the headline ZINC-like batch (bench.WORKLOAD: 128 graphs), in one process, the five alternating pass by pass (PASSES passes; median
and range); and the three new launches of a SimplifiedPNAConv layer alone (statistics, mean, adjoint) by device events at that batch's
shapes (C = 384), beside the same message / aggregate COMPOSED from torch ops on the device (context only: composed ops, not an earlier
implementation).

    python profiles/scripts/gnn_types.py [out.json]        (default: profiles/gnn_types.json)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import bench  # noqa: E402
from signnet_basisnet_amd import ops, optim, synth  # noqa: E402
from signnet_basisnet_amd.pyg_gnn_types import GNN, GNN_TYPES  # noqa: E402

DEV = "cuda:0"
W = bench.WORKLOAD
HIDDEN, LAYERS = 128, 4
PASSES = 5
EVAL_ITERS, TRAIN_ITERS, KERNEL_ITERS = 50, 20, 200


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


def _batch():
    return synth.make_batch(W["B"], seed=1, n_lo=W["n_lo"], n_hi=W["n_hi"], features=W["features"])


def _subjects(host):
    g = torch.Generator().manual_seed(0)
    data = synth.batch_to(host, DEV)
    target = torch.randn(host.num_graphs, 1, generator=g).to(DEV)
    out = {}
    for kind in GNN_TYPES:
        torch.manual_seed(0)
        m_eval = GNN(None, None, HIDDEN, 1, LAYERS, kind, 0, "add").to(DEV).eval()
        m_train = GNN(None, None, HIDDEN, 1, LAYERS, kind, 0, "add").to(DEV).train()
        o = optim.FlatAdam(m_train.parameters(), lr=1e-4)

        def fwd(m=m_eval):
            with torch.no_grad():
                return m(data)

        def step(m=m_train, o=o):
            o.zero_grad()
            (m(data) - target).abs().mean().backward()
            o.step()

        out[kind] = (fwd, step)
    return out


def _events(fn, iters=KERNEL_ITERS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _pna_launches_alone(host):
    """One SimplifiedPNAConv layer's message side at hidden 128 (C = 384) on the batch: the three new launches against the same
    quantities composed from torch ops on the device."""
    data = synth.batch_to(host, DEV)
    N, E, Cc = int(host.batch.numel()), int(host.edge_index.shape[1]), 3 * HIDDEN
    plan = ops.build_plan(data.batch, data.edge_index, host.num_graphs, 0)
    rplan = ops.build_plan(data.batch, data.edge_index.flip(0).contiguous(), host.num_graphs, 0)
    torch.manual_seed(0)
    ab = torch.randn(N, 2 * Cc, device=DEV)
    a, b, q, dr = ab[:, :Cc], ab[:, Cc:], torch.randn(E, Cc, device=DEV), torch.randn(N, Cc, device=DEV)
    bn = torch.nn.BatchNorm1d(Cc).to(DEV).train()
    src, dst = data.edge_index[0], data.edge_index[1]
    deg = torch.bincount(dst, minlength=N).clamp(min=1).unsqueeze(-1).float()
    state, _ = ops.spna_stats(a, b, q, plan, bn)

    def stats():
        return ops.spna_stats(a, b, q, plan, bn)

    def mean():
        return ops.spna_mean(a, b, q, plan, state[3], state[4])

    def adjoint():
        return ops.spna_bwd(a, b, q, plan, rplan, dr, state=state, gamma=bn.weight.detach())

    @torch.no_grad()
    def composed_stats():
        z = a[dst] + b[src] + q
        return z.mean(0), z.var(0, unbiased=False)

    @torch.no_grad()
    def composed_mean():
        y = torch.relu(F.batch_norm(a[dst] + b[src] + q, None, None, bn.weight, bn.bias, True, 0.0, bn.eps))
        return torch.zeros(N, Cc, device=DEV).index_add_(0, dst, y) / deg

    def composed_fwd_bwd():
        leaves = [t.detach().requires_grad_(True) for t in (a, b, q)]
        y = torch.relu(F.batch_norm(leaves[0][dst] + leaves[1][src] + leaves[2], None, None, bn.weight, bn.bias, True, 0.0, bn.eps))
        r = torch.zeros(N, Cc, device=DEV).index_add(0, dst, y) / deg
        r.backward(dr)
        return leaves[0].grad

    err = float((mean() - composed_mean()).abs().max() / composed_mean().abs().max())
    fns = dict(sn_spna_stats_f32=stats, sn_spna_mean_f32=mean, sn_spna_bwd_f32=adjoint, composed_torch_moments=composed_stats,
               composed_torch_mean=composed_mean, composed_torch_forward_and_backward=composed_fwd_bwd)
    for fn in fns.values():
        _events(fn, 10)                  # warm-up
    ms = {k: [] for k in fns}
    for _ in range(PASSES):
        for k, fn in fns.items():
            ms[k].append(_events(fn))
    return dict(nodes=N, edges=E, C=Cc, max_rel_diff_mean_vs_composed=err, ms={k: _stat(v) for k, v in ms.items()},
                note="device events over back-to-back calls, entry points alternating pass by pass; sn_spna_stats_f32 is two kernels "
                     "(partials, merge), sn_spna_bwd_f32 four (column sums, finish, apply, out-edge sums); the composed_* rows are the same "
                     "quantities from torch ops on the device (gathers, batch_norm, index_add; forward_and_backward includes the forward "
                     "that autograd needs) — context only, not an earlier implementation")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gnn_types.json")
    host = _batch()
    subjects = _subjects(host)
    for fwd, step in subjects.values():             # warm-up: lazy setup, allocator, packed weights
        _pass(fwd, 5)
        _pass(step, 5)
    ev = {n: [] for n in subjects}
    tr = {n: [] for n in subjects}
    for _ in range(PASSES):                         # the subjects alternate pass by pass: a drift of the clock or the host hits all
        for n, (fwd, step) in subjects.items():
            ev[n].append(_pass(fwd, EVAL_ITERS))
        for n, (fwd, step) in subjects.items():
            tr[n].append(_pass(step, TRAIN_ITERS))
    res = dict(device=bench.device_block(DEV), passes=PASSES,
               batch=dict(graphs=host.num_graphs, nodes=int(host.batch.numel()), edges=int(host.edge_index.shape[1])),
               model=f"GNN(None, None, {HIDDEN}, 1, {LAYERS}, gnn_type, 0, 'add')",
               models=[dict(gnn_type=n, eval_ms_per_forward=_stat(ev[n]), train_ms_per_step=_stat(tr[n])) for n in subjects],
               simplified_pna_launches=_pna_launches_alone(host))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for m in res["models"]:
        e, t = m["eval_ms_per_forward"], m["train_ms_per_step"]
        print(f"{m['gnn_type']}: eval {e['median']:.3f} ms [{e['min']:.3f}, {e['max']:.3f}], train {t['median']:.3f} ms/step [{t['min']:.3f}, {t['max']:.3f}]")
    for k, v in res["simplified_pna_launches"]["ms"].items():
        print(f"{k}: {v['median']:.4f} ms [{v['min']:.4f}, {v['max']:.4f}]")


if __name__ == "__main__":
    main()
