"""The three sign-invariant encoders of the DGL tree behind one base network: GatedGCNNet at the shipped
GatedGCN_ZINC_LapPE_signinv_GIN sizes (dgl_configs.SHIPPED['gatedgcn']) on 128 ZINC-like graphs, with sign_inv_net 'gin', 'gcn' and
'transformer' —

  eval ms per forward                   sign_inv_net + base net, eager launches
  eager training ms per step            forward, backward, optim.FlatAdam
  ms per train_graph.DGLBucketedStep    the captured step on the same batch

in one process, the three kinds alternating pass by pass (PASSES passes; median and range), and the two new launches alone
(sn_gcn_propagate_f32, sn_graph_attention_f32 and its backward) back to back by device events at the shapes the encoders give them.
What is measured is written down; nothing is compared with a threshold (there is no earlier implementation of these paths).

    python profiles/scripts/deepsigns_variants.py [out.json]        (default: profiles/deepsigns_variants.json)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from signnet_basisnet_amd import dgl_configs, dgl_nets, ops, optim, synth  # noqa: E402
from signnet_basisnet_amd import dgl_deepsigns as DS  # noqa: E402
from signnet_basisnet_amd.train_graph import DGLBucketedStep  # noqa: E402

DEV = "cuda:0"
KINDS = ("gin", "gcn", "transformer")
PASSES = 5
EVAL_ITERS, TRAIN_ITERS, OP_ITERS = 30, 10, 200


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
    data = synth.make_batch(128, seed=1)
    k = dgl_configs.SHIPPED["gatedgcn"]["pos_enc_dim"]
    src, dst = data.edge_index
    g = DS.Graph(src.to(DEV), dst.to(DEV), data.sizes)
    t = torch.randn(128, 1, generator=torch.Generator().manual_seed(0)).to(DEV)
    return data, g, data.x.squeeze(-1).to(DEV), synth.dgl_pos_enc(data, k).to(DEV), data.edge_attr.to(DEV), t


def _net(kind):
    cls, p = dgl_configs.net_params("gatedgcn", DEV)
    p["sign_inv_net"] = kind
    torch.manual_seed(0)
    return getattr(dgl_nets, cls)(p).to(DEV)


def _subjects(g, h, pe, e, t):
    out = {}
    for kind in KINDS:
        m_eval, m_train, m_cap = _net(kind).eval(), _net(kind).train(), _net(kind).train()
        o_train = optim.FlatAdam(m_train.parameters(), lr=1e-4)
        captured = DGLBucketedStep(m_cap, optim.FlatAdam(m_cap.parameters(), lr=1e-4), max_graphs=128)

        def fwd(m=m_eval):
            with torch.no_grad():
                p = m.sign_inv_net(g, pe.unsqueeze(-1)).squeeze(-1)
                return m(g, h, p, e, None)[0]

        def step(m=m_train, o=o_train):
            o.zero_grad()
            p = m.sign_inv_net(g, pe.unsqueeze(-1)).squeeze(-1)
            m.loss(m(g, h, p, e, None)[0], t).backward()
            o.step()

        def cap(s=captured):
            s.step(g, h, pe, e, None, t)

        out[kind] = (fwd, step, cap, sum(q.numel() for q in m_eval.sign_inv_net.parameters()))
    return out


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(OP_ITERS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / OP_ITERS


def _ops_alone(data, g):
    """The two launches at the shapes of the encoders above: the propagation over [N, 2 k hidden] (eval: both signs in the slot axis),
    the attention over N * 2 k rows of 2 heads of hidden // 2."""
    cfg = dgl_configs.SHIPPED["gatedgcn"]
    hidden, k = cfg["hidden_dim"], cfg["pos_enc_dim"]
    N = int(data.batch.numel())
    plan = DS.cached_plan(g, N)
    rplan = DS._cached_rplan(g, N)
    x = torch.randn(N, 2 * k * hidden, device=DEV)
    S, H, dh = 2 * k, 2, hidden // 2
    qkv = torch.randn(N * S, 3 * H * dh, device=DEV)
    D = H * dh
    q, kk, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
    out, lse = ops.graph_attention(q, kk, v, plan.graph_ptr, N, S, H)
    go = torch.randn_like(out)
    fns = {"sn_gcn_propagate_f32": lambda: ops.gcn_propagate(x, plan, rplan),
           "sn_graph_attention_f32": lambda: ops.graph_attention(q, kk, v, plan.graph_ptr, N, S, H),
           "sn_graph_attention_bwd_f32": lambda: ops.graph_attention_bwd(q, kk, v, out, lse, go, plan.graph_ptr, N, S, H)}
    for fn in fns.values():
        _events(fn)                      # warm-up
    ms = {n: [] for n in fns}
    for _ in range(PASSES):
        for n, fn in fns.items():
            ms[n].append(_events(fn))
    return dict(shapes=dict(nodes=N, edges=int(data.edge_index.shape[1]), graphs=128, propagate_row_floats=2 * k * hidden,
                            attention_rows=N * S, heads=H, head_width=dh),
                ms_per_launch={n: _stat(v) for n, v in ms.items()},
                note="device events over back-to-back calls (the output allocation of the Python wrapper included)")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "deepsigns_variants.json")
    data, g, h, pe, e, t = _batch()
    subjects = _subjects(g, h, pe, e, t)
    for fwd, step, cap, _ in subjects.values():          # warm-up: lazy setup, allocator, packed weights, the capture
        _pass(fwd, 3)
        _pass(step, 3)
        _pass(cap, 3)
    ev, tr, cp = ({n: [] for n in subjects} for _ in range(3))
    for _ in range(PASSES):                              # the kinds alternate pass by pass: a drift of the clock or the host hits all
        for n, (fwd, step, cap, _) in subjects.items():
            ev[n].append(_pass(fwd, EVAL_ITERS))
        for n, (fwd, step, cap, _) in subjects.items():
            tr[n].append(_pass(step, TRAIN_ITERS))
        for n, (fwd, step, cap, _) in subjects.items():
            cp[n].append(_pass(cap, TRAIN_ITERS))
    res = dict(device=bench.device_block(DEV), passes=PASSES, base_net="GatedGCNNet (dgl_configs.SHIPPED['gatedgcn'])",
               batch=dict(graphs=128, nodes=int(data.batch.numel()), edges=int(data.edge_index.shape[1])),
               kinds=[dict(sign_inv_net=n, sign_inv_parameters=subjects[n][3], eval_ms_per_forward=_stat(ev[n]),
                           eager_train_ms_per_step=_stat(tr[n]), bucketed_step_ms=_stat(cp[n])) for n in subjects],
               launches=_ops_alone(data, g))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for m in res["kinds"]:
        e_, t_, c_ = m["eval_ms_per_forward"], m["eager_train_ms_per_step"], m["bucketed_step_ms"]
        print(f"{m['sign_inv_net']}: eval {e_['median']:.3f} ms [{e_['min']:.3f}, {e_['max']:.3f}], eager train {t_['median']:.3f} ms/step "
              f"[{t_['min']:.3f}, {t_['max']:.3f}], bucketed step {c_['median']:.3f} ms [{c_['min']:.3f}, {c_['max']:.3f}]")
    for n, s in res["launches"]["ms_per_launch"].items():
        print(f"{n}: {s['median']:.4f} ms [{s['min']:.4f}, {s['max']:.4f}]")


if __name__ == "__main__":
    main()
