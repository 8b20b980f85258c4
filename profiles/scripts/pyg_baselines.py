"""The PyG trees' baselines next to SignNet on one stack: eval ms per forward and eager training ms per step of

  NetGINE(64)                      on a 128-graph Alchemy-like batch (synth.make_batch(features="alchemy", n_lo=6, n_hi=14))
  GNN(None, None, 128, 1, 6, ...)  on the headline ZINC-like batch (bench.WORKLOAD), pooling 'add', no positional encoding
  SignNetGNN                       at its shipped sizes on the same ZINC-like batch (bench.build_model)

in one process, the three alternating pass by pass (PASSES passes; median and range), and the Set2Set launch alone by device events
beside the same readout COMPOSED from torch ops on the device (context only: composed ops, not an earlier implementation).

    python profiles/scripts/pyg_baselines.py [out.json]        (default: profiles/pyg_baselines.json)
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
from signnet_basisnet_amd import ops, optim, synth  # noqa: E402
from signnet_basisnet_amd.pyg import GNN  # noqa: E402
from signnet_basisnet_amd.pyg_baselines import NetGINE  # noqa: E402

DEV = "cuda:0"
W = bench.WORKLOAD
PASSES = 5
EVAL_ITERS, TRAIN_ITERS, S2S_ITERS = 50, 20, 200


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


def _subjects():
    """name -> (eval forward, eager training step, description of the batch)"""
    g = torch.Generator().manual_seed(0)
    alch = synth.make_batch(128, seed=1, n_lo=6, n_hi=14, features="alchemy")
    zinc = synth.make_batch(W["B"], seed=1, n_lo=W["n_lo"], n_hi=W["n_hi"], features=W["features"])
    out = {}
    torch.manual_seed(0)
    for name, host, n_out, make in (
            ("NetGINE(64)", alch, 12, lambda: NetGINE(64)),
            (f"GNN(None, None, {W['hidden']}, 1, {W['nl_gnn']}, 'gine', 'add')", zinc, 1,
             lambda: GNN(None, None, W["hidden"], 1, W["nl_gnn"], "gine", "add")),
            ("SignNetGNN (bench workload)", zinc, W["n_out"], lambda: bench.build_model(DEV))):
        data = synth.batch_to(host, DEV)
        target = torch.randn(host.num_graphs, n_out, generator=g).to(DEV)
        m_eval, m_train = make().to(DEV).eval(), make().to(DEV).train()
        if hasattr(m_eval, "strict"):
            m_eval.strict = False          # the throughput mode bench.py times
        o = optim.FlatAdam(m_train.parameters(), lr=1e-4)

        def fwd(m=m_eval, d=data):
            with torch.no_grad():
                return m(d)

        def step(m=m_train, d=data, t=target, o=o):
            o.zero_grad()
            (m(d) - t).abs().mean().backward()
            o.step()

        out[name] = (fwd, step, dict(graphs=host.num_graphs, nodes=int(host.batch.numel()), edges=int(host.edge_index.shape[1])))
    return out


def _set2set_alone():
    """The readout of NetGINE(64) on the Alchemy-like batch: the one launch of ops.set2set vs the readout composed from torch ops."""
    host = synth.make_batch(128, seed=1, n_lo=6, n_hi=14, features="alchemy")
    d, T, B = 64, 6, host.num_graphs
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(2 * d, d).to(DEV)
    x = torch.randn(host.batch.numel(), d, device=DEV)
    batch = host.batch.to(DEV)
    gp = torch.tensor([0] + host.sizes, dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)
    ws = [t.detach() for t in (lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0)]

    def kernel():
        return ops.set2set(x, gp, *ws, T)

    @torch.no_grad()
    def composed():
        state = (x.new_zeros(1, B, d), x.new_zeros(1, B, d))
        qs = x.new_zeros(B, 2 * d)
        for _ in range(T):
            q, state = lstm(qs.unsqueeze(0), state)
            q = q.view(B, d)
            e = (x * q.index_select(0, batch)).sum(-1)
            top = x.new_full((B,), float("-inf")).scatter_reduce(0, batch, e, "amax", include_self=True)
            p = (e - top.index_select(0, batch)).exp()
            a = p / (x.new_zeros(B).index_add(0, batch, p).index_select(0, batch) + 1e-16)
            qs = torch.cat([q, x.new_zeros(B, d).index_add(0, batch, a.unsqueeze(-1) * x)], -1)
        return qs

    err = float((kernel() - composed()).abs().max() / composed().abs().max())

    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(S2S_ITERS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / S2S_ITERS

    for fn in (kernel, composed):
        events(fn)                       # warm-up
    k_ms, c_ms = [], []
    for _ in range(PASSES):
        k_ms.append(events(kernel))
        c_ms.append(events(composed))
    return dict(d=d, steps=T, graphs=B, nodes=int(x.shape[0]), max_rel_diff_vs_composed=err,
                set2set_launch_ms=_stat(k_ms), composed_torch_ops_ms=_stat(c_ms),
                note="device events over back-to-back calls; composed_torch_ops is the same readout from torch ops on the device "
                     "(nn.LSTM + index ops), context only")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pyg_baselines.json")
    subjects = _subjects()
    for fwd, step, _ in subjects.values():          # warm-up: lazy setup, allocator, packed weights
        _pass(fwd, 5)
        _pass(step, 5)
    ev = {n: [] for n in subjects}
    tr = {n: [] for n in subjects}
    for _ in range(PASSES):                         # the subjects alternate pass by pass: a drift of the clock or the host hits all
        for n, (fwd, step, _) in subjects.items():
            ev[n].append(_pass(fwd, EVAL_ITERS))
        for n, (fwd, step, _) in subjects.items():
            tr[n].append(_pass(step, TRAIN_ITERS))
    res = dict(device=bench.device_block(DEV), passes=PASSES,
               models=[dict(model=n, batch=subjects[n][2], eval_ms_per_forward=_stat(ev[n]), train_ms_per_step=_stat(tr[n])) for n in subjects],
               set2set=_set2set_alone())
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    for m in res["models"]:
        e, t = m["eval_ms_per_forward"], m["train_ms_per_step"]
        print(f"{m['model']}: eval {e['median']:.3f} ms [{e['min']:.3f}, {e['max']:.3f}], train {t['median']:.3f} ms/step [{t['min']:.3f}, {t['max']:.3f}]")
    s = res["set2set"]
    print(f"set2set launch {s['set2set_launch_ms']['median']:.4f} ms vs composed torch ops {s['composed_torch_ops_ms']['median']:.4f} ms "
          f"(max rel diff {s['max_rel_diff_vs_composed']:.1e})")


if __name__ == "__main__":
    main()
