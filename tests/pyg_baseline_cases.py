"""Shared by tests/test_pyg_baselines_cpu.py and tests/test_pyg_baselines_gpu.py: the case tables of the Set2Set kernel and CPU
restatements (float32 / float64, differentiable) of the three things the PyG baselines add —

  set2set_ref   PyG's Set2Set(d, processing_steps=T) from its published definition on torch.nn.LSTM plus index ops (an implementation of
                the LSTM cell independent of csrc/set2set.hip)
  netgine_ref   Alchemy/baseline_gin.py's NetGINE from a reference-keyed state_dict
  plain_gnn_ref GINESignNetPyG/core/model.py's GNN (gnn_type 'GINEConv') from a reference-keyed state_dict, on the oracle's blocks

The fixtures (tests/golden/netgine_*.npz, plain_gnn_*.npz: the reference's own modules, tests/golden/make_pyg_baselines.py) pin the
restatements in the CPU test; the GPU test then compares the kernels with them in float64.
"""
import types

import torch
import torch.nn.functional as F

from oracle import pyg_signnet as O

NETGINE_CASES = ["netgine_d16", "netgine_d64"]
PLAIN_GNN_CASES = ["plain_gnn_h16_l2_add", "plain_gnn_h16_l4_mean", "plain_gnn_h32_l2_mean_pe", "plain_gnn_h32_l4_add_pe"]
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

# single node, empty graph, the 64/65 boundary of a wave, several chunks of the node stream
MIXED = [1, 0, 64, 65, 200, 9, 37]
# id -> d, T, graph sizes, scale of x, x as a view offset by one float
SET2SET_CASES = {
    **{f"d{d}_T{T}": dict(d=d, T=T, sizes=MIXED) for d in (4, 64, 100, 128) for T in (1, 6)},      # under a vector, shipped, ragged, the limit
    "one_graph": dict(d=64, T=6, sizes=[37]),
    "empty_ends": dict(d=100, T=6, sizes=[0, 5, 70, 0]),
    "offset_view": dict(d=64, T=6, sizes=MIXED, offset=True),
    "saturated": dict(d=64, T=6, sizes=MIXED, scale=8.0),
}


def set2set_inputs(case, seed=0):
    """x [N, d] (unit scale times `scale`), the four LSTM tensors as torch.nn.LSTM(2d, d) initialises them, an upstream gradient [B, 2d]."""
    c = SET2SET_CASES[case] if isinstance(case, str) else case
    d, sizes = c["d"], c["sizes"]
    g = torch.Generator().manual_seed(1000 + seed + d + 7 * c["T"] + len(sizes))
    torch.manual_seed(2000 + seed + d)
    lstm = torch.nn.LSTM(2 * d, d)
    x = torch.randn(sum(sizes), d, generator=g) * c.get("scale", 1.0)
    gout = torch.randn(len(sizes), 2 * d, generator=g)
    return types.SimpleNamespace(d=d, T=c["T"], sizes=list(sizes), x=x, gout=gout, offset=bool(c.get("offset")),
                                 lstm={k: getattr(lstm, k).detach().clone() for k in LSTM_KEYS})


def set2set_ref(x, sizes, lstm, T):
    """q* [B, 2d]; dtype and gradients follow x and the LSTM tensors."""
    B, d = len(sizes), x.shape[1]
    cell = torch.nn.LSTM(2 * d, d).to(x.dtype)          # (its own parameters are never used: functional_call runs it on the caller's)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes, dtype=torch.long))
    state = (x.new_zeros(1, B, d), x.new_zeros(1, B, d))
    q_star = x.new_zeros(B, 2 * d)
    for _ in range(T):
        q, state = torch.func.functional_call(cell, lstm, (q_star.unsqueeze(0), state))
        q = q.view(B, d)
        e = (x * q.index_select(0, batch)).sum(-1)
        top = x.new_full((B,), float("-inf")).scatter_reduce(0, batch, e, "amax", include_self=True)
        p = (e - top.index_select(0, batch)).exp()
        a = p / (x.new_zeros(B).index_add(0, batch, p).index_select(0, batch) + 1e-16)
        r = x.new_zeros(B, d).index_add(0, batch, a.unsqueeze(-1) * x)          # a graph without nodes: r = 0
        q_star = torch.cat([q, r], dim=-1)
    return q_star


def set2set_ref_grads(inp, dtype):
    """(out, {x, weight_ih_l0, ...: gradient}) of sum(out * gout) in `dtype` on the CPU."""
    x = inp.x.detach().clone().to(dtype).requires_grad_(True)
    lstm = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in inp.lstm.items()}
    out = set2set_ref(x, inp.sizes, lstm, inp.T)
    (out * inp.gout.to(dtype)).sum().backward()
    return out.detach(), {"x": x.grad, **{k: v.grad for k, v in lstm.items()}}


def _lin(sd, pfx, x):
    return F.linear(x, sd[pfx + ".weight"], sd[pfx + ".bias"])


def netgine_ref(sd, data):
    """NetGINE.forward (baseline_gin.py:48-61) -> [B, 12]; dtype and gradients follow `sd` (data's float tensors in the same dtype)."""
    x, ea = data.x, data.edge_attr
    for i in range(1, 7):
        p = f"conv{i}"
        e = _lin(sd, p + ".bond_encoder.2", torch.relu(_lin(sd, p + ".bond_encoder.0", ea)))
        a = O.gine_aggregate(x, data.edge_index, e, sd[p + ".eps"])
        x = torch.relu(_lin(sd, p + ".mlp.2", torch.relu(_lin(sd, p + ".mlp.0", a))))
    q = set2set_ref(x, data.sizes, {k: sd["set2set.lstm." + k] for k in LSTM_KEYS}, 6)
    return _lin(sd, "fc4", torch.relu(_lin(sd, "fc1", q)))


def plain_gnn_ref(sd, nlayer, pooling, data, additional_x=None, training=False):
    """GNN.forward (core/model.py:44-79), GINEConv layers, res=True, dropout 0 -> [B, nout].  Train mode: batch statistics, forward value
    only (the running statistics are not touched)."""
    h = O.discrete_encoder(sd, "input_encoder", data.x.squeeze())
    if additional_x is not None:
        h = _lin(sd, "linear", torch.cat([h, additional_x], dim=-1))
    for l in range(nlayer):
        e = O.discrete_encoder(sd, f"edge_encoders.{l}", data.edge_attr)
        u = O.gine_aggregate(h, data.edge_index, e, sd[f"convs.{l}.layer.eps"])
        u = O.plain_mlp(sd, f"convs.{l}.nn", u, 2, False, training)
        h = torch.relu(O._bn_rows(sd, f"norms.{l}", u, training)) + h
    B = data.num_graphs
    pooled = h.new_zeros(B, h.shape[1]).index_add(0, data.batch, h)
    if pooling == "mean":
        size = torch.tensor(data.sizes, dtype=torch.long)
        pooled = pooled / size.clamp(min=1).unsqueeze(-1).to(h.dtype) + F.embedding(size, sd["size_embedder.weight"])
    return O.plain_mlp(sd, "output_encoder", pooled, 2, False, training)


def leaf_state_dict(sd, dtype):
    """Float tensors of a state_dict as `dtype` leaves that record gradients (running statistics included: they get none)."""
    return {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
