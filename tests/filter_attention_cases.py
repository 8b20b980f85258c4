"""Shared by tests/test_filter_attention_cpu.py and tests/test_filter_attention_gpu.py: float64 restatements, on DENSE matrices built from
the definitions, of what GatNet and ARMANet compute, the attention kernel's dispatch table, and the graphs of its tests.

  gat_conv_ref    PyG's GATConv behind its Linear: input self loops dropped, one loop per node, multi-edges counted as often as they occur;
                  e_ij = leaky_relu(f_j . att_l + f_i . att_r), softmax over j (a dense [N, N] count matrix carries the multiplicities),
                  out_i = act(sum_j a_ij f_j + bias)
  dense_arma      gcn_norm(..., add_self_loops=False): every input edge kept (self loops ordinary entries), degree over the target index
  arma_conv_ref   ARMAConv(in, out, 1, 1, False): relu(S (x W_init) + x W_root + b)
  net_ref         GatNet / ARMANet forward from a reference-keyed state_dict (differentiable, any dtype)

Messages go from edge_index[0] to edge_index[1].
"""
import os

import numpy as np
import torch

import filter_cases as FC

# ----------------------------------------------------------------------------- the kernel's dispatch table (csrc/filter_attention.hip)
MAX_HEADS, MAX_C = 16, 128                      # sn_gat_conv_max_heads / sn_gat_conv_max_channels
GROUP_WIDTH_STEPS = (1, 2, 4, 8, 16, 32, 64)    # C at which the group of lanes that owns one (node, head) reaches its next width
TWO_CHANNELS_ABOVE = 64                         # C > 64: a lane carries two channels
IN_DEGREE_THRESHOLDS = ()                       # none: a group walks its row serially with an online softmax, whatever the in-degree
BWD_MAX_BLOCKS = 512                            # rows of the parameter-partials block; more chunks of items than this are strided


def group_width(C):
    """min(64, the power of two >= C)."""
    w = 1
    while w < C and w < 64:
        w *= 2
    return w


def bwd_blocks(N, heads, C):
    chunks = -(-N * heads // (256 // group_width(C)))
    return min(chunks, BWD_MAX_BLOCKS)


# (heads, C) pairs of the kernel test: group widths 1, 8, 8 (ragged), 32, 64 (ragged, C = 33), 16 and 64 with two channels per lane
SHAPES = ((1, 1), (4, 8), (3, 5), (1, 32), (2, 33), (8, 16), (16, 128))
# the thresholds of the table those leave out: group widths 2 and 4 (the second ragged), and a ragged second channel (64 < C < 128: some
# lanes of the group carry one channel, some two)
EXTRA_SHAPES = ((1, 2), (2, 3), (2, 65))


def _star():
    """One hub (node 0) with 300 in-edges from distinct leaves, 5 of them given twice, and an input self loop on the hub."""
    leaves = np.arange(1, 301)
    src = np.concatenate([leaves, leaves[:5], [0]])
    dst = np.zeros_like(src)
    return np.stack([src, dst]), 301


GRAPHS = dict(FC.GRAPHS, star=_star())
KERNEL_GRAPHS = FC.SMALL + ("ring1030", "star")
# ((heads, C), act) on the two large graphs: every pair exactly once between them, both activations on each
LARGE_SHAPES = {"ring1030": (((1, 1), 1), ((4, 8), 0), ((2, 33), 1), ((16, 128), 0)),
                "star": (((3, 5), 1), ((1, 32), 0), ((8, 16), 1))}


# ----------------------------------------------------------------------------- dense float64 restatements
def dense_counts(ei, N, dtype=torch.float64):
    """M[i, j] = how often j -> i occurs among the edges without the input self loops, + 1 on the diagonal (the one loop per node)."""
    ei = torch.as_tensor(np.asarray(ei)).long().reshape(2, -1)
    M = torch.eye(N, dtype=dtype)
    for s, t in ei.t().tolist():
        if s != t:
            M[t, s] += 1.0
    return M


def gat_conv_ref(feat, att_l, att_r, bias, M, heads, act, slope=0.2):
    """feat [N, heads * C] (the Linear's output), M = dense_counts.  act: 0 none, 1 ELU."""
    N = feat.shape[0]
    f = feat.reshape(N, heads, -1)
    al = (f * att_l.reshape(1, heads, -1)).sum(-1)                         # [N, heads], the source term
    ar = (f * att_r.reshape(1, heads, -1)).sum(-1)
    e = torch.nn.functional.leaky_relu(al.unsqueeze(0) + ar.unsqueeze(1), slope)          # [i, j, h]
    mask = (M > 0).unsqueeze(-1)
    top = torch.where(mask, e, torch.full_like(e, float("-inf"))).amax(1, keepdim=True)
    p = torch.where(mask, (e - top).exp(), torch.zeros_like(e)) * M.unsqueeze(-1).to(e.dtype)
    a = p / p.sum(1, keepdim=True)
    out = torch.einsum("ijh,jhc->ihc", a, f).reshape(N, -1)
    if bias is not None:
        out = out + bias.reshape(-1)
    return torch.nn.functional.elu(out) if act else out


def gat_lse_ref(feat, att_l, att_r, M, heads, slope=0.2):
    N = feat.shape[0]
    f = feat.reshape(N, heads, -1)
    al = (f * att_l.reshape(1, heads, -1)).sum(-1)
    ar = (f * att_r.reshape(1, heads, -1)).sum(-1)
    e = torch.nn.functional.leaky_relu(al.unsqueeze(0) + ar.unsqueeze(1), slope)
    e = torch.where((M > 0).unsqueeze(-1), e + M.clamp_min(1e-300).log().unsqueeze(-1).to(e.dtype), torch.full_like(e, float("-inf")))
    return torch.logsumexp(e, 1)


def gat_conv_edges(feat, att_l, att_r, bias, ei, N, heads, act, slope=0.2):
    """The same layer over the edge list (for graphs too large for the dense form; the CPU test holds the two against each other):
    -> (out, lse [N, heads])."""
    ei = torch.as_tensor(np.asarray(ei)).long().reshape(2, -1)
    keep = ei[0] != ei[1]
    loop = torch.arange(N)
    src, dst = torch.cat([ei[0][keep], loop]), torch.cat([ei[1][keep], loop])
    f = feat.reshape(N, heads, -1)
    al = (f * att_l.reshape(1, heads, -1)).sum(-1)
    ar = (f * att_r.reshape(1, heads, -1)).sum(-1)
    e = torch.nn.functional.leaky_relu(al[src] + ar[dst], slope)
    top = torch.full((N, heads), float("-inf"), dtype=e.dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, heads), e.detach(), "amax")
    p = (e - top[dst]).exp()
    den = torch.zeros(N, heads, dtype=e.dtype).index_add(0, dst, p)
    out = torch.zeros(N, heads, f.shape[-1], dtype=e.dtype).index_add(0, dst, (p / den[dst]).unsqueeze(-1) * f[src]).reshape(N, -1)
    if bias is not None:
        out = out + bias.reshape(-1)
    return (torch.nn.functional.elu(out) if act else out), (top + den.log()).detach()


def dense_arma(ei, N, dtype=torch.float64):
    ei = torch.as_tensor(np.asarray(ei)).long().reshape(2, -1)
    A = torch.zeros(N, N, dtype=dtype)
    for s, t in ei.t().tolist():
        A[t, s] += 1.0                               # self loops stay
    deg = A.sum(1)                                   # over the target index
    dis = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    return dis[:, None] * A * dis[None, :]


def arma_conv_ref(x, S, init_weight, root_weight, bias):
    return torch.relu(S @ (x @ init_weight[0]) + x @ root_weight[0, 0] + bias.reshape(-1))


def net_ref(name, sd, x, ei, N):
    dt = x.dtype
    sd = {k: v.to(dt) for k, v in sd.items()}
    h = x
    layers = FC._n_layers(sd, "convs")
    if name == "GatNet":
        M = dense_counts(ei, N, dt)
        for i in range(layers):
            att_l = sd[f"convs.{i}.att_l"]
            f = h @ sd[f"convs.{i}.lin_l.weight"].t()
            h = gat_conv_ref(f, att_l, sd[f"convs.{i}.att_r"], sd[f"convs.{i}.bias"], M, att_l.shape[1], 1)
    elif name == "ARMANet":
        S = dense_arma(ei, N, dt)
        for i in range(layers):
            h = torch.relu(arma_conv_ref(h, S, sd[f"convs.{i}.init_weight"], sd[f"convs.{i}.root_weight"], sd[f"convs.{i}.bias"]))
    else:
        raise ValueError(name)
    return h @ sd["fc2.weight"].t() + sd["fc2.bias"]


ALIASED = ("lin_r.weight",)                          # GATConv.lin_r is lin_l: one parameter under two state_dict keys


def net_ref_training(name, sd, feat, ei, N, y, m, lr=0.01, steps=4, dtype=torch.float64):
    """(prediction, first-step gradients, losses of `steps` Adam steps) of the restatement: training.py:132-143 with torch.optim.Adam.
    The aliased key shares its partner's parameter; a parameter without a gradient (ARMAConv.weight) has no entry."""
    params = {k: torch.nn.Parameter(v.detach().clone().to(dtype)) for k, v in sd.items() if not k.endswith(ALIASED)}
    full = lambda: dict(params, **{k: params[k.replace("lin_r", "lin_l")] for k in sd if k.endswith(ALIASED)})      # noqa: E731
    feat, y, m = feat.to(dtype), y.to(dtype), m.to(dtype)
    with torch.no_grad():
        pre = net_ref(name, full(), feat, ei, N).clone()
    opt = torch.optim.Adam(params.values(), lr=lr)
    losses, grads = [], {}
    for step in range(steps):
        opt.zero_grad()
        loss = torch.square(m * (net_ref(name, full(), feat, ei, N) - y)).sum()
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().clone() for k, p in params.items() if p.grad is not None}
        opt.step()
        losses.append(float(loss.detach()))
    return pre, grads, torch.tensor(losses, dtype=torch.float64)


NET_CASES = ("gatnet", "gatnet_eig_abs", "armanet")
_FIXTURE = None


def fixture():
    """tests/golden/filter_attention_grid6.npz (make_filter_attention.py), loaded once: golden_util.load_filters' layout plus `restated`,
    `edge_index` and `N`."""
    global _FIXTURE
    if _FIXTURE is None:
        import golden_util as G
        fx = G.load_filters("filter_attention_grid6")
        z = np.load(os.path.join(G.GOLDEN, "filter_attention_grid6.npz"), allow_pickle=False)
        fx.restated = tuple(str(s) for s in z["meta/restated"])
        fx.edge_index = fx.inp["edge_index"].long()
        fx.N = fx.side * fx.side
        _FIXTURE = fx
    return _FIXTURE


_REF64 = {}


def fixture_ref64(case):
    """The float64 restatement of one fixture case, computed once and shared."""
    if case not in _REF64:
        fx = fixture()
        c = fx.cases[case]
        _REF64[case] = net_ref_training(c["args"]["net"], c["sd"], c["feat"], fx.edge_index, fx.N, fx.inp["y"][:, 0:1], fx.inp["m"],
                                        lr=c["args"]["lr"])
    return _REF64[case]
