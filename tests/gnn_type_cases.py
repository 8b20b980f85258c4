"""Plain-torch restatements (any dtype, differentiable) of the four wrappers of GINESignNetPyG/core/model_utils/pyg_gnn_wrapper.py that
pyg_gnn_types.py builds — GINConv, GCNConv, GATConv (torch_geometric 2.0.1's documented definitions) and SimplifiedPNAConv — of the GNN
around them (core/model.py:44-79), and of the three launches of csrc/simplified_pna.hip; plus the kernel case table of
tests/test_gnn_types_gpu.py and the fixture list of tests/golden/make_gnn_types.py.  tests/test_gnn_types_cpu.py pins the restatements to
the fixtures, i.e. to the reference's own code."""
import types

import torch
import torch.nn.functional as F

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
DEG_VOCAB = 200

# name -> (gnn_type, nhid, nlayer, pooling, additional_x given, graph sizes, seed)
FIXTURES = {
    "gnn_types_gin_h16_l2_add": ("GINConv", 16, 2, "add", False, [5, 9, 1, 7, 3], 71),
    "gnn_types_gcn_h16_l2_add": ("GCNConv", 16, 2, "add", False, [5, 9, 1, 7, 3], 72),
    "gnn_types_gcn_h16_l2_mean": ("GCNConv", 16, 2, "mean", False, [6, 4, 11, 2, 9], 73),
    "gnn_types_gat_h16_l2_add": ("GATConv", 16, 2, "add", False, [5, 9, 1, 7, 3], 74),
    "gnn_types_pna_h16_l2_add": ("SimplifiedPNAConv", 16, 2, "add", False, [5, 9, 1, 7, 3], 75),
    "gnn_types_pna_h16_l2_mean": ("SimplifiedPNAConv", 16, 2, "mean", False, [6, 4, 11, 2, 9], 76),
    "gnn_types_pna_h32_l3_add_pe": ("SimplifiedPNAConv", 32, 3, "add", True, [5, 9, 12, 7, 3], 77),
}


def odd_edges(data):
    """The fixture batches are molecules (symmetric, loop-free); every wrapper treats direction, self loops and multi-edges in its own way
    (GCNConv replaces the loops, GATConv drops them, SimplifiedPNAConv counts them), so a few are added inside the first graph: a
    one-directional edge, a duplicated edge, a self loop and a second self loop on the same node."""
    n0 = data.sizes[0]
    have = set(map(tuple, data.edge_index.t().tolist()))
    a, b = next((a, b) for a in range(n0) for b in range(a + 1, n0) if (a, b) not in have and (b, a) not in have)
    extra = torch.tensor([[a, a, 2 % n0, 2 % n0], [b, b, 2 % n0, 2 % n0]], dtype=torch.long)
    g = torch.Generator().manual_seed(len(data.sizes))
    out = types.SimpleNamespace(**vars(data))
    out.edge_index = torch.cat([data.edge_index, extra], 1).contiguous()
    out.edge_attr = torch.cat([data.edge_attr, torch.randint(1, 4, (extra.shape[1],), generator=g, dtype=torch.long)])
    return out


# ----------------------------------------------------------------------------- the layers
def _lin(sd, pfx, x):
    return F.linear(x, sd[pfx + ".weight"], sd.get(pfx + ".bias"))


def _bn(sd, pfx, x, training, buffers=None):
    """BatchNorm1d over the rows of x.  Train mode: batch statistics; with `buffers` (a dict) the buffers it leaves behind are recorded
    there (momentum 0.1, unbiased variance, num_batches_tracked + 1)."""
    if not training:
        return F.batch_norm(x, sd[pfx + ".running_mean"], sd[pfx + ".running_var"], sd[pfx + ".weight"], sd[pfx + ".bias"], False, 0.0, BN_EPS)
    if x.shape[0] < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {list(x.shape)}")
    if buffers is not None:
        with torch.no_grad():
            buffers[pfx + ".running_mean"] = (1 - BN_MOMENTUM) * sd[pfx + ".running_mean"] + BN_MOMENTUM * x.mean(0)
            buffers[pfx + ".running_var"] = (1 - BN_MOMENTUM) * sd[pfx + ".running_var"] + BN_MOMENTUM * x.var(0, unbiased=True)
            buffers[pfx + ".num_batches_tracked"] = sd[pfx + ".num_batches_tracked"] + 1
    return F.batch_norm(x, None, None, sd[pfx + ".weight"], sd[pfx + ".bias"], True, 0.0, BN_EPS)


def _mlp(sd, pfx, x, training, buffers):
    """MLP(nin, nout, 2, with_final_activation=False) of core/model_utils/elements.py: Linear -> [BatchNorm] -> ReLU -> Linear; norms.1
    exists and is never called."""
    x = _lin(sd, pfx + ".layers.0", x)
    if pfx + ".norms.0.weight" in sd:
        x = _bn(sd, pfx + ".norms.0", x, training, buffers)
    return _lin(sd, pfx + ".layers.1", torch.relu(x))


def _embed(sd, pfx, idx):
    if idx.dim() == 1:
        idx = idx.unsqueeze(1)
    return sum(F.embedding(idx[:, f], sd[f"{pfx}.embeddings.{f}.weight"]) for f in range(idx.shape[1]))


def gin_conv(sd, p, x, ei, e, training, buffers):
    """GINConv(nn, train_eps=True): nn((1 + eps) x_i + sum_{j -> i} x_j); the edge embedding is ignored (pyg_gnn_wrapper.py:15-16)."""
    agg = torch.zeros_like(x).index_add(0, ei[1], x.index_select(0, ei[0])) + (1 + sd[p + ".layer.eps"]) * x
    return _mlp(sd, p + ".nn", agg, training, buffers)


def gcn_norm_dense(ei, N, dtype):
    """D^-1/2 (A + I) D^-1/2 as torch_geometric's gcn_norm builds it from unit weights: the input's self loops are replaced by ONE unit
    loop per node, multi-edges add, and both factors come from the in-degree (the sum over the target index) of A + I.  Dense [N, N],
    row = target."""
    keep = ei[0] != ei[1]
    A = torch.zeros(N, N, dtype=dtype).index_put((ei[1][keep], ei[0][keep]), torch.ones(int(keep.sum()), dtype=dtype), accumulate=True)
    A = A + torch.eye(N, dtype=dtype)
    dis = A.sum(1).pow(-0.5)
    return dis[:, None] * A * dis[None, :]


def gcn_propagate(x, ei):
    """The same operator applied edge by edge (no dense matrix: any N)."""
    N = x.shape[0]
    keep = ei[0] != ei[1]
    s, t = ei[0][keep], ei[1][keep]
    deg = torch.ones(N, dtype=x.dtype).index_add(0, t, torch.ones(s.numel(), dtype=x.dtype))
    dis = deg.pow(-0.5)
    out = torch.zeros_like(x).index_add(0, t, x.index_select(0, s) * dis[s, None]) + x * dis[:, None]
    return out * dis[:, None]


def gcn_conv(sd, p, x, ei, e, training, buffers):
    out = gcn_propagate(F.linear(x, sd[p + ".layer.lin.weight"]), ei)
    return out + sd[p + ".layer.bias"] if p + ".layer.bias" in sd else out


def gat_conv(sd, p, x, ei, e, training, buffers, slope=0.2):
    """GATConv(nin, nout // H, H): x' = lin_src(x) as [N, H, C]; the input's self loops dropped, one loop per node; alpha = softmax over
    every target's edges of leaky_relu(<x'_j, att_src> + <x'_i, att_dst>); out_i = sum_j alpha_ij x'_j, heads concatenated."""
    att_s, att_d = sd[p + ".layer.att_src"], sd[p + ".layer.att_dst"]
    _, H, C = att_s.shape
    N = x.shape[0]
    xs = F.linear(x, sd[p + ".layer.lin_src.weight"]).view(N, H, C)
    keep = ei[0] != ei[1]
    loop = torch.arange(N)
    s, t = torch.cat([ei[0][keep], loop]), torch.cat([ei[1][keep], loop])
    logit = F.leaky_relu((xs * att_s).sum(-1)[s] + (xs * att_d).sum(-1)[t], slope)                       # [E', H]
    top = torch.full((N, H), float("-inf"), dtype=x.dtype).scatter_reduce(0, t[:, None].expand(-1, H), logit.detach(), "amax")
    w = (logit - top[t]).exp()
    w = w / torch.zeros(N, H, dtype=x.dtype).index_add(0, t, w)[t]
    out = torch.zeros(N, H, C, dtype=x.dtype).index_add(0, t, w[:, :, None] * xs[s]).reshape(N, H * C)
    return out + sd[p + ".layer.bias"] if p + ".layer.bias" in sd else out


def pna_conv(sd, p, x, ei, e, training, buffers):
    """SimplifiedPNAConv with aggregators=['mean'] as the reference composes it (pyg_gnn_wrapper.py:68-106): pre_nn on cat[x_i, x_j, e]
    per edge, scatter-mean at the targets, the in-degree embedding beside it, post_nn on cat[x, mean, deg_emb]."""
    N = x.shape[0]
    s, t = ei[0], ei[1]
    msg = _mlp(sd, p + ".pre_nn", torch.cat([x[t], x[s], e], -1), training, buffers)
    deg = torch.zeros(N, dtype=torch.long).index_add(0, t, torch.ones_like(t))
    mean = torch.zeros(N, msg.shape[1], dtype=x.dtype).index_add(0, t, msg) / deg.clamp(min=1)[:, None].to(x.dtype)
    out = torch.cat([x, mean, F.embedding(deg, sd[p + ".deg_embedder.weight"])], -1)
    return _mlp(sd, p + ".post_nn", out, training, buffers)


CONVS = {"GINConv": gin_conv, "GCNConv": gcn_conv, "GATConv": gat_conv, "SimplifiedPNAConv": pna_conv}


def gnn_ref(sd, gnn_type, nlayer, pooling, data, additional_x=None, training=False, buffers=None):
    """GNN.forward (core/model.py:44-79) with res=True, dropout 0 -> [B, nout]; dtype and gradients follow `sd`."""
    conv = CONVS[gnn_type]
    h = _embed(sd, "input_encoder", data.x.squeeze(-1) if data.x.dim() > 1 else data.x)
    if additional_x is not None:
        h = _lin(sd, "linear", torch.cat([h, additional_x], -1))
    for l in range(nlayer):
        e = _embed(sd, f"edge_encoders.{l}", data.edge_attr)
        u = conv(sd, f"convs.{l}", h, data.edge_index, e, training, buffers)
        h = torch.relu(_bn(sd, f"norms.{l}", u, training, buffers)) + h
    pooled = h.new_zeros(data.num_graphs, h.shape[1]).index_add(0, data.batch, h)
    if pooling == "mean":
        size = torch.tensor(data.sizes, dtype=torch.long)
        pooled = pooled / size.clamp(min=1)[:, None].to(h.dtype) + F.embedding(size, sd["size_embedder.weight"])
    return _mlp(sd, "output_encoder", pooled, training, buffers)


def leaf_state_dict(sd, dtype):
    return {k: (v.detach().clone().to(dtype).requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}


# ----------------------------------------------------------------------------- the launches of csrc/simplified_pna.hip
def spna_z(A, B, Q, ei):
    return (A[ei[1]] + B[ei[0]]) + Q


def spna_stats_ref(A, B, Q, ei, gamma, beta, running_mean, running_var):
    """What sn_spna_stats_f32 returns and leaves behind: mean, biased variance, rstd, folded scale / shift, count, moved running stats."""
    z = spna_z(A, B, Q, ei)
    if z.shape[0] < 2:
        raise ValueError("Expected more than 1 value per channel when training")
    mean, var = z.mean(0), z.var(0, unbiased=False)
    rstd = (var + BN_EPS).rsqrt()
    scale = gamma * rstd
    return types.SimpleNamespace(mean=mean, var=var, rstd=rstd, scale=scale, shift=beta - mean * scale, count=z.shape[0],
                                 running_mean=(1 - BN_MOMENTUM) * running_mean + BN_MOMENTUM * mean,
                                 running_var=(1 - BN_MOMENTUM) * running_var + BN_MOMENTUM * z.var(0, unbiased=True))


def spna_mean_ref(A, B, Q, ei, scale, shift):
    """r[i] = mean over i's in-edges of relu(z_e * scale + shift); zeros without in-edges (sn_spna_mean_f32)."""
    N = A.shape[0]
    y = torch.relu(spna_z(A, B, Q, ei) * scale + shift)
    deg = torch.zeros(N, dtype=torch.long).index_add(0, ei[1], torch.ones_like(ei[1]))
    return torch.zeros(N, A.shape[1], dtype=A.dtype).index_add(0, ei[1], y) / deg.clamp(min=1)[:, None].to(A.dtype)


def spna_train_ref(A, B, Q, ei, gamma, beta, dr):
    """Train mode through torch.autograd: r and the gradients of sum(r * dr) w.r.t. A, B, Q, gamma, beta (sn_spna_bwd_f32 with state)."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (A, B, Q, gamma, beta)]
    a, b, q, g, be = leaves
    z = spna_z(a, b, q, ei)
    y = torch.relu(F.batch_norm(z, None, None, g, be, True, 0.0, BN_EPS))
    N = A.shape[0]
    deg = torch.zeros(N, dtype=torch.long).index_add(0, ei[1], torch.ones_like(ei[1]))
    r = torch.zeros(N, A.shape[1], dtype=A.dtype).index_add(0, ei[1], y) / deg.clamp(min=1)[:, None].to(A.dtype)
    (r * dr).sum().backward()
    return r.detach(), dict(zip(("dA", "dB", "dQ", "dgamma", "dbeta"), (t.grad for t in leaves)))


def spna_eval_ref(A, B, Q, ei, scale, shift, dr):
    """Eval mode (folded scale / shift): r and the gradients w.r.t. A, B, Q (sn_spna_bwd_f32 without state)."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (A, B, Q)]
    r = spna_mean_ref(*leaves, ei, scale, shift)
    (r * dr).sum().backward()
    return r.detach(), dict(zip(("dA", "dB", "dQ"), (t.grad for t in leaves)))


# ----------------------------------------------------------------------------- kernel cases
def kernel_graph(kind):
    """(edge_index [2, E] int64, batch [N] int64, number of graphs) of the kernel tests.
    'degrees': two graphs in one batch; in the first (70 nodes) node 0 has in-degree 0, node 1 one in-edge, node 2 64, node 3 65 and node
    4 130 in-edges (every source twice: multi-edges), node 5 two self loops; the second is a 9-ring in both directions with a self loop.
    The edge list is shuffled, so no node's in-edges are contiguous in it."""
    if kind == "degrees":
        e = [(10, 1)]
        e += [(j, 2) for j in range(3, 67)]                     # 64
        e += [(j, 3) for j in range(4, 69)]                     # 65
        e += [(j, 4) for j in range(5, 70)] * 2                 # 130
        e += [(5, 5), (5, 5)]
        e += [(70 + i, 70 + (i + 1) % 9) for i in range(9)] + [(70 + (i + 1) % 9, 70 + i) for i in range(9)] + [(73, 73)]
        ei = torch.tensor(e, dtype=torch.long).t().contiguous()
        ei = ei[:, torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(3))].contiguous()
        return ei, torch.cat([torch.zeros(70, dtype=torch.long), torch.ones(9, dtype=torch.long)]), 2
    if kind == "n1_e2":                                         # one node, two self loops: the smallest train-mode case
        return torch.zeros(2, 2, dtype=torch.long), torch.zeros(1, dtype=torch.long), 1
    if kind == "n1_e0":
        return torch.zeros(2, 0, dtype=torch.long), torch.zeros(1, dtype=torch.long), 1
    if kind == "n2_e1":
        return torch.tensor([[0], [1]], dtype=torch.long), torch.zeros(2, dtype=torch.long), 1
    if kind == "n3_e2":
        return torch.tensor([[0, 2], [1, 1]], dtype=torch.long), torch.zeros(3, dtype=torch.long), 1
    raise KeyError(kind)


# name -> (graph, C, row stride of every matrix (0: C), 4-byte-offset pointers, modes run)
KERNEL_CASES = {
    "c12": ("degrees", 12, 0, False, ("eval", "train")),
    "c12_offset": ("degrees", 12, 0, True, ("eval", "train")),            # the pointers force the scalar path at a C that is a multiple of 4
    "c12_ld13": ("degrees", 12, 13, False, ("eval", "train")),            # the row stride does
    "c15": ("degrees", 15, 0, False, ("eval", "train")),
    "c48": ("degrees", 48, 0, False, ("eval", "train")),
    "c48_ld64": ("degrees", 48, 64, False, ("eval", "train")),            # vector path with padded rows
    "c384": ("degrees", 384, 0, False, ("eval", "train")),
    "c384_offset": ("degrees", 384, 0, True, ("train",)),                 # scalar path, two column chunks
    "n1_e2": ("n1_e2", 12, 0, False, ("eval", "train")),
    "n3_e2": ("n3_e2", 15, 0, False, ("eval", "train")),
    "n1_e0": ("n1_e0", 12, 0, False, ("eval",)),
    "n2_e1": ("n2_e1", 12, 0, False, ("eval",)),                          # (train mode raises: its own test)
}


def kernel_inputs(name, dtype=torch.float32):
    """Operands of one kernel case on the host, contiguous; the GPU test lays them out with the case's stride and offset."""
    kind, C, ld, offset, modes = KERNEL_CASES[name]
    ei, batch, B = kernel_graph(kind)
    N, E = batch.numel(), ei.shape[1]
    g = torch.Generator().manual_seed(1000 + C + N)
    r = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return types.SimpleNamespace(name=name, C=C, ld=ld or C, offset=offset, modes=modes, ei=ei, batch=batch, B=B, N=N, E=E,
                                 A=r(N, C).to(dtype), B_=r(N, C).to(dtype), Q=r(E, C).to(dtype), dr=r(N, C).to(dtype),
                                 gamma=(1 + 0.2 * r(C)).to(dtype), beta=(0.1 * r(C)).to(dtype),
                                 running_mean=(0.1 * r(C)).to(dtype), running_var=(torch.rand(C, generator=g) + 0.5).to(dtype))


def expected_path(name):
    """('vector' | 'scalar', column chunks of the reduction launches) — the dispatch the case is in the table for."""
    _, C, ld, offset, _ = KERNEL_CASES[name]
    vector = C % 4 == 0 and (ld or C) % 4 == 0 and not offset
    G = C // 4 if vector else C
    return ("vector" if vector else "scalar"), -(-G // 256)
