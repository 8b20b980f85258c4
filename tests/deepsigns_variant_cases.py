"""Shared by tests/test_deepsigns_variants_cpu.py and tests/test_deepsigns_variants_gpu.py: the case tables and CPU restatements
(float32 / float64, differentiable) of what the 'gcn' and 'transformer' sign-invariant nets of the DGL tree add —

  gcn_propagate_ref        dgl.nn.pytorch.GraphConv(norm='both') without its weight, from DGL's published definition (index ops)
  gcn_dense_operator       the same as a dense float64 matrix D_in^-1/2 A D_out^-1/2 (an independent second form)
  graph_attention_ref      the SetAttentionBlock's multi-head attention over the nodes of each graph, per slot, graph by graph
  gcn_deepsigns_ref        layers/deepsigns.py:13-31 GCNDeepSigns from a reference-keyed state_dict
  transformer_deepsigns_ref  layers/deepsigns.py:89-119 TransformerDeepSigns from a reference-keyed state_dict

The fixtures (tests/golden/ds_gcn_*.npz, ds_tf_*.npz: the reference's own modules, tests/golden/make_deepsigns_variants.py) pin the
restatements in the CPU test; the GPU test then compares the kernels and modules with them in float64.
"""
import math
import types

import torch
import torch.nn.functional as F

GCN_CASES = ["ds_gcn_h16_c4_l3_k4", "ds_gcn_h19_c3_l2_k5", "ds_gcn_h8_c12_l4_k6"]
TF_CASES = ["ds_tf_h16_l2_k3", "ds_tf_h15_l3_k4", "ds_tf_h24_l4_k6"]
CLASSES = {**{c: "GCNDeepSigns" for c in GCN_CASES}, **{c: "TransformerDeepSigns" for c in TF_CASES}}

# ----------------------------------------------------------------------------- propagation: graphs, widths, layouts
# 9 nodes, directed: in-degree != out-degree on six of them, the edge 0 -> 1 twice, a self loop at 2, node 7 without out-edges, node 8 without
# in-edges (at op level its row is the bias)
_DIRECTED = ([0, 0, 2, 3, 4, 5, 5, 6, 8, 1, 3, 8, 2], [1, 1, 2, 1, 3, 4, 7, 7, 0, 5, 6, 2, 7])


def prop_graph(name):
    """(N, src, dst) int64."""
    if name == "directed":
        return 9, torch.tensor(_DIRECTED[0]), torch.tensor(_DIRECTED[1])
    if name == "no_edges":
        return 5, torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=torch.long)
    if name == "n300":                      # more than one workgroup of 256 outputs at every width
        g = torch.Generator().manual_seed(300)
        return 300, torch.randint(0, 300, (1100,), generator=g), torch.randint(0, 300, (1100,), generator=g)
    raise KeyError(name)


PROP_GRAPHS = ["directed", "no_edges", "n300"]
PROP_WIDTHS = [1, 6, 8, 76]              # scalar, scalar (not a multiple of 4), one vector, 19 vectors
PROP_LAYOUTS = ["contiguous", "strided", "offset"]      # rows of a wider matrix; a view one float into a buffer (not 16-byte aligned)

# ----------------------------------------------------------------------------- attention: one batch, every size class
ATT_SIZES = [1, 2, 5, 64, 65, 130, 0]      # one node, under a tile, the tile, one past it, three tiles, an empty graph
ATT_SLOTS = [1, 3]
ATT_HEADS = 2
ATT_WIDTHS = [7, 8, 47, 64]
ATT_LAYOUTS = ["packed", "offset"]          # column blocks of one [R, 3 * heads * dh] projection; the same, one float into a buffer


def gcn_norms(src, dst, N, dtype):
    """(cout [N], cin [N]): clamp(out-/in-degree, 1)^-1/2."""
    dout = torch.bincount(src, minlength=N).to(dtype).clamp(min=1)
    din = torch.bincount(dst, minlength=N).to(dtype).clamp(min=1)
    return dout.pow(-0.5), din.pow(-0.5)


def gcn_propagate_ref(x, src, dst, bias=None):
    """x [N, ...]: cin_i * sum_{j -> i} cout_j x_j (+ bias over the last axis); dtype and gradients follow x."""
    N = x.shape[0]
    cout, cin = gcn_norms(src, dst, N, x.dtype)
    shp = (N,) + (1,) * (x.dim() - 1)
    h = x * cout.reshape(shp)
    out = torch.zeros_like(h).index_add(0, dst, h.index_select(0, src)) * cin.reshape(shp)
    return out if bias is None else out + bias


def gcn_dense_operator(src, dst, N):
    """D_in^-1/2 A D_out^-1/2 as a dense float64 [N, N] matrix (A[i, j] = number of edges j -> i)."""
    A = torch.zeros(N, N, dtype=torch.float64)
    A.index_put_((dst, src), torch.ones(src.numel(), dtype=torch.float64), accumulate=True)
    cout, cin = gcn_norms(src, dst, N, torch.float64)
    return cin[:, None] * A * cout[None, :]


def graph_attention_ref(q, k, v, sizes, S, heads, want_lse=False):
    """q, k, v [N*S, heads*dh] (rows node * S + slot) -> softmax_j(q_i . k_j / sqrt(dh)) v_j over the nodes j of i's graph, per slot
    and head; dtype and gradients follow the inputs.  want_lse: also the rows' log-sum-exp [N*S, heads]."""
    N = sum(sizes)
    D = q.shape[1]
    dh = D // heads
    q4, k4, v4 = (t.reshape(N, S, heads, dh) for t in (q, k, v))
    outs, lses, o = [], [], 0
    for n in sizes:
        if n:
            e = torch.einsum("xshd,yshd->shxy", q4[o:o + n], k4[o:o + n]) / math.sqrt(dh)
            outs.append(torch.einsum("shxy,yshd->xshd", torch.softmax(e, dim=-1), v4[o:o + n]))
            lses.append(torch.logsumexp(e, dim=-1).permute(2, 0, 1))
        o += n
    out = torch.cat(outs, 0).reshape(N * S, D) if outs else q.new_zeros(0, D)
    return (out, torch.cat(lses, 0).reshape(N * S, heads)) if want_lse else out


# ----------------------------------------------------------------------------- the modules
def params(fx):
    hidden, out, layers, k = (int(v) for v in fx.meta["params"])
    return types.SimpleNamespace(hidden=hidden, out=out, layers=layers, k=k, cls=str(fx.meta["cls"]))


def _bn(sd, pfx, x, training, buffers):
    """BatchNorm1d on [N, K, C] (the reference transposes to [N, C, K]: statistics over the N*K rows) or [N, C].  training: batch
    statistics, and — when `buffers` (a dict) is given — the running statistics in it move as nn.BatchNorm1d moves them."""
    w, b = sd[pfx + ".weight"], sd[pfx + ".bias"]
    rows = x.reshape(-1, x.shape[-1])
    if not training:
        rm, rv = sd[pfx + ".running_mean"].to(x.dtype), sd[pfx + ".running_var"].to(x.dtype)
        return (x - rm) / torch.sqrt(rv + 1e-5) * w + b
    mean, var = rows.mean(0), rows.var(0, unbiased=False)
    if buffers is not None:
        n = rows.shape[0]
        rm = buffers.get(pfx + ".running_mean", sd[pfx + ".running_mean"]).to(x.dtype)
        rv = buffers.get(pfx + ".running_var", sd[pfx + ".running_var"]).to(x.dtype)
        buffers[pfx + ".running_mean"] = (0.9 * rm + 0.1 * mean).detach()
        buffers[pfx + ".running_var"] = (0.9 * rv + 0.1 * var * n / max(n - 1, 1)).detach()
        buffers[pfx + ".num_batches_tracked"] = buffers.get(pfx + ".num_batches_tracked", sd[pfx + ".num_batches_tracked"]) + 1
    return (x - mean) / torch.sqrt(var + 1e-5) * w + b


def mlp_ref(sd, pfx, x, n_lins, training, buffers):
    """layers/mlp.py:37-56 with use_bn, relu, dropout 0."""
    for i in range(n_lins - 1):
        x = torch.relu(F.linear(x, sd[f"{pfx}.lins.{i}.weight"], sd[f"{pfx}.lins.{i}.bias"]))
        x = _bn(sd, f"{pfx}.bns.{i}", x, training, buffers)
    return F.linear(x, sd[f"{pfx}.lins.{n_lins - 1}.weight"], sd[f"{pfx}.lins.{n_lins - 1}.bias"])


def _n_lins(sd, pfx):
    return len({k.split(".")[len(pfx.split(".")) + 1] for k in sd if k.startswith(pfx + ".lins.")})


def gcn_ref(sd, src, dst, x, training, buffers):
    """GCN.forward (layers/gnns.py:33-45) on [N, K, c]; GraphConv applies its weight first where in > out."""
    L = len({k.split(".")[2] for k in sd if k.startswith("enc.layers.")})
    for l in range(L):
        if l:
            x = _bn(sd, f"enc.bns.{l - 1}", x, training, buffers)
        W, b = sd[f"enc.layers.{l}.weight"], sd[f"enc.layers.{l}.bias"]
        if W.shape[0] > W.shape[1]:
            x = gcn_propagate_ref(torch.matmul(x, W), src, dst, b)
        else:
            N = x.shape[0]
            cout, cin = gcn_norms(src, dst, N, x.dtype)
            h = x * cout.reshape(N, 1, 1)
            a = torch.zeros_like(h).index_add(0, dst, h.index_select(0, src))
            x = torch.matmul(a, W) * cin.reshape(N, 1, 1) + b
        if l < L - 1:
            x = torch.relu(x)
    return x


def gcn_deepsigns_ref(sd, k, src, dst, x, training=False, buffers=None):
    """GCNDeepSigns.forward (layers/deepsigns.py:25-31): x [N, k, 1] -> [N, k, 1]."""
    z = gcn_ref(sd, src, dst, x, training, buffers) + gcn_ref(sd, src, dst, -x, training, buffers)
    y = mlp_ref(sd, "rho", z.reshape(z.shape[0], -1), _n_lins(sd, "rho"), training, buffers)
    return y.reshape(x.shape[0], k, 1)


def set_transformer_ref(sd, sizes, feat, heads=2):
    """SetTransformerEncoder.forward on one slot: feat [N, d_model]."""
    L = len({k.split(".")[2] for k in sd if k.startswith("enc.layers.")})
    for l in range(L):
        p = f"enc.layers.{l}.mha."
        q, k, v = (F.linear(feat, sd[p + f"proj_{n}.weight"]) for n in "qkv")
        att = graph_attention_ref(q, k, v, sizes, 1, heads)
        feat = F.layer_norm(feat + F.linear(att, sd[p + "proj_o.weight"]), feat.shape[-1:], sd[p + "norm_in.weight"], sd[p + "norm_in.bias"], 1e-5)
        f = F.linear(torch.relu(F.linear(feat, sd[p + "ffn.0.weight"], sd[p + "ffn.0.bias"])), sd[p + "ffn.3.weight"], sd[p + "ffn.3.bias"])
        feat = F.layer_norm(feat + f, feat.shape[-1:], sd[p + "norm_inter.weight"], sd[p + "norm_inter.bias"], 1e-5)
    return feat


def transformer_deepsigns_ref(sd, k, sizes, x, training=False, buffers=None):
    """TransformerDeepSigns.forward (layers/deepsigns.py:108-119): x [N, k, 1] -> [N, k, 1], slot by slot as the reference."""
    xp = F.linear(x, sd["embed.weight"], sd["embed.bias"])
    xm = F.linear(-x, sd["embed.weight"], sd["embed.bias"])
    xs = [set_transformer_ref(sd, sizes, xp[:, i]) + set_transformer_ref(sd, sizes, xm[:, i]) for i in range(k)]
    y = mlp_ref(sd, "rho", torch.cat(xs, dim=1), _n_lins(sd, "rho"), training, buffers)
    return y.reshape(x.shape[0], k, 1)


def module_ref(fx, dtype, training=False, buffers=None, grads=False):
    """The fixture's module restated in `dtype` on the fixture's batch -> y, or (y, {parameter: gradient}) for the fixture's cotangent
    (train mode) when grads."""
    p = params(fx)
    sd = {k: (v.detach().clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in fx.sd.items()}
    if grads:
        for k_, v in sd.items():
            if v.is_floating_point() and not k_.endswith(("running_mean", "running_var")):
                v.requires_grad_(True)
    x = fx.inp["pos_enc"].to(dtype).unsqueeze(-1)
    ei = fx.inp["edge_index"]
    if p.cls == "GCNDeepSigns":
        y = gcn_deepsigns_ref(sd, p.k, ei[0], ei[1], x, training, buffers)
    else:
        y = transformer_deepsigns_ref(sd, p.k, [int(s) for s in fx.inp["sizes"]], x, training, buffers)
    if not grads:
        return y.detach()
    (y * fx.inp["cotangent"].to(dtype)).sum().backward()
    return y.detach(), {k_: v.grad for k_, v in sd.items() if v.requires_grad and v.grad is not None}


def build(fx, device=None):
    """The package's module of a fixture with the fixture's (reference-keyed) state_dict loaded."""
    from signnet_basisnet_amd import dgl_deepsigns as DS
    p = params(fx)
    net = getattr(DS, p.cls)(1, p.hidden, p.out, p.layers, p.k, use_bn=True, dropout=0.0, activation="relu")
    net.load_state_dict(fx.sd)
    return net if device is None else net.to(device)
