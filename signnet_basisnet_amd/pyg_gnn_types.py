"""The plain GNN of GINESignNetPyG for every `model.gnn_type` (train/zinc.py:31-46: for anything but 'SignNet' the script builds
`GNN(None, None, nhid, 1, nlayer, gnn_type, dropout, pool, res=True)`, core/model.py:9-79) over the five wrappers of
core/model_utils/pyg_gnn_wrapper.py: GINEConv (pyg.GNN, unchanged), GINConv, GCNConv, GATConv and SimplifiedPNAConv.

The four wrappers keep the reference's constructors and the `state_dict` keys it produces over torch_geometric 2.0.1 (restated from
that release's documented modules; PyG is not a dependency):

  GINConv            nn.layers.{0,1}.{weight,bias} (MLP(..., with_norm=False): both Linears keep their bias, no BatchNorm), the same
                     MLP a second time under layer.nn.*, layer.eps.  edge_attr is ignored (:15-16).
  GCNConv            layer.lin.weight (+ layer.bias when bias=True; GNN passes bias=not bn, so never here).
  GATConv            layer.att_src, layer.att_dst [1, heads, out], layer.lin_src.weight and its alias layer.lin_dst.weight.
  SimplifiedPNAConv  pre_nn.*, post_nn.* (MLP: layers.{0,1}, norms.{0,1} — norms.1 is registered and never called), deg_embedder.weight.

Launches per layer (eval; the train forward puts a statistics launch in front of every BatchNorm):
  GINConv   sn_gin_aggregate_f32, Linear+ReLU, Linear with the layer's BatchNorm, ReLU and residual in its epilogue
  GCNConv   sn_gcn_pyg_propagate_f32 (PyG's normalisation, csrc/pyg_gcn.hip), then ONE GEMM with BatchNorm, ReLU and residual folded in:
            D^-1/2 (A+I) D^-1/2 (x W^T) = (D^-1/2 (A+I) D^-1/2 x) W^T, so the propagation runs first
  GATConv   Linear, sn_gat_conv_f32 (act none, bias NULL) on the batch's CSR without the input self loops, BatchNorm+ReLU+residual
  SimplifiedPNAConv   A|B = x [W1[:, :d]; W1[:, d:2d]]^T in one GEMM, Q = e W1[:, 2d:]^T, sn_spna_mean_f32 (train: sn_spna_stats_f32 in
            front), the W2 GEMM on the [N, 3d] mean with rows of in-degree 0 written as zero, the degree embedding, then post_nn as two
            GEMMs over cat[x, W2-mean, deg_emb] (one 384-wide GEMM at d = 128: sn_masked_linear_f32 has no width limit)

dropout > 0 (core/model.py:65): wired as in pyg.GNN (site = the layer, between the ReLU and the residual) and, as there, refused by this
class; dropout_models.GNN is the subclass that takes it.
Not built, as in pyg.GNN: res=False, bn=False, dos_bins > 0; SimplifiedPNAConv with aggregators other than ['mean'] (GNN
cannot reach them) or nhid > 128.  Training: the eager step, or train_graph.BucketedStep (one captured step per capacity bucket;
the differentiable forward reads the padded batch's validity vectors under the switch `_bucket`).

Structure: the forwards are pyg.GNN's, written once per mode — input head, the residual-or-dropout frame around every layer, readout,
status hand-over.  GNN below adds the conv wrappers and overrides pyg.GNN's two hooks, `_conv_value(c, ea)` (eval / train value
without autograd) and `_conv_grad(c, ea)` (differentiable): each runs, per conv type, what that type needs once per forward — the
edge-id range check of the edge-blind convs, GCN's coefficients, GAT's operator pair, PNA's degrees — and returns the per-layer body
`layer(li, h, res) -> h` over the context `c` (plans, status word, validity vectors and the Linear/BatchNorm links of that mode:
pyg._ValueCtx / pyg._GradCtx).  'GINEConv' goes to pyg.GNN's own hooks.  A new conv type is one branch in each of the two hooks.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import autograd as AG
from . import ops
from . import pyg as _pyg
from .filter_baselines import _glorot, _operator_pair
from .pyg import MLP, DiscreteEncoder, GINEConv, _GINEps

GNN_TYPES = ("GINEConv", "GINConv", "GCNConv", "GATConv", "SimplifiedPNAConv")
PNA_MAX_HIDDEN = ops.SPNA_MAX_CHANNELS // 3          # 128: C = 3 * nhid channels per edge row
DEG_VOCAB = 200                                      # pyg_gnn_wrapper.py:61


class GINConv(nn.Module):
    def __init__(self, nin, nout, bias=True):
        super().__init__()
        self.nn = MLP(nin, nout, 2, False, bias=bias, with_norm=False)      # pyg_gnn_wrapper.py:10 ("Do not use BN")
        self.layer = _GINEps(self.nn)

    def reset_parameters(self):
        self.nn.reset_parameters()
        self.layer.reset_parameters()


class _GCNLayer(nn.Module):
    def __init__(self, nin, nout, bias):
        super().__init__()
        self.lin = nn.Linear(nin, nout, bias=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros(nout))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)


class GCNConv(nn.Module):
    def __init__(self, nin, nout, bias=True):
        super().__init__()
        self.layer = _GCNLayer(nin, nout, bias)

    def reset_parameters(self):
        self.layer.reset_parameters()


class _GATLayer(nn.Module):
    def __init__(self, nin, nout, heads, bias):
        super().__init__()
        self.heads, self.out_channels, self.negative_slope = heads, nout, 0.2
        self.lin_src = nn.Linear(nin, heads * nout, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = nn.Parameter(torch.empty(1, heads, nout))
        self.att_dst = nn.Parameter(torch.empty(1, heads, nout))
        if bias:
            self.bias = nn.Parameter(torch.zeros(heads * nout))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin_src.weight)
        _glorot(self.att_src)
        _glorot(self.att_dst)
        if self.bias is not None:
            nn.init.zeros_(self.bias)


class GATConv(nn.Module):
    def __init__(self, nin, nout, bias=True, nhead=1):
        super().__init__()
        mh, mc = 16, 128            # sn_gat_conv_max_heads / sn_gat_conv_max_channels (checked against the library in forward)
        if nhead < 1 or nout % nhead:
            raise ValueError(f"GATConv: nout = {nout} is not a multiple of nhead = {nhead}")
        if nhead > mh or nout // nhead > mc:
            raise ValueError(f"GATConv: nhead = {nhead}, {nout // nhead} channels per head is beyond the kernel's limits ({mh}, {mc})")
        self.layer = _GATLayer(nin, nout // nhead, nhead, bias)

    def reset_parameters(self):
        self.layer.reset_parameters()


class SimplifiedPNAConv(nn.Module):
    def __init__(self, nin, nout, bias=True, aggregators=("mean",), **kwargs):
        super().__init__()
        if list(aggregators) != ["mean"]:
            raise NotImplementedError(f"SimplifiedPNAConv: only aggregators=['mean'] is built on the HIP path (got {list(aggregators)!r})")
        if kwargs:
            raise NotImplementedError(f"SimplifiedPNAConv: MessagePassing options {sorted(kwargs)} are not built on the HIP path")
        if nin != nout:
            raise NotImplementedError("SimplifiedPNAConv: nin != nout is not built on the HIP path (GNN builds nhid -> nhid)")
        if nin > PNA_MAX_HIDDEN:
            raise ValueError(f"SimplifiedPNAConv: width {nin} > {PNA_MAX_HIDDEN} is not served (the message kernel takes 3 * width <= "
                             f"{ops.SPNA_MAX_CHANNELS} channels)")
        self.aggregators = list(aggregators)
        self.pre_nn = MLP(3 * nin, nin, 2, False)
        self.post_nn = MLP(3 * nin, nout, 2, False, bias=bias)
        self.deg_embedder = nn.Embedding(DEG_VOCAB, nin)

    def reset_parameters(self):
        self.pre_nn.reset_parameters()
        self.post_nn.reset_parameters()
        self.deg_embedder.reset_parameters()


_WRAPPERS = {"GINEConv": GINEConv, "GINConv": GINConv, "GCNConv": GCNConv, "GATConv": GATConv, "SimplifiedPNAConv": SimplifiedPNAConv}


def _gat_operator(data, N):
    """The batch's CSR by destination without the input self loops, and its transpose (the adjoint's), once per forward."""
    ei = data.edge_index
    keep = ei[0] != ei[1]
    s, t = ei[0][keep], ei[1][keep]
    return _operator_pair(s, t, torch.ones(s.numel(), dtype=torch.float32, device=ei.device), N)


class GNN(_pyg.GNN):
    """core/model.py's GNN with the reference's signature, for the five gnn_type values.  'GINEConv' is pyg.GNN itself (same launches, bit
    for bit).  Three modes: eval, the train-mode forward without autograd (batch statistics, running-statistics update) and the
    differentiable train-mode forward — pyg.GNN's forwards; this class supplies the conv modules and the two hooks below."""

    def __init__(self, nfeat_node, nfeat_edge, nhid, nout, nlayer, gnn_type, dropout=0, pooling="add", bn=True, dos_bins=0, res=True):
        if gnn_type not in _WRAPPERS:
            raise ValueError(f"GNN: unknown gnn_type {gnn_type!r}; one of {', '.join(GNN_TYPES)}")
        if not bn or dos_bins:
            raise NotImplementedError("GNN: bn=False and dos_bins > 0 are not built on the HIP path")
        super().__init__(nfeat_node, nfeat_edge, nhid, nout, nlayer, "gine", pooling, dropout=dropout, res=res)
        self.gnn_type = gnn_type
        if gnn_type != "GINEConv":
            self.convs = nn.ModuleList([_WRAPPERS[gnn_type](nhid, nhid, bias=not bn) for _ in range(nlayer)])      # core/model.py:15

    # ------------------------------------------------------------------ what the convs share per forward
    def _check_edge_ids(self, ea, status):
        """The edge-blind convs never read the edge embeddings, but the reference computes them (core/model.py:61) and nn.Embedding raises for
        an id outside its table: the first layer's tables (all layers' have one size) are looked up once, for the range check alone."""
        enc = self.edge_encoders[0]
        if isinstance(enc, DiscreteEncoder) and ea.numel():
            ops.embedding_sum(ea, [e.weight.detach() for e in enc.embeddings], status)

    @staticmethod
    def _degrees(plan):
        deg = plan.rowptr[1:] - plan.rowptr[:-1]                  # in-degree, int32 [N]
        return deg.long(), deg.clamp(max=1).contiguous()

    # ------------------------------------------------------------------ the conv-type hooks of pyg.GNN's two forwards
    def _conv_value(self, c, ea):
        """Eval / train-mode value without autograd: per conv type what it needs once per forward, then its layer body (module docstring)."""
        kind = self.gnn_type
        if kind == "GINEConv":
            return super()._conv_value(c, ea)
        plan, pack, lin_bn = c.plan, c.pack, c.lin_bn
        encs, convs, norms = list(self.edge_encoders), list(self.convs), list(self.norms)
        if kind != "SimplifiedPNAConv":
            self._check_edge_ids(ea, c.status)
        if kind == "GINConv":
            def layer(li, h, res):
                conv = convs[li]
                u = ops.gin_aggregate(h, plan, conv.layer.eps.detach())
                u = ops.masked_linear(u, pack(conv.nn.layers[0]), relu=True)
                return lin_bn(u, conv.nn.layers[1], norms[li], residual=res)
        elif kind == "GCNConv":
            dis = ops.gcn_pyg_coef(plan)

            def layer(li, h, res):
                return lin_bn(ops.gcn_pyg_propagate(h, plan, dis), convs[li].layer.lin, norms[li], residual=res)
        elif kind == "GATConv":
            op = _gat_operator(c.data, plan.N)

            def layer(li, h, res):
                L = convs[li].layer
                f = ops.masked_linear(h, pack(L.lin_src))
                z, _ = ops.gat_conv(f, L.att_src.detach(), L.att_dst.detach(), None, op, L.heads, None, L.negative_slope)
                return c.bn_act(z, norms[li], res)
        else:
            deg, has_in = self._degrees(plan)

            def layer(li, h, res):
                conv, d = convs[li], h.shape[1]
                W1 = conv.pre_nn.layers[0].weight.detach()
                pab = c.cached(("ab", id(conv)), lambda: ops.PackedLinear(ops.pack_weight(torch.cat([W1[:, :d], W1[:, d:2 * d]], 0).contiguous()),
                                                                          6 * d, d, None))
                pq = c.cached(("q", id(conv)), lambda: ops.PackedLinear(ops.pack_weight(W1[:, 2 * d:].contiguous()), 3 * d, d, None))
                ab = ops.masked_linear(h, pab)                                        # [N, 2C]: A | B
                q = ops.masked_linear(c.encode(encs[li], ea), pq)                     # [E, C]
                a, b = ab[:, :3 * d], ab[:, 3 * d:]
                bn0 = conv.pre_nn.norms[0]
                if c.train:
                    state, _ = ops.spna_stats(a, b, q, plan, bn0)
                    r = ops.spna_mean(a, b, q, plan, state[3], state[4])
                else:
                    f0 = c.bn_of(bn0)
                    r = ops.spna_mean(a, b, q, plan, f0.scale, f0.shift)
                m = ops.masked_linear(r, pack(conv.pre_nn.layers[1]), has_in, 1)      # W2 mean + b2 [deg > 0]
                de = ops.embedding_sum(deg, [conv.deg_embedder.weight.detach()], c.status)
                u = lin_bn(torch.cat([h, m, de], dim=-1), conv.post_nn.layers[0], conv.post_nn.norms[0])
                return lin_bn(u, conv.post_nn.layers[1], norms[li], residual=res)
        return layer

    def _conv_grad(self, c, ea):
        """Differentiable train mode.  Under a bucketed step (c.pad: the padded batch of train_graph.BucketedStep) per conv type:
          GINConv   the padding self loops feed padding nodes only, whose rows are zeros; the Linears mask them.
          GCNConv   needs no kernel of its own: sn_gcn_pyg_coef_f32 / _propagate_f32 skip self loops, and padding edges are self loops
                    on padding nodes, so the degree of every valid node and every term of its sum are the eager step's.
          GATConv   the operator pair comes from ops.csr_drop_loops (fixed shapes, no host read) in place of _gat_operator.
          SimplifiedPNAConv   the edge-row BatchNorm runs its masked launches (statistics and adjoint sums over counts[1] rows); degrees
                    of invalid rows are forced to 0."""
        kind = self.gnn_type
        if kind == "GINEConv":
            return super()._conv_grad(c, ea)
        plan, rplan, pad, vN, vE, k1, lin_bn = c.plan, c.rplan, c.pad, c.vN, c.vE, c.k1, c.lin_bn
        encs, convs, norms = list(self.edge_encoders), list(self.convs), list(self.norms)
        if kind != "SimplifiedPNAConv":
            self._check_edge_ids(ea, c.status)
        if kind == "GINConv":
            def layer(li, h, res):
                conv = convs[li]
                l0 = conv.nn.layers[0]
                u = AG.gin_aggregate(h, conv.layer.eps, plan, rplan)
                u = AG.linear(u, l0.weight, l0.bias, vN, k1, relu=True)
                return lin_bn(u, conv.nn.layers[1], norms[li], vN, residual=res)
        elif kind == "GCNConv":
            dis = ops.gcn_pyg_coef(plan)

            def layer(li, h, res):
                return lin_bn(AG.gcn_pyg_propagate(h, plan, rplan, dis), convs[li].layer.lin, norms[li], vN, residual=res)
        elif kind == "GATConv":
            op = _gat_operator(c.data, plan.N) if pad is None else ops.csr_drop_loops(plan, rplan)

            def layer(li, h, res):
                L = convs[li].layer
                f = AG.linear(h, L.lin_src.weight, None, vN, k1)
                z = AG.gat_conv(f, L.att_src, L.att_dst, None, op, L.heads, None, L.negative_slope)
                return AG.bn_act(z, norms[li], vN, k1, relu=True, residual=res)
        else:
            d = self.linear.weight.shape[0]
            deg, has_in = self._degrees(plan)
            if pad is not None:
                # (a padding node can carry hundreds of padding edges — all of them when N_cap - N = 1 — and deg_embedder has 200 rows)
                deg, has_in = self._valid_ids(deg, vN), self._valid_ids(has_in, vN)

            def layer(li, h, res):
                conv = convs[li]
                W1 = conv.pre_nn.layers[0].weight
                ab = AG.linear(h, torch.cat([W1[:, :d], W1[:, d:2 * d]], 0), None, vN, k1)
                q = AG.linear(c.encode(encs[li], ea, vE), W1[:, 2 * d:], None, vE, k1)
                if pad is None:
                    r = AG.spna_mean(ab, q, conv.pre_nn.norms[0], plan, rplan)
                else:
                    r = AG.spna_mean(ab, q, conv.pre_nn.norms[0], plan, rplan, vN, pad.counts)
                l1 = conv.pre_nn.layers[1]
                m = AG.linear(r, l1.weight, l1.bias, has_in, 1)
                de = AG.embedding_sum(deg, [conv.deg_embedder.weight], c.status)
                u = lin_bn(torch.cat([h, m, de], dim=-1), conv.post_nn.layers[0], conv.post_nn.norms[0], vN)
                return lin_bn(u, conv.post_nn.layers[1], norms[li], vN, residual=res)
        return layer
