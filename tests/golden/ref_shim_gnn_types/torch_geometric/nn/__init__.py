"""torch_geometric.nn: the existing stand-in's layers (GINConv, GINEConv, ...) plus a MessagePassing whose `aggregate` a subclass may
override, GCNConv and GATConv — restated from the PyG 2.0.1 documentation."""
import inspect
import os

import torch
import torch.nn.functional as F

from .. import _BEHIND, _behind
from ..utils import add_remaining_self_loops, add_self_loops, remove_self_loops, softmax

__path__.append(os.path.join(_BEHIND, "nn"))
_base = _behind("nn")
globals().update({k: v for k, v in vars(_base).items() if not k.startswith("_") and k not in ("inits", "conv")})
from . import conv, inits  # noqa: E402,F401   (found behind, through __path__)


def _scatter(src, index, dim_size, reduce):
    idx = index.view(-1, *([1] * (src.dim() - 1))).expand_as(src)
    out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype)
    if reduce in ("add", "sum"):
        return out.scatter_add_(0, idx, src)
    if reduce == "mean":
        cnt = torch.zeros_like(out).scatter_add_(0, idx, torch.ones_like(src)).clamp_(min=1)
        return out.scatter_add_(0, idx, src) / cnt
    if reduce in ("min", "max"):
        return out.scatter_reduce(0, idx, src, "a" + reduce, include_self=False)
    raise ValueError(reduce)


class MessagePassing(torch.nn.Module):
    """propagate(edge_index, **kw): message() is called with the arguments it names — `<name>_j` = kw[name] gathered at the source
    nodes edge_index[0], `<name>_i` at the targets edge_index[1], anything else passed through; aggregate(inputs, index, dim_size) reduces
    the messages at the targets with `aggr` ('add', 'mean', 'min', 'max') unless a subclass overrides it (aggr=None then); update() gets
    the aggregate.  flow source_to_target, node dimension 0."""

    def __init__(self, aggr="add", flow="source_to_target", node_dim=-2, **kwargs):
        super().__init__()
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim

    def propagate(self, edge_index, size=None, **kwargs):
        if self.flow != "source_to_target":
            raise NotImplementedError("stand-in: source_to_target only")
        src, dst = edge_index[0], edge_index[1]
        args, n = {}, None if size is None else size[1]
        for name in inspect.signature(self.message).parameters:
            if name.endswith(("_j", "_i")):
                t = kwargs[name[:-2]]
                if not (self.node_dim == 0 or (self.node_dim == -2 and t.dim() == 2)):
                    raise NotImplementedError("stand-in: the node dimension must be dimension 0")
                n = t.size(0) if n is None else n
                args[name] = t.index_select(0, src if name.endswith("_j") else dst)
            else:
                args[name] = kwargs[name]
        msg = self.message(**args)
        return self.update(self.aggregate(msg, index=dst, dim_size=n))

    def message(self, x_j):
        return x_j

    def aggregate(self, inputs, index, dim_size=None):
        return _scatter(inputs, index, dim_size, self.aggr)

    def update(self, aggr_out):
        return aggr_out


class Linear(torch.nn.Module):
    """PyG's own Linear: `weight` [out, in] (glorot), optional `bias` (zeros)."""

    def __init__(self, in_channels, out_channels, bias=True, weight_initializer="glorot"):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(out_channels, in_channels))
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.weight)          # 'glorot': uniform in +-sqrt(6 / (fan_in + fan_out))
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x):
        return F.linear(x, self.weight, self.bias)


class GCNConv(MessagePassing):
    """x' = D^-1/2 (A + I) D^-1/2 X W^T + b: the input's self loops are replaced by one unit loop per node (add_remaining_self_loops),
    deg is the sum of the edge weights over the TARGET index, norm_e = deg^-1/2[source] * deg^-1/2[target] (inf -> 0); `lin` has no
    bias, `bias` is a parameter of its own."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True, **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        if improved or cached or not add_self_loops or not normalize:
            raise NotImplementedError("stand-in: the defaults only")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin = Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter("bias", None)

    def reset_parameters(self):
        self.lin.reset_parameters()
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, edge_weight=None):
        n = x.size(0)
        w = torch.ones(edge_index.size(1), dtype=x.dtype) if edge_weight is None else edge_weight
        ei, w = add_remaining_self_loops(edge_index, w, 1.0, n)
        deg = torch.zeros(n, dtype=x.dtype).scatter_add_(0, ei[1], w)
        dis = deg.pow(-0.5)
        dis.masked_fill_(dis == float("inf"), 0)
        norm = dis[ei[0]] * w * dis[ei[1]]
        out = self.propagate(ei, x=self.lin(x), edge_weight=norm)
        return out if self.bias is None else out + self.bias

    def message(self, x_j, edge_weight):
        return edge_weight.view(-1, 1) * x_j


class GATConv(MessagePassing):
    """heads x out_channels attention (concat=True): x' = lin_src(x) viewed [N, H, C] (lin_dst is the same module for one input),
    a_src = <x', att_src>, a_dst = <x', att_dst>; the input's self loops are removed and one loop per node added; per edge j -> i
    alpha = softmax_i(leaky_relu(a_src[j] + a_dst[i], negative_slope)); out_i = sum_j alpha_ij x'_j, heads concatenated, + bias."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, bias=True,
                 **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(node_dim=0, **kwargs)
        if not concat or dropout or not add_self_loops:
            raise NotImplementedError("stand-in: concat=True, dropout=0, add_self_loops=True only")
        self.in_channels, self.out_channels, self.heads, self.negative_slope = in_channels, out_channels, heads, negative_slope
        self.lin_src = Linear(in_channels, heads * out_channels, bias=False)
        self.lin_dst = self.lin_src
        self.att_src = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_dst = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        if bias:
            self.bias = torch.nn.Parameter(torch.zeros(heads * out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        self.lin_src.reset_parameters()
        torch.nn.init.xavier_uniform_(self.att_src)
        torch.nn.init.xavier_uniform_(self.att_dst)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, edge_index):
        H, C = self.heads, self.out_channels
        xs = self.lin_src(x).view(-1, H, C)
        a_src, a_dst = (xs * self.att_src).sum(-1), (xs * self.att_dst).sum(-1)
        ei, _ = remove_self_loops(edge_index)
        ei, _ = add_self_loops(ei, num_nodes=x.size(0))
        alpha = F.leaky_relu(a_src.index_select(0, ei[0]) + a_dst.index_select(0, ei[1]), self.negative_slope)
        alpha = softmax(alpha, ei[1], num_nodes=x.size(0))
        out = self.propagate(ei, x=xs, alpha=alpha).reshape(-1, H * C)
        return out if self.bias is None else out + self.bias

    def message(self, x_j, alpha):
        return alpha.unsqueeze(-1) * x_j
