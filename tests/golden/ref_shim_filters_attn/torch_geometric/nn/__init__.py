"""torch_geometric.nn as LearningFilters/models.py imports it (models.py:9-11), with GATConv and ARMAConv of 2.0.1 restated from the
library's documentation (parameter names, shapes and registration order from memory of that release); `.conv` is ../ref_shim_filters'."""
import math
import os as _os

import torch
import torch.nn.functional as F

__path__.append(_os.path.join(_os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))),
                              "ref_shim_filters", "torch_geometric", "nn"))

from .conv import ChebConv, GCNConv, MessagePassing  # noqa: E402,F401
from .conv.gcn_conv import gcn_norm  # noqa: E402
from ..utils import add_self_loops as _add_self_loops, remove_self_loops as _remove_self_loops  # noqa: E402


def glorot(t):
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-bound, bound)


class GATConv(MessagePassing):
    """x' = lin_l(x) viewed [N, heads, out] (lin_r is the same module for one input tensor); alpha_l = <x', att_l>, alpha_r = <x', att_r>;
    self loops removed, then one per node; e = leaky_relu(alpha_l[source] + alpha_r[target]); softmax over each target's edges (maximum
    subtracted, denominator + 1e-16); out[target] = sum a * x'[source]; heads concatenated; + bias."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True, bias=True,
                 **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        if not concat or dropout:
            raise NotImplementedError("stand-in: concat=True and dropout=0 only (all LearningFilters/models.py uses)")
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout, self.add_self_loops = concat, negative_slope, dropout, add_self_loops
        self.lin_l = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.att_r = torch.nn.Parameter(torch.empty(1, heads, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(heads * out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.lin_l.weight)
        glorot(self.att_l)
        glorot(self.att_r)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, edge_index):
        N, H, C = x.size(0), self.heads, self.out_channels
        xl = self.lin_l(x).view(N, H, C)
        al, ar = (xl * self.att_l).sum(-1), (xl * self.att_r).sum(-1)
        if self.add_self_loops:
            edge_index, _ = _remove_self_loops(edge_index)
            edge_index, _ = _add_self_loops(edge_index, num_nodes=N)
        src, dst = edge_index[0], edge_index[1]
        e = F.leaky_relu(al[src] + ar[dst], self.negative_slope)
        top = torch.full((N, H), float("-inf"), dtype=e.dtype).scatter_reduce(0, dst.view(-1, 1).expand(-1, H), e, "amax", include_self=True)
        p = (e - top[dst]).exp()
        a = p / (torch.zeros(N, H, dtype=e.dtype).index_add_(0, dst, p)[dst] + 1e-16)
        out = torch.zeros(N, H, C, dtype=e.dtype).index_add_(0, dst, a.unsqueeze(-1) * xl[src]).view(N, H * C)
        return out if self.bias is None else out + self.bias


class ARMAConv(MessagePassing):
    """K = num_stacks parallel stacks of T = num_layers layers over S = gcn_norm(..., add_self_loops=False):
    X(t+1) = act(S X(t) W + X(0) V + b) with W = init_weight in the first layer, weight[t-1] after it; the stacks are averaged."""

    def __init__(self, in_channels, out_channels, num_stacks=1, num_layers=1, shared_weights=False, act=None, dropout=0.0, bias=True,
                 **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        if dropout:
            raise NotImplementedError("stand-in: dropout=0 only (all LearningFilters/models.py uses)")
        self.in_channels, self.out_channels, self.num_stacks, self.num_layers = in_channels, out_channels, num_stacks, num_layers
        self.act, self.shared_weights, self.dropout = torch.nn.ReLU() if act is None else act, shared_weights, dropout
        K, T = num_stacks, (1 if shared_weights else num_layers)
        self.init_weight = torch.nn.Parameter(torch.empty(K, in_channels, out_channels))
        self.weight = torch.nn.Parameter(torch.empty(max(1, T - 1), K, out_channels, out_channels))
        self.root_weight = torch.nn.Parameter(torch.empty(T, K, in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.empty(T, K, 1, out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.init_weight)
        glorot(self.weight)
        glorot(self.root_weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, edge_weight=None):
        edge_index, edge_weight = gcn_norm(edge_index, edge_weight, x.size(0), add_self_loops=False, dtype=x.dtype)
        src, dst = edge_index[0], edge_index[1]
        x = x.unsqueeze(-3)                                               # [1, N, F]: broadcast over the stacks
        out = x
        for t in range(self.num_layers):
            out = out @ (self.init_weight if t == 0 else self.weight[0 if self.shared_weights else t - 1])
            out = torch.zeros_like(out).index_add_(-2, dst, edge_weight.view(-1, 1) * out[..., src, :])
            out = out + x @ self.root_weight[0 if self.shared_weights else t]
            if self.bias is not None:
                out = out + self.bias[0 if self.shared_weights else t]
            out = self.act(out)
        return out.mean(dim=-3)
