"""gcn_norm and GCNConv of torch_geometric 2.0.1, restated from the documentation:
X' = D^-1/2 (A + I) D^-1/2 X Theta + b, the degree of A + I summed over the target index."""
import torch

from ...utils import add_remaining_self_loops
from . import MessagePassing


def gcn_norm(edge_index, edge_weight=None, num_nodes=None, improved=False, add_self_loops=True, dtype=None):
    fill = 2.0 if improved else 1.0
    n = int(edge_index.max()) + 1 if num_nodes is None else int(num_nodes)
    if edge_weight is None:
        edge_weight = torch.ones(edge_index.size(1), dtype=dtype)
    if add_self_loops:
        edge_index, edge_weight = add_remaining_self_loops(edge_index, edge_weight, fill, n)
    row, col = edge_index
    deg = torch.zeros(n, dtype=edge_weight.dtype).scatter_add_(0, col, edge_weight)
    dis = deg.pow(-0.5)
    dis.masked_fill_(dis == float("inf"), 0)
    return edge_index, dis[row] * edge_weight * dis[col]


class GCNConv(MessagePassing):
    """Parameters as 2.0.1 lays them out: `lin` (a bias-free Linear, glorot) and `bias` (zeros)."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True, **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.add_self_loops, self.normalize = improved, add_self_loops, normalize
        self.lin = torch.nn.Linear(in_channels, out_channels, bias=False)
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.xavier_uniform_(self.lin.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def forward(self, x, edge_index, edge_weight=None):
        if self.normalize:
            edge_index, edge_weight = gcn_norm(edge_index, edge_weight, x.size(0), self.improved, self.add_self_loops, dtype=x.dtype)
        out = self.propagate(edge_index, x=self.lin(x), edge_weight=edge_weight, size=None)
        return out if self.bias is None else out + self.bias

    def message(self, x_j, edge_weight):
        return x_j if edge_weight is None else edge_weight.view(-1, 1) * x_j
