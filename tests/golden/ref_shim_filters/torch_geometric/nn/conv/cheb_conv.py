"""ChebConv of torch_geometric 2.0.1, restated from the documentation:
X' = sum_{k=1..K} Z^(k) Theta^(k) + b,  Z^(1) = X, Z^(2) = L^ X, Z^(k) = 2 L^ Z^(k-1) - Z^(k-2),  L^ = 2 L / lambda_max - I,
lambda_max = 2 for the default 'sym' normalisation."""
import torch

from ...utils import add_self_loops, get_laplacian, remove_self_loops
from . import MessagePassing


class ChebConv(MessagePassing):
    """Parameters as 2.0.1 lays them out: `lins` (K bias-free Linears, glorot) and `bias` (zeros)."""

    def __init__(self, in_channels, out_channels, K, normalization="sym", bias=True, **kwargs):
        kwargs.setdefault("aggr", "add")
        super().__init__(**kwargs)
        assert K > 0
        assert normalization in [None, "sym", "rw"], "Invalid normalization"
        self.in_channels, self.out_channels, self.normalization = in_channels, out_channels, normalization
        self.lins = torch.nn.ModuleList([torch.nn.Linear(in_channels, out_channels, bias=False) for _ in range(K)])
        self.bias = torch.nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        for lin in self.lins:
            torch.nn.init.xavier_uniform_(lin.weight)
        if self.bias is not None:
            torch.nn.init.zeros_(self.bias)

    def __norm__(self, edge_index, num_nodes, edge_weight, normalization, lambda_max, dtype=None):
        edge_index, edge_weight = remove_self_loops(edge_index, edge_weight)
        edge_index, edge_weight = get_laplacian(edge_index, edge_weight, normalization, dtype, num_nodes)
        edge_weight = (2.0 * edge_weight) / lambda_max
        edge_weight.masked_fill_(edge_weight == float("inf"), 0)
        return add_self_loops(edge_index, edge_weight, fill_value=-1.0, num_nodes=num_nodes)

    def forward(self, x, edge_index, edge_weight=None, lambda_max=None):
        if self.normalization != "sym" and lambda_max is None:
            raise ValueError("lambda_max is needed for a normalisation other than 'sym'")
        lambda_max = 2.0 if lambda_max is None else lambda_max
        edge_index, norm = self.__norm__(edge_index, x.size(0), edge_weight, self.normalization, lambda_max, dtype=x.dtype)
        Tx_0 = x
        out = self.lins[0](Tx_0)
        if len(self.lins) > 1:
            Tx_1 = self.propagate(edge_index, x=x, norm=norm, size=None)
            out = out + self.lins[1](Tx_1)
        for lin in self.lins[2:]:
            Tx_2 = 2.0 * self.propagate(edge_index, x=Tx_1, norm=norm, size=None) - Tx_0
            out = out + lin(Tx_2)
            Tx_0, Tx_1 = Tx_1, Tx_2
        return out if self.bias is None else out + self.bias

    def message(self, x_j, norm):
        return norm.view(-1, 1) * x_j
