"""torch_geometric.nn: the existing stand-in's layers plus a working MessagePassing and Set2Set (restated from the documentation)."""
import inspect
import os

import torch

from .. import _BEHIND, _behind
from ..utils import softmax

__path__.append(os.path.join(_BEHIND, "nn"))
_base = _behind("nn")
globals().update({k: v for k, v in vars(_base).items() if not k.startswith("_") and k not in ("inits", "conv")})
from . import conv, inits  # noqa: E402,F401   (found behind, through __path__)


class MessagePassing(torch.nn.Module):
    """propagate(edge_index, **kw): message() is called with the arguments it names — `<name>_j` = kw[name] gathered at the source
    nodes edge_index[0], `<name>_i` at the targets edge_index[1], anything else passed through — its result is add-aggregated at the
    targets, and update() gets the aggregate.  flow source_to_target, node dimension 0, aggr 'add' only."""

    def __init__(self, aggr="add", flow="source_to_target", node_dim=0, **kwargs):
        super().__init__()
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim

    def propagate(self, edge_index, size=None, **kwargs):
        if self.aggr != "add" or self.flow != "source_to_target" or self.node_dim != 0:
            raise NotImplementedError("stand-in: add-aggregation from source to target along dim 0 only")
        src, dst = edge_index[0], edge_index[1]
        args = {}
        for name in inspect.signature(self.message).parameters:
            if name.endswith("_j"):
                args[name] = kwargs[name[:-2]].index_select(0, src)
            elif name.endswith("_i"):
                args[name] = kwargs[name[:-2]].index_select(0, dst)
            else:
                args[name] = kwargs[name]
        msg = self.message(**args)
        n = next(kwargs[k[:-2]].size(0) for k in args if k.endswith(("_j", "_i"))) if size is None else size[1]
        out = torch.zeros((n,) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add_(0, dst, msg)
        return self.update(out)

    def message(self, x_j):
        return x_j

    def update(self, aggr_out):
        return aggr_out


class Set2Set(torch.nn.Module):
    """Set2Set(in_channels, processing_steps, num_layers=1): q_t = LSTM(q*_{t-1}); a = softmax over each graph's nodes of <x_n, q_t>;
    r_t = sum_n a_n x_n; q*_t = [q_t, r_t]; the output is q*_T [batch_size, 2 in_channels] (q*_0 and the LSTM state start at zero)."""

    def __init__(self, in_channels, processing_steps, num_layers=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, 2 * in_channels
        self.processing_steps, self.num_layers = processing_steps, num_layers
        self.lstm = torch.nn.LSTM(self.out_channels, in_channels, num_layers)

    def reset_parameters(self):
        self.lstm.reset_parameters()

    def forward(self, x, batch):
        nb = int(batch.max()) + 1
        state = (x.new_zeros(self.num_layers, nb, self.in_channels), x.new_zeros(self.num_layers, nb, self.in_channels))
        q_star = x.new_zeros(nb, self.out_channels)
        for _ in range(self.processing_steps):
            q, state = self.lstm(q_star.unsqueeze(0), state)
            q = q.view(nb, self.in_channels)
            a = softmax((x * q.index_select(0, batch)).sum(-1, keepdim=True), batch, num_nodes=nb)
            r = x.new_zeros(nb, self.in_channels).index_add_(0, batch, a * x)
            q_star = torch.cat([q, r], dim=-1)
        return q_star
