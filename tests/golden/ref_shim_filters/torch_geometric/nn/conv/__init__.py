"""torch_geometric.nn.conv: MessagePassing with a working propagate (restated from the documentation), ChebConv, GCNConv."""
import inspect

import torch


class MessagePassing(torch.nn.Module):
    """propagate(edge_index, size=None, **kw): message() is called with the arguments it names — `<name>_j` = kw[name] gathered at the
    source nodes edge_index[0], `<name>_i` at the targets edge_index[1], anything else passed through — its result is add-aggregated at
    the targets, and update() gets the aggregate.  flow source_to_target, aggr 'add', node dimension -2 only."""

    def __init__(self, aggr="add", flow="source_to_target", node_dim=-2, **kwargs):
        super().__init__()
        self.aggr, self.flow, self.node_dim = aggr, flow, node_dim

    def propagate(self, edge_index, size=None, **kwargs):
        if self.aggr != "add" or self.flow != "source_to_target" or self.node_dim != -2:
            raise NotImplementedError("stand-in: add-aggregation from source to target along dim -2 only")
        src, dst = edge_index[0], edge_index[1]
        args, n = {}, None
        for name in inspect.signature(self.message).parameters:
            if name.endswith(("_j", "_i")):
                full = kwargs[name[:-2]]
                n = full.size(0)
                args[name] = full.index_select(0, src if name.endswith("_j") else dst)
            else:
                args[name] = kwargs[name]
        msg = self.message(**args)
        n = n if size is None else size[1]
        return self.update(torch.zeros((n,) + tuple(msg.shape[1:]), dtype=msg.dtype).index_add_(0, dst, msg))

    def message(self, x_j):
        return x_j

    def update(self, aggr_out):
        return aggr_out


from .cheb_conv import ChebConv  # noqa: E402,F401
from .gcn_conv import GCNConv, gcn_norm  # noqa: E402,F401
