"""torch_geometric.utils, restated from the documentation: remove_self_loops, add_self_loops, add_remaining_self_loops, get_laplacian.
Flow source_to_target: edge_index[0] is the source (`row`), edge_index[1] the target (`col`)."""
import torch


def _n(edge_index, num_nodes):
    return int(edge_index.max()) + 1 if num_nodes is None else int(num_nodes)


def remove_self_loops(edge_index, edge_attr=None):
    keep = edge_index[0] != edge_index[1]
    return edge_index[:, keep], (None if edge_attr is None else edge_attr[keep])


def add_self_loops(edge_index, edge_attr=None, fill_value=1.0, num_nodes=None):
    """Appends one (i, i) edge per node, with weight fill_value when weights are given."""
    n = _n(edge_index, num_nodes)
    loop = torch.arange(n, dtype=edge_index.dtype)
    if edge_attr is not None:
        edge_attr = torch.cat([edge_attr, edge_attr.new_full((n,), fill_value)])
    return torch.cat([edge_index, torch.stack([loop, loop])], dim=1), edge_attr


def add_remaining_self_loops(edge_index, edge_attr=None, fill_value=1.0, num_nodes=None):
    """One (i, i) edge per node behind the non-loop edges; a node that had a self loop keeps that loop's weight, the others get fill_value."""
    n = _n(edge_index, num_nodes)
    row, col = edge_index
    keep = row != col
    loop = torch.arange(n, dtype=edge_index.dtype)
    if edge_attr is not None:
        w = edge_attr.new_full((n,), fill_value)
        w[row[~keep]] = edge_attr[~keep]
        edge_attr = torch.cat([edge_attr[keep], w])
    return torch.cat([edge_index[:, keep], torch.stack([loop, loop])], dim=1), edge_attr


def get_laplacian(edge_index, edge_weight=None, normalization=None, dtype=None, num_nodes=None):
    """L = D - A (None), I - D^-1/2 A D^-1/2 ('sym') or I - D^-1 A ('rw') as (edge_index, weights): the off-diagonal entries of the input
    without its self loops, then one diagonal entry per node.  The degree is summed over the source index; 1/0 -> 0."""
    edge_index, edge_weight = remove_self_loops(edge_index, edge_weight)
    if edge_weight is None:
        edge_weight = torch.ones(edge_index.size(1), dtype=dtype)
    n = _n(edge_index, num_nodes)
    row, col = edge_index
    deg = torch.zeros(n, dtype=edge_weight.dtype).scatter_add_(0, row, edge_weight)
    if normalization is None:
        edge_index, _ = add_self_loops(edge_index, num_nodes=n)
        return edge_index, torch.cat([-edge_weight, deg])
    if normalization == "sym":
        dis = deg.pow(-0.5)
        dis.masked_fill_(dis == float("inf"), 0)
        edge_weight = dis[row] * edge_weight * dis[col]
    elif normalization == "rw":
        inv = 1.0 / deg
        inv.masked_fill_(inv == float("inf"), 0)
        edge_weight = inv[row] * edge_weight
    else:
        raise ValueError(normalization)
    return add_self_loops(edge_index, -edge_weight, fill_value=1.0, num_nodes=n)
