"""torch_geometric.utils: the existing stand-in's functions (degree, ...) plus the self-loop helpers and `softmax` that GCNConv and
GATConv are documented in terms of."""
import os

import torch

from .. import _BEHIND, _behind

__path__.append(os.path.join(_BEHIND, "utils"))
_base = _behind("utils")
globals().update({k: v for k, v in vars(_base).items() if not k.startswith("_")})


def remove_self_loops(edge_index, edge_attr=None):
    keep = edge_index[0] != edge_index[1]
    return edge_index[:, keep], None if edge_attr is None else edge_attr[keep]


def add_self_loops(edge_index, edge_attr=None, fill_value=1.0, num_nodes=None):
    """One loop per node appended behind the given edges (weight `fill_value`)."""
    n = int(edge_index.max()) + 1 if num_nodes is None else int(num_nodes)
    loop = torch.arange(n, dtype=edge_index.dtype)
    if edge_attr is not None:
        edge_attr = torch.cat([edge_attr, edge_attr.new_full((n,) + tuple(edge_attr.shape[1:]), fill_value)])
    return torch.cat([edge_index, torch.stack([loop, loop])], 1), edge_attr


def add_remaining_self_loops(edge_index, edge_attr=None, fill_value=1.0, num_nodes=None):
    """Every node ends up with exactly one loop: the given self loops are taken out, one loop per node is appended, and a node that had a
    loop keeps that loop's weight (documented behaviour; with unit weights every loop weighs `fill_value` = 1)."""
    n = int(edge_index.max()) + 1 if num_nodes is None else int(num_nodes)
    keep = edge_index[0] != edge_index[1]
    loop = torch.arange(n, dtype=edge_index.dtype)
    if edge_attr is not None:
        loop_w = edge_attr.new_full((n,) + tuple(edge_attr.shape[1:]), fill_value)
        loop_w[edge_index[0][~keep]] = edge_attr[~keep]
        edge_attr = torch.cat([edge_attr[keep], loop_w])
    return torch.cat([edge_index[:, keep], torch.stack([loop, loop])], 1), edge_attr


def softmax(src, index, ptr=None, num_nodes=None, dim=0):
    """Softmax of `src` over the entries that share an `index` value (the group maximum is subtracted first; the denominator is the group
    sum plus 1e-16)."""
    if dim != 0 or ptr is not None:
        raise NotImplementedError("stand-in: softmax along dim 0 by index only")
    n = int(index.max()) + 1 if num_nodes is None else int(num_nodes)
    idx = index.view(-1, *([1] * (src.dim() - 1))).expand_as(src)
    top = torch.full((n,) + tuple(src.shape[1:]), float("-inf"), dtype=src.dtype).scatter_reduce(0, idx, src, "amax", include_self=True)
    out = (src - top.index_select(0, index)).exp()
    tot = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).scatter_add_(0, idx, out)
    return out / (tot.index_select(0, index) + 1e-16)
