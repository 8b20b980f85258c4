"""torch_geometric.utils: the existing stand-in's functions plus `softmax`."""
import torch

from .. import _BEHIND, _behind
import os

__path__.append(os.path.join(_BEHIND, "utils"))
_base = _behind("utils")
globals().update({k: v for k, v in vars(_base).items() if not k.startswith("_")})


def softmax(src, index, ptr=None, num_nodes=None, dim=0):
    """Softmax of `src` over the entries that share an `index` value (documented: group-wise along `dim`; the group maximum is subtracted
    first and the denominator is the group sum plus 1e-16)."""
    if dim != 0 or ptr is not None:
        raise NotImplementedError("stand-in: softmax along dim 0 by index only")
    n = int(index.max()) + 1 if num_nodes is None else int(num_nodes)
    idx = index.view(-1, *([1] * (src.dim() - 1))).expand_as(src)
    top = torch.full((n,) + tuple(src.shape[1:]), float("-inf"), dtype=src.dtype).scatter_reduce(0, idx, src, "amax", include_self=True)
    out = (src - top.index_select(0, index)).exp()
    tot = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype).scatter_add_(0, idx, out)
    return out / (tot.index_select(0, index) + 1e-16)
