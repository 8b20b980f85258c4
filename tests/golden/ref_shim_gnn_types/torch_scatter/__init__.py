"""Stand-in for torch_scatter in front of ../ref_shim/torch_scatter: `scatter` with the reductions core/model_utils/pyg_gnn_wrapper.py
names (add / sum, mean, min, max), restated from the package's published semantics: entries of `src` that share an `index` value along
`dim` are reduced into that slot of the output, a slot nothing maps to is 0, and `mean` divides by the count clamped to 1.  Used only by
tests/golden/make_gnn_types.py."""
import torch


def _expand(index, src, dim):
    if dim < 0:
        dim += src.dim()
    if index.dim() == 1:
        shape = [1] * src.dim()
        shape[dim] = -1
        index = index.view(shape)
    return index.expand_as(src), dim


def scatter(src, index, dim=-1, out=None, dim_size=None, reduce="sum"):
    if out is not None:
        raise NotImplementedError("stand-in: no `out` argument")
    idx, dim = _expand(index, src, dim)
    if dim_size is None:
        dim_size = int(index.max()) + 1 if index.numel() else 0
    shape = list(src.shape)
    shape[dim] = dim_size
    zero = torch.zeros(shape, dtype=src.dtype, device=src.device)
    if reduce in ("add", "sum"):
        return zero.scatter_add_(dim, idx, src)
    if reduce == "mean":
        tot = zero.scatter_add_(dim, idx, src)
        cnt = torch.zeros(shape, dtype=src.dtype, device=src.device).scatter_add_(dim, idx, torch.ones_like(src)).clamp_(min=1)
        return tot / cnt if src.is_floating_point() else torch.div(tot, cnt, rounding_mode="floor")
    if reduce in ("min", "max"):
        return zero.scatter_reduce(dim, idx, src, "a" + reduce, include_self=False)
    raise ValueError(reduce)


def scatter_add(src, index, dim=-1, out=None, dim_size=None):
    return scatter(src, index, dim, out, dim_size, "sum")
