"""dgl.nn.pytorch: GINConv and GATConv of the existing stand-in, and GraphConv restated from DGL's published definition."""
import sys

import torch

from . import glob  # noqa: F401

_behind = sys.modules["_ref_shim_dgl"].nn.pytorch
GINConv, GATConv = _behind.GINConv, _behind.GATConv


class GraphConv(torch.nn.Module):
    """dgl.nn.pytorch.GraphConv: rst = D_in^-1/2 A D_out^-1/2 feat W + bias (norm='both', degrees clamped to 1), the weight applied
    before the aggregation when in_feats > out_feats; multi-edges add, self loops are ordinary edges; a zero-in-degree node raises
    unless allow_zero_in_degree.  weight [in, out] Glorot uniform, bias zeros.  feat may carry extra middle dimensions ([N, K, in])."""

    def __init__(self, in_feats, out_feats, norm="both", weight=True, bias=True, activation=None, allow_zero_in_degree=False):
        super().__init__()
        assert norm == "both" and weight and bias
        self._in_feats, self._out_feats, self._allow_zero = in_feats, out_feats, allow_zero_in_degree
        self.weight = torch.nn.Parameter(torch.Tensor(in_feats, out_feats))
        self.bias = torch.nn.Parameter(torch.Tensor(out_feats))
        torch.nn.init.xavier_uniform_(self.weight)
        torch.nn.init.zeros_(self.bias)
        self._activation = activation

    def forward(self, g, feat):
        src, dst = g.edges()
        N = feat.shape[0]
        in_deg = torch.bincount(dst, minlength=N)
        if not self._allow_zero and (in_deg == 0).any():
            raise RuntimeError("There are 0-in-degree nodes in the graph")
        shp = (N,) + (1,) * (feat.dim() - 1)
        out_deg = torch.bincount(src, minlength=N).to(feat.dtype).clamp(min=1)
        feat_src = feat * torch.pow(out_deg, -0.5).reshape(shp)
        if self._in_feats > self._out_feats:
            feat_src = torch.matmul(feat_src, self.weight)
            rst = torch.zeros_like(feat_src).index_add_(0, dst, feat_src.index_select(0, src))
        else:
            rst = torch.zeros_like(feat_src).index_add_(0, dst, feat_src.index_select(0, src))
            rst = torch.matmul(rst, self.weight)
        rst = rst * torch.pow(in_deg.to(feat.dtype).clamp(min=1), -0.5).reshape(shp)
        rst = rst + self.bias
        if self._activation is not None:
            rst = self._activation(rst)
        return rst
