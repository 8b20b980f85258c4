"""`core.model` of GINESignNetPyG for `dropin.install('gine_pyg', baselines=True)`: the plain GINE baseline that train/zinc.py:31-46
builds when model.gnn_type is not 'SignNet', behind the reference's constructor (core/model.py:11)."""
from ..pyg import GNN as _GNN


class GNN(_GNN):
    def __init__(self, nfeat_node, nfeat_edge, nhid, nout, nlayer, gnn_type, dropout=0, pooling="add", bn=True, dos_bins=0, res=True):
        if gnn_type != "GINEConv":
            raise NotImplementedError(f"GNN: only gnn_type='GINEConv' is built on the HIP path (got {gnn_type!r})")
        if not bn or dos_bins:
            raise NotImplementedError("GNN: bn=False and dos_bins > 0 are not built on the HIP path")
        super().__init__(nfeat_node, nfeat_edge, nhid, nout, nlayer, "gine", pooling, dropout=dropout, res=res)
