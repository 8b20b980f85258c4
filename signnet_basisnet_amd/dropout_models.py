"""The models that take train-mode dropout: the plain GNN of GINESignNetPyG for every model.gnn_type and the five DGL base
nets, with the reference's constructors.  Opt-in by class: pyg.GNN, pyg_gnn_types.GNN and the dgl_nets classes keep refusing `dropout > 0` /
`in_feat_dropout > 0` exactly as before; these subclasses carry the same parameters, `state_dict` keys and forwards and differ in one
class attribute.  With dropout 0 they ARE their base classes, launch for launch.

    from signnet_basisnet_amd.dropout_models import GNN, GatedGCNNet
    net = GatedGCNNet(dict(net_params, dropout=0.1)); net.seed_dropout(seed)
"""
from . import dgl_nets, pyg_gnn_types


class GNN(pyg_gnn_types.GNN):
    _feature_dropout = True


class GINNet(dgl_nets.GINNet):
    _feature_dropout = True


class GatedGCNNet(dgl_nets.GatedGCNNet):
    _feature_dropout = True


class PNANet(dgl_nets.PNANet):
    _feature_dropout = True


class TransformerNet(dgl_nets.TransformerNet):
    _feature_dropout = True


class GATNet(dgl_nets.GATNet):
    _feature_dropout = True


NETS = {c.__name__: c for c in (GINNet, GatedGCNNet, PNANet, TransformerNet, GATNet)}
