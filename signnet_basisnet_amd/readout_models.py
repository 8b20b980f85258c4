"""The five DGL base nets with `readout='max'`: dgl.max_nodes in front of MLPReadout, as
nets/ZINC_graph_regression/*_net.py run it for `--readout max`.

Opt-in by class, as dropout_models.py and dropout_signinv.py: the dgl_nets classes — and the dropout classes on top of them — keep refusing
`readout='max'` exactly as before; the subclasses here derive from their dropout_signinv counterparts (so one class takes dropout and `max`
together), carry the same parameters, buffers, `state_dict` keys and forwards and differ in one class attribute.  With readout 'sum' or
'mean' they ARE their base classes, launch for launch.

    from signnet_basisnet_amd.readout_models import GatedGCNNet
    net = GatedGCNNet(dict(net_params, readout="max"))

The value paths pool with sn_segment_max_f32, the differentiable path with autograd.segment_max (the gradient goes to the ONE row that
attains the maximum: of equal values the lowest row), and the one-launch eval kernels of GINNet, GatedGCNNet and TransformerNet take
SN_READOUT_MAX in their readout epilogue — eval stays one launch.
"""
from . import dropout_signinv


class GINNet(dropout_signinv.GINNet):
    _max_readout = True


class GatedGCNNet(dropout_signinv.GatedGCNNet):
    _max_readout = True


class PNANet(dropout_signinv.PNANet):
    _max_readout = True


class TransformerNet(dropout_signinv.TransformerNet):
    _max_readout = True


class GATNet(dropout_signinv.GATNet):
    _max_readout = True


NETS = {c.__name__: c for c in (GINNet, GatedGCNNet, PNANet, TransformerNet, GATNet)}
