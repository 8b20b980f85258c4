"""`--sign_inv_activation tanh | elu` in the sign-invariant encoders of the DGL tree.

Opt-in by class, as dropout_signinv.py and readout_models.py: the classes of dgl_deepsigns (and of dropout_signinv) keep refusing anything but
'relu' exactly as before; the subclasses here derive from their dropout_signinv counterparts (so `--dropout` composes), carry the same
parameters, buffers, `state_dict` keys and forwards and differ in one class attribute.  With activation 'relu' they ARE their base
classes, launch for launch and bit for bit — the three-launch fused forward of the GIN encoders included.

    from signnet_basisnet_amd.activation_signinv import GatedGCNNet
    net = GatedGCNNet(dict(net_params, lap_method="sign_inv", sign_inv_activation="tanh"))

What the reference accepts is mirrored with its errors: layers/mlp.py:23-30 takes relu | elu | tanh and raises ValueError('Invalid
activation') otherwise; layers/gnns.py:13 looks the name up in {'relu', 'tanh'} BEFORE the first MLP is built, so 'gin', 'masked_gin'
and 'gcn' raise KeyError for 'elu' and for any unknown name; only TransformerDeepSigns, whose activation reaches nothing but its rho
MLP, takes 'elu'.  The ReLU inside SetTransformerEncoder's feed-forward net is DGL's own and stays.

A non-ReLU activation site — behind every hidden Linear of an MLP (the GIN update nets, every rho) and behind GraphConv's bias — is the
layer-path GEMM with its bias and then ONE sn_act_affine_f32 launch (eval: with the folded BatchNorm that follows; train: bare, the
batch statistics are taken on the activated tensor) — one launch more than ReLU, which rides in the GEMM's epilogue; under autograd
autograd.activation, whose adjoint reads only the saved output.  Such an encoder has no stage kernels: the GIN encoders take the layer
path (`fused_stages` has no effect) and `matmul_precision` accepts "highest" only.
"""
from . import dgl_deepsigns, dropout_signinv, readout_models


class GINDeepSigns(dropout_signinv.GINDeepSigns):
    _signinv_activations = ("relu", "tanh")


class MaskedGINDeepSigns(dropout_signinv.MaskedGINDeepSigns):
    _signinv_activations = ("relu", "tanh")


class GCNDeepSigns(dropout_signinv.GCNDeepSigns):
    _signinv_activations = ("relu", "tanh")


class TransformerDeepSigns(dropout_signinv.TransformerDeepSigns):
    _signinv_activations = ("relu", "elu", "tanh")


ENCODERS = {"gcn": GCNDeepSigns, "gin": GINDeepSigns, "masked_gin": MaskedGINDeepSigns, "transformer": TransformerDeepSigns}


def get_sign_inv_net(net_params):
    """dropout_signinv.get_sign_inv_net with the classes of this module: `net_params['sign_inv_activation']` reaches the encoder, as in
    nets/ZINC_graph_regression/sign_inv_net.py:7-13."""
    return dgl_deepsigns.sign_inv_net_from(net_params, ENCODERS)


class _ActivationEncoder:
    _sign_inv_factory = staticmethod(get_sign_inv_net)


class GINNet(_ActivationEncoder, readout_models.GINNet):
    pass


class GatedGCNNet(_ActivationEncoder, readout_models.GatedGCNNet):
    pass


class PNANet(_ActivationEncoder, readout_models.PNANet):
    pass


class TransformerNet(_ActivationEncoder, readout_models.TransformerNet):
    pass


class GATNet(_ActivationEncoder, readout_models.GATNet):
    pass


NETS = {c.__name__: c for c in (GINNet, GatedGCNNet, PNANet, TransformerNet, GATNet)}
