"""Train-mode dropout in the sign-invariant encoders of the DGL tree: `--dropout P` with lap_method 'sign_inv'.

Opt-in by class, as dropout_models.py: the classes of dgl_deepsigns, its get_sign_inv_net and the dropout_models nets with lap_method
'sign_inv' keep refusing `dropout > 0` exactly as before; the subclasses here carry the same parameters, buffers, `state_dict` keys and
forwards and differ in one class attribute.  With dropout 0, and in eval at any dropout, they ARE their base classes, launch for launch.

    from signnet_basisnet_amd.dropout_signinv import GatedGCNNet
    net = GatedGCNNet(dict(net_params, lap_method="sign_inv", dropout=0.1)); net.seed_dropout(seed)

The masks are those of sn_dropout_f32 at site SN_SIGNINV_DROP_SITE + the ordinal of the reference module's dropout call within one
forward — enc(g, x), then enc(g, -x), then rho.  The two encoder calls draw different masks, so a train-mode forward with p > 0 is
NOT sign-invariant, in the reference as here; eval draws nothing and stays invariant bit for bit.  A stand-alone encoder is its own
ops.DropoutHolder (`enc.seed_dropout(seed, step)`); a net's `seed_dropout` seeds its `sign_inv_net` too, and each of the two states
advances once per training step: after `net.seed_dropout(seed, s)` the encoder's forward in handle_lap and the net's forward both draw
step s + 1, on disjoint sites.
"""
from . import dgl_deepsigns, dropout_models


class GINDeepSigns(dgl_deepsigns.GINDeepSigns):
    _signinv_dropout = True


class MaskedGINDeepSigns(dgl_deepsigns.MaskedGINDeepSigns):
    _signinv_dropout = True


class GCNDeepSigns(dgl_deepsigns.GCNDeepSigns):
    _signinv_dropout = True


class TransformerDeepSigns(dgl_deepsigns.TransformerDeepSigns):
    _signinv_dropout = True


ENCODERS = {"gcn": GCNDeepSigns, "gin": GINDeepSigns, "masked_gin": MaskedGINDeepSigns, "transformer": TransformerDeepSigns}


def get_sign_inv_net(net_params):
    """dgl_deepsigns.get_sign_inv_net with the classes of this module: `net_params['dropout']` reaches the encoder, as in
    nets/ZINC_graph_regression/sign_inv_net.py:7-13."""
    return dgl_deepsigns.sign_inv_net_from(net_params, ENCODERS)


class _SeedsEncoder:
    """One seed interface per model: the net's seed_dropout also seeds its sign_inv_net."""
    _sign_inv_factory = staticmethod(get_sign_inv_net)

    def seed_dropout(self, seed, step=0):
        super().seed_dropout(seed, step)
        enc = getattr(self, "sign_inv_net", None)
        if enc is not None:
            enc.seed_dropout(seed, step)
        return self


class GINNet(_SeedsEncoder, dropout_models.GINNet):
    pass


class GatedGCNNet(_SeedsEncoder, dropout_models.GatedGCNNet):
    pass


class PNANet(_SeedsEncoder, dropout_models.PNANet):
    pass


class TransformerNet(_SeedsEncoder, dropout_models.TransformerNet):
    pass


class GATNet(_SeedsEncoder, dropout_models.GATNet):
    pass


NETS = {c.__name__: c for c in (GINNet, GatedGCNNet, PNANet, TransformerNet, GATNet)}
