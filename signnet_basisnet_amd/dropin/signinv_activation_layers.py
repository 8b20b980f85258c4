"""`layers.deepsigns` of GraphPrediction for `dropin.install('graphprediction', sign_inv_activation=True)`: the four sign-invariant
encoders that take `activation='tanh'` (and 'elu' where the reference's own classes do: activation_signinv.py)."""
from ..activation_signinv import GCNDeepSigns, GINDeepSigns, MaskedGINDeepSigns, TransformerDeepSigns  # noqa: F401
from ..dgl_deepsigns import GCN, GIN, MLP  # noqa: F401
