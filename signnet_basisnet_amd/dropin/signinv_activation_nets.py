"""The five `nets.ZINC_graph_regression.*_net` names of GraphPrediction and `nets.ZINC_graph_regression.sign_inv_net` for
`dropin.install('graphprediction', sign_inv_activation=True)`: the base nets whose sign-invariant encoder takes `--sign_inv_activation
tanh | elu` (activation_signinv.py; `--dropout` and `--readout max` too)."""
from ..activation_signinv import GATNet, GatedGCNNet, GINNet, PNANet, TransformerNet, get_sign_inv_net  # noqa: F401
