"""The five `nets.ZINC_graph_regression.*_net` names of GraphPrediction and `nets.ZINC_graph_regression.sign_inv_net` for
`dropin.install('graphprediction', sign_inv_dropout=True)`: the base nets and the sign-invariant encoders that both take `--dropout`
(dropout_signinv.py)."""
from ..dropout_signinv import GATNet, GatedGCNNet, GINNet, PNANet, TransformerNet, get_sign_inv_net  # noqa: F401
