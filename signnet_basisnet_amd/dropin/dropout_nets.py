"""The five `nets.ZINC_graph_regression.*_net` names of GraphPrediction for `dropin.install('graphprediction', feature_dropout=True)`: the
base nets that also take `--dropout` / `--in_feat_dropout` (dropout_models.py)."""
from ..dropout_models import GATNet, GatedGCNNet, GINNet, PNANet, TransformerNet  # noqa: F401
