"""The five `nets.ZINC_graph_regression.*_net` names of GraphPrediction for `dropin.install('graphprediction', max_readout=True)`: the
base nets that take `--readout max` next to `sum` / `mean` (readout_models.py; dropout in the nets and the sign-invariant encoder too)."""
from ..readout_models import GATNet, GatedGCNNet, GINNet, PNANet, TransformerNet  # noqa: F401
