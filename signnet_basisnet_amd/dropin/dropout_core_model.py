"""`core.model` of GINESignNetPyG for `dropin.install('gine_pyg', baselines=True, feature_dropout=True)`: the plain GNN for every
model.gnn_type that also takes `train.dropout > 0` (dropout_models.GNN), behind the reference's constructor (core/model.py:11)."""
from ..dropout_models import GNN  # noqa: F401
