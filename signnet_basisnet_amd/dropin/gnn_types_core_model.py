"""`core.model` of GINESignNetPyG for `dropin.install('gine_pyg', baselines=True, gnn_types=True)`: the plain GNN that train/zinc.py:31-46
builds when model.gnn_type is not 'SignNet', for all five wrappers of core/model_utils/pyg_gnn_wrapper.py, behind the reference's
constructor (core/model.py:11).  Without gnn_types=True the name stays bound to `baseline_core_model` (GINEConv only)."""
from ..pyg_gnn_types import GNN  # noqa: F401
