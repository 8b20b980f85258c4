"""torch_geometric.nn as LearningFilters/models.py imports it (models.py:9-11)."""
import torch

from .conv import ChebConv, GCNConv, MessagePassing  # noqa: F401


class _NotBuilt(torch.nn.Module):
    def __init__(self, *a, **k):
        raise NotImplementedError("stand-in: GATConv / ARMAConv are not restated (GatNet and ARMANet are not built)")


GATConv = ARMAConv = _NotBuilt
