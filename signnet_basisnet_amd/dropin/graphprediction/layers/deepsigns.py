"""`from layers.deepsigns import GCNDeepSigns, GINDeepSigns, MaskedGINDeepSigns, TransformerDeepSigns`
(GraphPrediction/nets/.../sign_inv_net.py:1)."""
from signnet_basisnet_amd.dgl_deepsigns import (GCN, GIN, MLP, GCNDeepSigns, GINDeepSigns, MaskedGINDeepSigns,  # noqa: F401
                                                TransformerDeepSigns)
