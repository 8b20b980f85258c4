"""Stand-in for torch_geometric==2.0.1 (absent) with working GATConv and ARMAConv, for tests/golden/make_filter_attention.py only.
Everything else — MessagePassing, gcn_norm, get_laplacian, add_self_loops, ChebConv, GCNConv — is ../ref_shim_filters' stand-in, found
through the extended package paths; that directory keeps its GATConv / ARMAConv placeholders.  All of it is restated from the
library's documented definitions (none of its code is here)."""
import os as _os

__path__.append(_os.path.join(_os.path.dirname(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))), "ref_shim_filters",
                              "torch_geometric"))
