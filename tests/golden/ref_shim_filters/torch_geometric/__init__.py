"""Stand-in for torch_geometric==2.0.1 (absent), complete for LearningFilters/models.py's spectral baselines: a working
MessagePassing.propagate, gcn_norm, get_laplacian, add_self_loops, ChebConv and GCNConv, all restated from the library's documented
definitions (none of its code is here).  Used only by tests/golden/make_filter_baselines.py, ahead of ../ref_shim on sys.path.
GATConv and ARMAConv stay placeholders: GatNet / ARMANet are not built."""
