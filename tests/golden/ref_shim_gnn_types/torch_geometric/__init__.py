"""Stand-in for torch_geometric==2.0.1 in front of ../../ref_shim/torch_geometric: what GINESignNetPyG's core/model.py needs to build
its GNN for every gnn_type of core/model_utils/pyg_gnn_wrapper.py (a MessagePassing with an overridable aggregate, GCNConv, GATConv),
restated from the library's documentation.  Used only by tests/golden/make_gnn_types.py.  `__path__` runs on over the existing stand-in,
so every submodule this directory does not have (nn.inits, nn.conv, ...) is that one's; `_behind` loads the package file this directory
shadows, so its names (GINConv, GINEConv, utils.degree, ...) can be re-exported."""
import importlib.util
import os
import sys

_BEHIND = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "ref_shim", "torch_geometric")
__path__.append(_BEHIND)


def _behind(sub):
    """The existing stand-in's package `torch_geometric.<sub>`, loaded under a private name (its relative imports stay inside it)."""
    name = "_ref_shim_torch_geometric_" + sub
    if name not in sys.modules:
        d = os.path.join(_BEHIND, sub)
        spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]
