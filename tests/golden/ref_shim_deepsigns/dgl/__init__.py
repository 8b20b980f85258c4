"""Stand-in for dgl in front of ../../ref_shim/dgl: what layers/deepsigns.py's GCNDeepSigns and TransformerDeepSigns need on top of it
(dgl.nn.pytorch.GraphConv, dgl.nn.pytorch.glob.SetTransformerEncoder — placeholders there), restated from DGL's published definitions.
Used only by tests/golden/make_deepsigns_variants.py.  `__path__` runs on over the existing stand-in, so every submodule this directory
does not have (function) is that one's; its package file is loaded under a private name and its names re-exported."""
import importlib.util
import os
import sys

_BEHIND = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "ref_shim", "dgl")
__path__.append(_BEHIND)


def _behind():
    name = "_ref_shim_dgl"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(_BEHIND, "__init__.py"), submodule_search_locations=[_BEHIND])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


_behind()          # (nn.pytorch re-exports its GINConv / GATConv)
from . import nn  # noqa: E402,F401
from . import function  # noqa: E402,F401

Graph = _behind().Graph
sum_nodes, mean_nodes, max_nodes = _behind().sum_nodes, _behind().mean_nodes, _behind().max_nodes
