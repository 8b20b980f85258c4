"""Drop-in binding of the reference's entry scripts to the HIP modules.

The reference is pure Python: its "FFI" for this path is the set of dotted module names its entry scripts import
(`Alchemy/main_alchemy.py:20-22`, `GINESignNetPyG/train/zinc.py:2-6`, `GraphPrediction/main_ZINC_graph_regression.py:47`
through `nets/ZINC_graph_regression/load_net.py:6-10`, `LearningFilters/training.py:8-10`).  Two ways to rebind them, both
leaving every file of the reference tree untouched and every OTHER module of the tree (`core.config`, `core.train`,
`core.model`, `layers.mlp_readout_layer`, `nets.ZINC_graph_regression.load_net`, `utils`, `data.*`, `train.*`) importing from the
tree as before:

1. `install(tree)` puts a meta-path finder in front of the import system that answers exactly the names of `ALIASES[tree]` with the
   HIP modules.  It does not depend on the order of `sys.path` (main_alchemy.py:5-6 inserts '.' and '..' at position 0 itself, so
   no PYTHONPATH entry can win there), and it is what the runner uses:

       cd <reference>/GraphPrediction && python -m signnet_basisnet_amd.dropin.run main_ZINC_graph_regression.py --config ...

2. The shim directories next to this file (`alchemy/`, `gine_pyg/`, `graphprediction/`, `learningfilters/`): put ONE of them
   ahead of the tree on `sys.path`.  `sign_net/` and `core/` are regular packages in the reference, so the shim's `__init__.py`
   extends `__path__` over the tree's package of the same name; `layers/` and `nets/` are namespace packages in the reference, so
   the shim has no `__init__.py` there and the portions merge, the shim's modules first.
"""
from __future__ import annotations

import importlib
import importlib.abc
import importlib.machinery
import importlib.util
import os
import sys

_PKG = __name__

# tree -> {dotted name the reference imports: module of this package that provides it}
ALIASES = {
    "alchemy": {
        "sign_net.sign_net": _PKG + ".alchemy.sign_net.sign_net",
        "sign_net.transform": _PKG + ".alchemy.sign_net.transform",
    },
    "gine_pyg": {
        "core.sign_net": _PKG + ".gine_pyg.core.sign_net",
        "core.transform": _PKG + ".gine_pyg.core.transform",
    },
    "graphprediction": {
        "layers.deepsigns": _PKG + ".graphprediction.layers.deepsigns",
        **{"nets.ZINC_graph_regression." + m: _PKG + ".graphprediction.nets.ZINC_graph_regression." + m
           for m in ("sign_inv_net", "gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net")},
    },
    "learningfilters": {
        "models": _PKG + ".learningfilters.models",
        "signbasisnet": _PKG + ".learningfilters.signbasisnet",
        "ign": _PKG + ".learningfilters.ign",
    },
}

# Opt-in (`install(tree, baselines=True)`, the runner's `--baselines`): the trees' BASELINE models — competitors of SignNet that the same
# entry scripts build (Alchemy/main_alchemy.py:24-33, GINESignNetPyG/train/zinc.py:31-46).  Kept apart from ALIASES: they have no shim
# directory entry, and without the flag both names stay the tree's.
BASELINE_ALIASES = {
    "alchemy": {"baseline_gin": "signnet_basisnet_amd.pyg_baselines"},
    "gine_pyg": {"core.model": _PKG + ".baseline_core_model"},
}

# Opt-in with the same flag, for a name ALIASES already answers: the module that answers it INSTEAD.  LearningFilters keeps its baselines
# in the same `models.py` as the base networks (training.py:9), so `models` cannot move into BASELINE_ALIASES; with baselines=True it is
# bound to a module that adds the four polynomial-filter baselines (BernNet, GPRNet, ChebNet, GcnNet: filter_baselines.py) and resolves
# everything else — GatNet and ARMANet included — exactly as `learningfilters/models.py` does.
BASELINE_OVERRIDES = {
    "learningfilters": {"models": _PKG + ".baseline_filter_models"},
}

# Opt-in with `baselines="all"` (the runner's `--baselines=all`), on top of everything baselines=True binds: the module that answers the
# name INSTEAD of BASELINE_OVERRIDES' one.  For LearningFilters it adds GatNet and ARMANet, the last two nets of training.py's --net.
ALL_BASELINE_OVERRIDES = {
    "learningfilters": {"models": _PKG + ".all_baseline_filter_models"},
}


# Opt-in with `gnn_types=True` (the runner's `--gnn-types`), on top of whatever `baselines` binds: the module that answers the name INSTEAD.
# For GINESignNetPyG it is `core.model` with the plain GNN for every model.gnn_type (GINConv, GCNConv, GATConv, SimplifiedPNAConv next
# to GINEConv: pyg_gnn_types.py); without the flag `core.model` resolves exactly as before.
GNN_TYPE_OVERRIDES = {
    "gine_pyg": {"core.model": _PKG + ".gnn_types_core_model"},
}


# Opt-in with `feature_dropout=True` (the runner's `--feature-dropout`), on top of the flags above: the modules whose models take train-mode
# dropout (dropout_models.py).  GINESignNetPyG: `core.model` with the plain GNN for every model.gnn_type and `train.dropout > 0`;
# GraphPrediction: the five base nets with `--dropout` / `--in_feat_dropout`.  Without the flag every name resolves exactly as before.
FEATURE_DROPOUT_OVERRIDES = {
    "gine_pyg": {"core.model": _PKG + ".dropout_core_model"},
    "graphprediction": {"nets.ZINC_graph_regression." + m: _PKG + ".dropout_nets"
                        for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net")},
}


# Opt-in with `sign_inv_dropout=True` (the runner's `--sign-inv-dropout`; implies feature_dropout), on top of the flags above: the base
# nets AND the sign-invariant encoder in front of them take `--dropout` (dropout_signinv.py), so `--lap_method sign_inv --dropout 0.1`
# trains.  Without the flag every name — `nets.ZINC_graph_regression.sign_inv_net` included — resolves exactly as before.
SIGN_INV_DROPOUT_OVERRIDES = {
    "graphprediction": {"nets.ZINC_graph_regression." + m: _PKG + ".signinv_dropout_nets"
                        for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net", "sign_inv_net")},
}


# Opt-in with `max_readout=True` (the runner's `--max-readout`; implies sign_inv_dropout), on top of the flags above: the five base nets
# from readout_models.py, which take `--readout max` next to `sum` / `mean`.  Without the flag every name resolves exactly as before and
# `max` is refused as before.
MAX_READOUT_OVERRIDES = {
    "graphprediction": {"nets.ZINC_graph_regression." + m: _PKG + ".max_readout_nets"
                        for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net")},
}


# Opt-in with `sign_inv_activation=True` (the runner's `--sign-inv-activation`; implies max_readout), on top of the flags above: the five
# base nets, `nets.ZINC_graph_regression.sign_inv_net` and `layers.deepsigns` from activation_signinv.py, whose sign-invariant encoders
# take `--sign_inv_activation tanh` (and `elu` where the reference's own classes do).  Without the flag every name resolves exactly as
# before and anything but `relu` is refused as before.
SIGN_INV_ACTIVATION_OVERRIDES = {
    "graphprediction": {**{"nets.ZINC_graph_regression." + m: _PKG + ".signinv_activation_nets"
                           for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net", "sign_inv_net")},
                        "layers.deepsigns": _PKG + ".signinv_activation_layers"},
}


def _baseline_table(tree: str, baselines, gnn_types=False, feature_dropout=False, sign_inv_dropout=False, max_readout=False,
                    sign_inv_activation=False) -> dict:
    """What `baselines` (False, True or "all"), `gnn_types`, `feature_dropout`, `sign_inv_dropout`, `max_readout` and
    `sign_inv_activation` add to ALIASES[tree]."""
    max_readout = max_readout or sign_inv_activation
    if baselines not in (False, True, "all"):
        raise ValueError(f"baselines must be False, True or 'all', got {baselines!r}")
    table = {}
    if baselines:
        table.update(BASELINE_ALIASES.get(tree, {}))
        table.update(BASELINE_OVERRIDES.get(tree, {}))
    if baselines == "all":
        table.update(ALL_BASELINE_OVERRIDES.get(tree, {}))
    if gnn_types:
        table.update(GNN_TYPE_OVERRIDES.get(tree, {}))
    if feature_dropout or sign_inv_dropout or max_readout:
        table.update(FEATURE_DROPOUT_OVERRIDES.get(tree, {}))
    if sign_inv_dropout or max_readout:
        table.update(SIGN_INV_DROPOUT_OVERRIDES.get(tree, {}))
    if max_readout:
        table.update(MAX_READOUT_OVERRIDES.get(tree, {}))
    if sign_inv_activation:
        table.update(SIGN_INV_ACTIVATION_OVERRIDES.get(tree, {}))
    return table


# entry script (basename) -> tree, for the runner
SCRIPTS = {
    "main_alchemy.py": "alchemy",
    "zinc.py": "gine_pyg",
    "main_ZINC_graph_regression.py": "graphprediction",
    "training.py": "learningfilters",
}


def shim_dir(tree: str) -> str:
    if tree not in ALIASES:
        raise KeyError(f"unknown reference tree {tree!r}; one of {sorted(ALIASES)}")
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), tree)


class _AliasLoader(importlib.abc.Loader):
    def __init__(self, target: str):
        self.target = target

    def create_module(self, spec):
        return None

    def exec_module(self, module):
        impl = importlib.import_module(self.target)
        keep = {"__name__", "__spec__", "__loader__", "__package__", "__path__", "__file__", "__cached__"}
        for k, v in vars(impl).items():
            if k not in keep:
                module.__dict__[k] = v
        module.__dict__["__signnet_hip__"] = self.target
        module.__dict__.setdefault("__file__", getattr(impl, "__file__", None))


class AliasFinder(importlib.abc.MetaPathFinder):
    """Answers the names of `ALIASES[tree]` and nothing else; every other import goes on to the normal finders."""

    def __init__(self, tree: str, baselines=False, gnn_types=False, feature_dropout=False, sign_inv_dropout=False, max_readout=False,
                 sign_inv_activation=False):
        self.tree = tree
        self.table = dict(ALIASES[tree])
        self.table.update(_baseline_table(tree, baselines, gnn_types, feature_dropout, sign_inv_dropout, max_readout, sign_inv_activation))

    def find_spec(self, fullname, path=None, target=None):
        impl = self.table.get(fullname)
        if impl is None:
            return None
        return importlib.machinery.ModuleSpec(fullname, _AliasLoader(impl), origin=impl)


def install(tree: str, baselines=False, gnn_types=False, feature_dropout=False, sign_inv_dropout=False, max_readout=False,
            sign_inv_activation=False) -> AliasFinder:
    """Route the reference's module names of `tree` to the HIP modules.  Idempotent per tree.  baselines=True also routes the names of
    `BASELINE_ALIASES[tree]` (NetGINE / the plain GINE GNN) and rebinds those of `BASELINE_OVERRIDES[tree]` (LearningFilters' `models`, with
    the four polynomial-filter baselines); baselines="all" rebinds those of `ALL_BASELINE_OVERRIDES[tree]` on top (LearningFilters'
    `models` with GatNet and ARMANet too); gnn_types=True rebinds those of `GNN_TYPE_OVERRIDES[tree]` (GINESignNetPyG's `core.model` with
    the plain GNN for every model.gnn_type); feature_dropout=True rebinds those of `FEATURE_DROPOUT_OVERRIDES[tree]` (the models that take
    train-mode dropout); sign_inv_dropout=True implies feature_dropout and rebinds those of `SIGN_INV_DROPOUT_OVERRIDES[tree]` on top
    (GraphPrediction's base nets and `sign_inv_net` with dropout in the sign-invariant encoder too); max_readout=True implies
    sign_inv_dropout and rebinds those of `MAX_READOUT_OVERRIDES[tree]` on top (GraphPrediction's base nets with `--readout max`);
    sign_inv_activation=True implies max_readout and rebinds those of `SIGN_INV_ACTIVATION_OVERRIDES[tree]` on top (GraphPrediction's base
    nets, `sign_inv_net` and `layers.deepsigns` with `--sign_inv_activation tanh | elu`); a finder installed with less is extended in place."""
    shim_dir(tree)
    extra = _baseline_table(tree, baselines, gnn_types, feature_dropout, sign_inv_dropout, max_readout, sign_inv_activation)
    for f in sys.meta_path:
        if isinstance(f, AliasFinder) and f.tree == tree:
            for name, impl in extra.items():
                bound_for_all = ALL_BASELINE_OVERRIDES.get(tree, {}).get(name)
                if bound_for_all is not None and f.table.get(name) == bound_for_all:
                    continue                    # already bound for "all": a later baselines=True takes nothing away
                bound_for_types = GNN_TYPE_OVERRIDES.get(tree, {}).get(name)
                if bound_for_types is not None and f.table.get(name) == bound_for_types:
                    continue                    # already bound for gnn_types: a later call without the flag takes nothing away
                bound_for_dropout = FEATURE_DROPOUT_OVERRIDES.get(tree, {}).get(name)
                bound_for_signinv = SIGN_INV_DROPOUT_OVERRIDES.get(tree, {}).get(name)
                bound_for_max = MAX_READOUT_OVERRIDES.get(tree, {}).get(name)
                bound_for_act = SIGN_INV_ACTIVATION_OVERRIDES.get(tree, {}).get(name)
                if bound_for_act is not None and f.table.get(name) == bound_for_act:
                    continue                    # already bound for sign_inv_activation: a later call with less takes nothing away
                if bound_for_max is not None and f.table.get(name) == bound_for_max and impl != bound_for_act:
                    continue                    # likewise for max_readout
                if bound_for_signinv is not None and f.table.get(name) == bound_for_signinv and impl not in (bound_for_max, bound_for_act):
                    continue                    # likewise for sign_inv_dropout
                if bound_for_dropout is not None and f.table.get(name) == bound_for_dropout and \
                        impl not in (bound_for_signinv, bound_for_max, bound_for_act):
                    continue                    # likewise for feature_dropout
                if f.table.get(name) != impl:
                    f.table[name] = impl
                    sys.modules.pop(name, None)
            return f
    finder = AliasFinder(tree, baselines, gnn_types, feature_dropout, sign_inv_dropout, max_readout, sign_inv_activation)
    sys.meta_path.insert(0, finder)
    for name in finder.table:           # a module imported before install() would otherwise stay bound to the tree's file
        sys.modules.pop(name, None)
    return finder


def uninstall(tree: str | None = None) -> None:
    for f in list(sys.meta_path):
        if isinstance(f, AliasFinder) and (tree is None or f.tree == tree):
            sys.meta_path.remove(f)
            for name in f.table:
                sys.modules.pop(name, None)


def reference_module(name: str, exclude_dir: str):
    """The module `name` as the NEXT location on `sys.path` (not `exclude_dir`) provides it, loaded under a private name.

    Used by `learningfilters/models.py` to hand the spectral baselines of `training.py:9` (ChebNet, BernNet, ...) on to the
    reference's own `models.py`: they are competitors of the path, not part of it, and stay the reference's code.
    """
    private = "_signnet_reference_" + name.replace(".", "_")
    if private in sys.modules:
        return sys.modules[private]
    exclude = os.path.realpath(exclude_dir)
    search = [p for p in sys.path if os.path.realpath(p or os.getcwd()) != exclude]
    spec = importlib.machinery.PathFinder.find_spec(name, search)
    if spec is None or spec.loader is None or not spec.origin or os.path.realpath(os.path.dirname(spec.origin)) == exclude:
        return None
    spec = importlib.util.spec_from_file_location(private, spec.origin)
    module = importlib.util.module_from_spec(spec)
    sys.modules[private] = module
    try:
        spec.loader.exec_module(module)
    except BaseException:
        sys.modules.pop(private, None)
        raise
    return module
