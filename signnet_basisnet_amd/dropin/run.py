"""Run one of the reference's entry scripts, unchanged, on the HIP modules.

    cd <reference>/Alchemy          && python -m signnet_basisnet_amd.dropin.run main_alchemy.py
    cd <reference>/GINESignNetPyG   && python -m signnet_basisnet_amd.dropin.run train/zinc.py model.gnn_type GINEConv ...
    cd <reference>/GraphPrediction  && python -m signnet_basisnet_amd.dropin.run main_ZINC_graph_regression.py --config configs/...
    cd <reference>/LearningFilters  && python -m signnet_basisnet_amd.dropin.run training.py --net DS --use_eig --lap_method basis_inv

The script is executed with `runpy` as `__main__` with its own `sys.argv`; `sys.path[0]` is the script's directory as under
`python script.py` (the working directory stays where the caller is: the scripts open `data/...`, `configs/...` relative to it,
and GINESignNetPyG's README runs `python -m train.zinc` from the tree root, which is why '' stays on the path too).  The only
difference to a plain run is the finder of `dropin.install(tree)`: the names listed in `dropin.ALIASES[tree]` come from this
package, everything else from the tree.  `--tree` overrides the guess from the script's file name.  `--baselines` (before the script)
also binds the trees' baseline models, `dropin.BASELINE_ALIASES`: `baseline_gin` (NetGINE) and `core.model` (the plain GINE GNN of
`model.gnn_type GINEConv`); without it both stay the tree's.  For LearningFilters it rebinds `models`
(`dropin.BASELINE_OVERRIDES`) so that BernNet, GPRNet, ChebNet and GcnNet are the HIP classes of `filter_baselines.py`.
`--baselines=all` binds GatNet and ARMANet as well (`dropin.ALL_BASELINE_OVERRIDES`):

    cd <reference>/LearningFilters  && python -m signnet_basisnet_amd.dropin.run --baselines=all training.py --net GatNet

`--gnn-types` (with `--baselines`) rebinds GINESignNetPyG's `core.model` (`dropin.GNN_TYPE_OVERRIDES`) to the plain GNN for every
`model.gnn_type` — GINConv, GCNConv, GATConv and SimplifiedPNAConv next to GINEConv:

    cd <reference>/GINESignNetPyG   && python -m signnet_basisnet_amd.dropin.run --baselines --gnn-types -m train.zinc model.gnn_type SimplifiedPNAConv

`--feature-dropout` rebinds the names of `dropin.FEATURE_DROPOUT_OVERRIDES` to the models that take train-mode dropout
(`dropout_models.py`): GraphPrediction's five base nets with `--dropout` / `--in_feat_dropout`, and GINESignNetPyG's `core.model` (every
`model.gnn_type`) with `train.dropout`; without it a non-zero dropout is refused as before:

    cd <reference>/GraphPrediction  && python -m signnet_basisnet_amd.dropin.run --feature-dropout main_ZINC_graph_regression.py --config configs/gatedgcn/GatedGCN_ZINC_NoPE.json --dropout 0.1

`--sign-inv-dropout` (implies `--feature-dropout`) rebinds the names of `dropin.SIGN_INV_DROPOUT_OVERRIDES` on top: GraphPrediction's five
base nets and `nets.ZINC_graph_regression.sign_inv_net` from `dropout_signinv.py`, so `--dropout` also reaches the sign-invariant encoder
(`lap_method` 'sign_inv'), as in the reference; without it that combination is refused as before:

    cd <reference>/GraphPrediction  && python -m signnet_basisnet_amd.dropin.run --sign-inv-dropout main_ZINC_graph_regression.py --config configs/gatedgcn/GatedGCN_ZINC_LapPE_signinv_GIN.json --dropout 0.1

`--max-readout` (implies `--sign-inv-dropout`) rebinds the names of `dropin.MAX_READOUT_OVERRIDES` on top: GraphPrediction's five base nets
from `readout_models.py`, which take `--readout max` (dgl.max_nodes) next to `sum` / `mean`; without it `max` is refused as before:

    cd <reference>/GraphPrediction  && python -m signnet_basisnet_amd.dropin.run --max-readout main_ZINC_graph_regression.py --config configs/gatedgcn/GatedGCN_ZINC_NoPE.json --readout max

`--sign-inv-activation` (implies `--max-readout`) rebinds the names of `dropin.SIGN_INV_ACTIVATION_OVERRIDES` on top: GraphPrediction's five
base nets, `nets.ZINC_graph_regression.sign_inv_net` and `layers.deepsigns` from `activation_signinv.py`, whose sign-invariant encoders take
`--sign_inv_activation tanh` (and `elu` where the reference's own classes take it: the Transformer encoder); without it anything but `relu`
is refused as before:

    cd <reference>/GraphPrediction  && python -m signnet_basisnet_amd.dropin.run --sign-inv-activation main_ZINC_graph_regression.py --config configs/gatedgcn/GatedGCN_ZINC_LapPE_signinv_GIN.json --sign_inv_activation tanh

`--attn-dropout=counter` makes "counter" the `attn_dropout_source` of every `pyg.SignNetGNN` the run constructs (Alchemy, GINESignNetPyG):
the train-mode attention-dropout masks are evaluated inside the attention kernels from (seed, step) — seed torch.initial_seed() unless
the script calls `seed_dropout` — instead of drawn with torch's device generator.
"""
from __future__ import annotations

import os
import runpy
import sys

from . import ALIASES, SCRIPTS, install


def main(argv=None) -> None:
    argv = list(sys.argv[1:] if argv is None else argv)
    tree, baselines, gnn_types, feature_dropout, sign_inv_dropout, max_readout = None, False, False, False, False, False
    more = {}                                       # keywords of install() that are handed on only when their flag is given
    while argv and argv[0].startswith("--"):        # the runner's own options come before the script
        if argv[0] == "--baselines":
            baselines, argv = True, argv[1:]
        elif argv[0] == "--gnn-types":
            gnn_types, argv = True, argv[1:]
        elif argv[0] == "--feature-dropout":
            feature_dropout, argv = True, argv[1:]
        elif argv[0] == "--sign-inv-dropout":
            feature_dropout, sign_inv_dropout, argv = True, True, argv[1:]
        elif argv[0] == "--max-readout":
            feature_dropout, sign_inv_dropout, max_readout, argv = True, True, True, argv[1:]
        elif argv[0] == "--sign-inv-activation":
            feature_dropout, sign_inv_dropout, max_readout, argv = True, True, True, argv[1:]
            more["sign_inv_activation"] = True
        elif argv[0].startswith("--attn-dropout="):
            from ..pyg import SignNetGNN
            try:
                SignNetGNN.DEFAULT_ATTN_DROPOUT_SOURCE = SignNetGNN.check_attn_dropout_source(argv[0].split("=", 1)[1])
            except ValueError as e:
                raise SystemExit(f"{argv[0]}: {e}")
            argv = argv[1:]
        elif argv[0].startswith("--baselines="):
            value = argv[0].split("=", 1)[1]
            if value != "all":
                raise SystemExit(f"--baselines={value}: the only value is 'all' (plain --baselines binds the built baselines without GatNet / ARMANet)")
            baselines, argv = "all", argv[1:]
        elif argv[0] == "--tree":
            if len(argv) < 2:
                raise SystemExit("--tree needs a value: " + ", ".join(sorted(ALIASES)))
            tree, argv = argv[1], argv[2:]
        elif argv[0].startswith("--tree="):
            tree, argv = argv[0].split("=", 1)[1], argv[1:]
        else:
            break
    if not argv:
        raise SystemExit("usage: python -m signnet_basisnet_amd.dropin.run [--tree T] [--baselines[=all]] [--gnn-types] [--feature-dropout] [--sign-inv-dropout] [--max-readout] [--sign-inv-activation] [--attn-dropout=counter] <entry script> "
                         "[script arguments ...]\n"
                         "trees: " + ", ".join(f"{t} ({s})" for s, t in SCRIPTS.items()))
    if argv[0] == "-m":
        # `-m package.module` from the tree root, as GINESignNetPyG's README runs `python -m train.zinc`: the module is found on sys.path
        # (the working directory first) and run as __main__
        if len(argv) < 2:
            raise SystemExit("-m needs a module name, e.g. -m train.zinc")
        module = argv[1]
        if tree is None:
            tree = SCRIPTS.get(module.rsplit(".", 1)[-1] + ".py")
            if tree is None:
                raise SystemExit(f"cannot tell the reference tree from the module {module!r}; pass --tree " + "|".join(sorted(ALIASES)))
        install(tree, baselines=baselines, gnn_types=gnn_types, feature_dropout=feature_dropout, sign_inv_dropout=sign_inv_dropout,
                max_readout=max_readout, **more)
        if os.getcwd() in sys.path:
            sys.path.remove(os.getcwd())
        sys.path.insert(0, os.getcwd())
        sys.argv = [module] + argv[2:]
        runpy.run_module(module, run_name="__main__", alter_sys=True)
        return
    script = argv[0]
    if not os.path.isfile(script):
        raise SystemExit(f"{script}: no such entry script (run from the reference tree, as the script's README says)")
    if tree is None:
        tree = SCRIPTS.get(os.path.basename(script))
        if tree is None:
            raise SystemExit(f"cannot tell the reference tree from {os.path.basename(script)!r}; pass --tree " + "|".join(sorted(ALIASES)))
    install(tree, baselines=baselines, gnn_types=gnn_types, feature_dropout=feature_dropout, sign_inv_dropout=sign_inv_dropout,
                max_readout=max_readout, **more)
    script_dir = os.path.dirname(os.path.abspath(script))
    for p in (os.getcwd(), script_dir):          # script_dir ends up first, as under `python script.py`
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    sys.argv = [script] + argv[1:]
    runpy.run_path(script, run_name="__main__")


if __name__ == "__main__":
    main()
