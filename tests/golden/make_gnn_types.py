"""Regenerates tests/golden/gnn_types_*.npz: GINESignNetPyG's plain GNN (core/model.py) for the gnn_type values GINConv, GCNConv, GATConv
and SimplifiedPNAConv, run through the ORIGINAL code — core/model.py over core/model_utils/pyg_gnn_wrapper.py, imported unchanged — on
CPU.  The graph library comes from tests/golden/ref_shim_gnn_types/ (a MessagePassing with an overridable aggregate, GCNConv, GATConv,
torch_scatter.scatter with add / mean / min / max) in front of tests/golden/ref_shim/.  Arrays only; the helpers are make_golden.py's,
the case list is tests/gnn_type_cases.py's.

    python tests/golden/make_gnn_types.py      # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

  gnn_types_<case>   state_dict (BatchNorm buffers randomised), batch (a molecule batch plus a directed edge, a duplicated edge and two
                     self loops: gnn_type_cases.odd_edges), [additional_x], eval and train-mode outputs, every BatchNorm buffer after the
                     train-mode forward (the never-called norms.1 of SimplifiedPNAConv's two MLPs included)
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, SHIM, data_arrays, randomise, save, sd_arrays, synth  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import gnn_type_cases as C  # noqa: E402

SHIM_GNN_TYPES = os.path.join(HERE, "ref_shim_gnn_types")


def _import(name):
    """One module of GINESignNetPyG, with the two stand-in directories ahead of everything."""
    for m in list(sys.modules):
        if m.split(".")[0] in ("core", "torch_geometric", "torch_scatter") or m.startswith("_ref_shim_torch_geometric_"):
            del sys.modules[m]
    sys.path[:0] = [SHIM_GNN_TYPES, SHIM, os.path.join(REF, "GINESignNetPyG")]
    try:
        return importlib.import_module(name)
    finally:
        del sys.path[:3]


def case(name, gnn_type, nhid, nlayer, pooling, with_pe, sizes, seed):
    mod = _import("core.model")
    torch.manual_seed(seed)
    model = mod.GNN(None, None, nhid, 1, nlayer, gnn_type, 0, pooling, res=True)        # train/zinc.py:38-46
    randomise(model, seed + 1)
    data = C.odd_edges(synth.make_batch(len(sizes), seed=seed, sizes=sizes))
    pe = torch.randn(data.num_nodes, nhid, generator=torch.Generator().manual_seed(seed + 2)) if with_pe else None
    arrays = {**sd_arrays(model), **data_arrays(data), "meta/nhid_nlayer": np.array([nhid, nlayer], dtype=np.int64),
              "meta/pooling": np.array(pooling), "meta/gnn_type": np.array(gnn_type)}
    if pe is not None:
        arrays["in/additional_x"] = pe.numpy()
    model.eval()
    with torch.no_grad():
        arrays["out/eval/y"] = model(data, pe).numpy()
    model.train()
    with torch.no_grad():
        arrays["out/train/y"] = model(data, pe).numpy()
    for k, v in model.state_dict().items():
        if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked") and ".layer.nn." not in k:
            arrays["out/train/buffers/" + k] = v.detach().clone().numpy()
    save(name, **arrays)


def main():
    for name, args in C.FIXTURES.items():
        case(name, *args)


if __name__ == "__main__":
    main()
