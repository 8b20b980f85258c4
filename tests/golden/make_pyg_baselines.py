"""Regenerates tests/golden/netgine_*.npz and tests/golden/plain_gnn_*.npz: the BASELINE models of the two PyG trees run through the
ORIGINAL code — Alchemy/baseline_gin.py (NetGINE) and GINESignNetPyG/core/model.py (GNN with gnn_type 'GINEConv', no positional
encoding) — on CPU.  The graph library comes from tests/golden/ref_shim_baselines/ (MessagePassing.propagate, Set2Set, softmax) in
front of tests/golden/ref_shim/.  Arrays only; the helpers are make_golden.py's.

    python tests/golden/make_pyg_baselines.py      # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

  netgine_d<dim>         state_dict, batch, target, eval output, the L1 loss at the first and second Adam step (main_alchemy.py:92,102)
  netgine_d<dim>_grads   the reference's own autograd gradient of every parameter at the first step
  plain_gnn_<case>       state_dict, batch, [additional_x], eval and train-mode outputs, the BatchNorm buffers after the train-mode forward
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, SHIM, data_arrays, randomise, save, sd_arrays, synth  # noqa: E402

SHIM_BASELINES = os.path.join(HERE, "ref_shim_baselines")
LR, WEIGHT_DECAY = 1e-3, 1e-5          # main_alchemy.py:92

# name -> (dim, graph sizes (a one-node graph among them), seed)
NETGINE = {
    "netgine_d16": (16, [7, 1, 12, 9, 6], 51),
    "netgine_d64": (64, [9, 14, 1, 6, 11, 8], 52),
}
# name -> (nhid, nlayer, pooling, additional_x given, graph sizes, seed)
PLAIN_GNN = {
    "plain_gnn_h16_l2_add": (16, 2, "add", False, [5, 9, 12, 7, 3], 61),
    "plain_gnn_h16_l4_mean": (16, 4, "mean", False, [6, 4, 11, 2, 9], 62),
    "plain_gnn_h32_l2_mean_pe": (32, 2, "mean", True, [5, 9, 12, 7, 3], 63),
    "plain_gnn_h32_l4_add_pe": (32, 4, "add", True, [6, 4, 11, 2, 9], 64),
}


def _import(tree, name):
    """One reference module from one tree, with the two stand-in directories ahead of everything."""
    for m in list(sys.modules):
        if m.split(".")[0] in ("core", "baseline_gin", "torch_geometric", "torch_scatter") or m.startswith("_ref_shim_torch_geometric_"):
            del sys.modules[m]
    sys.path[:0] = [SHIM_BASELINES, SHIM, os.path.join(REF, tree)]
    try:
        return importlib.import_module(name)
    finally:
        del sys.path[:3]


def netgine_case(name, dim, sizes, seed):
    mod = _import("Alchemy", "baseline_gin")
    torch.manual_seed(seed)
    model = mod.NetGINE(dim)
    randomise(model, seed + 1)           # (the six eps)
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes, features="alchemy")
    target = torch.randn(len(sizes), 12, generator=torch.Generator().manual_seed(seed + 2))
    arrays = {**sd_arrays(model), **data_arrays(data), "in/y_target": target.numpy(), "meta/dim": np.array(dim, dtype=np.int64),
              "meta/lr_wd": np.array([LR, WEIGHT_DECAY])}
    model.eval()
    with torch.no_grad():
        arrays["out/eval/y"] = model(data).numpy()
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WEIGHT_DECAY)
    lf = torch.nn.L1Loss()
    losses, grads = [], {}
    for step in range(2):
        opt.zero_grad()
        loss = lf(model(data), target)
        loss.backward()
        if step == 0:
            grads = {"out/grad/" + k: p.grad.detach().clone().numpy() for k, p in model.named_parameters()}
        opt.step()
        losses.append(float(loss.detach()))
    arrays["out/loss"] = np.array(losses, dtype=np.float64)
    save(name, **arrays)
    save(name + "_grads", **grads)


def plain_gnn_case(name, nhid, nlayer, pooling, with_pe, sizes, seed):
    mod = _import("GINESignNetPyG", "core.model")
    torch.manual_seed(seed)
    model = mod.GNN(None, None, nhid, 1, nlayer, "GINEConv", 0, pooling, res=True)        # train/zinc.py:38-46
    randomise(model, seed + 1)
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    pe = torch.randn(data.num_nodes, nhid, generator=torch.Generator().manual_seed(seed + 2)) if with_pe else None
    arrays = {**sd_arrays(model), **data_arrays(data), "meta/nhid_nlayer": np.array([nhid, nlayer], dtype=np.int64),
              "meta/pooling": np.array(pooling)}
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
    for name, (dim, sizes, seed) in NETGINE.items():
        netgine_case(name, dim, sizes, seed)
    for name, args in PLAIN_GNN.items():
        plain_gnn_case(name, *args)


if __name__ == "__main__":
    main()
