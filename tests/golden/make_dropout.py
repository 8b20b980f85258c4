"""Regenerates tests/golden/dropout_*.npz: the reference's own modules in TRAIN mode with dropout 0.25, the masks drawn by the
counter-based generator of csrc/dropout.hip instead of torch's.  torch.nn.functional.dropout and nn.Dropout.forward are replaced, for
the duration of a forward, by the numpy restatement of the mask contract (tests/dropout_cases.keep_mask): call number s of a forward
is site s, the logical [R, C] shape is the tensor's (C = its last dimension), (seed, step) are fixed.  Everything else — shims, graphs,
helpers, the scaled-down nets — is make_pyg_baselines.py's, make_gnn_types.py's and make_baseline_pe.py's.  Arrays only.

    python tests/golden/make_dropout.py      # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

  dropout_<case>   state_dict (BatchNorm buffers randomised), batch, cotangent; the eval output (dropout is the identity there); the
                   train-mode output, the gradient of sum(y * cotangent) w.r.t. every parameter and the BatchNorm buffers afterwards, from
                   the reference in float32 (the DGL nets: without the float32 gradients, which their tolerance rule does not read) — and
                   output and gradients once more from the same module in float64 (`y64`, `grad64/`), the yardstick of the project's
                   tolerance rules; the masks drawn (bit-packed, site order) with their parameters, which
                   tests/test_dropout_cases_cpu.py checks against the generator
"""
from __future__ import annotations

import contextlib
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, data_arrays, randomise, save, sd_arrays, synth  # noqa: E402
import make_baseline_pe  # noqa: E402
import make_gnn_types  # noqa: E402
import make_pyg_baselines  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import dropout_cases as DC  # noqa: E402
import gnn_type_cases as GC  # noqa: E402

P, SEED, STEP = 0.25, 20240607, 3

# name -> (gnn_type, nhid, nlayer, pooling, graph sizes, seed): the plain GNN of GINESignNetPyG (core/model.py)
PLAIN_GNN = {
    "dropout_plain_gnn_gine_h16_l2_add": ("GINEConv", 16, 2, "add", [5, 9, 12, 7, 3], 161),
    "dropout_plain_gnn_gcn_h16_l2_mean": ("GCNConv", 16, 2, "mean", [6, 4, 11, 2, 9], 162),
}


# the five DGL base nets at pe_init 'no_pe', the scaled-down nets of make_baseline_pe.py: name -> (net, in_feat_dropout, dropout)
DGL_NETS = {
    "dropout_gatedgcn_nope": ("gatedgcn", P, P),
    "dropout_gin_nope": ("gin", P, P),
    "dropout_pna_nope": ("pna", P, P),
    "dropout_transformer_nope": ("transformer", P, P),
    "dropout_gat_nope": ("gat", P, 0.0),           # (gat_net.py reads `dropout` and never uses it)
}


class Sites:
    """The stand-in of F.dropout / nn.Dropout.forward: site = the ordinal of the call within one forward."""

    def __init__(self):
        self.masks = []

    def reset(self):
        self.masks = []

    def __call__(self, x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        assert p > 0.0, "a site with p = 0 would still take an ordinal: build the fixtures with every site active"
        C = x.shape[-1]
        keep = DC.keep_mask(x.numel() // C, C, p, SEED, STEP, len(self.masks))
        self.masks.append(keep)
        return x * (torch.from_numpy(keep).to(x.dtype) * float(DC.scale_of(p))).view(x.shape)


@contextlib.contextmanager
def patched(sites):
    import torch.nn.functional as F
    old_f, old_m = F.dropout, torch.nn.Dropout.forward
    F.dropout = sites
    torch.nn.Dropout.forward = lambda self, x: sites(x, self.p, self.training, self.inplace)
    sites.reset()
    try:
        yield sites
    finally:
        F.dropout, torch.nn.Dropout.forward = old_f, old_m


def train_arrays(model, forward, cot, grad32=True):
    """Train-mode forward + backward of `model` (float32) and of a float64 copy made before it ran; the eval output first."""
    arrays = {}
    model64 = copy.deepcopy(model).double()
    sites = Sites()
    model.eval()
    with torch.no_grad(), patched(sites):
        arrays["out/eval/y"] = forward(model, torch.float32).numpy()
    assert not sites.masks
    for m, dtype, tag in ((model, torch.float32, ""), (model64, torch.float64, "64")):
        m.train()
        with patched(sites):
            y = forward(m, dtype)
            (y * cot.to(dtype)).sum().backward()
        arrays[f"out/train/y{tag}"] = y.detach().numpy()
        for k, p in m.named_parameters():
            if p.grad is not None and ".layer.nn." not in k and (tag or grad32):
                arrays[f"out/train/grad{tag}/" + k] = p.grad.detach().numpy()
        if not tag:
            for k, v in m.state_dict().items():
                if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked") and ".layer.nn." not in k:
                    arrays["out/train/buffers/" + k] = v.detach().clone().numpy()
            masks = list(sites.masks)
    assert masks and all((a == b).all() for a, b in zip(masks, sites.masks)) and len(masks) == len(sites.masks)
    arrays["meta/dropout_seed"] = np.array(SEED, dtype=np.int64)
    arrays["meta/dropout_step"] = np.array(STEP, dtype=np.int64)
    arrays["meta/dropout_p"] = np.array(P, dtype=np.float64)
    arrays["meta/dropout_site_shapes"] = np.array([k.shape for k in masks], dtype=np.int64)
    for s, k in enumerate(masks):
        arrays[f"out/dropout_mask/{s}"] = np.packbits(k.reshape(-1))
    return arrays


def plain_gnn_case(name, gnn_type, nhid, nlayer, pooling, sizes, seed):
    mod = make_pyg_baselines._import("GINESignNetPyG", "core.model") if gnn_type == "GINEConv" else make_gnn_types._import("core.model")
    torch.manual_seed(seed)
    model = mod.GNN(None, None, nhid, 1, nlayer, gnn_type, P, pooling, res=True)        # train/zinc.py:38-46 with train.dropout
    randomise(model, seed + 1)
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    if gnn_type != "GINEConv":
        data = GC.odd_edges(data)
    cot = torch.randn(len(sizes), 1, generator=torch.Generator().manual_seed(seed + 3))
    arrays = {**sd_arrays(model), **data_arrays(data), "in/cotangent": cot.numpy(), "meta/nhid_nlayer": np.array([nhid, nlayer], dtype=np.int64),
              "meta/pooling": np.array(pooling), "meta/gnn_type": np.array(gnn_type)}
    arrays.update(train_arrays(model, lambda m, dtype: m(data), cot))
    save(name, **arrays)


def dgl_case(name, net_name, p_in, p_drop):
    net, data, sn, meta = make_baseline_pe._build(net_name, pe_init="no_pe", lap_method="none", pe_aggregate="none",
                                                  in_feat_dropout=p_in, dropout=p_drop)
    if net_name == "transformer":          # transformer_net.py:68-69 never hands `dropout` to its layers: set on the layers themselves
        for L in net.layers:
            L.dropout = p_drop
    cot = torch.randn(len(data.sizes), 1, generator=torch.Generator().manual_seed(7))
    arrays = {**sd_arrays(net), **data_arrays(data), **meta, "in/cotangent": cot.numpy(),
              "meta/p_in_feat_p_drop": np.array([p_in, p_drop], dtype=np.float64)}
    if sn is not None:
        arrays["in/snorm_n"] = sn.numpy()

    def forward(m, dtype):
        g = make_baseline_pe._graph(data)
        return m(g, data.x.squeeze(-1), None, data.edge_attr, None if sn is None else sn.to(dtype))[0]

    arrays.update(train_arrays(net, forward, cot, grad32=False))      # (this family's gradient rule compares with float64 alone)
    save(name, **arrays)


def main():
    for name, args in PLAIN_GNN.items():
        plain_gnn_case(name, *args)
    for name, args in DGL_NETS.items():
        dgl_case(name, *args)


if __name__ == "__main__":
    main()
