"""Regenerates tests/golden/ds_gcn_*.npz and tests/golden/ds_tf_*.npz: GCNDeepSigns and TransformerDeepSigns of the DGL tree run through
the ORIGINAL code (GraphPrediction/layers/deepsigns.py over layers/gnns.py, layers/mlp.py) on CPU.  The graph library comes from
tests/golden/ref_shim_deepsigns/ (GraphConv, SetTransformerEncoder restated from DGL's published definitions) in front of
tests/golden/ref_shim/.  Arrays only; the helpers are make_golden.py's.

    python tests/golden/make_deepsigns_variants.py      # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

Every fixture: the seeded state_dict (BatchNorm running statistics and affines randomised), the batch and its positional encoding, the
eval output, the train-mode output and the BatchNorm buffers after that ONE train-mode forward, and the reference's own autograd
gradient of every parameter for the fixed cotangent `in/cotangent` (train mode, loss = sum(y * cotangent)).
"""
from __future__ import annotations

import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import HERE, REF, SHIM, data_arrays, randomise, save, sd_arrays, synth  # noqa: E402

SHIM_DEEPSIGNS = os.path.join(HERE, "ref_shim_deepsigns")

# name -> (class, hidden, out, layers, k, graph sizes, seed).  GCN: no graph without edges (GraphConv raises for a zero-in-degree node),
# out < hidden (the weight in front of the last aggregation), out > hidden (behind it), an odd width; Transformer: a one-node graph,
# head widths 8 and 7 (hidden 15: heads * d_head = 14 != d_model).
# The seeds are those, of 15-40 tried per case, at which the REFERENCE's own fp32 train-mode output and gradients lie closest to their
# float64 values (1e-6 .. 4e-6 relative): rho's train-mode BatchNorm runs over the batch's ~40 node rows, and a channel that is nearly
# constant on them amplifies every rounding in front of it.  For the same reason the Transformer cases scale `embed.weight` by
# EMBED_SCALE: with nn.Linear(1, hidden)'s initial weight every row of embed(x) is the bias plus a few percent (|x| ~ 0.1), the
# encoder's output is nearly the same row for every node, and the reference's fp32 gradients are then 1e-2 from float64.
EMBED_SCALE = 8.0
CASES = {
    "ds_gcn_h16_c4_l3_k4": ("GCNDeepSigns", 16, 4, 3, 4, [5, 9, 12, 7, 3, 6], 291),
    "ds_gcn_h19_c3_l2_k5": ("GCNDeepSigns", 19, 3, 2, 5, [6, 4, 11, 2, 9, 8], 392),
    "ds_gcn_h8_c12_l4_k6": ("GCNDeepSigns", 8, 12, 4, 6, [7, 10, 5, 8, 11], 103),
    "ds_tf_h16_l2_k3": ("TransformerDeepSigns", 16, 4, 2, 3, [5, 1, 12, 7, 9, 6], 94),
    "ds_tf_h15_l3_k4": ("TransformerDeepSigns", 15, 4, 3, 4, [6, 4, 11, 1, 9, 8], 125),
    "ds_tf_h24_l4_k6": ("TransformerDeepSigns", 24, 4, 4, 6, [7, 10, 1, 8, 13], 96),
}


def _import(name):
    """One reference module of the DGL tree, with the two stand-in directories ahead of everything."""
    for m in list(sys.modules):
        if m.split(".")[0] in ("layers", "nets", "dgl", "_ref_shim_dgl"):
            del sys.modules[m]
    sys.path[:0] = [SHIM_DEEPSIGNS, SHIM, os.path.join(REF, "GraphPrediction")]
    try:
        return importlib.import_module(name)
    finally:
        del sys.path[:3]


def case(name, cls, hidden, out, layers, k, sizes, seed):
    mod = _import("layers.deepsigns")
    import dgl  # the stand-in
    torch.manual_seed(seed)
    net = getattr(mod, cls)(1, hidden, out, layers, k, use_bn=True, dropout=0.0, activation="relu")
    randomise(net, seed + 1)
    with torch.no_grad():                    # (GraphConv's bias starts at zero: make it count)
        for n, p in net.named_parameters():
            if n.startswith("enc.layers.") and n.endswith(".bias") and p.dim() == 1 and float(p.abs().max()) == 0.0:
                p.copy_(0.1 * torch.randn(p.shape, generator=torch.Generator().manual_seed(seed + 5)))
        if cls == "TransformerDeepSigns":
            net.embed.weight.mul_(EMBED_SCALE)
    sd0 = {k_: v.detach().clone() for k_, v in net.state_dict().items()}
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    pe = synth.dgl_pos_enc(data, k)
    g = dgl.Graph(data.edge_index[0], data.edge_index[1], torch.tensor(data.sizes))
    x = pe.unsqueeze(-1)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 3))
    arrays = {**sd_arrays(net), **data_arrays(data), "in/pos_enc": pe.numpy(), "in/cotangent": cot.numpy(),
              "meta/params": np.array([hidden, out, layers, k], dtype=np.int64), "meta/cls": np.array(cls)}
    net.eval()
    with torch.no_grad():
        arrays["out/eval/y"] = net(g, x.clone()).numpy()
    net.train()
    with torch.no_grad():
        arrays["out/train/y"] = net(g, x.clone()).numpy()
    for k_, v in net.state_dict().items():
        if k_.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked"):
            arrays["out/train/buffers/" + k_] = v.detach().clone().numpy()
    net.load_state_dict(sd0)
    net.train()
    net.zero_grad()
    (net(g, x.clone()) * cot).sum().backward()
    for k_, p in net.named_parameters():
        arrays["out/grad/" + k_] = p.grad.detach().clone().numpy()
    save(name, **arrays)


def main():
    for name, args in CASES.items():
        case(name, *args)


if __name__ == "__main__":
    main()
