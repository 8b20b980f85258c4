"""Regenerates tests/golden/baseline_*.npz: the rows SignNet is compared against in the DGL tree (GraphPrediction/configs: *_NoPE.json,
*_LapPE.json, GatedGCN_ZINC_LapPE_abs.json / _can.json) run through the ORIGINAL code — the reference's five base nets and the
reference's own handle_lap (train/train_ZINC_graph_regression.py:13-51) — on CPU, with the graph ops supplied by tests/golden/ref_shim/.
Arrays only; the helpers are make_golden.py's.

    python tests/golden/make_baseline_pe.py        # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

  baseline_handle_lap_k8                       handle_lap's network-free branches on one batch of real eigenvectors
  baseline_<net>_nope (five nets)              the sibling dgl_* fixture's scaled-down net at pe_init 'no_pe'
  baseline_gatedgcn_{sign_flip,abs_val,canonical}   GatedGCN at pe_init 'lap_pe' behind handle_lap
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _fresh_import, data_arrays, randomise, save, sd_arrays, synth  # noqa: E402

FLIP_SEED = 1234          # torch.manual_seed before the reference's sign_flip draw


def _dgl():
    import dgl  # the shim
    if not hasattr(dgl, "broadcast_nodes"):
        # dgl.broadcast_nodes by its published meaning: graph g's row for every node of graph g
        dgl.broadcast_nodes = lambda g, x: x.repeat_interleave(g.batch_num_nodes(), 0)
    return dgl


def _handle_lap():
    mods = _fresh_import("GraphPrediction", ["train.train_ZINC_graph_regression"])
    _dgl()
    return mods[0].handle_lap


def _graph(data):
    return _dgl().Graph(data.edge_index[0], data.edge_index[1], torch.tensor(data.sizes))


def canonical_margin(pe, sizes):
    """float64 [B, K]: |s_pos - s_neg| / max(s_pos, s_neg) where the sums decide (n_pos >= n_neg, a non-zero sum); +inf where the
    counts already decide or the column is all zero."""
    out = np.full((len(sizes), pe.shape[1]), np.inf)
    p = pe.double().numpy()
    r = 0
    for b, n in enumerate(sizes):
        blk = p[r:r + n]
        r += n
        n_pos, n_neg = (blk >= 0).sum(0), (blk < 0).sum(0)
        s_pos, s_neg = np.where(blk >= 0, blk, 0).sum(0), np.abs(np.where(blk < 0, blk, 0)).sum(0)
        big = np.maximum(s_pos, s_neg)
        m = (n_pos >= n_neg) & (big > 0)
        out[b, m] = np.abs(s_pos - s_neg)[m] / big[m]
    return out


def _lap(handle_lap, method, pe, g):
    """pe through the reference's handle_lap (sign_flip: under FLIP_SEED) -> (p, the uniforms it drew or None)."""
    u = None
    if method == "sign_flip":
        torch.manual_seed(FLIP_SEED)
        u = torch.rand(pe.size(1))
        torch.manual_seed(FLIP_SEED)
    p = handle_lap(types.SimpleNamespace(lap_method=method), pe.clone(), g, "cpu")
    return p, u


def handle_lap_case(name, k, sizes, seed):
    handle_lap = _handle_lap()
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    pe = synth.dgl_pos_enc(data, k)
    arrays = {"in/pos_enc": pe.numpy(), "in/sizes": np.array(sizes, dtype=np.int64), "meta/flip_seed": np.array(FLIP_SEED),
              "meta/margin": canonical_margin(pe, sizes)}
    for method in ("abs_val", "canonical", "none", "sign_flip"):
        p, u = _lap(handle_lap, method, pe, _graph(data))
        arrays[f"out/{method}"] = p.numpy()
        if u is not None:
            arrays["in/u"] = u.numpy()
    save(name, **arrays)


COMMON = dict(num_atom_type=28, num_bond_type=4, in_feat_dropout=0.0, dropout=0.0, batch_norm=True, residual=True, edge_feat=True,
              device="cpu", lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4, sign_inv_net="none")
# (module, class, the sibling dgl_* fixture's scaled-down parameters, sizes, seed, snorm)
NETS = {
    "gin": ("gin_net", "GINNet", dict(hidden_dim=24, out_dim=24, L=3, pos_enc_dim=6, readout="mean"), [5, 9, 12, 7, 3], 33, False),
    "gatedgcn": ("gatedgcn_net", "GatedGCNNet", dict(hidden_dim=28, out_dim=28, L=2, pos_enc_dim=8, readout="mean"), [6, 4, 11, 2], 35,
                 False),
    "pna": ("pna_net", "PNANet",
            dict(hidden_dim=20, out_dim=20, L=3, pos_enc_dim=6, readout="sum", graph_norm=True, aggregators="mean max min std",
                 scalers="identity amplification attenuation", towers=5, divide_input_first=True, divide_input_last=True, edge_dim=8,
                 pretrans_layers=1, posttrans_layers=1, gru=False, lambda_loss=1000), [5, 9, 12, 7, 3], 36, True),
    "transformer": ("transformer_net", "TransformerNet",
                    dict(hidden_dim=32, out_dim=32, L=2, pos_enc_dim=8, n_heads=8, full_graph=False, readout="sum", layer_norm=True),
                    [6, 4, 11, 2], 38, False),
    "gat": ("gat_net", "GATNet", dict(hidden_dim=12, out_dim=12, L=3, pos_enc_dim=6, n_heads=4, readout="mean"), [5, 9, 12, 7, 3], 39,
            False),
}
AVG_D = (2.2, 0.6, 1.1)       # lin, exp, log (main_ZINC_graph_regression.py:400-405)


def _build(net_name, **over):
    module, cls, params, sizes, seed, snorm = NETS[net_name]
    mods = _fresh_import("GraphPrediction", ["nets.ZINC_graph_regression." + module])
    p = dict(COMMON, **params)
    p.update(over)
    if net_name == "pna":
        p["avg_d"] = dict(lin=torch.tensor(AVG_D[0]), exp=torch.tensor(AVG_D[1]), log=torch.tensor(AVG_D[2]))
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(mods[0], cls)(p)
    randomise(net, seed + 1)
    if net_name == "gat":
        with torch.no_grad():
            for n_, p_ in net.named_parameters():
                if n_.startswith("layers.") and n_.endswith(".bias") and n_.count(".") == 2:       # GATConv.bias (zero-initialised)
                    p_.copy_(0.1 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(seed + 2)))
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    sn = torch.cat([torch.full((n, 1), 1.0 / n) for n in data.sizes]).sqrt() if snorm else None         # data/molecules.py:307-308
    meta = {"meta/hidden_L_k": np.array([p["hidden_dim"], p["L"], p["pos_enc_dim"]], dtype=np.int64)}
    for key in ("n_heads", "towers", "edge_dim"):
        if key in p:
            meta["meta/" + key] = np.array(p[key], dtype=np.int64)
    if net_name == "pna":
        meta["meta/avg_d"] = np.array(AVG_D, dtype=np.float64)
    return net, data, sn, meta


def _run(name, net, data, sn, p, arrays, h_last):
    for mode in ("eval", "train"):
        net.train(mode == "train")
        g = _graph(data)
        with torch.no_grad():
            y, _ = net(g, data.x.squeeze(-1), None if p is None else p.clone(), data.edge_attr, sn)
        arrays[f"out/{mode}/y"] = y.numpy()
        if h_last:
            arrays[f"out/{mode}/h_last"] = g.ndata["h"].numpy()
    save(name, **arrays)


def nope_case(net_name):
    net, data, sn, meta = _build(net_name, pe_init="no_pe", lap_method="none", pe_aggregate="none")
    arrays = {**sd_arrays(net), **data_arrays(data), **meta}
    if sn is not None:
        arrays["in/snorm_n"] = sn.numpy()
    _run(f"baseline_{net_name}_nope", net, data, sn, None, arrays, h_last=net_name != "gin")


def lappe_case(method):
    handle_lap = _handle_lap()
    net, data, sn, meta = _build("gatedgcn", pe_init="lap_pe", lap_method=method, pe_aggregate="add")
    k = int(meta["meta/hidden_L_k"][2])
    pe = synth.dgl_pos_enc(data, k)
    p, u = _lap(handle_lap, method, pe, _graph(data))
    arrays = {**sd_arrays(net), **data_arrays(data), **meta, "in/pos_enc": pe.numpy(), "out/p": p.numpy(),
              "meta/flip_seed": np.array(FLIP_SEED)}
    if u is not None:
        arrays["in/u"] = u.numpy()
    if method == "canonical":
        arrays["meta/margin"] = canonical_margin(pe, data.sizes)
    _run(f"baseline_gatedgcn_{method}", net, data, sn, p, arrays, h_last=True)


def main():
    handle_lap_case("baseline_handle_lap_k8", 8, [3, 5, 9, 12, 17, 20], 11)
    for net_name in NETS:
        nope_case(net_name)
    for method in ("sign_flip", "abs_val", "canonical"):
        lappe_case(method)


if __name__ == "__main__":
    main()
