"""Regenerates tests/golden/readout_max_*.npz: the reference's five base nets of the DGL tree with net_params['readout'] = 'max'
(GraphPrediction/nets/ZINC_graph_regression/*_net.py: `hg = dgl.max_nodes(g, 'h')`) on CPU, with the graph ops supplied by
tests/golden/ref_shim/.  Arrays only; the helpers are make_golden.py's, the nets' scaled-down sizes make_baseline_pe.py's.

    python tests/golden/make_readout_max.py        # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

  readout_max_{gin,gatedgcn,pna,transformer,gat}   the sibling baseline_<net>_nope fixture's net at readout 'max'
  readout_max_gatedgcn_signinv                     GatedGCN at pe_init 'lap_pe' behind its own sign_inv_net (gin)
  readout_max_transformer_full                     TransformerNet with full_graph True (the complete graph of make_full_graph.py)

Every case is run twice from the same state, in float32 and on a float64 copy of the net:

  in/target                                         the L1 targets
  out/eval/{y,h_last,hg}[64]                        eval forward: scores, final node features, the pooled rows MLPReadout receives
  out/train/{y,h_last,hg}[64], out/train/bn[64]/*   train-mode forward, the BatchNorm buffers after it
  out/train/grad[64]/<parameter>                    gradient of the net's own L1 `loss` w.r.t. every parameter
  meta/gap_eval, meta/gap_train  [B, out_dim]       top-1 minus top-2 of the float32 final node features per (graph, channel), relative to
                                                    the channel's largest magnitude over the batch (+inf for a one-node graph)

The shim's max_nodes is scatter_reduce('amax'), whose backward splits the gradient evenly among tied rows; DGL's segment reduce — and
sn_segment_max_bwd_f32 — hand it to one row.  The two agree where no two rows tie, so a fixture whose smallest gap is below MIN_GAP is
REFUSED: below it a float32 rounding could move the gradient to another node (MIN_GAP is 100 x the 1e-5 forward tolerance).  The float64
copy must pick the same rows.
"""
from __future__ import annotations

import copy
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import data_arrays, save, sd_arrays, synth  # noqa: E402
import make_baseline_pe as BP  # noqa: E402
import make_full_graph as FG  # noqa: E402

MIN_GAP = 1e-3

# name -> (net of make_baseline_pe.NETS, parameter overrides, seed or None for the sibling's).  The seeds are the first of the sibling's,
# 101, 102, ... for which the reference alone clears MIN_GAP in eval and in train mode.  A net without positional encoding gives
# 1-WL-equivalent nodes of a graph IDENTICAL features — an exact tie of the maximum — so PNA and GAT, whose NoPE runs never cleared the rule, are
# run at pe_init 'lap_pe' with lap_method 'none' (the raw eigenvectors break the symmetry).  GAT ends in ReLU and a mean over its heads: a
# channel that is 0 at every node of a graph is an exact tie too, and few draws have none (937 is the first of 300, 301, ...).
CASES = {
    "readout_max_gin": ("gin", dict(pe_init="no_pe", lap_method="none", pe_aggregate="none"), 117),
    "readout_max_gatedgcn": ("gatedgcn", dict(pe_init="no_pe", lap_method="none", pe_aggregate="none"), 106),
    "readout_max_pna": ("pna", dict(pe_init="lap_pe", lap_method="none", pe_aggregate="add"), 101),
    "readout_max_transformer": ("transformer", dict(pe_init="no_pe", lap_method="none", pe_aggregate="none"), 101),
    "readout_max_gat": ("gat", dict(pe_init="lap_pe", lap_method="none", pe_aggregate="add"), 937),
    "readout_max_gatedgcn_signinv": ("gatedgcn", dict(pe_init="lap_pe", lap_method="sign_inv", pe_aggregate="add", sign_inv_net="gin",
                                                      sign_inv_layers=3, sign_inv_activation="relu", phi_out_dim=4), 103),
    "readout_max_transformer_full": ("transformer", dict(pe_init="no_pe", lap_method="none", pe_aggregate="none", full_graph=True,
                                                         hidden_dim=24, out_dim=24, n_heads=3, L=2), None),
}
FULL_GAMMA = [0.35, 0.8]


def gaps(h, sizes):
    """[B, C] float64: (top-1 - top-2) / max|channel| of the rows of every graph; +inf for a one-node graph."""
    h = h.double()
    scale = h.abs().amax(0).clamp_min(1e-300)
    out, r = [], 0
    for n in sizes:
        blk = h[r:r + n]
        r += n
        if n < 2:
            out.append(torch.full((h.shape[1],), float("inf"), dtype=torch.float64))
        else:
            top = blk.topk(2, dim=0).values
            out.append((top[0] - top[1]) / scale)
    return torch.stack(out)


def _argmax_rows(h, sizes):
    out, r = [], 0
    for n in sizes:
        out.append(h[r:r + n].argmax(0) + r)
        r += n
    return torch.stack(out)


def case(name, net_name, over, seed):
    params = dict(over, readout="max")
    if seed is not None:
        BP.NETS[net_name] = BP.NETS[net_name][:4] + (seed,) + BP.NETS[net_name][5:]
    net, data, sn, meta = BP._build(net_name, **params)
    sizes, seed = data.sizes, BP.NETS[net_name][4]
    full = bool(params.get("full_graph"))
    lap = params["pe_init"] == "lap_pe"
    dgl = BP._dgl()
    if full:
        with torch.no_grad():
            for layer, v in zip(net.layers, FULL_GAMMA):
                layer.gamma.fill_(v)
        src, dst, real, e_full = FG.full_edges(data)
    pe = synth.dgl_pos_enc(data, int(meta["meta/hidden_L_k"][2])) if lap else None
    target = torch.randn(len(sizes), 1, generator=torch.Generator().manual_seed(seed + 7))
    cfg = dict(BP.COMMON)
    cfg.update(BP.NETS[net_name][2])
    cfg.update(params)
    if net_name == "pna":
        cfg["avg_d"] = dict(lin=BP.AVG_D[0], exp=BP.AVG_D[1], log=BP.AVG_D[2])
    arrays = {**sd_arrays(net), **data_arrays(data), **meta, "in/target": target.numpy(), "meta/net": np.array(net_name),
              "meta/net_params": np.array(json.dumps(cfg, sort_keys=True))}
    if sn is not None:
        arrays["in/snorm_n"] = sn.numpy()
    if lap:
        arrays["in/pos_enc"] = pe.numpy()
    if full:
        arrays.update({"in/full_src": src.numpy(), "in/full_dst": dst.numpy(), "in/real": real.numpy(), "in/e_full": e_full.numpy(),
                       "meta/gamma": np.array(FULL_GAMMA, dtype=np.float64)})

    def graph():
        if not full:
            return BP._graph(data)
        g = dgl.Graph(src, dst, torch.tensor(sizes))
        g.edata["real"] = real
        return g

    def forward(m, dtype, store):
        g = graph()
        p = None
        if lap:             # handle_lap (train_ZINC_graph_regression.py:13-51): 'sign_inv' through the net's own encoder, 'none' unchanged
            p = pe.to(dtype).clone()
            if params["lap_method"] == "sign_inv":
                p = m.sign_inv_net(g, p.unsqueeze(-1)).squeeze(-1)
        hook = m.MLP_layer.register_forward_pre_hook(lambda mod, args: store.__setitem__("hg", args[0].detach().clone()))
        y, _ = m(g, data.x.squeeze(-1), p, e_full if full else data.edge_attr, None if sn is None else sn.to(dtype))
        hook.remove()
        store["h_last"] = g.ndata["h"].detach().clone()
        return y

    for m, dtype, tag in ((net, torch.float32, ""), (copy.deepcopy(net).double(), torch.float64, "64")):
        for mode in ("eval", "train"):
            m.train(mode == "train")
            st = {}
            if mode == "eval":
                with torch.no_grad():
                    y = forward(m, dtype, st)
            else:
                y = forward(m, dtype, st)
                m.loss(y, target.to(dtype)).backward()
                for key, buf in m.named_buffers():
                    arrays[f"out/train/bn{tag}/{key}"] = buf.detach().numpy()
                for key, q in m.named_parameters():
                    if q.grad is not None:
                        arrays[f"out/train/grad{tag}/{key}"] = q.grad.detach().numpy()
            arrays[f"out/{mode}/y{tag}"] = y.detach().numpy()
            arrays[f"out/{mode}/h_last{tag}"] = st["h_last"].numpy()
            arrays[f"out/{mode}/hg{tag}"] = st["hg"].numpy()
    worst = {}
    for mode in ("eval", "train"):
        h32, h64 = torch.from_numpy(arrays[f"out/{mode}/h_last"]), torch.from_numpy(arrays[f"out/{mode}/h_last64"])
        gap = gaps(h32, sizes)
        arrays[f"meta/gap_{mode}"] = gap.numpy()
        worst[mode] = float(gap.min())
        if worst[mode] < MIN_GAP:
            raise SystemExit(f"{name}: smallest {mode} gap {worst[mode]:.2e} < {MIN_GAP:g}: not written — choose another seed")
        if not torch.equal(_argmax_rows(h32, sizes), _argmax_rows(h64, sizes)):
            raise SystemExit(f"{name}: float32 and float64 pick different rows in {mode} mode: not written — choose another seed")
    save(name, **arrays)
    a = arrays
    rel = lambda x, y: float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
    wg = max((rel(a[k_], a["out/train/grad64/" + k_[len("out/train/grad/"):]]), k_) for k_ in a if k_.startswith("out/train/grad/"))
    print(f"   smallest gap: eval {worst['eval']:.2e}, train {worst['train']:.2e}; fp32 vs float64: eval y {rel(a['out/eval/y'], a['out/eval/y64']):.1e}, "
          f"train y {rel(a['out/train/y'], a['out/train/y64']):.1e}, worst gradient {wg[0]:.1e} ({wg[1][len('out/train/grad/'):]})")


def main():
    only = sys.argv[1:]
    for name, (net_name, over, seed) in CASES.items():
        if not only or name in only:
            sibling = BP.NETS[net_name]
            case(name, net_name, over, seed)
            BP.NETS[net_name] = sibling


if __name__ == "__main__":
    main()
