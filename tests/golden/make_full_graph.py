"""Regenerates tests/golden/fullgraph_*.npz: the reference's own TransformerNet with net_params['full_graph'] = True
(GraphPrediction/nets/ZINC_graph_regression/transformer_net.py + layers/transformer.py:118-228) on CPU, with the graph ops supplied by
tests/golden/ref_shim/.  Arrays only; the helpers are make_golden.py's.

    python tests/golden/make_full_graph.py        # needs the reference tree where make_golden.py looks for it (not needed to run the tests)

The complete graph of every molecule is built as data/molecules.py:211-235 builds it — networkx.complete_graph(n) turned into a
directed edge list, the bonds' classes and real = 1 copied onto their pairs, class 0 / real = 0 everywhere else.  `gamma` is set
explicitly after `randomise`.  Every case is run twice from the same state: in float32 and on a float64 copy of the net.

  in/full_src, in/full_dst, in/real, in/e_full     the full edge list (batch node ids), the flags and the per-pair classes
  in/target                                         the L1 targets
  out/eval/{y,h_last}[64]                           eval forward
  out/train/y[64], out/train/bn[64]/<buffer>        train-mode forward, the BatchNorm buffers after it
  out/train/grad[64]/<parameter>                    gradient of loss(y, target) (the net's own L1 `loss`) w.r.t. every parameter
"""
from __future__ import annotations

import contextlib
import copy
import io
import os
import sys

import networkx as nx
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import _fresh_import, data_arrays, randomise, save, sd_arrays, synth  # noqa: E402

COMMON = dict(num_atom_type=28, num_bond_type=4, in_feat_dropout=0.0, dropout=0.0, batch_norm=True, residual=True, edge_feat=True,
              device="cpu", lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4, layer_norm=True, full_graph=True)

CASES = {
    "fullgraph_tf_h32_l2_k8_add": dict(
        params=dict(hidden_dim=32, out_dim=32, L=2, pos_enc_dim=8, n_heads=8, readout="sum", pe_init="lap_pe", lap_method="none",
                    pe_aggregate="add", sign_inv_net="none"),
        sizes=[6, 4, 11, 2], seed=38, gamma=[0.1, 0.6]),
    "fullgraph_tf_h24_l3_nope_mean": dict(
        params=dict(hidden_dim=24, out_dim=24, L=3, pos_enc_dim=6, n_heads=3, readout="mean", pe_init="no_pe", lap_method="none",
                    pe_aggregate="none", sign_inv_net="none"),
        sizes=[1, 5, 9, 12, 3], seed=41, gamma=[0.35, -0.3, 1.7]),
    "fullgraph_tf_h16_l2_signinv_concat": dict(
        params=dict(hidden_dim=16, out_dim=16, L=2, pos_enc_dim=4, n_heads=4, readout="sum", pe_init="lap_pe", lap_method="sign_inv",
                    pe_aggregate="concat", sign_inv_net="gin", sign_inv_layers=3, sign_inv_activation="relu", phi_out_dim=4),
        sizes=[6, 4, 10, 2, 7], seed=43, gamma=[0.25, 0.8]),
}


def full_edges(data):
    """data/molecules.py:211-235 per graph, concatenated with batch node ids: (src, dst, real, e) int64."""
    ei = data.edge_index
    cls = {(int(a), int(b)): int(c) for a, b, c in zip(ei[0], ei[1], data.edge_attr.reshape(-1))}
    src, dst, real, feat = [], [], [], []
    off = 0
    for n in data.sizes:
        for u, v in nx.complete_graph(n).to_directed().edges():
            key = (off + u, off + v)
            src.append(key[0])
            dst.append(key[1])
            real.append(int(key in cls))
            feat.append(cls.get(key, 0))
        off += n
    t = lambda a: torch.tensor(a, dtype=torch.int64)
    return t(src), t(dst), t(real), t(feat)


def _dgl():
    import dgl  # the shim
    if not hasattr(dgl, "broadcast_nodes"):
        dgl.broadcast_nodes = lambda g, x: x.repeat_interleave(g.batch_num_nodes(), 0)
    return dgl


def case(name, params, sizes, seed, gamma):
    mods = _fresh_import("GraphPrediction", ["nets.ZINC_graph_regression.transformer_net"])
    dgl = _dgl()
    p = dict(COMMON, **params)
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        net = mods[0].TransformerNet(p)
    randomise(net, seed + 1)
    with torch.no_grad():
        for layer, v in zip(net.layers, gamma):
            layer.gamma.fill_(v)
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    src, dst, real, e_full = full_edges(data)
    k = p["pos_enc_dim"]
    lap = p["pe_init"] == "lap_pe"
    pe = synth.dgl_pos_enc(data, k) if lap else None
    target = torch.randn(len(sizes), 1, generator=torch.Generator().manual_seed(seed + 7))
    arrays = {**sd_arrays(net), **data_arrays(data), "in/full_src": src.numpy(), "in/full_dst": dst.numpy(), "in/real": real.numpy(),
              "in/e_full": e_full.numpy(), "in/target": target.numpy(),
              "meta/params": np.array([p["hidden_dim"], p["L"], k, p["n_heads"]], dtype=np.int64),
              "meta/gamma": np.array(gamma, dtype=np.float64), "meta/pe_init": np.array(p["pe_init"]),
              "meta/lap_method": np.array(p["lap_method"]), "meta/pe_aggregate": np.array(p["pe_aggregate"]),
              "meta/readout": np.array(p["readout"])}
    if lap:
        arrays["in/pos_enc"] = pe.numpy()
    net64 = copy.deepcopy(net).double()

    def graph():
        g = dgl.Graph(src, dst, torch.tensor(data.sizes))
        g.edata["real"] = real
        return g

    def pos(m, g, dtype):
        if not lap:
            return None
        x = pe.to(dtype)
        return m.sign_inv_net(g, x.unsqueeze(-1).clone()).squeeze(-1) if p["lap_method"] == "sign_inv" else x.clone()

    for m, dtype, tag in ((net, torch.float32, ""), (net64, torch.float64, "64")):
        m.eval()
        g = graph()
        with torch.no_grad():
            y, _ = m(g, data.x.squeeze(-1), pos(m, g, dtype), e_full, None)
        arrays[f"out/eval/y{tag}"] = y.numpy()
        arrays[f"out/eval/h_last{tag}"] = g.ndata["h"].numpy()
        m.train()
        g = graph()
        y, _ = m(g, data.x.squeeze(-1), pos(m, g, dtype), e_full, None)
        m.loss(y, target.to(dtype)).backward()
        arrays[f"out/train/y{tag}"] = y.detach().numpy()
        for key, buf in m.named_buffers():
            arrays[f"out/train/bn{tag}/{key}"] = buf.detach().numpy()
        for key, q in m.named_parameters():
            if q.grad is not None:
                arrays[f"out/train/grad{tag}/{key}"] = q.grad.detach().numpy()
    save(name, **arrays)
    a = arrays
    rel = lambda x, y: float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
    worst = max((rel(a[k_], a["out/train/grad64/" + k_[len("out/train/grad/"):]]), k_) for k_ in a if k_.startswith("out/train/grad/"))
    print(f"   fp32 vs float64: eval y {rel(a['out/eval/y'], a['out/eval/y64']):.1e}, train y {rel(a['out/train/y'], a['out/train/y64']):.1e}, "
          f"worst gradient {worst[0]:.1e} ({worst[1][len('out/train/grad/'):]}); edges {len(src)}, real {int(real.sum())}")
    for li in range(p["L"]):
        print(f"   layers.{li}.gamma grad {a[f'out/train/grad64/layers.{li}.gamma']}")


def main():
    for name, c in CASES.items():
        case(name, **c)


if __name__ == "__main__":
    main()
