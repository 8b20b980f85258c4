"""CPU: the baseline PE rows of the DGL tree (NoPE, sign-flip, abs and canonical LapPE) — constructors, state_dict keys against the
reference's fixtures (tests/golden/baseline_*.npz, made by tests/golden/make_baseline_pe.py), handle_lap's refusal, the step classes'
refusals, the entry point sn_lap_pe_transform_f32 (declared, bound, argument checks on the host), and the margin condition of the
canonical fixture.  No GPU needed."""
import os
import re
import types

import numpy as np
import pytest
import torch

import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the sibling dgl_* fixture's scaled-down parameters of each net (make_baseline_pe.NETS), as the constructors take them
_COMMON = dict(num_atom_type=28, num_bond_type=4, in_feat_dropout=0.0, dropout=0.0, batch_norm=True, residual=True, edge_feat=True,
               lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4)
_CLS = {"gin": "GINNet", "gatedgcn": "GatedGCNNet", "pna": "PNANet", "transformer": "TransformerNet", "gat": "GATNet"}
_READOUT = {"gin": "mean", "gatedgcn": "mean", "pna": "sum", "transformer": "sum", "gat": "mean"}
NET_FIXTURES = [("gin", "nope"), ("gatedgcn", "nope"), ("gat", "nope"), ("pna", "nope"), ("transformer", "nope"),
                ("gatedgcn", "sign_flip"), ("gatedgcn", "abs_val"), ("gatedgcn", "canonical")]


def fixture_net(net, row, device="cpu"):
    """(fixture, the HIP net built with the fixture's parameters) — shared with tests/test_lap_baselines_gpu.py."""
    from signnet_basisnet_amd import dgl_nets
    fx = G.load(f"baseline_{net}_{row}")
    hidden, L, k = (int(v) for v in fx.meta["hidden_L_k"])
    p = dict(_COMMON, hidden_dim=hidden, out_dim=hidden, L=L, pos_enc_dim=k, readout=_READOUT[net], device=device)
    if row == "nope":
        p.update(pe_init="no_pe", lap_method="none", pe_aggregate="none")
    else:
        p.update(pe_init="lap_pe", lap_method=row, pe_aggregate="add")
    if net in ("gat", "transformer"):
        p["n_heads"] = int(fx.meta["n_heads"])
    if net == "transformer":
        p.update(full_graph=False, layer_norm=True)
    if net == "pna":
        a = fx.meta["avg_d"]
        p.update(graph_norm=True, aggregators="mean max min std", scalers="identity amplification attenuation",
                 towers=int(fx.meta["towers"]), divide_input_first=True, divide_input_last=True, edge_dim=int(fx.meta["edge_dim"]),
                 pretrans_layers=1, posttrans_layers=1, gru=False, avg_d=dict(lin=float(a[0]), exp=float(a[1]), log=float(a[2])))
    return fx, getattr(dgl_nets, _CLS[net])(p)


@pytest.mark.parametrize("net,row", NET_FIXTURES)
def test_state_dict_keys_equal_the_reference_nets(net, row):
    fx, m = fixture_net(net, row)
    assert [str(k) for k in fx.meta["sd_keys"]] == list(m.state_dict().keys())          # the reference's keys, in its order
    assert sorted(fx.sd) == sorted(m.state_dict())                                        # (every tensor is stored)
    m.load_state_dict(fx.sd, strict=True)
    assert hasattr(m, "embedding_p") == (row != "nope") and not hasattr(m, "pe_proj") and getattr(m, "sign_inv_net", None) is None


# net_params of the twelve shipped baseline configs (GraphPrediction/configs/*/*_ZINC_NoPE.json, *_ZINC_LapPE.json,
# GatedGCN_ZINC_LapPE_abs.json, GatedGCN_ZINC_LapPE_can.json), written out as plain values
_PNA = dict(graph_norm=True, aggregators="mean max min std", scalers="identity amplification attenuation", towers=5,
            divide_input_first=True, divide_input_last=True, edge_dim=40, pretrans_layers=1, posttrans_layers=1, gru=False,
            lambda_loss=1000, avg_d=dict(lin=2.2, exp=0.6, log=1.1))
_GAT = dict(n_heads=4, sign_inv_net="none", sign_inv_layers=0)
_TF = dict(n_heads=8, full_graph=False, layer_norm=True)
_NOPE = dict(pe_init="no_pe", lap_method="none", pe_aggregate="none")
SHIPPED_BASELINES = {
    "GIN_ZINC_NoPE": ("GINNet", dict(hidden_dim=122, out_dim=122, L=16, readout="mean", pos_enc_dim=8, **_NOPE)),
    "GIN_ZINC_LapPE": ("GINNet", dict(hidden_dim=122, out_dim=122, L=16, readout="mean", pos_enc_dim=8, pe_init="lap_pe",
                                      lap_method="sign_flip", pe_aggregate="add")),
    "GatedGCN_ZINC_NoPE": ("GatedGCNNet", dict(hidden_dim=77, out_dim=77, L=16, readout="mean", pos_enc_dim=8, **_NOPE)),
    "GatedGCN_ZINC_LapPE": ("GatedGCNNet", dict(hidden_dim=77, out_dim=77, L=16, readout="mean", pos_enc_dim=8, pe_init="lap_pe",
                                                lap_method="sign_flip", pe_aggregate="add")),
    "GatedGCN_ZINC_LapPE_abs": ("GatedGCNNet", dict(hidden_dim=77, out_dim=77, L=16, readout="mean", pos_enc_dim=8, pe_init="lap_pe",
                                                    lap_method="abs_val", pe_aggregate="add")),
    "GatedGCN_ZINC_LapPE_can": ("GatedGCNNet", dict(hidden_dim=77, out_dim=77, L=16, readout="mean", pos_enc_dim=8, pe_init="lap_pe",
                                                    lap_method="canonical", pe_aggregate="add")),
    "GAT_ZINC_NoPE": ("GATNet", dict(hidden_dim=65, out_dim=65, L=8, readout="mean", pos_enc_dim=8, pe_init="no_pe",
                                     lap_method="sign_flip", pe_aggregate="none", **_GAT)),
    "GAT_ZINC_LapPE": ("GATNet", dict(hidden_dim=65, out_dim=65, L=8, readout="mean", pos_enc_dim=8, pe_init="lap_pe",
                                      lap_method="sign_flip", pe_aggregate="concat", **_GAT)),
    "PNA_ZINC_NoPE": ("PNANet", dict(hidden_dim=80, out_dim=80, L=16, readout="sum", pos_enc_dim=16, **_NOPE, **_PNA)),
    "PNA_ZINC_LapPE": ("PNANet", dict(hidden_dim=80, out_dim=80, L=16, readout="sum", pos_enc_dim=8, pe_init="lap_pe",
                                      lap_method="sign_flip", pe_aggregate="add", **_PNA)),
    "Transformer_ZINC_NoPE": ("TransformerNet", dict(hidden_dim=80, out_dim=80, L=8, readout="mean", pos_enc_dim=16, **_NOPE, **_TF)),
    "Transformer_ZINC_LapPE": ("TransformerNet", dict(hidden_dim=80, out_dim=80, L=8, readout="mean", pos_enc_dim=16, pe_init="lap_pe",
                                                      lap_method="sign_flip", pe_aggregate="concat", **_TF)),
}


@pytest.mark.parametrize("name", list(SHIPPED_BASELINES))
def test_constructors_accept_the_shipped_baseline_configs(name):
    from signnet_basisnet_amd import dgl_configs, dgl_nets
    cls, over = SHIPPED_BASELINES[name]
    p = dict(_COMMON, device="cpu")
    p.update(over)
    net = getattr(dgl_nets, cls)(p)
    lap = p["pe_init"] == "lap_pe"
    assert hasattr(net, "embedding_p") == lap                                   # (built for 'rand_walk' / 'lap_pe' only)
    assert hasattr(net, "pe_proj") == (p["pe_aggregate"] == "concat" and cls != "GATNet")      # gat_net.py never builds one
    assert getattr(net, "sign_inv_net", None) is None
    # dgl_configs.BASELINES holds the same twelve rows
    twin = {k: v for k, v in dgl_configs.BASELINES.items() if v["cls"] == cls and all(v.get(f) == over[f] for f in over)}
    assert len(twin) == 1, (name, list(twin))


@pytest.mark.parametrize("cls", ["GINNet", "GatedGCNNet", "GATNet", "PNANet", "TransformerNet"])
def test_constructors_still_refuse_what_is_not_built(cls):
    from signnet_basisnet_amd import dgl_nets
    name = next(n for n, (c, _) in SHIPPED_BASELINES.items() if c == cls and n.endswith("NoPE"))
    base = dict(_COMMON, device="cpu")
    base.update(SHIPPED_BASELINES[name][1], hidden_dim=32, out_dim=32)           # (a width every net takes)
    if cls == "PNANet":
        base.update(hidden_dim=40, out_dim=40)
    getattr(dgl_nets, cls)(dict(base))
    for bad in (dict(pe_init="rand_walk"), dict(lap_lspe=True), dict(use_lapeig_loss=True), dict(dropout=0.1), dict(in_feat_dropout=0.1),
                dict(readout="max")):
        with pytest.raises(NotImplementedError):
            getattr(dgl_nets, cls)(dict(base, **bad))


def test_handle_lap_raises_the_reference_error_for_an_unknown_method():
    from signnet_basisnet_amd import dgl_nets
    with pytest.raises(ValueError, match="^invalid laplacian method$"):
        dgl_nets.handle_lap(types.SimpleNamespace(lap_method="rand_walk"), torch.zeros(3, 2), None, "cpu")
    p = torch.randn(3, 2)
    assert dgl_nets.handle_lap(types.SimpleNamespace(lap_method="none"), p, None) is p            # raw eigenvectors: its input
    with pytest.raises(RuntimeError, match="GPU only"):                                            # no CPU fallback
        dgl_nets.handle_lap(types.SimpleNamespace(lap_method="abs_val"), p, None)


def _step(net, **kw):
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    return DGLBucketedStep(net, optim.FlatAdam(net.parameters(), lr=1e-3), **kw)


def test_bucketed_step_takes_the_new_nets_and_refuses_inconsistent_ones():
    from signnet_basisnet_amd import dgl_configs, dgl_nets
    for net, row in NET_FIXTURES:
        s = _step(fixture_net(net, row)[1])
        assert s.lap_method == (None if row == "nope" else row) and s.flip_rng == "host"
    assert _step(fixture_net("gatedgcn", "sign_flip")[1], flip_rng="device").flip_rng == "device"
    with pytest.raises(ValueError, match="flip_rng"):
        _step(fixture_net("gatedgcn", "sign_flip")[1], flip_rng="cuda")
    cls, p = dgl_configs.net_params("gatedgcn", "cpu")                       # a sign_inv net ...
    net = getattr(dgl_nets, cls)(p)
    assert _step(net).lap_method == "sign_inv"
    net.lap_method = "canonical"                                             # ... altered after construction: it carries a sign_inv_net
    with pytest.raises(ValueError, match="lap_method|sign_inv_net"):
        _step(net)
    net = fixture_net("gatedgcn", "abs_val")[1]
    net.lap_method = "sign_inv"                                              # and the reverse: no sign_inv_net to run
    with pytest.raises(ValueError, match="lap_method|sign_inv_net"):
        _step(net)
    net.lap_method = "rand_walk"
    with pytest.raises(ValueError, match="lap_method"):
        _step(net)
    # NoPE: p may be None (the pad keeps zero columns); a LapPE net needs it
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    g = Graph(torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.long), torch.tensor([3, 2]))
    s = _step(fixture_net("gatedgcn", "abs_val")[1])
    with pytest.raises(ValueError, match="pos_enc_dim"):
        s.step(g, torch.zeros(5, dtype=torch.long), None, None, None, torch.zeros(2, 1))
    s = _step(fixture_net("gin", "nope")[1])
    assert tuple(s._zero_p(5, torch.device("cpu")).shape) == (5, s.K) and not s._zero_p(5, torch.device("cpu")).any()


def test_transform_entry_point_is_declared_bound_and_validates_on_the_host():
    from signnet_basisnet_amd import build
    build.build()
    from signnet_basisnet_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "signnet_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    assert re.search(r"\bsn_lap_pe_transform_f32\s*\(", hdr)
    assert "sn_lap_pe_transform_f32" in _lib.SIGNATURES and hasattr(L, "sn_lap_pe_transform_f32")
    modes = dict(re.findall(r"#define SN_LAP_(\w+) (\d+)", hdr))
    assert {k.lower(): int(v) for k, v in modes.items()} == ops.LAP_MODES
    assert len(_lib.SIGNATURES["sn_lap_pe_transform_f32"]) == len(re.search(r"sn_lap_pe_transform_f32\s*\((.*?)\)", hdr, re.S).group(1).split(","))
    assert int(re.search(r"#define SN_ABI_VERSION (\d+)", hdr).group(1)) == 3 == L.sn_version()
    f = L.sn_lap_pe_transform_f32
    buf = (torch.zeros(8).data_ptr())                          # (a host address: every call below is refused or returns before a launch)
    assert f(None, 8, None, 8, 0, 8, 3, None, None, 0, None) == 0           # N == 0: SN_OK without a launch
    assert f(None, 8, None, 8, 4, 0, 1, None, None, 0, None) == 0           # K == 0
    for args, word in (((None, 8, None, 8, 4, 8, 0, None, None, 0, None), b"null"),
                       ((buf, 8, buf, 8, 4, 8, 9, None, None, 0, None), b"mode"),
                       ((buf, 8, buf, 8, -1, 8, 0, None, None, 0, None), b"negative"),
                       ((buf, 7, buf, 8, 4, 8, 0, None, None, 0, None), b"stride"),
                       ((buf, 8, buf, 8, 4, 8, 1, None, None, 0, None), b"uniforms"),
                       ((buf, 8, buf, 8, 4, 8, 3, None, None, 2, None), b"graph_ptr")):
        assert f(*args) == -1 and b"sn_lap_pe_transform_f32" in L.sn_last_error() and word in L.sn_last_error(), (args, L.sn_last_error())
    with pytest.raises(ValueError, match="unknown mode"):
        ops.lap_pe_transform(torch.zeros(2, 2), "rand_walk")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.lap_pe_transform(torch.zeros(2, 2), "abs_val")


def test_canonical_fixture_margin_condition():
    """Sums of n <= 20 fp32 terms differ between summation orders by at most about 2 n 2^-24 = 2.4e-6 relative: a (graph, column) pair
    whose margin |s_pos - s_neg| / max(s_pos, s_neg) is at least 1e-4 has one right answer, a pair below it is a rounding coin toss in
    the reference itself and is excluded from the exact comparison (tests/test_lap_baselines_gpu.py).  The condition of that test:
    at most 10 % of the 48 pairs are excluded.  (On this batch: 2 of 48 — margins 8e-8 and 4e-7; the next is 5e-3.)"""
    fx = G.load("baseline_handle_lap_k8")
    m = fx.meta["margin"]
    sizes = [int(s) for s in fx.inp["sizes"]]
    assert m.shape == (6, 8) and m.dtype == np.float64 and sizes == [3, 5, 9, 12, 17, 20] and max(sizes) <= 20
    below = int((m < 1e-4).sum())
    print("margins below 1e-4:", np.sort(m[m < 1e-4]), "next:", np.sort(m[m >= 1e-4])[0])
    assert below <= 0.10 * m.size, (below, m.size)
    # the margin array is what its definition says (float64 restatement on the stored encoding)
    p, r = fx.inp["pos_enc"].double().numpy(), 0
    for b, n in enumerate(sizes):
        blk = p[r:r + n]
        r += n
        n_pos, n_neg = (blk >= 0).sum(0), (blk < 0).sum(0)
        s_pos, s_neg = np.where(blk >= 0, blk, 0).sum(0), np.abs(np.where(blk < 0, blk, 0)).sum(0)
        for c in range(8):
            big = max(s_pos[c], s_neg[c])
            want = abs(s_pos[c] - s_neg[c]) / big if (n_pos[c] >= n_neg[c] and big > 0) else np.inf
            assert m[b, c] == want, (b, c)
    assert np.isinf(m[0, 3:]).all()           # the 3-node graph's zero-padded columns: never excluded, never flipped
