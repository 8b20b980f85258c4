"""CPU: the numpy restatement of the dropout mask contract (tests/dropout_cases.py) is Philox4x32-10, its masks have the properties the
modules rely on, the case table reaches both dispatch paths, and the committed dropout fixtures were drawn by this generator."""
import glob
import os

import numpy as np
import pytest

import dropout_cases as DC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _hex(ws):
    return " ".join(f"{int(w):08x}" for w in ws)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_random123_known_answers(counter, key, want):
    assert _hex(DC.philox4x32_10(counter, key)) == want


def test_threshold_and_scale():
    assert DC.threshold_of(0.5) == 1 << 31
    assert DC.threshold_of(DC.P_TINY) == 0
    assert DC.threshold_of(0.1) == 429496729
    assert DC.scale_of(0.5) == np.float32(2.0) and DC.scale_of(0.9).dtype == np.float32


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate(p):
    n = 1 << 16
    q = 1.0 - DC.threshold_of(p) / 2.0 ** 32
    rate = DC.keep_mask(256, 256, p, DC.SEED, DC.STEP, DC.SITE).mean()
    assert abs(rate - q) <= 5.0 * np.sqrt(q * (1.0 - q) / n), (rate, q)


def test_keep_rate_of_the_recorded_draw():
    assert round(float(DC.keep_mask(64, 64, 0.3, 1234, 0, 7).mean()), 4) == 0.6978


def test_tiny_p_keeps_everything():
    assert DC.keep_mask(33, 77, DC.P_TINY, DC.SEED, DC.STEP, DC.SITE).all()


def test_masks_of_different_site_step_seed_differ():
    a = DC.keep_mask(33, 77, 0.5, DC.SEED, DC.STEP, DC.SITE)
    for other in (DC.keep_mask(33, 77, 0.5, DC.SEED, DC.STEP, DC.SITE + 1), DC.keep_mask(33, 77, 0.5, DC.SEED, DC.STEP + 1, DC.SITE),
                  DC.keep_mask(33, 77, 0.5, DC.SEED + 1, DC.STEP, DC.SITE), DC.keep_mask(33, 77, 0.5, DC.SEED + (1 << 32), DC.STEP, DC.SITE)):
        # two independent fair masks of 2541 elements agree on ~half: far from all
        assert 0.4 < (a == other).mean() < 0.6
    # only the low word of the step enters the counter
    assert (a == DC.keep_mask(33, 77, 0.5, DC.SEED, DC.STEP + (1 << 32), DC.SITE)).all()


@pytest.mark.parametrize("b", [1, 3, 4, 77, (1 << 34) - 6])
def test_base_is_an_offset_into_one_stream(b):
    if b < 1000:
        full = DC.words(b + 40, DC.SEED, DC.STEP, DC.SITE)
        assert (DC.words(40, DC.SEED, DC.STEP, DC.SITE, base=b) == full[b:]).all()
    else:       # past 2^34 the group index needs the counter's second word
        w = DC.words(16, DC.SEED, DC.STEP, DC.SITE, base=b)
        g = (b + np.arange(16)) >> 2
        assert g.min() < (1 << 32) <= g.max()
        for k in range(16):
            i = b + k
            ref = DC.philox4x32_10(((i >> 2) & DC.MASK32, i >> 34, DC.SITE, DC.STEP), (DC.SEED & DC.MASK32, DC.SEED >> 32))
            assert int(ref[i & 3]) == int(w[k])


def test_shape_only_enters_through_the_logical_index():
    assert (DC.keep_mask(3, 5, 0.5, 1, 2, 3).ravel() == DC.keep_mask(5, 3, 0.5, 1, 2, 3).ravel()).all()


def test_dispatch_predicate_and_case_table():
    assert DC.vector_path(128, 0, [128, 128, 128], [0, 16, 32])
    assert not DC.vector_path(77, 0, [80, 80], [0, 0])
    assert not DC.vector_path(128, 3, [128], [0])
    assert not DC.vector_path(128, 0, [128, 130], [0])
    assert not DC.vector_path(128, 0, [128], [0, 4])
    paths = {c.path for c in DC.CASES}
    assert paths == {"vector", "scalar", "none"}
    assert len({c.id for c in DC.CASES}) == len(DC.CASES)
    for c in DC.CASES:
        ld = c.ld or c.C
        assert ld >= c.C
        want = "none" if c.R == 0 else ("vector" if DC.vector_path(c.C, c.base, [ld], [4 if c.offset else 0]) else "scalar")
        assert c.path == want, c.id
    # the issue's shapes, each in the three layouts with and without a residual
    for R, C, ld0 in DC.SHAPES:
        rows = [c for c in DC.CASES if (c.R, c.C) == (R, C) and c.base == 0]
        assert {(False, False), (False, True), (True, False), (True, True)} <= {(c.offset, c.residual) for c in rows}, (R, C)
        assert any((c.ld or C) > (ld0 or C) for c in rows), (R, C)
    # groups that straddle rows; both paths past one grid pass; the high counter word
    assert any(c.C % 4 and c.R > 1 for c in DC.CASES)
    for path in ("vector", "scalar"):
        assert any(c.path == path and DC.n_groups(c.R, c.C, c.base, path == "vector") > DC.ONE_PASS_GROUPS for c in DC.CASES)
    assert any(c.base < (1 << 34) <= c.base + c.R * c.C for c in DC.CASES)
    assert {c.p for c in DC.CASES} >= {0.1, 0.5, 0.9, DC.P_TINY}


def test_fixtures_were_drawn_by_this_generator():
    """Every dropout fixture records the masks its reference forward drew (site order) with their parameters: they are keep_mask's."""
    files = sorted(glob.glob(os.path.join(GOLDEN, "dropout_*.npz")))
    assert files, "no dropout fixtures"
    for f in files:
        z = np.load(f)
        seed, step, p = int(z["meta/dropout_seed"]), int(z["meta/dropout_step"]), float(z["meta/dropout_p"])
        shapes = z["meta/dropout_site_shapes"]
        assert len(shapes) >= 1
        for s, (R, C) in enumerate(shapes):
            want = DC.keep_mask(int(R), int(C), p, seed, step, s)
            got = np.unpackbits(z[f"out/dropout_mask/{s}"])[:R * C].astype(bool).reshape(R, C)
            assert (got == want).all(), (f, s)
        assert f"out/dropout_mask/{len(shapes)}" not in z.files


# ----------------------------------------------------------------------------- the opt-in (no GPU: constructors only)
def test_dropout_is_opt_in_by_class():
    """The classes every other test builds refuse dropout > 0 with their old messages; dropout_models.py's subclasses take it and add no
    parameter, buffer or state_dict key."""
    import test_lap_baselines_cpu as LC
    from signnet_basisnet_amd import dgl_nets, dropout_models, pyg, pyg_gnn_types
    with pytest.raises(NotImplementedError, match=r"GNN: dropout > 0 is not built on the HIP path \(core/config.py's default is 0\)"):
        pyg.GNN(None, None, 16, 1, 2, "gine", dropout=0.1)
    for kind in pyg_gnn_types.GNN_TYPES:
        with pytest.raises(NotImplementedError, match="dropout > 0 is not built"):
            pyg_gnn_types.GNN(None, None, 16, 1, 2, kind, 0.5, "add")
        m = dropout_models.GNN(None, None, 16, 1, 2, kind, 0.5, "add")
        assert m.dropout == 0.5 and list(m.state_dict()) == list(pyg_gnn_types.GNN(None, None, 16, 1, 2, kind, 0, "add").state_dict())
        with pytest.raises(ValueError, match="between 0 and 1"):
            dropout_models.GNN(None, None, 16, 1, 2, kind, 1.5, "add")
    with pytest.raises(NotImplementedError, match="HIP GatedGCNLayer: dropout 0.0 and graph_norm=False"):
        dgl_nets.GatedGCNLayer(8, 8, 0.1, True, residual=True, graph_norm=False)
    for cls in ("GINNet", "GatedGCNNet", "GATNet", "PNANet", "TransformerNet"):
        name = next(n for n, (c, _) in LC.SHIPPED_BASELINES.items() if c == cls and n.endswith("NoPE"))
        base = dict(LC._COMMON, device="cpu")
        base.update(LC.SHIPPED_BASELINES[name][1], hidden_dim=40 if cls == "PNANet" else 32, out_dim=40 if cls == "PNANet" else 32)
        for bad in (dict(dropout=0.1), dict(in_feat_dropout=0.1)):
            with pytest.raises(NotImplementedError, match=rf"HIP {cls}: dropout 0.0 \(as in the shipped configs\)"):
                getattr(dgl_nets, cls)(dict(base, **bad))
        net = dropout_models.NETS[cls](dict(base, dropout=0.1, in_feat_dropout=0.2))
        ref = getattr(dgl_nets, cls)(dict(base))
        assert (net.p_drop, net.p_in_feat, net.in_feat_dropout.p) == (0.1, 0.2, 0.2)
        assert list(net.state_dict()) == list(ref.state_dict()) and len(list(net.buffers())) == len(list(ref.buffers()))
        assert isinstance(net, getattr(dgl_nets, cls))


def test_dropin_binds_the_dropout_models_only_with_the_flag():
    from signnet_basisnet_amd import dropin as D
    nets = ["nets.ZINC_graph_regression." + m for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net")]
    assert D.AliasFinder("graphprediction").table == D.ALIASES["graphprediction"]
    f = D.AliasFinder("graphprediction", feature_dropout=True)
    assert all(f.table[n] == D.FEATURE_DROPOUT_OVERRIDES["graphprediction"][n] for n in nets)
    assert f.table["nets.ZINC_graph_regression.sign_inv_net"] == D.ALIASES["graphprediction"]["nets.ZINC_graph_regression.sign_inv_net"]
    assert D.AliasFinder("gine_pyg", baselines=True, gnn_types=True).table["core.model"] == D.GNN_TYPE_OVERRIDES["gine_pyg"]["core.model"]
    assert D.AliasFinder("gine_pyg", baselines=True, feature_dropout=True).table["core.model"] == D.FEATURE_DROPOUT_OVERRIDES["gine_pyg"]["core.model"]
    import importlib
    mod = importlib.import_module(D.FEATURE_DROPOUT_OVERRIDES["graphprediction"][nets[1]])
    from signnet_basisnet_amd import dropout_models
    assert mod.GatedGCNNet is dropout_models.GatedGCNNet
    assert importlib.import_module(D.FEATURE_DROPOUT_OVERRIDES["gine_pyg"]["core.model"]).GNN is dropout_models.GNN
