"""CPU: dropout in the sign-invariant encoders of the DGL tree (signnet_basisnet_amd.dropout_signinv) — what needs no device.  The site
table of tests/signinv_dropout_cases.py against the masks the reference's own modules drew (tests/golden/ds_dropout_*.npz), the opt-in
surface (the existing refusals stay, the new classes construct with the same state_dict keys), the drop-in tables, and the host-side
path predicate of sn_affine_dropout_f32."""
import importlib
import re

import numpy as np
import pytest
import torch

import dropout_cases as DC
import golden_util as G
import signinv_dropout_cases as SC


def _net_params(kind, dropout, lap_method="sign_inv", **over):
    p = dict(num_atom_type=28, num_bond_type=4, hidden_dim=12, out_dim=12, in_feat_dropout=0.0, dropout=dropout, L=2, readout="mean",
             batch_norm=True, residual=True, edge_feat=True, device="cpu", pe_init="lap_pe", lap_method=lap_method, lap_lspe=False,
             use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4, pos_enc_dim=4, sign_inv_net=kind, sign_inv_layers=3,
             sign_inv_activation="relu", phi_out_dim=4, pe_aggregate="add")
    p.update(over)
    return p


# ----------------------------------------------------------------------------- the site table against the reference's recorded sites
@pytest.mark.parametrize("name", SC.ENCODER_CASES)
def test_site_table_reproduces_the_encoder_fixtures(name):
    fx = G.load(name)
    kind = str(fx.meta["kind"])
    hidden, _, L, k = (int(v) for v in fx.meta["params"])
    N = int(sum(int(s) for s in fx.inp["sizes"]))
    table = SC.site_table(kind, N, hidden, L, k)
    assert len(table) == SC.site_count(kind, L) == len(fx.meta["dropout_sites"])
    assert [t[0] for t in table] == [int(s) for s in fx.meta["dropout_sites"]]
    assert [[t[1], t[2]] for t in table] == fx.meta["dropout_site_shapes"].tolist()
    p, seed, step = float(fx.meta["dropout_p"]), int(fx.meta["dropout_seed"]), int(fx.meta["dropout_step"])
    assert all(float(q) == p for q in fx.meta["dropout_site_p"])
    for s, keep in enumerate(SC.masks(table, p, seed, step)):
        rec = SC.unpack(fx.out[f"dropout_mask/{s}"].numpy(), fx.meta["dropout_site_shapes"][s])
        assert np.array_equal(keep, rec), f"{name}: site {s}"
    # the two encoder calls draw different masks
    per_call = (len(table) - (3 if kind == "transformer" else L - 1)) // 2
    if per_call:
        m = SC.masks(table, p, seed, step)
        assert not np.array_equal(m[0], m[per_call])


def test_site_counts():
    for L in (2, 3, 4, 8):
        assert SC.site_count("gin", L) == SC.site_count("masked_gin", L) == 5 * L - 3
        assert SC.site_count("gcn", L) == 3 * L - 3
        assert SC.site_count("transformer", L) == 3
        assert SC.fused_sites("gin", L) == 3 * L - 1 and SC.fused_sites("gcn", L) == L - 1 and SC.fused_sites("transformer", L) == 3
    assert SC.site_count("gin", 8) == 37          # the shipped sign_inv_layers


@pytest.mark.parametrize("name", SC.NET_CASES)
def test_site_table_reproduces_the_net_fixtures(name):
    """handle_lap + net: the encoder's sites in its own range, then the net's small ordinals from 0 (tests/golden/make_dropout.py's rule)."""
    fx = G.load(name)
    kind = str(fx.meta["kind"])
    hidden, _, k = (int(v) for v in fx.meta["hidden_L_k"])
    N = int(sum(int(s) for s in fx.inp["sizes"]))
    table = SC.site_table(kind, N, hidden, SC.NET_SIGN_INV_LAYERS, k)
    sites = [int(s) for s in fx.meta["dropout_sites"]]
    n = len(table)
    assert sites[:n] == [t[0] for t in table] and sites[n:] == list(range(len(sites) - n)) and len(sites) > n
    assert [[t[1], t[2]] for t in table] == fx.meta["dropout_site_shapes"][:n].tolist()
    p, seed, step = float(fx.meta["dropout_p"]), int(fx.meta["dropout_seed"]), int(fx.meta["dropout_step"])
    for s, (site, shape) in enumerate(zip(sites, fx.meta["dropout_site_shapes"])):
        keep = DC.keep_mask(int(shape[0]), int(shape[1]), p, seed, step, site)
        assert np.array_equal(keep, SC.unpack(fx.out[f"dropout_mask/{s}"].numpy(), shape)), f"{name}: site {s}"


def test_site_range_is_disjoint_from_the_others():
    from signnet_basisnet_amd import ops
    assert ops.SIGNINV_DROP_SITE == SC.SITE0 == 0x53490000
    hdr = open(importlib.import_module("test_abi").HEADER).read()
    assert re.search(r"#define\s+SN_SIGNINV_DROP_SITE\s+0x53490000u", hdr)
    assert SC.SITE0 > 1 << 16 and abs(SC.SITE0 - ops.ATTN_DROP_SITE) > 1 << 16


# ----------------------------------------------------------------------------- opt-in surface
def _ctor_args(kind):
    return (1, 8, 4, 3, 4) + (("cpu",) if kind == "masked_gin" else ())


@pytest.mark.parametrize("kind", list(SC.CLASSES))
def test_base_classes_still_refuse_and_the_new_classes_construct(kind):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import dropout_signinv as S
    cls = SC.CLASSES[kind]
    with pytest.raises(NotImplementedError, match=rf"{cls}: dropout=0.1 is not implemented by the HIP modules"):
        getattr(DS, cls)(*_ctor_args(kind), use_bn=True, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout=0.1"):
        DS.get_sign_inv_net(_net_params(kind, 0.1))
    new = getattr(S, cls)(*_ctor_args(kind), use_bn=True, dropout=0.1)
    base = getattr(DS, cls)(*_ctor_args(kind), use_bn=True, dropout=0.0)
    assert isinstance(new, getattr(DS, cls)) and new.p_drop == 0.1 and base.p_drop == 0.0
    assert list(new.state_dict().keys()) == list(base.state_dict().keys())
    assert [tuple(v.shape) for v in new.state_dict().values()] == [tuple(v.shape) for v in base.state_dict().values()]
    assert len(list(new.buffers())) == len(list(base.buffers()))
    made = S.get_sign_inv_net(_net_params(kind, 0.1, hidden_dim=8))
    assert type(made) is getattr(S, cls) and list(made.state_dict().keys()) == list(base.state_dict().keys())
    with pytest.raises(ValueError, match="between 0 and 1"):
        getattr(S, cls)(*_ctor_args(kind), use_bn=True, dropout=1.5)
    with pytest.raises(ValueError, match="Invalid sign inv net"):
        S.get_sign_inv_net(_net_params("gat", 0.1))
    # the site arithmetic of the module equals the table's
    L = 3
    n_rho = len(new.rho.lins) - 1
    assert 2 * new._enc_sites() + n_rho == SC.site_count(kind, L)
    assert new._rho_site0() == SC.SITE0 + 2 * new._enc_sites()


@pytest.mark.parametrize("cls", ["GINNet", "GatedGCNNet", "PNANet", "TransformerNet", "GATNet"])
def test_nets_refuse_as_before_and_the_new_nets_build_the_new_encoder(cls):
    from signnet_basisnet_amd import dgl_nets, dropout_models
    from signnet_basisnet_amd import dropout_signinv as S
    extra = {}
    if cls == "PNANet":
        extra = dict(graph_norm=True, aggregators="mean max min std", scalers="identity amplification attenuation", towers=4,
                     divide_input_first=True, divide_input_last=True, edge_dim=8, pretrans_layers=1, posttrans_layers=1, gru=False,
                     avg_d=dict(lin=torch.tensor(2.2), exp=torch.tensor(0.6), log=torch.tensor(1.1)), readout="sum")
    if cls in ("TransformerNet", "GATNet"):
        extra = dict(n_heads=4, full_graph=False, layer_norm=True)
    params = _net_params("gin", 0.1, **extra)
    with pytest.raises(NotImplementedError):
        getattr(dgl_nets, cls)(params)
    if cls != "GATNet":                       # (gat_net.py reads `dropout` and never uses it: its own refusal is in_feat_dropout's)
        with pytest.raises(NotImplementedError, match="GINDeepSigns: dropout=0.1"):
            getattr(dropout_models, cls)(params)
    net = getattr(S, cls)(params)
    assert S.NETS[cls] is getattr(S, cls) and isinstance(net, getattr(dropout_models, cls))
    assert type(net.sign_inv_net) is S.GINDeepSigns and net.sign_inv_net.p_drop == 0.1
    base = getattr(dgl_nets, cls)(dict(params, dropout=0.0))
    assert list(net.state_dict().keys()) == list(base.state_dict().keys())
    assert type(base.sign_inv_net).__module__.endswith("dgl_deepsigns")
    # without a sign-invariant encoder the new nets are the dropout_models nets
    plain = getattr(S, cls)(dict(params, pe_init="no_pe", lap_method="none", pe_aggregate="none"))
    assert not hasattr(plain, "sign_inv_net")
    plain.seed_dropout(3, 1)


# ----------------------------------------------------------------------------- drop-in
NAMES = ["nets.ZINC_graph_regression." + m for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net", "sign_inv_net")]


def test_dropin_binds_the_new_modules_only_with_the_flag():
    from signnet_basisnet_amd import dropin as D
    from signnet_basisnet_amd import dropout_signinv as S
    assert set(D.SIGN_INV_DROPOUT_OVERRIDES["graphprediction"]) == set(NAMES)
    assert D.AliasFinder("graphprediction").table == D.ALIASES["graphprediction"]
    f = D.AliasFinder("graphprediction", feature_dropout=True)
    assert f.table[NAMES[-1]] == D.ALIASES["graphprediction"][NAMES[-1]]
    assert all(f.table[n] == D.FEATURE_DROPOUT_OVERRIDES["graphprediction"][n] for n in NAMES[:-1])
    f = D.AliasFinder("graphprediction", sign_inv_dropout=True)
    assert all(f.table[n] == D.SIGN_INV_DROPOUT_OVERRIDES["graphprediction"][n] for n in NAMES)
    assert f.table["layers.deepsigns"] == D.ALIASES["graphprediction"]["layers.deepsigns"]
    # the flag implies feature_dropout for the trees it does not name
    assert D.AliasFinder("gine_pyg", baselines=True, sign_inv_dropout=True).table["core.model"] == \
        D.FEATURE_DROPOUT_OVERRIDES["gine_pyg"]["core.model"]
    mod = importlib.import_module(D.SIGN_INV_DROPOUT_OVERRIDES["graphprediction"][NAMES[1]])
    assert mod.GatedGCNNet is S.GatedGCNNet and mod.get_sign_inv_net is S.get_sign_inv_net
    assert all(getattr(mod, c) is S.NETS[c] for c in S.NETS)


def _resolve(finder, name):
    """The module the installed finder answers `name` with (the parent packages `nets` / `nets.ZINC_graph_regression` are the tree's)."""
    spec = finder.find_spec(name)
    assert spec is not None and spec.origin == finder.table[name]
    return importlib.import_module(spec.origin)


def test_install_resolves_the_entry_scripts_names_to_the_new_classes():
    """What `dropin.run --sign-inv-dropout main_ZINC_graph_regression.py --config ..._LapPE_signinv_GIN.json --dropout 0.1` imports."""
    from signnet_basisnet_amd import dgl_deepsigns, dgl_nets
    from signnet_basisnet_amd import dropin as D
    from signnet_basisnet_amd import dropout_signinv as S
    D.uninstall("graphprediction")
    try:
        f = D.install("graphprediction", feature_dropout=True)
        assert _resolve(f, NAMES[1]).GatedGCNNet is not S.GatedGCNNet
        assert D.install("graphprediction", sign_inv_dropout=True) is f          # extends the installed finder in place
        gated = _resolve(f, NAMES[1])
        assert gated.GatedGCNNet is S.GatedGCNNet
        assert _resolve(f, NAMES[-1]).get_sign_inv_net is S.get_sign_inv_net
        net = gated.GatedGCNNet(_net_params("gin", 0.1))
        assert type(net.sign_inv_net) is S.GINDeepSigns
        D.install("graphprediction", feature_dropout=True)                       # a later call with less takes nothing away
        assert _resolve(f, NAMES[1]).GatedGCNNet is S.GatedGCNNet
        assert f.find_spec("nets.ZINC_graph_regression.load_net") is None         # everything else stays the tree's
    finally:
        D.uninstall("graphprediction")
    f = D.install("graphprediction")
    try:
        assert _resolve(f, NAMES[1]).GatedGCNNet is dgl_nets.GatedGCNNet
        assert _resolve(f, NAMES[-1]).get_sign_inv_net is dgl_deepsigns.get_sign_inv_net
    finally:
        D.uninstall("graphprediction")


def test_runner_knows_the_flag():
    from signnet_basisnet_amd.dropin import run
    assert "--sign-inv-dropout" in run.__doc__
    with pytest.raises(SystemExit, match=r"\[--sign-inv-dropout\]"):
        run.main(["--sign-inv-dropout"])


# ----------------------------------------------------------------------------- the host's path predicate
@pytest.mark.parametrize("args,want", SC.PATH_TABLE)
def test_path_predicate(args, want):
    assert SC.path(*args) == want


def test_path_table_falsifies_every_clause_alone():
    row = SC.PATH_TABLE[0][0]
    flat = SC.PATH_TABLE[2][0]
    assert SC.path(*row) == "row" and SC.path(*flat) == "flat"
    one_off = lambda a, b: sum(x != y for x, y in zip(a, b)) == 1        # noqa: E731
    off_row = [a for a, w in SC.PATH_TABLE if w != "row" and one_off(a, row)]
    assert {tuple(i for i in range(8) if a[i] != row[i]) for a in off_row} >= {(3,), (4,), (5,), (6,), (7,)}
    off_flat = [a for a, w in SC.PATH_TABLE if w == "scalar" and one_off(a, flat)]
    assert {tuple(i for i in range(8) if a[i] != flat[i]) for a in off_flat} == {(1,), (2,), (3,), (4,), (5,)}
    # group counts: the shipped odd width moves in 128-bit accesses on the flat path
    assert SC.n_groups(111037, 67, 0, "flat") == (111037 * 67 + 3) // 4
    assert SC.n_groups(*SC.BIG, 0, "row") > SC.MAX_BLOCKS * 256 and SC.n_groups(*SC.BIG_FLAT, 0, "flat") > SC.MAX_BLOCKS * 256
    nv = SC.nvalid_for(7)
    assert nv.tolist() == [0, 1, 2] and SC.rowvalid(7, nv).tolist() == [False, False, False, True, False, False, True]
