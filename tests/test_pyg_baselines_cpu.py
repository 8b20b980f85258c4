"""CPU: the PyG trees' baselines (NetGINE with its Set2Set readout, the plain GINE GNN) as far as they go without a GPU — the float
restatements of tests/pyg_baseline_cases.py reproduce the reference's own outputs (tests/golden/netgine_*.npz, plain_gnn_*.npz), the HIP
modules load the reference's state_dicts strictly, the two new entry points validate on the host, the drop-in binds the baselines only
when asked to, and what is not built refuses loudly."""
import sys

import pytest
import torch

import golden_util as G
import pyg_baseline_cases as C
from parity_util import close
from test_dropin_cpu import REPORT, _run, make_alchemy_tree, make_gine_tree

FIXTURE_REL = 1e-6


def _gnn_meta(fx):
    nhid, nlayer = (int(v) for v in fx.meta["nhid_nlayer"])
    return nhid, nlayer, str(fx.meta["pooling"])


# ----------------------------------------------------------------------------- the restatements are the reference's modules
@pytest.mark.parametrize("name", C.NETGINE_CASES)
def test_netgine_restatement_reproduces_the_reference(name):
    fx, gr = G.load(name), G.load(name + "_grads")
    data = G.as_data(fx.inp)
    sd = C.leaf_state_dict(fx.sd, torch.float32)
    y = C.netgine_ref(sd, data)
    close(y, fx.out["eval/y"], f"{name}: y", rel=FIXTURE_REL)
    loss = torch.nn.functional.l1_loss(y, fx.inp["y_target"])
    close(loss, fx.out["loss"][0].float(), f"{name}: loss", rel=FIXTURE_REL)
    loss.backward()
    sd64 = C.leaf_state_dict(fx.sd, torch.float64)
    torch.nn.functional.l1_loss(C.netgine_ref(sd64, _f64(data)), fx.inp["y_target"].double()).backward()
    assert set(gr.out) == {"grad/" + k for k in fx.sd}
    for k in fx.sd:          # two fp32 evaluations of one gradient: equal at 1e-6 or both as close to float64
        close(sd[k].grad, gr.out["grad/" + k], f"{name}: d {k}", rel=FIXTURE_REL, ref64=sd64[k].grad)


def _f64(data):
    import parity_util as PU
    return PU.data_f64(data)


@pytest.mark.parametrize("name", C.PLAIN_GNN_CASES)
def test_plain_gnn_restatement_reproduces_the_reference(name):
    fx = G.load(name)
    data = G.as_data(fx.inp)
    _, nlayer, pooling = _gnn_meta(fx)
    pe = fx.inp.get("additional_x")
    assert (pe is not None) == name.endswith("_pe")
    with torch.no_grad():
        close(C.plain_gnn_ref(fx.sd, nlayer, pooling, data, pe, False), fx.out["eval/y"], f"{name}: eval y", rel=FIXTURE_REL)
        close(C.plain_gnn_ref(fx.sd, nlayer, pooling, data, pe, True), fx.out["train/y"], f"{name}: train y", rel=FIXTURE_REL)


@pytest.mark.parametrize("case", ["d4_T6", "d64_T6", "d100_T6"])
def test_set2set_restatement_is_finite_and_two_orders_inside_the_gate(case):
    inp = C.set2set_inputs(case)
    with torch.no_grad():
        o32 = C.set2set_ref(inp.x, inp.sizes, inp.lstm, inp.T)
        o64 = C.set2set_ref(inp.x.double(), inp.sizes, {k: v.double() for k, v in inp.lstm.items()}, inp.T)
    assert torch.isfinite(o32).all() and o32.shape == (len(inp.sizes), 2 * inp.d)
    assert torch.equal(o32[1, inp.d:], torch.zeros(inp.d))          # the empty graph: r = 0
    close(o32, o64, case, rel=2e-7)


# ----------------------------------------------------------------------------- the modules take the reference's checkpoints
@pytest.mark.parametrize("name", C.NETGINE_CASES)
def test_netgine_loads_the_reference_state_dict_strictly(name):
    from signnet_basisnet_amd.pyg_baselines import NetGINE
    fx = G.load(name)
    m = NetGINE(int(fx.meta["dim"]))
    m.load_state_dict(fx.sd, strict=True)
    assert [str(k) for k in fx.meta["sd_keys"]] == list(m.state_dict().keys())


@pytest.mark.parametrize("name", C.PLAIN_GNN_CASES)
def test_plain_gnn_loads_the_reference_state_dict_strictly(name):
    from signnet_basisnet_amd.dropin.baseline_core_model import GNN
    fx = G.load(name)
    nhid, nlayer, pooling = _gnn_meta(fx)
    m = GNN(None, None, nhid, 1, nlayer, "GINEConv", 0, pooling, res=True)          # train/zinc.py:38-46
    m.load_state_dict(G.full_state_dict(fx), strict=True)
    assert sorted(str(k) for k in fx.meta["sd_keys"]) == sorted(m.state_dict().keys())


# ----------------------------------------------------------------------------- ABI
def test_set2set_entry_points_validate_on_the_host():
    from signnet_basisnet_amd import _lib, build
    build.build()
    lib = _lib.lib()
    rc = lib.sn_set2set_f32(None, 4, 8, None, 1, None, None, None, None, 6, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"sn_set2set_f32" in lib.sn_last_error()
    rc = lib.sn_set2set_bwd_f32(None, 4, 8, None, 1, None, None, 6, *([None] * 10))
    assert rc == -1 and b"sn_set2set_bwd_f32" in lib.sn_last_error()
    assert "sn_set2set_f32" in _lib.SIGNATURES and "sn_set2set_bwd_f32" in _lib.SIGNATURES


# ----------------------------------------------------------------------------- drop-in: opt-in only
def test_runner_binds_the_baselines_only_with_the_flag(tmp_path):
    for tree, make, name in (("alchemy", make_alchemy_tree, "NetGINE"), ("gine_pyg", make_gine_tree, "GNN")):
        root = tmp_path / tree
        root.mkdir()
        script, expected = make(str(root))
        assert expected[name] == "tree"
        got = _run([sys.executable, "-m", "signnet_basisnet_amd.dropin.run", script], cwd=str(root))
        assert {k: got.get(k) for k in expected} == expected
        got = _run([sys.executable, "-m", "signnet_basisnet_amd.dropin.run", "--baselines", script], cwd=str(root))
        assert {k: got.get(k) for k in expected} == dict(expected, **{name: "hip"})


def test_install_binds_the_baselines_only_when_asked(tmp_path):
    make_alchemy_tree(str(tmp_path))
    for flag, origin in (("", "tree"), ("baselines=True", "hip")):
        code = (f"import sys; sys.path.insert(0, {str(tmp_path)!r})\nimport signnet_basisnet_amd.dropin as D\n"
                f"D.install('alchemy', {flag})\nfrom baseline_gin import NetGINE\nfrom sign_net.sign_net import SignNetGNN\n" + REPORT)
        got = _run([sys.executable, "-c", code], cwd=str(tmp_path))
        assert got["NetGINE"] == origin and got["SignNetGNN"] == "hip"


def test_baseline_names_live_in_their_own_table():
    import signnet_basisnet_amd.dropin as D
    assert D.BASELINE_ALIASES == {"alchemy": {"baseline_gin": "signnet_basisnet_amd.pyg_baselines"},
                                  "gine_pyg": {"core.model": "signnet_basisnet_amd.dropin.baseline_core_model"}}
    for tree, table in D.BASELINE_ALIASES.items():
        assert not set(table) & set(D.ALIASES[tree])
        assert all(D.AliasFinder(tree).find_spec(n) is None for n in table)
        assert all(D.AliasFinder(tree, baselines=True).find_spec(n) is not None for n in table)
        assert all(D.AliasFinder(tree, baselines=True).find_spec(n) is not None for n in D.ALIASES[tree])


# ----------------------------------------------------------------------------- refusals
def test_what_is_not_built_refuses():
    from signnet_basisnet_amd import ops, pyg
    from signnet_basisnet_amd.dropin.baseline_core_model import GNN
    from signnet_basisnet_amd.pyg_baselines import NetGINE
    with pytest.raises(NotImplementedError, match="dropout"):
        GNN(None, None, 16, 1, 2, "GINEConv", 0.5, "add")
    with pytest.raises(NotImplementedError, match="res=False"):
        GNN(None, None, 16, 1, 2, "GINEConv", 0, "add", res=False)
    with pytest.raises(NotImplementedError, match="GINEConv"):
        GNN(None, None, 16, 1, 2, "GCNConv")
    with pytest.raises(NotImplementedError, match="dropout"):
        pyg.GNN(None, None, 16, 1, 2, "gine", dropout=0.1)
    with pytest.raises(NotImplementedError):
        pyg.GNN(None, None, 16, 1, 2, "alchemy")(G.as_data(G.load("netgine_d16").inp))
    fx = G.load("plain_gnn_h16_l2_add")
    for mode in (True, False):          # host tensors: no CPU path, in either mode
        with pytest.raises(RuntimeError, match="GPU only"):
            GNN(None, None, 16, 1, 2, "GINEConv").train(mode)(G.as_data(fx.inp))
        with pytest.raises(RuntimeError, match="GPU only"):
            NetGINE(16).train(mode)(G.as_data(G.load("netgine_d16").inp))
    inp = C.set2set_inputs("d4_T1")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.set2set(inp.x, torch.zeros(len(inp.sizes) + 1, dtype=torch.int32), *inp.lstm.values(), inp.T)
