"""CPU: the plain GNN for every model.gnn_type (pyg_gnn_types.py) as far as it goes without a GPU — the restatements of
tests/gnn_type_cases.py reproduce the reference's own outputs and buffers (tests/golden/gnn_types_*.npz, made by make_gnn_types.py from
core/model.py over pyg_gnn_wrapper.py), the HIP modules have the reference's state_dict keys and shapes, what is not built refuses, the
drop-in binds the new `core.model` only with the new flag, the new entry points validate on the host, and the kernel case table covers
both sides of every dispatch predicate of csrc/simplified_pna.hip."""
import json
import sys

import pytest
import torch

import gnn_type_cases as C
import golden_util as G
import test_oracle_golden as TOG
from test_dropin_cpu import _run, make_gine_tree

TOL = TOG.TOL_BS          # the tolerance of test_oracle_golden.py's train-mode fixtures


def _meta(fx):
    nhid, nlayer = (int(v) for v in fx.meta["nhid_nlayer"])
    return str(fx.meta["gnn_type"]), nhid, nlayer, str(fx.meta["pooling"])


def _model(fx):
    from signnet_basisnet_amd.pyg_gnn_types import GNN
    kind, nhid, nlayer, pooling = _meta(fx)
    return GNN(None, None, nhid, 1, nlayer, kind, 0, pooling, res=True)          # train/zinc.py:38-46


# ----------------------------------------------------------------------------- the restatements are the reference's modules
@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_restatement_reproduces_the_reference(name):
    fx = G.load(name)
    kind, nhid, nlayer, pooling = _meta(fx)
    assert (kind, nhid, nlayer, pooling) == C.FIXTURES[name][:4]
    data, pe = G.as_data(fx.inp), fx.inp.get("additional_x")
    sd = G.full_state_dict(fx)
    with torch.no_grad():
        y = C.gnn_ref(sd, kind, nlayer, pooling, data, pe, False)
        buffers = {}
        yt = C.gnn_ref(sd, kind, nlayer, pooling, data, pe, True, buffers)
    torch.testing.assert_close(y, fx.out["eval/y"], **TOL)
    torch.testing.assert_close(yt, fx.out["train/y"], **TOL)
    assert (fx.out["train/y"] - fx.out["eval/y"]).abs().max() > 1e-3          # (the two modes differ: the buffers are not trivial)
    seen = 0
    for k, ref in fx.out.items():
        if not k.startswith("train/buffers/"):
            continue
        key = k[len("train/buffers/"):]
        got = buffers.get(key, sd[key])             # a BatchNorm the forward never calls keeps its buffers
        if key.endswith("num_batches_tracked"):
            assert int(got) == int(ref), key
        else:
            torch.testing.assert_close(got, ref, **TOL, msg=lambda m, key=key: f"{key}: {m}")
        seen += 1
    assert seen >= 3 * (nlayer + (pooling != "mean"))          # norms.l, and output_encoder.norms.0 unless the pooling is 'mean'


def test_the_fixture_batches_have_what_the_wrappers_treat_differently():
    for name in C.FIXTURES:
        ei = G.load(name).inp["edge_index"]
        pairs = set(map(tuple, ei.t().tolist()))
        assert bool((ei[0] == ei[1]).any()) and len(pairs) < ei.shape[1]          # self loops, multi-edges
        assert any((b, a) not in pairs for a, b in pairs)                          # a one-directional edge


# ----------------------------------------------------------------------------- the modules: keys, shapes, unused buffers
@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_state_dict_keys_and_shapes_are_the_references(name):
    fx = G.load(name)
    m = _model(fx)
    sd = m.state_dict()
    assert [str(k) for k in fx.meta["sd_keys"]] == list(sd.keys())
    assert [str(s) for s in fx.meta["sd_shapes"]] == [",".join(map(str, v.shape)) for v in sd.values()]
    m.load_state_dict(G.full_state_dict(fx), strict=True)


def test_gat_and_gin_double_registrations_alias_one_tensor():
    from signnet_basisnet_amd.pyg_gnn_types import GNN
    g = GNN(None, None, 16, 1, 1, "GATConv").convs[0].layer
    assert g.lin_src.weight is g.lin_dst.weight and g.att_src.shape == (1, 1, 16)
    g = GNN(None, None, 16, 1, 1, "GINConv").convs[0]
    assert g.nn.layers[0].weight is g.layer.nn.layers[0].weight and g.nn.layers[0].bias is not None and g.nn.layers[1].bias is not None
    assert not [k for k in g.state_dict() if "norms" in k]
    assert "layer.bias" not in GNN(None, None, 16, 1, 1, "GCNConv").convs[0].state_dict()          # GNN passes bias=not bn


def test_unused_norms_keep_their_buffers_in_the_fixtures():
    for name, spec in C.FIXTURES.items():
        if spec[0] != "SimplifiedPNAConv":
            continue
        fx = G.load(name)
        keys = [k for k in fx.out if k.startswith("train/buffers/") and ".norms.1.num_batches_tracked" in k and "output_encoder" not in k]
        assert len(keys) == 2 * spec[2]
        assert all(int(fx.out[k]) == 0 for k in keys)
        used = [k for k in fx.out if k.startswith("train/buffers/") and ".norms.0.num_batches_tracked" in k]
        assert used and all(int(fx.out[k]) == 1 for k in used)


# ----------------------------------------------------------------------------- refusals
def test_what_is_not_built_refuses():
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.pyg_gnn_types import GNN, GATConv, SimplifiedPNAConv
    for kind in ("GINEConv", "GINConv", "GCNConv", "GATConv", "SimplifiedPNAConv"):
        with pytest.raises(NotImplementedError, match="dropout"):
            GNN(None, None, 16, 1, 2, kind, 0.5, "add")
        with pytest.raises(NotImplementedError, match="res=False"):
            GNN(None, None, 16, 1, 2, kind, 0, "add", res=False)
        with pytest.raises(NotImplementedError, match="bn=False"):
            GNN(None, None, 16, 1, 2, kind, 0, "add", bn=False)
        with pytest.raises(NotImplementedError, match="dos_bins"):
            GNN(None, None, 16, 1, 2, kind, 0, "add", dos_bins=4)
    with pytest.raises(ValueError, match="gnn_type"):
        GNN(None, None, 16, 1, 2, "SignNet")
    with pytest.raises(NotImplementedError, match="aggregators"):
        SimplifiedPNAConv(16, 16, aggregators=["mean", "max"])
    with pytest.raises(ValueError, match="128"):
        GNN(None, None, 132, 1, 2, "SimplifiedPNAConv")
    GNN(None, None, 128, 1, 1, "SimplifiedPNAConv")
    with pytest.raises(ValueError, match="nhead"):
        GATConv(16, 16, nhead=3)
    with pytest.raises(ValueError, match="nhead"):
        GATConv(64, 64, nhead=32)
    assert GATConv(16, 16, nhead=4).layer.att_src.shape == (1, 4, 4)
    for name in ("gnn_types_gin_h16_l2_add", "gnn_types_gcn_h16_l2_add", "gnn_types_gat_h16_l2_add", "gnn_types_pna_h16_l2_add"):
        fx = G.load(name)
        for mode in (True, False):          # host tensors: no CPU path, in either mode
            with pytest.raises(RuntimeError, match="GPU only"):
                _model(fx).train(mode)(G.as_data(fx.inp))
    x = C.kernel_inputs("c12")
    plan = type("P", (), dict(N=x.N, E=x.E, rowptr=None, col=None, eperm=None))()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.spna_mean(x.A, x.B_, x.Q, plan, x.gamma, x.beta)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gcn_pyg_propagate(x.A, plan, torch.ones(x.N))


# ----------------------------------------------------------------------------- drop-in: opt-in only
def test_gnn_type_overrides_live_in_their_own_table():
    import signnet_basisnet_amd.dropin as D
    assert D.GNN_TYPE_OVERRIDES == {"gine_pyg": {"core.model": "signnet_basisnet_amd.dropin.gnn_types_core_model"}}
    assert D.BASELINE_ALIASES == {"alchemy": {"baseline_gin": "signnet_basisnet_amd.pyg_baselines"},
                                  "gine_pyg": {"core.model": "signnet_basisnet_amd.dropin.baseline_core_model"}}
    assert D.BASELINE_OVERRIDES == {"learningfilters": {"models": "signnet_basisnet_amd.dropin.baseline_filter_models"}}
    assert D.ALL_BASELINE_OVERRIDES == {"learningfilters": {"models": "signnet_basisnet_amd.dropin.all_baseline_filter_models"}}
    old, new = D.BASELINE_ALIASES["gine_pyg"]["core.model"], D.GNN_TYPE_OVERRIDES["gine_pyg"]["core.model"]
    assert D.AliasFinder("gine_pyg").find_spec("core.model") is None
    assert D.AliasFinder("gine_pyg", gnn_types=False, baselines=True).find_spec("core.model").origin == old
    assert D.AliasFinder("gine_pyg", baselines="all").find_spec("core.model").origin == old
    assert D.AliasFinder("gine_pyg", baselines=True, gnn_types=True).find_spec("core.model").origin == new
    for tree in D.ALIASES:          # no other tree, and no other name of this one, resolves differently with the flag
        a, b = D.AliasFinder(tree, baselines="all").table, D.AliasFinder(tree, baselines="all", gnn_types=True).table
        assert {k: v for k, v in b.items() if a.get(k) != v} == ({"core.model": new} if tree == "gine_pyg" else {})


_WHICH = ("import sys, json\ntry:\n    GNN(None, None, 16, 1, 2, 'GCNConv')\n    built = True\nexcept NotImplementedError:\n    built = False\nexcept TypeError:\n    built = None\n"          # (the tree's stub class)
          "print('REPORT ' + json.dumps({'bound': getattr(sys.modules['core.model'], '__signnet_hip__', 'tree'), 'gcn': built}))\n")


def test_install_and_runner_bind_the_new_core_model_only_with_the_flag(tmp_path):
    make_gine_tree(str(tmp_path))
    old, new = "signnet_basisnet_amd.dropin.baseline_core_model", "signnet_basisnet_amd.dropin.gnn_types_core_model"
    for flags, want in (("baselines=True", (old, False)), ("baselines=True, gnn_types=True", (new, True))):
        code = (f"import sys; sys.path.insert(0, {str(tmp_path)!r})\nimport signnet_basisnet_amd.dropin as D\n"
                f"D.install('gine_pyg', {flags})\nfrom core.model import GNN\n" + _WHICH)
        got = _run([sys.executable, "-c", code], cwd=str(tmp_path))
        assert (got["bound"], got["gcn"]) == want
    # a finder installed with the flag keeps it when a later call does not give it
    code = (f"import sys; sys.path.insert(0, {str(tmp_path)!r})\nimport signnet_basisnet_amd.dropin as D\n"
            "D.install('gine_pyg', baselines=True, gnn_types=True)\nD.install('gine_pyg', baselines=True)\nfrom core.model import GNN\n" + _WHICH)
    assert _run([sys.executable, "-c", code], cwd=str(tmp_path))["bound"] == new
    # the runner: a script that ends like train/zinc.py's import block, as a path and as `-m train.zinc`
    with open(tmp_path / "train" / "zinc.py", "a") as f:
        f.write(_WHICH)
    (tmp_path / "train" / "__init__.py").write_text("")
    run = [sys.executable, "-m", "signnet_basisnet_amd.dropin.run"]
    assert _run(run + ["train/zinc.py"], cwd=str(tmp_path))["bound"] == "tree"
    assert _run(run + ["--baselines", "train/zinc.py"], cwd=str(tmp_path))["bound"] == old
    assert _run(run + ["--baselines", "--gnn-types", "train/zinc.py", "model.gnn_type", "SimplifiedPNAConv"], cwd=str(tmp_path)) == \
        {"bound": new, "gcn": True}
    assert _run(run + ["--baselines", "--gnn-types", "-m", "train.zinc", "model.gnn_type", "SimplifiedPNAConv"], cwd=str(tmp_path)) == \
        {"bound": new, "gcn": True}


# ----------------------------------------------------------------------------- ABI and dispatch
def test_new_entry_points_validate_on_the_host():
    from signnet_basisnet_amd import _lib, build
    build.build()
    lib = _lib.lib()
    nul = (None, 12, None, 12, None, 12)
    cases = {
        "sn_spna_stats_f32": nul + (12, 4, 8, None, None, None, None, None, 1e-5, 0.1, None, None, None, None, None, None),
        "sn_spna_mean_f32": nul + (12, 4, 8, None, None, None, None, None, None, 12, None),
        "sn_spna_bwd_f32": nul + (12, 4, 8) + (None,) * 6 + (12,) + (None,) * 5 + (12, None, 12, None, 12, None, None, None, None),
        "sn_gcn_pyg_coef_f32": (4, 8, None, None, None, None),
        "sn_gcn_pyg_propagate_f32": (None, 4, 4, 4, 8, None, None, None, None, 4, None),
    }
    for name, args in cases.items():
        assert len(args) == len(_lib.SIGNATURES[name]), name
        rc = getattr(lib, name)(*args)
        assert rc == -1 and name.encode() in lib.sn_last_error(), (name, rc, lib.sn_last_error())
    assert lib.sn_version() == 3


def test_kernel_case_table_covers_both_sides_of_every_dispatch_predicate():
    from signnet_basisnet_amd import _lib, build, ops
    build.build()
    lib = _lib.lib()
    seen = set()
    for name, (kind, Cc, ld, offset, modes) in C.KERNEL_CASES.items():
        x = C.kernel_inputs(name)
        ld = ld or Cc
        base = 4 if offset else 0                       # byte offset of every pointer inside a 16-byte aligned buffer
        vec = ops.spna_vector_path(Cc, [ld] * 4, [4096 + base] * 4)
        assert vec == bool(lib.sn_spna_vector_path(Cc, ld, ld, ld, ld, 4096 + base, 4096 + base, 4096 + base, 4096 + base))
        nblk, npb, ny, gw, slots = ops.spna_cut(x.N, Cc, vec)
        assert (("vector" if vec else "scalar"), ny) == C.expected_path(name)
        assert nblk * npb >= x.N > (nblk - 1) * npb and ny * gw >= (Cc // 4 if vec else Cc) and 1 <= slots * gw <= 256
        assert nblk <= lib.sn_spna_blocks(x.N, Cc)      # the work buffers the wrappers size hold every partial
        seen.add((vec, ny, nblk > 1, slots > 1))
    assert {s[0] for s in seen} == {True, False}          # vector and scalar
    assert {s[1] for s in seen} == {1, 2}                 # one and two column chunks
    assert {s[2] for s in seen} == {True, False}          # one workgroup and several (the block-order merge)
    assert {s[3] for s in seen} == {True, False}          # one node slot and several (the in-workgroup merge)
    # each single condition of the vector predicate flips it
    assert ops.spna_vector_path(12, [12] * 4, [0] * 4) and not ops.spna_vector_path(15, [16] * 4, [0] * 4)
    assert not ops.spna_vector_path(12, [12, 12, 13, 12], [0] * 4) and not ops.spna_vector_path(12, [12] * 4, [0, 0, 0, 4])
    assert C.KERNEL_CASES["c12_offset"][3] and C.KERNEL_CASES["c12_ld13"][2] == 13
    # the degree mix the kernel cases promise
    ei, batch, B = C.kernel_graph("degrees")
    deg = torch.bincount(ei[1], minlength=batch.numel())
    assert B == 2 and {0, 1, 64, 65, 130} <= set(deg.tolist()) and bool((ei[0] == ei[1]).any())
    assert len(set(map(tuple, ei.t().tolist()))) < ei.shape[1] and not bool((ei[1][1:] >= ei[1][:-1]).all())


def test_kernel_restatements_agree_with_each_other():
    """spna_train_ref (F.batch_norm + autograd) and spna_stats_ref / spna_mean_ref (explicit moments, folded affine) are two routes to the
    same r; in float64 they agree to rounding."""
    x = C.kernel_inputs("c15", torch.float64)
    st = C.spna_stats_ref(x.A, x.B_, x.Q, x.ei, x.gamma, x.beta, x.running_mean, x.running_var)
    r = C.spna_mean_ref(x.A, x.B_, x.Q, x.ei, st.scale, st.shift)
    r2, grads = C.spna_train_ref(x.A, x.B_, x.Q, x.ei, x.gamma, x.beta, x.dr)
    torch.testing.assert_close(r, r2, rtol=1e-12, atol=1e-12)
    assert not bool(r[0].any()) and st.count == x.E and set(grads) == {"dA", "dB", "dQ", "dgamma", "dbeta"}
    with pytest.raises(ValueError, match="more than 1 value"):
        y = C.kernel_inputs("n2_e1")
        C.spna_stats_ref(y.A, y.B_, y.Q, y.ei, y.gamma, y.beta, y.running_mean, y.running_var)
    # GCN: the edge-by-edge operator is the dense one
    ei, batch, _ = C.kernel_graph("degrees")
    v = torch.randn(batch.numel(), 5, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    torch.testing.assert_close(C.gcn_propagate(v, ei), C.gcn_norm_dense(ei, batch.numel(), torch.float64) @ v, rtol=1e-12, atol=1e-12)
    assert json.dumps(sorted(C.KERNEL_CASES))          # (names are plain strings: they are pytest ids)
