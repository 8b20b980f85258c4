"""CPU: GatNet and ARMANet (the last two nets of the LearningFilters table) as far as they go without a GPU — the float64 restatement
(tests/filter_attention_cases.py) against the fixture of the reference's classes, state_dict keys and shapes, the opt-in factories and
the drop-in, the constructor refusals, FilterGraph's ARMA operator against its dense definition, and the host-side validation of the two
attention entry points."""
import json
import os
import subprocess
import sys
import types

import pytest
import torch

import filter_attention_cases as AC
import filter_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))


# ----------------------------------------------------------------------------- the restatement is the reference
@pytest.mark.parametrize("case", AC.NET_CASES)
def test_float64_restatement_agrees_with_the_reference_fixture(case):
    """The fixture records the fp32-vs-float64 error of the classes that made it; the dense restatement in float64 has to sit that close to
    the fp32 fixture (+ 1e-6: two float64 evaluations that sum in different orders)."""
    fx = AC.fixture()
    c = fx.cases[case]
    pre, grads, losses = AC.fixture_ref64(case)
    assert _rel(c["pre"], pre) <= c["err64/pre"] + 1e-6
    assert _rel(c["losses"], losses) <= c["err64/losses"] + 1e-6
    assert set(grads) == set(c["grad"])
    for k, g in grads.items():
        assert _rel(c["grad"][k], g) <= c["err64/grad/" + k] + 1e-6, k
    biases = [k for k in c["sd"] if k.endswith("bias")]
    assert biases and all(float(c["sd"][k].abs().max()) > 0 for k in biases)            # perturbed away from the zero initialisation
    if case == "armanet":
        assert "convs.0.weight" in c["sd"] and "convs.0.weight" not in c["grad"]         # unused at one layer: no gradient
        assert torch.equal(c["sd1"]["convs.0.weight"], c["sd"]["convs.0.weight"])
    if case == "gatnet_eig_abs":
        assert c["feat"].shape[1] == 1 + 2 * fx.N


def test_fixture_marks_all_three_cases_restated():
    fx = AC.fixture()
    assert fx.restated == AC.NET_CASES and tuple(fx.cases) == AC.NET_CASES


@pytest.mark.parametrize("case", AC.NET_CASES)
def test_state_dict_keys_and_shapes_are_the_references(case):
    from signnet_basisnet_amd import filter_baselines as FB
    fx = AC.fixture()
    c = fx.cases[case]
    net = FB.gen_baseline(c["args"]["net"], c["feat"].shape[1], c["args"]["hidden_channels"], c["args"]["num_layers"], extra=True)
    sd = net.state_dict()
    assert list(sd) == list(c["sd"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in c["sd"].items()}
    net.load_state_dict(c["sd"], strict=True)
    for k, v in net.state_dict().items():
        assert v.dtype == torch.float32 and torch.equal(v, c["sd"][k]), k
    assert [k for k, _ in net.named_parameters()] == [k for k in c["sd"] if not k.endswith("lin_r.weight")]


@torch.no_grad()
def test_constructors_initialise_as_pyg_does():
    from signnet_basisnet_amd import filter_baselines as FB
    torch.manual_seed(0)
    conv = FB.GATConv(5, 8, heads=4)
    assert conv.lin_r is conv.lin_l and conv.lin_l.bias is None and tuple(conv.lin_l.weight.shape) == (32, 5)
    assert tuple(conv.att_l.shape) == tuple(conv.att_r.shape) == (1, 4, 8) and float(conv.bias.abs().max()) == 0
    assert float(conv.att_l.abs().max()) <= (6 / 12) ** 0.5 and float(conv.lin_l.weight.abs().max()) <= (6 / 37) ** 0.5
    arma = FB.ARMAConv(5, 8)
    assert [tuple(p.shape) for p in (arma.init_weight, arma.weight, arma.root_weight, arma.bias)] == [(1, 5, 8), (1, 1, 8, 8), (1, 1, 5, 8), (1, 1, 1, 8)]
    assert float(arma.bias.abs().max()) == 0 and float(arma.init_weight.abs().max()) <= (6 / 13) ** 0.5
    net = FB.GatNet(3, hidden_channels=16, num_heads=2, num_layers=3)
    assert [(c.in_channels, c.out_channels, c.heads) for c in net.convs] == [(3, 8, 2), (16, 8, 2), (16, 8, 2)] and net.fc2.in_features == 16


def test_constructor_refusals():
    from signnet_basisnet_amd import filter_baselines as FB
    for kw in (dict(dropout=0.5), dict(concat=False), dict(add_self_loops=False)):
        with pytest.raises(NotImplementedError):
            FB.GATConv(4, 4, heads=2, **kw)
    for kw in (dict(num_stacks=2), dict(num_layers=2), dict(shared_weights=True), dict(dropout=0.1)):
        with pytest.raises(NotImplementedError):
            FB.ARMAConv(4, 4, **kw)
    with pytest.raises(ValueError, match="multiple of num_heads"):
        FB.GatNet(1, hidden_channels=30, num_heads=4)
    FB.GatNet(1, hidden_channels=30, num_heads=4, num_layers=1)                  # one layer: the reference runs there too (fc2 aside)


# ----------------------------------------------------------------------------- factories and drop-in
def test_gen_model_builds_the_two_only_for_all():
    from signnet_basisnet_amd import filter_baselines as FB
    from signnet_basisnet_amd import learning_filters as LF
    eig = types.SimpleNamespace(N=36, pe_dim=0, uniq_mults=[], num_eigenspaces=0)
    for net, cls in FB.EXTRA_NETS.items():
        with pytest.raises(NotImplementedError):
            LF.gen_model(LF.FilterArgs(net=net), eig, "cpu")
        with pytest.raises(NotImplementedError, match="not a polynomial filter"):
            LF.gen_model(LF.FilterArgs(net=net), eig, "cpu", baselines=True)
        with pytest.raises(NotImplementedError):
            FB.gen_baseline(net, 1)
        m = LF.gen_model(LF.FilterArgs(net=net, hidden_channels=16, num_layers=3), eig, "cpu", baselines="all")
        assert type(m) is cls and m.fc2.in_features == 16 and len(m.convs) == 3
    assert set(FB.EXTRA_NETS) == set(FB.NOT_BUILT) == {"GatNet", "ARMANet"} and not set(FB.EXTRA_NETS) & set(FB.NETS)
    for net, cls in FB.NETS.items():                                             # "all" includes what True builds
        assert type(LF.gen_model(LF.FilterArgs(net=net), eig, "cpu", baselines="all")) is cls
    with pytest.raises(ValueError, match="baselines"):
        LF.gen_model(LF.FilterArgs(net="GatNet"), eig, "cpu", baselines="every")


def _report(code, cwd):
    out = subprocess.run([sys.executable, "-c", code], cwd=cwd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("REPORT ")][-1][7:])


def test_dropin_binds_the_two_only_for_all(tmp_path):
    code = ("import json, signnet_basisnet_amd.dropin as D\nD.install('learningfilters'FLAG)\n"
            "from models import ChebNet,BernNet,GcnNet,GatNet,ARMANet,GPRNet,MLP,EqDeepSetsEncoder, Transformer\n"
            "print('REPORT ' + json.dumps({c.__name__: c.__module__ for c in (ChebNet,BernNet,GcnNet,GatNet,ARMANet,GPRNet,MLP,EqDeepSetsEncoder,Transformer)}))")
    plain, flagged, every = (_report(code.replace("FLAG", f), str(tmp_path)) for f in ("", ", baselines=True", ", baselines='all'"))
    hip = "signnet_basisnet_amd.filter_baselines"
    assert every["GatNet"] == every["ARMANet"] == hip
    assert all(r[n] != hip for r in (plain, flagged) for n in ("GatNet", "ARMANet"))
    assert {n: v for n, v in every.items() if n not in ("GatNet", "ARMANet")} == {n: v for n, v in flagged.items() if n not in ("GatNet", "ARMANet")}


def test_dropin_tables_and_the_runner_flag(tmp_path):
    import signnet_basisnet_amd.dropin as D
    from signnet_basisnet_amd.dropin import run
    assert D.ALL_BASELINE_OVERRIDES == {"learningfilters": {"models": "signnet_basisnet_amd.dropin.all_baseline_filter_models"}}
    assert D.AliasFinder("learningfilters", baselines="all").find_spec("models").origin.endswith(".all_baseline_filter_models")
    assert D.AliasFinder("alchemy", baselines="all").table == D.AliasFinder("alchemy", baselines=True).table
    with pytest.raises(ValueError):
        D.AliasFinder("learningfilters", baselines="some")
    try:
        f = D.install("learningfilters", baselines=True)
        assert D.install("learningfilters", baselines="all") is f and f.table["models"].endswith(".all_baseline_filter_models")
        assert D.install("learningfilters", baselines=True) is f and f.table["models"].endswith(".all_baseline_filter_models")
    finally:
        D.uninstall("learningfilters")
    # the runner: --baselines=all reaches install() as "all"
    script = tmp_path / "training.py"
    script.write_text("import models\nprint('BOUND', models.__signnet_hip__, models.GatNet.__module__)\n")
    out = subprocess.run([sys.executable, "-m", "signnet_basisnet_amd.dropin.run", "--baselines=all", str(script)], cwd=str(tmp_path),
                         capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr
    assert "BOUND signnet_basisnet_amd.dropin.all_baseline_filter_models signnet_basisnet_amd.filter_baselines" in out.stdout
    with pytest.raises(SystemExit, match="all"):
        run.main(["--baselines=most", str(script)])


@pytest.mark.parametrize("tree", ["alchemy", "gine_pyg", "learningfilters"])
@pytest.mark.parametrize("flag", [True, "all"])
def test_install_still_extends_a_plain_finder_in_place(tree, flag):
    """install(tree) followed by install(tree, baselines=...) binds what a fresh install with the flag binds, for every tree: the names of
    BASELINE_ALIASES (alchemy's `baseline_gin`, gine_pyg's `core.model`) are in no override table and must not be skipped."""
    import signnet_basisnet_amd.dropin as D
    want = D.AliasFinder(tree, baselines=flag).table
    assert set(D.BASELINE_ALIASES.get(tree, {})) <= set(want)
    try:
        f = D.install(tree)
        assert f.table == D.ALIASES[tree]
        assert D.install(tree, baselines=flag) is f and f.table == want
        assert D.install(tree) is f and f.table == want                          # a later plain install takes nothing away
    finally:
        D.uninstall(tree)


# ----------------------------------------------------------------------------- FilterGraph's ARMA operator
@pytest.mark.parametrize("name", FC.SMALL)
def test_arma_operator_matches_the_dense_definition(name):
    from signnet_basisnet_amd.filter_baselines import FilterGraph
    ei, N = FC.GRAPHS[name]
    g = FilterGraph(torch.as_tensor(ei), N)
    assert g._arma is None                                                       # built on first use
    op, dense = g.arma, AC.dense_arma(ei, N)
    assert g.arma is op
    assert op.rowptr.dtype == torch.int32 and op.col.dtype == torch.int32 and op.w.dtype == torch.float32
    assert int(op.rowptr[0]) == 0 and int(op.rowptr[-1]) == op.nnz == torch.as_tensor(ei).shape[1]      # every input edge, self loops too
    W = FC.operator_dense(op)
    assert float((W - dense).abs().max()) <= 2e-7 * max(float(dense.abs().max()), 1.0)
    assert torch.equal(FC.operator_dense(op.t), W.t()) and op.t.t is op
    if name == "dup_selfloop_shuffled":
        assert float(W[2, 2]) > 0 and float(W[3, 3]) > 0                         # the input self loops are ordinary entries


def test_edge_list_restatement_is_the_dense_one():
    """A self-check of the references, not of the package (it passes without the feature): filter_attention_cases.gat_conv_edges, which
    the GPU kernel test compares against where the dense form is too large, against the dense gat_conv_ref, with the log-sum-exp."""
    gen = torch.Generator().manual_seed(3)
    for name in FC.SMALL:
        ei, N = FC.GRAPHS[name]
        M = AC.dense_counts(ei, N)
        for heads, C in ((1, 1), (3, 5)):
            f, al, ar, b = (torch.randn(*s, generator=gen, dtype=torch.float64) for s in ((N, heads * C), (heads * C,), (heads * C,), (heads * C,)))
            for act in (0, 1):
                out, lse = AC.gat_conv_edges(f, al, ar, b, ei, N, heads, act)
                assert float((out - AC.gat_conv_ref(f, al, ar, b, M, heads, act)).abs().max()) <= 1e-12
                assert float((lse - AC.gat_lse_ref(f, al, ar, M, heads)).abs().max()) <= 1e-12
    # a duplicated edge counts twice, an input self loop not at all
    ei = torch.tensor([[0, 0, 1, 2, 2], [1, 1, 2, 0, 2]])
    assert torch.equal(AC.dense_counts(ei, 3), torch.tensor([[1.0, 0, 1], [2, 1, 0], [0, 1, 1]], dtype=torch.float64))


# ----------------------------------------------------------------------------- entry points: host-side validation, no launch
def test_entry_points_validate_on_the_host():
    from signnet_basisnet_amd import _lib, ops
    L = _lib.lib()
    assert (L.sn_gat_conv_max_heads(), L.sn_gat_conv_max_channels()) == (AC.MAX_HEADS, AC.MAX_C) == ops.gat_conv_limits()
    assert AC.MAX_HEADS >= 16 and AC.MAX_C >= 128
    for C in range(1, AC.MAX_C + 1):
        assert L.sn_gat_conv_group_width(C) == AC.group_width(C) == ops.gat_conv_group_width(C)
    assert L.sn_gat_conv_group_width(0) == 0 and L.sn_gat_conv_group_width(AC.MAX_C + 1) == 0
    assert sorted({AC.group_width(C) for C in range(1, AC.MAX_C + 1)}) == list(AC.GROUP_WIDTH_STEPS)
    for N, H, C in ((1, 1, 1), (36, 4, 8), (1024, 4, 8), (1030, 16, 128), (301, 3, 5), (100000, 8, 16)):
        assert L.sn_gat_conv_bwd_blocks(N, H, C) == AC.bwd_blocks(N, H, C)
    assert L.sn_gat_conv_bwd_blocks(0, 1, 1) == 0 and L.sn_gat_conv_bwd_blocks(4, 17, 1) == 0

    def fwd(N=4, heads=2, C=3, act=1, nnz=0):
        return L.sn_gat_conv_f32(None, None, None, None, N, heads, C, 0.2, act, None, None, nnz, None, None, None)

    def bwd(N=4, heads=2, C=3, act=1, nnz=0):
        return L.sn_gat_conv_bwd_f32(None, None, None, None, None, None, N, heads, C, 0.2, act, None, None, None, None, nnz, None, None, None, None)

    for fn, name in ((fwd, b"sn_gat_conv_f32"), (bwd, b"sn_gat_conv_bwd_f32")):
        for kw, word in ((dict(N=0), b"N"), (dict(heads=0), b"heads"), (dict(C=0), b"C"), (dict(C=-3), b"C"), (dict(act=2), b"act"),
                         (dict(act=-1), b"act"), (dict(nnz=-1), b"nnz"), ({}, b"NULL")):
            assert fn(**kw) == -1, (name, kw)
            assert name in L.sn_last_error() and word in L.sn_last_error(), (kw, L.sn_last_error())
        for kw, word in ((dict(heads=AC.MAX_HEADS + 1), b"heads"), (dict(C=AC.MAX_C + 1), b"C =")):
            assert fn(**kw) == -3, (name, kw)                                    # SN_ERR_UNSUPPORTED, before the pointers are looked at
            assert name in L.sn_last_error() and word in L.sn_last_error() and b"limit" in L.sn_last_error()


def test_wrappers_validate_before_a_launch_and_run_on_the_gpu_only():
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import filter_baselines as FB
    from signnet_basisnet_amd import ops
    ei = torch.tensor([[0, 1], [1, 0]])
    g = FB.FilterGraph(ei, 2)
    v = torch.zeros(6)
    for heads, width in ((AC.MAX_HEADS + 1, AC.MAX_HEADS + 1), (1, AC.MAX_C + 1)):
        with pytest.raises(ValueError, match="limits"):
            ops.gat_conv(torch.zeros(2, width), torch.zeros(width), torch.zeros(width), None, g.lap, heads)
        with pytest.raises(ValueError, match="limits"):
            ops.gat_conv_bwd(torch.zeros(2, width), torch.zeros(width), torch.zeros(width), torch.zeros(2, width), torch.zeros(2, heads),
                             torch.zeros(2, width), g.lap, heads)
    with pytest.raises(ValueError, match="act"):
        ops.gat_conv(torch.zeros(2, 6), v, v, None, g.lap, 2, act="relu")
    with pytest.raises(ValueError, match="heads"):
        ops.gat_conv(torch.zeros(2, 6), v, v, None, g.lap, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gat_conv(torch.zeros(2, 6), v, v, None, g.lap, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gat_conv_bwd(torch.zeros(2, 6), v, v, torch.zeros(2, 6), torch.zeros(2, 2), torch.zeros(2, 6), g.lap, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        AG.gat_conv(torch.zeros(2, 6), v, v, v, g, 2, "elu")
    for net in (FB.GatNet(1), FB.ARMANet(1)):
        with pytest.raises(RuntimeError, match="GPU only"):
            net(torch.zeros(2, 1), ei)
