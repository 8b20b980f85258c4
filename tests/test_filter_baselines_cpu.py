"""CPU: the LearningFilters spectral baselines (BernNet, GPRNet, ChebNet, GcnNet) as far as they go without a GPU — the float64
restatement (tests/filter_cases.py, BernConv in its original 65-propagation form) against the reference's own fixture, state_dict keys
and shapes, FilterGraph's operators against the dense definitions, the factories and the drop-in, host-side validation of the two new
entry points, and the index-exact emulation of the kernel's schedule (tests/poly_filter_emulation.py) against dense float64."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import filter_cases as FC
import poly_filter_emulation as EMU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the restatement is the reference
@pytest.mark.parametrize("case", FC.NET_CASES)
def test_float64_restatement_agrees_with_the_reference_fixture(case):
    """The fixture records the reference's own fp32-vs-float64 error; the restatement in float64 has to sit that close to the fp32 fixture
    (+ 1e-6: the two float64 evaluations sum in different orders and the Horner-free form differs in rounding, never in value)."""
    fx = FC.fixture()
    c = fx.cases[case]
    pre, grads, losses = FC.fixture_ref64(case)

    def rel(a, b):
        return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))
    assert rel(c["pre"], pre) <= c["err64/pre"] + 1e-6
    assert rel(c["losses"], losses) <= c["err64/losses"] + 1e-6
    assert set(grads) == set(c["grad"])
    for k, g in grads.items():
        assert rel(c["grad"][k], g) <= c["err64/grad/" + k] + 1e-6, k
    assert float(c["sd"]["coe"][3]) < 0 if "coe" in c["sd"] else True          # one Bernstein coefficient sits behind the ReLU


@pytest.mark.parametrize("case", FC.NET_CASES)
def test_state_dict_keys_and_shapes_are_the_references(case):
    from signnet_basisnet_amd import filter_baselines as FB
    fx = FC.fixture()
    c = fx.cases[case]
    net = FB.gen_baseline(c["args"]["net"], c["feat"].shape[1], c["args"]["hidden_channels"], c["args"]["num_layers"])
    sd = net.state_dict()
    assert list(sd) == list(c["sd"])
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in c["sd"].items()}
    net.load_state_dict(c["sd"], strict=True)                                    # prop1.temp: float64 in the fixture, float32 here
    assert all(v.dtype == torch.float32 for v in net.state_dict().values())
    for k, v in net.state_dict().items():
        assert torch.equal(v, c["sd"][k].float()), k


def test_fixture_marks_the_restated_layers():
    assert FC.fixture().restated == ("chebnet", "gcnnet")


def test_constructors_keep_the_references_quirks():
    from signnet_basisnet_amd import filter_baselines as FB
    assert torch.equal(FB.BernNet(1).coe.detach(), torch.ones(11))
    assert all(float(c.bias.detach().abs().max()) == 0 for c in FB.BernNet(3).convs)
    np.random.seed(7)
    t = FB.GPRNet(1).prop1.temp.detach()
    np.random.seed(7)
    bound = np.sqrt(3 / 11)
    want = np.random.uniform(-bound, bound, 11)
    want = want / np.sum(np.abs(want))
    assert t.dtype == torch.float32 and torch.equal(t, torch.tensor(want).float())
    assert len(FB.ChebNet(1).convs[0].lins) == 3 and FB.ChebNet(1).convs[0].lins[0].bias is None


# ----------------------------------------------------------------------------- FilterGraph
@pytest.mark.parametrize("name", FC.SMALL)
def test_filter_graph_operators_match_the_dense_definitions(name):
    from signnet_basisnet_amd.filter_baselines import FilterGraph
    ei, N = FC.GRAPHS[name]
    g = FilterGraph(torch.as_tensor(ei), N)
    for op, dense in ((g.lap, FC.dense_lap_adj(ei, N)), (g.gcn, FC.dense_gcn(ei, N))):
        assert op.rowptr.dtype == torch.int32 and op.col.dtype == torch.int32 and op.w.dtype == torch.float32
        assert int(op.rowptr[0]) == 0 and int(op.rowptr[-1]) == op.nnz and bool((op.rowptr[1:] >= op.rowptr[:-1]).all())
        assert op.nnz == 0 or (0 <= int(op.col.min()) and int(op.col.max()) < N)
        W = FC.operator_dense(op)
        assert float((W - dense).abs().max()) <= 2e-7 * max(float(dense.abs().max()), 1.0)          # fp32 weights vs float64: two roundings
        assert torch.equal(FC.operator_dense(op.t), W.t()) and op.t.t is op
    if name == "directed_cycle_chord":
        W = FC.operator_dense(g.lap)
        assert not torch.equal(W, W.t())                                         # the backward really needs the transposed operator


def test_filter_graph_refuses_bad_edges_and_caches_by_tensor():
    from signnet_basisnet_amd import filter_baselines as FB
    with pytest.raises(ValueError):
        FB.FilterGraph(torch.tensor([[0, 4], [1, 0]]), 4)
    with pytest.raises(ValueError):
        FB.FilterGraph(torch.zeros(2, 3), 4)
    ei = torch.tensor([[0, 1], [1, 0]])
    g = FB.as_filter_graph(ei, 2)
    assert FB.as_filter_graph(ei, 2) is g and FB.as_filter_graph(g, 2) is g
    ei[0, 0] = 1                                                                 # an in-place edit bumps the version: a new graph
    assert FB.as_filter_graph(ei, 2) is not g
    with pytest.raises(ValueError):
        FB.as_filter_graph(g, 3)


# ----------------------------------------------------------------------------- factories and drop-in
def test_gen_model_default_still_raises_and_the_flag_builds():
    import types
    from signnet_basisnet_amd import filter_baselines as FB
    from signnet_basisnet_amd import learning_filters as LF
    eig = types.SimpleNamespace(N=36, pe_dim=0, uniq_mults=[], num_eigenspaces=0)
    for net in LF.GRAPH_CONV_BASELINES:
        with pytest.raises(NotImplementedError):
            LF.gen_model(LF.FilterArgs(net=net), eig, "cpu")
    for net, cls in FB.NETS.items():
        m = LF.gen_model(LF.FilterArgs(net=net, hidden_channels=16, num_layers=3), eig, "cpu", baselines=True)
        assert type(m) is cls and m.fc2.in_features == 16
        assert len(m.lins if net == "GPRNet" else m.convs) == 3
    for net in ("GatNet", "ARMANet"):
        with pytest.raises(NotImplementedError, match="not a polynomial filter"):
            LF.gen_model(LF.FilterArgs(net=net), eig, "cpu", baselines=True)


def test_models_run_on_the_gpu_only():
    from signnet_basisnet_amd import filter_baselines as FB
    with pytest.raises(RuntimeError, match="GPU only"):
        FB.GcnNet(1)(torch.zeros(2, 1), torch.tensor([[0, 1], [1, 0]]))


def _report(code, cwd):
    out = subprocess.run([sys.executable, "-c", code], cwd=cwd, capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("REPORT ")][-1][7:])


def test_dropin_binds_the_four_baselines_only_with_the_flag(tmp_path):
    code = ("import json, signnet_basisnet_amd.dropin as D\nD.install('learningfilters'FLAG)\n"
            "from models import ChebNet,BernNet,GcnNet,GatNet,ARMANet,GPRNet,MLP,EqDeepSetsEncoder, Transformer\n"
            "print('REPORT ' + json.dumps({c.__name__: c.__module__ for c in (ChebNet,BernNet,GcnNet,GatNet,ARMANet,GPRNet,MLP,EqDeepSetsEncoder,Transformer)}))")
    plain = _report(code.replace("FLAG", ""), str(tmp_path))
    flagged = _report(code.replace("FLAG", ", baselines=True"), str(tmp_path))
    four = ("ChebNet", "BernNet", "GcnNet", "GPRNet")
    assert all(flagged[n] == "signnet_basisnet_amd.filter_baselines" for n in four)
    assert all(plain[n] != "signnet_basisnet_amd.filter_baselines" for n in four)
    rest = [n for n in plain if n not in four]
    assert {n: flagged[n] for n in rest} == {n: plain[n] for n in rest}           # GatNet, ARMANet and the base models: exactly as before


def test_dropin_extends_an_installed_finder_and_keeps_the_tables_apart():
    import signnet_basisnet_amd.dropin as D
    assert D.BASELINE_OVERRIDES == {"learningfilters": {"models": "signnet_basisnet_amd.dropin.baseline_filter_models"}}
    assert "learningfilters" not in D.BASELINE_ALIASES and set(D.BASELINE_OVERRIDES["learningfilters"]) <= set(D.ALIASES["learningfilters"])
    assert D.AliasFinder("learningfilters").find_spec("models").origin == D.ALIASES["learningfilters"]["models"]
    assert D.AliasFinder("learningfilters", baselines=True).find_spec("models").origin.endswith("baseline_filter_models")
    try:
        f = D.install("learningfilters")
        assert f.table["models"] == D.ALIASES["learningfilters"]["models"]
        assert D.install("learningfilters", baselines=True) is f and f.table["models"].endswith("baseline_filter_models")
    finally:
        D.uninstall("learningfilters")


# ----------------------------------------------------------------------------- entry points: host-side validation, no launch
def test_entry_points_validate_on_the_host():
    from signnet_basisnet_amd import _lib, ops
    L = _lib.lib()
    cap = L.sn_poly_filter_max_nodes(10, 0)
    assert cap >= 4096 and cap == EMU.MAX_NODES == ops.poly_filter_max_nodes(10) == ops.poly_filter_max_nodes(3, "chebyshev")
    assert L.sn_poly_filter_max_nodes(-1, 0) == 0 and L.sn_poly_filter_max_nodes(3, 2) == 0
    for N, d in ((1, 1), (36, 33), (2048, 70), (2049, 70), (4096, 3), (4097, 3), (8192, 32)):
        assert L.sn_poly_filter_launch_shape(N, d, None, None) == EMU.launch_shape(N, d)[0]
    assert L.sn_poly_filter_launch_shape(8193, 4, None, None) == 0
    big = [None, cap + 1, 4, 3, 0, None, None, None, 0, 1.0, 1.0, None, 0, 0, 0, None, 0, 0, 0, 0, None, None]
    assert L.sn_poly_basis_f32(*big) == -1 and b"capacity" in L.sn_last_error()
    assert L.sn_poly_combine_f32(None, 0, 4, 0, 0, cap + 1, 4, 3, 0, None, None, None, 0, 1.0, 1.0, None, None, None) == -1
    assert b"sn_poly_combine_f32" in L.sn_last_error() and b"capacity" in L.sn_last_error()
    assert L.sn_poly_basis_f32(None, 4, 4, 3, 7, None, None, None, 0, 1.0, 1.0, None, 0, 0, 0, None, 0, 0, 0, 0, None, None) == -1
    assert b"mode" in L.sn_last_error()


def test_one_node_above_the_capacity_raises_before_anything_else():
    """ValueError from the host wrapper: raised from the node count alone, before the tensors are looked at (no launch, no GPU needed)."""
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.filter_baselines import FilterGraph
    cap = ops.poly_filter_max_nodes(10)
    ei, N = FC.ring(cap + 1)
    g = FilterGraph(torch.as_tensor(ei), N)
    x = torch.zeros(N, 3)
    with pytest.raises(ValueError, match="capacity"):
        ops.poly_basis(x, g.lap, 10, "monomial", 1.0, -1.0)
    with pytest.raises(ValueError, match="capacity"):
        ops.poly_combine(x, g.gcn, 3, "chebyshev", 0.0, 1.0)


# ----------------------------------------------------------------------------- the kernel's schedule, emulated
def _emu_case(name, d, K, mode, seed, transpose=False):
    from signnet_basisnet_amd.filter_baselines import FilterGraph
    ei, N = FC.GRAPHS[name] if name in FC.GRAPHS else FC.ring(int(name[4:]))
    g = FilterGraph(torch.as_tensor(ei), N)
    op = g.lap.t if transpose else g.lap
    S = FC.dense_lap_adj(ei, N)
    S = torch.eye(N, dtype=torch.float64) - (S.t() if transpose else S)         # L (or L^T): diag_add 1, scale -1
    rng = np.random.RandomState(seed)
    return op, S, N, rng


@pytest.mark.parametrize("name,d,K,mode,transpose", [
    ("single", 1, 3, "monomial", False), ("path5_isolated", 3, 3, "chebyshev", False), ("directed_cycle_chord", 5, 10, "monomial", True),
    ("dup_selfloop_shuffled", 6, 3, "chebyshev", True), ("grid6", 33, 10, "monomial", False), ("grid6", 7, 1, "chebyshev", False),
    ("ring1030", 5, 3, "monomial", False), ("ring2100", 3, 1, "chebyshev", False), ("ring4200", 2, 1, "monomial", False)])
def test_emulated_schedule_matches_dense_float64(name, d, K, mode, transpose):
    op, S, N, rng = _emu_case(name, d, K, mode, 11, transpose)
    cheb = mode == "chebyshev"
    rp, col, w = op.rowptr.numpy(), op.col.numpy(), op.w.numpy().astype(np.float64)
    Sd = torch.eye(N, dtype=torch.float64) - FC.operator_dense(op)              # the operator exactly as stored (fp32 weights)
    x = rng.randn(N, d)
    gst = rng.randn(K + 1, N, d)
    # basis into a [N, K+1, d] layout (k stride d, node stride (K+1) d: the C strides are general) with dots against a reversed stack
    B = np.full(N * (K + 1) * d, np.nan)
    part = EMU.basis(x, rp, col, w, 1.0, -1.0, K, cheb, B=B, b_sk=d, b_ld=(K + 1) * d, g=gst.reshape(-1), g_sk=N * d, g_ld=d, g_reverse=True)
    want = FC.basis_ref(Sd, torch.from_numpy(x), K, mode)
    got = torch.from_numpy(B.reshape(N, K + 1, d)).permute(1, 0, 2)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * scale
    dots = torch.from_numpy(part.sum(0))
    wd = (want * torch.from_numpy(gst).flip(0)).sum((1, 2))
    assert part.shape == (EMU.launch_shape(N, d)[0], K + 1) and float((dots - wd).abs().max()) <= 1e-11 * max(float(wd.abs().max()), 1.0)
    # combine over the standard stack, reversed, with coefficients; and the shared-x form without
    c = rng.randn(K + 1)
    y = EMU.combine(gst.reshape(-1), N * d, d, True, N, d, rp, col, w, 1.0, -1.0, K, cheb, c=c)
    wy = FC.combine_ref(Sd, torch.from_numpy(gst), torch.from_numpy(c), K, mode, reverse=True)
    assert float((torch.from_numpy(y) - wy).abs().max()) <= 1e-12 * max(float(wy.abs().max()), 1.0) * 2 ** K
    y = EMU.combine(np.ascontiguousarray(x).reshape(-1), 0, d, False, N, d, rp, col, w, 1.0, -1.0, K, cheb)
    wy = FC.combine_ref(Sd, torch.from_numpy(x), None, K, mode)
    assert float((torch.from_numpy(y) - wy).abs().max()) <= 1e-12 * max(float(wy.abs().max()), 1.0) * 2 ** K
    # and the stored operator is the definition's, to fp32 rounding of its weights
    assert float((Sd - S).abs().max()) <= 2e-7


def test_emulated_launch_shapes_are_the_librarys():
    """The emulation's grid, block and LDS size against what the library launches (sn_poly_filter_launch_shape), at and around every
    slice-width boundary; the LDS stays inside the 160 KiB a workgroup can have."""
    import ctypes as C
    from signnet_basisnet_amd import _lib
    L = _lib.lib()
    for N in (1, 15, 16, 17, 36, 255, 256, 257, 1030, 2048, 2049, 4096, 4097, 8192):
        for d in (1, 3, 32, 33, 70):
            nt, lds = C.c_int(0), C.c_int64(0)
            blocks = L.sn_poly_filter_launch_shape(N, d, C.byref(nt), C.byref(lds))
            assert (blocks, nt.value, lds.value) == EMU.launch_shape(N, d)[:2] + (8 * EMU.launch_shape(N, d)[2],), (N, d)
            assert lds.value <= 160 * 1024 and 64 <= nt.value <= 1024 and nt.value % 64 == 0
    assert EMU.launch_shape(2048, 32)[0] == 8 and EMU.launch_shape(2049, 32)[0] == 16 and EMU.launch_shape(4097, 32)[0] == 32


def test_bernstein_rewrite_is_the_65_propagation_form():
    """out = sum_i c_i L^i (2I - L)^(K - i) x: the two-launch form (basis over M, combine over L with the stack reversed), and its adjoint
    (basis over L^T, dots against the reversed T, combine over M^T with both reversed), in dense float64 against autograd of the original."""
    ei, N = FC.GRAPHS["directed_cycle_chord"]
    A = FC.dense_lap_adj(ei, N)
    I = torch.eye(N, dtype=torch.float64)
    L, M, K = I - A, I + A, 10
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 4, generator=g, dtype=torch.float64, requires_grad=True)
    coe = (1 + 0.5 * torch.randn(K + 1, generator=g, dtype=torch.float64)).requires_grad_(True)
    Wt, b = torch.eye(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    out = FC.bern_conv_ref(x, A, coe, Wt, b, K)
    cot = torch.randn(N, 4, generator=g, dtype=torch.float64)
    dx, dcoe = torch.autograd.grad(out, (x, coe), cot)
    import math
    binom = torch.tensor([math.comb(K, i) / 2.0 ** K for i in range(K + 1)], dtype=torch.float64)
    c = binom * torch.relu(coe.detach())
    T = FC.basis_ref(M, x.detach(), K, "monomial")
    y = FC.combine_ref(L, T, c, K, "monomial", reverse=True)
    assert float((y - out.detach()).abs().max()) <= 1e-12 * float(out.abs().max())
    U = FC.basis_ref(L.t(), cot, K, "monomial")
    dc = (U * T.flip(0)).sum((1, 2))
    assert float((dc * binom * (coe.detach() > 0) - dcoe).abs().max()) <= 1e-12 * float(dcoe.abs().max())
    dx2 = FC.combine_ref(M.t(), U, c.flip(0), K, "monomial", reverse=True)
    assert float((dx2 - dx).abs().max()) <= 1e-12 * float(dx.abs().max())
