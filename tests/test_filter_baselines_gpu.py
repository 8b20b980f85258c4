"""-m gpu: the LearningFilters spectral baselines on the device — the polynomial-filter kernels (sn_poly_basis_f32 / sn_poly_combine_f32,
both recurrences) against float64 on every graph shape and slice width, their autograd Functions on non-symmetric graphs, the four
networks against the reference's fixture through the float64 restatement (tests/filter_cases.py), the captured epoch, the 'abs_val' /
'sign_flip' features, and BernNet once at the reference's full size (32 x 32 grid).

Tolerance (filter_cases.bound): 1e-5 of the output's scale against float64; where the fixture's recorded fp32-vs-float64 error of the
reference's own evaluation is larger than 1e-5, 4 x that recorded error."""
import copy
import math

import numpy as np
import pytest
import torch

import filter_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS, ORDERS = (1, 3, 32, 33, 70), (1, 3, 10)


def _graph(name):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.filter_baselines import FilterGraph
    if name == "ring_capacity":
        ei, N = FC.ring(ops.poly_filter_max_nodes(10))
    elif name.startswith("ring") and name not in FC.GRAPHS:
        ei, N = FC.ring(int(name[4:]))
    else:
        ei, N = FC.GRAPHS[name]
    return ei, N, FilterGraph(torch.as_tensor(ei).to(DEV), N)


def _rel(got, want):
    want = want.double()
    return float((got.detach().cpu().double() - want).abs().max() / want.abs().max().clamp_min(1e-300))


# (operator kind, diag_add, scale) per recurrence: L = I - A and gcn_norm's A for the monomials, ChebConv's L^ = -A for Chebyshev
SETTINGS = {"monomial": (("lap", 1.0, -1.0), ("gcn", 0.0, 1.0)), "chebyshev": (("lap", 0.0, -1.0),)}
KERNEL_GRAPHS = ("single", "path5_isolated", "directed_cycle_chord", "dup_selfloop_shuffled", "grid6", "ring1030", "ring3000", "ring_capacity")


@pytest.mark.parametrize("mode", ["monomial", "chebyshev"])
@pytest.mark.parametrize("name", KERNEL_GRAPHS)
def test_kernels_against_float64(name, mode):
    """Both entry points; twice, bitwise equal.  Graphs of up to 2048 nodes (the 4-channel slices) run every width with every order, on the
    operator and its transpose.  ring3000 (2-channel slices) and ring_capacity (sn_poly_filter_max_nodes nodes, 1-channel slices) are
    symmetric and run six (width, order) pairs that use every width and every order at least once."""
    from signnet_basisnet_amd import ops
    ei, N, g = _graph(name)
    gen = torch.Generator().manual_seed(N)
    worst = 0.0
    # (the reduced list on the large rings keeps the float64 side of the test quick)
    shapes = [(d, K) for d in WIDTHS for K in ORDERS] if N <= 2048 else [(1, 1), (1, 10), (3, 1), (32, 3), (33, 10), (70, 10)]
    for kind, diag_add, scale in SETTINGS[mode]:
        for transpose in ((False, True) if N <= 2048 else (False,)):
            op = getattr(g, kind)
            op = op.t if transpose else op
            W = FC.sparse_operator(ei, N, kind, transpose)
            for d, K in shapes:
                x = torch.randn(N, d, generator=gen)
                st = torch.randn(K + 1, N, d, generator=gen)
                c = torch.randn(K + 1, generator=gen)
                xd, sd_, cd = x.to(DEV), st.to(DEV), c.to(DEV)
                # basis: the stack, and the dots against a reversed stack
                B, dots = ops.poly_basis(xd, op, K, mode, diag_add, scale, g=sd_, g_reverse=True)
                B2, dots2 = ops.poly_basis(xd, op, K, mode, diag_add, scale, g=sd_, g_reverse=True)
                assert torch.equal(B, B2) and torch.equal(dots, dots2)
                # the float64 stack is the same doubles unrounded: the fp32 stack is its rounding, and reading fp32 values back as a
                # float64 stack changes nothing
                B64, dots64 = ops.poly_basis(xd, op, K, mode, diag_add, scale, g=sd_.double(), g_reverse=True, stack_dtype=torch.float64)
                assert B64.dtype == torch.float64 and torch.equal(B64.float(), B) and torch.equal(dots64, dots)
                want = FC.basis_apply(W, diag_add, scale, x.double(), K, mode)
                wdots = (want * st.double().flip(0)).sum((1, 2))
                e1 = _rel(B, want)
                e2 = _rel(dots, wdots)
                # basis without the stack, against one shared block
                only = ops.poly_basis(xd, op, K, mode, diag_add, scale, want_stack=False, g=sd_[0].contiguous())
                wo = (want * st[0].double()).sum((1, 2))
                e3 = _rel(only, wo)
                # combine: a reversed stack with coefficients; one shared block without
                y = ops.poly_combine(sd_, op, K, mode, diag_add, scale, cd, reverse=True)
                assert torch.equal(y, ops.poly_combine(sd_, op, K, mode, diag_add, scale, cd, reverse=True))
                assert torch.equal(y, ops.poly_combine(sd_.double(), op, K, mode, diag_add, scale, cd, reverse=True))
                e4 = _rel(y, FC.combine_apply(W, diag_add, scale, st.double(), c.double(), K, mode, reverse=True))
                e5 = _rel(ops.poly_combine(xd, op, K, mode, diag_add, scale), FC.combine_apply(W, diag_add, scale, x.double(), None, K, mode))
                errs = (e1, e2, e3, e4, e5)
                worst = max(worst, *errs)
                assert max(errs) <= FC.bound(), (name, mode, kind, transpose, d, K, errs)
    print(f"{name} {mode}: worst relative error {worst:.2e}")


def test_one_node_above_the_capacity_raises_without_a_launch():
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.filter_baselines import BernNet, FilterGraph
    cap = ops.poly_filter_max_nodes(10)
    ei, N = FC.ring(cap + 1)
    g = FilterGraph(torch.as_tensor(ei).to(DEV), N)
    x = torch.zeros(N, 2, device=DEV)
    with pytest.raises(ValueError, match="capacity"):
        ops.poly_basis(x, g.lap, 10, "monomial", 1.0, 1.0)
    with pytest.raises(ValueError, match="capacity"):
        ops.poly_combine(x, g.lap, 10, "monomial", 1.0, -1.0)
    with pytest.raises(ValueError, match="capacity"):
        BernNet(2).to(DEV)(x, g)


# ----------------------------------------------------------------------------- the autograd Functions on non-symmetric graphs
@pytest.mark.parametrize("name", ["directed_cycle_chord", "dup_selfloop_shuffled", "path5_isolated"])
def test_function_gradients_against_float64_autograd(name):
    from signnet_basisnet_amd import autograd as AG
    ei, N, g = _graph(name)
    A, G = FC.dense_lap_adj(ei, N), FC.dense_gcn(ei, N)                        # float64, from the definitions
    gen = torch.Generator().manual_seed(7)
    d, K = 5, 10
    x = torch.randn(N, d, generator=gen)
    cot = torch.randn(N, d, generator=gen)
    c = torch.randn(K + 1, generator=gen)

    def check(hip_fn, ref_fn, tensors, what):
        """ref_fn — the reference's formulas on dense matrices — runs in float64 and in float32; its own fp32 error sets the bound."""
        hs = [t.clone().to(DEV).requires_grad_(True) for t in tensors]
        r64 = [t.double().requires_grad_(True) for t in tensors]
        r32 = [t.clone().requires_grad_(True) for t in tensors]
        out, ref, ref32 = hip_fn(*hs), ref_fn(torch.float64, *r64), ref_fn(torch.float32, *r32)
        w = out.shape[1]
        out.backward(cot[:, :w].to(DEV).contiguous())
        ref.backward(cot[:, :w].double())
        ref32.backward(cot[:, :w])
        pairs = [(out, ref.detach(), ref32.detach(), "output")] + [(h.grad, r.grad, q.grad, f"grad {i}") for i, (h, r, q) in enumerate(zip(hs, r64, r32))]
        for got, want, want32, n in pairs:
            e, rec = _rel(got, want), _rel(want32, want)
            print(f"{name} {what} {n}: {e:.2e} (the reference's formulas in fp32: {rec:.2e}, bound {FC.bound(rec):.2e})")
            assert e <= FC.bound(rec), (what, n, e, rec)
        hs2 = [t.clone().to(DEV).requires_grad_(True) for t in tensors]
        hip_fn(*hs2).backward(cot[:, :w].to(DEV).contiguous())
        assert all(torch.equal(a.grad, b.grad) for a, b in zip(hs, hs2)), what + ": not reproducible"

    def gpr_ref(dt, x_, c_):                         # models.py:175-184
        h, hidden = x_, x_ * c_[0]
        for k in range(K):
            h = G.to(dt) @ h
            hidden = hidden + c_[k + 1] * h
        return hidden

    def cheb_ref(dt, x_, b_, *ws):                   # ChebConv's documented recurrence
        T0, Lh = x_, -A.to(dt)
        o = T0 @ ws[0].t()
        T1 = Lh @ x_
        o = o + T1 @ ws[1].t()
        for w_ in ws[2:]:
            T2 = 2.0 * (Lh @ T1) - T0
            o, T0, T1 = o + T2 @ w_.t(), T1, T2
        return torch.relu(o + b_)

    check(lambda x_, c_: AG.poly_combine_shared(x_, c_, g.gcn, K, "monomial", 0.0, 1.0), gpr_ref, (x, c), "GPR propagation")
    cb = c.abs() * torch.tensor([math.comb(K, i) / 2.0 ** K for i in range(K + 1)])
    check(lambda x_, c_: AG.bern_prop(x_, c_, c_.detach().flip(0), g.lap, K),
          lambda dt, x_, c_: FC.bern_prop_ref(x_, A.to(dt), c_, K), (x, cb), "Bernstein propagation")
    Ws = [0.3 * torch.randn(4, d, generator=gen) for _ in range(3)]
    b = torch.randn(4, generator=gen)
    check(lambda x_, b_, *ws: AG.cheb_conv(x_, list(ws), b_, g.lap, 0.0, -1.0, relu=True), cheb_ref, (x, b, *Ws), "ChebConv")
    Wio = 0.3 * torch.randn(d, 4, generator=gen)
    check(lambda x_, w_, b_: AG.linear_io(x_, w_, b_, relu=True), lambda dt, x_, w_, b_: torch.relu(x_ @ w_ + b_), (x, Wio, b), "linear_io")


# ----------------------------------------------------------------------------- the networks against the fixture
def _setup(case):
    from signnet_basisnet_amd import filter_baselines as FB
    from signnet_basisnet_amd import learning_filters as LF
    fx = FC.fixture()
    c = fx.cases[case]
    args = LF.FilterArgs(**c["args"])
    eig = LF.GridEigen(fx.inp["eigvals"].to(DEV), fx.inp["eigvecs"].to(DEV), args)
    model = LF.gen_model(args, eig, DEV, baselines=True)
    model.load_state_dict(c["sd"])
    graph = FB.FilterGraph(fx.edge_index.to(DEV), fx.N)
    x, y, m = fx.inp["x"][:, 0:1].contiguous().to(DEV), fx.inp["y"][:, 0:1].contiguous().to(DEV), fx.inp["m"].to(DEV)
    return fx, c, args, eig, model, graph, x, y, m


@pytest.mark.parametrize("case", FC.NET_CASES)
def test_network_prediction_gradients_and_loss_curve(case):
    """Prediction, every first-step gradient and the four-step loss curve against the float64 restatement, bound per quantity from the
    fixture's recorded error of the reference's own fp32 evaluation (filter_cases.bound).

    Every figure is printed (-s).  BernConv hands its stacks from one launch to the next in float64: `(2I - L)^k x` is about 2^k large
    and the second launch takes it through `L^i` and the 2^-K weights, which amplifies an fp32 rounding of the stored stack (with fp32
    stacks `bernnet_eig_abs` reaches 1.1e-5 on one gradient; with float64 stacks every case is within 1.5e-6)."""
    from signnet_basisnet_amd import learning_filters as LF
    from signnet_basisnet_amd.optim import Adam
    fx, c, args, eig, model, graph, x, y, m = _setup(case)
    pre64, grads64, losses64 = FC.fixture_ref64(case)
    model.train()
    feat = LF.get_lap_feat(args.use_eig, eig, x, args.lap_method, model)
    assert torch.equal(feat.cpu(), c["feat"])
    pre = model(feat, graph)
    with torch.no_grad():
        model.eval()
        assert torch.equal(model(feat, fx.edge_index.to(DEV)), pre)            # eval mode, and an edge tensor in place of the FilterGraph
        model.train()
    e = _rel(pre, pre64)
    print(f"{case}: prediction {e:.2e} (bound {FC.bound(c['err64/pre']):.2e})")
    assert e <= FC.bound(c["err64/pre"])
    LF.masked_square_loss(pre, y, m).backward()
    for k, p in model.named_parameters():
        e = _rel(p.grad, grads64[k])
        print(f"{case}: grad {k} {e:.2e} (bound {FC.bound(c['err64/grad/' + k]):.2e})")
        assert e <= FC.bound(c["err64/grad/" + k]), k
    opt = Adam(model.parameters(), lr=args.lr)
    losses = [LF.train_step(model, opt, args, eig, x, y, m, graph)[0].item() for _ in range(4)]
    e = _rel(torch.tensor(losses, dtype=torch.float64), losses64)
    print(f"{case}: losses {losses} {e:.2e} (bound {FC.bound(c['err64/losses']):.2e})")
    assert e <= FC.bound(c["err64/losses"])


@pytest.mark.parametrize("case", ["bernnet", "gprnet", "chebnet", "gcnnet"])
def test_graphed_epoch_with_a_graph_replays_the_eager_step_bit_for_bit(case):
    from signnet_basisnet_amd import learning_filters as LF
    from signnet_basisnet_amd.optim import FlatAdam
    fx, c, args, eig, model, graph, x, y, m = _setup(case)
    model_g = copy.deepcopy(model)
    opt_e, opt_g = FlatAdam(model.parameters(), lr=args.lr), FlatAdam(model_g.parameters(), lr=args.lr)
    ge = LF.GraphedEpoch(model_g, opt_g, args, eig, x, y, m, graph=graph)
    le, lg = [], []
    for _ in range(4):
        le.append(LF.train_step(model, opt_e, args, eig, x, y, m, graph)[0].item())
        lg.append(ge.step()[0].item())
    assert le == lg, (le, lg)
    for (k1, p1), (k2, p2) in zip(model.named_parameters(), model_g.named_parameters()):
        assert torch.equal(p1, p2), k1


def test_lap_feat_abs_val_and_sign_flip_are_exact():
    from signnet_basisnet_amd import learning_filters as LF
    from signnet_basisnet_amd.optim import FlatAdam
    fx = FC.fixture()
    x = fx.inp["x"][:, 0:1].contiguous().to(DEV)
    for method in ("abs_val", "sign_flip"):
        args = LF.FilterArgs(net="MLP", use_eig=True, lap_method=method)
        eig = LF.GridEigen(fx.inp["eigvals"].to(DEV), fx.inp["eigvecs"].to(DEV), args)
        feat = LF.get_lap_feat(True, eig, x, method, None, u=fx.lapfeat["u"])
        assert torch.equal(feat.cpu(), fx.lapfeat[method]), method
    torch.manual_seed(5)
    drawn = LF.get_lap_feat(True, eig, x, "sign_flip", None)                    # no u: torch.rand(k) on the host, as the reference draws
    torch.manual_seed(5)
    assert torch.equal(drawn, LF.get_lap_feat(True, eig, x, "sign_flip", None, u=torch.rand(eig.eigvecs.shape[1])))
    with pytest.raises(NotImplementedError, match="sign_flip"):
        LF.GraphedEpoch(torch.nn.Linear(1, 1), FlatAdam([torch.nn.Parameter(torch.zeros(1, device=DEV))], lr=0.1), args, eig, x, x, x)


# ----------------------------------------------------------------------------- full size, once
def test_bernnet_on_the_32x32_grid():
    """The reference's size (N = 1024, hidden 32, 2 layers, K = 10): eval against the float64 restatement (65 dense propagations per layer),
    and two optimisation steps lower the loss."""
    from signnet_basisnet_amd import filter_baselines as FB
    from signnet_basisnet_amd import learning_filters as LF
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.optim import Adam
    ei, N = synth.grid_graph(32)
    torch.manual_seed(0)
    model = FB.BernNet(1).to(DEV)
    with torch.no_grad():
        model.coe.copy_(1 + 0.3 * torch.randn(11))
    gen = torch.Generator().manual_seed(1)
    x, y = torch.randn(N, 1, generator=gen), torch.randn(N, 1, generator=gen)
    m = torch.ones(N, 1)
    graph = FB.FilterGraph(torch.as_tensor(np.asarray(ei)).to(DEV), N)
    model.eval()
    with torch.no_grad():
        pre = model(x.to(DEV), graph)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    want64 = FC.net_ref("BernNet", sd, x.double(), ei, N)
    want32 = FC.net_ref("BernNet", sd, x, ei, N)
    rec = _rel(want32, want64)                       # the same formulas in fp32: the recorded error of the reference's own evaluation
    e = _rel(pre, want64)
    print(f"32x32 BernNet: {e:.2e}; the 65-propagation form in fp32: {rec:.2e}; bound {FC.bound(rec):.2e}")
    assert e <= FC.bound(rec)
    args = LF.FilterArgs(net="BernNet")
    eig = LF.GridEigen(torch.zeros(N, device=DEV), torch.zeros(N, N, device=DEV), args)
    opt = Adam(model.parameters(), lr=args.lr)
    losses = [LF.train_step(model, opt, args, eig, x.to(DEV), y.to(DEV), m.to(DEV), graph)[0].item() for _ in range(3)]
    assert losses[2] < losses[1] < losses[0], losses
