"""-m gpu: readout='max' (DESIGN.md §4.6a).

  kernels   sn_segment_max_f32 / sn_segment_max_bwd_f32 through the C ABI over the table of tests/readout_max_cases.py, on 16-byte
            aligned buffers (128-bit loads where C % 4 == 0) and on views at a 4-byte offset (the scalar path), between NaN / sentinel
            guards, against the restatement with torch.equal — max is exact; exact ties, NaN, empty graphs, the adjoint
  nets      the readout_models nets on the reference's fixtures (tests/golden/make_readout_max.py): eval on the one-launch path and on
            the layer path, train value and BatchNorm buffers, every parameter gradient; sum / mean unchanged bit for bit
  captured  DGLBucketedStep.step / step_from, GraphedDGLForward, the full-graph Transformer in bond form
"""
import types

import pytest
import torch

import parity_util as PU
import readout_max_cases as RC
from parity_util import close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SENT_F, SENT_I = float("nan"), -777


# ----------------------------------------------------------------------------- the kernels through the C ABI
def _guarded(n, dtype, offset):
    """(buffer, view of n elements): the view starts `offset` elements behind a 16-byte aligned address, guards on both sides."""
    buf = torch.full((GUARD + offset + n + GUARD,), SENT_F if dtype == torch.float32 else SENT_I, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + offset:GUARD + offset + n]


def _intact(buf, n, offset):
    lo, hi = buf[:GUARD + offset], buf[GUARD + offset + n:]
    if buf.dtype == torch.float32:
        return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
    return bool((lo == SENT_I).all()) and bool((hi == SENT_I).all())


def _call_max(x, sizes, offset, want_arg=True):
    """x [N, C] host float32 -> (out, arg) on the host, through the C ABI; checks the guards and that a second call gives the same bits."""
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    N, C = x.shape
    B = len(sizes)
    xb, xv = _guarded(max(N * C, 1), torch.float32, offset)
    xv[:N * C].copy_(x.reshape(-1))
    gp = RC.graph_ptr(sizes).to(DEV)
    runs = []
    for _ in range(2):
        ob, ov = _guarded(B * C, torch.float32, offset)
        ab, av = _guarded(B * C, torch.int32, offset)
        check(lib().sn_segment_max_f32(ptr(xv), B, C, ptr(gp), ptr(ov), ptr(av) if want_arg else None, stream()), "sn_segment_max_f32")
        torch.cuda.synchronize()
        assert _intact(ob, B * C, offset) and _intact(ab, B * C, offset)
        if not want_arg:
            assert bool((av == SENT_I).all())                               # arg NULL: not written
        runs.append((ov.reshape(B, C).cpu(), av.reshape(B, C).cpu()))
    assert (xv.data_ptr() % 16 == 0) == (offset == 0)
    assert runs[0][0].view(torch.int32).equal(runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1])
    return runs[0]


def _call_bwd(dy, arg, sizes, C, offset):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    N, B = sum(sizes), len(sizes)
    gp = RC.graph_ptr(sizes).to(DEV)
    dyb, dyv = _guarded(B * C, torch.float32, offset)
    dyv.copy_(dy.reshape(-1))
    argd = arg.to(DEV).contiguous()
    runs = []
    for _ in range(2):
        db, dv = _guarded(max(N * C, 1), torch.float32, offset)              # poisoned with NaN: every row must be written
        check(lib().sn_segment_max_bwd_f32(ptr(dyv), ptr(argd), B, C, ptr(gp), ptr(dv), stream()), "sn_segment_max_bwd_f32")
        torch.cuda.synchronize()
        assert _intact(db, max(N * C, 1), offset)
        runs.append(dv[:N * C].reshape(N, C).cpu())
    assert runs[0].view(torch.int32).equal(runs[1].view(torch.int32))
    return runs[0]


def _same(a, ref64):
    """float32 result equals the float64 restatement exactly, NaN where it is NaN."""
    a = a.double()
    nan = torch.isnan(ref64)
    return bool((torch.isnan(a) == nan).all()) and torch.equal(torch.where(nan, torch.zeros_like(a), a), torch.where(nan, torch.zeros_like(a), ref64))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("C", RC.WIDTHS)
@pytest.mark.parametrize("li", range(len(RC.SIZE_LISTS)))
def test_kernel_grid_equals_the_restatement(li, C, offset):
    sizes = RC.SIZE_LISTS[li]
    x = RC.grid_input(sizes, C, seed=100 * li + C)
    want, warg = RC.segment_max_ref(x, sizes)
    out, arg = _call_max(x, sizes, offset)
    assert _same(out, want) and torch.equal(arg, warg)
    out2, _ = _call_max(x, sizes, offset, want_arg=False)
    assert _same(out2, want)
    # the adjoint: one non-zero per (graph, channel) of a non-empty graph, every row written
    dy = torch.randint(1, 513, (len(sizes), C), generator=torch.Generator().manual_seed(C)).float() / 256.0
    dx = _call_bwd(dy, arg, sizes, C, offset)
    assert torch.equal(dx.double(), RC.segment_max_bwd_ref(dy, warg, sizes, sum(sizes)))
    assert int((dx != 0).sum()) == C * sum(1 for n in sizes if n)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("C", RC.WIDTHS)
def test_exact_ties_go_to_the_lowest_row(C, offset):
    """Multiples of 2^-8 below 1; the maximum 2.0 planted at the first row, the last row, two rows that land in different row lanes,
    and every row — one pattern per graph, for sizes 17, 65 and 300.  arg is the lowest planted row at every channel."""
    sizes, plant, first = [], [], []
    for n in RC.TIE_SIZES:
        for rows in ([0], [n - 1], [3, n - 2], [n // 2 + 1, n // 2 + 2], list(range(n))):
            sizes.append(n)
            plant.append(rows)
    x = torch.randint(-256, 256, (sum(sizes), C), generator=torch.Generator().manual_seed(C)).float() / 256.0
    r = 0
    for n, rows in zip(sizes, plant):
        x[[r + i for i in rows]] = 2.0
        first.append(r + rows[0])
        r += n
    out, arg = _call_max(x, sizes, offset)
    assert bool((out == 2.0).all())
    assert torch.equal(arg, torch.tensor(first, dtype=torch.int32).reshape(-1, 1).expand(-1, C))
    want, warg = RC.segment_max_ref(x, sizes)
    assert torch.equal(arg, warg) and _same(out, want)


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("C", [1, 4, 77, 260])
def test_nan_and_empty_graphs(C, offset):
    sizes = [0, 17, 0, 65, 300, 2100, 1, 0]
    x = RC.grid_input(sizes, C, seed=7)
    starts = RC.graph_ptr(sizes).tolist()
    nan_rows = {1: [5], 3: [64, 10], 5: [2050, 2000], 6: [0]}              # graph -> rows with a NaN (4: none)
    for b, rows in nan_rows.items():
        for i in rows:
            x[starts[b] + i, ::2] = float("nan")                            # even channels only
    x[starts[4] + 7, :] = float("-inf")
    out, arg = _call_max(x, sizes, offset)
    want, warg = RC.segment_max_ref(x, sizes)
    assert _same(out, want) and torch.equal(arg, warg)
    for b in (0, 2, 7):
        assert bool((out[b] == 0).all()) and bool((arg[b] == -1).all())
    for b, rows in nan_rows.items():
        assert bool(torch.isnan(out[b, ::2]).all()) and bool((arg[b, ::2] == starts[b] + min(rows)).all())
        assert not bool(torch.isnan(out[b, 1::2]).any())
    assert not bool(torch.isnan(out[4]).any())
    # a graph whose every entry is -inf: the value is -inf at its first row, not the empty graph's 0
    y = torch.full((3, C), float("-inf"))
    o2, a2 = _call_max(y, [3], offset)
    assert bool((o2 == float("-inf")).all()) and bool((a2 == 0).all())


def test_host_ops_and_autograd_node():
    from signnet_basisnet_amd import autograd as AG, ops
    sizes = [0, 5, 17, 0, 65, 1]
    C = 77
    x = RC.grid_input(sizes, C, seed=3)
    plan = types.SimpleNamespace(B=len(sizes), graph_ptr=RC.graph_ptr(sizes).to(DEV))
    want, warg = RC.segment_max_ref(x, sizes)
    out, arg = ops.segment_max(x.to(DEV), plan, want_arg=True)
    assert _same(out.cpu(), want) and torch.equal(arg.cpu(), warg)
    assert torch.equal(ops.segment_max(x.to(DEV), plan), out)
    leaf = x.to(DEV).requires_grad_(True)
    y = AG.segment_max(leaf, plan)
    assert torch.equal(y.detach(), out)
    dy = torch.randn(len(sizes), C, generator=torch.Generator().manual_seed(1))
    (y * dy.to(DEV)).sum().backward()
    assert torch.equal(leaf.grad.cpu().double(), RC.segment_max_bwd_ref(dy, warg, sizes, sum(sizes)))
    # ops.segment_pool keeps its behaviour next to it
    mean = ops.segment_pool(x.to(DEV), plan, "mean").cpu()
    assert bool((mean[0] == 0).all()) and torch.allclose(mean[1], x[0:5].mean(0), rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------- the nets on the reference's fixtures
# train-mode tolerance and gradient coefficient of the sibling tests of each net (tests/test_lap_baselines_gpu.py TRAIN_TOL / GRAD_TOL)
TRAIN_TOL = {"gin": (5e-4, 5e-5), "gatedgcn": (1e-3, 1e-4), "gat": (1e-3, 1e-4), "pna": (1e-3, 1e-4), "transformer": (1e-3, 1e-4)}
GRAD_TOL = {"gin": 2e-3, "gatedgcn": 3e-3, "gat": 1e-4, "pna": 5e-3, "transformer": 2e-3}
ONE_LAUNCH = {"gin": "sn_gin_net_fused_f32", "gatedgcn": "sn_gatedgcn_fused_f32"}


def _inputs(fx, form="edges"):
    """A fresh graph object per call (a batch plan is cached on it).  form 'edges': the fixture's own edge list (the complete graph for
    the full-graph Transformer); 'bonds': the molecular graph for a net with full_graph_input = 'bonds'."""
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    full = "full_src" in fx.inp
    if full and form == "edges":
        g = Graph(fx.inp["full_src"].to(DEV), fx.inp["full_dst"].to(DEV), fx.inp["sizes"])
        g.edata["real"] = fx.inp["real"].to(DEV)
        e = fx.inp["e_full"].to(DEV)
    else:
        ei = fx.inp["edge_index"]
        g = Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"])
        e = fx.inp["edge_attr"].reshape(-1).to(DEV) if full else fx.inp["edge_attr"].to(DEV)
    sn = fx.inp["snorm_n"].to(DEV) if "snorm_n" in fx.inp else None
    pe = fx.inp["pos_enc"].to(DEV) if "pos_enc" in fx.inp else None
    return g, fx.inp["x"].reshape(-1).to(DEV), pe, e, sn


def _run(net, fx, form="edges"):
    from signnet_basisnet_amd import dgl_nets
    g, h, pe, e, sn = _inputs(fx, form)
    p = dgl_nets.handle_lap(net, pe, g) if pe is not None else None
    return net(g, h, p, e, sn)[0]


def _build(name, form="edges", **kw):
    fx, net = RC.build(name, DEV, **kw)
    if form == "bonds":
        net.full_graph_input = "bonds"
    return fx, net


def _spans(fn):
    from signnet_basisnet_amd import ops
    fn()
    rec = ops.KernelTimer()
    with rec:
        y = fn()
    return y, [n for n, _, _ in rec.spans]


def _forms(name):
    return ["edges", "bonds"] if name == "readout_max_transformer_full" else ["edges"]


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_eval_scores_match_the_reference_on_both_paths(name):
    for form in _forms(name):
        fx, net = _build(name, form)
        kind = str(fx.meta["net"])
        net.eval()

        def run():
            with torch.no_grad():
                return _run(net, fx, form).clone()
        y, names = _spans(run)
        print(f"{name} [{form}] eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, fx.out['eval/y64']):.2e}  "
              f"|ref - f64| {PU.relerr(fx.out['eval/y'], fx.out['eval/y64']):.2e}")
        close(y, fx.out["eval/y"], f"{name} [{form}]: eval y", ref64=fx.out["eval/y64"])
        net.check_last()
        if kind in ONE_LAUNCH:                                              # the one-launch path took it, with max in its epilogue
            assert names.count(ONE_LAUNCH[kind]) == 1 and "sn_segment_max_f32" not in names, names
            net.fused_stages = False
            y_l, names_l = _spans(run)
            assert ONE_LAUNCH[kind] not in names_l and names_l.count("sn_segment_max_f32") == 1, names_l
            close(y_l, fx.out["eval/y"], f"{name}: eval y (layer path)", ref64=fx.out["eval/y64"])
            close(y, y_l, f"{name}: one launch vs layer path")
        else:
            assert names.count("sn_segment_max_f32") == 1 and "sn_segment_pool_f32" not in names, names
        if hasattr(net, "_h_last") and kind != "gin":
            close(net._h_last, fx.out["eval/h_last"], f"{name}: eval h_last", ref64=fx.out["eval/h_last64"])
        # as many launches as the same net with readout 'mean'
        _, mean = _build(name, form, readout="mean")
        mean.eval()

        def run_mean():
            with torch.no_grad():
                return _run(mean, fx, form).clone()
        for fused in (True, False):
            net.fused_stages = mean.fused_stages = fused
            n_max, n_mean = _spans(run)[1], _spans(run_mean)[1]
            assert len(n_max) == len(n_mean), (fused, n_max, n_mean)
            assert [n.replace("sn_segment_max_f32", "sn_segment_pool_f32") for n in n_max] == n_mean


def test_transformer_one_launch_path_takes_max():
    """The one-launch Transformer kernel is written for hidden 64 = 8 heads of 8 (the fixtures are smaller): seeded random weights, the
    comparison of tests/test_lap_baselines_gpu.py's sum / mean test of the two paths."""
    from signnet_basisnet_amd import readout_models
    fx = RC.fixture("readout_max_transformer")
    torch.manual_seed(3)
    m = readout_models.TransformerNet(RC.net_params(fx, DEV, hidden_dim=64, out_dim=64, n_heads=8))
    PU.bn_randomize(m, 4)
    m = m.to(DEV).eval()

    def run():
        with torch.no_grad():
            return _run(m, fx).clone()
    y, names = _spans(run)
    assert names.count("sn_transformer_net_fused_f32") == 1 and "sn_segment_max_f32" not in names, names
    m.check_last()
    m.fused_stages = False
    y_l, names_l = _spans(run)
    assert "sn_transformer_net_fused_f32" not in names_l and names_l.count("sn_segment_max_f32") == 1
    assert bool(torch.isfinite(y).all())
    close(y, y_l, "transformer max: one launch vs layer path")
    m.readout = "mean"                       # another function: the kernel read the mode
    m.invalidate()
    m.fused_stages = True
    assert PU.relerr(run(), y) > 1e-3


def _check_buffers(net, fx, kind, what):
    rtol, atol = TRAIN_TOL[kind]
    sd, n = net.state_dict(), 0
    for k, ref in fx.out.items():
        if not k.startswith("train/bn/"):
            continue
        key = k[len("train/bn/"):]
        if key.endswith("num_batches_tracked"):
            assert int(sd[key]) == int(ref), f"{what}: {key}"
        else:
            torch.testing.assert_close(sd[key].cpu(), ref, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {key}: {m}")
        n += 1
    return n


def _check_gradients(net, fx, kind, what):
    """The rule of tests/test_dgl_basisnet_gpu.py::_check_param_grads (test_lap_baselines_gpu.py, test_training_gpu.py) against the
    reference's float64 gradients, over EVERY parameter — the sign-invariant encoder's included."""
    g64 = {k[len("train/grad64/"):]: v for k, v in fx.out.items() if k.startswith("train/grad64/")}
    gmax = max(float(g.abs().max()) for g in g64.values())
    seen, worst = 0, (0.0, None)
    for k, p in net.named_parameters():
        ref = g64.get(k, torch.zeros(p.shape, dtype=torch.float64))
        ours = p.grad if p.grad is not None else torch.zeros_like(p)
        scale = max(float(ref.abs().max()), 1e-2 * gmax)
        err = float((ours.detach().cpu().double() - ref).abs().max())
        worst = max(worst, (err / scale, k))
        assert err <= GRAD_TOL[kind] * scale + 1e-7, (what, k, err, scale)
        seen += 1
    print(f"{what}: worst gradient {worst[0]:.2e} of its scale ({worst[1]}); bound {GRAD_TOL[kind]:g}")
    assert seen > 10 and set(g64) <= {k for k, _ in net.named_parameters()}


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_train_mode_value_buffers_and_gradients_match_the_reference(name):
    for form in _forms(name):
        fx, net = _build(name, form)
        kind = str(fx.meta["net"])
        rtol, atol = TRAIN_TOL[kind]
        net.train()
        with torch.no_grad():
            yv = _run(net, fx, form)
        print(f"{name} [{form}] train y: |hip - ref| {PU.relerr(yv, fx.out['train/y']):.2e}  |ref - f64| {PU.relerr(fx.out['train/y'], fx.out['train/y64']):.2e}")
        torch.testing.assert_close(yv.cpu(), fx.out["train/y"], rtol=rtol, atol=atol)
        nb = _check_buffers(net, fx, kind, f"{name} [{form}] (train, no autograd)")
        assert nb or kind == "gat"                                          # (GAT has no BatchNorm)
        fx, net = _build(name, form)
        net.train()
        yg = _run(net, fx, form)
        assert yg.requires_grad
        torch.testing.assert_close(yg.detach().cpu(), fx.out["train/y"], rtol=rtol, atol=atol)
        net.loss(yg, fx.inp["target"].to(DEV)).backward()
        _check_buffers(net, fx, kind, f"{name} [{form}] (train, autograd)")
        _check_gradients(net, fx, kind, f"{name} [{form}]")


@pytest.mark.parametrize("readout", ["mean", "sum"])
@pytest.mark.parametrize("name", RC.FIXTURES)
def test_sum_and_mean_are_the_base_classes_bit_for_bit(name, readout):
    from signnet_basisnet_amd import dgl_nets
    fx, a = _build(name, readout=readout)
    _, b = RC.build(name, DEV, module=dgl_nets, readout=readout)
    for fused in (True, False):
        a.fused_stages = b.fused_stages = fused
        for mode in (False, True):
            a.train(mode), b.train(mode)
            with torch.no_grad():
                ya, yb = _run(a, fx), _run(b, fx)
            assert torch.equal(ya, yb), (fused, mode)
    ya, yb = _run(a.train(), fx), _run(b.train(), fx)
    ya.abs().sum().backward(), yb.abs().sum().backward()
    for (k, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), k


def test_seed_dropout_with_max():
    """One class takes dropout and max together: the masks depend on (seed, step) alone."""
    fx, net = _build("readout_max_gatedgcn_signinv", dropout=0.25)
    with torch.no_grad():                    # eval draws nothing: the scores of the net without dropout
        assert torch.equal(_run(net.eval(), fx), _run(_build("readout_max_gatedgcn_signinv")[1].eval(), fx))
    net.train()
    ys = []
    for seed in (5, 5, 6):
        net.seed_dropout(seed)
        with torch.no_grad():
            ys.append(_run(net, fx).clone())
    assert torch.equal(ys[0], ys[1]) and not torch.equal(ys[0], ys[2]) and bool(torch.isfinite(ys[0]).all())
    net.seed_dropout(5)
    y = _run(net, fx)
    y.abs().sum().backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)


@pytest.mark.parametrize("method", ["sign_flip", "abs_val", "canonical", "none", "sign_inv"])
def test_every_lap_method_through_handle_lap(method):
    """GatedGCN with max behind each lap_method: the layer path and the one-launch path agree, train mode differentiates."""
    from signnet_basisnet_amd import dgl_nets, readout_models
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    fx = RC.fixture("readout_max_gatedgcn_signinv")
    cfg = RC.net_params(fx, DEV, lap_method=method)
    if method != "sign_inv":
        cfg["sign_inv_net"] = "none"
    torch.manual_seed(2)
    m = readout_models.GatedGCNNet(cfg)
    PU.bn_randomize(m, 3)
    m = m.to(DEV).eval()
    ei = fx.inp["edge_index"]
    pe, h, e = fx.inp["pos_enc"].to(DEV), fx.inp["x"].reshape(-1).to(DEV), fx.inp["edge_attr"].to(DEV)

    def run():
        g = Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"])
        torch.manual_seed(9)
        return m(g, h, dgl_nets.handle_lap(m, pe, g), e, None)[0]
    with torch.no_grad():
        y = run().clone()
        m.fused_stages = False
        y_l = run().clone()
    close(y, y_l, f"{method}: one launch vs layer path")
    m.train()
    yt = run()
    m.loss(yt, fx.inp["target"].to(DEV)).backward()
    assert bool(torch.isfinite(yt).all()) and all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    assert bool(m.MLP_layer.FC_layers[0].weight.grad.any()) and bool(m.embedding_h.weight.grad.any())


# ----------------------------------------------------------------------------- captured and recorded paths
LISTS = [[0, 1, 2, 6], [2, 9, 0, 8]]          # two shuffled batches of the store_cases pool: four graphs each, max_graphs = 8
BUCKET = (96, 192)
LR, SEED = 1e-4, 7


def _step_net(seed=3):
    from signnet_basisnet_amd import optim, readout_models
    fx = RC.fixture("readout_max_gatedgcn_signinv")
    cfg = RC.net_params(fx, DEV, lap_method="none", sign_inv_net="none")
    torch.manual_seed(seed)
    m = readout_models.GatedGCNNet(cfg).to(DEV).train()
    return m, optim.FlatAdam(m.parameters(), lr=LR)


def _step_check(padded_losses, o2, batches, case="none"):
    """The padded steps against the eager loop on the unpadded batches: the comparison and bounds of
    tests/test_lap_baselines_gpu.py::test_captured_step_follows_the_eager_loop."""
    import test_lap_baselines_gpu as LB
    from test_dgl_bucketed_step_gpu import _close_losses, _close_params
    m1, o1 = _step_net()
    eager = LB._eager_loop(m1, o1, batches)
    mn, on = _step_net()
    noisy = LB._eager_loop(mn, on, LB._noisy(batches, case))
    print(f"eager {eager}\n noisy {noisy}\n padded {padded_losses}")
    assert all(map(lambda v: v == v and abs(v) < float("inf"), padded_losses))
    _close_losses(eager, noisy, padded_losses, rel=1e-5)
    _close_params(o1, on, o2, len(batches), LR)


@pytest.fixture(scope="module")
def pool():
    import store_cases as SC
    return SC.pool("zinc")


def test_bucketed_step_follows_the_eager_step(pool):
    import test_lap_baselines_gpu as LB
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    m2, o2 = _step_net()
    ds = LB._samples(pool, m2)
    batches = [LB._dev_batch(ds, idx) for idx in LISTS]
    s = DGLBucketedStep(m2, o2, max_graphs=8)
    padded = [s.step(b.g, b.h, b.p, b.e, b.sn, b.t, bucket=BUCKET).item() for b in batches]
    s.check()
    assert s.captures == 1 and s.hits == 1          # one bucket; B = 4 < max_graphs: four empty graph slots read 0
    _step_check(padded, o2, batches)
    LB._release(s)


def test_step_from_a_store_follows_the_eager_step(pool):
    import test_lap_baselines_gpu as LB
    from signnet_basisnet_amd.data import DGLGraphStore
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    m2, o2 = _step_net()
    ds = LB._samples(pool, m2)
    store = DGLGraphStore.from_samples(ds, DEV)
    s = DGLBucketedStep(m2, o2, max_graphs=8)
    padded = [s.step_from(store, idx, bucket=BUCKET).item() for idx in LISTS]
    s.check()
    assert s.captures == 1 and s.hits == 1
    _step_check(padded, o2, [LB._dev_batch(ds, idx) for idx in LISTS])
    LB._release(s)


def test_graphed_forward_replays_the_eager_forward():
    from signnet_basisnet_amd import dgl_nets, synth
    from signnet_basisnet_amd.serving import GraphedDGLForward
    from test_serving_gpu import _inputs as serving_inputs, _permuted
    m, _ = _step_net(2)
    PU.bn_randomize(m, 3)
    m.eval()
    a = synth.make_batch(24, seed=11)
    b = _permuted(a, list(reversed(range(24))))
    (ga, ha, pa, ea, _), (gb, hb, pb, eb, _) = serving_inputs(a, m.pos_enc_dim), serving_inputs(b, m.pos_enc_dim)
    pa, pb = pa.squeeze(-1).contiguous(), pb.squeeze(-1).contiguous()

    def eager(g, h, p, e):
        with torch.no_grad():
            return m(g, h, dgl_nets.handle_lap(m, p, g), e, None)[0].clone()
    ya, yb = eager(ga, ha, pa, ea), eager(gb, hb, pb, eb)
    assert not torch.equal(ya, yb)
    gf = GraphedDGLForward(m, ga, ha, pa, ea, None)
    assert torch.equal(gf().clone(), ya)
    assert torch.equal(gf(gb, hb, pb, eb).clone(), yb)          # a second batch of the recorded shape
    gf.check()


def test_full_graph_transformer_in_bond_form_through_the_bucketed_step():
    import bond_attention_cases as BC
    import test_bond_attention_gpu as TB
    from signnet_basisnet_amd import optim, readout_models
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    fx = RC.fixture("readout_max_transformer_full")

    def small():
        torch.manual_seed(5)
        net = readout_models.TransformerNet(RC.net_params(fx, DEV, pos_enc_dim=4))          # (the width of _batch's unread pos_enc)
        net.full_graph_input = "bonds"
        net = net.to(DEV).train()
        return net, optim.FlatAdam(net.parameters(), lr=LR)
    batches = [TB._batch(TB.BATCHES[0], 1), TB._batch(TB.BATCHES[1], 2)]
    m1, o1 = small()
    eager, ge = TB._eager(m1, o1, batches)
    m2, o2 = small()
    s = DGLBucketedStep(m2, o2, max_graphs=8, granule=TB.GRANULE)
    padded, gp = [], []
    for b in batches:
        padded.append(s.step(b.g, b.h, b.p, b.e, None, b.t).item())
        gp.append(TB._grads(m2))
    torch.cuda.synchronize()
    s.check()
    assert s.captures == 1 and s.hits == 1
    print("losses: eager", eager, "padded", padded)
    BC.close_losses(eager, eager, padded)          # (a NoPE net reads no pos_enc: the eager step's sensitivity to it is exactly 0)
    BC.close_grads(ge[0], ge[0], gp[0])
    s.release()
