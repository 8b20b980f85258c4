"""-m gpu: GatNet and ARMANet on the device — the attention kernel pair (sn_gat_conv_f32 / sn_gat_conv_bwd_f32) against float64 on every
graph and every group width of its dispatch table (tests/filter_attention_cases.py), its limits, the three fixture cases through the
float64 restatement, the captured epoch, the launch counts, and both nets once at the reference's full size (32 x 32 grid).

Tolerance (filter_cases.bound): 1e-5 of the quantity's scale against float64, or 4 x the error of the same formulas evaluated in fp32 on
the CPU (`rec`) where that is larger.  The scale is the quantity's largest magnitude.  A gradient that cancels to nothing — one node,
or rows whose logits all have one sign, where leaky_relu is linear and d att_r is identically zero — has no scale of its own; there
the scale is 1e-4 of the largest term of its sum (`floor` below), which holds such a gradient to 1e-9 of a term: float64 noise passes,
fp32 noise does not."""
import copy

import numpy as np
import pytest
import torch

import filter_attention_cases as AC
import filter_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _graph(name):
    from signnet_basisnet_amd.filter_baselines import FilterGraph
    ei, N = AC.GRAPHS[name]
    return ei, N, FilterGraph(torch.as_tensor(ei).to(DEV), N)


def _err(got, want, floor=0.0):
    want = want.detach().double().cpu().reshape(-1)
    got = got.detach().double().cpu().reshape(-1)
    return float((got - want).abs().max() / max(float(want.abs().max()), floor, 1e-300))


def _floors(feat, cot):
    f, c = float(feat.detach().abs().max()), float(cot.detach().abs().max())
    return {"out": 1e-4 * f, "lse": 0.0, "feat": 1e-4 * c, "att_l": 1e-4 * c * f * f, "att_r": 1e-4 * c * f * f, "bias": 1e-4 * c}


def _reference(tensors, cot, ei, N, heads, act, dtype):
    """filter_attention_cases.gat_conv_edges and its autograd gradients in `dtype` on the CPU."""
    t = {k: (None if v is None else v.detach().clone().to(dtype).requires_grad_(True)) for k, v in tensors.items()}
    out, lse = AC.gat_conv_edges(t["feat"], t["att_l"], t["att_r"], t["bias"], ei, N, heads, act)
    out.backward(cot.to(dtype))
    res = {"out": out.detach(), "lse": lse}
    res.update({k: v.grad for k, v in t.items() if v is not None})
    return res


def _raw_calls(t, cot, op, heads, C, act):
    """Both entry points on buffers with a NaN row in front of and behind every output: the rows must survive, every row between must
    be written.  -> out, lse, dfeat, the parameter partials."""
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    L, N, D = lib(), op.N, heads * C
    out, lse = torch.full((N + 2, D), NAN, device=DEV), torch.full((N + 2, heads), NAN, device=DEV)
    check(L.sn_gat_conv_f32(ptr(t["feat"]), ptr(t["att_l"]), ptr(t["att_r"]), ptr(t["bias"]), N, heads, C, 0.2, act, ptr(op.rowptr), ptr(op.col),
                            op.nnz, out[1:].data_ptr(), lse[1:].data_ptr(), stream()), "sn_gat_conv_f32")
    blocks = L.sn_gat_conv_bwd_blocks(N, heads, C)
    assert blocks == AC.bwd_blocks(N, heads, C)
    dfeat, part = torch.full((N + 2, D), NAN, device=DEV), torch.full((blocks + 2, 3 * D), NAN, device=DEV)
    work = torch.empty(5 * N * heads, dtype=torch.float64, device=DEV)
    o = out[1:-1].contiguous()
    check(L.sn_gat_conv_bwd_f32(ptr(t["feat"]), ptr(t["att_l"]), ptr(t["att_r"]), ptr(o), ptr(lse[1:-1].contiguous()), ptr(cot), N, heads, C, 0.2,
                                act, ptr(op.rowptr), ptr(op.col), ptr(op.t.rowptr), ptr(op.t.col), op.nnz, dfeat[1:].data_ptr(),
                                part[1:].data_ptr(), ptr(work), stream()), "sn_gat_conv_bwd_f32")
    for name, buf in (("out", out), ("lse", lse), ("dfeat", dfeat), ("part", part)):
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), name + ": a sentinel row was written"
        assert not bool(torch.isnan(buf[1:-1]).any()), name + ": a row was left unwritten"
    return o, lse[1:-1], dfeat[1:-1], part[1:-1]


def _check_config(name, ei, N, g, heads, C, act, with_bias, gen, scale_logits_to=None):
    from signnet_basisnet_amd import ops
    D = heads * C
    t = {"feat": torch.randn(N, D, generator=gen), "att_l": torch.randn(D, generator=gen), "att_r": torch.randn(D, generator=gen),
         "bias": torch.randn(D, generator=gen) if with_bias else None}
    cot = torch.randn(N, D, generator=gen)
    if scale_logits_to is not None:
        f = t["feat"].double().reshape(N, heads, C)
        al, ar = (f * t["att_l"].double().reshape(1, heads, C)).sum(-1), (f * t["att_r"].double().reshape(1, heads, C)).sum(-1)
        e = torch.as_tensor(np.asarray(ei)).long().reshape(2, -1)
        src, dst = torch.cat([e[0], torch.arange(N)]), torch.cat([e[1], torch.arange(N)])
        t["feat"] = t["feat"] * (scale_logits_to / float((al[src] + ar[dst]).abs().max()))       # the largest |al_j + ar_i| becomes 80
    want, want32 = _reference(t, cot, ei, N, heads, act, torch.float64), _reference(t, cot, ei, N, heads, act, torch.float32)
    d = {k: (None if v is None else v.to(DEV)) for k, v in t.items()}
    cd = cot.to(DEV)
    out, lse, dfeat, part = _raw_calls(d, cd, g.lap, heads, C, act)
    out2, lse2 = ops.gat_conv(d["feat"], d["att_l"], d["att_r"], d["bias"], g.lap, heads, "elu" if act else None)
    grads = ops.gat_conv_bwd(d["feat"], d["att_l"], d["att_r"], out2, lse2, cd, g.lap, heads, "elu" if act else None)
    again = ops.gat_conv_bwd(d["feat"], d["att_l"], d["att_r"], out2, lse2, cd, g.lap, heads, "elu" if act else None)
    assert torch.equal(out, out2) and torch.equal(lse, lse2) and torch.equal(dfeat, grads[0]), "two calls differ"
    assert all(torch.equal(a, b) for a, b in zip(grads, again)), "the reduced parameter gradients are not reproducible"
    got = {"out": out, "lse": lse, "feat": dfeat, "att_l": grads[1], "att_r": grads[2], "bias": grads[3]}
    # the partials the raw call left are the ones the wrapper reduced
    assert _err(part.double().sum(0), torch.cat([grads[1], grads[2], grads[3]]).double(), 1e-30) <= 1e-5
    floors = _floors(t["feat"], cot)
    worst = 0.0
    for k, w in want.items():
        assert bool(torch.isfinite(got[k]).all()), (name, heads, C, act, k)
        e, rec = _err(got[k], w, floors[k]), _err(want32[k], w, floors[k])
        worst = max(worst, e / FC.bound(rec))
        assert e <= FC.bound(rec), (name, heads, C, act, with_bias, k, e, rec)
    return worst, (t, d, out, lse)


# ----------------------------------------------------------------------------- 1. the kernel pair against float64
@pytest.mark.parametrize("name", AC.KERNEL_GRAPHS)
def test_kernels_against_float64(name):
    """Forward (out, lse) and adjoint (dfeat, d att_l, d att_r, d bias) on every graph: the small ones with every (heads, C) pair, both
    activations, with and without bias; ring1030 and the star with the pairs of LARGE_SHAPES, bias alternating."""
    ei, N, g = _graph(name)
    gen = torch.Generator().manual_seed(N + 11)
    if name in AC.LARGE_SHAPES:
        configs = [(hc, act, i % 2 == 0) for i, (hc, act) in enumerate(AC.LARGE_SHAPES[name])]
    else:
        configs = [(hc, act, b) for hc in AC.SHAPES + AC.EXTRA_SHAPES for act in (0, 1) for b in (True, False)]
    worst = 0.0
    for (heads, C), act, with_bias in configs:
        worst = max(worst, _check_config(name, ei, N, g, heads, C, act, with_bias, gen)[0])
    print(f"{name}: worst error / bound {worst:.3f} over {len(configs)} configurations")


@pytest.mark.parametrize("name,heads,C", [("grid6", 4, 8), ("dup_selfloop_shuffled", 2, 33), ("star", 1, 1)])
def test_logits_of_magnitude_80_stay_finite_and_within_bound(name, heads, C):
    ei, N, g = _graph(name)
    gen = torch.Generator().manual_seed(80)
    worst, (t, d, out, lse) = _check_config(name, ei, N, g, heads, C, 1, True, gen, scale_logits_to=80.0)
    f = t["feat"].double().reshape(N, heads, C)
    al = (f * t["att_l"].double().reshape(1, heads, C)).sum(-1)
    ar = (f * t["att_r"].double().reshape(1, heads, C)).sum(-1)
    e = torch.as_tensor(np.asarray(ei)).long().reshape(2, -1)
    s = al[torch.cat([e[0], torch.arange(N)])] + ar[torch.cat([e[1], torch.arange(N)])]
    s = s.detach()
    print(f"{name}: alpha_l + alpha_r in [{float(s.min()):.1f}, {float(s.max()):.1f}], |lse| up to {float(lse.abs().max()):.1f}; "
          f"worst error / bound {worst:.3f}")
    assert abs(float(s.abs().max()) - 80.0) < 1e-3 and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(out).all())


def test_isolated_node_duplicates_and_input_self_loops():
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.filter_baselines import FilterGraph
    gen = torch.Generator().manual_seed(5)
    # the isolated node 5 of path5_isolated attends over itself alone: feat + bias, to the bit
    ei, N, g = _graph("path5_isolated")
    for heads, C in ((3, 5), (2, 33)):
        feat, al, ar, b = (torch.randn(*s, generator=gen).to(DEV) for s in ((N, heads * C), (heads * C,), (heads * C,), (heads * C,)))
        out, lse = ops.gat_conv(feat, al, ar, b, g.lap, heads, None)
        assert torch.equal(out[5], feat[5] + b)
        assert torch.equal(ops.gat_conv(feat, al, ar, None, g.lap, heads, None)[0][5], feat[5])
        assert torch.equal(ops.gat_conv(feat, al, ar, b, g.lap, heads, "elu")[0][5], torch.nn.functional.elu(feat[5] + b))
    # a duplicated edge counts twice: 0 -> 1 given twice is not the graph with it once, and is the restatement with multiplicity 2
    once, twice = torch.tensor([[0, 2, 1], [1, 1, 2]]), torch.tensor([[0, 2, 0, 1], [1, 1, 1, 2]])
    heads, C = 2, 3
    feat, al, ar, b = (torch.randn(*s, generator=gen) for s in ((3, heads * C), (heads * C,), (heads * C,), (heads * C,)))
    outs = {}
    for key, e in (("once", once), ("twice", twice)):
        gg = FilterGraph(e.to(DEV), 3)
        outs[key] = ops.gat_conv(feat.to(DEV), al.to(DEV), ar.to(DEV), b.to(DEV), gg.lap, heads, "elu")[0].cpu()
        M = AC.dense_counts(e, 3)
        assert float(M[1, 0]) == (2.0 if key == "twice" else 1.0)
        assert _err(outs[key], AC.gat_conv_ref(feat.double(), al.double(), ar.double(), b.double(), M, heads, 1)) <= FC.bound()
    assert float((outs["once"][1] - outs["twice"][1]).abs().max()) > 1e-3 and torch.equal(outs["once"][2], outs["twice"][2])
    # an input self loop changes nothing: every node has exactly one loop either way
    looped = torch.cat([twice, torch.tensor([[1, 2], [1, 2]])], dim=1)
    g0, g1 = FilterGraph(twice.to(DEV), 3), FilterGraph(looped.to(DEV), 3)
    cot = torch.randn(3, heads * C, generator=gen).to(DEV)
    res = []
    for gg in (g0, g1):
        out, lse = ops.gat_conv(feat.to(DEV), al.to(DEV), ar.to(DEV), b.to(DEV), gg.lap, heads, "elu")
        res.append((out, lse) + ops.gat_conv_bwd(feat.to(DEV), al.to(DEV), ar.to(DEV), out, lse, cot, gg.lap, heads, "elu"))
    assert all(torch.equal(a, b_) for a, b_ in zip(*res))


def test_autograd_function_returns_all_four_gradients():
    from signnet_basisnet_amd import autograd as AG
    ei, N, g = _graph("dup_selfloop_shuffled")
    gen = torch.Generator().manual_seed(9)
    heads, C = 4, 8
    t = {"feat": torch.randn(N, heads * C, generator=gen), "att_l": torch.randn(1, heads, C, generator=gen),
         "att_r": torch.randn(1, heads, C, generator=gen), "bias": torch.randn(heads * C, generator=gen)}
    cot = torch.randn(N, heads * C, generator=gen)
    want, want32 = _reference(t, cot, ei, N, heads, 1, torch.float64), _reference(t, cot, ei, N, heads, 1, torch.float32)
    d = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    out = AG.gat_conv(d["feat"], d["att_l"], d["att_r"], d["bias"], g, heads, "elu")
    out.backward(cot.to(DEV))
    floors = _floors(t["feat"], cot)
    for k, v in d.items():
        assert v.grad is not None and v.grad.shape == v.shape, k
        assert _err(v.grad, want[k], floors[k]) <= FC.bound(_err(want32[k], want[k], floors[k])), k
    assert AG.gat_conv(d["feat"], d["att_l"], d["att_r"], None, g.lap, heads, None).shape == out.shape      # no bias, a bare operator


# ----------------------------------------------------------------------------- 2. limits
def test_one_above_each_limit_raises_without_a_launch():
    from signnet_basisnet_amd import ops
    ei, N, g = _graph("grid6")
    rec = ops.KernelTimer()
    with rec:
        for heads, C in ((AC.MAX_HEADS + 1, 1), (1, AC.MAX_C + 1)):
            D = heads * C
            feat, v = torch.zeros(N, D, device=DEV), torch.zeros(D, device=DEV)
            with pytest.raises(ValueError, match="limits"):
                ops.gat_conv(feat, v, v, v, g.lap, heads)
            with pytest.raises(ValueError, match="limits"):
                ops.gat_conv_bwd(feat, v, v, feat, torch.zeros(N, heads, device=DEV), feat, g.lap, heads)
        D = AC.MAX_HEADS * AC.MAX_C                                                # at the limits: runs
        out, _ = ops.gat_conv(torch.ones(N, D, device=DEV), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV), None, g.lap, AC.MAX_HEADS, None)
    assert [n for n, _, _ in rec.spans] == ["sn_gat_conv_f32"]
    assert torch.equal(out, torch.ones(N, D, device=DEV))                          # equal logits: the mean of equal rows


# ----------------------------------------------------------------------------- 3. the fixture cases
def _setup(case):
    from signnet_basisnet_amd import filter_baselines as FB
    from signnet_basisnet_amd import learning_filters as LF
    fx = AC.fixture()
    c = fx.cases[case]
    args = LF.FilterArgs(**c["args"])
    eig = LF.GridEigen(fx.inp["eigvals"].to(DEV), fx.inp["eigvecs"].to(DEV), args)
    model = LF.gen_model(args, eig, DEV, baselines="all")
    model.load_state_dict(c["sd"])
    graph = FB.FilterGraph(fx.edge_index.to(DEV), fx.N)
    x, y, m = fx.inp["x"][:, 0:1].contiguous().to(DEV), fx.inp["y"][:, 0:1].contiguous().to(DEV), fx.inp["m"].to(DEV)
    return fx, c, args, eig, model, graph, x, y, m


def _adam_spread(g, delta, lr, eps=1e-8):
    """How far Adam's first step lr * g / (|g| + eps) can move, element by element, when g moves by at most delta."""
    step = lambda v: lr * v / (v.abs() + eps)          # noqa: E731
    return torch.maximum((step(g + delta) - step(g)).abs(), (step(g - delta) - step(g)).abs())


@pytest.mark.parametrize("case", AC.NET_CASES)
def test_network_prediction_gradients_loss_curve_and_first_step(case):
    """Prediction, every first-step gradient and the four-step loss curve against the float64 restatement, bound per quantity from the
    fixture's recorded error of the fp32 CPU evaluation; the parameters after one FlatAdam step against the fixture's, element by
    element, as far as the gradient's bound lets Adam's first step move (an element whose gradient is within the bound of zero may go
    either way by lr; every other one is pinned)."""
    from signnet_basisnet_amd import learning_filters as LF
    from signnet_basisnet_amd.optim import Adam, FlatAdam
    fx, c, args, eig, model, graph, x, y, m = _setup(case)
    pre64, grads64, losses64 = AC.fixture_ref64(case)
    model.train()
    feat = LF.get_lap_feat(args.use_eig, eig, x, args.lap_method, model)
    assert torch.equal(feat.cpu(), c["feat"])
    pre = model(feat, graph)
    with torch.no_grad():
        model.eval()
        assert torch.equal(model(feat, fx.edge_index.to(DEV)), pre)            # eval mode, and an edge tensor in place of the FilterGraph
        model.train()
    e = _err(pre, pre64)
    print(f"{case}: prediction {e:.2e} (bound {FC.bound(c['err64/pre']):.2e})")
    assert e <= FC.bound(c["err64/pre"])
    LF.masked_square_loss(pre, y, m).backward()
    named = dict(model.named_parameters())
    assert {k for k, p in named.items() if p.grad is not None} == set(grads64)
    for k, g64 in grads64.items():
        e = _err(named[k].grad, g64)
        print(f"{case}: grad {k} {e:.2e} (bound {FC.bound(c['err64/grad/' + k]):.2e})")
        assert e <= FC.bound(c["err64/grad/" + k]), k
    stepped = copy.deepcopy(model)
    opt = Adam(model.parameters(), lr=args.lr)
    losses = [LF.train_step(model, opt, args, eig, x, y, m, graph)[0].item() for _ in range(4)]
    e = _err(torch.tensor(losses, dtype=torch.float64), losses64)
    print(f"{case}: losses {losses} {e:.2e} (bound {FC.bound(c['err64/losses']):.2e})")
    assert e <= FC.bound(c["err64/losses"])
    LF.train_step(stepped, FlatAdam(stepped.parameters(), lr=args.lr), args, eig, x, y, m, graph)
    for k, v in stepped.state_dict().items():
        gk = k.replace("lin_r", "lin_l")
        if gk in grads64:
            # Adam's first step is lr * g / (|g| + eps), monotone in g: a gradient within delta of the float64 one lands within
            # _adam_spread(g64, delta) of the float64 step.  Ours is allowed delta = bound * max|g64|, the fixture's fp32 run has its
            # recorded err64 * max|g64|.  Both then work in fp32: the step passes through about five roundings (m, v, its root, the
            # bias corrections, the quotient: 5 ulps of lr each way) and p - step is rounded once more (an ulp of |p| each way).
            g64, gmax = grads64[gk], float(grads64[gk].abs().max())
            tol = _adam_spread(g64, FC.bound(c["err64/grad/" + gk]) * gmax, args.lr) + _adam_spread(g64, c["err64/grad/" + gk] * gmax, args.lr) \
                + 2.4e-7 * (c["sd"][k].double().abs() + 5 * args.lr)
            assert bool(((v.detach().cpu().double() - c["sd1"][k].double()).abs() <= tol).all()), k
        else:
            assert torch.equal(v.cpu(), c["sd1"][k]) and torch.equal(v.cpu(), c["sd"][k]), k      # ARMAConv.weight: never moves


@pytest.mark.parametrize("case", AC.NET_CASES)
def test_graphed_epoch_replays_the_eager_step_bit_for_bit(case):
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


# ----------------------------------------------------------------------------- 4. launch counts
# Launches behind one recorded entry point, where it is not one.  ops.KernelTimer records entry points, not launches: the 2 is READ from
# the source (sn_gat_conv_bwd_f32 issues k_gat_bwd_dst and k_gat_bwd_src, csrc/filter_attention.hip), not measured.  What the test
# measures is which entry points a layer calls and how often; "at most 3" then follows from 2 + the one reduction.
LAUNCHES = {"sn_gat_conv_bwd_f32": 2}


def _spans(fn):
    from signnet_basisnet_amd import ops
    fn()
    rec = ops.KernelTimer()
    with rec:
        y = fn()
    return y, [n for n, _, _ in rec.spans]


def test_launch_counts():
    from signnet_basisnet_amd import filter_baselines as FB
    ei, N, g = _graph("grid6")
    x = torch.randn(N, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    conv = FB.GATConv(3, 8, heads=4).to(DEV)

    def fwd():
        with torch.no_grad():
            return conv(x, g, act="elu")
    _, names = _spans(fwd)
    assert names == ["sn_masked_linear_f32", "sn_gat_conv_f32"], names           # a GATConv layer forward: the GEMM and the attention
    xg = x.clone().requires_grad_(True)

    def bwd():
        conv.zero_grad()
        conv(xg, g, act="elu").sum().backward()
    _, names = _spans(bwd)
    i = names.index("sn_gat_conv_bwd_f32")
    attention = names[i:i + 2]
    assert attention == ["sn_gat_conv_bwd_f32", "sn_train_reduce_parts_f32"] and names.count("sn_gat_conv_bwd_f32") == 1, names
    assert sum(LAUNCHES.get(n, 1) for n in attention) <= 3
    assert all(p.grad is not None for p in conv.parameters()) and xg.grad is not None
    # ARMANet adds no launch of a new kernel: nothing it runs is outside what GcnNet and BernNet already run
    def train(net):
        def run():
            net.zero_grad()
            net(x, g).sum().backward()
        return set(_spans(run)[1])
    known = train(FB.GcnNet(3).to(DEV)) | train(FB.BernNet(3).to(DEV))
    arma = train(FB.ARMANet(3).to(DEV))
    assert arma <= known and not any(n.startswith("sn_gat_conv") for n in arma), arma - known
    assert "sn_poly_combine_f32" in arma


# ----------------------------------------------------------------------------- 5. full size, once
@pytest.mark.parametrize("net", ["GatNet", "ARMANet"])
def test_full_size_32x32_grid(net):
    """The reference's size (N = 1024, hidden 32, 2 layers, 4 heads): the prediction and one training step — loss and every gradient —
    against the dense float64 restatement; `rec` is the same restatement in fp32."""
    from signnet_basisnet_amd import filter_baselines as FB
    from signnet_basisnet_amd import learning_filters as LF
    from signnet_basisnet_amd import synth
    ei, N = synth.grid_graph(32)
    torch.manual_seed(0)
    model = FB.EXTRA_NETS[net](1).to(DEV)
    gen = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    x, y = torch.randn(N, 1, generator=gen), torch.randn(N, 1, generator=gen)
    m = torch.ones(N, 1)
    graph = FB.FilterGraph(torch.as_tensor(np.asarray(ei)).to(DEV), N)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    pre64, g64, l64 = AC.net_ref_training(net, sd, x, ei, N, y, m, steps=1)
    pre32, g32, l32 = AC.net_ref_training(net, sd, x, ei, N, y, m, steps=1, dtype=torch.float32)
    model.train()
    pre = model(x.to(DEV), graph)
    loss = LF.masked_square_loss(pre, y.to(DEV), m.to(DEV))
    loss.backward()
    checks = [("pre", pre, pre64, pre32), ("loss", loss.reshape(1), l64, l32)]
    named = dict(model.named_parameters())
    assert {k for k, p in named.items() if p.grad is not None} == set(g64)
    checks += [("grad " + k, named[k].grad, g64[k], g32[k]) for k in g64]
    for what, got, w64, w32 in checks:
        e, rec = _err(got, w64), _err(w32, w64)
        print(f"32x32 {net} {what}: {e:.2e} (the restatement in fp32: {rec:.2e}, bound {FC.bound(rec):.2e})")
        assert e <= FC.bound(rec), what
