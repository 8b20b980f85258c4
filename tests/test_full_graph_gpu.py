"""-m gpu: full-graph attention for TransformerNet (full_graph=True).

  op grid        sn_full_attention_f32 / sn_full_attention_bwd_f32 through the C ABI, between sentinel guards, against the float64
                 restatement of tests/full_graph_cases.py by parity_util.attributed — forward and every gradient; dgamma (a one-entry sum
                 with cancellation) on the scale max(|entry|, root-sum-square of its per-edge terms in float64); repeated calls
                 bit-identical; shapes, class counts, real patterns, gamma arms, a live clamp, strided blocks, 4-byte-offset views,
                 the refusals and the out-of-range class
  make_full_graph  sn_make_full_graph equals the restatement exactly; self loops and repeated edges raise
  modules        the three reference fixtures tests/golden/fullgraph_*.npz: eval, train-mode value path, differentiable path
Every figure is printed before it is asserted."""
import ctypes as C
import functools

import pytest
import torch

import full_graph_cases as FC
import parity_util as PU
from parity_util import attributed, close, close_conditioned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 65            # floats in front of and behind every output: an odd count, so that outputs sit at 4-byte-offset addresses
SENT = 12345.0
GRADS = ("Q", "K", "V", "Q2", "K2", "Tr", "Tf")


# ----------------------------------------------------------------------------- the op through the C ABI
def _plans(inp):
    from signnet_basisnet_amd import ops
    sizes = torch.tensor(inp.sizes)
    batch = torch.repeat_interleave(torch.arange(len(inp.sizes)), sizes).to(DEV)
    ei = torch.stack([inp.src, inp.dst]).to(DEV)
    return ops.build_plan(batch, ei, len(inp.sizes), 0), ops.build_plan(batch, ei.flip(0).contiguous(), len(inp.sizes), 0)


def _dev(inp, offset=False):
    """The case's tensors on the device; offset: every float block starts 4 bytes into its own allocation."""
    def put(t):
        if not offset:
            return t.to(DEV).contiguous()
        base = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        v = base[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 8 == 4 and v.is_contiguous()
        return v
    return {n: put(getattr(inp, n)) for n in FC.FLOATS + ("dout",)} | {"codes": inp.codes.to(DEV)}


def _guarded(*shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.float32, device=DEV)
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _intact(bufs, what):
    for buf, view in bufs:
        n = view.numel()
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + n:] == SENT).all()), f"{what}: a write outside an output"
        assert not bool(torch.isnan(view).any()), f"{what}: an output element was not written"


def call_fwd(t, inp, plan, ld=None, status=None):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    N, d = inp.Q.shape
    out, den = _guarded(N, d), _guarded(N, inp.heads)
    st = torch.zeros(1, dtype=torch.int32, device=DEV) if status is None else status
    check(lib().sn_full_attention_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), ld or d, ptr(t["Tr"]), ptr(t["Tf"]),
                                      inp.C, ptr(t["codes"]), ptr(t["gamma"]), N, inp.heads, d // inp.heads, ptr(plan.rowptr), ptr(plan.col),
                                      ptr(plan.eperm), ptr(out[1]), ptr(den[1]), ptr(st), stream()), "sn_full_attention_f32")
    _intact([out, den], "sn_full_attention_f32")
    if status is None:
        assert int(st.item()) == 0
    return out[1], den[1]


def call_bwd(t, inp, plan, rplan, out, den, ld=None):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    N, d = inp.Q.shape
    H, dk = inp.heads, d // inp.heads
    bufs = [_guarded(N, d) for _ in range(5)] + [_guarded(inp.C, d), _guarded(inp.C, d), _guarded(1)]
    scratch = torch.empty(max(int(lib().sn_full_attention_bwd_scratch_floats(N, plan.E, H, dk, inp.C)), 2), dtype=torch.float32, device=DEV)
    g = [ptr(b[1]) for b in bufs]
    check(lib().sn_full_attention_bwd_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), ld or d, ptr(t["Tr"]), ptr(t["Tf"]),
                                          inp.C, ptr(t["codes"]), ptr(t["gamma"]), ptr(out), ptr(den), ptr(t["dout"]), N, plan.E, H, dk,
                                          ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(rplan.rowptr), ptr(rplan.col),
                                          ptr(rplan.eperm), g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], ptr(scratch), stream()),
          "sn_full_attention_bwd_f32")
    _intact(bufs, "sn_full_attention_bwd_f32")
    # (dQ, dK, dV, dQ2, dK2, dTr, dTf, dgamma) -> by name
    names = ("Q", "K", "V", "Q2", "K2", "Tr", "Tf", "gamma")
    return {n: b[1] for n, b in zip(names, bufs)}


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(inputs, fp32 out, fp32 gradients, float64 out, float64 gradients, dgamma's term scale) of one case, computed once."""
    inp = FC.op_inputs(**dict(key))
    o32, g32 = FC.run_ref(inp, inp.dout, torch.float32)
    o64, g64 = FC.run_ref(inp, inp.dout, torch.float64)
    return inp, o32, g32, o64, g64, FC.dgamma_terms_rss(inp, inp.dout)


def _check_dgamma(hip, g32, g64, rss, gamma, what):
    hip, g32, g64 = float(hip), float(g32), float(g64)
    if not 0.0 <= gamma <= 1.0:
        assert hip == 0.0 and g64 == 0.0, f"{what}: dgamma must be exactly 0 on a clamped arm ({hip}, {g64})"
        return
    scale = max(abs(g64), rss)
    e_hip, e_cpu = abs(hip - g64), abs(g32 - g64)
    print(f"{what} d gamma: {hip:.6e} (f64 {g64:.6e}); |hip - f64| {e_hip / scale:.2e}  |cpu32 - f64| {e_cpu / scale:.2e} of max(|entry|, rss {rss:.3e})")
    assert e_hip <= max(PU.REL * scale, 2.0 * e_cpu + PU.ATTR * scale), what


def _run_case(case, offset=False):
    inp, o32, g32, o64, g64, rss = _reference(tuple(sorted(case.items())))
    what = " ".join(f"{k}={v}" for k, v in sorted(case.items()))
    plan, rplan = _plans(inp)
    t = _dev(inp, offset)
    out, den = call_fwd(t, inp, plan)
    e = attributed(out, o32, o64, f"{what}: out")
    print(f"{what} out: |hip - f64| {e[0]:.2e}  |cpu32 - f64| {e[1]:.2e}")
    # a node without in-edges: exactly 0
    deg = torch.bincount(inp.dst, minlength=inp.Q.shape[0])
    if bool((deg == 0).any()):
        assert not bool(out[(deg == 0).to(DEV)].any())
    grads = call_bwd(t, inp, plan, rplan, out, den)
    for n in GRADS:
        e = attributed(grads[n], g32[n], g64[n], f"{what}: d {n}")
        print(f"{what} d {n}: |hip - f64| {e[0]:.2e}  |cpu32 - f64| {e[1]:.2e}")
    _check_dgamma(grads["gamma"], g32["gamma"], g64["gamma"], rss, float(inp.gamma), what)
    # repeated calls are bit-identical
    out2, den2 = call_fwd(t, inp, plan)
    grads2 = call_bwd(t, inp, plan, rplan, out2, den2)
    assert _bits(out, out2) and _bits(den, den2) and all(_bits(grads[n], grads2[n]) for n in grads), f"{what}: not reproducible"
    return inp, t, plan, rplan, out, den, grads


SHAPES = [(8, 8), (4, 32), (1, 1), (3, 5), (8, 4)]


@pytest.mark.parametrize("heads,dk", SHAPES)
def test_op_shapes(heads, dk):
    _run_case(dict(heads=heads, dk=dk))


@pytest.mark.parametrize("C", [1, 16])
def test_op_class_counts(C):
    _run_case(dict(heads=3, dk=5, C=C, gamma=0.6))


@pytest.mark.parametrize("pattern", [p for p in FC.PATTERNS if p != "molecule"])
def test_op_real_patterns(pattern):
    _run_case(dict(heads=3, dk=5, pattern=pattern, gamma=0.6, seed=2))


@pytest.mark.parametrize("gamma", [0.6, -0.3, 1.7])
def test_op_gamma_arms(gamma):
    _run_case(dict(heads=8, dk=8, gamma=gamma, seed=3))


def test_op_with_a_live_clamp():
    inp = FC.op_inputs(**FC.CLAMP_CASE)
    rp, fp, rm, fm, near = FC.clamp_conditions(inp)
    assert rp >= 1 and fp >= 1 and rm >= 1 and fm >= 1 and near == 0, (rp, fp, rm, fm, near)
    _run_case(dict(FC.CLAMP_CASE))


def test_four_byte_offset_views_and_strided_blocks_are_bit_equal():
    from signnet_basisnet_amd import ops
    case = dict(heads=3, dk=5, seed=4, gamma=0.6)
    inp, t, plan, rplan, out, den, grads = _run_case(case)
    _, _, _, _, out_o, den_o, grads_o = _run_case(case, offset=True)
    assert _bits(out, out_o) and _bits(den, den_o) and all(_bits(grads[n], grads_o[n]) for n in grads)
    # the five blocks as the column blocks of one projection, read in place
    d = inp.Q.shape[1]
    P5 = torch.cat([t[n] for n in ("Q", "K", "V", "Q2", "K2")], 1).contiguous()
    v = [P5[:, i * d:(i + 1) * d] for i in range(5)]
    o5, den5 = ops.full_attention(*v, t["Tr"], t["Tf"], t["codes"], t["gamma"], plan, inp.heads, want_den=True)
    assert _bits(o5, out) and _bits(den5, den)
    g5 = ops.full_attention_bwd(*v, t["Tr"], t["Tf"], t["codes"], t["gamma"], o5, den5, t["dout"], plan, rplan, inp.heads)
    for n, g in zip(GRADS + ("gamma",), g5):
        assert _bits(g, grads[n]), n


def test_autograd_node_returns_the_c_abi_gradients():
    from signnet_basisnet_amd import autograd as AG
    inp, t, plan, rplan, out, den, grads = _run_case(dict(heads=8, dk=4))
    leaf = {n: t[n].clone().requires_grad_(True) for n in FC.FLOATS}
    o = AG.full_attention(leaf["Q"], leaf["K"], leaf["V"], leaf["Q2"], leaf["K2"], leaf["Tr"], leaf["Tf"], leaf["gamma"], t["codes"], plan, rplan,
                          inp.heads)
    assert _bits(o, out)
    o.backward(t["dout"])
    for n in FC.FLOATS:
        assert _bits(leaf[n].grad, grads[n].reshape(leaf[n].shape)), n


def test_zero_fake_weight_matches_the_sparse_kernel():
    """gamma = -0.3: L = 0, the fake edges weigh exactly 0 and the output is the shipped sparse attention over the real sub-list with
    Ee = T_real[class]."""
    from signnet_basisnet_amd import ops
    inp, t, plan, rplan, out, den, grads = _run_case(dict(heads=8, dk=8, gamma=-0.3, seed=3))
    m = (inp.codes & 1).bool()
    sizes = torch.tensor(inp.sizes)
    batch = torch.repeat_interleave(torch.arange(len(inp.sizes)), sizes).to(DEV)
    rplan_ = ops.build_plan(batch, torch.stack([inp.src[m], inp.dst[m]]).to(DEV), len(inp.sizes), 0)
    Ee = t["Tr"][(inp.codes[m].long() >> 1).to(DEV)].contiguous()
    sparse = ops.edge_attention(t["Q"], t["K"], t["V"], Ee, rplan_, inp.heads)
    print(f"full (L = 0) vs sn_edge_attention_f32 on the real edges: {PU.relerr(out, sparse):.2e}")
    close(out, sparse, "full attention at L = 0 vs edge_attention")


def test_limits_are_refused_through_the_c_abi():
    from signnet_basisnet_amd._lib import lib, ptr
    inp = FC.op_inputs(1, 1, sizes=(2, 3))
    plan, rplan = _plans(inp)
    t = _dev(inp)
    N = inp.Q.shape[0]
    one = torch.zeros(64, dtype=torch.float32, device=DEV)
    L = lib()

    def fwd(Cc, dk):
        return L.sn_full_attention_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), 64, ptr(t["Tr"]), ptr(t["Tf"]), Cc,
                                       ptr(t["codes"]), ptr(t["gamma"]), N, 1, dk, ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(one),
                                       ptr(one), None, None)

    def bwd(Cc, dk):
        p = ptr(one)
        return L.sn_full_attention_bwd_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), 64, ptr(t["Tr"]), ptr(t["Tf"]), Cc,
                                           ptr(t["codes"]), ptr(t["gamma"]), p, p, p, N, plan.E, 1, dk, ptr(plan.rowptr), ptr(plan.col),
                                           ptr(plan.eperm), ptr(rplan.rowptr), ptr(rplan.col), ptr(rplan.eperm), p, p, p, p, p, p, p, p, p, None)

    for fn, name in ((fwd, b"sn_full_attention_f32"), (bwd, b"sn_full_attention_bwd_f32")):
        assert fn(4, 33) == -1 and name in L.sn_last_error() and b"head width 33" in L.sn_last_error()
        assert fn(17, 1) == -1 and name in L.sn_last_error() and b"17 edge classes" in L.sn_last_error()
        assert fn(0, 1) == -1


def test_class_outside_the_table_is_flagged_and_raised():
    from signnet_basisnet_amd import ops
    inp = FC.op_inputs(3, 5, seed=6, sizes=(2, 5, 9))
    plan, _ = _plans(inp)
    t = _dev(inp)
    bad = t["codes"].clone()
    bad[7] = 2 * inp.C + 1            # class id = C on a real edge
    bad[8] = -2                       # and a negative one
    args = (t["Q"], t["K"], t["V"], t["Q2"], t["K2"], t["Tr"], t["Tf"])
    with pytest.raises(IndexError, match="index out of range"):
        ops.full_attention(*args, bad, t["gamma"], plan, inp.heads)
    st = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.full_attention(*args, bad, t["gamma"], plan, inp.heads, status=st)
    assert int(st.item()) == 1 and bool(torch.isfinite(out).all())
    with ops.defer_status() as words:
        ops.full_attention(*args, bad, t["gamma"], plan, inp.heads)
    with pytest.raises(IndexError):
        ops.raise_deferred(words)
    st.zero_()
    ops.full_attention(*args, t["codes"], t["gamma"], plan, inp.heads, status=st)
    assert int(st.item()) == 0
    with pytest.raises(ValueError, match="head width"):
        ops.full_attention(*(torch.zeros(plan.N, 33, device=DEV) for _ in range(5)), torch.zeros(4, 33, device=DEV),
                           torch.zeros(4, 33, device=DEV), t["codes"], t["gamma"], plan, 1)


# ----------------------------------------------------------------------------- make_full_graph
def _sparse_graph(sizes, src, dst):
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    return Graph(src.to(DEV), dst.to(DEV), torch.tensor(sizes))


def test_make_full_graph_equals_the_restatement():
    from signnet_basisnet_amd import ops
    sizes = FC.GRID_SIZES
    src, dst, cls = FC.molecule_edges(sizes, 9)
    perm = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(1))
    src, dst, cls = src[perm], dst[perm], cls[perm]
    rec = ops.KernelTimer()
    g = _sparse_graph(sizes, src, dst)
    with rec:
        full, ef = ops.make_full_graph(g, cls.to(DEV))
    assert [s[0] for s in rec.spans].count("sn_make_full_graph") == 1
    fs, fd, real, e_full = FC.make_full_graph_ref(sizes, src, dst, cls)
    got_s, got_d = full.edges()
    assert got_s.dtype == torch.int64 and full.edata["real"].dtype == torch.int64 and ef.dtype == torch.int64
    assert torch.equal(got_s.cpu(), fs) and torch.equal(got_d.cpu(), fd)
    assert torch.equal(full.edata["real"].cpu(), real) and torch.equal(ef.cpu(), e_full) and int(real.sum()) == src.numel()
    assert full.batch_num_nodes().tolist() == sizes and full.batch_num_edges().tolist() == [n * (n - 1) for n in sizes]
    # a batch without edges: every pair is fake
    none = torch.zeros(0, dtype=torch.int64)
    full0, ef0 = ops.make_full_graph(_sparse_graph([3, 1, 2], none, none), none.to(DEV))
    assert full0.edges()[0].numel() == 8 and not bool(full0.edata["real"].any()) and not bool(ef0.any())


@pytest.mark.parametrize("extra", [([3], [3]), ([0], [0]), ([1], [2])], ids=["self_loop", "self_loop_of_a_one_node_graph", "repeated_edge"])
def test_make_full_graph_refuses_self_loops_and_repeated_edges(extra):
    from signnet_basisnet_amd import ops
    sizes = [1, 3, 4]
    src, dst = torch.tensor([1, 2, 4, 5] + extra[0]), torch.tensor([2, 1, 5, 4] + extra[1])
    cls = torch.zeros(src.numel(), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="self loop or a repeated"):
        ops.make_full_graph(_sparse_graph(sizes, src, dst), cls)
    with ops.defer_status() as words:
        ops.make_full_graph(_sparse_graph(sizes, src, dst), cls)
    with pytest.raises(ValueError, match="self loop or a repeated"):
        ops.raise_deferred(words)


# ----------------------------------------------------------------------------- the modules on the reference fixtures
def build(name, cls=None, **over):
    from signnet_basisnet_amd import dgl_nets
    fx = FC.fixture(name)
    net = (cls or dgl_nets.TransformerNet)(FC.net_params(fx, **over))
    net.load_state_dict(fx.sd, strict=True)
    return net.to(DEV)


def inputs(fx):
    """A fresh graph object per call (a batch plan is cached on it by the first forward that sees it)."""
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    g = Graph(fx.inp["full_src"].to(DEV), fx.inp["full_dst"].to(DEV), fx.inp["sizes"])
    g.edata["real"] = fx.inp["real"].to(DEV)
    pe = fx.inp["pos_enc"].to(DEV) if "pos_enc" in fx.inp else None
    return g, fx.inp["x"].reshape(-1).to(DEV), pe, fx.inp["e_full"].to(DEV)


def run(net, fx):
    from signnet_basisnet_amd import dgl_nets
    g, h, pe, e = inputs(fx)
    p = dgl_nets.handle_lap(net, pe, g) if pe is not None else None
    return net(g, h, p, e, None)[0]


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_eval_forward_matches_the_reference(name):
    from signnet_basisnet_amd import ops
    fx = FC.fixture(name)
    net = build(name).eval()
    with torch.no_grad():
        y = run(net, fx)
    print(f"{name} eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, fx.out['eval/y64']):.2e}  "
          f"|ref - f64| {PU.relerr(fx.out['eval/y'], fx.out['eval/y64']):.2e}")
    close(y, fx.out["eval/y"], f"{name}: eval y", ref64=fx.out["eval/y64"])
    close(net._h_last, fx.out["eval/h_last"], f"{name}: eval h_last", ref64=fx.out["eval/h_last64"])
    assert net._stage(inputs(fx)[0]) is None
    # one launch per op (fused_layers = False) computes the same function
    net.fused_layers = False
    with torch.no_grad():
        y1 = run(net, fx)
    close(y1, fx.out["eval/y"], f"{name}: eval y (unfused)", ref64=fx.out["eval/y64"])
    # the graph from ops.make_full_graph gives the same bits as the fixture's stored edge list
    net.fused_layers = True
    from signnet_basisnet_amd import dgl_nets
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    ei = fx.inp["edge_index"]
    full, ef = ops.make_full_graph(Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"]), fx.inp["edge_attr"].reshape(-1).to(DEV))
    _, h, pe, _ = inputs(fx)
    with torch.no_grad():
        y2 = net(full, h, dgl_nets.handle_lap(net, pe, full) if pe is not None else None, ef, None)[0]
    assert _bits(y2, y)


def _check_buffers(net, fx, what):
    sd = net.state_dict()
    n = 0
    for k, ref in fx.out.items():
        if not k.startswith("train/bn/"):
            continue
        key = k[len("train/bn/"):]
        if key.endswith("num_batches_tracked"):
            assert int(sd[key]) == int(ref), f"{what}: {key}"
        else:
            close_conditioned(sd[key], ref, fx.out["train/bn64/" + key], f"{what}: {key}")
        n += 1
    assert n


def _check_gradients(net, fx, name):
    g32 = {k[len("train/grad/"):]: v for k, v in fx.out.items() if k.startswith("train/grad/")}
    g64 = {k[len("train/grad64/"):]: v for k, v in fx.out.items() if k.startswith("train/grad64/")}
    assert g32 and set(g32) == set(g64)
    got = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    assert set(g64) <= set(got), sorted(set(g64) - set(got))
    # (a bias in front of a batch-statistics BatchNorm has the gradient 0 and float64 returns its rounding noise: compared together with
    #  its Linear's weight gradient, as tests/test_dropout_modules_gpu.py does)
    gmax = max(float(g.abs().max()) for g in g64.values())
    paired = {k for k in g64 if k.endswith(".bias") and float(g64[k].abs().max()) <= 1e-12 * gmax and k[:-4] + "weight" in g64}
    for k in sorted(g64):
        print(f"{name} d {k}: |hip - f64| {PU.relerr(got[k], g64[k]):.2e}  |ref32 - f64| {PU.relerr(g32[k], g64[k]):.2e}")
    for l, gm in enumerate(fx.meta["gamma"]):
        k = f"layers.{l}.gamma"
        if not 0.0 <= float(gm) <= 1.0:
            assert float(got[k]) == 0.0 and float(g64[k]) == 0.0, k
            paired.add(k)                                            # (checked: exactly 0)
    for k in sorted(set(g64) - paired):
        close_conditioned(got[k], g32[k], g64[k], f"{name}: d {k}")
    for k in sorted(k for k in paired if k.endswith(".bias")):
        w = k[:-4] + "weight"
        both = lambda g: torch.cat([g[w].detach().cpu().reshape(-1), g[k].detach().cpu().reshape(-1)])          # noqa: E731
        close_conditioned(both(got), both(g32), both(g64), f"{name}: d ({w} | {k})")
    for k in ("layers.0.attention_h.Q_2.weight", "layers.0.attention_h.K_2.weight", "layers.0.attention_h.E_2.weight", "embedding_e.weight"):
        assert bool(got[k].any()), k


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_train_mode_matches_the_reference(name):
    fx = FC.fixture(name)
    y32, y64 = fx.out["train/y"], fx.out["train/y64"]
    # value path: train mode without autograd
    net = build(name).train()
    with torch.no_grad():
        yv = run(net, fx)
    print(f"{name} train y: |hip - ref| {PU.relerr(yv, y32):.2e}  |hip - f64| {PU.relerr(yv, y64):.2e}  |ref - f64| {PU.relerr(y32, y64):.2e}")
    close_conditioned(yv, y32, y64, f"{name}: train y")
    _check_buffers(net, fx, f"{name} (train, no autograd)")
    # differentiable path
    net = build(name).train()
    yg = run(net, fx)
    print(f"{name} train y (autograd): |hip - f64| {PU.relerr(yg, y64):.2e}")
    close_conditioned(yg, y32, y64, f"{name}: train y (autograd)")
    net.loss(yg, fx.inp["target"].to(DEV)).backward()
    _check_buffers(net, fx, f"{name} (train, autograd)")
    _check_gradients(net, fx, name)


def test_flat_adam_step_moves_the_fake_pair_parameters():
    from signnet_basisnet_amd import optim
    name = FC.FIXTURES[0]
    fx = FC.fixture(name)
    net = build(name).train()
    opt = optim.FlatAdam(net.parameters(), lr=1e-2)
    A = net.layers[0].attention_h
    watch = {"Q_2": A.Q_2.weight, "K_2": A.K_2.weight, "E_2": A.E_2.weight, "gamma": net.layers[0].gamma, "E": A.E.weight,
             "embedding_e": net.embedding_e.weight}
    before = {k: v.detach().clone() for k, v in watch.items()}
    opt.zero_grad()
    loss = net.loss(run(net, fx), fx.inp["target"].to(DEV))
    loss.backward()
    opt.step()
    for k, v in watch.items():
        assert not torch.equal(v.detach(), before[k]), k
    assert net.layers[0].gamma is net.layers[0].attention_h.gamma
    with torch.no_grad():
        assert bool(torch.isfinite(run(net.eval(), fx)).all())


def test_dropout_class_inherits_the_full_graph_paths():
    from signnet_basisnet_amd import dropout_models
    name = FC.FIXTURES[1]
    fx = FC.fixture(name)
    for mode in (False, True):
        a, b = build(name).train(mode), build(name, dropout_models.TransformerNet).train(mode)
        with torch.no_grad():
            assert _bits(run(a, fx), run(b, fx))
    net = build(name, dropout_models.TransformerNet, in_feat_dropout=0.1).train()
    for L in net.layers:              # as the reference: the net never hands `dropout` to its layers
        L.dropout = 0.25
    with torch.no_grad():
        yv = run(net, fx)
    y = run(net, fx)
    y.abs().sum().backward()
    assert bool(torch.isfinite(yv).all()) and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in net.parameters() if p.grad is not None)
    with torch.no_grad():
        y0 = run(build(name).train(), fx)
    assert PU.relerr(yv, y0) > 1e-4


def test_eval_layer_launches_nothing_with_a_row_per_pair(monkeypatch):
    """An eval layer is five launches — the packed projection, the attention, O_h, the two FFN Linears — and no Linear, embedding or
    pointwise launch runs over E_full rows: the attention is the only launch that sees the pairs."""
    from signnet_basisnet_amd import ops
    name = FC.FIXTURES[0]
    fx = FC.fixture(name)
    net = build(name).eval()
    with torch.no_grad():
        run(net, fx)                      # fills the eval cache (packed weights, class tables)
    E_full, N = fx.inp["full_src"].numel(), fx.inp["x"].shape[0]
    rows = []
    real_linear = ops.masked_linear
    monkeypatch.setattr(ops, "masked_linear", lambda x, *a, **k: (rows.append(x.shape[0]), real_linear(x, *a, **k))[1])
    rec = ops.KernelTimer()
    with rec, torch.no_grad():
        run(net, fx)
    names = [s[0] for s in rec.spans]
    L = len(net.layers)
    assert names.count("sn_full_attention_f32") == L and names.count("sn_masked_linear_f32") == 1 + 4 * L + 3
    assert names.count("sn_embedding_sum_f32") == 1 and not any("edge_attention" in n or "pointwise" in n for n in names)
    assert E_full not in rows and set(rows) <= {N, len(fx.inp["sizes"])}, rows
    assert set(names) <= {"sn_batch_plan", "sn_embedding_sum_f32", "sn_masked_linear_f32", "sn_full_attention_f32", "sn_segment_pool_f32"}, names
