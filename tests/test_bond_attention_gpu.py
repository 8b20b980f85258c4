"""-m gpu: full-graph attention from the bond graph.

  op grid    sn_bond_full_attention_f32 / sn_bond_full_attention_bwd_f32 through the C ABI, between sentinel guards, against the float64
             restatement by parity_util.attributed — forward and every gradient; dgamma on the scale max(|entry|, root-sum-square of
             its per-pair terms); repeated calls bit-identical; the case table of tests/bond_attention_cases.py (shapes, patterns,
             gamma arms, a live clamp, graphs at the staging limits, a 450-node graph, an empty graph), strided blocks and
             4-byte-offset views, status words, refusals, and a padded batch whose spare graph changes no bit
  modules    the three reference fixtures in bond form: eval, train-mode value path, differentiable path, the launches of an eval layer
  wrappers   DGLBucketedStep (step, step_from on a DGLGraphStore), GraphedDGLForward, the refusals that stay
Every figure is printed before it is asserted."""
import functools
import types

import pytest
import torch

import bond_attention_cases as BC
import full_graph_cases as FC
import parity_util as PU
from parity_util import attributed, close, close_conditioned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 65            # floats in front of and behind every output: an odd count, so that outputs sit at 4-byte-offset addresses
SENT = 12345.0
GRADS = ("Q", "K", "V", "Q2", "K2", "Tr", "Tf")


# ----------------------------------------------------------------------------- the op through the C ABI
def _plan(sizes, src, dst):
    from signnet_basisnet_amd import ops
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).to(DEV)
    return ops.build_plan(batch, torch.stack([src, dst]).to(DEV), len(sizes), 0)


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
    return {n: put(getattr(inp, n)) for n in FC.FLOATS + ("dout",)} | {"e": inp.bcls.to(DEV)}


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


def call_fwd(t, inp, plan, status=None, gv=None, ev=None, e=None):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    N, d = inp.Q.shape
    out, den = _guarded(N, d), _guarded(N, inp.heads)
    st = torch.zeros(2, dtype=torch.int32, device=DEV) if status is None else status
    check(lib().sn_bond_full_attention_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), d, ptr(t["Tr"]), ptr(t["Tf"]),
                                           inp.C, ptr(t["e"] if e is None else e), ptr(t["gamma"]), N, plan.B, plan.E, inp.heads,
                                           d // inp.heads, ptr(plan.graph_ptr), ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(gv),
                                           ptr(ev), ptr(out[1]), ptr(den[1]), ptr(st), stream()), "sn_bond_full_attention_f32")
    _intact([out, den], "sn_bond_full_attention_f32")
    if status is None:
        assert st.tolist() == [0, 0]
    return out[1], den[1]


def call_bwd(t, inp, plan, out, den, gv=None, ev=None):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    N, d = inp.Q.shape
    H, dk = inp.heads, d // inp.heads
    bufs = [_guarded(N, d) for _ in range(5)] + [_guarded(inp.C, d), _guarded(inp.C, d), _guarded(1)]
    scratch = torch.empty(max(int(lib().sn_bond_full_attention_bwd_scratch_floats(N, plan.B, H, dk, inp.C)), 2), dtype=torch.float32, device=DEV)
    g = [ptr(b[1]) for b in bufs]
    check(lib().sn_bond_full_attention_bwd_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), d, ptr(t["Tr"]), ptr(t["Tf"]),
                                               inp.C, ptr(t["e"]), ptr(t["gamma"]), ptr(out), ptr(den), ptr(t["dout"]), N, plan.B, plan.E, H, dk,
                                               ptr(plan.graph_ptr), ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), ptr(gv), ptr(ev),
                                               g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], ptr(scratch), stream()),
          "sn_bond_full_attention_bwd_f32")
    _intact(bufs, "sn_bond_full_attention_bwd_f32")
    names = ("Q", "K", "V", "Q2", "K2", "Tr", "Tf", "gamma")
    return {n: b[1] for n, b in zip(names, bufs)}


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _key(case):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in case.items()))


@functools.lru_cache(maxsize=None)
def _reference(key):
    """(inputs, fp32 out, fp32 gradients, float64 out, float64 gradients, dgamma's term scale) of one case, computed once: the float64
    (and fp32 CPU) restatement on the case's expanded edge list."""
    inp = BC.bond_inputs(**dict(key))
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
    inp, o32, g32, o64, g64, rss = _reference(_key(case))
    what = " ".join(f"{k}={v}" for k, v in sorted(case.items()) if k != "sizes")
    plan = _plan(inp.sizes, inp.bsrc, inp.bdst)
    t = _dev(inp, offset)
    out, den = call_fwd(t, inp, plan)
    e = attributed(out, o32, o64, f"{what}: out")
    print(f"{what} out: |hip - f64| {e[0]:.2e}  |cpu32 - f64| {e[1]:.2e}")
    off = 0
    for n in inp.sizes:                   # a one-node graph has no pair: exact zeros
        if n == 1:
            assert not bool(out[off].any()) and not bool(den[off].any())
        off += n
    grads = call_bwd(t, inp, plan, out, den)
    for n in GRADS:
        e = attributed(grads[n], g32[n], g64[n], f"{what}: d {n}")
        print(f"{what} d {n}: |hip - f64| {e[0]:.2e}  |cpu32 - f64| {e[1]:.2e}")
    assert not bool(grads["Tf"][1:].any()), "rows >= 1 of dT_fake are zero"
    _check_dgamma(grads["gamma"], g32["gamma"], g64["gamma"], rss, float(inp.gamma), what)
    out2, den2 = call_fwd(t, inp, plan)
    grads2 = call_bwd(t, inp, plan, out2, den2)
    assert _bits(out, out2) and _bits(den, den2) and all(_bits(grads[n], grads2[n]) for n in grads), f"{what}: not reproducible"
    return inp, t, plan, out, den, grads


def _id(case):
    return " ".join(f"{k}={v}" for k, v in sorted(case.items()) if k != "sizes") + (f" graphs={len(case['sizes'])}" if "sizes" in case else "")


@pytest.mark.parametrize("case", BC.CASES, ids=_id)
def test_op_case_table(case):
    if case == BC.CLAMP_CASE:
        rp, fp, rm, fm, near = FC.clamp_conditions(BC.bond_inputs(**case))
        assert rp >= 1 and fp >= 1 and rm >= 1 and fm >= 1 and near == 0, (rp, fp, rm, fm, near)
    _run_case(dict(case))


def test_four_byte_offset_views_and_strided_blocks_are_bit_equal():
    from signnet_basisnet_amd import ops
    case = dict(heads=3, dk=5, seed=4, gamma=0.6)
    inp, t, plan, out, den, grads = _run_case(case)
    _, _, _, out_o, den_o, grads_o = _run_case(case, offset=True)
    assert _bits(out, out_o) and _bits(den, den_o) and all(_bits(grads[n], grads_o[n]) for n in grads)
    # the five blocks as the column blocks of one [N, 5d] projection, read in place
    d = inp.Q.shape[1]
    P5 = torch.cat([t[n] for n in ("Q", "K", "V", "Q2", "K2")], 1).contiguous()
    v = [P5[:, i * d:(i + 1) * d] for i in range(5)]
    o5, den5 = ops.bond_full_attention(*v, t["Tr"], t["Tf"], t["e"], t["gamma"], plan, inp.heads, want_den=True)
    assert _bits(o5, out) and _bits(den5, den)
    g5 = ops.bond_full_attention_bwd(*v, t["Tr"], t["Tf"], t["e"], t["gamma"], o5, den5, t["dout"], plan, inp.heads)
    for n, g in zip(GRADS + ("gamma",), g5):
        assert _bits(g, grads[n]), n


def test_bond_form_follows_the_edge_list_kernel():
    """The same batch through sn_make_full_graph + sn_full_attention_f32: the two kernels sum a destination's pairs in different
    orders, so they agree as two fp32 evaluations of one function do (the project's close rule), not bit for bit."""
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    inp, t, plan, out, den, grads = _run_case(dict(heads=8, dk=8, gamma=0.6, seed=3))
    full, ef = ops.make_full_graph(Graph(inp.bsrc.to(DEV), inp.bdst.to(DEV), torch.tensor(inp.sizes)), t["e"])
    fplan = _plan(inp.sizes, *(x.cpu() for x in full.edges()))
    codes = ops.full_graph_codes(ef, full.edata["real"])
    edge = ops.full_attention(t["Q"], t["K"], t["V"], t["Q2"], t["K2"], t["Tr"], t["Tf"], codes, t["gamma"], fplan, inp.heads)
    print(f"bond form vs edge-list kernel: {PU.relerr(out, edge):.2e}")
    close(out, edge, "bond form vs edge-list kernel")


def test_autograd_node_returns_the_c_abi_gradients():
    from signnet_basisnet_amd import autograd as AG
    inp, t, plan, out, den, grads = _run_case(dict(heads=8, dk=4))
    leaf = {n: t[n].clone().requires_grad_(True) for n in FC.FLOATS}
    o = AG.bond_full_attention(leaf["Q"], leaf["K"], leaf["V"], leaf["Q2"], leaf["K2"], leaf["Tr"], leaf["Tf"], leaf["gamma"], t["e"], plan,
                               inp.heads)
    assert _bits(o, out)
    o.backward(t["dout"])
    for n in FC.FLOATS:
        assert _bits(leaf[n].grad, grads[n].reshape(leaf[n].shape)), n


def test_limits_are_refused_through_the_c_abi():
    from signnet_basisnet_amd._lib import lib, ptr
    inp = BC.bond_inputs(1, 1, sizes=(2, 3))
    plan = _plan(inp.sizes, inp.bsrc, inp.bdst)
    t = _dev(inp)
    N = inp.Q.shape[0]
    one = torch.zeros(64, dtype=torch.float32, device=DEV)
    L = lib()

    def fwd(Cc, dk):
        return L.sn_bond_full_attention_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), 64, ptr(t["Tr"]), ptr(t["Tf"]), Cc,
                                            ptr(t["e"]), ptr(t["gamma"]), N, plan.B, plan.E, 1, dk, ptr(plan.graph_ptr), ptr(plan.rowptr),
                                            ptr(plan.col), ptr(plan.eperm), None, None, ptr(one), ptr(one), None, None)

    def bwd(Cc, dk):
        p = ptr(one)
        return L.sn_bond_full_attention_bwd_f32(ptr(t["Q"]), ptr(t["K"]), ptr(t["V"]), ptr(t["Q2"]), ptr(t["K2"]), 64, ptr(t["Tr"]), ptr(t["Tf"]),
                                                Cc, ptr(t["e"]), ptr(t["gamma"]), p, p, p, N, plan.B, plan.E, 1, dk, ptr(plan.graph_ptr),
                                                ptr(plan.rowptr), ptr(plan.col), ptr(plan.eperm), None, None, p, p, p, p, p, p, p, p, p, None)

    for fn, name in ((fwd, b"sn_bond_full_attention_f32"), (bwd, b"sn_bond_full_attention_bwd_f32")):
        assert fn(4, 33) == -1 and name in L.sn_last_error() and b"head width 33" in L.sn_last_error()
        assert fn(17, 1) == -1 and name in L.sn_last_error() and b"17 edge classes" in L.sn_last_error()
        assert fn(0, 1) == -1


def test_class_outside_the_table_is_flagged_and_contributes_nothing():
    from signnet_basisnet_amd import ops
    inp = BC.bond_inputs(3, 5, seed=6, sizes=(2, 5, 9))
    plan = _plan(inp.sizes, inp.bsrc, inp.bdst)
    t = _dev(inp)
    args = (t["Q"], t["K"], t["V"], t["Q2"], t["K2"], t["Tr"], t["Tf"])
    for value in (inp.C, -1):
        bad = t["e"].clone()
        bad[3] = value
        with pytest.raises(IndexError, match="index out of range"):
            ops.bond_full_attention(*args, bad, t["gamma"], plan, inp.heads)
        st = torch.zeros(2, dtype=torch.int32, device=DEV)
        out = ops.bond_full_attention(*args, bad, t["gamma"], plan, inp.heads, status=st)
        assert st.tolist() == [1, 0] and bool(torch.isfinite(out).all())
        # the pair contributes nothing: the float64 restatement without that pair
        keep = torch.ones(inp.src.numel(), dtype=torch.bool)
        keep[(inp.src == inp.bsrc[3]) & (inp.dst == inp.bdst[3])] = False
        a = FC.to_dtype(inp, torch.float64)
        ref = FC.full_attention_ref(a.Q, a.K, a.V, a.Q2, a.K2, a.Tr, a.Tf, a.codes[keep], a.gamma, a.src[keep], a.dst[keep], a.heads)
        close(out, ref.float(), "a bond of a class outside the table contributes nothing", ref64=ref)
    with ops.defer_status() as words:
        ops.bond_full_attention(*args, bad, t["gamma"], plan, inp.heads)
    with pytest.raises(IndexError):
        ops.raise_deferred(words)
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    ops.bond_full_attention(*args, t["e"], t["gamma"], plan, inp.heads, status=st)
    assert st.tolist() == [0, 0]
    with pytest.raises(ValueError, match="head width"):
        ops.bond_full_attention(*(torch.zeros(plan.N, 33, device=DEV) for _ in range(5)), torch.zeros(4, 33, device=DEV),
                                torch.zeros(4, 33, device=DEV), t["e"], t["gamma"], plan, 1)


@pytest.mark.parametrize("extra,flag", [(([3], [3]), 1), (([0], [0]), 1), (([1], [2]), 2)],
                         ids=["self_loop", "self_loop_of_a_one_node_graph", "repeated_edge"])
def test_self_loops_and_repeated_bonds_raise_the_flag(extra, flag):
    """The flags of sn_make_full_graph (1: a self loop, 2: a repeated (u, v)) in the second status word; nothing faults, every output is
    written and finite."""
    from signnet_basisnet_amd import ops
    sizes = [1, 3, 4]
    inp = BC.bond_inputs(2, 4, sizes=tuple(sizes), seed=12)
    src, dst = torch.tensor([1, 2, 4, 5] + extra[0]), torch.tensor([2, 1, 5, 4] + extra[1])
    inp.bsrc, inp.bdst, inp.bcls = src, dst, torch.zeros(src.numel(), dtype=torch.int64)
    plan = _plan(sizes, src, dst)
    t = _dev(inp)
    st = torch.zeros(2, dtype=torch.int32, device=DEV)
    out, den = call_fwd(t, inp, plan, status=st)
    assert st.tolist() == [0, flag] and bool(torch.isfinite(out).all())
    grads = call_bwd(t, inp, plan, out, den)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    args = (t["Q"], t["K"], t["V"], t["Q2"], t["K2"], t["Tr"], t["Tf"], t["e"], t["gamma"], plan, inp.heads)
    with pytest.raises(ValueError, match="self loop, a repeated"):
        ops.bond_full_attention(*args)
    with ops.defer_status() as words:
        ops.bond_full_attention(*args)
    with pytest.raises(ValueError, match="self loop, a repeated"):
        ops.raise_deferred(words)


@pytest.mark.parametrize("case", [dict(heads=8, dk=8, gamma=0.6, seed=3, sizes=(5, 9, 17, 1, 33)), dict(BC.LIMIT_CASE)], ids=["staged", "limits"])
def test_an_invalid_spare_graph_changes_no_bit(case):
    """A padded batch: two empty graphs and a spare graph of 300 nodes appended, with self-loop padding edges spread over its nodes
    (hundreds of nodes, self loops, repeated edges — the bucket's convention), graph_valid 0 and edge_valid 0.  Its rows are exact
    zeros, no flag is raised, and every valid row and gradient — tables and dgamma included — is bit-equal to the unpadded call."""
    inp, t, plan, out, den, grads = _run_case(case)
    N, E, B = inp.Q.shape[0], inp.bsrc.numel(), len(inp.sizes)
    spare, pad_e = 300, 700
    gen = torch.Generator().manual_seed(5)
    pad = types.SimpleNamespace(**vars(inp))
    for n in ("Q", "K", "V", "Q2", "K2", "dout"):
        setattr(pad, n, torch.cat([getattr(inp, n), torch.randn(spare, inp.Q.shape[1], generator=gen)]))      # garbage rows
    loops = N + torch.arange(pad_e) % spare
    pad.bsrc, pad.bdst = torch.cat([inp.bsrc, loops]), torch.cat([inp.bdst, loops])
    pad.bcls = torch.cat([inp.bcls, torch.randint(-3, 9, (pad_e,), generator=gen)])                            # and garbage classes
    pad.sizes = list(inp.sizes) + [0, 0, spare]
    pplan = _plan(pad.sizes, pad.bsrc, pad.bdst)
    tp = _dev(pad)
    i32 = dict(dtype=torch.int32, device=DEV)
    gv = torch.cat([torch.ones(B, **i32), torch.zeros(3, **i32)])
    ev = torch.cat([torch.ones(E, **i32), torch.zeros(pad_e, **i32)])
    st = torch.zeros(2, **i32)
    pout, pden = call_fwd(tp, pad, pplan, status=st, gv=gv, ev=ev)
    assert st.tolist() == [0, 0]
    assert _bits(pout[:N], out) and _bits(pden[:N], den) and not bool(pout[N:].any()) and not bool(pden[N:].any())
    pg = call_bwd(tp, pad, pplan, pout, pden, gv=gv, ev=ev)
    for n in ("Q", "K", "V", "Q2", "K2"):
        assert _bits(pg[n][:N], grads[n]) and not bool(pg[n][N:].any()), n
    for n in ("Tr", "Tf", "gamma"):
        assert _bits(pg[n], grads[n]), n
    # an invalid edge inside a valid graph is not a bond: the result is that of the batch without it
    ev2 = torch.ones(E, **i32)
    ev2[0] = 0
    o2, _ = call_fwd(t, inp, plan, ev=ev2)
    keep = torch.ones(E, dtype=torch.bool)
    keep[0] = False
    less = types.SimpleNamespace(**vars(inp))
    less.bsrc, less.bdst, less.bcls = inp.bsrc[keep], inp.bdst[keep], inp.bcls[keep]
    o3, _ = call_fwd(_dev(less), less, _plan(inp.sizes, less.bsrc, less.bdst))
    assert _bits(o2, o3)


# ----------------------------------------------------------------------------- the modules on the reference fixtures, bond form
def build(name, cls=None, form="bonds", **over):
    from signnet_basisnet_amd import dgl_nets
    fx = FC.fixture(name)
    net = (cls or dgl_nets.TransformerNet)(FC.net_params(fx, **over))
    net.load_state_dict(fx.sd, strict=True)
    if form != "edges":
        net.full_graph_input = form
    return net.to(DEV)


def inputs(fx):
    """The MOLECULAR graph of the fixture and its bond classes (a fresh graph object per call)."""
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    ei = fx.inp["edge_index"]
    g = Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"])
    pe = fx.inp["pos_enc"].to(DEV) if "pos_enc" in fx.inp else None
    return g, fx.inp["x"].reshape(-1).to(DEV), pe, fx.inp["edge_attr"].reshape(-1).to(DEV)


def run(net, fx):
    """handle_lap on the graph the fixture's run gave it (a sign-invariant net of the reference sees the complete graph), then the base
    net in bond form on the molecular graph."""
    from signnet_basisnet_amd import dgl_nets
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    g, h, pe, e = inputs(fx)
    p = None
    if pe is not None:
        full = Graph(fx.inp["full_src"].to(DEV), fx.inp["full_dst"].to(DEV), fx.inp["sizes"])
        p = dgl_nets.handle_lap(net, pe, full)
    return net(g, h, p, e, None)[0]


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_eval_forward_matches_the_reference(name):
    fx = FC.fixture(name)
    net = build(name).eval()
    with torch.no_grad():
        y = run(net, fx)
    print(f"{name} eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, fx.out['eval/y64']):.2e}  "
          f"|ref - f64| {PU.relerr(fx.out['eval/y'], fx.out['eval/y64']):.2e}")
    close(y, fx.out["eval/y"], f"{name}: eval y", ref64=fx.out["eval/y64"])
    close(net._h_last, fx.out["eval/h_last"], f"{name}: eval h_last", ref64=fx.out["eval/h_last64"])
    net.fused_layers = False                     # one launch per op computes the same function
    with torch.no_grad():
        y1 = run(net, fx)
    close(y1, fx.out["eval/y"], f"{name}: eval y (unfused)", ref64=fx.out["eval/y64"])


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
    #  its Linear's weight gradient, as tests/test_full_graph_gpu.py does)
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
    net = build(name).train()                    # value path: train mode without autograd
    with torch.no_grad():
        yv = run(net, fx)
    print(f"{name} train y: |hip - ref| {PU.relerr(yv, y32):.2e}  |hip - f64| {PU.relerr(yv, y64):.2e}  |ref - f64| {PU.relerr(y32, y64):.2e}")
    close_conditioned(yv, y32, y64, f"{name}: train y")
    _check_buffers(net, fx, f"{name} (train, no autograd)")
    net = build(name).train()                    # differentiable path
    yg = run(net, fx)
    print(f"{name} train y (autograd): |hip - f64| {PU.relerr(yg, y64):.2e}")
    close_conditioned(yg, y32, y64, f"{name}: train y (autograd)")
    net.loss(yg, fx.inp["target"].to(DEV)).backward()
    _check_buffers(net, fx, f"{name} (train, autograd)")
    _check_gradients(net, fx, name)


def test_eval_layer_is_five_launches_and_nothing_builds_the_full_graph():
    from signnet_basisnet_amd import ops
    name = FC.FIXTURES[1]                        # (NoPE: no sign-invariant net in front)
    fx = FC.fixture(name)
    net = build(name).eval()
    with torch.no_grad():
        run(net, fx)                             # fills the eval cache (packed weights, class tables)
    rec = ops.KernelTimer()
    with rec, torch.no_grad(), ops.defer_status() as words:
        run(net, fx)
    ops.raise_deferred(words)
    names = [s[0] for s in rec.spans]
    L = len(net.layers)
    assert names.count("sn_bond_full_attention_f32") == L and names.count("sn_masked_linear_f32") == 4 * L + 3
    assert "sn_make_full_graph" not in names and "sn_full_attention_f32" not in names
    assert set(names) <= {"sn_batch_plan", "sn_embedding_sum_f32", "sn_masked_linear_f32", "sn_bond_full_attention_f32", "sn_segment_pool_f32"}, names
    i = names.index("sn_bond_full_attention_f32")
    assert names[i - 1:i + 4] == ["sn_masked_linear_f32", "sn_bond_full_attention_f32"] + ["sn_masked_linear_f32"] * 3      # five per layer
    # the edge form of the same net keeps its launches, and needs the flagged graph
    edges = build(name, form="edges").eval()
    with pytest.raises(ValueError, match=r"edata\['real'\]"):
        run(edges, fx)


# ----------------------------------------------------------------------------- the wrappers
def _small_net(seed=3, lr=1e-4):
    from signnet_basisnet_amd import dgl_nets, optim
    torch.manual_seed(seed)
    p = dict(FC.COMMON, hidden_dim=32, out_dim=32, L=2, pos_enc_dim=4, n_heads=4, readout="mean", pe_init="no_pe", lap_method="none",
             pe_aggregate="add", sign_inv_net="none", device=DEV)
    net = dgl_nets.TransformerNet(p)
    with torch.no_grad():
        for i, L in enumerate(net.layers):
            L.gamma.fill_(0.3 + 0.2 * i)
    net.full_graph_input = "bonds"
    net = net.to(DEV).train()
    return net, optim.FlatAdam(net.parameters(), lr=lr)


def _batch(sizes, seed):
    """A small shuffled molecular batch (bond order permuted) with atom ids, bond classes, a pos_enc nobody reads, and targets."""
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    src, dst, cls = FC.molecule_edges(list(sizes), seed)
    gen = torch.Generator().manual_seed(seed)
    perm = torch.randperm(src.numel(), generator=gen)
    src, dst, cls = src[perm], dst[perm], cls[perm]
    N = sum(sizes)
    return types.SimpleNamespace(g=Graph(src.to(DEV), dst.to(DEV), torch.tensor(sizes)), h=torch.randint(0, 28, (N,), generator=gen).to(DEV),
                                 p=torch.randn(N, 4, generator=gen).to(DEV), e=cls.to(DEV), t=torch.randn(len(sizes), 1, generator=gen).to(DEV),
                                 N=N, E=src.numel(), sizes=list(sizes), src=src, dst=dst)


def _grads(m):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}


def _eager(net, o, batches):
    losses, grads = [], []
    for b in batches:
        o.zero_grad()
        y, _ = net(b.g, b.h, None, b.e, None)
        loss = net.loss(y, b.t)
        loss.backward()
        grads.append(_grads(net))
        o.step()
        losses.append(loss.item())
    return losses, grads


BATCHES = ((7, 12, 3, 20, 9), (15, 4, 11, 1, 8, 6))          # 51 and 45 nodes: different shapes, one bucket of the granule below
GRANULE = dict(N=64, E=128)


def test_bucketed_step_follows_the_eager_bond_form_step(monkeypatch):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    batches = [_batch(BATCHES[0], 1), _batch(BATCHES[1], 2)]
    m1, o1 = _small_net()
    eager, ge = _eager(m1, o1, batches)
    noisy, gn = eager, ge                         # (a NoPE net reads no pos_enc: the eager step's sensitivity to it is exactly 0)

    def bucketed(noisy_padding):
        pack = ops.bucket_pack_dgl
        gen = torch.Generator(device=DEV)

        def noisy_pack(g, h, p, e, snorm_n, target, out):
            r = pack(g, h, p, e, snorm_n, target, out)
            N, E, B = (int(v) for v in out.counts.tolist())
            gen.manual_seed(N)
            out.h[N:] = torch.randint(0, 28, out.h[N:].shape, generator=gen, device=DEV)
            out.e[E:] = torch.randint(0, 4, out.e[E:].shape, generator=gen, device=DEV)
            out.p[N:] = torch.randn(out.p[N:].shape, generator=gen, device=DEV)
            out.target[B:] = torch.randn(out.target[B:].shape, generator=gen, device=DEV)
            return r
        if noisy_padding:
            monkeypatch.setattr(ops, "bucket_pack_dgl", noisy_pack)
        m, o = _small_net()
        s = DGLBucketedStep(m, o, max_graphs=8, granule=GRANULE)
        assert s.bucket_of(batches[0].g, batches[0].h) == s.bucket_of(batches[1].g, batches[1].h)
        losses, grads = [], []
        for b in batches:
            losses.append(s.step(b.g, b.h, b.p, b.e, None, b.t).item())
            grads.append(_grads(m))
        torch.cuda.synchronize()
        assert s.captures == 1 and s.hits == 1
        s.check()
        s.release()
        return losses, grads, o.flat_p.clone()

    padded, gp, p0 = bucketed(False)
    print("losses: eager", eager, "padded", padded)
    BC.close_losses(eager, noisy, padded)
    BC.close_grads(ge[0], gn[0], gp[0])
    # other garbage in the padding region: not a bit of the losses, the gradients or the parameters moves
    padded2, gp2, p1 = bucketed(True)
    assert padded == padded2 and torch.equal(p0, p1)
    for k in range(2):
        for n in gp[k]:
            assert (gp[k][n] is None) == (gp2[k][n] is None) and (gp[k][n] is None or torch.equal(gp[k][n], gp2[k][n])), n


def test_step_from_a_graph_store_equals_step_on_its_collated_batch():
    from signnet_basisnet_amd import data
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    samples = []
    for i, n in enumerate(BATCHES[0] + BATCHES[1]):
        b = _batch((n,), 20 + i)
        samples.append((Graph(b.src, b.dst, torch.tensor([n])), b.h.cpu(), b.p.cpu(), b.e.cpu(), None, b.t.cpu().reshape(-1)))
    store = data.DGLGraphStore.from_samples(samples, DEV)
    idx = [[0, 3, 5, 9, 2], [10, 1, 4, 7, 8, 6]]
    runs = []
    for from_store in (False, True):
        m, o = _small_net()
        s = DGLBucketedStep(m, o, max_graphs=8, granule=GRANULE)
        losses = []
        for ix in idx:
            if from_store:
                losses.append(s.step_from(store, ix).item())
            else:
                g, h, p, e, sn, t = store.collate(ix)
                losses.append(s.step(g, h, p, e, sn, t).item())
        torch.cuda.synchronize()
        assert s.captures == 1 and s.hits == 1
        s.check()
        runs.append((losses, _grads(m), o.flat_p.clone()))
        s.release()
    (l0, g0, p0), (l1, g1, p1) = runs
    assert l0 == l1 and torch.equal(p0, p1)
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None) and (g0[n] is None or torch.equal(g0[n], g1[n])), n


def test_graphed_forward_replays_the_eager_eval_forward():
    from signnet_basisnet_amd import serving
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    net, _ = _small_net()
    net.eval()
    a = _batch(BATCHES[0], 1)
    # a second batch of the same shape: the same graphs, other atoms and bond classes, the bonds in another order
    gen = torch.Generator().manual_seed(9)
    perm = torch.randperm(a.E, generator=gen)
    b = types.SimpleNamespace(**vars(a))
    b.g = Graph(a.src[perm].to(DEV), a.dst[perm].to(DEV), torch.tensor(a.sizes))
    b.h, b.e = torch.randint(0, 28, (a.N,), generator=gen).to(DEV), torch.randint(0, 4, (a.E,), generator=gen).to(DEV)
    with torch.no_grad():
        ya, yb = net(a.g, a.h, None, a.e, None)[0].clone(), net(b.g, b.h, None, b.e, None)[0].clone()
    assert not torch.equal(ya, yb)
    fwd = serving.GraphedDGLForward(net, a.g, a.h, None, a.e)
    assert _bits(fwd(), ya)
    assert _bits(fwd(b.g, b.h, None, b.e), yb)
    fwd.check()
    assert _bits(fwd(a.g, a.h, None, a.e), ya)
    bad = a.e.clone()
    bad[2] = 4                                   # a bond class outside embedding_e
    fwd(a.g, a.h, None, bad)
    with pytest.raises(IndexError):
        fwd.check()
    fwd(a.g, a.h, None, a.e)
    fwd.check()
    # the form is part of the recording
    net.full_graph_input = "edges"
    with pytest.raises(RuntimeError, match="full_graph_input changed"):
        fwd(a.g, a.h, None, a.e)
    net.full_graph_input = "bonds"
    assert _bits(fwd(a.g, a.h, None, a.e), ya)


def test_refusals_stay_for_the_edge_form_and_a_changed_form_raises():
    from signnet_basisnet_amd import data, ops, serving
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    net, o = _small_net()
    b = _batch(BATCHES[0], 1)
    s = DGLBucketedStep(net, o, max_graphs=8, granule=GRANULE)
    net.full_graph_input = "edges"
    with pytest.raises(RuntimeError, match="full_graph_input changed"):
        s.step(b.g, b.h, b.p, b.e, None, b.t)
    assert s.captures == 0
    with pytest.raises(NotImplementedError, match="DGLBucketedStep does not carry the edge flag"):
        DGLBucketedStep(net, o, max_graphs=8)
    with pytest.raises(NotImplementedError, match="GraphedDGLForward does not carry the edge flag"):
        serving.GraphedDGLForward(net.eval(), b.g, b.h, None, b.e)
    net.train()
    net.full_graph_input = "bonds"
    full, ef = ops.make_full_graph(b.g, b.e)
    with pytest.raises(NotImplementedError, match="DGLBucketedStep does not carry the edge flag"):
        s.step(full, b.h, b.p, ef, None, b.t)
    with pytest.raises(NotImplementedError, match="DGLGraphStore does not carry the edge flag"):
        data.DGLGraphStore.from_batch((full, b.h, b.p, ef, None), b.t, DEV)
    assert s.captures == 0
