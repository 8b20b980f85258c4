"""-m gpu: every dispatch branch of the adjoint kernels (csrc/backward.hip, csrc/attention16.hip, csrc/gated.hip) against float64.

One parametrized test per op over its table in tests/adjoint_cases.py.  A row runs the HIP path, the float32 CPU autograd and the float64
CPU autograd of the restatement on the same inputs and the same seeded cotangents, and checks the forward value and every input
gradient with the project's attribution rule (parity_util.attributed):

    |hip - f64| <= max(REL * scale, 2 |cpu32 - f64| + ATTR * scale),   scale = max |f64|

Only the two CPU evaluations enter a bound.  tests/test_adjoint_cases_cpu.py asserts, without a GPU, that every row reaches the kernel
it names, that float32 itself is within REL there, and that no ReLU decision sits within rounding of zero.
"""
import pytest
import torch

import adjoint_cases as AC
import parity_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ids(cases):
    return [c.id for c in cases]


def offset_view(t):
    """a contiguous device copy of t that starts 4 bytes into a 16-byte aligned buffer"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def to_dev(t, offset=False):
    return (offset_view(t) if offset else t.to(DEV)).detach().requires_grad_(True)


def nv_dev(aux):
    return None if aux.get("nv") is None else aux["nv"].to(DEV)


def backward(outs, offset=False):
    cots = [AC.cotangent(i, o.shape).float() for i, o in enumerate(outs)]
    torch.autograd.backward(outs, [offset_view(c) if offset else c.to(DEV) for c in cots])


def accept(hip, r32, r64, what, factor=None):
    """parity_util.attributed; `factor` (a row's case-specific bound, stated at the row with its measurements) replaces the 2 of the rule"""
    if factor is None:
        return PU.attributed(hip, r32, r64, what)
    hip, r32, r64 = hip.detach().cpu().double(), r32.detach().double(), r64.detach().double()
    scale = max(r64.abs().max().item(), 1e-300)
    e_hip, e_cpu = (hip - r64).abs().max().item(), (r32 - r64).abs().max().item()
    assert e_hip <= max(PU.REL * scale, factor * e_cpu + PU.ATTR * scale), \
        f"{what}: |hip - f64| {e_hip / scale:.2e} vs |cpu32 - f64| {e_cpu / scale:.2e} (relative to max |f64| {scale:.3e}; allowed {factor:g}x)"
    return e_hip / scale, e_cpu / scale


def check_case(case, hip, leaves=None, aux=None):
    """hip(case, aux, leaves) -> (outputs, gradients) on the device; compared with the restatement in both CPU precisions"""
    op = AC.OPS[case.op]
    if leaves is None:
        leaves, aux = op.gen(case.p)
    outs, grads = hip(case, aux, leaves)
    o64, g64 = AC.reference(case, AC.F64, leaves, aux)
    o32, g32 = AC.reference(case, AC.F32, leaves, aux)
    assert len(outs) == len(o64) and len(grads) == len(g64)
    worst = (0.0, 0.0, "")
    for what, h, a32, a64 in [(f"output {i}", *t) for i, t in enumerate(zip(outs, o32, o64))] + \
                             [(f"grad {i}", *t) for i, t in enumerate(zip(grads, g32, g64))]:
        assert h is not None, f"{case.id} {what}: no gradient"
        assert tuple(h.shape) == tuple(a64.shape), f"{case.id} {what}: shape {tuple(h.shape)} vs {tuple(a64.shape)}"
        e = accept(h, a32, a64, f"{case.id} [{case.branch}] {what}", case.factor)
        worst = max(worst, (*e, what))
    print(f"\n{case.id}: worst |hip - f64| {worst[0]:.2e}, |cpu32 - f64| there {worst[1]:.2e} ({worst[2]})", end="")


def autograd_case(fn, offset=False):
    def hip(case, aux, leaves):
        xs = [to_dev(t, offset and t.dim() == 2) for t in leaves]
        outs = fn(case.p, aux, *xs)
        backward(outs, offset)
        return outs, [x.grad for x in xs]
    return hip


# ---------------------------------------------------------------------------- set attention
@pytest.mark.parametrize("case", AC.ATTENTION, ids=ids(AC.ATTENTION))
def test_set_attention(case):
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import ops
    p = case.p
    leaves, aux = AC.attention_gen(p)
    pm = None
    if p["drop"]:
        torch.manual_seed(7)
        pm = ops.attention_dropout_mask(p["N"], p["K"], p["H"], 0.25, DEV)
        aux["pm"] = pm.cpu()
        vals = set(aux["pm"].unique().tolist())
        assert vals <= {0.0, aux["pm"].max().item()} and (not aux["pm"].any() or abs(aux["pm"].max().item() - 1 / 0.75) < 1e-6)
    nvd = nv_dev(aux)
    check_case(case, autograd_case(lambda p, aux, q, k, v: (AG.set_attention(q, k, v, p["N"], p["K"], p["H"], nvd, pm),), p["offset"]),
               leaves, aux)


def test_set_attention_backward_rejects_more_than_160k_of_lds_before_any_launch():
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    r = AC.ATTENTION_REJECTED
    N, K, H, dk = r["N"], r["K"], r["H"], r["dk"]
    q, k, v, g = (torch.randn(N * K, H * dk, device=DEV) for _ in range(4))
    dq, dk_, dv = (torch.full_like(q, 7.0) for _ in range(3))
    with pytest.raises(RuntimeError, match="LDS"):
        check(lib().sn_set_attention_bwd_f32(ptr(q), ptr(k), ptr(v), ptr(g), N, K, H, dk, None, None, ptr(dq), ptr(dk_), ptr(dv), stream()),
              "sn_set_attention_bwd_f32")
    torch.cuda.synchronize()
    for t in (dq, dk_, dv):
        assert bool((t == 7.0).all())
    test_set_attention(AC.ATTENTION[2])          # the entry point serves the next call


# ---------------------------------------------------------------------------- LayerNorm
def _layernorm_hip(case, aux, leaves):
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd._lib import lib
    p = case.p
    nvd, per = nv_dev(aux), (2 if p["res"] else 1)
    xs = [to_dev(t, p["offset"] and t.dim() == 2) for t in leaves]
    gamma, beta = xs[-2:]
    L, calls = lib(), []
    if p["acc"]:          # parameters whose .grad the optimiser owns (optim.FlatAdam): the adjoint adds into them
        for t in (gamma, beta):
            t.grad = torch.zeros_like(t)
            t._sn_direct_grad = True
        orig = L.sn_masked_layernorm_bwd_acc_f32

        def counted(*a):
            calls.append(1)
            return orig(*a)
        L.sn_masked_layernorm_bwd_acc_f32 = counted
    try:
        outs = []
        for i in range(aux["npass"]):          # one backward pass per forward, nothing zeroed in between
            y = AG.masked_layernorm(xs[i * per], xs[i * per + 1] if p["res"] else None, gamma, beta, aux["eps"], nvd, aux["K"])
            y.backward(AC.cotangent(i, y.shape).float().to(DEV))
            outs.append(y)
    finally:
        if p["acc"]:
            L.sn_masked_layernorm_bwd_acc_f32 = orig
    assert len(calls) == (aux["npass"] if p["acc"] else 0)
    return outs, [x.grad for x in xs]


@pytest.mark.parametrize("case", AC.LAYERNORM, ids=ids(AC.LAYERNORM))
def test_masked_layernorm(case):
    check_case(case, _layernorm_hip)


# ---------------------------------------------------------------------------- Linear / weight gradient
@pytest.mark.parametrize("case", AC.LINEAR, ids=ids(AC.LINEAR))
def test_linear(case):
    from signnet_basisnet_amd import autograd as AG
    leaves, aux = AC.linear_gen(case.p)
    nvd = nv_dev(aux)
    check_case(case, autograd_case(lambda p, aux, x, W, *b: (AG.linear(x, W, b[0] if b else None, nvd, aux["K"], relu=p["relu"]),)), leaves, aux)


def _wgrad_raw_hip(case, aux, leaves):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    p = case.p
    (d_in, d_out), R = p["d"], p["R"]
    X, DY = (t.to(DEV) for t in leaves)
    x, dy = X[:, aux["cx"]:aux["cx"] + d_in], DY[:, aux["cy"]:aux["cy"] + d_out]
    n = d_in * d_out
    buf = torch.full((n + 8 + d_out,), 7.0, dtype=torch.float32, device=DEV)
    dW = buf[:n].view(d_out, d_in)
    db = (buf[n + 8:] if p["sep_db"] else buf[n:n + d_out]) if p["want_bias"] else None
    scratch = torch.empty(int(lib().sn_linear_wgrad_scratch_floats(R, d_in, d_out)), dtype=torch.float32, device=DEV)
    check(lib().sn_linear_wgrad_f32(ptr(x), p["ldx"], ptr(dy), p["ldy"], R, d_in, d_out, ptr(nv_dev(aux)), aux["K"], ptr(dW), ptr(db),
                                    ptr(scratch), stream()), "sn_linear_wgrad_f32")
    if p["sep_db"]:
        assert bool((buf[n:n + 8] == 7.0).all())
    return (dW,) + ((db,) if p["want_bias"] else ()), []


@pytest.mark.parametrize("case", AC.WGRAD_RAW, ids=ids(AC.WGRAD_RAW))
def test_linear_wgrad_strides_and_separate_bias(case):
    check_case(case, _wgrad_raw_hip)


# ---------------------------------------------------------------------------- BatchNorm + activation
def _bn_module(C):
    return torch.nn.BatchNorm1d(C, eps=AC.BN_EPS).to(DEV).train()


def _bn_act_fn(p, aux, z, gamma, beta, *rr):
    from signnet_basisnet_amd import autograd as AG
    bn = _bn_module(p["C"])
    bn.weight, bn.bias = torch.nn.Parameter(gamma.detach()), torch.nn.Parameter(beta.detach())
    y = AG._BnAct.apply(z, gamma, beta, rr[0] if rr else None, bn, nv_dev(aux), aux["K"], p["relu"])      # the leaves' .grad are filled
    assert int(bn.num_batches_tracked) == 1
    return (y,)


def _bn_act_strided_hip(case, aux, leaves):
    """sn_bn_act_bwd_f32 on column slices of wider matrices (ldz, ldd, ldo > C); statistics and forward from the contiguous op"""
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    p = case.p
    C_, R = p["C"], p["R"]
    ldz, ldd, ldo = p["ld"]
    z, gamma, beta = (t.to(DEV) for t in leaves)
    nvd = nv_dev(aux)
    bn = _bn_module(C_)
    bn.weight, bn.bias = torch.nn.Parameter(gamma), torch.nn.Parameter(beta)
    mean, _, rstd, scale, shift, count = ops.bn_train_stats(z, bn, nvd, aux["K"])
    y = ops.masked_affine(z, nvd, aux["K"], scale=scale, shift=shift, relu=p["relu"])
    Z, DY, DZ = (torch.full((R, ld), 7.0, dtype=torch.float32, device=DEV) for ld in (ldz, ldd, ldo))
    Z[:, :C_] = z
    DY[:, :C_] = AC.cotangent(0, (R, C_)).float().to(DEV)
    sums = torch.empty(2 * C_, dtype=torch.float32, device=DEV)
    scratch = torch.empty(int(lib().sn_bn_act_bwd_scratch_floats(R, C_)), dtype=torch.float32, device=DEV)
    check(lib().sn_bn_act_bwd_f32(ptr(Z), ldz, ptr(DY), ldd, R, C_, ptr(nvd), aux["K"], ptr(mean), ptr(rstd), ptr(scale), ptr(shift),
                                  int(p["relu"]), ptr(count), ptr(sums), ptr(DZ), ldo, ptr(scratch), stream()), "sn_bn_act_bwd_f32")
    assert bool((DZ[:, C_:] == 7.0).all())
    return (y,), [DZ[:, :C_], sums[C_:], sums[:C_]]


@pytest.mark.parametrize("case", AC.BN_ACT, ids=ids(AC.BN_ACT))
def test_bn_act(case):
    check_case(case, _bn_act_strided_hip if case.p["ld"] else autograd_case(_bn_act_fn))


def _linear_bn_act_fn(p, aux, x, W, gamma, beta, *rr):
    from signnet_basisnet_amd import autograd as AG
    bn = _bn_module(p["C"])
    bn.weight, bn.bias = torch.nn.Parameter(gamma.detach()), torch.nn.Parameter(beta.detach())
    return (AG._LinearBnAct.apply(x, W, aux["b"].to(DEV), gamma, beta, rr[0] if rr else None, bn, nv_dev(aux), aux["K"], p["relu"]),)


@pytest.mark.parametrize("case", AC.LINEAR_BN_ACT, ids=ids(AC.LINEAR_BN_ACT))
def test_linear_bn_act(case):
    check_case(case, autograd_case(_linear_bn_act_fn))


# ---------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("case", AC.EMBEDDING, ids=ids(AC.EMBEDDING))
def test_embedding_sum(case):
    from signnet_basisnet_amd import autograd as AG
    leaves, aux = AC.embedding_gen(case.p)
    idx_d = aux["idx"].to(DEV)
    runs = []

    def hip(case, aux, leaves):
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        o, g = autograd_case(lambda p, aux, *tables: (AG.embedding_sum(idx_d, list(tables), status),))(case, aux, leaves)
        assert int(status.item()) == (1 if case.p["oor"] else 0)          # an id outside its table: reported, contributes nothing
        runs.append(g)
        return o, g
    check_case(case, hip, leaves, aux)
    hip(case, aux, leaves)
    for a, b in zip(*runs):                                               # no atomics: bitwise reproducible
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------- aggregations
def _plans(ei, batch):
    from signnet_basisnet_amd import ops
    B = int(batch.max()) + 1
    plan = ops.build_plan(batch.to(DEV), ei.to(DEV), B, 0)
    return plan, ops.build_plan(batch.to(DEV), ei.flip(0).contiguous().to(DEV), B, 0)


@pytest.mark.parametrize("case", AC.GATED, ids=ids(AC.GATED))
def test_gated_aggregate(case):
    from signnet_basisnet_amd import autograd as AG
    leaves, aux = AC.gated_gen(case.p)
    plan, rplan = _plans(aux["ei"], aux["batch"])
    deg = torch.bincount(aux["ei"][1], minlength=aux["batch"].numel())
    assert int(deg.max()) >= 39 and int((deg == 0).sum()) > 0 and int(aux["batch"].max()) > 0

    def fn(p, aux, Ah, Bh, Dh, Eh, Ce):
        if p["blocked"]:
            Cc = p["C"]
            X = torch.cat([Ah, Bh, Dh, Eh], 1)
            Ah, Bh, Dh, Eh = (X[:, i * Cc:(i + 1) * Cc] for i in range(4))
        return AG.gated_aggregate(Ah, Bh, Dh, Eh, Ce, plan, rplan)
    check_case(case, autograd_case(fn), leaves, aux)


@pytest.mark.parametrize("case", AC.SLOT_SUM, ids=ids(AC.SLOT_SUM))
def test_slot_sum_and_broadcast(case):
    from signnet_basisnet_amd import autograd as AG
    check_case(case, autograd_case(lambda p, aux, x: (AG.slot_sum(x, p["N"], p["K"], nv_dev(aux)),)))


@pytest.mark.parametrize("case", AC.MASKED_ADD, ids=ids(AC.MASKED_ADD))
def test_masked_add(case):
    from signnet_basisnet_amd import autograd as AG
    check_case(case, autograd_case(lambda p, aux, a, b: (AG.masked_add(a, b, nv_dev(aux), aux["K"]),)))


def _segment_plan(batch):
    return _plans(torch.zeros(2, 0, dtype=torch.int64), batch)[0]


@pytest.mark.parametrize("case", AC.SEGMENT_POOL, ids=ids(AC.SEGMENT_POOL))
def test_segment_pool_and_broadcast(case):
    from signnet_basisnet_amd import autograd as AG
    plan = _segment_plan(AC.segment_batch())
    check_case(case, autograd_case(lambda p, aux, h: (AG.segment_pool(h, plan, p["mode"]),)))


@pytest.mark.parametrize("case", AC.SEGMENT_BCAST_ADD, ids=ids(AC.SEGMENT_BCAST_ADD))
def test_segment_bcast_add(case):
    from signnet_basisnet_amd import autograd as AG
    plan = _segment_plan(AC.segment_batch())
    check_case(case, autograd_case(lambda p, aux, x1, x2: (AG.segment_bcast_add(x1, x2, plan, relu=p["relu"]),)))


@pytest.mark.parametrize("case", AC.RELU_BWD, ids=ids(AC.RELU_BWD))
def test_relu_bwd(case):
    from signnet_basisnet_amd import autograd as AG
    check_case(case, lambda case, aux, leaves: ((AG.relu_bwd(aux["y"].to(DEV), leaves[0].to(DEV), nv_dev(aux), aux["K"]),), []))


@pytest.mark.parametrize("case", AC.DOT, ids=ids(AC.DOT))
def test_dot(case):
    from signnet_basisnet_amd import autograd as AG
    check_case(case, lambda case, aux, leaves: ((AG.dot(leaves[0].to(DEV), leaves[1].to(DEV)),), []))


# ---------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("case", AC.ADAM, ids=ids(AC.ADAM))
def test_adam_step(case):
    """One step from the float64 state of step t - 1: the UPDATE p_new - p_old and both moments against the float64 step written out in
    adjoint_cases.adam_f64, with torch.optim.Adam in float32 as the fp32 reference."""
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    p = case.p
    lr, b1, b2, eps = AC.ADAM_HYPER[p["hyper"]]
    par, grad, m, v = AC.adam_gen(p)
    u64, m64, v64 = AC.adam_f64(p, par, grad, m, v)
    u32, m32, v32 = AC.adam_torch32(p, par, grad, m, v)
    q = torch.nn.Parameter(par.to(DEV))
    md, vd, gd = m.float().to(DEV), v.float().to(DEV), grad.to(DEV)
    if p["gs"] == 1.0:
        opt = optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=p["wd"])
        opt.t, opt.state[q], q.grad = p["step"] - 1, (md, vd), gd
        opt.step()
        assert opt.t == p["step"]
    else:                    # the gradient scale is FlatAdam's (1 / world size): the entry point directly
        check(lib().sn_adam_step_f32(ptr(q), ptr(gd), ptr(md), ptr(vd), q.numel(), lr, b1, b2, eps, p["wd"], p["step"], p["gs"], stream()),
              "sn_adam_step_f32")
    u_hip = q.detach().cpu().double() - par.double()
    worst = []
    for what, h, a32, a64 in (("update", u_hip, u32, u64), ("m", md, m32, m64), ("v", vd, v32, v64)):
        e_hip, e_cpu = (h.detach().cpu().double() - a64).abs().max().item(), (a32.double() - a64).abs().max().item()
        worst.append(f"{what} {e_hip / a64.abs().max().item():.2e} (cpu32 {e_cpu / a64.abs().max().item():.2e})")
    print(f"\n{case.id}: |hip - f64| / max|f64|: " + ", ".join(worst), end="")
    for what, h, a32, a64 in (("update", u_hip, u32, u64), ("m", md, m32, m64), ("v", vd, v32, v64)):
        accept(h, a32, a64, f"{case.id} {what}", case.factor)
