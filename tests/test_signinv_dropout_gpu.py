"""-m gpu: train-mode dropout in the sign-invariant encoders of the DGL tree (signnet_basisnet_amd.dropout_signinv).

  kernel     sn_affine_dropout_f32 through the C ABI on buffers with NaN and sentinel guards (tests/test_dropout_gpu.py's Placed): the
             kept set is numpy's (tests/dropout_cases.keep_mask and the row mask), the values equal ops.dropout(ops.masked_affine(...))
             bit for bit on each of the three paths, nothing outside the output is written
  autograd   bn_drop against bn_act followed by dropout: output, gradients and running statistics bit for bit
  encoders   the four encoders on the reference's fixtures (tests/golden/ds_dropout_*.npz): output, running statistics and every
             parameter gradient under the rules of the p = 0 tests of the same family — GIN encoders: assert_close(5e-4, 5e-5) for the
             output (tests/test_dgl_basisnet_gpu.py) and 2e-3 of the tensor + 1e-5 of the largest gradient against float64
             (tests/test_training_gpu.py); gcn / transformer: parity_util.close / close_conditioned and attributed
             (tests/test_deepsigns_variants_gpu.py) — with the fixture's float64 run as the yardstick
  identity   eval at p > 0 and train at p = 0 are the base classes, bit for bit and launch for launch
  launches   the recorded entry points of one differentiable forward + backward, derived from the site table
  steps      masks move with the step, repeat after seeding, belong to their own forward; the net's seed reaches the encoder
  captured   DGLBucketedStep follows the eager steps from the same seed, draws fresh masks per replay, leaves the step words alone
Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import dropout_cases as DC
import golden_util as G
import parity_util as PU
import signinv_dropout_cases as SC
from parity_util import attributed, close, close_conditioned
from test_dropout_gpu import PAD, SENT, Placed, _state  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _nothing_is_launched_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, the rest of the grid is not run: {e}", returncode=3)


@pytest.fixture(scope="module")
def L():
    from signnet_basisnet_amd import _lib
    return _lib


# ----------------------------------------------------------------------------- the kernel
def _kcases():
    out = []
    for i, (R, C, ld) in enumerate(SC.SHAPES):
        p = SC.PS[i % 3]
        none = R == 0
        out.append((f"{R}x{C}-plain-p{p}", R, C, ld, False, 0, p, "none" if none else ("row" if C % 4 == 0 else "flat")))
        out.append((f"{R}x{C}-offset-p{p}", R, C, ld, True, 0, p, "none" if none else "scalar"))
        if C % 4 and R:
            out.append((f"{R}x{C}-strided-p{p}", R, C, (ld or C) + 3, False, 0, p, "scalar"))
    for base in SC.BASES[1:]:          # 2^34 - 6 crosses into the counter's high word at its 7th element
        out.append((f"2x8-base{base}", 2, 8, None, False, base, 0.5, "scalar"))
    out.append(("2x8-base8", 2, 8, None, False, 8, 0.5, "row"))
    out.append(("2x8-base2^34", 2, 8, None, False, 1 << 34, 0.5, "row"))
    out.append(("3x5-base2^34", 3, 5, None, False, 1 << 34, 0.5, "flat"))
    for p in SC.PS:
        out.append((f"33x77-p{p}", 33, 77, None, False, 0, p, "flat"))
        out.append((f"5x68-ld72-p{p}", 5, 68, 72, False, 0, p, "row"))
        out.append((f"33x77-offset-p{p}", 33, 77, None, True, 0, p, "scalar"))
    return out


KCASES = _kcases()


def _kernel_case(L, R, C, ld, offset, base, p, want, affine, masked, scale_off=False):
    from signnet_basisnet_amd import ops
    what = f"{R}x{C} ld={ld} off={offset} base={base} p={p} affine={affine} masked={masked}"
    g = torch.Generator().manual_seed(R * 1000 + C)
    x = torch.rand(R, C, generator=g) + 0.5                       # x, scale, shift > 0: fma(x, scale, shift) is never 0
    X = Placed(R, C, ld or C, offset, float("nan"), x)
    Y = Placed(R, C, ld or C, offset, SENT)
    sc = sh = None
    if affine:
        buf = torch.empty(2, C + 8, device=DEV)
        o = 1 if scale_off else 0
        sc, sh = buf[0, o:o + C], buf[1, o:o + C]
        sc.copy_(torch.rand(C, generator=g) + 0.5)
        sh.copy_(torch.rand(C, generator=g) + 0.25)
    nv_np = SC.nvalid_for(R) if masked else None
    nv = torch.from_numpy(nv_np).to(DEV) if masked else None
    state = _state(SC.SEED, SC.STEP)
    got_path = "none" if R == 0 else SC.path(C, X.ld, Y.ld, base, X.ptr, Y.ptr, sc.data_ptr() if affine else 0, sh.data_ptr() if affine else 0)
    assert got_path == want, f"{what}: the case reaches {got_path}, not {want}"
    thr, ps = DC.threshold_of(p), float(DC.scale_of(p))
    rc = L.lib().sn_affine_dropout_f32(X.ptr, X.ld, R, C, L.ptr(nv), SC.K_MASK if masked else 0, L.ptr(sc), L.ptr(sh), thr, ps,
                                       state.data_ptr(), SC.SITE, base, Y.ptr, Y.ld, L.stream())
    L.check(rc, "sn_affine_dropout_f32")
    torch.cuda.synchronize()
    Y.assert_sentinels(what)
    if R == 0:
        return
    y = Y.v.contiguous()
    keep = DC.keep_mask(R, C, p, SC.SEED, SC.STEP, SC.SITE, base)
    if masked:
        keep = keep & SC.rowvalid(R, nv_np)[:, None]
    got = y.cpu().numpy() != 0.0
    assert (got == keep).all(), f"{what}: {int((got != keep).sum())} elements of the kept set differ from numpy's"
    xc = x.to(DEV)
    mid = ops.masked_affine(xc, nv, SC.K_MASK if masked else 0, scale=sc.contiguous() if affine else None,
                            shift=sh.contiguous() if affine else None) if (affine or masked) else xc
    ref = ops.dropout(mid, p, state, SC.SITE, base=base)
    assert torch.equal(y.view(torch.int32), ref.view(torch.int32)), f"{what}: not the composition's bits"
    # the step word moves on the device; the launch's host arguments do not
    state[1:].add_(1)
    rc = L.lib().sn_affine_dropout_f32(X.ptr, X.ld, R, C, L.ptr(nv), SC.K_MASK if masked else 0, L.ptr(sc), L.ptr(sh), thr, ps,
                                       state.data_ptr(), SC.SITE, base, Y.ptr, Y.ld, L.stream())
    L.check(rc, "sn_affine_dropout_f32")
    keep2 = DC.keep_mask(R, C, p, SC.SEED, SC.STEP + 1, SC.SITE, base)
    if masked:
        keep2 = keep2 & SC.rowvalid(R, nv_np)[:, None]
    assert ((Y.v.contiguous().cpu().numpy() != 0.0) == keep2).all(), f"{what}: the next step's mask"


@pytest.mark.parametrize("case", KCASES, ids=[c[0] for c in KCASES])
def test_affine_dropout_case(L, case):
    _, R, C, ld, offset, base, p, want = case
    for affine in (True, False):
        for masked in (True, False):
            _kernel_case(L, R, C, ld, offset, base, p, want, affine, masked)


def test_every_path_is_reached_and_a_flat_group_straddles_a_valid_and_an_invalid_row():
    assert {c[7] for c in KCASES} == {"row", "flat", "scalar", "none"}
    R, C = 37 * 3, 67
    assert any(c[1:3] == (R, C) and c[7] == "flat" for c in KCASES)
    valid = SC.rowvalid(R, SC.nvalid_for(R))
    first, last = (np.arange(0, R * C - 3, 4)) // C, (np.arange(0, R * C - 3, 4) + 3) // C
    assert int(((first != last) & (valid[first] != valid[last])).sum()) > 10


def test_scale_off_a_16_byte_boundary_takes_the_flat_path(L):
    _kernel_case(L, 7, 4, None, False, 0, 0.5, "flat", True, True, scale_off=True)
    _kernel_case(L, 5, 68, 72, False, 0, 0.5, "scalar", True, False, scale_off=True)


@pytest.mark.parametrize("shape,want", [(SC.BIG, "row"), (SC.BIG_FLAT, "flat")], ids=["row", "flat"])
def test_more_groups_than_the_grid_cap(L, shape, want):
    assert SC.n_groups(*shape, 0, want) > SC.MAX_BLOCKS * 256
    _kernel_case(L, shape[0], shape[1], None, False, 0, 0.5, want, True, True)


def test_more_groups_than_the_grid_cap_scalar(L):
    assert SC.n_groups(*SC.BIG, 0, "scalar") > SC.MAX_BLOCKS * 256
    _kernel_case(L, SC.BIG[0], SC.BIG[1], None, True, 0, 0.5, "scalar", True, True)


def test_bad_arguments_are_refused_on_the_host(L):
    lib = L.lib()
    x, y = torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV)
    s, st = torch.ones(8, device=DEV), _state(1, 1)
    nv = torch.ones(4, dtype=torch.int32, device=DEV)
    ok = [x.data_ptr(), 8, 4, 8, None, 0, s.data_ptr(), s.data_ptr(), 1 << 31, 2.0, st.data_ptr(), 7, 0, y.data_ptr(), 8, L.stream()]
    assert lib.sn_affine_dropout_f32(*ok) == 0
    for i, v in ((0, None), (13, None), (10, None), (1, 7), (14, 7), (3, 0), (12, -1), (7, None), (0, x.data_ptr() + 2), (10, st.data_ptr() + 4)):
        a = list(ok)
        a[i] = v
        assert lib.sn_affine_dropout_f32(*a) == -1 and b"sn_affine_dropout_f32" in lib.sn_last_error(), (i, v)
    a = list(ok)
    a[4] = nv.data_ptr()                        # nvalid without K
    assert lib.sn_affine_dropout_f32(*a) == -1
    torch.cuda.synchronize()


def test_ops_affine_dropout_conventions():
    from signnet_basisnet_amd import ops
    x = torch.rand(9, 5, device=DEV) + 0.5
    sc, sh = torch.rand(5, device=DEV) + 0.5, torch.rand(5, device=DEV)
    snap = _state(3, 4)
    rec = ops.KernelTimer()
    with rec:
        y0 = ops.affine_dropout(x, sc, sh, 0.0, snap, SC.SITE)
    assert [s[0] for s in rec.spans] == ["sn_masked_affine_f32"] and torch.equal(y0, ops.masked_affine(x, scale=sc, shift=sh))
    assert not bool(ops.affine_dropout(x, sc, sh, 1.0, snap, SC.SITE).any())
    with pytest.raises(ValueError, match="between 0 and 1"):
        ops.affine_dropout(x, sc, sh, 1.5, snap, SC.SITE)
    with pytest.raises(ValueError, match="go together"):
        ops.affine_dropout(x, sc, None, 0.5, snap, SC.SITE)
    y = ops.affine_dropout(x, None, None, 0.5, snap, SC.SITE)
    assert torch.equal(y, ops.dropout(x, 0.5, snap, SC.SITE))


# ----------------------------------------------------------------------------- autograd.bn_drop
@pytest.mark.parametrize("R,C,masked", [(111, 67, True), (24, 8, False), (33, 77, False), (30, 68, True)])
def test_bn_drop_is_bn_act_then_dropout_bit_for_bit(R, C, masked):
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import ops
    g = torch.Generator().manual_seed(R + C)
    z0, cot = torch.randn(R, C, generator=g).to(DEV), torch.randn(R, C, generator=g).to(DEV)
    nv = torch.from_numpy(SC.nvalid_for(R)).to(DEV) if masked else None
    K = SC.K_MASK if masked else 0
    snap = _state(11, 3)
    res = []
    for fused in (False, True):
        bn = torch.nn.BatchNorm1d(C)
        with torch.no_grad():
            bn.weight.copy_(1 + 0.2 * torch.randn(C, generator=torch.Generator().manual_seed(1)))
            bn.bias.copy_(0.1 * torch.randn(C, generator=torch.Generator().manual_seed(2)))
        bn = bn.to(DEV).train()
        z = z0.clone().requires_grad_(True)
        rec = ops.KernelTimer()
        with rec:
            y = AG.bn_drop(z, bn, 0.5, snap, SC.SITE, nv, K) if fused else AG.dropout(AG.bn_act(z, bn, nv, K, relu=False), 0.5, snap, SC.SITE)
            n_fwd = len(rec.spans)
            (y * cot).sum().backward()
        names = [s[0] for s in rec.spans]
        res.append((y.detach(), z.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(), bn.running_var.clone(),
                    int(bn.num_batches_tracked), names[:n_fwd], names[n_fwd:]))
    a, b = res
    for i, what in enumerate(("y", "dz", "dgamma", "dbeta", "running_mean", "running_var")):
        assert torch.equal(a[i].view(torch.int32), b[i].view(torch.int32)), what
    assert a[6] == b[6] == 1
    assert bool((b[0] == 0).any()) and bool((b[0] != 0).any())
    # one launch where the composition has two; the same two backward launches
    assert b[7].count("sn_affine_dropout_f32") == 1 and "sn_masked_affine_f32" not in b[7] and "sn_dropout_f32" not in b[7]
    assert a[7].count("sn_masked_affine_f32") == 1 and a[7].count("sn_dropout_f32") == 1
    assert [n for n in b[8] if n.startswith("sn_")] == [n for n in a[8] if n.startswith("sn_")] == ["sn_dropout_f32", "sn_bn_act_bwd_f32"]
    # p = 0 is bn_act itself
    bn0 = torch.nn.BatchNorm1d(C).to(DEV).train()
    rec = ops.KernelTimer()
    with rec:
        AG.bn_drop(z0, bn0, 0.0, snap, SC.SITE, nv, K)
    assert "sn_affine_dropout_f32" not in [s[0] for s in rec.spans]


# ----------------------------------------------------------------------------- the encoders on the reference's fixtures
@functools.lru_cache(maxsize=None)
def fixture(name):
    return G.load(name)


def _encoder(name, new, dropout=None):
    """The fixture's encoder with the fixture's weights: a class of dropout_signinv (new) or of dgl_deepsigns (dropout 0)."""
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import dropout_signinv as S
    fx = fixture(name)
    kind = str(fx.meta["kind"])
    hidden, out, layers, k = (int(v) for v in fx.meta["params"])
    p = float(fx.meta["dropout_p"]) if dropout is None else dropout
    args = (1, hidden, out, layers, k) + ((DEV,) if kind == "masked_gin" else ())
    m = getattr(S if new else DS, SC.CLASSES[kind])(*args, use_bn=True, dropout=p if new else 0.0, activation="relu")
    m.load_state_dict(fx.sd, strict=True)
    return m.to(DEV)


def _inputs(fx):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    ei = fx.inp["edge_index"]
    return DS.Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"]), fx.inp["pos_enc"].unsqueeze(-1).to(DEV)


def _seed(model, fx):
    """The fixture's forward is step `dropout_step`: a train-mode forward advances the step first."""
    model.seed_dropout(int(fx.meta["dropout_seed"]), int(fx.meta["dropout_step"]) - 1)


def _recorded(fn):
    from signnet_basisnet_amd import ops
    rec = ops.KernelTimer()
    with rec:
        y = fn()
    return y, [s[0] for s in rec.spans]


def _check_buffers(model, fx, what):
    sd, n = model.state_dict(), 0
    for key, ref in fx.out.items():
        if key.startswith("train/buffers/"):
            k = key[len("train/buffers/"):]
            n += 1
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(ref), f"{what}: {k}"
            else:
                close(sd[k], ref, f"{what}: {k}")
    assert n


def _check_output(y, fx, kind, what):
    y32, y64 = fx.out["train/y"], fx.out["train/y64"]
    ref_err = PU.relerr(y32, y64)
    print(f"{what}: |hip - ref| {PU.relerr(y, y32):.2e}  |hip - f64| {PU.relerr(y, y64):.2e}  |ref - f64| {ref_err:.2e}")
    if kind in ("gin", "masked_gin"):
        torch.testing.assert_close(y.detach().cpu(), y32, rtol=5e-4, atol=5e-5)
    elif ref_err > PU.REL:
        close_conditioned(y, y32, y64, what)
    else:
        close(y, y32, what, ref64=y64)


def _check_gradients(model, fx, kind, what):
    g32 = {k[len("train/grad/"):]: v for k, v in fx.out.items() if k.startswith("train/grad/")}
    g64 = {k[len("train/grad64/"):]: v for k, v in fx.out.items() if k.startswith("train/grad64/")}
    got = {k: q.grad for k, q in model.named_parameters()}
    assert set(got) == set(g64) == set(g32) and all(v is not None for v in got.values())
    gmax = max(float(v.abs().max()) for v in g64.values())
    for k in sorted(got):
        print(f"{what} d {k}: |hip - f64| {PU.relerr(got[k], g64[k]):.2e}  |ref32 - f64| {PU.relerr(g32[k], g64[k]):.2e}")
    for k in sorted(got):
        if kind in ("gin", "masked_gin"):
            e = float((got[k].detach().cpu().double() - g64[k]).abs().max())
            assert e <= 2e-3 * float(g64[k].abs().max()) + 1e-5 * gmax + 1e-6, f"{what}: d {k}: {e:.3e} vs {float(g64[k].abs().max()):.3e}"
        else:
            attributed(got[k], g32[k], g64[k], f"{what}: d {k}")


@pytest.mark.parametrize("name", SC.ENCODER_CASES)
def test_encoders_on_the_reference_fixtures(name):
    fx = fixture(name)
    kind = str(fx.meta["kind"])
    g, x = _inputs(fx)
    # value path: train mode without autograd
    model = _encoder(name, True).train()
    _seed(model, fx)
    with torch.no_grad():
        yv = model(g, x)
    _check_output(yv, fx, kind, f"{name}: train y (value)")
    _check_buffers(model, fx, f"{name} (train, no autograd)")
    # and it is not the dropout-free output
    with torch.no_grad():
        y0 = _encoder(name, False).train()(g, x)
    assert PU.relerr(y0, fx.out["train/y64"]) > 1e-3
    # differentiable path: the same masks, every parameter gradient
    model = _encoder(name, True).train()
    _seed(model, fx)
    yg = model(g, x)
    assert yg.requires_grad
    _check_output(yg, fx, kind, f"{name}: train y (autograd)")
    # (other masks move the output by O(1); the same masks leave fp32 rounding through the BatchNorms: tests/test_dropout_modules_gpu.py)
    print(f"{name}: |value - autograd| {PU.relerr(yv, yg):.2e}")
    assert PU.relerr(yv, yg) < 1e-2
    (yg * fx.inp["cotangent"].to(DEV)).sum().backward()
    _check_buffers(model, fx, f"{name} (train, autograd)")
    _check_gradients(model, fx, kind, name)
    assert model.dropout_state(torch.device(DEV)).t.tolist() == [int(fx.meta["dropout_seed"]), int(fx.meta["dropout_step"])]


# ----------------------------------------------------------------------------- identity with the base classes
@pytest.mark.parametrize("name", SC.ENCODER_CASES)
def test_eval_and_p0_are_the_base_classes(name):
    fx = fixture(name)
    g, x = _inputs(fx)
    base, new = _encoder(name, False).eval(), _encoder(name, True).eval()

    def ev(m):
        def run():
            with torch.no_grad():
                return m(g, x)
        run()
        return _recorded(run)
    (y0, n0), (y1, n1) = ev(base), ev(new)
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32)) and n0 == n1 and n1
    assert not any("dropout" in n for n in n1)
    torch.testing.assert_close(y1.cpu(), fx.out["eval/y"], rtol=5e-4, atol=5e-5)      # (the fixture's weights are the ones that ran)
    with torch.no_grad():          # eval invariance stays bit-exact
        assert torch.equal(new(g, -x), y1)
    # p = 0 in train mode: the base class's launches and bits, value path and differentiable path
    cot = fx.inp["cotangent"].to(DEV)
    outs = []
    for m in (_encoder(name, False).train(), _encoder(name, True, dropout=0.0).train()):
        with torch.no_grad():
            yv, nv = _recorded(lambda: m(g, x))

        def fb():
            y = m(g, x)
            (y * cot).sum().backward()
            return y.detach()
        yg, ng = _recorded(fb)
        outs.append((yv, nv, yg, ng, [q.grad.clone() for q in m.parameters()]))
    a, b = outs
    assert a[1] == b[1] and a[3] == b[3] and not any("dropout" in n for n in b[1] + b[3])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(u, v) for u, v in zip(a[4], b[4]))


# ----------------------------------------------------------------------------- launch structure at p > 0
@pytest.mark.parametrize("name", SC.ENCODER_CASES)
def test_launch_structure(name):
    """Derived from the site table: a post-BatchNorm site is ONE sn_affine_dropout_f32 in place of that BatchNorm's sn_masked_affine_f32,
    an inter-layer site one sn_dropout_f32; the backward regenerates every site's mask with one sn_dropout_f32."""
    fx = fixture(name)
    kind, L_ = str(fx.meta["kind"]), int(fx.meta["params"][2])
    total, fused = SC.site_count(kind, L_), SC.fused_sites(kind, L_)
    g, x = _inputs(fx)
    cot = fx.inp["cotangent"].to(DEV)
    counts = []
    for m in (_encoder(name, False).train(), _encoder(name, True).train()):
        y, fwd = _recorded(lambda: m(g, x))
        _, bwd = _recorded(lambda: (y * cot).sum().backward())
        with torch.no_grad():
            m(g, x)                       # (the value path keeps its batch plan on the graph object: built by whoever comes first)
            _, val = _recorded(lambda: m(g, x))
        counts.append((fwd, bwd, val))
    (f0, b0, v0), (f1, b1, v1) = counts
    for what, n0, n1 in (("differentiable forward", f0, f1), ("value path", v0, v1)):
        assert n1.count("sn_affine_dropout_f32") == fused, what
        assert n1.count("sn_dropout_f32") == total - fused, what
        assert n1.count("sn_masked_affine_f32") == n0.count("sn_masked_affine_f32") - fused, what
        assert len(n1) == len(n0) + (total - fused), what
    assert b1.count("sn_dropout_f32") == total and "sn_affine_dropout_f32" not in b1
    assert len(b1) == len(b0) + total and b1.count("sn_bn_act_bwd_f32") == b0.count("sn_bn_act_bwd_f32")


# ----------------------------------------------------------------------------- step behaviour
STEP_CASES = [SC.ENCODER_CASES[i] for i in (0, 3, 5, 6)]          # one per encoder


@pytest.mark.parametrize("name", STEP_CASES)
def test_steps_differ_repeat_after_seeding_and_a_backward_uses_its_own_masks(name):
    fx = fixture(name)
    kind = str(fx.meta["kind"])
    g, x = _inputs(fx)
    cot = fx.inp["cotangent"].to(DEV)
    model = _encoder(name, True).train()
    model.seed_dropout(7, 0)
    with torch.no_grad():
        a1, a2 = model(g, x), model(g, x)
    assert not torch.equal(a1, a2)
    model.seed_dropout(7, 0)
    with torch.no_grad():
        b1, b2 = model(g, x), model(g, x)
    assert torch.equal(a1.view(torch.int32), b1.view(torch.int32)) and torch.equal(a2.view(torch.int32), b2.view(torch.int32))
    assert model.dropout_state(torch.device(DEV)).t.tolist() == [7, 2]
    # enc(g, x) and enc(g, -x) draw different masks: a train-mode forward with p > 0 is not sign-invariant, as in the reference
    if kind != "transformer":            # (its encoder has no site: rho's masks do not see the sign)
        model.seed_dropout(7, 0)
        with torch.no_grad():
            c1 = model(g, -x)
        print(f"{name}: |y(x) - y(-x)| {PU.relerr(c1, a1):.2e}")
        assert PU.relerr(c1, a1) > 1e-3

    def grads():
        gr = {k: q.grad.clone() for k, q in model.named_parameters() if q.grad is not None}
        model.zero_grad(set_to_none=True)
        return gr

    # forward A, forward B, backward B, backward A: A's gradients are those of A's own masks
    model.seed_dropout(7, 0)
    yA = model(g, x)
    yB = model(g, x)
    (yB * cot).sum().backward()
    gB = grads()
    (yA * cot).sum().backward()
    gA = grads()
    model.seed_dropout(7, 0)
    (model(g, x) * cot).sum().backward()
    gA_alone = grads()
    model.seed_dropout(7, 1)
    (model(g, x) * cot).sum().backward()
    gB_alone = grads()
    assert set(gA) == set(gA_alone)
    for k in gA:
        if bool(gA_alone[k].any()):
            close(gA[k], gA_alone[k], f"{name}: d {k} of forward A after an interleaved forward")
            close(gB[k], gB_alone[k], f"{name}: d {k} of forward B")
    assert max(PU.relerr(gA[k], gB[k]) for k in gA if bool(gB[k].any())) > 1e-2


def test_the_state_is_no_buffer_and_no_state_dict_key():
    name = SC.ENCODER_CASES[0]
    fx = fixture(name)
    g, x = _inputs(fx)
    m0, m1 = _encoder(name, False).train(), _encoder(name, True).train()
    with torch.no_grad():
        m0(g, x), m1(g, x)
    assert list(m0.state_dict().keys()) == list(m1.state_dict().keys())
    assert len(list(m0.buffers())) == len(list(m1.buffers())) and len(list(m0.parameters())) == len(list(m1.parameters()))
    assert "_sn_dropout_state" not in m0.__dict__, "a model without an active site creates no state"


# ----------------------------------------------------------------------------- handle_lap + net
def _net(name, new=True, dropout=0.1):
    from signnet_basisnet_amd import dgl_nets
    from signnet_basisnet_amd import dropout_signinv as S
    fx = fixture(name)
    cls, family, params = SC.net_params(name, DEV, dropout if new else 0.0)
    m = getattr(S if new else dgl_nets, cls)(params)
    if new and dropout and family == "transformer":      # as the reference: the net never hands `dropout` to its layers (make_dropout.py)
        for layer in m.layers:
            layer.dropout = dropout
    m.load_state_dict(fx.sd, strict=True)
    return m.to(DEV), family


def _net_forward(net, fx):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd.dgl_nets import handle_lap
    ei = fx.inp["edge_index"]
    g = DS.Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"])
    p = handle_lap(net, fx.inp["pos_enc"].to(DEV), g)
    return net(g, fx.inp["x"].squeeze(-1).to(DEV), p, fx.inp["edge_attr"].to(DEV), None)[0]


@pytest.mark.parametrize("name", SC.NET_CASES)
def test_net_level_fixtures_through_handle_lap(name):
    """Scores at TRAIN_TOL and gradients at GRAD_TOL of the family (tests/test_lap_baselines_gpu.py, as tests/test_dropout_modules_gpu.py
    holds the same nets to at pe_init 'no_pe'); the encoder's gradients by the same rule as the net's."""
    from test_lap_baselines_gpu import GRAD_TOL, TRAIN_TOL
    fx = fixture(name)
    y32, y64 = fx.out["train/y"], fx.out["train/y64"]
    net, family = _net(name)
    rtol, atol = TRAIN_TOL[family]
    seed, step = int(fx.meta["dropout_seed"]), int(fx.meta["dropout_step"])
    net.train().seed_dropout(seed, step - 1)
    assert net.sign_inv_net.dropout_state(torch.device(DEV)).t.tolist() == [seed, step - 1], "the net's seed reaches the encoder"
    with torch.no_grad():
        yv = _net_forward(net, fx)
    print(f"{name} train y: |hip - ref| {PU.relerr(yv, y32):.2e}  |hip - f64| {PU.relerr(yv, y64):.2e}  |ref - f64| {PU.relerr(y32, y64):.2e}")
    torch.testing.assert_close(yv.cpu(), y32, rtol=rtol, atol=atol)
    _check_buffers(net, fx, f"{name} (train, no autograd)")
    # both holders advanced once, on disjoint sites
    assert net.dropout_state(torch.device(DEV)).t.tolist() == [seed, step]
    assert net.sign_inv_net.dropout_state(torch.device(DEV)).t.tolist() == [seed, step]
    with torch.no_grad():
        y0 = _net_forward(_net(name, new=False)[0].train(), fx)
    assert PU.relerr(y0, y64) > 1e-3
    net, _ = _net(name)
    net.train().seed_dropout(seed, step - 1)
    yg = _net_forward(net, fx)
    assert yg.requires_grad
    print(f"{name} train y (autograd): |hip - f64| {PU.relerr(yg, y64):.2e}")
    torch.testing.assert_close(yg.detach().cpu(), y32, rtol=rtol, atol=atol)
    (yg * fx.inp["cotangent"].to(DEV)).sum().backward()
    _check_buffers(net, fx, f"{name} (train, autograd)")
    g64 = {k[len("train/grad64/"):]: v for k, v in fx.out.items() if k.startswith("train/grad64/")}
    gmax = max(float(v.abs().max()) for v in g64.values())
    tol, seen = GRAD_TOL[family], 0
    for k, q in net.named_parameters():
        if k not in g64:
            assert q.grad is None or not bool(q.grad.any()), k
            continue
        ours = q.grad if q.grad is not None else torch.zeros_like(q)
        scale = max(float(g64[k].abs().max()), 1e-2 * gmax)
        err = float((ours.detach().cpu().double() - g64[k]).abs().max())
        print(f"{name} d {k}: {err / scale:.2e} of max(|f64|, 1e-2 gmax)")
        assert err <= tol * scale + 1e-7, (name, k, err, scale)
        seen += 1
    assert seen > 10 and any(k.startswith("sign_inv_net.") for k in g64)


# ----------------------------------------------------------------------------- captured step
BUCKET_SHAPES = ([5, 9, 12, 7, 3], [8, 4, 11, 6, 10, 2, 7])


def _step_net(lr, seed=3):
    from signnet_basisnet_amd import dropout_signinv as S
    from signnet_basisnet_amd import optim
    _, _, params = SC.net_params(SC.NET_CASES[0], DEV, 0.1)           # gatedgcn + gin, p = 0.1
    torch.manual_seed(seed)
    net = S.GatedGCNNet(params).to(DEV).train()
    net.seed_dropout(9, 0)
    return net, optim.FlatAdam(net.parameters(), lr=lr), params["pos_enc_dim"]


def test_bucketed_step_follows_the_eager_steps_from_the_same_seed():
    """The bounds of the p = 0 padded-vs-eager tests (tests/test_dgl_bucketed_step_gpu.py's helpers, unchanged): a padded step draws the
    eager step's masks, since a valid element's logical index does not move when the batch is padded."""
    import test_dgl_bucketed_step_gpu as T
    from test_deepsigns_variants_gpu import _batch
    lr = 1e-4
    k = _step_net(lr)[2]
    batches = [_batch(k, s, seed=5 + i) for i, s in enumerate(BUCKET_SHAPES)]
    bucket = (max(b.N for b in batches) + 9, max(b.E for b in batches) + 14)
    m1, o1, _ = _step_net(lr)
    eager, ge, _ = T._eager(m1, o1, batches)
    mn, on, _ = _step_net(lr)
    noisy, gn, _ = T._eager(mn, on, T._perturbed(batches))
    m2, o2, _ = _step_net(lr)
    s, padded, gp, _ = T._bucketed(m2, o2, batches, bucket=bucket)
    assert s.captures == 1 and s.hits == 1
    s.check()
    print(f"eager {eager}  noisy {noisy}  padded {padded}")
    T._close_losses(eager, noisy, padded)
    T._close_grads(ge[0], gn[0], gp[0])
    T._close_params(o1, on, o2, len(batches), lr)
    dev = torch.device(DEV)
    for m in (m1, m2):
        assert m.dropout_state(dev).t.tolist() == [9, 2] and m.sign_inv_net.dropout_state(dev).t.tolist() == [9, 2]
    assert getattr(m2.sign_inv_net, "_bucket", None) is None, "the switch does not outlive the step"
    # the same batches WITHOUT dropout give other losses: the masks were drawn
    T._release(s)


def test_replays_draw_fresh_masks_and_the_warm_up_leaves_the_step_words():
    import test_dgl_bucketed_step_gpu as T
    from test_deepsigns_variants_gpu import _batch
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    net, opt, k = _step_net(0.0)                                    # lr 0: the parameters stay, only the masks move a loss
    b = _batch(k, BUCKET_SHAPES[0], seed=5)
    dev = torch.device(DEV)
    s = DGLBucketedStep(net, opt, max_graphs=16)
    l1 = s.step(b.g, b.h, b.p, b.e, None, b.t).item()
    # the warm-up and the capture did not count: the first replay drew step 1 in both states
    assert net.dropout_state(dev).t.tolist() == [9, 1] and net.sign_inv_net.dropout_state(dev).t.tolist() == [9, 1]
    l2 = s.step(b.g, b.h, b.p, b.e, None, b.t).item()
    assert net.dropout_state(dev).t.tolist() == [9, 2] and net.sign_inv_net.dropout_state(dev).t.tolist() == [9, 2]
    assert s.captures == 1 and s.hits == 1 and l1 != l2
    net.seed_dropout(9, 0)                                          # re-seeding reproduces, with no host argument of the graph changed
    r1 = s.step(b.g, b.h, b.p, b.e, None, b.t).item()
    r2 = s.step(b.g, b.h, b.p, b.e, None, b.t).item()
    assert (r1, r2) == (l1, l2) and s.captures == 1
    # only the encoder's step word moved back: the encoder's masks alone change the loss
    net.seed_dropout(9, 0)
    net.dropout_state(dev).set(9, 5)
    assert s.step(b.g, b.h, b.p, b.e, None, b.t).item() != l1
    s.check()
    T._release(s)
