"""-m gpu: `--sign_inv_activation tanh | elu` in the sign-invariant encoders of the DGL tree (signnet_basisnet_amd.activation_signinv,
DESIGN.md §4.5k).

  kernels    sn_act_affine_f32 and sn_act_affine_bwd_f32 through the C ABI against float64 on the grid of
             tests/signinv_activation_cases.py: every R x C, contiguous / strided / misaligned views, the (nvalid, K = 5) row mask, with
             and without scale / shift, outputs between NaN guards; invalid rows exactly 0; repeats and the three access paths bit-equal
  modules    every tests/golden/ds_act_*.npz fixture in eval, train value, BatchNorm buffers and every parameter gradient under
             parity_util.close(..., ref64=) / attributed (1e-5 of the tensor's scale, float64 attribution); eval sign invariance bit for
             bit; the launch-count condition; activation='relu' through the new classes is dropout_signinv, bits and launches
  net        the GatedGCN fixture eager; one padded DGLBucketedStep against the eager step; a GraphedDGLForward replay against eager

THE KERNEL TOLERANCE is measured, not chosen: on the grid's own inputs torch's CPU float32 tanh / elu — the arithmetic the reference trains
with — is compared with float64 in float32 ulps of the result; the kernel may be at most 4 x that figure (two math libraries round
differently, the fused multiply-add adds one rounding) and never needs to be below 2 ulp.  The adjoint is held to the same rule against
dy * act'(a) in float64, a being the SAVED float32 activation output — the only thing the adjoint reads (1 - a^2 has no relative
accuracy with respect to the float64 tanh near saturation: tanh(20) is 1 - 8e-18, its float32 value 1).  With scale / shift the result
is checked in two steps that together say more than an ulp count of a sum that may cancel: the launch without an affine is within the
bound, and the launch with one is the correctly rounded fma of THAT output (|y - a*scale - shift| <= 1/2 ulp(y)); the error against
float64 is also held to the rule in ulps of |a*scale| + |shift|, the magnitude that does not cancel, with torch's CPU float32
`act(x) * scale + shift` — the activation and the BatchNorm apply behind it, as the reference evaluates them — as the yardstick.
Measured on the MI355X over the whole grid (largest error in float32 ulps; torch-CPU | kernel; the test prints them with -s):
    tanh forward   0.51 | 1.31 (bound 2.05)     with scale / shift 1.59 | 2.12 (bound 6.4)     adjoint 1428 | 1.43
    elu  forward   0.66 | 0.89 (bound 2.6)      with scale / shift 1.57 | 1.34 (bound 6.3)     adjoint 1.44 | 1.44 (bound 5.8)
(torch's float32 `dy * (1 - a * a)` cancels near saturation — 1428 ulp of the float64 product; the kernel's fma(-a, a, 1) does not.)
Every figure is printed before it is asserted."""
import functools
import types

import pytest
import torch

import golden_util as G
import parity_util as PU
import signinv_activation_cases as AC
from parity_util import attributed, close
from test_dropout_gpu import Placed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _nothing_is_launched_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, the rest of the file is not run: {e}", returncode=3)


@pytest.fixture(scope="module")
def L():
    from signnet_basisnet_amd import _lib
    return _lib


# ----------------------------------------------------------------------------- the kernels
def _cpu32_adjoint(dy, a, act):
    """torch's CPU float32 evaluation of dy * act'(a): what autograd's TanhBackward / EluBackward compute from the saved output."""
    return dy * (1 - a * a) if act == "tanh" else dy * torch.where(a > 0, torch.ones_like(a), a + 1)


@functools.lru_cache(maxsize=None)
def _grid_case(R, C):
    x = AC.grid_input(R, C, seed=R * 1000 + C)
    dy = torch.randn(R, C, generator=torch.Generator().manual_seed(R * 1000 + C + 7))
    sc = torch.rand(C, generator=torch.Generator().manual_seed(C)) + 0.5
    sh = torch.randn(C, generator=torch.Generator().manual_seed(C + 1))
    nv = AC.nvalid_for(R)
    return types.SimpleNamespace(x=x, dy=dy, sc=sc, sh=sh, nv=nv, valid=AC.rowvalid(R, nv))


@functools.lru_cache(maxsize=None)
def torch_cpu_ulps(act):
    """(forward, forward with scale / shift, adjoint): the largest error of torch's CPU float32 activation, of `act(x) * scale + shift`
    in float32 (the activation and the BatchNorm apply behind it, as the reference evaluates them) and of the adjoint over ALL inputs of
    the grid, in float32 ulps of the float64 result — for the affine form in ulps of |a * scale| + |shift| (_affine_unit)."""
    f, fa, b = 0.0, 0.0, 0.0
    for R in AC.ROWS:
        for C in AC.COLS:
            if R == 0:
                continue
            c = _grid_case(R, C)
            a32 = AC.act_f(act)(c.x)
            a64, y64 = AC.act_ref(c.x, act, None, c.sc, c.sh)
            f = max(f, AC.ulps(a32, a64))
            fa = max(fa, AC.ulps(a32 * c.sc + c.sh, y64, unit=_affine_unit(a64, c)))
            b = max(b, AC.ulps(_cpu32_adjoint(c.dy, a32, act), AC.act_grad_ref(c.dy, a32, act)))
    return f, fa, b


def _affine_unit(a64, c):
    """The magnitude an error of fma(a, scale, shift) is counted against: |a * scale| + |shift|, which does not cancel."""
    return a64.abs() * c.sc.double().abs() + c.sh.double().abs()


def _bound(cpu_ulp):
    return max(2.0, 4.0 * cpu_ulp)


def _guards_untouched(P, what):
    chk = P.buf.clone()
    chk[P.o:P.o + P.n].view(P.rows + 3, P.ld)[:P.rows, :P.cols] = NAN
    bad = (~torch.isnan(chk)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} words outside the output were written (first at buffer word {int(bad[0])})"


def _place(R, C, layout, data=None):
    extra, off = AC.LAYOUTS[layout]
    return Placed(R, C, C + extra, bool(off), NAN, data)


def _fwd(L, X, R, C, act, nv, sc, sh, Y):
    rc = L.lib().sn_act_affine_f32(X.ptr, X.ld, R, C, L.ptr(nv), AC.K_MASK if nv is not None else 0, AC.ACT_CODES[act], L.ptr(sc), L.ptr(sh),
                                   Y.ptr, Y.ld, L.stream())
    L.check(rc, "sn_act_affine_f32")


def _bwd(L, DY, A, R, C, act, nv, DX):
    rc = L.lib().sn_act_affine_bwd_f32(DY.ptr, DY.ld, A.ptr, A.ld, R, C, L.ptr(nv), AC.K_MASK if nv is not None else 0, AC.ACT_CODES[act],
                                       DX.ptr, DX.ld, L.stream())
    L.check(rc, "sn_act_affine_bwd_f32")


def _read(P, what):
    """The output view; every element written (an input NaN is the only NaN an output may hold: checked by ulps())."""
    torch.cuda.synchronize()
    _guards_untouched(P, what)
    return P.v.contiguous().cpu()


WORST = {}          # (act, direction) -> largest kernel error seen, in ulps


def _kernel_case(L, R, C, act, paths):
    cpu_f, cpu_fa, cpu_b = torch_cpu_ulps(act)
    bf, bfa, bb = _bound(cpu_f), _bound(cpu_fa), _bound(cpu_b)
    c = _grid_case(R, C)
    scd, shd = c.sc.to(DEV), c.sh.to(DEV)
    nvd = c.nv.to(DEV)
    bits = {}
    for layout in AC.LAYOUTS:
        for masked in (False, True):
            what = f"{act} {R}x{C} {layout} masked={masked}"
            nv, valid = (nvd, c.valid) if masked else (None, None)
            X, A, Y = _place(R, C, layout, c.x), _place(R, C, layout), _place(R, C, layout)
            want = "none" if R == 0 else AC.path(C, (X.ld, A.ld), (X.ptr, A.ptr))
            paths.add(want)
            _fwd(L, X, R, C, act, nv, None, None, A)
            _fwd(L, X, R, C, act, nv, scd, shd, Y)
            a, y = _read(A, what), _read(Y, what + " affine")
            if R == 0:
                continue
            a64, y64 = AC.act_ref(c.x, act, valid, c.sc, c.sh)
            a64m = a64 if valid is None else torch.where(valid[:, None], a64, torch.zeros_like(a64))
            e = AC.ulps(a, a64m)
            unit = _affine_unit(a64, c)
            e_aff = AC.ulps(y, y64, unit=unit if valid is None else torch.where(valid[:, None], unit, torch.ones_like(unit)))
            # the launch with an affine is the correctly rounded fma of the launch without one
            exact = a.double() * c.sc.double() + c.sh.double()
            if valid is not None:
                exact = torch.where(valid[:, None], exact, torch.zeros_like(exact))
            fin = torch.isfinite(exact)
            half = float(((y.double() - exact).abs()[fin] / AC.ulp32(y.double())[fin]).max())
            WORST[(act, "fwd")] = max(WORST.get((act, "fwd"), 0.0), e)
            WORST[(act, "aff")] = max(WORST.get((act, "aff"), 0.0), e_aff)
            print(f"{what}: act {e:.2f} ulp (bound {bf:.2f}: torch-CPU {cpu_f:.2f}), with affine {e_aff:.2f} ulp (bound {bfa:.2f}: "
                  f"torch-CPU {cpu_fa:.2f}), fma residue {half:.3f} ulp")
            assert e <= bf and e_aff <= bfa and half <= 0.5 + 1e-6, what
            if valid is not None:
                inv = ~valid
                assert not bool(a[inv].view(torch.int32).any()) and not bool(y[inv].view(torch.int32).any()), f"{what}: invalid rows are +0"
            # the adjoint, from the saved output of the launch above
            DY, DX = _place(R, C, layout, c.dy), _place(R, C, layout)
            _bwd(L, DY, A, R, C, act, nv, DX)
            dx = _read(DX, what + " adjoint")
            eb = AC.ulps(dx, AC.act_grad_ref(c.dy, a, act, valid))
            WORST[(act, "bwd")] = max(WORST.get((act, "bwd"), 0.0), eb)
            print(f"{what}: adjoint {eb:.2f} ulp (bound {bb:.2f}: torch-CPU {cpu_b:.2f})")
            assert eb <= bb, what
            if valid is not None:
                assert not bool(dx[~valid].view(torch.int32).any()), f"{what}: invalid rows of the adjoint are +0"
            # repeats are bit-identical
            _fwd(L, X, R, C, act, nv, scd, shd, Y)
            _bwd(L, DY, A, R, C, act, nv, DX)
            assert torch.equal(_read(Y, what).view(torch.int32), y.view(torch.int32)), f"{what}: a repeat differs"
            assert torch.equal(_read(DX, what).view(torch.int32), dx.view(torch.int32)), f"{what}: a repeated adjoint differs"
            # every layout — the row-vector, flat-vector and scalar paths — gives the same bits on the same data
            key = masked
            if key in bits:
                for got, ref, n in zip((a, y, dx), bits[key], ("act", "affine", "adjoint")):
                    assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{what}: {n} differs from the contiguous layout's bits"
            else:
                bits[key] = (a, y, dx)


@pytest.mark.parametrize("act", ["tanh", "elu"])
@pytest.mark.parametrize("C", AC.COLS)
def test_kernel_grid_against_float64(L, C, act):
    paths = set()
    for R in AC.ROWS:
        _kernel_case(L, R, C, act, paths)
    assert paths == ({"none", "row", "scalar"} if C % 4 == 0 else {"none", "flat", "scalar"}), paths
    t = torch_cpu_ulps(act)
    print(f"{act} C={C}: worst so far forward {WORST.get((act, 'fwd'), 0):.2f} ulp, with affine {WORST.get((act, 'aff'), 0):.2f} ulp, "
          f"adjoint {WORST.get((act, 'bwd'), 0):.2f} ulp; torch-CPU {t[0]:.2f} / {t[1]:.2f} / {t[2]:.2f}")


def test_scale_off_a_16_byte_boundary_leaves_the_row_path_with_the_same_bits(L):
    R, C = 65, 64
    c = _grid_case(R, C)
    buf = torch.zeros(2, C + 8, device=DEV)
    outs = []
    for o in (0, 1):
        sc, sh = buf[0, o:o + C], buf[1, o:o + C]
        sc.copy_(c.sc)
        sh.copy_(c.sh)
        X, Y = _place(R, C, "contiguous", c.x), _place(R, C, "contiguous")
        assert AC.path(C, (X.ld, Y.ld), (X.ptr, Y.ptr), (sc.data_ptr(), sh.data_ptr())) == ("row", "flat")[o]
        _fwd(L, X, R, C, "tanh", None, sc, sh, Y)
        outs.append(_read(Y, f"scale offset {o}"))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("layout,want", [("contiguous", "row"), ("offset", "scalar")])
def test_more_groups_than_the_grid_cap(L, layout, want):
    """The second pass of the grid-stride loop (2048 blocks of 256 lanes), forward and adjoint, against torch on the device's own output."""
    R, C = AC.BIG
    x = torch.randn(R, C, generator=torch.Generator().manual_seed(5))
    dy = torch.randn(R, C, generator=torch.Generator().manual_seed(6))
    X, A, DY, DX = _place(R, C, layout, x), _place(R, C, layout), _place(R, C, layout, dy), _place(R, C, layout)
    assert AC.path(C, (X.ld, A.ld), (X.ptr, A.ptr)) == want and (R * C // 4 if want == "row" else R * C) > 2048 * 256
    _fwd(L, X, R, C, "elu", None, None, None, A)
    _bwd(L, DY, A, R, C, "elu", None, DX)
    a, dx = _read(A, "big"), _read(DX, "big adjoint")
    assert AC.ulps(a, AC.act_ref(x, "elu")[0]) <= _bound(torch_cpu_ulps("elu")[0])
    assert AC.ulps(dx, AC.act_grad_ref(dy, a, "elu")) <= _bound(torch_cpu_ulps("elu")[2])


def test_error_codes_and_the_python_wrappers(L):
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import ops
    lib = L.lib()
    x, y = torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, device=DEV)
    s = torch.ones(8, device=DEV)
    ok = [x.data_ptr(), 8, 4, 8, None, 0, 1, s.data_ptr(), s.data_ptr(), y.data_ptr(), 8, L.stream()]
    assert lib.sn_act_affine_f32(*ok) == 0
    for i, v, msg in ((6, 0, b"unknown activation"), (6, 3, b"unknown activation"), (7, None, b"scale and shift go together"),
                      (8, None, b"scale and shift go together"), (0, None, b"bad arguments"), (9, None, b"bad arguments"), (1, 7, b"bad arguments")):
        a = list(ok)
        a[i] = v
        assert lib.sn_act_affine_f32(*a) == -1 and msg in lib.sn_last_error(), (i, v, lib.sn_last_error())
    okb = [x.data_ptr(), 8, y.data_ptr(), 8, 4, 8, None, 0, 2, s.data_ptr(), 8, L.stream()]
    dxb = torch.zeros(4, 8, device=DEV)
    okb[9] = dxb.data_ptr()
    assert lib.sn_act_affine_bwd_f32(*okb) == 0
    for i, v in ((8, 0), (8, 7), (0, None), (2, None), (9, None), (3, 7)):
        a = list(okb)
        a[i] = v
        assert lib.sn_act_affine_bwd_f32(*a) == -1 and b"sn_act_affine_bwd_f32" in lib.sn_last_error(), (i, v)
    torch.cuda.synchronize()
    # the wrappers: ops.act_affine / autograd.activation save the output alone and mask both directions
    R, C = 33, 19
    c = _grid_case(63, 19)
    xs = c.x[:R].clone()
    xs[~torch.isfinite(xs)] = 0.5
    nv = AC.nvalid_for(R).to(DEV)
    valid = AC.rowvalid(R, AC.nvalid_for(R))
    for act in ("tanh", "elu"):
        xd = xs.to(DEV).requires_grad_(True)
        out = AG.activation(xd, act, nv, AC.K_MASK)
        assert torch.equal(out.detach(), ops.act_affine(xs.to(DEV), act, nv, AC.K_MASK))
        saved = out.grad_fn.saved_tensors
        assert len(saved) == 1 and saved[0].data_ptr() == out.data_ptr(), "the adjoint keeps the activation output and nothing else"
        (out * c.dy[:R].to(DEV)).sum().backward()
        a64, _ = AC.act_ref(xs, act, valid)
        assert AC.ulps(xd.grad, AC.act_grad_ref(c.dy[:R], out.detach().cpu(), act, valid)) <= _bound(torch_cpu_ulps(act)[2])
        assert not bool(xd.grad.cpu()[~valid].any()) and not bool(out.detach().cpu()[~valid].any())
    assert ops.act_affine(torch.zeros(0, 8, device=DEV), "tanh").shape == (0, 8)


# ----------------------------------------------------------------------------- the modules on the reference's fixtures
@functools.lru_cache(maxsize=None)
def fixture(name):
    return G.load(name)


def _inputs(fx):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    ei = fx.inp["edge_index"]
    return DS.Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"]), fx.inp["pos_enc"].unsqueeze(-1).to(DEV)


def _seed(model, fx):
    if float(fx.meta["dropout_p"]) > 0.0:          # the fixture's forward is step `dropout_step`: a train-mode forward advances the step first
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


def _check_gradients(model, fx, what):
    """parity_util.attributed per parameter against the reference's float32 and float64 gradients.  A gradient that is zero in exact
    arithmetic (a bias directly in front of a train-mode BatchNorm: 1e-18 in float64, 1e-9 in any float32 run) has no scale of its own:
    a tensor below 1e-9 of the model's largest gradient entry is held to 1e-5 of that entry (the generator's margin rule)."""
    g32 = {k[len("grad/"):]: v for k, v in fx.out.items() if k.startswith("grad/")}
    g64 = {k[len("grad64/"):]: v for k, v in fx.out.items() if k.startswith("grad64/")}
    got = {k: q.grad for k, q in model.named_parameters() if k in g64 or q.grad is not None}
    assert set(got) == set(g64) == set(g32) and all(v is not None for v in got.values())
    top = max(float(v.abs().max()) for v in g64.values())
    for k in sorted(got):
        print(f"{what} d {k}: |hip - f64| {PU.relerr(got[k], g64[k]):.2e}  |ref32 - f64| {PU.relerr(g32[k], g64[k]):.2e}")
    for k in sorted(got):
        if float(g64[k].abs().max()) < 1e-9 * top:
            e = float((got[k].detach().cpu().double() - g64[k]).abs().max())
            assert e <= PU.REL * top, f"{what}: d {k} (zero in exact arithmetic): {e:.3e} vs 1e-5 of {top:.3e}"
        else:
            attributed(got[k], g32[k], g64[k], f"{what}: d {k}")


@pytest.mark.parametrize("name", AC.ENCODER_CASES)
def test_modules_on_the_reference_fixtures(name):
    fx = fixture(name)
    p = AC.params(fx)
    g, x = _inputs(fx)
    y64_eval = AC.module_ref(fx, torch.float64)
    model = AC.build(fx, DEV).eval()
    assert model._act == p.act
    with torch.no_grad():
        y = model(g, x)
    print(f"{name} eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, y64_eval):.2e}")
    close(y, fx.out["eval/y"], f"{name}: eval y", ref64=y64_eval)
    # sign invariance in eval, bit for bit: a negated eigenvector column swaps the two rows of the merged sign axis, nothing else
    flips = torch.tensor([1.0, -1.0] * p.k)[:p.k].view(1, p.k, 1).to(DEV)
    with torch.no_grad():
        assert torch.equal(model(g, x * flips), y) and torch.equal(model(g, -x), y)
    # train mode without autograd
    y32, y64 = fx.out["train/y"], fx.out["train/y64"]
    model.train()
    _seed(model, fx)
    with torch.no_grad():
        yt = model(g, x)
    print(f"{name} train y: |hip - ref| {PU.relerr(yt, y32):.2e}  |hip - f64| {PU.relerr(yt, y64):.2e}  |ref - f64| {PU.relerr(y32, y64):.2e}")
    close(yt, y32, f"{name}: train y", ref64=y64)
    _check_buffers(model, fx, f"{name} (train, no autograd)")
    # train mode under autograd: the same forward, every parameter gradient
    model = AC.build(fx, DEV).train()
    _seed(model, fx)
    yg = model(g, x)
    assert yg.requires_grad
    close(yg, y32, f"{name}: train y (autograd)", ref64=y64)
    (yg * fx.inp["cotangent"].to(DEV)).sum().backward()
    _check_buffers(model, fx, f"{name} (train, autograd)")
    _check_gradients(model, fx, name)


def _sites(p):
    """(eval, train) activation sites of one forward: eval runs both signs of the encoder in one pass."""
    rho = (4 if p.kind == "transformer" else p.layers) - 1
    enc = {"gin": p.layers, "masked_gin": p.layers, "gcn": p.layers - 1, "transformer": 0}[p.kind]
    return enc + rho, 2 * enc + rho


@pytest.mark.parametrize("name", AC.ENCODER_CASES[:5])
def test_launch_count_condition(name):
    """An activation site is the layer-path GEMM with its bias and ONE sn_act_affine_f32 launch: one recorded launch more than the ReLU
    layer path per site, forward.  Backward, one sn_act_affine_bwd_f32 per site stands where the ReLU path runs its (unrecorded)
    sn_relu_bwd_f32: every other recorded entry point is the same."""
    from signnet_basisnet_amd import dropout_signinv as S
    fx = fixture(name)
    p = AC.params(fx)
    assert all(w.shape[0] <= w.shape[1] for k, w in fx.sd.items() if p.kind == "gcn" and k.startswith("enc.layers.") and k.endswith(".weight")
               and not k.startswith(f"enc.layers.{p.layers - 1}.")), "every activated GraphConv of the fixture has its ReLU in the GEMM epilogue"
    n_eval, n_train = _sites(p)
    g, x = _inputs(fx)
    cot = fx.inp["cotangent"].to(DEV)
    counts = []
    for m in (AC.build(fx, DEV, module=S, activation="relu"), AC.build(fx, DEV)):
        m.fused_stages = False                      # the ReLU LAYER path (a non-ReLU encoder takes it whatever the switch says)
        m.eval()
        with torch.no_grad():
            m(g, x)
            _, ev = _recorded(lambda: m(g, x))
        m.train()
        y, fwd = _recorded(lambda: m(g, x))
        _, bwd = _recorded(lambda: (y * cot).sum().backward())
        with torch.no_grad():
            m(g, x)
            _, val = _recorded(lambda: m(g, x))
        counts.append((ev, fwd, bwd, val))
    (e0, f0, b0, v0), (e1, f1, b1, v1) = counts
    for what, n0, n1, sites in (("eval", e0, e1, n_eval), ("differentiable forward", f0, f1, n_train), ("train value", v0, v1, n_train)):
        print(f"{name} {what}: relu {len(n0)} launches, {p.act} {len(n1)} ({sites} sites)")
        assert n1.count("sn_act_affine_f32") == sites and "sn_act_affine_f32" not in n0, what
        assert len(n1) == len(n0) + sites, what
        assert sorted(n for n in n1 if n != "sn_act_affine_f32") == sorted(n0), what
    assert b1.count("sn_act_affine_bwd_f32") == n_train and "sn_act_affine_bwd_f32" not in b0
    assert sorted(n for n in b1 if n != "sn_act_affine_bwd_f32") == sorted(b0)


@pytest.mark.parametrize("name", AC.ENCODER_CASES)
def test_relu_through_the_new_classes_is_dropout_signinv(name):
    """Bit for bit and launch for launch: eval (the three-launch fused forward of the GIN encoders included), the train value and the
    differentiable path with every gradient — at the fixture's dropout, from the same seed."""
    from signnet_basisnet_amd import dropout_signinv as S
    fx = fixture(name)
    p = AC.params(fx)
    g, x = _inputs(fx)
    cot = fx.inp["cotangent"].to(DEV)
    outs = []
    for mod in (S, None):
        m = AC.build(fx, DEV, module=mod, activation="relu").eval()
        assert m._act is None
        with torch.no_grad():
            m(g, x)
            ye, ne = _recorded(lambda: m(g, x))
        if p.kind in ("gin", "masked_gin"):
            assert ne == ["sn_deepsigns_phi_f32", "sn_mlp_chain_f32"] and m._fused.ok, ne
        m.train()
        _seed(m, fx)
        with torch.no_grad():
            yv, nv = _recorded(lambda: m(g, x))
        _seed(m, fx)

        def fb():
            y = m(g, x)
            (y * cot).sum().backward()
            return y.detach()
        yg, ng = _recorded(fb)
        outs.append((ye, ne, yv, nv, yg, ng, [q.grad.clone() for q in m.parameters()]))
    a, b = outs
    assert a[1] == b[1] and a[3] == b[3] and a[5] == b[5] and not any("sn_act_affine" in n for n in b[1] + b[3] + b[5])
    for i in (0, 2, 4):
        assert torch.equal(a[i].view(torch.int32), b[i].view(torch.int32))
    assert all(torch.equal(u, v) for u, v in zip(a[6], b[6]))


@pytest.mark.parametrize("name", AC.ENCODER_CASES[:2])
def test_a_non_relu_gin_encoder_never_takes_the_fused_forward(name):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    fx = fixture(name)
    g, x = _inputs(fx)
    m = AC.build(fx, DEV).eval()
    assert m.fused_stages and not DS._FusedDeepSigns(m).ok
    with torch.no_grad():
        m(g, x)
        _, names = _recorded(lambda: m(g, x))
    assert m._fused is not None and not m._fused.ok
    assert "sn_deepsigns_phi_f32" not in names and "sn_mlp_chain_f32" not in names and "sn_act_affine_f32" in names
    with pytest.raises(ValueError, match="only 'highest'"):
        m.matmul_precision = "high"


# ----------------------------------------------------------------------------- net level
def _fixture_net(device=DEV):
    from signnet_basisnet_amd import activation_signinv as A
    fx = fixture(AC.NET_CASE)
    net = A.GatedGCNNet(AC.net_params(fx, device))
    net.load_state_dict(fx.sd, strict=True)
    return fx, net.to(device)


def _net_forward(net, fx):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd.dgl_nets import handle_lap
    ei = fx.inp["edge_index"]
    g = DS.Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"])
    p = handle_lap(net, fx.inp["pos_enc"].to(DEV), g)
    return net(g, fx.inp["x"].squeeze(-1).to(DEV), p, fx.inp["edge_attr"].to(DEV), None)[0]


def test_net_level_fixture_eager():
    fx, net = _fixture_net()
    y64_eval = AC.net_ref(fx, torch.float64)
    net.eval()
    with torch.no_grad():
        y = _net_forward(net, fx)
    print(f"net eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, y64_eval):.2e}")
    close(y, fx.out["eval/y"], "net: eval y", ref64=y64_eval)
    y32, y64 = fx.out["train/y"], fx.out["train/y64"]
    net.train()
    with torch.no_grad():
        yt = _net_forward(net, fx)
    print(f"net train y: |hip - ref| {PU.relerr(yt, y32):.2e}  |hip - f64| {PU.relerr(yt, y64):.2e}  |ref - f64| {PU.relerr(y32, y64):.2e}")
    close(yt, y32, "net: train y", ref64=y64)
    _check_buffers(net, fx, "net (train, no autograd)")
    fx, net = _fixture_net()
    net.train()
    yg = _net_forward(net, fx)
    close(yg, y32, "net: train y (autograd)", ref64=y64)
    (yg * fx.inp["cotangent"].to(DEV)).sum().backward()
    _check_buffers(net, fx, "net (train, autograd)")
    _check_gradients(net, fx, "net")


SHAPES = ([5, 9, 12, 7, 3], [8, 4, 11, 6, 10, 2, 7])


def _step_net(lr, seed=3):
    from signnet_basisnet_amd import activation_signinv as A
    from signnet_basisnet_amd import optim
    fx = fixture(AC.NET_CASE)
    params = AC.net_params(fx, DEV)
    torch.manual_seed(seed)
    net = A.GatedGCNNet(params).to(DEV)
    return net, optim.FlatAdam(net.parameters(), lr=lr), params["pos_enc_dim"]


def test_bucketed_step_follows_the_eager_step():
    """One padded step through a capacity bucket against the eager step — loss and gradients — and a second, differently shaped batch
    through the same capture, at the bounds tests/test_dgl_bucketed_step_gpu.py holds the ReLU encoder to (its helpers, unchanged):
    tanh(0 + b) is not 0, so a padding row that entered a statistic or a gradient would show here."""
    import test_dgl_bucketed_step_gpu as T
    from test_deepsigns_variants_gpu import _batch
    lr = 1e-4
    k = _step_net(lr)[2]
    batches = [_batch(k, s, seed=5 + i) for i, s in enumerate(SHAPES)]
    bucket = (max(b.N for b in batches) + 9, max(b.E for b in batches) + 14)
    m1, o1, _ = _step_net(lr)
    eager, ge, _ = T._eager(m1.train(), o1, batches)
    mn, on, _ = _step_net(lr)
    noisy, gn, _ = T._eager(mn.train(), on, T._perturbed(batches))
    m2, o2, _ = _step_net(lr)
    s, padded, gp, _ = T._bucketed(m2.train(), o2, batches, bucket=bucket)
    assert s.captures == 1 and s.hits == 1
    s.check()
    print(f"eager {eager}  noisy {noisy}  padded {padded}")
    T._close_losses(eager, noisy, padded)
    T._close_grads(ge[0], gn[0], gp[0])
    T._close_params(o1, on, o2, len(batches), lr)
    assert getattr(m2.sign_inv_net, "_bucket", None) is None, "the switch does not outlive the step"
    T._release(s)


def test_recorded_serving_replays_the_eager_forward():
    from signnet_basisnet_amd import serving
    from test_deepsigns_variants_gpu import _batch
    net, _, k = _step_net(1e-4)
    b = _batch(k, SHAPES[0], seed=5)
    net.eval()
    with torch.no_grad():
        p = net.sign_inv_net(b.g, b.p.unsqueeze(-1)).squeeze(-1)
        y, _ = net(b.g, b.h, p, b.e, None)
    assert torch.isfinite(y).all()
    pe = b.p.unsqueeze(-1)
    fwd = serving.GraphedDGLForward(net, b.g, b.h, pe, b.e)
    for _ in range(2):
        assert torch.equal(fwd(b.g, b.h, pe, b.e), y), "the recorded forward replays the eager eval output"
    fwd.check()
    del fwd
