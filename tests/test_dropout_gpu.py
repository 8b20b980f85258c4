"""-m gpu: sn_dropout_f32 through the C ABI against the numpy restatement of its mask contract (tests/dropout_cases.py).

Every operand is a view into a larger buffer: inputs sit in NaN (a load past C or past R poisons the result), the output in a
sentinel-filled buffer whose gap columns C .. ld - 1, rows behind R and guard words must come back bit-unchanged, with no sentinel
left inside.  Per row of the case table:

  mask     x has no zeros, so `y != residual` IS the keep mask: it equals numpy's exactly
  values   |y - y64| <= 2^-22 (|x| scale + |residual|): at most two fp32 roundings (one when the multiply-add is fused)
  repeat   a second launch is bit-identical
  step     after the step word is bumped ON THE DEVICE the same launch, no host argument changed, draws the next step's mask
"""
import numpy as np
import pytest
import torch

import dropout_cases as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7777.25
PAD = 3


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


class Placed:
    """[rows, cols] float32 view with leading dimension ld into a larger device buffer, 16 bytes of guard in front (20 with `offset`:
    the view is then 4 bytes off a 16-byte boundary), PAD rows and a guard behind; everything outside the view = fill."""

    def __init__(self, rows, cols, ld, offset, fill, data=None):
        self.rows, self.cols, self.ld, self.fill = rows, cols, ld, fill
        self.o = 5 if offset else 4
        self.n = (rows + PAD) * ld
        self.buf = torch.full((self.o + self.n + 8,), fill, dtype=torch.float32, device=DEV)
        self.v = self.buf[self.o:self.o + self.n].view(rows + PAD, ld)[:rows, :cols]
        if data is not None:
            self.v.copy_(data)
        assert self.ptr % 16 == (4 if offset else 0)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.o           # (a zero-row view reports a null data_ptr)

    def assert_sentinels(self, what):
        chk = self.buf.clone()
        chk[self.o:self.o + self.n].view(self.rows + PAD, self.ld)[:self.rows, :self.cols] = self.fill
        want = torch.tensor([self.fill], dtype=torch.float32).view(torch.int32)[0].item()
        bad = (chk.view(torch.int32) != want).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} words outside the output were written (first at buffer word {int(bad[0])})"
        if self.rows * self.cols:
            left = int((self.v.contiguous().view(torch.int32) == want).sum())
            assert left == 0, f"{what}: {left} output elements were never written"


def _operands(c):
    """x without zeros (|x| in [0.5, 1.5)), a residual that is never +-x*scale by accident, all placed per the row's layout."""
    g = torch.Generator().manual_seed(c.R * 1000 + c.C)
    x = (torch.rand(c.R, c.C, generator=g) + 0.5) * (torch.randint(0, 2, (c.R, c.C), generator=g) * 2 - 1).float()
    res = torch.randn(c.R, c.C, generator=g) if c.residual else None
    ld = c.ld or c.C
    X = Placed(c.R, c.C, ld, c.offset, float("nan"), x)
    Rz = Placed(c.R, c.C, ld, c.offset, float("nan"), res) if c.residual else None
    Y = Placed(c.R, c.C, ld, c.offset, SENT)
    return x, res, X, Rz, Y


def _launch(L, c, X, Rz, Y, state, site=DC.SITE):
    thr, scale = DC.threshold_of(c.p), float(DC.scale_of(c.p))
    rc = L.lib().sn_dropout_f32(X.ptr, X.ld, c.R, c.C, thr, scale, state.data_ptr(), site, c.base, Rz.ptr if Rz else None,
                                Rz.ld if Rz else 0, Y.ptr, Y.ld, L.stream())
    L.check(rc, "sn_dropout_f32")


def _state(seed, step):
    seed &= (1 << 64) - 1
    return torch.tensor([seed - (1 << 64) if seed >> 63 else seed, step], dtype=torch.int64).to(DEV)


def _check(c, x, res, y, step):
    keep = DC.keep_mask(c.R, c.C, c.p, DC.SEED, step, DC.SITE, c.base)
    r = np.zeros((c.R, c.C)) if res is None else res.double().numpy()
    yn = y.cpu().numpy()
    got = yn != (0.0 if res is None else res.numpy())
    assert (got == keep).all(), f"{c.id}: {int((got != keep).sum())} mask elements differ from the Philox restatement"
    scale = np.float64(DC.scale_of(c.p))
    y64 = np.where(keep, x.double().numpy() * scale, 0.0) + r
    bound = 2.0 ** -22 * (np.abs(x.double().numpy()) * scale + np.abs(r))
    err = np.abs(yn.astype(np.float64) - y64)
    assert (err <= bound).all(), f"{c.id}: max err/bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}"
    return keep


@pytest.mark.parametrize("c", DC.CASES, ids=[c.id for c in DC.CASES])
def test_dropout_case(L, c):
    ld = c.ld or c.C
    x, res, X, Rz, Y = _operands(c)
    assert DC.vector_path(c.C, c.base, [ld] * (3 if c.residual else 2), [t.ptr for t in (X, Y, Rz) if t is not None]) == (c.path == "vector") \
        or c.path == "none"
    state = _state(DC.SEED, DC.STEP)
    _launch(L, c, X, Rz, Y, state)
    torch.cuda.synchronize()
    if c.R == 0:
        Y.assert_sentinels(c.id)
        return
    Y.assert_sentinels(c.id)
    y1 = Y.v.contiguous().clone()
    keep = _check(c, x, res, y1, DC.STEP)
    if DC.threshold_of(c.p) == 0:
        assert keep.all()
    # repeat: bit-identical
    _launch(L, c, X, Rz, Y, state)
    assert torch.equal(Y.v.contiguous().view(torch.int32), y1.view(torch.int32)), f"{c.id}: the repeat differs"
    # the step word moves on the device; the launch's host arguments do not
    state[1:].add_(1)
    _launch(L, c, X, Rz, Y, state)
    keep2 = _check(c, x, res, Y.v.contiguous(), DC.STEP + 1)
    Y.assert_sentinels(c.id + " (next step)")
    if DC.threshold_of(c.p) and c.R * c.C >= 64:
        assert (keep2 != keep).any()


def test_offset_pointers_draw_the_aligned_mask(L):
    """The mask belongs to the logical index: the vector path and the scalar path (4-byte-offset pointers) give the same bits."""
    ys = []
    for off in (False, True):
        c = DC.Case("pair", 7, 128, None, off, True, 0, 0.5, "vector" if not off else "scalar")
        x, res, X, Rz, Y = _operands(c)
        _launch(L, c, X, Rz, Y, _state(99, 5))
        ys.append(Y.v.contiguous().clone())
    assert torch.equal(ys[0].view(torch.int32), ys[1].view(torch.int32))


def test_sites_are_independent_streams(L):
    c = DC.Case("sites", 33, 77, None, False, False, 0, 0.5, "scalar")
    x, res, X, Rz, Y = _operands(c)
    st = _state(DC.SEED, DC.STEP)
    masks = []
    for site in (0, 1):
        _launch(L, c, X, Rz, Y, st, site=site)
        got = (Y.v != 0).cpu().numpy()
        assert (got == DC.keep_mask(33, 77, 0.5, DC.SEED, DC.STEP, site)).all()
        masks.append(got)
    assert (masks[0] != masks[1]).any()


def test_argument_checks(L):
    lib = L.lib()
    buf = torch.zeros(64, device=DEV)
    st = _state(1, 0)
    p, s = buf.data_ptr(), st.data_ptr()
    for args in [(None, 4, 2, 4, 0, 1.0, s, 0, 0, None, 0, p, 4, None),          # null x
                 (p, 4, 2, 4, 0, 1.0, None, 0, 0, None, 0, p + 64, 4, None),      # null state
                 (p, 3, 2, 4, 0, 1.0, s, 0, 0, None, 0, p + 64, 4, None),         # ldx < C
                 (p, 4, 2, 4, 0, 1.0, s, 0, 0, None, 0, p + 64, 3, None),         # ldy < C
                 (p, 4, 2, 4, 0, 1.0, s, 0, 0, p + 128, 3, p + 64, 4, None),      # ldr < C
                 (p, 4, 2, 4, 0, 1.0, s, 0, -1, None, 0, p + 64, 4, None),        # base < 0
                 (p, 4, -1, 4, 0, 1.0, s, 0, 0, None, 0, p + 64, 4, None),        # R < 0
                 (p, 4, 2, 0, 0, 1.0, s, 0, 0, None, 0, p + 64, 4, None),         # C = 0
                 (p + 2, 4, 2, 4, 0, 1.0, s, 0, 0, None, 0, p + 64, 4, None)]:    # 2-byte-offset pointer
        assert lib.sn_dropout_f32(*args) == -1 and b"sn_dropout_f32" in lib.sn_last_error(), args
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


# ----------------------------------------------------------------------------- ops.dropout / AG.dropout
def test_ops_dropout_edge_probabilities():
    from signnet_basisnet_amd import ops
    st = ops.DropoutState(seed=5, device=DEV)
    x = torch.randn(9, 12, device=DEV)
    r = torch.randn(9, 12, device=DEV)
    snap = st.snapshot()
    assert ops.dropout(x, 0.0, snap, 0) is x
    assert torch.equal(ops.dropout(x, 0.0, snap, 0, residual=r), x + r)
    assert torch.equal(ops.dropout(x, 1.0, snap, 0), torch.zeros_like(x))
    assert torch.equal(ops.dropout(x, 1.0, snap, 0, residual=r), r)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="dropout probability has to be between 0 and 1"):
            ops.dropout(x, bad, snap, 0)
    y = ops.dropout(x, 0.25, snap, 3, residual=r)
    keep = torch.from_numpy(DC.keep_mask(9, 12, 0.25, 5, 0, 3)).to(DEV)
    assert torch.equal(y != r, keep)


def test_dropout_state():
    from signnet_basisnet_amd import ops
    torch.manual_seed(1234)
    st = ops.DropoutState(device=DEV)
    assert st.t.dtype == torch.int64 and st.t.tolist() == [1234, 0]
    snap = st.snapshot()
    st.advance().advance()
    assert st.t.tolist() == [1234, 2] and snap.tolist() == [1234, 0] and snap.data_ptr() != st.t.data_ptr()
    st.set((1 << 64) - 1, 7)
    assert st.t.tolist() == [-1, 7]
    x = torch.ones(4, 8, device=DEV)
    # seed 2^64 - 1: both key words are ffffffff
    assert torch.equal(ops.dropout(x, 0.5, st.snapshot(), 0) != 0, torch.from_numpy(DC.keep_mask(4, 8, 0.5, (1 << 64) - 1, 7, 0)).to(DEV))


@pytest.mark.parametrize("shape", [(33, 77), (6, 128)])
def test_autograd_dropout(shape):
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import ops
    p = 0.5
    st = ops.DropoutState(seed=77, device=DEV)
    st.set(77, 9)
    snap = st.snapshot()
    g = torch.Generator().manual_seed(3)
    x = ((torch.rand(*shape, generator=g) + 0.5)).to(DEV).requires_grad_()
    r = torch.randn(*shape, generator=g).to(DEV).requires_grad_()
    dy = (torch.rand(*shape, generator=g) + 0.5).to(DEV)
    y = AG.dropout(x, p, snap, 2, residual=r)
    st.advance()                       # the state moves on; the forward's snapshot does not
    y.backward(dy)
    keep = torch.from_numpy(DC.keep_mask(shape[0], shape[1], p, 77, 9, 2)).to(DEV)
    assert torch.equal(y.detach() != r.detach(), keep)
    assert torch.equal(x.grad != 0, keep), "dx's zero pattern is not y's"
    scale = torch.tensor(float(DC.scale_of(p)), device=DEV)
    assert torch.equal(x.grad[keep].view(torch.int32), (dy * scale)[keep].view(torch.int32)), "dx != dy * scale on kept elements"
    assert torch.equal(r.grad, dy)
    # without a residual; p = 0 is the identity and records nothing
    x2 = x.detach().clone().requires_grad_()
    y2 = AG.dropout(x2, p, snap, 2)
    y2.backward(dy)
    assert torch.equal(x2.grad, x.grad)
    assert AG.dropout(x2, 0.0, snap, 2) is x2
