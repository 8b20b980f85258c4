"""-m gpu: every dispatch branch of the forward primitives of csrc/ops.hip against float64, through the C ABI.

One parametrized test per op over its table in tests/ops_cases.py.  A row re-asserts, with the device's own CU count, that the host
dispatch takes the branch the row names, then runs the entry point on operands that are VIEWS into larger buffers:

  misaligned   the operand starts 4 bytes into a 16-byte aligned buffer
  strided      the operand is a column block of a wider row matrix; the gap columns and the rows behind an input hold NaN, so a load
               past d_in or past R poisons the result
  sentinels    every output lies in a sentinel-filled buffer with rows behind R, the gap columns d_out .. ld - 1 and guard words in
               front and behind: after the call every sentinel must be bit-unchanged (a vector store past d_out, a tile that writes
               rows >= R), and no sentinel may be left INSIDE the output (an output tile no block wrote)

Values are accepted by the project's rule (parity_util.attributed) against the float32 and float64 restatements:

    |hip - f64| <= max(REL * scale, 2 |cpu32 - f64| + ATTR * scale),   scale = max |f64|

The aggregations promise the reference's summation order: they are also bit-equal to the float32 restatement.  Counts are exact.
tests/test_ops_cases_cpu.py asserts, without a GPU, that every row reaches the branch it names and that float32 itself is within REL.
"""
import ctypes
import functools

import pytest
import torch

import ops_cases as OC
import parity_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7777.25
PAD = 16                       # sentinel / NaN rows behind every row matrix


@pytest.fixture(autouse=True)
def _nothing_is_launched_after_a_device_error():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, the rest of the grid is not run: {e}", returncode=3)


def ids(cases):
    return [c.id for c in cases]


def _bits(t):
    return t.view(torch.int32)


class Placed:
    """[rows, cols] float32 view with leading dimension ld into a larger device buffer: 16 bytes of guard in front (20 when `offset`:
    the view is then 4 bytes off a 16-byte boundary), `pad` more rows and a guard behind, everything outside the view = `fill`"""

    def __init__(self, rows, cols, ld=None, offset=False, pad=PAD, fill=SENT, data=None):
        self.rows, self.cols, self.ld, self.pad, self.fill = rows, cols, ld or cols, pad, fill
        self.o = 5 if offset else 4
        self.n = (rows + pad) * self.ld
        self.buf = torch.full((self.o + self.n + 8,), fill, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.v = self.buf[self.o:self.o + self.n].view(rows + pad, self.ld)[:rows, :cols]
        if data is not None:
            self.v.copy_(data)
        assert self.v.data_ptr() % 16 == (4 if offset else 0)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def assert_sentinels(self, what, inside=True):
        """everything outside the view is bit-unchanged; inside=False: only the guards in front of and behind the whole block (scratch)"""
        chk = self.buf.clone()
        if inside:
            chk[self.o:self.o + self.n].view(self.rows + self.pad, self.ld)[:self.rows, :self.cols] = self.fill
        else:
            chk[self.o:self.o + self.n] = self.fill
        want = _bits(torch.tensor([self.fill], dtype=torch.float32))[0].item()
        bad = (_bits(chk) != want).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} words outside the output were written (first at buffer word {int(bad[0])}, view starts at {self.o}, ld {self.ld})"
        if inside and self.rows * self.cols:
            left = int((_bits(self.v.contiguous()) == want).sum())
            assert left == 0, f"{what}: {left} output elements were never written"


def inp(t, ld=None, offset=False):
    t2 = t if t.dim() == 2 else t[None, :]
    return Placed(t2.shape[0], t2.shape[1], ld, offset, pad=PAD if t.dim() == 2 else 0, fill=float("nan"), data=t2.to(DEV))


def vec_out(n, data=None):
    return Placed(1, n, pad=0, data=None if data is None else data[None, :].to(DEV))


def i32(t):
    return None if t is None else t.to(torch.int32).to(DEV)


@functools.lru_cache(None)
def cu_count():
    from signnet_basisnet_amd._lib import check, lib
    cus = ctypes.c_int(0)
    check(lib().sn_device_info(ctypes.byref(cus), None, None), "sn_device_info")
    assert cus.value > 0
    return cus.value


def assert_branch(case):
    got = OC.OPS[case.op].predicate(case.p, cu_count())
    assert got == case.branch, f"{case.id}: on {cu_count()} CUs the host takes [{got}], the row was written for [{case.branch}]"


class Worst:
    def __init__(self, case):
        self.case, self.w = case, (0.0, 0.0, "")

    def check(self, what, hip, r32, r64):
        assert tuple(hip.shape) == tuple(r64.shape), f"{self.case.id} {what}: shape {tuple(hip.shape)} vs {tuple(r64.shape)}"
        assert bool(torch.isfinite(hip).all()), f"{self.case.id} [{self.case.branch}] {what}: not finite (a load outside the operand, or an element never written)"
        e = PU.attributed(hip, r32, r64, f"{self.case.id} [{self.case.branch}] {what}")
        self.w = max(self.w, (*e, what))

    def report(self):
        print(f"\n{self.case.id}: worst |hip - f64| {self.w[0]:.2e}, |cpu32 - f64| there {self.w[1]:.2e} ({self.w[2]})", end="")


# ---------------------------------------------------------------------------- masked linear
def _linear_operands(p, t):
    from signnet_basisnet_amd import ops
    d_in, d_out, names, off, ldx, ldy, ldr, ldbb = OC.linear_lds(p)
    d = {"x": inp(t["x"], ldx, "x" in off), "wp": ops.pack_weight(t["W"].to(DEV)), "nv": i32(t["nv"]), "K": t["K"]}
    for n in names:
        d[n] = inp(t[n], {"res": ldr, "bbias": ldbb}.get(n), n in off)
    return d


def _linear_call(p, flags, d, R, y):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    d_in, d_out, names, off, ldx, ldy, ldr, ldbb = OC.linear_lds(p)
    g = lambda n: d[n].ptr if n in d else None
    if "bbias" in names:
        check(lib().sn_masked_linear_blockbias_f32(d["x"].ptr, ldx, R, d_in, ptr(d["wp"]), d_out, g("bias"), g("bbias"), OC.BB_ROWS, ldbb,
                                                   flags & ~OC.EPI_BLOCK_BIAS, g("scale"), g("shift"), y.ptr, ldy, stream()),
              "sn_masked_linear_blockbias_f32")
    else:
        check(lib().sn_masked_linear_f32(d["x"].ptr, ldx, R, d_in, ptr(d["wp"]), d_out, g("bias"), ptr(d["nv"]), d["K"], flags, g("scale"),
                                         g("shift"), g("res"), ldr if "res" in names else 0, y.ptr, ldy, stream()), "sn_masked_linear_f32")


@pytest.mark.parametrize("case", OC.LINEAR, ids=ids(OC.LINEAR))
def test_masked_linear(case):
    assert_branch(case)
    p = case.p
    t = OC.linear_gen(case)
    flags = OC.EPIS[p["epi"]][0]
    d_in, d_out, names, off, ldx, ldy, ldr, ldbb = OC.linear_lds(p)
    R = p["R"]
    d = _linear_operands(p, t)
    y = Placed(R, d_out, ldy, "y" in off)
    _linear_call(p, flags, d, R, y)
    torch.cuda.synchronize()
    y.assert_sentinels(f"{case.id} [{case.branch}] y")
    w = Worst(case)
    w.check("y", y.v.cpu(), OC.linear_ref(flags, t, OC.F32), OC.linear_ref(flags, t, OC.F64))
    if p.get("first16"):          # the same products in the same order as the per-wave kernel a 16-row launch takes
        p16 = dict(p, R=16)
        assert OC.linear_branch(p16, cu_count()).startswith("k_linear<true,true>")
        y16 = Placed(16, d_out, ldy)
        _linear_call(p, flags, d, 16, y16)
        torch.cuda.synchronize()
        y16.assert_sentinels(f"{case.id} 16-row launch")
        assert torch.equal(y16.v, y.v[:16]), f"{case.id}: k_linear_lds<16,16> differs in bits from k_linear on the first 16 rows"
    w.report()


@pytest.mark.parametrize("name", sorted(OC.LINEAR_REJECTED))
def test_masked_linear_rejects_contradictory_flags_before_any_launch(name):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    flags, msg = OC.LINEAR_REJECTED[name]
    case = OC.LINEAR[1]                    # (128, 128) x 33 rows with every operand
    t = OC.linear_gen(case)
    d = _linear_operands(case.p, t)
    R, dd = case.p["R"], 128
    y = Placed(R, dd)
    with pytest.raises(RuntimeError, match=msg):
        check(lib().sn_masked_linear_f32(d["x"].ptr, dd, R, dd, ptr(d["wp"]), dd, d["bias"].ptr, ptr(d["nv"]), t["K"], flags, d["scale"].ptr,
                                         d["shift"].ptr, d["res"].ptr, dd, y.ptr, dd, stream()), "sn_masked_linear_f32")
    torch.cuda.synchronize()
    assert bool((y.buf == SENT).all())
    test_masked_linear(case)               # the entry point serves the next call


# ---------------------------------------------------------------------------- linear + BatchNorm statistics
def _stat_outputs(C, t):
    out = {k: vec_out(C) for k in ("mean", "var", "rstd", "scale", "shift")}
    out["count"] = vec_out(1)
    for k in ("rmean", "rvar"):
        out[k] = None if t[k] is None else vec_out(C, t[k])
    return out


def _check_stats(w, out, s32, s64):
    for k, pl in out.items():
        if pl is not None:
            pl.assert_sentinels(f"{w.case.id} {k}")
            w.check(k, pl.v[0].cpu(), s32[k], s64[k])
    assert out["count"].v.item() == s64["count"].item(), f"{w.case.id}: count {out['count'].v.item()} vs {s64['count'].item()}"


@pytest.mark.parametrize("case", OC.LINEAR_BN, ids=ids(OC.LINEAR_BN))
def test_linear_bn_train(case):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    assert_branch(case)
    p = case.p
    t = OC.linear_bn_gen(case)
    (d_in, d_out), R, off = p["d"], p["R"], p.get("off") or ()
    ldx, ldz = p.get("ldx") or d_in, p.get("ldz") or d_out
    x, wp, nv = inp(t["x"], ldx, "x" in off), ops.pack_weight(t["W"].to(DEV)), i32(t["nv"])
    bias = inp(t["bias"], None, "bias" in off) if "bias" in t else None
    gamma, beta = (None if t[k] is None else inp(t[k]) for k in ("gamma", "beta"))
    z, z2 = Placed(R, d_out, ldz, "z" in off), Placed(R, d_out, ldz, "z" in off)
    out = _stat_outputs(d_out, t)
    op = lambda pl: None if pl is None else pl.ptr
    scratch = Placed(1, max(int(lib().sn_linear_bn_scratch_floats(R, d_in, d_out)), 1), pad=0)
    check(lib().sn_linear_bn_train_f32(x.ptr, ldx, R, d_in, ptr(wp), d_out, op(bias), ptr(nv), t["K"], z.ptr, ldz, op(gamma), op(beta), OC.BN_EPS,
                                       OC.BN_MOMENTUM, op(out["rmean"]), op(out["rvar"]), out["mean"].ptr, out["var"].ptr, out["rstd"].ptr,
                                       out["scale"].ptr, out["shift"].ptr, out["count"].ptr, scratch.ptr, stream()), "sn_linear_bn_train_f32")
    check(lib().sn_masked_linear_f32(x.ptr, ldx, R, d_in, ptr(wp), d_out, op(bias), ptr(nv), t["K"], OC.EPI_BIAS if bias is not None else 0, None,
                                     None, None, 0, z2.ptr, ldz, stream()), "sn_masked_linear_f32")
    torch.cuda.synchronize()
    z.assert_sentinels(f"{case.id} [{case.branch}] z")
    z2.assert_sentinels(f"{case.id} z of sn_masked_linear_f32")
    scratch.assert_sentinels(f"{case.id} scratch", inside=False)
    assert torch.equal(z.v, z2.v), f"{case.id}: z differs in bits from sn_masked_linear_f32"
    (z32, s32), (z64, s64) = OC.linear_bn_ref(t, OC.F32), OC.linear_bn_ref(t, OC.F64)
    w = Worst(case)
    w.check("z", z.v.cpu(), z32, z64)
    _check_stats(w, out, s32, s64)
    w.report()


# ---------------------------------------------------------------------------- column statistics
def _stats_inputs(case):
    t = OC.stats_gen(case)
    nv, K, valid = t["mask"]
    ld = case.p.get("ld") or case.p["C"]
    s32, s64 = (OC.stats_ref(t["x"], valid, dt, t["gamma"], t["beta"], t["rmean"], t["rvar"]) for dt in (OC.F32, OC.F64))
    return t, inp(t["x"], ld), ld, i32(nv), K, s32, s64


def _stats_scratch(R, C):
    from signnet_basisnet_amd._lib import lib
    nb = int(lib().sn_colstats_blocks(R))
    return Placed(1, nb * (C + 1), pad=0)


@pytest.mark.parametrize("case", OC.COLSTATS, ids=ids(OC.COLSTATS))
def test_masked_colstats(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    assert_branch(case)
    R, C = case.p["R"], case.p["C"]
    t, x, ld, nv, K, s32, s64 = _stats_inputs(case)
    out = {k: vec_out(C) for k in ("mean", "var")}
    out["count"] = vec_out(1)
    scratch = _stats_scratch(R, C)
    check(lib().sn_masked_colstats_f32(x.ptr, ld, R, C, ptr(nv), K, out["mean"].ptr, out["var"].ptr, out["count"].ptr, scratch.ptr, stream()),
          "sn_masked_colstats_f32")
    torch.cuda.synchronize()
    scratch.assert_sentinels(f"{case.id} scratch", inside=False)
    w = Worst(case)
    _check_stats(w, out, s32, s64)
    w.report()


@pytest.mark.parametrize("case", OC.BN_STATS, ids=ids(OC.BN_STATS))
def test_bn_train_stats(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    assert_branch(case)
    R, C = case.p["R"], case.p["C"]
    t, x, ld, nv, K, s32, s64 = _stats_inputs(case)
    gamma, beta = (None if t[k] is None else inp(t[k]) for k in ("gamma", "beta"))
    out = _stat_outputs(C, t)
    op = lambda pl: None if pl is None else pl.ptr
    scratch = _stats_scratch(R, C)
    check(lib().sn_bn_train_stats_f32(x.ptr, ld, R, C, ptr(nv), K, op(gamma), op(beta), OC.BN_EPS, OC.BN_MOMENTUM, op(out["rmean"]), op(out["rvar"]),
                                      out["mean"].ptr, out["var"].ptr, out["rstd"].ptr, out["scale"].ptr, out["shift"].ptr, out["count"].ptr,
                                      scratch.ptr, stream()), "sn_bn_train_stats_f32")
    torch.cuda.synchronize()
    scratch.assert_sentinels(f"{case.id} scratch", inside=False)
    w = Worst(case)
    _check_stats(w, out, s32, s64)
    w.report()


# ---------------------------------------------------------------------------- aggregations
@functools.lru_cache(None)
def agg_fixture():
    """the hand-built batch, its CPU CSR and the plan ops.build_plan makes of it (the same arrays: asserted)"""
    from signnet_basisnet_amd import ops
    batch, ei, sizes = OC.agg_batch()
    csr = OC.agg_csr(batch, ei, sizes)
    plan = ops.build_plan(batch.to(DEV), ei.to(DEV), len(sizes), 0)
    plan.check()
    for name, mine in zip(("rowptr", "col", "eperm", "graph_ptr"), csr):
        assert torch.equal(getattr(plan, name).cpu().long(), mine), f"build_plan: {name} is not the stable destination sort"
    return batch, ei, sizes, csr, plan


def _agg_case(case, launch):
    assert_branch(case)
    batch, ei, sizes, csr, plan = agg_fixture()
    p = case.p
    N, E, W, off = batch.numel(), ei.shape[1], p.get("F") or p["C"], p.get("off") or ()
    t = OC.agg_gen(case, N, E)
    d = {"x": inp(t["x"], None, "x" in off), "out": Placed(N, W, None, "out" in off), "eps": None if t["eps"] is None else t["eps"].reshape(1).to(DEV)}
    for k in ("ea", "plus"):
        if k in t:
            d[k] = inp(t[k], None, k in off)
    launch(d, plan, N, W)
    torch.cuda.synchronize()
    d["out"].assert_sentinels(f"{case.id} [{case.branch}] out")
    kw = dict(eps=t["eps"], ea=t.get("ea"), negate=bool(p.get("negate")), plus=t.get("plus"))
    r32, r64 = OC.agg_ref(t["x"], csr, OC.F32, **kw), OC.agg_ref(t["x"], csr, OC.F64, **kw)
    hip = d["out"].v.cpu()
    w = Worst(case)
    w.check("out", hip, r32, r64)
    assert torch.equal(hip, r32), (f"{case.id} [{case.branch}]: not the reference's summation order ({int((hip != r32).sum())} elements differ from "
                                   f"the float32 sum in edge order, self term last)")
    w.report()


@pytest.mark.parametrize("case", OC.GIN, ids=ids(OC.GIN))
def test_gin_aggregate(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    _agg_case(case, lambda d, plan, N, F: check(lib().sn_gin_aggregate_f32(d["x"].ptr, d["out"].ptr, N, F, ptr(plan.rowptr), ptr(plan.col),
                                                                           ptr(d["eps"]), int(bool(case.p.get("negate"))), stream()),
                                                "sn_gin_aggregate_f32"))


@pytest.mark.parametrize("case", OC.GIN_ADD, ids=ids(OC.GIN_ADD))
def test_gin_aggregate_add(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    _agg_case(case, lambda d, plan, N, F: check(lib().sn_gin_aggregate_add_f32(d["x"].ptr, d["plus"].ptr, d["out"].ptr, N, F, ptr(plan.rowptr),
                                                                               ptr(plan.col), ptr(d["eps"]), stream()), "sn_gin_aggregate_add_f32"))


@pytest.mark.parametrize("case", OC.SLAB, ids=ids(OC.SLAB))
def test_gin_aggregate_slab(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    _agg_case(case, lambda d, plan, N, F: check(lib().sn_gin_aggregate_slab_f32(d["x"].ptr, d["out"].ptr, N, F, plan.B, ptr(plan.graph_ptr),
                                                                                ptr(plan.rowptr), ptr(plan.col), ptr(d["eps"]),
                                                                                int(bool(case.p.get("negate"))), stream()),
                                                "sn_gin_aggregate_slab_f32"))


@pytest.mark.parametrize("case", OC.GINE, ids=ids(OC.GINE))
def test_gine_aggregate(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    _agg_case(case, lambda d, plan, N, C: check(lib().sn_gine_aggregate_f32(d["x"].ptr, d["ea"].ptr, d["out"].ptr, N, C, ptr(plan.rowptr),
                                                                            ptr(plan.col), ptr(plan.eperm), ptr(d["eps"]), stream()),
                                                "sn_gine_aggregate_f32"))


# ---------------------------------------------------------------------------- segment pool
@pytest.mark.parametrize("case", OC.POOL, ids=ids(OC.POOL))
def test_segment_pool(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    assert_branch(case)
    C, mode = case.p["C"], case.p["mode"]
    xs, lens = OC.pool_gen(case)
    gp = torch.tensor([0] + lens).cumsum(0).to(torch.int32).to(DEV)
    x, out = inp(xs), Placed(len(lens), C, pad=4)
    check(lib().sn_segment_pool_f32(x.ptr, len(lens), C, ptr(gp), 1 if mode == "mean" else 0, out.ptr, stream()), "sn_segment_pool_f32")
    torch.cuda.synchronize()
    out.assert_sentinels(f"{case.id} out")
    hip = out.v.cpu()
    w = Worst(case)
    w.check("out", hip, OC.pool_ref(xs, lens, mode, OC.F32), OC.pool_ref(xs, lens, mode, OC.F64))
    assert not bool(hip[[i for i, n in enumerate(lens) if n == 0]].any()), f"{case.id}: an empty segment is not 0"
    w.report()
