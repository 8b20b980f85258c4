"""Case tables, input generators and dtype-generic torch restatements for the forward-primitive grid (tests/test_ops_grid_gpu.py runs
the HIP kernels on them through the C ABI, tests/test_ops_cases_cpu.py checks the conditions that make that comparison mean something).
Importable without a GPU: nothing here touches a device or the package's library.

The forward primitives of csrc/ops.hip pick one of several kernels from the shape, the leading dimensions, the pointer alignment, the
epilogue flags and (for the LDS-resident Linear) the CU count.  A row of a table exists for ONE such choice: its `branch` string is a
" | "-separated list of names, each a kernel or a host branch with the source condition that selects it, and the `*_branch` functions
below restate the host dispatch (row parameters, CU count -> branch string).  The CPU test asserts predicate(row) == row.branch and that
the rows of an op reach every name its predicate can return, so an edit of a table cannot silently move a case onto another kernel.

Alignment is a per-operand flag: `off` lists the operands that start 4 bytes into a 16-byte aligned buffer.  A leading dimension that
is None is the dense one.  A `&&` chain of the host code is restated with its short circuit: the FIRST false clause is the one named
(`false_clauses` lists them all, for the rows that falsify exactly one).

A restatement maps the inputs to the outputs in the dtype it is given: float64 is the exact value, float32 the reference's arithmetic.
"""
import zlib

import torch

F32, F64 = torch.float32, torch.float64
CUS = 256                        # the CU count the tables are written for (MI355X); the GPU test re-asserts with the device's own

EPI_BIAS, EPI_RELU_PRE, EPI_AFFINE, EPI_RELU, EPI_RESIDUAL, EPI_BLOCK_BIAS, EPI_RESIDUAL_PRE, EPI_LEAKY = 1, 2, 4, 8, 16, 32, 64, 128
LIN_LDS_MIN_ROWS, CS_SPLIT, BN_EPS, BN_MOMENTUM = 32, 16, 1e-5, 0.1


def cdiv(a, b):
    return -(-a // b)


class Case:
    def __init__(self, op, branch, **p):
        self.op, self.branch, self.p = op, branch, p

    @property
    def id(self):
        return self.op + "-" + "-".join(f"{k}{_short(v)}" for k, v in self.p.items() if v is not None and v is not False)

    def __repr__(self):
        return self.id


def _short(v):
    if v is True:
        return ""
    if isinstance(v, (tuple, list)):
        return "x".join(str(x) for x in v)
    return str(v)


def rng(case_or_id, salt=0):
    name = case_or_id if isinstance(case_or_id, str) else case_or_id.id
    return torch.Generator().manual_seed((zlib.crc32(name.encode()) + salt) % (2 ** 31))


def names(branch):
    return set(branch.split(" | "))


# ============================================================================ row masks
def mask_rows(mode, R, g):
    """-> (nvalid int32 [cdiv(R, K)] or None, K, bool [R]).  'k7': K = 7 (does not divide a 16-row tile), ragged counts 0 .. 7.
    'k1': K = 1, counts in {0, 1}.  Both kill rows 16 .. 47 (a 16-row tile with no valid row, where there are that many rows) and rows
    64 .. 255 of a batch of >= 512 rows (whole waves and a whole workgroup of the LDS-resident Linear with nothing valid)."""
    if mode is None:
        return None, 0, torch.ones(R, dtype=torch.bool)
    K = {"k7": 7, "k1": 1}[mode]
    N = cdiv(R, K)
    nv = torch.randint(0, K + 1, (N,), generator=g, dtype=torch.int32)
    nv[0] = K
    if N > 1:
        nv[-1] = 1
    dead = [(16, 48)] + ([(64, 256)] if R >= 512 else [])
    for lo, hi in dead:
        if R >= hi:
            nv[lo // K:cdiv(hi, K)] = 0
            nv[lo // K] = lo % K                           # the node that straddles the front edge keeps its slots before it
    valid = (torch.arange(K)[None, :] < nv[:, None]).reshape(-1)[:R]
    return nv, K, valid


# ============================================================================ masked linear
# name -> (flags, operands the call passes besides x / Wp / y)
EPIS = {
    "none": (0, ()),
    "pyg": (EPI_BIAS | EPI_AFFINE | EPI_RELU | EPI_RESIDUAL, ("bias", "scale", "shift", "res")),          # bias, mask, affine, relu, residual
    "dgl": (EPI_BIAS | EPI_RELU_PRE | EPI_AFFINE, ("bias", "scale", "shift")),                            # bias, relu, affine
    "leaky_res": (EPI_LEAKY | EPI_RESIDUAL, ("res",)),
    "respre": (EPI_RESIDUAL_PRE | EPI_AFFINE | EPI_RELU, ("scale", "shift", "res")),
    "bb": (EPI_BLOCK_BIAS | EPI_RELU_PRE | EPI_AFFINE, ("scale", "shift", "bbias")),                      # sn_masked_linear_blockbias_f32
    "bb_bias": (EPI_BIAS | EPI_BLOCK_BIAS | EPI_RELU_PRE | EPI_AFFINE, ("bias", "scale", "shift", "bbias")),
}
BB_ROWS = 13                      # rows per block-bias row: does not divide 16, so a tile straddles two bias rows
LINEAR_REJECTED = {"relu+leaky": (EPI_RELU | EPI_LEAKY, "exclusive"), "residual+residual_pre": (EPI_RESIDUAL | EPI_RESIDUAL_PRE, "not both")}


def linear_lds(p):
    d_in, d_out = p["d"]
    ops = EPIS[p["epi"]][1]
    off = p.get("off") or ()
    ld = lambda k, dense: p.get(k) or dense
    return d_in, d_out, ops, off, ld("ldx", d_in), ld("ldy", d_out), ld("ldr", d_out), ld("ldbb", d_out)


def false_clauses(p):
    """every false clause of `xv` and of `yv` (masked_linear_impl), in source order"""
    d_in, d_out, ops, off, ldx, ldy, ldr, ldbb = linear_lds(p)
    xv = [n for n, bad in (("d_in % 4", d_in % 4), ("ldx % 4", ldx % 4), ("x", "x" in off)) if bad]
    yv = [n for n, bad in (("d_out % 4", d_out % 4), ("ldy % 4", ldy % 4), ("y", "y" in off),
                           ("bias", "bias" in ops and "bias" in off), ("scale", "scale" in ops and "scale" in off),
                           ("shift", "shift" in ops and "shift" in off), ("residual", "res" in ops and "res" in off),
                           ("ldr % 4", "res" in ops and ldr % 4), ("bbias", "bbias" in ops and "bbias" in off),
                           ("ldbb % 4", "bbias" in ops and ldbb % 4)) if bad]
    return xv, yv


def lin_lds_blocks(R, d_in, d_out, cus):
    """-> (workgroups, why not) of a k_linear_lds launch"""
    nti, nto = cdiv(d_in, 16), cdiv(d_out, 16)
    if nti > 16 or nto > 16:
        return 0, "no lds: nti or nto > 16"
    if nti * nto * 1024 > 128 * 1024:
        return 0, "no lds: weight > 128K"
    want = cdiv(cdiv(R, 16), 4)
    return min(want, cus), None


def lds_kernel(nti, nto):
    return "k_linear_lds<%d,%d>" % ((8, 8) if nti <= 8 and nto <= 8 else (16, 8) if nto <= 8 else (8, 16) if nti <= 8 else (16, 16))


def grid_y(R, nto):
    """the grid.y split of k_linear: otc = ceil(nto / gridDim.y) output tiles per block"""
    gx = cdiv(R, 64)
    ny = 1 if gx >= 512 else cdiv(512, gx)
    gy = min(ny, nto)
    otc = cdiv(nto, gy)
    if ny == 1:
        return "ny = 1"
    if gy == nto:
        return "ny >= nto"
    if (gy - 1) * otc >= nto:
        return "1 < ny < nto: a trailing block gets no tile"
    return "1 < ny < nto: the last block gets fewer tiles" if nto % gy else "1 < ny < nto: even split"


def linear_branch(p, cus=CUS):
    """masked_linear_impl (ops.hip): kernel | xv | yv | LDS size and workgroup cap, or why not the LDS kernel | grid.y regime | operand"""
    d_in, d_out, ops, off, ldx, ldy, ldr, ldbb = linear_lds(p)
    R, nti, nto = p["R"], cdiv(d_in, 16), cdiv(d_out, 16)
    fx, fy = false_clauses(p)
    xv, yv = not fx, not fy
    tx, ty = "xv" if xv else "!xv: " + fx[0], "yv" if yv else "!yv: " + fy[0]
    b = lambda v: "true" if v else "false"
    why = "no lds: !xv or !yv" if not (xv and yv) else "no lds: R < 32" if R < LIN_LDS_MIN_ROWS else None
    if why is None:
        blocks, why = lin_lds_blocks(R, d_in, d_out, cus)
        if blocks:
            return " | ".join([lds_kernel(nti, nto), tx, ty, "lds > 64K (raised)" if nti * nto * 1024 > 64 * 1024 else "lds <= 64K",
                               "want < cus" if cdiv(cdiv(R, 16), 4) < cus else "capped at cus"])
    if nti >= 32 and nto <= 4 and R <= 8192:
        return " | ".join([f"k_linear_ksplit<{b(xv)},{b(yv)}>", tx, ty, why])
    return " | ".join([f"k_linear<{b(xv)},{b(yv)}>", tx, ty, why, grid_y(R, nto), "operand held once" if nti <= 8 else "kc loop"])


LINEAR_BRANCHES = (
    {f"k_linear_lds<{a},{b}>" for a in (8, 16) for b in (8, 16)} | {f"k_linear{k}<{a},{b}>" for k in ("", "_ksplit") for a in ("true", "false")
                                                                    for b in ("true", "false")} |
    {"xv", "yv"} | {"!xv: " + c for c in ("d_in % 4", "ldx % 4", "x")} |
    {"!yv: " + c for c in ("d_out % 4", "ldy % 4", "y", "bias", "scale", "shift", "residual", "ldr % 4", "bbias", "ldbb % 4")} |
    {"lds > 64K (raised)", "lds <= 64K", "want < cus", "capped at cus", "no lds: !xv or !yv", "no lds: R < 32", "no lds: nti or nto > 16",
     "no lds: weight > 128K", "ny = 1", "ny >= nto", "1 < ny < nto: a trailing block gets no tile",
     "1 < ny < nto: the last block gets fewer tiles", "1 < ny < nto: even split", "operand held once", "kc loop"})


def _L(d, R, epi="none", mask=None, **kw):
    p = dict(d=d, R=R, epi=epi, mask=mask, **kw)
    return Case("linear", None, **p)


def _rows(*specs):
    """(branch string written out, Case built from the parameters): the table states the branch, the predicate only confirms it"""
    out = []
    for branch, case in specs:
        case.branch = branch
        out.append(case)
    return out


_LDS88 = "k_linear_lds<8,8> | xv | yv | lds <= 64K | "
_KL = lambda xv, yv, tx, ty, why, gy, opnd: f"k_linear<{xv},{yv}> | {tx} | {ty} | {why} | {gy} | {opnd}"
_NOVEC, _FEW, _WIDE = "no lds: !xv or !yv", "no lds: R < 32", "no lds: nti or nto > 16"
_CL = dict(R=40, epi="pyg", mask="k7")                   # the clause rows: every operand of yv is passed, one clause false
_CLB = dict(R=40, epi="bb_bias")
LINEAR = _rows(
    # ---- kernel selection: k_linear_lds
    (_LDS88 + "want < cus", _L((16, 16), 32)),
    (_LDS88 + "want < cus", _L((128, 128), 33, "pyg", "k7")),
    (_LDS88 + "want < cus", _L((128, 128), 47, "dgl", "k1")),
    (_LDS88 + "want < cus", _L((128, 128), 4097, "leaky_res", "k7", cu_dependent=True)),          # want = 65
    (_LDS88 + "capped at cus", _L((16, 16), 32784, "respre", "k1")),                                # want = 513 > any CU count <= 512
    (_LDS88 + "want < cus", _L((16, 16), 48, "bb")),
    ("k_linear_lds<16,8> | xv | yv | lds <= 64K | want < cus", _L((144, 64), 33, "pyg", "k1")),
    ("k_linear_lds<16,8> | xv | yv | lds > 64K (raised) | want < cus", _L((256, 128), 47, "bb")),
    ("k_linear_lds<8,16> | xv | yv | lds <= 64K | want < cus", _L((64, 144), 40, "respre", "k7")),
    ("k_linear_lds<8,16> | xv | yv | lds > 64K (raised) | want < cus", _L((128, 256), 33, "dgl", "k7")),
    ("k_linear_lds<8,16> | xv | yv | lds <= 64K | want < cus", _L((64, 144), 32, "none", "k1")),
    ("k_linear_lds<16,16> | xv | yv | lds > 64K (raised) | want < cus", _L((144, 224), 47, "leaky_res", "k1", first16=True)),
    ("k_linear_lds<16,16> | xv | yv | lds > 64K (raised) | want < cus", _L((176, 176), 4097, "pyg", "k7", first16=True, cu_dependent=True)),
    ("k_linear_lds<16,16> | xv | yv | lds > 64K (raised) | want < cus", _L((176, 176), 33, "dgl", first16=True)),
    # ---- fall-through to k_linear
    (_KL("true", "true", "xv", "yv", "no lds: weight > 128K", "ny >= nto", "kc loop"), _L((256, 144), 33, "dgl", "k7")),
    (_KL("true", "true", "xv", "yv", _WIDE, "ny >= nto", "kc loop"), _L((300, 72), 47, "pyg", "k1")),
    (_KL("true", "true", "xv", "yv", _FEW, "ny >= nto", "kc loop"), _L((144, 64), 16, "respre")),             # nti = 9: 8 + 1
    (_KL("true", "true", "xv", "yv", _FEW, "ny >= nto", "kc loop"), _L((300, 72), 17, "leaky_res", "k7")),    # nti = 19: 8 + 8 + 3
    (_KL("true", "true", "xv", "yv", _WIDE, "1 < ny < nto: the last block gets fewer tiles", "kc loop"), _L((300, 72), 12800, "bb")),
    (_KL("true", "true", "xv", "yv", _WIDE, "1 < ny < nto: a trailing block gets no tile", "kc loop"), _L((300, 72), 8193, "dgl", "k7")),
    (_KL("true", "true", "xv", "yv", _WIDE, "1 < ny < nto: even split", "kc loop"), _L((300, 96), 12800, "none", "k1")),
    (_KL("false", "false", "!xv: d_in % 4", "!yv: d_out % 4", _NOVEC, "ny = 1", "operand held once"), _L((5, 3), 32769, "pyg", "k1")),
    (_KL("true", "false", "xv", "!yv: d_out % 4", _NOVEC, "ny >= nto", "operand held once"), _L((64, 30), 17, "bb")),
    (_KL("false", "true", "!xv: d_in % 4", "yv", _NOVEC, "ny >= nto", "operand held once"), _L((30, 64), 100, "leaky_res", "k7")),
    (_KL("false", "false", "!xv: d_in % 4", "!yv: d_out % 4", _NOVEC, "ny >= nto", "kc loop"), _L((301, 70), 33, "respre", "k1")),
    (_KL("true", "false", "xv", "!yv: d_out % 4", _NOVEC, "ny >= nto", "kc loop"), _L((144, 30), 33, "dgl", "k7")),
    # ---- k_linear_ksplit: nti >= 32, nto <= 4, R <= 8192
    (f"k_linear_ksplit<true,true> | xv | yv | {_FEW}", _L((512, 4), 1)),
    (f"k_linear_ksplit<true,true> | xv | yv | {_WIDE}", _L((512, 4), 8192, "dgl", "k1")),
    (_KL("true", "true", "xv", "yv", _WIDE, "ny >= nto", "kc loop"), _L((512, 4), 8193)),
    (f"k_linear_ksplit<true,false> | xv | !yv: d_out % 4 | {_NOVEC}", _L((600, 33), 17, "pyg", "k7")),
    (f"k_linear_ksplit<true,true> | xv | yv | {_FEW}", _L((2048, 20), 17, "leaky_res", "k1")),
    (f"k_linear_ksplit<false,true> | !xv: d_in % 4 | yv | {_NOVEC}", _L((602, 64), 17, "respre", "k7")),
    (f"k_linear_ksplit<false,false> | !xv: d_in % 4 | !yv: d_out % 4 | {_NOVEC}", _L((602, 33), 17, "bb")),
    (f"k_linear_ksplit<true,true> | xv | yv | {_WIDE}", _L((512, 64), 40, "bb_bias")),
    (f"k_linear_ksplit<true,true> | xv | yv | {_WIDE}", _L((608, 48), 33, "none", "k7")),
    # ---- every clause of xv and yv falsified alone on a vectorisable (128, 128)
    (_KL("false", "true", "!xv: ldx % 4", "yv", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), ldx=129, alone=True, **_CL)),
    (_KL("false", "true", "!xv: x", "yv", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), off=("x",), alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: ldy % 4", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), ldy=129, alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: y", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), off=("y",), alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: bias", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), off=("bias",), alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: scale", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), off=("scale",), alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: shift", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), off=("shift",), alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: residual", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), off=("res",), alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: ldr % 4", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), ldr=129, alone=True, **_CL)),
    (_KL("true", "false", "xv", "!yv: bbias", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), off=("bbias",), alone=True, **_CLB)),
    (_KL("true", "false", "xv", "!yv: ldbb % 4", _NOVEC, "ny >= nto", "operand held once"), _L((128, 128), ldbb=129, alone=True, **_CLB)),
    # ---- strided but vector: stays on the LDS kernel
    (_LDS88 + "want < cus", _L((128, 128), ldx=256, **_CL)),
    (_LDS88 + "want < cus", _L((128, 128), ldy=132, **_CL)),
    (_LDS88 + "want < cus", _L((128, 128), ldr=132, **_CL)),
    (_LDS88 + "want < cus", _L((128, 128), ldbb=132, **_CLB)),
    (_LDS88 + "want < cus", _L((128, 128), ldx=132, ldy=136, ldr=140, **_CL)),
)


def linear_gen(case):
    """-> dict of float32 CPU tensors (x, W and the operands of the row's epilogue), nv / K / valid"""
    p = case.p
    g = rng(case)
    d_in, d_out = p["d"]
    R = p["R"]
    rn = lambda *s: torch.randn(*s, generator=g)
    t = {"x": rn(R, d_in), "W": rn(d_out, d_in) / d_in ** 0.5}
    for name in EPIS[p["epi"]][1]:
        t[name] = {"bias": lambda: rn(d_out), "scale": lambda: 0.5 + torch.rand(d_out, generator=g), "shift": lambda: rn(d_out),
                   "res": lambda: rn(R, d_out), "bbias": lambda: rn(cdiv(R, BB_ROWS), d_out)}[name]()
    t["nv"], t["K"], t["valid"] = mask_rows(p["mask"], R, g)
    assert not ("bbias" in t and t["nv"] is not None), "the block-bias entry point takes no mask"
    return t


def linear_ref(flags, t, dt, rows=None):
    """the epilogue order of k_linear / k_linear_ksplit / k_linear_lds: bias, block bias, residual_pre, relu_pre, affine, relu | leaky,
    residual; invalid rows are zero"""
    c = lambda n: t[n].to(dt)
    R = t["x"].shape[0]
    v = c("x") @ c("W").t()
    if flags & EPI_BIAS:
        v = v + c("bias")
    if flags & EPI_BLOCK_BIAS:
        v = v + c("bbias")[torch.arange(R) // BB_ROWS]
    if flags & EPI_RESIDUAL_PRE:
        v = v + c("res")
    if flags & EPI_RELU_PRE:
        v = v.clamp_min(0)
    if flags & EPI_AFFINE:
        v = v * c("scale") + c("shift")
    if flags & EPI_RELU:
        v = v.clamp_min(0)
    if flags & EPI_LEAKY:
        v = torch.where(v > 0, v, v * torch.tensor(0.01, dtype=F32).to(dt))
    if flags & EPI_RESIDUAL:
        v = v + c("res")
    return torch.where(t["valid"][:, None], v, torch.zeros((), dtype=dt))


# ============================================================================ column statistics / train-mode BatchNorm statistics
def stats_ref(z, valid, dt, gamma=None, beta=None, rmean=None, rvar=None):
    """-> dict(mean, var (biased), count, rstd, scale, shift, rmean, rvar) of the valid rows; no valid row: mean = var = 0; the running
    variance is the unbiased one where there is more than one row (k_bn_train_finish1)"""
    zv = z.to(dt)[valid]
    n, C = zv.shape
    if n:
        mean, var = zv.mean(0), (zv.var(0, unbiased=False) if n > 1 else torch.zeros(C, dtype=dt))
    else:
        mean, var = torch.zeros(C, dtype=dt), torch.zeros(C, dtype=dt)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(BN_EPS, dtype=F32).to(dt))
    scale = rstd if gamma is None else gamma.to(dt) * rstd
    shift = -mean * scale if beta is None else beta.to(dt) - mean * scale
    out = dict(mean=mean, var=var, count=torch.tensor([float(n)], dtype=dt), rstd=rstd, scale=scale, shift=shift)
    if rmean is not None:
        m = torch.tensor(BN_MOMENTUM, dtype=F32).to(dt)
        unb = var * (n / (n - 1.0)) if n > 1 else var
        out["rmean"], out["rvar"] = (1 - m) * rmean.to(dt) + m * mean, (1 - m) * rvar.to(dt) + m * unb
    return out


def stats_mask(p):
    """-> (nvalid or None, K, bool [R]) of a statistics row; hand-placed for the first-valid-row search of k_colstats_moments"""
    R, mode = p["R"], p.get("mask")
    if mode is None:
        return None, 0, torch.ones(R, dtype=torch.bool)
    g = rng("stats-mask-%d-%s" % (R, mode))
    if mode in ("k1z", "none_valid", "one_valid"):
        K = 1
        nv = torch.randint(0, 2, (R,), generator=g, dtype=torch.int32)
        if mode != "k1z":
            nv.zero_()
        if mode == "one_valid":
            nv[R * 2 // 3] = 1
    else:                   # "tail": K = 5 over 640 rows = five 128-row blocks of k_colstats_moments
        K = 5
        assert R == 640
        nv = torch.randint(1, K + 1, (R // K,), generator=g, dtype=torch.int32)
        nv[25], nv[26], nv[27] = 2, 0, 3           # row 128 (block 1) is slot 3 of node 25: invalid; node 26 empty; node 27 is found
        nv[51:77] = 0                              # rows 255 .. 384: block 2 (rows 256 .. 383) has no valid row
    valid = (torch.arange(K)[None, :] < nv[:, None]).reshape(-1)[:R]
    return nv, K, valid


def colstats_blocks(R):
    return min(max(cdiv(R, 64), 1), 2048)


def colstats_branch(p, cus=CUS):
    """sn_masked_colstats_f32: reduction levels | block clamp | column passes | where the count column of k_colstats_reduce sits | ldx | mask"""
    R, C = p["R"], p["C"]
    nblk = colstats_blocks(R)
    two = nblk > 2 * CS_SPLIT
    valid = stats_mask(p)[2]
    return " | ".join(["two-level reduce" if two else "single-level reduce", "2048-block clamp" if cdiv(R, 64) > 2048 else "blocks = cdiv(R, 64)",
                       "C <= 64" if C <= 64 else "C > 256" if C > 256 else "C > 64"] +
                      (["count column in a block of its own" if C % 256 == 0 else "count column shares a block"] if two else []) +
                      ["ldx > C" if p.get("ld") else "dense", "no mask" if p.get("mask") is None else "count 0" if not valid.any() else "masked"])


COLSTATS_BRANCHES = {"two-level reduce", "single-level reduce", "2048-block clamp", "blocks = cdiv(R, 64)", "C <= 64", "C > 64", "C > 256",
                     "count column in a block of its own", "count column shares a block", "ldx > C", "dense", "no mask", "count 0", "masked"}


def bn_stats_blocks(R):
    nfull = colstats_blocks(R)
    return nfull // 2 if nfull > 1 else 1


def bn_stats_branch(p, cus=CUS):
    """sn_bn_train_stats_f32: k_bn_train_finish1 width | block clamp | column passes | ldx | what the first-valid-row search meets"""
    R, C = p["R"], p["C"]
    nblk = bn_stats_blocks(R)
    rpb = cdiv(max(R, 1), nblk)
    nv, K, valid = stats_mask(p)
    out = ["finish1<64>" if nblk > 256 else "finish1<16>", "2048-block clamp" if cdiv(R, 64) > 2048 else "blocks from cdiv(R, 64)",
           "C <= 64" if C <= 64 else "C > 256" if C > 256 else "C > 64", "ldx > C" if p.get("ld") else "dense"]
    if nv is None:
        return " | ".join(out + ["no mask"])
    nval = int(valid.sum())
    tail = dead = False
    for b in range(nblk):
        r0, r1 = b * rpb, min((b + 1) * rpb, R)
        if r0 < r1:
            tail |= (not bool(valid[r0])) and bool(valid[r0:r1].any())
            dead |= not bool(valid[r0:r1].any())
    out.append("K = 1 with zeros" if K == 1 else "K > 1")
    if tail:
        out.append("a block starts in a node's invalid tail")
    if dead and nval:
        out.append("a block with no valid row")
    out.append("no valid row at all" if nval == 0 else "one valid row" if nval == 1 else "n > 1")
    return " | ".join(out)


BN_STATS_BRANCHES = {"finish1<64>", "finish1<16>", "2048-block clamp", "blocks from cdiv(R, 64)", "C <= 64", "C > 64", "C > 256", "ldx > C", "dense",
                     "no mask", "K = 1 with zeros", "K > 1", "a block starts in a node's invalid tail", "a block with no valid row",
                     "no valid row at all", "one valid row", "n > 1"}

# (R, C, extras): one list for both entry points
_STATS = [(1, 44, {}), (63, 1, {}), (64, 64, {}), (65, 65, {}), (65, 255, {}), (63, 256, {}), (37, 300, {}), (2049, 44, {}),
          (2049, 255, {}), (2049, 256, {}), (32769, 4, {}), (32897, 4, {}), (131073, 4, {}), (65, 44, dict(ld=47)), (2049, 65, dict(ld=68, mask="k1z")),
          (640, 44, dict(mask="tail")), (640, 70, dict(mask="k1z")), (300, 44, dict(mask="none_valid")), (300, 20, dict(mask="one_valid")),
          (37, 4, dict(ill=True)), (4097, 4, dict(ill=True)), (131073, 4, dict(ill=True, mask="k1z"))]


def _stats_cases(op, pred):
    out = []
    for R, C, kw in _STATS:
        p = dict(R=R, C=C, ld=kw.get("ld"), mask=kw.get("mask"), ill=kw.get("ill", False))
        out.append(Case(op, pred(p), **p))
    return out


COLSTATS = _stats_cases("colstats", colstats_branch)
BN_STATS = _stats_cases("bn_stats", bn_stats_branch) + [
    Case("bn_stats", bn_stats_branch(p), **p) for p in (dict(R=65, C=44, ld=None, mask=None, ill=False, noaffine=True),
                                                         dict(R=640, C=44, ld=None, mask="tail", ill=False, norunning=True))]
# the branch strings the rows above were written for (the CPU test pins them: a change of a predicate or of _STATS has to show up here)
STATS_PINNED = {
    "colstats-R2049-C256": "two-level reduce | blocks = cdiv(R, 64) | C > 64 | count column in a block of its own | dense | no mask",
    "colstats-R2049-C255": "two-level reduce | blocks = cdiv(R, 64) | C > 64 | count column shares a block | dense | no mask",
    "colstats-R131073-C4": "two-level reduce | 2048-block clamp | C <= 64 | count column shares a block | dense | no mask",
    "colstats-R65-C44-ld47": "single-level reduce | blocks = cdiv(R, 64) | C <= 64 | ldx > C | no mask",
    "colstats-R37-C300": "single-level reduce | blocks = cdiv(R, 64) | C > 256 | dense | no mask",
    "colstats-R300-C44-masknone_valid": "single-level reduce | blocks = cdiv(R, 64) | C <= 64 | dense | count 0",
    "bn_stats-R32769-C4": "finish1<16> | blocks from cdiv(R, 64) | C <= 64 | dense | no mask",          # 513 // 2 = 256 blocks: not > 256
    "bn_stats-R32897-C4": "finish1<64> | blocks from cdiv(R, 64) | C <= 64 | dense | no mask",          # 515 // 2 = 257
    "bn_stats-R131073-C4": "finish1<64> | 2048-block clamp | C <= 64 | dense | no mask",
    "bn_stats-R2049-C44": "finish1<16> | blocks from cdiv(R, 64) | C <= 64 | dense | no mask",
    "bn_stats-R640-C44-masktail": "finish1<16> | blocks from cdiv(R, 64) | C <= 64 | dense | K > 1 | a block starts in a node's invalid tail | "
                                  "a block with no valid row | n > 1",
    "bn_stats-R640-C70-maskk1z": "finish1<16> | blocks from cdiv(R, 64) | C > 64 | dense | K = 1 with zeros | a block starts in a node's invalid tail | "
                                 "n > 1",
    "bn_stats-R300-C44-masknone_valid": "finish1<16> | blocks from cdiv(R, 64) | C <= 64 | dense | K = 1 with zeros | no valid row at all",
    "bn_stats-R300-C20-maskone_valid": "finish1<16> | blocks from cdiv(R, 64) | C <= 64 | dense | K = 1 with zeros | a block starts in a node's invalid "
                                       "tail | a block with no valid row | one valid row",
}


def stats_gen(case):
    """-> x [R, C] float32, (nv, K, valid), gamma, beta, running mean / var (None where the row passes NULL).  `ill`: columns of mean
    1000 and unit variance."""
    p = case.p
    g = rng(case)
    R, C = p["R"], p["C"]
    x = torch.randn(R, C, generator=g)
    if p.get("ill"):
        x = (x.double() + 1000.0).float()
    else:
        x = x * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    aff, run = not p.get("noaffine"), not p.get("norunning")
    return dict(x=x, mask=stats_mask(p), gamma=0.5 + torch.rand(C, generator=g) if aff else None, beta=torch.randn(C, generator=g) if aff else None,
                rmean=torch.randn(C, generator=g) * 0.1 if run else None, rvar=torch.rand(C, generator=g) + 0.5 if run else None)


# ============================================================================ linear + BatchNorm statistics
def linear_bn_branch(p, cus=CUS):
    """sn_linear_bn_train_f32: the fused k_linear_lds<8,8,STATS> launch, or the first reason (in source order) for the two-call fallback"""
    d_in, d_out = p["d"]
    off = p.get("off") or ()
    ldx, ldz, R = p.get("ldx") or d_in, p.get("ldz") or d_out, p["R"]
    for name, bad in (("d_in % 4", d_in % 4), ("ldx % 4", ldx % 4), ("x", "x" in off), ("d_out % 4", d_out % 4), ("ldz % 4", ldz % 4),
                      ("z", "z" in off), ("bias", not p.get("nobias") and "bias" in off), ("d_out > 128", d_out > 128), ("d_in > 128", d_in > 128),
                      ("R < 32", R < LIN_LDS_MIN_ROWS)):
        if bad:
            return "fallback: " + name
    nblk = lin_lds_blocks(R, d_in, d_out, cus)[0]
    return "k_linear_lds<8,8,STATS> | " + ("want < cus" if cdiv(cdiv(R, 16), 4) < cus else "capped at cus") + " | " + \
        ("finish1<64>" if nblk > 256 else "finish1<16>")


# (finish1<64> behind the fused launch needs more than 256 workgroups, i.e. more than 256 CUs: sn_bn_train_stats_f32's rows run it here)
LINEAR_BN_BRANCHES = {"k_linear_lds<8,8,STATS>", "want < cus", "capped at cus", "finish1<16>"} | {
    "fallback: " + n for n in ("d_in % 4", "ldx % 4", "x", "d_out % 4", "ldz % 4", "z", "bias", "d_out > 128", "d_in > 128", "R < 32")}


def _LB(d, R, mask=None, **kw):
    p = dict(d=d, R=R, mask=mask, **kw)
    return Case("linear_bn", None, **p)


_FUSED = "k_linear_lds<8,8,STATS> | want < cus | finish1<16>"
LINEAR_BN = _rows(
    (_FUSED, _LB((16, 16), 32)),
    (_FUSED, _LB((12, 12), 40, "k7")),
    (_FUSED, _LB((128, 128), 40, "k1")),
    (_FUSED, _LB((128, 128), 4097, "k7", cu_dependent=True)),
    (_FUSED, _LB((16, 16), 4097, "k1", noaffine=True, cu_dependent=True)),
    (_FUSED, _LB((12, 12), 32, "k7", norunning=True)),
    (_FUSED, _LB((128, 128), 32, nobias=True, ldx=132, ldz=136)),
    ("k_linear_lds<8,8,STATS> | capped at cus | finish1<16>", _LB((16, 16), 32784, "k7", cu_dependent=True)),           # (finish1<64> above 256 CUs)
    ("fallback: R < 32", _LB((16, 16), 31, "k7")),
    ("fallback: x", _LB((16, 16), 40, "k1", off=("x",))),
    ("fallback: ldz % 4", _LB((16, 16), 40, ldz=17)),
    ("fallback: d_out > 128", _LB((16, 132), 40, "k7")),
    ("fallback: d_in > 128", _LB((132, 16), 40, "k1")),
    ("fallback: d_out % 4", _LB((16, 14), 40, "k7")),
    ("fallback: d_in % 4", _LB((14, 16), 40)),
    ("fallback: ldx % 4", _LB((16, 16), 40, "k1", ldx=17)),
    ("fallback: z", _LB((16, 16), 40, off=("z",), noaffine=True, norunning=True)),
    ("fallback: bias", _LB((16, 16), 40, "k7", off=("bias",))),
)


def linear_bn_gen(case):
    p = case.p
    g = rng(case)
    d_in, d_out = p["d"]
    R = p["R"]
    t = {"x": torch.randn(R, d_in, generator=g), "W": torch.randn(d_out, d_in, generator=g) / d_in ** 0.5}
    if not p.get("nobias"):
        t["bias"] = torch.randn(d_out, generator=g)
    t["nv"], t["K"], t["valid"] = mask_rows(p["mask"], R, g)
    aff, run = not p.get("noaffine"), not p.get("norunning")
    t.update(gamma=0.5 + torch.rand(d_out, generator=g) if aff else None, beta=torch.randn(d_out, generator=g) if aff else None,
             rmean=torch.randn(d_out, generator=g) * 0.1 if run else None, rvar=torch.rand(d_out, generator=g) + 0.5 if run else None)
    return t


def linear_bn_ref(t, dt):
    z = linear_ref(EPI_BIAS if "bias" in t else 0, t, dt)
    return z, stats_ref(z, t["valid"], dt, t["gamma"], t["beta"], t["rmean"], t["rvar"])


# ============================================================================ GIN / GINE aggregations on one hand-built batch
def agg_batch():
    """-> (batch int64 [N], edge_index int64 [2, E], sizes).  Graph 0 is written by hand: node 0 isolated (no edge at all), node 1 in-degree 1, node 2
    in-degree 3, node 3 in-degree 5, node 4 a double edge 5 -> 4, node 6 a self loop.  Graph 1 has 70 nodes (too many for the slab
    kernel's LDS at 64 vector columns), graph 2 is empty; the rest are random; N = 601 (odd, over one 512-node round)."""
    g = rng("agg-batch")
    sizes = [9, 70, 0, 37, 50, 41, 23, 50, 33, 48, 29, 50, 44, 38, 50, 29]
    assert sum(sizes) == 601
    src = [8, 4, 1, 7, 4, 1, 5, 7, 8, 5, 5, 6, 2]
    dst = [1, 2, 2, 2, 3, 3, 3, 3, 3, 4, 4, 6, 7]
    base = 9
    for n in sizes[1:]:
        if n:
            ring = torch.arange(n)
            e = torch.randint(0, n, (2, 2 * n), generator=g)
            s, d = torch.cat([ring, (ring + 1) % n, e[0]]), torch.cat([(ring + 1) % n, ring, e[1]])
            src += (s + base).tolist()
            dst += (d + base).tolist()
        base += n
    ei = torch.tensor([src, dst], dtype=torch.int64)
    ei = ei[:, torch.randperm(ei.shape[1], generator=g)]              # edge ids are not sorted by destination
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return batch, ei, sizes


def agg_csr(batch, ei, sizes):
    """the in-edge CSR in edge-id order per destination: rowptr [N + 1], col (source), eperm (edge id), graph_ptr [B + 1]"""
    N = batch.numel()
    eperm = torch.sort(ei[1], stable=True)[1]
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.bincount(ei[1], minlength=N).cumsum(0)
    gp = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    gp[1:] = torch.tensor(sizes).cumsum(0)
    return rowptr, ei[0][eperm], eperm, gp


def agg_ref(x, csr, dt, eps=None, ea=None, negate=False, plus=None):
    """sum over the in-edges IN EDGE ORDER (one addition per round, starting from 0), then the self term (1 + eps) * x with the product
    rounded on its own, then the negation, then `plus`.  ea: GINE's message relu(x_j + e)."""
    rowptr, col, eperm, _ = csr
    x = x.to(dt)
    deg = rowptr[1:] - rowptr[:-1]
    acc = torch.zeros_like(x)
    for k in range(int(deg.max()) if deg.numel() else 0):
        rows = (deg > k).nonzero()[:, 0]
        e = rowptr[rows] + k
        m = x[col[e]]
        if ea is not None:
            m = (m + ea.to(dt)[eperm[e]]).clamp_min(0)
        acc[rows] = acc[rows] + m
    sc = torch.ones((), dtype=F32) + (eps if eps is not None else torch.zeros((), dtype=F32))          # 1.f + *eps, in float32
    prod = x * sc.to(dt)
    r = acc + prod
    if negate:
        r = 0 - r
    if plus is not None:
        r = r + plus.to(dt)
    return r


def gin_group(FV):
    return 256 if FV > 128 else 128 if FV > 64 else 64 if FV > 32 else 32


def gin_branch(p, cus=CUS):
    """sn_gin_aggregate_f32 / sn_gin_aggregate_add_f32: vector type (and the first clause that refuses float4) | column-group width"""
    F, off = p["F"], p.get("off") or ()
    why = "F % 4" if F % 4 else "x misaligned" if "x" in off else "out misaligned" if "out" in off else None
    if why is None:
        return f"k_gin_gather<float4,{gin_group(F // 4)}>" + (" | plus" if p.get("plus") else "")
    return f"k_gin_gather<float,{gin_group(F)}> | {why}"


GIN_BRANCHES = {f"k_gin_gather<{t},{w}>" for t in ("float", "float4") for w in (32, 64, 128, 256)} | {"F % 4", "x misaligned", "out misaligned"}
GIN_ADD_BRANCHES = {f"k_gin_gather<float4,{w}>" for w in (32, 64, 128, 256)} | {"plus"}


def _G(op, **p):
    return Case(op, None, **p)


_GF = lambda w, why: f"k_gin_gather<float,{w}> | {why}"
GIN = _rows(
    (_GF(32, "F % 4"), _G("gin", F=1)),
    (_GF(32, "x misaligned"), _G("gin", F=32, off=("x",))),
    (_GF(64, "F % 4"), _G("gin", F=33, negate=True)),
    (_GF(64, "out misaligned"), _G("gin", F=64, off=("out",))),
    (_GF(128, "F % 4"), _G("gin", F=65, noeps=True)),
    (_GF(128, "x misaligned"), _G("gin", F=128, off=("x",))),
    (_GF(128, "out misaligned"), _G("gin", F=128, off=("out",), negate=True)),
    (_GF(256, "F % 4"), _G("gin", F=129)),
    (_GF(256, "F % 4"), _G("gin", F=257, negate=True, noeps=True)),
    (_GF(256, "x misaligned"), _G("gin", F=300, off=("x", "out"))),
    ("k_gin_gather<float4,32>", _G("gin", F=4)),
    ("k_gin_gather<float4,32>", _G("gin", F=128, negate=True)),
    ("k_gin_gather<float4,64>", _G("gin", F=132)),
    ("k_gin_gather<float4,64>", _G("gin", F=256, noeps=True)),
    ("k_gin_gather<float4,128>", _G("gin", F=260)),
    ("k_gin_gather<float4,128>", _G("gin", F=512)),
    ("k_gin_gather<float4,256>", _G("gin", F=516, negate=True)),
    ("k_gin_gather<float4,256>", _G("gin", F=1028)),
    ("k_gin_gather<float4,256>", _G("gin", F=1200, noeps=True)),
)
GIN_ADD = _rows(
    ("k_gin_gather<float4,32> | plus", _G("gin_add", F=128, plus=True)),
    ("k_gin_gather<float4,64> | plus", _G("gin_add", F=256, plus=True, noeps=True)),
    ("k_gin_gather<float4,128> | plus", _G("gin_add", F=512, plus=True)),
    ("k_gin_gather<float4,256> | plus", _G("gin_add", F=1028, plus=True)),
)
SLAB_LDS = 64 * 1024


def slab_branch(p, cus=CUS):
    """sn_gin_aggregate_slab_f32: vector type | column chunks | which arm of k_gin_slab the batch's graphs take in this launch"""
    F, off = p["F"], p.get("off") or ()
    vec = F % 4 == 0 and "x" not in off and "out" not in off
    FV, CH, sz = (F // 4, min(F // 4, 64), 16) if vec else (F, min(F, 256), 4)
    nchunk = cdiv(FV, CH)
    batch, ei, sizes = agg_batch()
    rowptr, _, _, gp = agg_csr(batch, ei, sizes)
    arms = set()
    for b, n in enumerate(sizes):
        if n:
            ne = int(rowptr[gp[b + 1]] - rowptr[gp[b]])
            for c in range(nchunk):
                arms.add("lds" if n * min(FV - c * CH, CH) * sz + (n + 1 + ne) * 4 <= SLAB_LDS else "fallback")
    return " | ".join(["k_gin_slab<float4>" if vec else "k_gin_slab<float>", "nchunk > 1" if nchunk > 1 else "nchunk = 1",
                       {("lds",): "every graph in LDS", ("fallback", "lds"): "LDS arm and fallback arm in one launch"}[tuple(sorted(arms))]])


SLAB_BRANCHES = {"k_gin_slab<float4>", "k_gin_slab<float>", "nchunk > 1", "nchunk = 1", "every graph in LDS", "LDS arm and fallback arm in one launch"}
_BOTH = "LDS arm and fallback arm in one launch"
SLAB = _rows(
    ("k_gin_slab<float> | nchunk = 1 | every graph in LDS", _G("slab", F=33)),
    (f"k_gin_slab<float> | nchunk > 1 | {_BOTH}", _G("slab", F=257, negate=True)),
    (f"k_gin_slab<float> | nchunk > 1 | {_BOTH}", _G("slab", F=300, off=("x",), noeps=True)),
    ("k_gin_slab<float4> | nchunk = 1 | every graph in LDS", _G("slab", F=128)),
    (f"k_gin_slab<float4> | nchunk = 1 | {_BOTH}", _G("slab", F=256, negate=True)),
    (f"k_gin_slab<float4> | nchunk > 1 | {_BOTH}", _G("slab", F=260)),
    (f"k_gin_slab<float4> | nchunk > 1 | {_BOTH}", _G("slab", F=300, noeps=True)),
)


def gine_branch(p, cus=CUS):
    """sn_gine_aggregate_f32: vector type (and the first clause that refuses float4) | the XCD chunk rule of the grid lambda"""
    C, off = p["C"], p.get("off") or ()
    why = "C % 4" if C % 4 else next((f"{n} misaligned" for n in ("x", "ea", "out") if n in off), None)
    cols = C if why else C // 4
    return " | ".join(["k_gine_gather<float>" if why else "k_gine_gather<float4>"] + ([why] if why else []) + ["cols >= 64" if cols >= 64 else "cols < 64"])


GINE_BRANCHES = {"k_gine_gather<float>", "k_gine_gather<float4>", "C % 4", "x misaligned", "ea misaligned", "out misaligned", "cols >= 64", "cols < 64"}
GINE = _rows(
    ("k_gine_gather<float4> | cols < 64", _G("gine", C=20)),
    ("k_gine_gather<float4> | cols >= 64", _G("gine", C=256, noeps=True)),
    ("k_gine_gather<float4> | cols >= 64", _G("gine", C=260)),
    ("k_gine_gather<float> | C % 4 | cols < 64", _G("gine", C=1)),
    ("k_gine_gather<float> | C % 4 | cols < 64", _G("gine", C=37, noeps=True)),
    ("k_gine_gather<float> | C % 4 | cols < 64", _G("gine", C=63)),
    ("k_gine_gather<float> | C % 4 | cols >= 64", _G("gine", C=65)),
    ("k_gine_gather<float> | ea misaligned | cols >= 64", _G("gine", C=128, off=("ea",))),
    ("k_gine_gather<float> | x misaligned | cols < 64", _G("gine", C=20, off=("x",))),
    ("k_gine_gather<float> | out misaligned | cols < 64", _G("gine", C=44, off=("out",))),
)


def agg_gen(case, N, E):
    p = case.p
    g = rng(case)
    W = p.get("F") or p["C"]
    t = {"x": torch.randn(N, W, generator=g), "eps": None if p.get("noeps") else torch.tensor(0.1 + 0.05 * (W % 7), dtype=F32)}
    if case.op == "gine":
        t["ea"] = torch.randn(E, W, generator=g)
    if p.get("plus"):
        t["plus"] = torch.randn(N, W, generator=g)
    return t


# ============================================================================ segment pool
def pool_rl(C):
    cw = 1
    while cw < C and cw < 256:
        cw <<= 1
    return 256 // cw


def pool_lens(C):
    rl = pool_rl(C)
    return [0, 1, 8 * rl - 1, 0, 8 * rl, 8 * rl + 1, 24 * rl + 3, 2, 0]


def pool_branch(p, cus=CUS):
    """k_segment_pool: row lanes | column chunks over blockIdx.y | which loops the segments of the row run | mode"""
    C = p["C"]
    rl, lens = pool_rl(C), pool_lens(C)
    return " | ".join([f"RL = {rl}", "gridDim.y > 1" if C > 256 else "gridDim.y = 1"] +
                      (["eight loads in flight"] if any(n > 7 * rl for n in lens) else []) +
                      (["tail loop only"] if any(0 < n <= 7 * rl for n in lens) else []) +
                      (["empty segment"] if 0 in lens else []) + [p["mode"]])


POOL_BRANCHES = {"RL = 256", "RL = 8", "RL = 1", "gridDim.y > 1", "gridDim.y = 1", "eight loads in flight", "tail loop only", "empty segment", "add", "mean"}
POOL = [Case("pool", f"RL = {pool_rl(C)} | gridDim.y {'> 1' if C > 256 else '= 1'} | eight loads in flight | tail loop only | empty segment | {m}",
             C=C, mode=m) for C in (1, 20, 256, 300) for m in ("add", "mean")]


def pool_gen(case):
    C = case.p["C"]
    lens = pool_lens(C)
    return torch.randn(sum(lens), C, generator=rng(case)), lens


def pool_ref(x, lens, mode, dt):
    out, lo = [], 0
    for n in lens:
        s = x[lo:lo + n].to(dt).sum(0)
        out.append(s * (torch.ones((), dtype=F32) / float(max(n, 1))).to(dt) if mode == "mean" else s)      # the kernel scales by 1.f / n
        lo += n
    return torch.stack(out)


# ============================================================================ registry
class Op:
    def __init__(self, cases, predicate, branches):
        self.cases, self.predicate, self.branches = cases, predicate, branches


OPS = {"linear": Op(LINEAR, linear_branch, LINEAR_BRANCHES), "linear_bn": Op(LINEAR_BN, linear_bn_branch, LINEAR_BN_BRANCHES),
       "colstats": Op(COLSTATS, colstats_branch, COLSTATS_BRANCHES), "bn_stats": Op(BN_STATS, bn_stats_branch, BN_STATS_BRANCHES),
       "gin": Op(GIN, gin_branch, GIN_BRANCHES), "gin_add": Op(GIN_ADD, gin_branch, GIN_ADD_BRANCHES), "slab": Op(SLAB, slab_branch, SLAB_BRANCHES),
       "gine": Op(GINE, gine_branch, GINE_BRANCHES), "pool": Op(POOL, pool_branch, POOL_BRANCHES)}

# The branches the grid was written for (none of them was reached by an op-level test before), each with a row that takes it and the
# name in that row's branch string that says so; tests/test_ops_cases_cpu.py checks the list against the tables.
NAMED = [
    ("k_linear_lds<16,16>", "linear-d144x224-R47-epileaky_res-maskk1-first16", "k_linear_lds<16,16>"),
    ("k_linear_lds<16,16>", "linear-d176x176-R4097-epipyg-maskk7-first16-cu_dependent", "k_linear_lds<16,16>"),
    ("k_linear_ksplit<false,true>", "linear-d602x64-R17-epirespre-maskk7", "k_linear_ksplit<false,true>"),
    ("k_linear_ksplit<false,false>", "linear-d602x33-R17-epibb", "k_linear_ksplit<false,false>"),
    ("k_linear_ksplit<true,false> on a second shape", "linear-d600x33-R17-epipyg-maskk7", "k_linear_ksplit<true,false>"),
    ("xv falsified by ldx alone", "linear-d128x128-R40-epipyg-maskk7-ldx129-alone", "!xv: ldx % 4"),
    ("xv falsified by the pointer alone", "linear-d128x128-R40-epipyg-maskk7-offx-alone", "!xv: x"),
    ("yv: ldy", "linear-d128x128-R40-epipyg-maskk7-ldy129-alone", "!yv: ldy % 4"),
    ("yv: y", "linear-d128x128-R40-epipyg-maskk7-offy-alone", "!yv: y"),
    ("yv: bias", "linear-d128x128-R40-epipyg-maskk7-offbias-alone", "!yv: bias"),
    ("yv: scale", "linear-d128x128-R40-epipyg-maskk7-offscale-alone", "!yv: scale"),
    ("yv: shift", "linear-d128x128-R40-epipyg-maskk7-offshift-alone", "!yv: shift"),
    ("yv: residual", "linear-d128x128-R40-epipyg-maskk7-offres-alone", "!yv: residual"),
    ("yv: ldr", "linear-d128x128-R40-epipyg-maskk7-ldr129-alone", "!yv: ldr % 4"),
    ("yv: bbias", "linear-d128x128-R40-epibb_bias-offbbias-alone", "!yv: bbias"),
    ("yv: ldbb", "linear-d128x128-R40-epibb_bias-ldbb129-alone", "!yv: ldbb % 4"),
    ("ldx > d_in on the vector path", "linear-d128x128-R40-epipyg-maskk7-ldx256", "k_linear_lds<8,8>"),
    ("ldy > d_out on the vector path", "linear-d128x128-R40-epipyg-maskk7-ldy132", "k_linear_lds<8,8>"),
    ("ldr > d_out on the vector path", "linear-d128x128-R40-epipyg-maskk7-ldr132", "k_linear_lds<8,8>"),
    ("ldbb > d_out on the vector path", "linear-d128x128-R40-epibb_bias-ldbb132", "k_linear_lds<8,8>"),
    ("grid.y: the last block gets fewer tiles", "linear-d300x72-R12800-epibb", "1 < ny < nto: the last block gets fewer tiles"),
    ("grid.y: ot_lo >= nto for a trailing block", "linear-d300x72-R8193-epidgl-maskk7", "1 < ny < nto: a trailing block gets no tile"),
    ("grid.y: ny = 1", "linear-d5x3-R32769-epipyg-maskk1", "ny = 1"),
    ("R <= 8192 of the ksplit condition", "linear-d512x4-R8192-epidgl-maskk1", "k_linear_ksplit<true,true>"),
    ("R = 8193: past the ksplit condition", "linear-d512x4-R8193-epinone", "k_linear<true,true>"),
    ("lin_lds_blocks: want < CU count", "linear-d16x16-R48-epibb", "want < cus"),
    ("lin_lds_blocks: capped at the CU count", "linear-d16x16-R32784-epirespre-maskk1", "capped at cus"),
    ("k_gine_gather<float>", "gine-C37-noeps", "k_gine_gather<float>"),
    ("k_gine_gather<float> on C % 4 == 0, misaligned", "gine-C128-offea", "ea misaligned"),
    ("GINE grid: cols < 64", "gine-C63", "cols < 64"),
    ("GINE grid: cols >= 64", "gine-C65", "cols >= 64"),
    ("k_gin_gather<float> on F % 4 == 0, x misaligned", "gin-F128-offx", "x misaligned"),
    ("k_gin_gather<float> on F % 4 == 0, out misaligned", "gin-F128-offout-negate", "out misaligned"),
    ("k_gin_slab: need > lds_bytes", "slab-F256-negate", "LDS arm and fallback arm in one launch"),
    ("k_gin_slab<float>: the same", "slab-F257-negate", "LDS arm and fallback arm in one launch"),
    ("sn_gin_aggregate_add_f32", "gin_add-F128-plus", "plus"),
    ("colstats: two-level reduce", "colstats-R2049-C44", "two-level reduce"),
    ("colstats: single-level reduce", "colstats-R65-C65", "single-level reduce"),
    ("colstats: the 2048-block clamp", "colstats-R131073-C4", "2048-block clamp"),
    ("bn_train_stats: the 2048-block clamp", "bn_stats-R131073-C4", "2048-block clamp"),
    ("k_bn_train_finish1<64>", "bn_stats-R32897-C4", "finish1<64>"),
    ("k_bn_train_finish1<16> at 256 blocks", "bn_stats-R32769-C4", "finish1<16>"),
    ("C > 64: several c0 passes", "bn_stats-R65-C65", "C > 64"),
    ("C > 256", "colstats-R37-C300", "C > 256"),
    ("C = 255: the count column shares the last block", "colstats-R2049-C255", "count column shares a block"),
    ("C = 256: the count column in a block of its own", "colstats-R2049-C256", "count column in a block of its own"),
    ("ldx > C", "bn_stats-R65-C44-ld47", "ldx > C"),
    ("a block that starts inside a node's invalid tail", "bn_stats-R640-C44-masktail", "a block starts in a node's invalid tail"),
    ("a block with no valid row", "bn_stats-R640-C44-masktail", "a block with no valid row"),
    ("a batch with no valid row", "bn_stats-R300-C44-masknone_valid", "no valid row at all"),
    ("k_segment_pool: eight loads in flight", "pool-C20-modeadd", "eight loads in flight"),
    ("k_segment_pool: gridDim.y > 1", "pool-C300-modeadd", "gridDim.y > 1"),
    ("k_segment_pool: an empty segment in mean mode", "pool-C300-modemean", "empty segment"),
]
