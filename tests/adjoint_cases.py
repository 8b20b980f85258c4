"""Case tables, input generators and dtype-generic torch restatements for the adjoint grid (tests/test_adjoint_grid_gpu.py runs the
HIP kernels on them, tests/test_adjoint_cases_cpu.py checks the conditions that make that comparison mean something).  Importable
without a GPU: nothing here touches a device or the package's library.

Every adjoint of csrc/backward.hip, csrc/attention16.hip and csrc/gated.hip picks one of several kernels from the shape, the leading
dimensions and the pointer alignment.  A row of a table exists for ONE such choice: its `branch` string names the kernel or host
branch and the source condition that selects it, and the `*_branch` functions below restate the host dispatch (shape, strides,
alignment -> branch string).  The CPU test asserts predicate(row) == row.branch and that the rows of an op reach every name its
predicate can return, so an edit of a table cannot silently move a case onto another kernel.

A restatement maps the op's differentiable inputs (`leaves`) to its outputs in the dtype it is given: torch.autograd over it is the exact
adjoint in float64 and the reference's own fp32 adjoint in float32.  `reference(case, dtype)` runs it with seeded cotangents.

ReLU decisions: an adjoint with a ReLU in it is discontinuous — a pre-activation within rounding of zero falls on different sides in
fp32 and float64 and moves a gradient entry by a whole term, and with 1e5 .. 1e7 elements in the large rows that happens by chance.
The generators therefore push every valid pre-activation away from zero (`PUSH` of the tensor's rms; the CPU test asserts `MARGIN`).
That is a condition on the inputs, not a tolerance on the kernels.

Not here: the GIN / GINE aggregations, whose adjoints have one path each and are run over widths and topologies by
tests/test_topology_gpu.py::test_aggregation_adjoints_on_arbitrary_topologies.
"""
import math

import numpy as np
import torch

MARGIN = 1e-3            # asserted: min |pre-activation| over valid elements >= MARGIN * rms(pre-activation)
PUSH = 2e-3              # what the generators establish (the assertion keeps a factor two of room for the float32 cast of the inputs)
COT_SEED = 99
F32, F64 = torch.float32, torch.float64


class Case:
    def __init__(self, op, branch, factor=None, **p):
        self.op, self.branch, self.factor, self.p = op, branch, factor, p

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


def rng(*seed):
    return torch.Generator().manual_seed(hash(tuple(int(s) for s in seed)) % (2 ** 31))


def ragged_nvalid(N, K, g, zeros=False):
    """valid slot counts that include K and 1 (and 0 when a row count only factors as R x 1: then validity is per row)"""
    lo = 0 if zeros else 1
    nv = torch.randint(lo, K + 1, (N,), generator=g, dtype=torch.int32)
    nv[0] = K
    if N > 1:
        nv[-1] = 1
    if N > 2 and K > 1:
        nv[N // 2] = K - 1
    return nv


def row_mask(nv, K, R):
    if nv is None:
        return torch.ones(R, dtype=torch.bool)
    return (torch.arange(K)[None, :] < nv[:, None]).reshape(-1)


def slots_for(R):
    """(N, K) with N*K == R and K as large as the row count allows (K = 1: nvalid in {0, 1} marks whole rows)"""
    for K in (16, 17, 13, 9, 8, 7, 5, 3, 2):
        if R % K == 0 and R > K:
            return R // K, K
    return R, 1


def masked_rows(R, masked, g):
    """-> (nvalid or None, K, bool row mask)"""
    if not masked:
        return None, 0, torch.ones(R, dtype=torch.bool)
    N, K = slots_for(R)
    nv = ragged_nvalid(N, K, g, zeros=(K == 1))
    return nv, K, row_mask(nv, K, R)


def cotangent(i, shape):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(COT_SEED + i), dtype=F64)


# ============================================================================ ReLU margins
def push_elementwise(z, pre_fn, valid, iters=20):
    """Move the elements of the fp32 tensor z whose pre-activation pre_fn(z64) -> (a, da/dz) lies within PUSH * rms(a) of zero to the
    far side of 3 * PUSH * rms(a).  pre_fn may depend on statistics of z (BatchNorm): iterate until nothing is left."""
    for _ in range(iters):
        a, slope = pre_fn(z.double())
        rms = a[valid].pow(2).mean().sqrt()
        bad = (a.abs() < PUSH * rms) & valid[:, None]
        if not bool(bad.any()):
            return z
        sgn = torch.where(a >= 0, 1.0, -1.0).double()
        z = torch.where(bad, z.double() + sgn * 3 * PUSH * rms / slope, z.double()).float()
    raise AssertionError("push_elementwise: pre-activations near zero remain")


def push_linear(x, W, pre_fn, valid, iters=200):
    """The same where the pre-activation is pre_fn(x64 @ W64^T): a row of x is moved along W[o] / |W[o]|^2, which shifts z[r, o] alone by
    the wanted amount and the row's other outputs by less; repeated until every valid element is clear."""
    W64 = W.double()
    wn = (W64 * W64).sum(1)
    for _ in range(iters):
        a, slope = pre_fn(x.double() @ W64.t())
        rms = a[valid].pow(2).mean().sqrt()
        bad = (a.abs() < PUSH * rms) & valid[:, None]
        if not bool(bad.any()):
            return x
        rows = bad.any(1).nonzero()[:, 0]
        o = bad[rows].to(torch.uint8).argmax(1)
        sgn = torch.where(a[rows, o] >= 0, 1.0, -1.0).double()
        dz = sgn * 3 * PUSH * rms / slope[o]
        xd = x.double()
        xd[rows] += dz[:, None] * W64[o] / wn[o][:, None]
        x = xd.float()
    raise AssertionError("push_linear: pre-activations near zero remain")


def relu_margin(a, valid):
    """min |a| over the valid rows, in units of rms(a) over them (float64)"""
    av = a.double()[valid]
    return (av.abs().min() / av.pow(2).mean().sqrt()).item()


# ============================================================================ set attention
ATT_LDS_LIMIT, LDS_DEFAULT = 160 * 1024, 64 * 1024


def attention_branch(K, dk, aligned=True):
    """sn_set_attention_f32 (ops.hip) / sn_set_attention_bwd_f32 (backward.hip) + attention16_{forward,backward} (attention16.hip)"""
    out = []
    for d, lds in (("fwd", 4 * (3 * K * dk + K * (K + 1))), ("bwd", 4 * (4 * K * dk + 2 * K * (K + 1)))):
        scalar = "k_set_attention" + ("_bwd" if d == "bwd" else "")
        if lds > ATT_LDS_LIMIT:
            out.append(f"SN_REQUIRE {d}: LDS > 160 KiB")
        elif K <= 16 and dk in (16, 32, 64) and aligned:
            out.append(f"k_attn16_{d}<{dk}>")
        elif lds > LDS_DEFAULT:
            out.append(scalar + " raised LDS")
        else:
            out.append(scalar)
    return " | ".join(out)


ATTENTION_BRANCHES = ({f"k_attn16_{d}<{w}>" for d in ("fwd", "bwd") for w in (16, 32, 64)} |
                      {"k_set_attention", "k_set_attention_bwd", "k_set_attention raised LDS", "k_set_attention_bwd raised LDS"})


def _att(branch, K, dk, N, H=4, offset=False):
    return [Case("attention", branch, K=K, dk=dk, N=N, H=H, drop=drop, offset=offset) for drop in (False, True)]


def _mp(w):
    return f"k_attn16_fwd<{w}> | k_attn16_bwd<{w}>"


_SCALAR = "k_set_attention | k_set_attention_bwd"
ATTENTION = (
    # matrix pipe: K <= 16, dk in {16, 32, 64}, q / k / v / dout 16-byte aligned
    _att(_mp(32), 16, 32, 2950)              # the headline model's attention
    + _att(_mp(16), 8, 16, 37) + _att(_mp(64), 16, 64, 37) + _att(_mp(32), 1, 32, 37)
    + _att(_mp(16), 13, 16, 31, H=3)         # 93 waves: not a multiple of the four waves of a workgroup
    + _att(_mp(16), 16, 16, 1)
    + _att(_mp(16), 16, 16, 1, H=1)          # a single wave in the grid: the other three waves of its workgroup idle
    + _att(_mp(64), 5, 64, 2, H=1)
    # scalar kernels
    + _att(_SCALAR, 16, 27, 37)              # K <= 16 but width 108 (Alchemy)
    + _att(_SCALAR, 17, 32, 29) + _att(_SCALAR, 37, 27, 11)
    + _att("k_set_attention | k_set_attention_bwd raised LDS", 64, 32, 3)               # bwd 66 048 B of LDS > 64 KiB, fwd 41 216 B
    + _att("k_set_attention raised LDS | k_set_attention_bwd raised LDS", 64, 64, 3)    # fwd 65 792 B, bwd 98 816 B
    # matrix-pipe shapes behind pointers 4 bytes off a 16-byte boundary: the host predicate sends them to the scalar kernels
    + _att(_SCALAR, 16, 32, 37, offset=True) + _att(_SCALAR, 8, 16, 5, offset=True)
)
ATTENTION_REJECTED = dict(K=64, dk=128, N=2, H=1)          # bwd needs 164 352 B of LDS: SN_REQUIRE before any launch


def attention_gen(p):
    N, K, H, dk = p["N"], p["K"], p["H"], p["dk"]
    g = rng(1, N, K, H, dk)
    nv = ragged_nvalid(N, K, g)
    valid = row_mask(nv, K, N * K)
    q, k, v = (torch.randn(N * K, H * dk, generator=g) * valid[:, None] for _ in range(3))
    pm = None
    if p.get("drop"):          # stand-in with the layout and values of ops.attention_dropout_mask (the GPU test draws its own on the device)
        pm = (torch.rand(N, H, K, K, generator=g) >= 0.25).float() / 0.75
    return [q, k, v], dict(nv=nv, valid=valid, pm=pm, K=K)


def attention_ref(p, aux, q, k, v):
    N, K, H, dk = p["N"], p["K"], p["H"], p["dk"]
    qh, kh, vh = (t.view(N, K, H, dk).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) / dk ** 0.5
    ok = torch.arange(K)[None, :] < aux["nv"][:, None]
    pr = torch.softmax(s.masked_fill(~ok[:, None, None, :], float("-inf")), -1)
    if aux["pm"] is not None:
        pr = pr * aux["pm"].to(q.dtype)
    return ((pr @ vh).permute(0, 2, 1, 3).reshape(N * K, H * dk) * aux["valid"][:, None].to(q.dtype),)


# ============================================================================ LayerNorm adjoint
LN_BLOCK_ROWS = 64       # 4 * LN_ROWS = LNV_ROWS


def layernorm_branch(C, R, aligned=True, acc=False):
    """layernorm_bwd_impl (backward.hip): the row kernel, then k_cols_reduce over ceil(R / 64) partial rows (16 lanes per column; a lane
    takes the eight-loads-in-flight loop only when more than 7 * 16 partials remain for it)"""
    kern = f"k_layernorm_bwd_v4<{C // 4}>" if C in (32, 64, 128, 256) and aligned else "k_layernorm_bwd"
    nblk = -(-max(R, 1) // LN_BLOCK_ROWS)
    red = "k_cols_reduce unrolled" if nblk > 7 * 16 else ("k_cols_reduce >16 partials" if nblk > 16 else "k_cols_reduce <=16 partials")
    return " | ".join([kern, red] + (["accumulate"] if acc else []))


LAYERNORM_BRANCHES = ({f"k_layernorm_bwd_v4<{l}>" for l in (8, 16, 32, 64)} |
                      {"k_layernorm_bwd", "k_cols_reduce unrolled", "k_cols_reduce >16 partials", "k_cols_reduce <=16 partials", "accumulate"})


LN_KERNEL = {32: "k_layernorm_bwd_v4<8>", 64: "k_layernorm_bwd_v4<16>", 128: "k_layernorm_bwd_v4<32>", 256: "k_layernorm_bwd_v4<64>",
             12: "k_layernorm_bwd", 44: "k_layernorm_bwd", 108: "k_layernorm_bwd"}
LN_REDUCE = {1: "k_cols_reduce <=16 partials", 63: "k_cols_reduce <=16 partials", 64: "k_cols_reduce <=16 partials",
             65: "k_cols_reduce <=16 partials", 1105: "k_cols_reduce >16 partials", 4097: "k_cols_reduce >16 partials",
             47200: "k_cols_reduce unrolled"}


def _ln(C, R, masked=True, res=True, offset=False, acc=False):
    br = " | ".join(["k_layernorm_bwd" if offset else LN_KERNEL[C], LN_REDUCE[R]] + (["accumulate"] if acc else []))
    return Case("layernorm", br, C=C, R=R, masked=masked, res=res, offset=offset, acc=acc)


LAYERNORM = (
    [_ln(C, R, masked=(i + j) % 3 != 0, res=(i + j) % 2 == 0)
     for i, C in enumerate((32, 64, 128, 256, 12, 44, 108)) for j, R in enumerate((1, 63, 64, 65, 4097))]     # 4097 = 256 * 16 + 1 = 17 * 241
    + [_ln(C, 2950 * 16, res=(C != 64)) for C in (32, 64, 128, 256, 108)]                                      # the headline's 47 200 slot rows: 738 partials
    + [_ln(128, 4097, masked=False, res=False), _ln(44, 63, masked=False, res=False)]                         # nvalid = None
    + [_ln(128, R, offset=True) for R in (65, 4097)]                                                            # vectorised width, rows 4 bytes off: generic kernel
    + [_ln(C, R, acc=True) for C, R in ((128, 4097), (108, 65), (32, 1105))]                                     # two passes added into one .grad
)


def layernorm_gen(p):
    C, R = p["C"], p["R"]
    g = rng(2, C, R, p["masked"], p["res"])
    nv, K, valid = masked_rows(R, p["masked"], g)
    npass = 2 if p.get("acc") else 1
    leaves = []
    for _ in range(npass):
        leaves.append(torch.randn(R, C, generator=g))
        if p["res"]:
            leaves.append(torch.randn(R, C, generator=g))
    leaves += [torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)]
    return leaves, dict(nv=nv, K=K, valid=valid, eps=1e-6, npass=npass)


def layernorm_ref(p, aux, *leaves):
    gamma, beta = leaves[-2:]
    per = 2 if p["res"] else 1
    outs = []
    for i in range(aux["npass"]):
        u = leaves[i * per] + (leaves[i * per + 1] if p["res"] else 0)
        outs.append(torch.nn.functional.layer_norm(u, (p["C"],), gamma, beta, aux["eps"]) * aux["valid"][:, None].to(u.dtype))
    return tuple(outs)


# ============================================================================ weight gradient (k_wgrad + reductions)
def wgrad_branch(R, d_in, d_out, ldx=None, ldy=None, aligned=True, fused_bias=True, want_bias=True):
    """sn_linear_wgrad_f32 (backward.hip)"""
    ldx, ldy = ldx or d_in, ldy or d_out
    vec = d_in % 4 == 0 and d_out % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and aligned
    rpb = 128
    while -(-R // rpb) > 512:
        rpb *= 2
    nblk = -(-max(R, 1) // rpb)
    if fused_bias:
        red = "fused bias reduction, sum_parts " + ("tmp stage" if nblk > 32 else "single stage")
    else:
        red = "k_sum_strided" + (" x2" if want_bias else " dW only")
    return " | ".join(["k_wgrad vec" if vec else "k_wgrad scalar", f"rpb {rpb}", red])


WGRAD_BRANCHES = {"k_wgrad vec", "k_wgrad scalar", "rpb 128", "rpb 256", "fused bias reduction, sum_parts tmp stage",
                  "fused bias reduction, sum_parts single stage", "k_sum_strided x2", "k_sum_strided dW only"}
WGRAD_DIMS = ((128, 128), (108, 108), (27, 108), (128, 1), (1, 128), (130, 66))


WG_KERNEL = {(128, 128): "k_wgrad vec", (108, 108): "k_wgrad vec", (27, 108): "k_wgrad scalar", (128, 1): "k_wgrad scalar",
             (1, 128): "k_wgrad scalar", (130, 66): "k_wgrad scalar"}
_ONE, _TMP = "fused bias reduction, sum_parts single stage", "fused bias reduction, sum_parts tmp stage"
WG_ROWS = {1: "rpb 128 | " + _ONE, 127: "rpb 128 | " + _ONE, 128: "rpb 128 | " + _ONE, 129: "rpb 128 | " + _ONE, 4097: "rpb 128 | " + _TMP,
           65536: "rpb 128 | " + _TMP, 65537: "rpb 256 | " + _TMP, 70001: "rpb 256 | " + _TMP}


def _lin(d, R, masked, bias, relu=False):
    return Case("linear", WG_KERNEL[d] + " | " + WG_ROWS[R], d=d, R=R, masked=masked, bias=bias, relu=relu)


LINEAR = (
    [_lin(d, R, masked=(i + j) % 2 == 0, bias=(i + j) % 3 != 0, relu=(i + 2 * j) % 4 == 0)
     for i, d in enumerate(WGRAD_DIMS) for j, R in enumerate((1, 127, 128, 129, 4097))]          # 4097 rows: 33 partials, the tmp stage
    # 65 536 rows: 512 chunks of 128; one row more: 257 chunks of 256.  70 001 = 7 * 73 * 137: the all-eigenvector ZINC batch's phi rows
    + [_lin((128, 128), 65536, True, True), _lin((128, 128), 65537, False, True), _lin((128, 128), 70001, True, True),
       _lin((128, 128), 70001, False, False),
       _lin((27, 108), 65536, False, True), _lin((27, 108), 65537, True, False), _lin((27, 108), 70001, True, True),
       _lin((130, 66), 65537, True, True), _lin((108, 108), 70001, False, True), _lin((1, 128), 65536, True, True),
       _lin((128, 1), 70001, False, True)]
)


def _wraw(branch, d, R, ldx, ldy, masked, sep_db, want_bias=True):
    return Case("wgrad_raw", branch, d=d, R=R, ldx=ldx, ldy=ldy, masked=masked, sep_db=sep_db, want_bias=want_bias)


WGRAD_RAW = [
    # column slices of wider matrices, strides multiples of 4: float4 path
    _wraw("k_wgrad vec | rpb 128 | " + _TMP, (128, 128), 4097, 256, 132, True, False),
    # strides not multiples of 4: scalar path on a vectorisable width
    _wraw("k_wgrad scalar | rpb 128 | " + _TMP, (128, 128), 4097, 257, 131, True, False),
    _wraw("k_wgrad scalar | rpb 128 | " + _ONE, (108, 108), 129, 110, 220, False, False),
    # db not directly behind dW: two k_sum_strided launches
    _wraw("k_wgrad vec | rpb 128 | k_sum_strided x2", (128, 128), 4097, 128, 128, True, True),
    _wraw("k_wgrad scalar | rpb 256 | k_sum_strided x2", (27, 108), 70001, 27, 108, True, True),
    _wraw("k_wgrad scalar | rpb 128 | k_sum_strided dW only", (130, 66), 129, 130, 66, False, True, want_bias=False),
]


def linear_gen(p):
    (d_in, d_out), R = p["d"], p["R"]
    g = rng(3, d_in, d_out, R, p["masked"], p["bias"])
    nv, K, valid = masked_rows(R, p["masked"], g)
    x = torch.randn(R, d_in, generator=g) * valid[:, None]
    W = torch.randn(d_out, d_in, generator=g) / d_in ** 0.5
    b = torch.randn(d_out, generator=g)
    if p["relu"]:
        b64 = b.double() if p["bias"] else 0
        x = push_linear(x, W, lambda z: (z + b64, torch.ones(d_out, dtype=F64)), valid) * valid[:, None]
    return [x, W] + ([b] if p["bias"] else []), dict(nv=nv, K=K, valid=valid)


def linear_pre(p, aux, x, W, *b):
    return x @ W.t() + (b[0] if b else 0)


def linear_ref(p, aux, x, W, *b):
    y = linear_pre(p, aux, x, W, *b)
    if p["relu"]:
        y = torch.relu(y)
    return (y * aux["valid"][:, None].to(y.dtype),)


def wgrad_raw_gen(p):
    (d_in, d_out), R = p["d"], p["R"]
    g = rng(4, d_in, d_out, R, p["ldx"], p["ldy"])
    nv, K, valid = masked_rows(R, p["masked"], g)
    X, DY = torch.randn(R, p["ldx"], generator=g), torch.randn(R, p["ldy"], generator=g)        # invalid rows carry data: the kernel masks them
    # the slices start 4 floats in where the wider matrix has the room: the pointers stay 16-byte aligned, the strides alone decide
    return [X, DY], dict(nv=nv, K=K, valid=valid, cx=4 if p["ldx"] - d_in >= 4 else 0, cy=4 if p["ldy"] - d_out >= 4 else 0)


def wgrad_raw_ref(p, aux, X, DY):
    (d_in, d_out) = p["d"]
    m = aux["valid"][:, None].to(X.dtype)
    x, dy = X[:, aux["cx"]:aux["cx"] + d_in] * m, DY[:, aux["cy"]:aux["cy"] + d_out] * m
    return (dy.t() @ x,) + ((dy.sum(0),) if p["want_bias"] else ())


# ============================================================================ BatchNorm + activation adjoint
def bn_branch(R):
    """sn_bn_act_bwd_f32 (backward.hip): ceil(R / 64) workgroups of 64 rows, capped at 2048 (then more rows per workgroup)"""
    b = -(-max(R, 1) // 64)
    return " | ".join(["bn_bwd_blocks capped at 2048" if b > 2048 else "bn_bwd_blocks R/64",
                       "sum_parts tmp stage" if min(b, 2048) > 32 else "sum_parts single stage"])


BN_BRANCHES = {"bn_bwd_blocks capped at 2048", "bn_bwd_blocks R/64", "sum_parts tmp stage", "sum_parts single stage", "ld > C"}


BN_ROWS = {63: "bn_bwd_blocks R/64 | sum_parts single stage", 64: "bn_bwd_blocks R/64 | sum_parts single stage",
           65: "bn_bwd_blocks R/64 | sum_parts single stage", 129: "bn_bwd_blocks R/64 | sum_parts single stage",
           2113: "bn_bwd_blocks R/64 | sum_parts tmp stage", 4225: "bn_bwd_blocks R/64 | sum_parts tmp stage",
           47200: "bn_bwd_blocks R/64 | sum_parts tmp stage", 131073: "bn_bwd_blocks capped at 2048 | sum_parts tmp stage",
           140000: "bn_bwd_blocks capped at 2048 | sum_parts tmp stage"}
LBN_WGRAD = {(128, 128, 4225): "k_wgrad vec | rpb 128 | " + _TMP, (27, 108, 65): "k_wgrad scalar | rpb 128 | " + _ONE,
             (130, 66, 129): "k_wgrad scalar | rpb 128 | " + _ONE}


def _bn(C, R, relu, masked, res, ld=None, linear=None):
    br = BN_ROWS[R] + (" | ld > C" if ld else "")
    if linear:
        br += " | " + LBN_WGRAD[(linear, C, R)]
    return Case("linear_bn_act" if linear else "bn_act", br, C=C, R=R, relu=relu, masked=masked, res=res, ld=ld, d_in=linear)


BN_ACT = (
    [_bn(C, R, relu=(i + j) % 3 != 0, masked=(i + j) % 2 == 0, res=(i + j) % 4 == 1)
     for i, C in enumerate((1, 44, 108, 128)) for j, R in enumerate((63, 64, 65, 2113))]        # 2113 rows: 34 partials, the tmp stage
    + [_bn(C, 47200, relu=(C != 44), masked=True, res=(C == 128)) for C in (1, 44, 108, 128)]
    + [_bn(16, 140000, True, True, False), _bn(16, 140000, False, False, True), _bn(16, 131073, True, False, False)]      # > 131 072 rows: the cap
    + [_bn(44, 65, True, True, False, ld=(48, 47, 50)), _bn(128, 2113, True, False, False, ld=(132, 256, 129))]            # ldz, ldd, ldo > C
)
LINEAR_BN_ACT = [_bn(128, 4225, True, True, True, linear=128), _bn(108, 65, True, False, False, linear=27),
                 _bn(66, 129, False, True, False, linear=130)]
WGRAD_VIA_BN = {"k_wgrad vec", "k_wgrad scalar", "rpb 128", "fused bias reduction, sum_parts tmp stage",
                "fused bias reduction, sum_parts single stage"}
BN_EPS = 1e-5


def _bn_pre(z, valid, gamma, beta):
    zv = z[valid]
    mean, var = zv.mean(0), zv.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + BN_EPS)
    return (z - mean) * rstd * gamma + beta, gamma * rstd


def bn_act_gen(p):
    C, R = p["C"], p["R"]
    g = rng(5, C, R, p["relu"], p["masked"], p["res"])
    nv, K, valid = masked_rows(R, p["masked"], g)
    z = torch.randn(R, C, generator=g)                         # invalid rows carry data: statistics and adjoint must skip them
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    if p["relu"]:
        z = push_elementwise(z, lambda z64: _bn_pre(z64, valid, gamma.double(), beta.double()), valid)
    leaves = [z, gamma, beta]
    if p["res"]:
        leaves.append(torch.randn(R, C, generator=g) * valid[:, None])
    return leaves, dict(nv=nv, K=K, valid=valid)


def bn_act_pre(p, aux, z, gamma, beta, *r):
    return _bn_pre(z, aux["valid"], gamma, beta)[0]


def bn_act_ref(p, aux, z, gamma, beta, *r):
    a = bn_act_pre(p, aux, z, gamma, beta)
    if p["relu"]:
        a = torch.relu(a)
    if r:
        a = a + r[0]
    return (a * aux["valid"][:, None].to(a.dtype),)


def linear_bn_act_gen(p):
    C, R, d_in = p["C"], p["R"], p["d_in"]
    g = rng(6, C, R, d_in)
    nv, K, valid = masked_rows(R, p["masked"], g)
    x = torch.randn(R, d_in, generator=g) * valid[:, None]
    W, b = torch.randn(C, d_in, generator=g) / d_in ** 0.5, torch.randn(C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    if p["relu"]:
        x = push_linear(x, W, lambda z: _bn_pre(z + b.double(), valid, gamma.double(), beta.double()), valid) * valid[:, None]
    leaves = [x, W, gamma, beta]          # (the gradient of a bias in front of a BatchNorm is identically zero: b is not a leaf)
    if p["res"]:
        leaves.append(torch.randn(R, C, generator=g) * valid[:, None])
    return leaves, dict(nv=nv, K=K, valid=valid, b=b)


def linear_bn_act_pre(p, aux, x, W, gamma, beta, *r):
    # (the Linear's output is masked before the statistics; they run over the valid rows only, so the mask changes nothing here)
    return _bn_pre(x @ W.t() + aux["b"].to(x.dtype), aux["valid"], gamma, beta)[0]


def linear_bn_act_ref(p, aux, x, W, gamma, beta, *r):
    a = linear_bn_act_pre(p, aux, x, W, gamma, beta)
    if p["relu"]:
        a = torch.relu(a)
    if r:
        a = a + r[0]
    return (a * aux["valid"][:, None].to(a.dtype),)


# ============================================================================ embedding adjoint
def embedding_branch(C, R):
    """sn_embedding_sum_bwd_layers_f32 (backward.hip)"""
    bs = 256 if C >= 256 else (C + 63) // 64 * 64
    return " | ".join([f"chunk block {bs}", "chunk LDS raised" if 64 * C * 4 > 65536 else "chunk LDS default",
                       "gather float4" if C % 4 == 0 and C // 4 <= 256 else "gather scalar",
                       "gather passes > 1" if -(-R // 64) > 1024 else "gather one pass"])


EMBEDDING_BRANCHES = {"chunk block 64", "chunk block 128", "chunk block 256", "chunk LDS raised", "chunk LDS default", "gather float4",
                      "gather scalar", "gather passes > 1", "gather one pass"}


EMB_WIDTH = {1: "chunk block 64 | chunk LDS default | gather scalar", 8: "chunk block 64 | chunk LDS default | gather float4",
             20: "chunk block 64 | chunk LDS default | gather float4", 127: "chunk block 128 | chunk LDS default | gather scalar",
             128: "chunk block 128 | chunk LDS default | gather float4", 256: "chunk block 256 | chunk LDS default | gather float4",
             260: "chunk block 256 | chunk LDS raised | gather float4", 512: "chunk block 256 | chunk LDS raised | gather float4"}


def _emb(C, R, vocab, oor=False):
    return Case("embedding", EMB_WIDTH[C] + (" | gather passes > 1" if R == 70001 else " | gather one pass"), C=C, R=R, vocab=vocab, oor=oor)


EMBEDDING = (
    [_emb(C, R, vocab=((28,), (500, 3), (5,), (11, 5))[(i + j) % 4])
     for i, C in enumerate((1, 127, 128, 256, 260, 512)) for j, R in enumerate((1, 63, 64, 65, 5000))]
    + [_emb(1, 5000, (1,)), _emb(128, 65, (1,)), _emb(1, 5000, (65535,)), _emb(128, 5000, (65535,)),
       _emb(20, 5000, (65535, 2)),                     # two feature columns with very different table sizes
       _emb(8, 70001, (30,)),                          # 1094 chunks: the gather's second pass over the chunk lists
       _emb(128, 300, (11, 5), oor=True), _emb(127, 65, (28,), oor=True)]
)


def embedding_gen(p):
    C, R, vocab = p["C"], p["R"], p["vocab"]
    g = rng(7, C, R, *vocab)
    idx = torch.stack([torch.randint(0, V, (R,), generator=g) for V in vocab], 1)
    if p["oor"]:                                         # ids outside [0, V): one past the end and a negative one
        idx[R // 3, 0] = vocab[0]
        idx[R // 2, len(vocab) - 1] = -1
    tables = [torch.randn(V, C, generator=g) for V in vocab]
    return tables, dict(idx=idx)


def embedding_ref(p, aux, *tables):
    idx = aux["idx"]
    out = 0
    for f, T in enumerate(tables):
        ok = (idx[:, f] >= 0) & (idx[:, f] < T.shape[0])
        out = out + T[idx[:, f].clamp(0, T.shape[0] - 1)] * ok[:, None].to(T.dtype)
    return (out,)


# ============================================================================ graph aggregations
def topology_batch():
    """the multi-graph batch of tests/test_topology_gpu.py: a hub with 39 in-edges, isolated nodes, multi-edges, self loops, a shuffled
    edge list -> (edge_index [2, E], batch [N], sizes)"""
    from test_topology_gpu import _batch, _topologies
    host = _batch(_topologies(np.random.default_rng(11)), "zinc", seed=3)
    return host.edge_index, host.batch, host.sizes


def gated_branch(C, ldn):
    """sn_gated_aggregate_f32 (gated.hip); its adjoint (k_gated_bwd_dst + k_gated_bwd_src) has one path"""
    return "k_gated_fwd_v4" if C % 4 == 0 and ldn % 4 == 0 else "k_gated_fwd"          # (and 16-byte aligned pointers: torch allocations are)


GATED_BRANCHES = {"k_gated_fwd_v4", "k_gated_fwd"}
GATED_WIDTH = {1: "k_gated_fwd", 3: "k_gated_fwd", 20: "k_gated_fwd_v4", 70: "k_gated_fwd", 128: "k_gated_fwd_v4"}
GATED = ([Case("gated", GATED_WIDTH[C], C=C, blocked=False) for C in (1, 3, 20, 70, 128)]
         # A/B/D/E as the column blocks of one [N, 4C] matrix, as the GatedGCN layer passes them (ldn = 4C)
         + [Case("gated", GATED_WIDTH[C], C=C, blocked=True) for C in (3, 70, 128)])


def gated_gen(p):
    C = p["C"]
    ei, batch, _ = topology_batch()
    N, E = batch.numel(), ei.shape[1]
    g = rng(8, C)
    leaves = [torch.randn(N, C, generator=g) for _ in range(4)] + [torch.randn(E, C, generator=g)]
    return leaves, dict(ei=ei, batch=batch)


def gated_ref(p, aux, Ah, Bh, Dh, Eh, Ce):
    src, dst = aux["ei"]
    en = Dh[src] + Eh[dst] + Ce
    sg = torch.sigmoid(en)
    num = torch.zeros_like(Ah).index_add_(0, dst, Bh[src] * sg)
    den = torch.zeros_like(Ah).index_add_(0, dst, sg)
    return Ah + num / (den + 1e-6), en


SLOT_KC = [(K, C) for K in (1, 16, 64) for C in (1, 27, 128)]
SLOT_SUM = [Case("slot_sum", "k_slot_sum + k_slot_bcast", K=K, C=C, N=37) for K, C in SLOT_KC]
MASKED_ADD = [Case("masked_add", "k_masked_affine residual", K=K, C=C, N=37) for K, C in SLOT_KC] + \
             [Case("masked_add", "k_masked_affine residual", K=0, C=C, N=131) for C in (1, 27, 128)]
SEGMENT_SIZES = [5, 1, 64, 30, 1, 17]
SEGMENT_POOL = [Case("segment_pool", "k_segment_pool + k_segment_bcast", C=C, mode=m) for C in (1, 27, 128) for m in ("add", "mean")]
SEGMENT_BCAST_ADD = [Case("segment_bcast_add", "k_segment_bcast + k_pointwise + k_relu_bwd + k_segment_pool", C=C, relu=r)
                     for C in (1, 27, 128) for r in (False, True)]
RELU_BWD = [Case("relu_bwd", "k_relu_bwd", C=C, R=R, masked=m) for C in (1, 27, 128) for R, m in ((65, True), (4097, False))] + \
           [Case("relu_bwd", "k_relu_bwd", C=128, R=70001, masked=True)]


def slot_gen(p):
    N, K, C = p["N"], p["K"], p["C"]
    g = rng(9, N, K, C)
    if K == 0:
        return [torch.randn(N, C, generator=g) for _ in range(2)], dict(nv=None, K=0, valid=torch.ones(N, dtype=torch.bool))
    nv = ragged_nvalid(N, K, g)
    valid = row_mask(nv, K, N * K)
    return [torch.randn(N * K, C, generator=g) * valid[:, None] for _ in range(2)], dict(nv=nv, K=K, valid=valid)


def slot_sum_gen(p):
    leaves, aux = slot_gen(p)
    return leaves[:1], aux


def slot_sum_ref(p, aux, x):
    return ((x * aux["valid"][:, None].to(x.dtype)).view(p["N"], p["K"], p["C"]).sum(1),)


def masked_add_ref(p, aux, a, b):
    return ((a + b) * aux["valid"][:, None].to(a.dtype),)


def segment_batch():
    return torch.repeat_interleave(torch.arange(len(SEGMENT_SIZES)), torch.tensor(SEGMENT_SIZES))


def segment_pool_gen(p):
    g = rng(10, p["C"])
    return [torch.randn(sum(SEGMENT_SIZES), p["C"], generator=g)], dict(batch=segment_batch())


def segment_pool_ref(p, aux, h):
    out = torch.zeros(len(SEGMENT_SIZES), p["C"], dtype=h.dtype).index_add_(0, aux["batch"], h)
    return (out / torch.tensor(SEGMENT_SIZES, dtype=h.dtype)[:, None] if p["mode"] == "mean" else out,)


def segment_bcast_add_gen(p):
    g = rng(11, p["C"])
    batch = segment_batch()
    x1, x2 = torch.randn(batch.numel(), p["C"], generator=g), torch.randn(len(SEGMENT_SIZES), p["C"], generator=g)
    if p["relu"]:
        x1 = push_elementwise(x1, lambda z: (z + x2.double()[batch], torch.ones(p["C"], dtype=F64)), torch.ones(batch.numel(), dtype=torch.bool))
    return [x1, x2], dict(batch=batch, valid=torch.ones(batch.numel(), dtype=torch.bool))


def segment_bcast_add_pre(p, aux, x1, x2):
    return x1 + x2[aux["batch"]]


def segment_bcast_add_ref(p, aux, x1, x2):
    y = segment_bcast_add_pre(p, aux, x1, x2)
    return (torch.relu(y) if p["relu"] else y,)


def relu_bwd_gen(p):
    C, R = p["C"], p["R"]
    g = rng(12, C, R)
    nv, K, valid = masked_rows(R, p["masked"], g)
    pre = push_elementwise(torch.randn(R, C, generator=g), lambda z: (z, torch.ones(C, dtype=F64)), valid)
    return [torch.randn(R, C, generator=g)], dict(nv=nv, K=K, valid=valid, pre=pre, y=torch.relu(pre))      # invalid rows of y carry data


def relu_bwd_pre(p, aux, dy):
    return aux["pre"].to(dy.dtype)


def relu_bwd_ref(p, aux, dy):
    """sn_relu_bwd_f32 is linear in dy: its restatement is the map itself"""
    return (dy * (aux["y"] > 0).to(dy.dtype) * aux["valid"][:, None].to(dy.dtype),)


# ============================================================================ dot product
def dot_branch(n):
    """sn_dot_f32 (backward.hip): ceil(n / 256) workgroups, at most 256 (then a grid-stride loop)"""
    b = -(-max(n, 1) // 256)
    return "k_dot_partial 256 blocks, grid stride" if b > 256 else ("k_dot_partial one block" if b == 1 else "k_dot_partial n/256 blocks")


DOT_BRANCHES = {"k_dot_partial 256 blocks, grid stride", "k_dot_partial one block", "k_dot_partial n/256 blocks"}
DOT = [Case("dot", b, n=n) for n, b in ((1, "k_dot_partial one block"), (255, "k_dot_partial one block"), (256, "k_dot_partial one block"),
                                        (257, "k_dot_partial n/256 blocks"), (65536, "k_dot_partial n/256 blocks"),
                                        (65537, "k_dot_partial 256 blocks, grid stride"), (1000003, "k_dot_partial 256 blocks, grid stride"))]


def dot_gen(p):
    g = rng(13, p["n"])
    a = torch.randn(p["n"], generator=g)
    return [a, 0.5 * a + torch.randn(p["n"], generator=g)], {}      # E[a b] = 1/2: the sum is not a cancellation to zero


def dot_ref(p, aux, a, b):
    return ((a * b).sum().reshape(1),)


# ============================================================================ Adam
ADAM_HYPER = {"torch": (1e-3, 0.9, 0.999, 1e-8), "test": (1e-2, 0.9, 0.99, 1e-8)}
ADAM = [Case("adam", "k_adam", n=n, hyper=h, wd=wd, gs=gs, step=t)
        for n in (1, 257, 1000003) for h in ("torch", "test") for wd in (0.0, 0.01) for gs in (1.0, 0.25) for t in (1, 10, 2000)]


def adam_gen(p):
    """Parameter, gradient and the float64 moments of step t - 1: those of a gradient history with per-element mean mu and second moment
    nu, m = (1 - b1^(t-1)) mu, v = (1 - b2^(t-1)) nu — the state Adam has after t - 1 steps, without running them."""
    n, t = p["n"], p["step"]
    _, b1, b2, _ = ADAM_HYPER[p["hyper"]]
    g = rng(14, n, t)
    par, grad = 0.05 * torch.randn(n, generator=g), torch.randn(n, generator=g)
    mu = torch.randn(n, generator=g, dtype=F64) * 0.3
    nu = mu * mu + torch.rand(n, generator=g, dtype=F64) + 0.1
    return par, grad, (1 - b1 ** (t - 1)) * mu, (1 - b2 ** (t - 1)) * nu


def adam_f64(p, par, grad, m, v):
    """One step of torch.optim.Adam (no amsgrad) written out in float64 -> (update = p_new - p_old, m_new, v_new)"""
    lr, b1, b2, eps = ADAM_HYPER[p["hyper"]]
    t = p["step"]
    par, gi = par.double(), grad.double() * p["gs"]
    gi = gi + p["wd"] * par
    m = b1 * m + (1 - b1) * gi
    v = b2 * v + (1 - b2) * gi * gi
    denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
    return -(lr / (1 - b1 ** t)) * (m / denom), m, v


def adam_torch32(p, par, grad, m, v):
    """The same step by torch.optim.Adam in float32 on the CPU, from the float32 cast of the same state"""
    lr, b1, b2, eps = ADAM_HYPER[p["hyper"]]
    q = torch.nn.Parameter(par.clone())
    opt = torch.optim.Adam([q], lr=lr, betas=(b1, b2), eps=eps, weight_decay=p["wd"], foreach=False, fused=False)
    q.grad = grad * p["gs"]
    opt.state[q] = {"step": torch.tensor(float(p["step"] - 1)), "exp_avg": m.float().clone(), "exp_avg_sq": v.float().clone()}
    opt.step()
    st = opt.state[q]
    return q.detach().double() - par.double(), st["exp_avg"], st["exp_avg_sq"]


# ============================================================================ registry
class Op:
    def __init__(self, cases, gen, ref, predicate, branches, pre=None, grads=True):
        self.cases, self.gen, self.ref, self.predicate, self.branches, self.pre, self.grads = cases, gen, ref, predicate, branches, pre, grads


def _const(cases):
    return (lambda p: cases[0].branch), {cases[0].branch}


OPS = {
    "attention": Op(ATTENTION, attention_gen, attention_ref, lambda p: attention_branch(p["K"], p["dk"], not p["offset"]), ATTENTION_BRANCHES),
    "layernorm": Op(LAYERNORM, layernorm_gen, layernorm_ref, lambda p: layernorm_branch(p["C"], p["R"], not p["offset"], p["acc"]),
                    LAYERNORM_BRANCHES),
    "linear": Op(LINEAR, linear_gen, linear_ref, lambda p: wgrad_branch(p["R"], *p["d"]),
                 WGRAD_BRANCHES - {"k_sum_strided x2", "k_sum_strided dW only"}, pre=linear_pre),
    "wgrad_raw": Op(WGRAD_RAW, wgrad_raw_gen, wgrad_raw_ref,
                    lambda p: wgrad_branch(p["R"], p["d"][0], p["d"][1], p["ldx"], p["ldy"], True, not p["sep_db"], p["want_bias"]),
                    {"k_wgrad vec", "k_wgrad scalar", "rpb 128", "rpb 256", "k_sum_strided x2", "k_sum_strided dW only",
                     "fused bias reduction, sum_parts tmp stage", "fused bias reduction, sum_parts single stage"}, grads=False),
    "bn_act": Op(BN_ACT, bn_act_gen, bn_act_ref, lambda p: bn_branch(p["R"]) + (" | ld > C" if p["ld"] else ""), BN_BRANCHES, pre=bn_act_pre),
    "linear_bn_act": Op(LINEAR_BN_ACT, linear_bn_act_gen, linear_bn_act_ref,
                        lambda p: bn_branch(p["R"]) + " | " + wgrad_branch(p["R"], p["d_in"], p["C"]),
                        {"bn_bwd_blocks R/64", "sum_parts tmp stage", "sum_parts single stage"} | WGRAD_VIA_BN, pre=linear_bn_act_pre),
    "embedding": Op(EMBEDDING, embedding_gen, embedding_ref, lambda p: embedding_branch(p["C"], p["R"]), EMBEDDING_BRANCHES),
    "gated": Op(GATED, gated_gen, gated_ref, lambda p: gated_branch(p["C"], 4 * p["C"] if p["blocked"] else p["C"]), GATED_BRANCHES),
    "slot_sum": Op(SLOT_SUM, slot_sum_gen, slot_sum_ref, *_const(SLOT_SUM)),
    "masked_add": Op(MASKED_ADD, slot_gen, masked_add_ref, *_const(MASKED_ADD)),
    "segment_pool": Op(SEGMENT_POOL, segment_pool_gen, segment_pool_ref, *_const(SEGMENT_POOL)),
    "segment_bcast_add": Op(SEGMENT_BCAST_ADD, segment_bcast_add_gen, segment_bcast_add_ref, *_const(SEGMENT_BCAST_ADD), pre=segment_bcast_add_pre),
    "relu_bwd": Op(RELU_BWD, relu_bwd_gen, relu_bwd_ref, *_const(RELU_BWD), pre=relu_bwd_pre, grads=False),
    "dot": Op(DOT, dot_gen, dot_ref, lambda p: dot_branch(p["n"]), DOT_BRANCHES, grads=False),
}
HAS_RELU = {"linear": lambda p: p["relu"], "bn_act": lambda p: p["relu"], "linear_bn_act": lambda p: p["relu"],
            "segment_bcast_add": lambda p: p["relu"], "relu_bwd": lambda p: True}


def reference(case, dtype, leaves=None, aux=None):
    """-> (outputs, gradients of the leaves) of the restatement in `dtype` (gradients: [] for the ops that are plain linear maps)"""
    op = OPS[case.op]
    if leaves is None:
        leaves, aux = op.gen(case.p)
    xs = [t.detach().to(dtype).requires_grad_(op.grads) for t in leaves]
    outs = op.ref(case.p, aux, *xs)
    if not op.grads:
        return [o.detach() for o in outs], []
    torch.autograd.backward(outs, [cotangent(i, o.shape).to(dtype) for i, o in enumerate(outs)])
    return [o.detach() for o in outs], [x.grad for x in xs]
