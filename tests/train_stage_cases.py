"""Case tables, host restatements of the dispatch, input generators and dtype-generic torch restatements for the training-link grid
(tests/test_train_stage_grid_gpu.py runs csrc/train.hip on them, tests/test_train_stage_cases_cpu.py checks the conditions that make that
comparison mean something).  Importable without a GPU and without the library: nothing here touches a device.

A public function of train_stage.py is a short chain of launches; which kernel a launch is, how many workgroups it gets and which runtime
arms of the kernel it walks follow from the row count, the group count, the widths, the weight's alignment and — for the backward — from
WHO OWNS the parameters' gradients.  `trace(case)` restates that chain on the host (train.hip: tile_mode / sn_train_linear_blocks /
sn_train_linear_bwd_blocks / sn_train_bn_bwd_blocks and the two dispatchers; train_stage.py: linear_fwd / linear_bwd / _mlp2_backward) and
returns the branch atoms of every launch plus, per launch structure, the number of calls of the reduction / finish entry points, which
the GPU test counts on the library handle.  A row's `branch` NAMES the kernel-level atoms (kernels, workgroup-count rules, no-row exits);
BRANCHES pins, per op, everything its rows reach — runtime arms included.  The CU count is a parameter (the caps are CUs / G);
the tables are written for 256 CUs.

Launch structures (`variants` of a row):
  autograd         plain parameters: the kernels hand dW / db / d gamma / d beta back to autograd, a finish launch in front of every link
  direct           parameters whose .grad the optimiser owns (optim.FlatAdam): consumer-side merge, deferred reductions — the default
  direct-nomerge   ... with train_stage.MERGE_COEF off: the BatchNorm finish fused into sn_train_post_link_f32
  direct-nodefer   ... with train_stage.DEFER_DW off: sn_train_post_link_f32 / accumulating sn_train_reduce_parts_f32 behind every link
  direct-plain     both off
A weight that is a view (ldw = d_in + 1, or one float off a 16-byte boundary) cannot own a contiguous .grad: those rows run the autograd
structure only.  They are what reaches the non-split full-width persistent forward; no row depends on an environment variable.

A backward arm is named with the kernel it ran in: "merge @split" is the TBMerge prologue of k_tlin_bwd<8,8,true,2,SPLIT>.  "gx = null
@split" does not exist: the dispatch sends a full-width link without an input gradient to k_tlin_bwd<8,8,true,4>.

Masks: one validity vector per row of the table, shared by the G groups — by construction of the kernels' arguments (nvalid is indexed by
the row within the group), which is also how the phi(+x) / phi(-x) passes use them.

ReLU decisions: as in tests/adjoint_cases.py every valid pre-activation is pushed PUSH of its tensor's rms away from zero and the CPU test
asserts MARGIN.  Where the tensor in front of the ReLU is free (the raw rows' operand) that is push_elementwise; behind one or two Linears
and a BatchNorm nothing is free but the input rows, and push_rows moves a row along the gradient of the offending element.
"""
import functools
import types
from collections import Counter

import torch

from adjoint_cases import F32, F64, MARGIN, PUSH, Case, cotangent, push_elementwise, ragged_nvalid, rng, row_mask      # noqa: F401
from adjoint_cases import slots_for

CUS = 256
TILE_MODE_MAX = 512          # row tiles, all groups together
BN_EPS = 1e-5
VARIANTS = {"autograd": (False, False, False), "direct": (True, True, True), "direct-nomerge": (True, False, True),
            "direct-nodefer": (True, True, False), "direct-plain": (True, False, False)}          # (direct, merge, defer)
COUNTED = ("sn_train_bn_bwd_finish_f32", "sn_train_post_link_f32", "sn_train_reduce_parts_f32", "sn_train_reduce_jobs_f32",
           "sn_train_dot_jobs_f64", "sn_train_dot_finish_f64")


def cdiv(a, b):
    return -(-a // b)


# ============================================================================ host restatement of the dispatch (train.hip:1729-1885)
def tile_mode(R, G):
    return cdiv(max(R, 1), 16) * max(G, 1) <= TILE_MODE_MAX


def fwd_blocks(R, G, cus=CUS):
    tiles = cdiv(max(R, 1), 16)
    return tiles if tile_mode(R, G) else min(cdiv(tiles, 4), max(cus // max(G, 1), 1))


def bwd_blocks(R, G, cus=CUS):
    return cdiv(max(R, 1), 16) if tile_mode(R, G) else min(cdiv(max(R, 1), 64), max(cus // max(G, 1), 1))


def bn_bwd_blocks(R, G, cus=CUS):
    return min(cdiv(max(R, 1), 32 if tile_mode(R, G) else 128), max(2 * cus // max(G, 1), 1))


def _b(v):
    return "true" if v else "false"


def _nv(K):
    return "nvalid null" if K == 0 else ("nvalid K = 1" if K == 1 else "nvalid K > 1")


def fwd_branch(R, G, d_in, d_out, stats, K=0, bias=False, in_scale=False, in_relu=False, out_relu=False, w_vec=True, cus=CUS):
    """sn_train_linear_f32.  w_vec: the weight is 16-byte aligned with ldw % 4 == 0."""
    if R == 0:
        return ["fwd R = 0 memset" if stats else "fwd R = 0 no stats"]
    full = d_in == 128 and d_out == 128
    if tile_mode(R, G):
        out = [f"k_tlin_fwd_tile<8,{_b(stats)}>", "fwd blocks = tiles"]
    else:
        out = [f"k_tlin_fwd<8,8,{_b(stats)},true,SPLIT>" if full and w_vec else f"k_tlin_fwd<8,8,{_b(stats)},{_b(full)}>",
               "fwd blocks capped at CUs/G" if cdiv(cdiv(R, 16), 4) > max(cus // G, 1) else "fwd blocks = tiles/4"]
    if in_scale:
        out.append("in_scale + in_relu" if in_relu else "in_scale")
    elif in_relu:
        out.append("in_relu")
    return out + (["bias"] if bias else []) + (["out_relu"] if out_relu else []) + [_nv(K)]


def bwd_kind(R, G, d_in, d_out, gx):
    if tile_mode(R, G):
        return "tile"
    return "split" if d_in == 128 and d_out == 128 and gx else "persistent"


def bwd_branch(R, G, d_in, d_out, gx=True, coef=False, merge=False, mask=False, x_state=False, x_relu=False, sums=False, acc=False,
               dot=False, want_db=False, cus=CUS):
    """sn_train_linear_bwd_f32"""
    if x_relu and not x_state:          # the dW product forms relu(.) only behind the operand's affine: refused before any launch
        return ["SN_REQUIRE x_relu needs x_scale"]
    if R == 0:
        return ["bwd R = 0"]
    full, kind = d_in == 128 and d_out == 128, bwd_kind(R, G, d_in, d_out, gx)
    kern = {"tile": f"k_tlin_bwd<8,8,{_b(full)},1>", "split": "k_tlin_bwd<8,8,true,2,SPLIT>", "persistent": f"k_tlin_bwd<8,8,{_b(full)},4>"}[kind]
    blocks = "bwd blocks = R/16" if kind == "tile" else ("bwd blocks capped at CUs/G" if cdiv(R, 64) > max(cus // G, 1) else "bwd blocks = R/64")
    arms = [n for n, on in (("coef", coef), ("merge", merge), ("mask", mask), ("x_state + x_relu", x_state and x_relu),
                            ("x_state", x_state and not x_relu), ("x_mean + sums_part", sums),
                            ("gx_accumulate", acc), ("dot_x", dot), ("want_db", want_db), ("no db", not want_db), ("gx = null", not gx)) if on]
    return [kern, blocks] + [f"{a} @{kind}" for a in arms]


def bn_bwd_branch(R, G, cus=CUS):
    """sn_train_bn_bwd_blocks"""
    want = cdiv(max(R, 1), 32 if tile_mode(R, G) else 128)
    if want > max(2 * cus // G, 1):
        return "bn_bwd_blocks capped at 2·CUs/G"
    return "bn_bwd_blocks R/32" if tile_mode(R, G) else "bn_bwd_blocks R/128"


def _c16(kernel, C):
    return f"{kernel} C % 16 {'!=' if C % 16 else '=='} 0"


class Trace:
    """atoms in launch order (no repeats), the (R, G) every blocks entry point is asked for, and the counted calls per variant"""

    def __init__(self, cus):
        self.cus, self.atoms, self.shapes, self.calls = cus, [], [], {}

    def add(self, atoms):
        for a in atoms:
            if a not in self.atoms:
                self.atoms.append(a)

    def call(self, variant, name, n=1):
        self.calls.setdefault(variant, Counter())[name] += n

    def fwd(self, R, G, d_in, d_out, bn, K, **kw):
        self.add(fwd_branch(R, G, d_in, d_out, bn, K, cus=self.cus, **kw))
        self.shapes.append(("fwd", R, G))
        if bn and R > 0:
            self.add([_c16("k_tbn_finish", d_out)])

    def apply(self, R, relu, res):
        if R > 0:
            self.add(["k_tbn_apply relu" if relu else "k_tbn_apply no relu", "k_tbn_apply residual" if res else "k_tbn_apply no residual"])

    def bn_sums(self, R, G):
        self.add([bn_bwd_branch(R, G, self.cus)])
        self.shapes.append(("bn", R, G))

    def bn_finish(self, variant, C):
        self.add([_c16("k_tbn_bwd_finish", C)])
        self.call(variant, "sn_train_bn_bwd_finish_f32")

    def bwd(self, variant, R, G, d_in, d_out, fuse_bn=False, **kw):
        """the link and the reduction behind it (train_stage.linear_bwd)"""
        direct, _, defer = VARIANTS[variant]
        self.add(bwd_branch(R, G, d_in, d_out, cus=self.cus, **kw))
        self.shapes.append(("bwd", R, G))
        dot, want_db = kw.get("dot", False), kw.get("want_db", False)
        if direct and defer and not fuse_bn:
            self.add(["reduce_jobs"] + (["dot_jobs"] if dot else []))
            self.call(variant, "sn_train_reduce_jobs_f32", 0)          # (one launch per backward pass: counted by the op's trace)
        elif direct and (fuse_bn or dot or want_db):
            self.add(["post_link + bn finish" if fuse_bn else "post_link"] + (["post_link + dot"] if dot else []))
            self.call(variant, "sn_train_post_link_f32")
        elif direct:
            self.add(["reduce_parts accumulate"])
            self.call(variant, "sn_train_reduce_parts_f32")
        else:
            self.add(["reduce_parts overwrite"] + (["dot_finish"] if dot else []))
            self.call(variant, "sn_train_reduce_parts_f32")
            if dot:
                self.call(variant, "sn_train_dot_finish_f64")

    def deferred(self, variant, dot=False):
        """the end of a backward pass: one launch for every deferred dW / db, one for the eps gradients"""
        direct, _, defer = VARIANTS[variant]
        if direct and defer:
            self.call(variant, "sn_train_reduce_jobs_f32")
            if dot:
                self.call(variant, "sn_train_dot_jobs_f64")


def _mlp2_fwd(t, R, G, K, d, bias, bn2, relu_out, res, w_vec=True):
    t.fwd(R, G, d[0], d[1], True, K, bias=bias, w_vec=w_vec)
    t.fwd(R, G, d[1], d[2], bn2, K, bias=bias, in_scale=True, in_relu=True, w_vec=w_vec)
    if bn2:
        t.apply(R, relu_out, res)


def _mlp2_bwd(t, v, R, G, d, bias, bn2, relu_out, want_dx, dot=False):
    """train_stage._mlp2_backward under launch structure v"""
    direct, merge, defer = VARIANTS[v]
    can_merge = direct and merge and R > 0
    if bn2:
        t.bn_sums(R, G)
        if not can_merge:
            t.bn_finish(v, d[2])
    fuse_bn = direct and not can_merge                  # the finish of bn1 inside the post launch of the second link
    t.bwd(v, R, G, d[1], d[2], fuse_bn=fuse_bn, coef=bn2 and not can_merge, merge=bn2 and can_merge, mask=bn2 and relu_out, x_state=True,
          x_relu=True, sums=True, want_db=bias)
    if not can_merge and not fuse_bn:
        t.bn_finish(v, d[1])
    elif fuse_bn:
        t.add([_c16("k_tbn_bwd_finish", d[1])])
    t.bwd(v, R, G, d[0], d[1], gx=want_dx, coef=not can_merge, merge=can_merge, dot=dot, want_db=bias)


def _link_bwd(t, v, R, d, bias, relu, want_dx, bn):
    direct, merge, defer = VARIANTS[v]
    can_merge = bn and direct and merge and R > 0
    if bn:
        t.bn_sums(R, 1)
        if not can_merge:
            t.bn_finish(v, d[1])
    t.bwd(v, R, 1, d[0], d[1], gx=want_dx, coef=bn and not can_merge, merge=can_merge, mask=relu, want_db=bias)


def trace(case, cus=CUS):
    p, t = case.p, Trace(cus)
    op, d = case.op, p.get("d")
    R, G, K = rows_of(case), p.get("G", 1), slots_of(case)
    w_vec = not p.get("wview")
    if op == "mlp2_bn":
        _mlp2_fwd(t, R, G, K, d, p["bias"], p["bn2"], p["relu_out"], p["res"], w_vec)
        for v in p["variants"]:
            _mlp2_bwd(t, v, R, G, d, p["bias"], p["bn2"], p["relu_out"], p["want_dx"])
    elif op == "gin_layer":
        t.add(["gin_aggregate" + (" doubled plan" if G == 2 else "")])
        _mlp2_fwd(t, R, G, K, (d, d, d), p["bias"], True, True, True)
        for v in p["variants"]:
            _mlp2_bwd(t, v, R, G, (d, d, d), p["bias"], True, True, True, dot=True)
    elif op == "gine_layer":
        t.add(["gine_aggregate" + (" [L,E,C] block" if p["block"] else "")])
        for _ in range(2 if p["block"] else 1):
            _mlp2_fwd(t, R, 1, K, (d, d, d), p["bias"], True, True, True)
        for v in p["variants"]:
            for _ in range(2 if p["block"] else 1):
                _mlp2_bwd(t, v, R, 1, (d, d, d), p["bias"], True, True, True, dot=True)
    elif op == "lin_bn":
        t.fwd(R, 1, d[0], d[1], True, K, bias=p["bias"], w_vec=w_vec)
        t.apply(R, p["relu"], p["res"])
        for v in p["variants"]:
            _link_bwd(t, v, R, d, p["bias"], p["relu"], p["want_dx"], True)
    elif op == "linear":
        t.fwd(R, 1, d[0], d[1], False, K, bias=p["bias"], out_relu=p["relu"], w_vec=w_vec)
        for v in p["variants"]:
            _link_bwd(t, v, R, d, p["bias"], p["relu"], p["want_dx"], False)
    elif op == "qkv":
        for _ in range(3):
            t.fwd(R, 1, d, d, False, K)
        for v in p["variants"]:
            for i in range(3):
                t.bwd(v, R, 1, d, d, acc=i > 0)
    elif op == "sign_sum":
        t.add(["k_masked_affine residual", "repeat(2, 1)"])
    elif op == "scalar_mlp":
        t.add(["k_smlp" + (" negate_second" if G == 2 else ""), bn_bwd_branch(R, G, cus)] + [f"k_smlp accumulate {_b(VARIANTS[v][0])}" for v in p["variants"]])
        t.shapes.append(("bn", R, G))
    elif op == "raw_link":
        im = p["in_mode"] or ""
        t.fwd(R, G, d[0], d[1], False, K, bias=p["bias"], in_scale="scale" in im, in_relu="relu" in im, out_relu=p["out_relu"],
              w_vec=not p["wview"])
        if im == "relu":          # the forward's in_relu-alone arm has no backward of its own: refused, then run as x_scale = 1, x_shift = 0
            t.add(bwd_branch(R, G, d[0], d[1], x_relu=True, cus=cus))
        t.add(bwd_branch(R, G, d[0], d[1], gx=True, mask=p["out_relu"], x_state=bool(im), x_relu="relu" in im, want_db=p["bias"], cus=cus)
              + ["reduce_parts overwrite"] + (["ldx > d_in"] if p["ldx"] else []))
        t.shapes.append(("bwd", R, G))
    else:
        raise KeyError(op)
    if op not in ("sign_sum", "scalar_mlp", "raw_link"):
        for v in p["variants"]:
            t.deferred(v, dot=op in ("gin_layer", "gine_layer"))
    return t


def branch_of(case, cus=CUS):
    return " | ".join(trace(case, cus).atoms)


# ============================================================================ rows
class Row(Case):
    def __init__(self, op, branch, **p):
        super().__init__(op, " | ".join(branch) if isinstance(branch, (list, tuple)) else branch, **p)


ALL_DIRECT = ("autograd", "direct", "direct-nomerge", "direct-nodefer", "direct-plain")
TWO = ("autograd", "direct")
VIEW = ("autograd",)


@functools.lru_cache(maxsize=None)
def graphs(n, seed=41):
    """a synth.make_batch molecule batch -> ei [2, E], batch [N], sizes"""
    from signnet_basisnet_amd import synth
    data = synth.make_batch(n, seed=seed)
    return types.SimpleNamespace(ei=data.edge_index, batch=data.batch, sizes=list(data.sizes), N=int(data.batch.numel()), E=int(data.edge_index.shape[1]))


def rows_of(case):
    """rows per group"""
    p = case.p
    if case.op == "gin_layer":
        return graphs(p["graphs"]).N * p["K"]
    if case.op == "gine_layer":
        return graphs(p["graphs"]).N
    return p["R"]


def slots_of(case):
    """K as the kernels get it (0: nvalid null)"""
    p = case.p
    if case.op == "gin_layer":
        return p["K"]
    if case.op == "gine_layer":
        return 1 if p["padded"] else 0
    m = p.get("mask")
    if m is None:
        return 0
    return slots_for(p["R"])[1] if m == "ragged" else 1


def _mlp2(br, d, G, R, mask, bias=False, bn2=True, relu_out=True, res=True, want_dx=True, wview=None, variants=TWO):
    return Row("mlp2_bn", br, d=d, G=G, R=R, mask=mask, bias=bias, bn2=bn2, relu_out=relu_out, res=res, want_dx=want_dx, wview=wview,
               variants=variants)


def _linbn(br, d, R, mask, bias=False, relu=True, res=False, want_dx=True, wview=None, variants=TWO):
    return Row("lin_bn", br, d=d, R=R, mask=mask, bias=bias, relu=relu, res=res, want_dx=want_dx, wview=wview, variants=variants)


def _lin(br, d, R, mask, bias=False, relu=False, want_dx=True, wview=None, variants=TWO):
    return Row("linear", br, d=d, R=R, mask=mask, bias=bias, relu=relu, want_dx=want_dx, wview=wview, variants=variants)


def _raw(br, d, R, G, mask, in_mode, bias=False, out_relu=False, ldx=None, wview=None):
    return Row("raw_link", br, d=d, R=R, G=G, mask=mask, in_mode=in_mode, bias=bias, out_relu=out_relu, ldx=ldx, wview=wview)


# What a row NAMES (its `branch`): the kernels, the workgroup-count rules and the no-row exits of its launches, in launch order — the
# atoms KERNEL_LEVEL() selects from trace().  The CPU test asserts that trace() gives exactly these; the runtime arms a row walks come
# from trace() alone and are pinned per op by ARMS below.
FT, FN, FB = "k_tlin_fwd_tile<8,true>", "k_tlin_fwd_tile<8,false>", "fwd blocks = tiles"
F4, FC = "fwd blocks = tiles/4", "fwd blocks capped at CUs/G"
B16, B64, BC = "bwd blocks = R/16", "bwd blocks = R/64", "bwd blocks capped at CUs/G"
N32, N128, NC = "bn_bwd_blocks R/32", "bn_bwd_blocks R/128", "bn_bwd_blocks capped at 2·CUs/G"
BSPLIT = "k_tlin_bwd<8,8,true,2,SPLIT>"
REFUSED = "SN_REQUIRE x_relu needs x_scale"


def fk(stats, full, split=False):
    return f"k_tlin_fwd<8,8,{_b(stats)},{_b(full)}{',SPLIT' if split else ''}>"


def bk(full, rt):
    return f"k_tlin_bwd<8,8,{_b(full)},{rt}>"


_KERNEL_PREFIX = ("k_tlin_", "fwd blocks", "bwd blocks", "fwd R = 0", "bwd R = 0", "bn_bwd_blocks", "k_masked_affine", "repeat(", "SN_REQUIRE")


def kernel_level(atoms):
    return [a for a in atoms if a.startswith(_KERNEL_PREFIX)]


def _rows():
    S_TILE_T, S_TILE_F = [FT, FB, N32, bk(True, 1), B16], [FT, FB, N32, bk(False, 1), B16]
    S_SPLIT = [fk(True, True, True), F4, N128, BSPLIT, B64]
    S_PERS = [fk(True, False), F4, N128, bk(False, 4), B64]
    return [
        # ---- mlp2_bn: around the tile-mode switch at 512 row tiles
        _mlp2(S_TILE_T, (128, 128, 128), 1, 8192, "ragged", variants=ALL_DIRECT),               # G = 1: the last tile-mode count, R % 16 = 0
        _mlp2(S_SPLIT, (128, 128, 128), 1, 8193, "ragged", bias=True, variants=ALL_DIRECT),     # the first persistent one: split, R % 16 = 1
        _mlp2(S_TILE_F, (64, 64, 64), 2, 4096, "rows", bias=True),                              # G = 2: last tile-mode count, K = 1 mask
        _mlp2(S_PERS, (64, 64, 64), 2, 4097, "ragged", bias=True, variants=ALL_DIRECT),         # first persistent, R % 64 = 1: a last round of one row
        _mlp2(S_PERS, (20, 108, 124), 3, 2721, "ragged", bias=True),                            # G = 3: 171 x 3 = 513 tiles
        _mlp2([fk(True, True, True), FC, N128, BSPLIT, BC], (128, 128, 128), 2, 8209, None),    # fwd ceil(514/4) = 129, bwd ceil(8209/64) = 129 > 256/2
        _mlp2([fk(True, False), FC, NC, bk(False, 4), BC], (4, 4, 4), 4, 16385, "rows", bias=True, relu_out=False),      # G = 4: every cap; bn_bwd ceil(16385/128) = 129 > 128
        _mlp2(S_TILE_F, (4, 128, 4), 1, 47, None, bias=True, res=False),                        # unequal widths both ways, R % 16 = 15
        _mlp2([FT, FB, FN, bk(False, 1), B16], (32, 128, 64), 1, 135, "ragged", bias=True, bn2=False, res=False),       # bn2 = None: the second link without coef / merge / stats
        _mlp2(S_TILE_F, (64, 64, 64), 2, 80, "last"),                                           # every valid row in the last workgroup's range
        _mlp2(S_TILE_F, (108, 108, 108), 2, 240, "ragged", bias=True, relu_out=False, res=False),      # bn_apply without ReLU and residual
        _mlp2([fk(True, True), F4, N128, BSPLIT, B64], (128, 128, 128), 1, 8193, "ragged", wview="ld", variants=VIEW),   # ldw = 129: the non-split full-width forward with stats
        _mlp2(S_SPLIT + [bk(True, 4)], (128, 128, 128), 1, 8193, None, want_dx=False),          # first layer, no input gradient: k_tlin_bwd<8,8,true,4>
        _mlp2([fk(True, False), F4, fk(False, False), bk(False, 4), B64], (64, 64, 64), 1, 8193, "ragged", bn2=False, res=False, want_dx=False),
        # ---- lin_bn
        _linbn(S_SPLIT, (128, 128), 8193, "ragged", relu=True, res=True, variants=ALL_DIRECT),
        _linbn(S_TILE_F, (128, 4), 33, "rows", bias=True, relu=False, variants=ALL_DIRECT),
        _linbn(S_TILE_F, (4, 128), 47, None, bias=True, relu=True, res=True, want_dx=False),
        _linbn(S_PERS, (64, 108), 8193, None, relu=True, variants=ALL_DIRECT),
        _linbn([fk(True, True), F4, N128, BSPLIT, B64], (128, 128), 8193, None, relu=False, wview="off", variants=VIEW),
        _linbn(["fwd R = 0 memset", N32, "bwd R = 0"], (64, 64), 0, None, bias=True),            # no rows: memset of the moment partials, no launch
        # ---- linear
        _lin([fk(False, True, True), F4, BSPLIT, B64], (128, 128), 8193, "ragged", bias=True, relu=True, variants=("autograd", "direct", "direct-nodefer")),
        _lin([fk(False, True), F4, BSPLIT, B64], (128, 128), 8193, None, wview="off", variants=VIEW),        # weight one float off: non-split forward, no stats
        _lin([fk(False, True, True), F4, bk(True, 4), B64], (128, 128), 8193, None, bias=True, want_dx=False),
        _lin([FN, FB, bk(True, 1), B16], (128, 128), 64, "rows", want_dx=False, variants=("autograd", "direct", "direct-nodefer")),     # gx = null
        _lin([fk(False, False), F4, bk(False, 4), B64], (64, 64), 8193, None, relu=True, variants=("autograd", "direct", "direct-nodefer")),
        _lin([FN, FB, bk(False, 1), B16], (4, 128), 5, None, bias=True),                         # fewer rows than one tile
        _lin([FN, FB, bk(False, 1), B16], (128, 4), 16, "rows", relu=True, wview="ld", variants=VIEW),
        _lin(["fwd R = 0 no stats", "bwd R = 0"], (64, 64), 0, None, bias=True),
        # ---- qkv: the only user of gx_accumulate
        Row("qkv", [fk(False, True, True), F4, BSPLIT, B64], d=128, R=8193, mask="ragged", variants=("autograd", "direct", "direct-nodefer")),
        Row("qkv", [fk(False, False), F4, bk(False, 4), B64], d=64, R=8193, mask=None, variants=TWO),
        Row("qkv", [FN, FB, bk(False, 1), B16], d=20, R=47, mask="rows", variants=("autograd", "direct", "direct-nodefer")),
        # ---- sign_sum
        Row("sign_sum", ["k_masked_affine residual", "repeat(2, 1)"], d=128, R=100, mask="ragged"),
        Row("sign_sum", ["k_masked_affine residual", "repeat(2, 1)"], d=20, R=33, mask=None),
        # ---- gin_layer / gine_layer: the only users of dot_x, dot_part and the eps gradient
        Row("gin_layer", S_SPLIT, d=128, G=2, graphs=14, K=16, bias=False, variants=ALL_DIRECT),       # 2 x (N * 16) rows: split
        Row("gin_layer", S_PERS, d=64, G=2, graphs=14, K=16, bias=True, variants=ALL_DIRECT),          # persistent
        Row("gin_layer", S_TILE_F, d=20, G=2, graphs=3, K=16, bias=True, variants=ALL_DIRECT),         # tile mode
        Row("gin_layer", S_TILE_T, d=128, G=1, graphs=3, K=16, bias=False, variants=TWO),
        Row("gine_layer", S_TILE_T, d=128, graphs=5, block=False, padded=False, bias=False, variants=ALL_DIRECT),
        Row("gine_layer", S_TILE_F, d=64, graphs=6, block=True, padded=False, bias=True, variants=TWO),
        Row("gine_layer", S_TILE_F, d=20, graphs=6, block=False, padded=True, bias=True, variants=TWO),             # nvalid with K = 1: a padded batch
        # ---- scalar_mlp
        Row("scalar_mlp", [N32], d=12, G=2, R=240, mask="ragged", variants=TWO),
        Row("scalar_mlp", [N32], d=20, G=1, R=57, mask="rows", variants=TWO),
        Row("scalar_mlp", [N128], d=4, G=1, R=8193, mask="ragged", variants=TWO),                # past the tile-mode switch: R/128 workgroups
        # ---- raw entry points: the operand arms no public function reaches, column slices, poisoned padding
        _raw([FN, FB, bk(False, 1), B16], (64, 64), 100, 2, "rows", "scale", bias=True, ldx=72),
        _raw([FN, FB, REFUSED, bk(False, 1), B16], (64, 20), 100, 1, "ragged", "relu", out_relu=True),
        _raw([fk(False, True), F4, REFUSED, BSPLIT, B64], (128, 128), 8193, 1, None, "relu", bias=True, ldx=136, wview="ld"),
        _raw([fk(False, False), F4, bk(False, 4), B64], (108, 64), 4097, 2, "ragged", "scale+relu", ldx=112),
    ]


# ============================================================================ generators
def make_mask(R, mask, g):
    """-> (nvalid int32 or None, K, bool [R])"""
    if mask is None or R == 0:
        return None, 0, torch.ones(R, dtype=torch.bool)
    if mask == "ragged":
        N, K = slots_for(R)
        nv = ragged_nvalid(N, K, g, zeros=(K == 1))
    elif mask == "rows":
        K, nv = 1, (torch.rand(R, generator=g) < 0.8).to(torch.int32)
        nv[0], nv[R // 2] = 1, 0
    elif mask == "last":                      # the rows of the last 16-row tile: every other workgroup's moment / column-sum partials have count 0
        K, nv = 1, torch.zeros(R, dtype=torch.int32)
        nv[(R - 1) // 16 * 16:] = 1
    else:
        raise KeyError(mask)
    return nv, K, row_mask(nv, K, R)


def push_rows(x, pre_fn, valid, iters=100):
    """Move rows of the fp32 input x until every valid element of every pre-activation pre_fn(x64) -> [a [rows, P], ...] is PUSH of its
    tensor's rms away from zero: a row with an offending element a[r, o] moves along d a[r, o] / d x[r] by what shifts that element to the
    far side of 3 * PUSH * rms (first order; the batch statistics and the other elements of the row move by less; repeated)."""
    shape = x.shape
    for _ in range(iters):
        xd = x.double().reshape(shape[0], -1).requires_grad_(True)
        pres = pre_fn(xd.reshape(shape))
        an = torch.cat([a / a.detach()[valid].pow(2).mean().sqrt() for a in pres], 1)
        bad = (an.detach().abs() < PUSH) & valid[:, None]
        if not bool(bad.any()):
            return x
        rows = bad.any(1).nonzero()[:, 0]
        col = bad[rows].to(torch.uint8).argmax(1)
        sel = an[rows, col]
        (J,) = torch.autograd.grad(sel.sum(), xd)
        xr = rows % shape[0]
        Jr = J[xr]
        n2 = (Jr * Jr).sum(1)
        assert bool((n2 > 1e-12).all()), "push_rows: a pre-activation near zero that the input row does not move"
        step = torch.where(sel.detach() >= 0, 1.0, -1.0) * 3 * PUSH
        xn = xd.detach().clone()
        xn.index_add_(0, xr, step[:, None] * Jr / n2[:, None])
        x = xn.float().reshape(shape)
    raise AssertionError("push_rows: pre-activations near zero remain")


def _params(L, g, names):
    """names: (key, d_in, d_out, bias, bn)"""
    for key, d_in, d_out, bias, bn in names:
        L["W" + key] = torch.randn(d_out, d_in, generator=g) / d_in ** 0.5
        if bias:
            L["b" + key] = torch.randn(d_out, generator=g) * 0.5
        if bn:
            L["g" + key], L["be" + key] = torch.rand(d_out, generator=g) + 0.5, torch.randn(d_out, generator=g) * 0.3
    return L


def _bn(z, m, gamma, beta, stats, key):
    zv = z[m]
    if zv.shape[0] == 0:
        return z * gamma + beta
    mean, var = zv.mean(0), zv.var(0, unbiased=False)
    if stats is not None:
        stats.setdefault(key, []).append((mean.detach(), zv.detach().var(0, unbiased=True)))
    return (z - mean) / torch.sqrt(var + BN_EPS) * gamma + beta


def _link(x, L, key, m, stats, pres, relu=True, bn=True):
    z = x @ L["W" + key].t() + (L["b" + key] if "b" + key in L else 0)
    a = _bn(z, m, L["g" + key], L["be" + key], stats, "bn" + key) if bn else z
    if relu and pres is not None:
        pres.append(a)
    return torch.relu(a) if relu else a


def _mlp2_ref(u, L, m, G, keys=("1", "2"), bn2=True, relu_out=True, stats=None, pres=None):
    """[G * R, d] -> relu(bn2(lin2(relu(bn1(lin1 u))))) per group, unmasked; pres: the ReLU pre-activations, groups stacked"""
    mf, R = m.to(u.dtype)[:, None], m.numel()
    ys, p1, p2 = [], [], []
    for ug in u.reshape(G, R, u.shape[-1]):
        h = _link(ug, L, keys[0], m, stats, p1) * mf
        ys.append(_link(h, L, keys[1], m, stats, p2, relu=bn2 and relu_out, bn=bn2))
    if pres is not None:
        pres.append(torch.cat(p1, 0))
        if p2:
            pres.append(torch.cat(p2, 0))
    return torch.cat(ys, 0)


def _f64(L):
    return {k: v.double() for k, v in L.items()}


def _push(L, key, fn, valid, G):
    """push the input L[key]; fn(L64 with the input replaced) -> pres"""
    L64 = _f64(L)

    def pre(x64):
        pres = []
        fn({**L64, key: x64}, pres)
        return pres
    vv = valid.repeat(G)
    if bool(vv.any()):
        L[key] = push_rows(L[key], pre, vv)


def mlp2_gen(p):
    d, G, R = p["d"], p["G"], p["R"]
    g = rng(21, *d, G, R, p["bias"], p["bn2"])
    nv, K, valid = make_mask(R, p["mask"], g)
    aux = dict(nv=nv, K=K, valid=valid, G=G)
    L = {"x": torch.randn(G * R, d[0], generator=g) * valid.repeat(G)[:, None]}
    _params(L, g, (("1", d[0], d[1], p["bias"], True), ("2", d[1], d[2], p["bias"], p["bn2"])))
    if p["res"]:
        L["res"] = torch.randn(G * R, d[2], generator=g) * valid.repeat(G)[:, None]
    _push(L, "x", lambda L64, pres: mlp2_ref(p, aux, L64, pres=pres), valid, G)
    return L, aux


def mlp2_ref(p, aux, L, stats=None, pres=None):
    m, G = aux["valid"], aux["G"]
    y = _mlp2_ref(L["x"], L, m, G, bn2=p["bn2"], relu_out=p["relu_out"], stats=stats, pres=pres)
    if "res" in L:
        y = y + L["res"]
    return (y * m.repeat(G)[:, None].to(y.dtype),)


def lin_bn_gen(p):
    d, R = p["d"], p["R"]
    g = rng(22, *d, R, p["bias"], p["relu"])
    nv, K, valid = make_mask(R, p["mask"], g)
    aux = dict(nv=nv, K=K, valid=valid, G=1)
    L = _params({"x": torch.randn(R, d[0], generator=g) * valid[:, None]}, g, (("", d[0], d[1], p["bias"], True),))
    if p["res"]:
        L["res"] = torch.randn(R, d[1], generator=g) * valid[:, None]
    if p["relu"]:
        _push(L, "x", lambda L64, pres: lin_bn_ref(p, aux, L64, pres=pres), valid, 1)
    return L, aux


def lin_bn_ref(p, aux, L, stats=None, pres=None):
    y = _link(L["x"], L, "", aux["valid"], stats, pres, relu=p["relu"])
    if "res" in L:
        y = y + L["res"]
    return (y * aux["valid"][:, None].to(y.dtype),)


def linear_gen(p):
    d, R = p["d"], p["R"]
    g = rng(23, *d, R, p["bias"], p["relu"])
    nv, K, valid = make_mask(R, p["mask"], g)
    aux = dict(nv=nv, K=K, valid=valid, G=1)
    L = _params({"x": torch.randn(R, d[0], generator=g) * valid[:, None]}, g, (("", d[0], d[1], p["bias"], False),))
    if p["relu"]:
        _push(L, "x", lambda L64, pres: linear_ref(p, aux, L64, pres=pres), valid, 1)
    return L, aux


def linear_ref(p, aux, L, stats=None, pres=None):
    y = _link(L["x"], L, "", aux["valid"], stats, pres, relu=p["relu"], bn=False)
    return (y * aux["valid"][:, None].to(y.dtype),)


def qkv_gen(p):
    d, R = p["d"], p["R"]
    g = rng(24, d, R)
    nv, K, valid = make_mask(R, p["mask"], g)
    L = {"x": torch.randn(R, d, generator=g) * valid[:, None]}
    for k in "qkv":
        L["W" + k] = torch.randn(d, d, generator=g) / d ** 0.5
    return L, dict(nv=nv, K=K, valid=valid, G=1)


def qkv_ref(p, aux, L, stats=None, pres=None):
    m = aux["valid"][:, None].to(L["x"].dtype)
    return tuple((L["x"] @ L["W" + k].t()) * m for k in "qkv")


def sign_sum_gen(p):
    d, R = p["d"], p["R"]
    g = rng(25, d, R)
    nv, K, valid = make_mask(R, p["mask"], g)
    return {"x": torch.randn(2 * R, d, generator=g) * valid.repeat(2)[:, None]}, dict(nv=nv, K=K, valid=valid, G=1)


def sign_sum_ref(p, aux, L, stats=None, pres=None):
    R = aux["valid"].numel()
    return ((L["x"][:R] + L["x"][R:]) * aux["valid"][:, None].to(L["x"].dtype),)


def gin_gen(p):
    d, G, K = p["d"], p["G"], p["K"]
    gr = graphs(p["graphs"])
    g = rng(26, d, G, gr.N, K)
    nv = torch.repeat_interleave(torch.tensor([min(n, K) for n in gr.sizes], dtype=torch.int32), torch.tensor(gr.sizes))   # = plan.nvalid
    valid = row_mask(nv, K, gr.N * K)
    aux = dict(nv=nv, K=K, valid=valid, G=G, gr=gr)
    L = {"x": torch.randn(G * gr.N * K, d, generator=g) * valid.repeat(G)[:, None], "eps": torch.tensor([0.3])}
    _params(L, g, (("1", d, d, p["bias"], True), ("2", d, d, p["bias"], True)))
    _push(L, "x", lambda L64, pres: gin_ref(p, aux, L64, pres=pres), valid, G)
    return L, aux


def gin_ref(p, aux, L, stats=None, pres=None):
    """relu(bn2(lin2(relu(bn1(lin1((1 + eps) x + sum_nbr x)))))) + x per group, over the node axis of [G, N, K * d]"""
    gr, G, K, x = aux["gr"], aux["G"], aux["K"], L["x"]
    xn = x.reshape(G, gr.N, -1)
    a = (1 + L["eps"]) * xn + torch.zeros_like(xn).index_add_(1, gr.ei[1], xn[:, gr.ei[0]])
    y = _mlp2_ref(a.reshape(x.shape), L, aux["valid"], G, stats=stats, pres=pres) + x
    return (y * aux["valid"].repeat(G)[:, None].to(y.dtype),)


def gine_gen(p):
    d = p["d"]
    gr = graphs(p["graphs"])
    g = rng(27, d, gr.N, p["block"], p["padded"])
    nv, K, valid = None, 0, torch.ones(gr.N, dtype=torch.bool)
    if p["padded"]:                 # the nodes of the last graph and of the third are padding (0 / 1 per node, K = 1)
        nv, K = torch.ones(gr.N, dtype=torch.int32), 1
        nv[gr.batch == len(gr.sizes) - 1] = 0
        nv[gr.batch == 2] = 0
        valid = nv.bool()
    Ln = 2 if p["block"] else 1
    aux = dict(nv=nv, K=K, valid=valid, G=1, gr=gr, layers=Ln)
    L = {"x": torch.randn(gr.N, d, generator=g) * valid[:, None]}
    L["e"] = torch.randn(Ln, gr.E, d, generator=g) if p["block"] else torch.randn(gr.E, d, generator=g)
    for l in range(Ln):
        L[f"eps{l}"] = torch.tensor([0.3 - 0.5 * l])
        _params(L, g, ((f"{l}a", d, d, p["bias"], True), (f"{l}b", d, d, p["bias"], True)))
    _push(L, "x", lambda L64, pres: gine_ref(p, aux, L64, pres=pres), valid, 1)
    return L, aux


def gine_ref(p, aux, L, stats=None, pres=None):
    """h -> relu(bn2(lin2(relu(bn1(lin1((1 + eps) h + sum_j relu(h_j + e_ji))))))) + h, one or two layers (the block form: layer l reads
    plane l of e).  The message ReLU is not pushed: relu(h_j + e_ji) has 1e3 .. 1e4 elements and a free e, and its decisions are the
    aggregation kernel's (tests/test_topology_gpu.py), a producer here."""
    gr, m, h = aux["gr"], aux["valid"], L["x"]
    mf = m[:, None].to(h.dtype)
    for l in range(aux["layers"]):
        e = L["e"][l] if p["block"] else L["e"]
        u = (1 + L[f"eps{l}"]) * h + torch.zeros_like(h).index_add_(0, gr.ei[1], torch.relu(h[gr.ei[0]] + e))
        h = (_mlp2_ref(u, L, m, 1, keys=(f"{l}a", f"{l}b"), stats=stats, pres=pres) + h) * mf
    return (h,)


def scalar_gen(p):
    d, G, R = p["d"], p["G"], p["R"]
    g = rng(28, d, G, R)
    nv, K, valid = make_mask(R, p["mask"], g)
    aux = dict(nv=nv, K=K, valid=valid, G=G)
    L = {"x": torch.randn(R, generator=g) * valid, "W1": torch.tensor([[1e-3]]), "g1": torch.rand(1, generator=g) + 0.5,
         "be1": torch.randn(1, generator=g) * 0.3, "W2": torch.randn(d, 1, generator=g) * 3e-3, "g2": torch.rand(d, generator=g) + 0.5,
         "be2": torch.randn(d, generator=g) * 0.3}
    _push(L, "x", lambda L64, pres: scalar_ref(p, aux, L64, pres=pres), valid, G)
    return L, aux


def scalar_ref(p, aux, L, stats=None, pres=None):
    """the literal composition Linear(1, 1).BN.ReLU.Linear(1, d).BN.ReLU on a and (G = 2) on -a"""
    a, m, G = L["x"], aux["valid"], aux["G"]
    x = torch.cat([a, -a] if G == 2 else [a])[:, None]
    y = _mlp2_ref(x, L, m, G, stats=stats, pres=pres)
    return (y * m.repeat(G)[:, None].to(y.dtype),)


def raw_gen(p):
    d, R, G = p["d"], p["R"], p["G"]
    g = rng(29, *d, R, G, len(p["in_mode"] or ""))
    nv, K, valid = make_mask(R, p["mask"], g)
    vv = valid.repeat(G)
    im = p["in_mode"] or ""
    s = (torch.rand(G, d[0], generator=g) + 0.5) if "scale" in im else torch.ones(G, d[0])
    t = (torch.randn(G, d[0], generator=g) * 0.3) if "scale" in im else torch.zeros(G, d[0])
    aux = dict(nv=nv, K=K, valid=valid, G=G, s=s, t=t)
    L = _params({"x": torch.randn(G * R, d[0], generator=g)}, g, (("", d[0], d[1], p["bias"], False),))      # invalid rows carry data: the kernel masks them
    if "relu" in im:          # the operand's own ReLU: the tensor in front of it is free
        sr, tr = s.double().repeat_interleave(R, 0), t.double().repeat_interleave(R, 0)
        L["x"] = push_elementwise(L["x"], lambda x64: (x64 * sr + tr, sr), vv)
    if p["out_relu"]:
        _push(L, "x", lambda L64, pres: raw_ref(p, aux, L64, pres=pres), valid, G)
    return L, aux


def raw_ref(p, aux, L, stats=None, pres=None):
    """y = [relu]([relu](x * s[g] + t[g]) W^T + b) on valid rows.  The kernel's gx is the gradient with respect to x * s + t — the operand
    the forward link formed on load — so the affine is applied to the VALUE of x only."""
    x, R = L["x"], aux["valid"].numel()
    xa = x * aux["s"].to(x.dtype).repeat_interleave(R, 0) + aux["t"].to(x.dtype).repeat_interleave(R, 0)
    xa = x + (xa - x).detach()
    im = p["in_mode"] or ""
    if "relu" in im:
        if pres is not None and not p["out_relu"]:
            pres.append(xa)
        xa = torch.relu(xa)
    y = xa @ L["W"].t() + (L["b"] if "b" in L else 0)
    if p["out_relu"]:
        if pres is not None:
            pres.append(y)
        y = torch.relu(y)
    return (y * aux["valid"].repeat(aux["G"])[:, None].to(y.dtype),)


def zero_bias(case):
    """leaves whose true gradient is 0: a bias in front of a batch-statistics BatchNorm"""
    p = case.p
    if case.op in ("gin_layer", "gine_layer"):
        return {k for k in ("b1", "b2", "b0a", "b0b", "b1a", "b1b")}
    if case.op == "mlp2_bn":
        return {"b1"} | ({"b2"} if p["bn2"] else set())
    return {"b"} if case.op == "lin_bn" else set()


OPS = {"mlp2_bn": (mlp2_gen, mlp2_ref), "lin_bn": (lin_bn_gen, lin_bn_ref), "linear": (linear_gen, linear_ref), "qkv": (qkv_gen, qkv_ref),
       "sign_sum": (sign_sum_gen, sign_sum_ref), "gin_layer": (gin_gen, gin_ref), "gine_layer": (gine_gen, gine_ref),
       "scalar_mlp": (scalar_gen, scalar_ref), "raw_link": (raw_gen, raw_ref)}


def wants_grad(case, name):
    return not (name == "x" and case.p.get("want_dx") is False)


def reference(case, dtype, L, aux, npass=1):
    """-> (outputs, {leaf: gradient} summed over npass backward passes with the cotangents of pass 0 .. npass - 1, BatchNorm statistics
    {site: [(mean, unbiased variance) per group]}, ReLU pre-activations)"""
    _, ref = OPS[case.op]
    X = {k: v.detach().to(dtype).requires_grad_(wants_grad(case, k)) for k, v in L.items()}
    stats, pres = {}, []
    outs = ref(case.p, aux, X, stats=stats, pres=pres)
    vv = aux["valid"].repeat(aux["G"] if outs[0].shape[0] != aux["valid"].numel() else 1)
    for i in range(npass):
        torch.autograd.backward(outs, [cots(case, i, j, o.shape, vv).to(dtype) for j, o in enumerate(outs)], retain_graph=i + 1 < npass)
    return [o.detach() for o in outs], {k: v.grad for k, v in X.items() if v.requires_grad}, stats, [a.detach() for a in pres]


def cots(case, i, j, shape, vv):
    """the cotangent of output j in pass i: zero on invalid rows (the convention of train_stage.py: every producer masks them)"""
    c = cotangent(7 * i + j, shape)
    return c * vv[:, None].to(c.dtype) if c.shape[0] == vv.numel() else c


# ============================================================================ the table and what it has to reach
TABLE = _rows()
BY_OP = {op: [c for c in TABLE if c.op == op] for op in OPS}

_KINDS = ("tile", "persistent", "split")
FWD_KERNELS = ({f"k_tlin_fwd_tile<8,{s}>" for s in ("true", "false")} | {f"k_tlin_fwd<8,8,{s},{f}>" for s in ("true", "false") for f in ("true", "false")} |
               {f"k_tlin_fwd<8,8,{s},true,SPLIT>" for s in ("true", "false")} |
               {"fwd R = 0 memset", "fwd R = 0 no stats", "fwd blocks = tiles", "fwd blocks = tiles/4", "fwd blocks capped at CUs/G"})
BWD_KERNELS = ({f"k_tlin_bwd<8,8,{f},{rt}>" for f in ("true", "false") for rt in (1, 4)} |
               {"k_tlin_bwd<8,8,true,2,SPLIT>", "bwd R = 0", "bwd blocks = R/16", "bwd blocks = R/64", "bwd blocks capped at CUs/G"})
BWD_ARMS = ({f"{a} @{k}" for a in ("coef", "merge", "mask", "x_state + x_relu", "x_mean + sums_part", "gx_accumulate", "dot_x", "want_db", "no db")
             for k in _KINDS} | {"gx = null @tile", "gx = null @persistent"})
FWD_ARMS = {"in_scale + in_relu", "in_scale", "in_relu", "bias", "out_relu", "nvalid null", "nvalid K > 1", "nvalid K = 1"}
BN_ATOMS = {"bn_bwd_blocks R/32", "bn_bwd_blocks R/128", "bn_bwd_blocks capped at 2·CUs/G", "k_tbn_apply relu", "k_tbn_apply no relu",
            "k_tbn_apply residual", "k_tbn_apply no residual", "k_tbn_finish C % 16 != 0", "k_tbn_finish C % 16 == 0",
            "k_tbn_bwd_finish C % 16 != 0", "k_tbn_bwd_finish C % 16 == 0"}
REDUCTIONS = {"reduce_parts overwrite", "reduce_parts accumulate", "reduce_jobs", "post_link", "post_link + bn finish", "post_link + dot",
              "dot_finish", "dot_jobs"}
OTHER = {"SN_REQUIRE x_relu needs x_scale", "x_state @tile", "ldx > d_in", "gin_aggregate", "gin_aggregate doubled plan", "gine_aggregate",
         "gine_aggregate [L,E,C] block", "k_masked_affine residual", "repeat(2, 1)", "k_smlp", "k_smlp negate_second",
         "k_smlp accumulate true", "k_smlp accumulate false"}
DECLARED = FWD_KERNELS | BWD_KERNELS | BWD_ARMS | FWD_ARMS | BN_ATOMS | REDUCTIONS | OTHER



def _at(arms, kinds=_KINDS):
    return {f"{a} @{k}" for a in arms for k in kinds}


_NV = {"nvalid null", "nvalid K > 1", "nvalid K = 1"}
_FIN = {"k_tbn_finish C % 16 != 0", "k_tbn_finish C % 16 == 0", "k_tbn_bwd_finish C % 16 != 0", "k_tbn_bwd_finish C % 16 == 0"}
_APPLY = {"k_tbn_apply relu", "k_tbn_apply no relu", "k_tbn_apply residual", "k_tbn_apply no residual"}
_LINK2 = ("coef", "merge", "mask", "x_state + x_relu", "x_mean + sums_part")
# what the rows of each op have to reach, and nothing else: kernels and workgroup-count rules first, then the runtime arms
BRANCHES = {
    "mlp2_bn": {FT, FN, FB, F4, FC, fk(True, True, True), fk(True, False), fk(True, True), fk(False, False), N32, N128, NC, bk(True, 1),
                bk(False, 1), bk(False, 4), bk(True, 4), BSPLIT, B16, B64, BC} | _NV | {"bias", "in_scale + in_relu"} | _FIN | _APPLY |
               _at(_LINK2 + ("want_db", "no db")) | {"gx = null @persistent", "reduce_parts overwrite", "reduce_parts accumulate", "reduce_jobs",
                                                    "post_link", "post_link + bn finish"},
    "lin_bn": {FT, FB, F4, fk(True, True, True), fk(True, False), fk(True, True), "fwd R = 0 memset", N32, N128, bk(False, 1), bk(False, 4),
               BSPLIT, "bwd R = 0", B16, B64} | _NV | {"bias"} | _FIN | _APPLY | _at(("coef", "merge", "mask")) |
              {"no db @split", "no db @persistent", "want_db @tile", "gx = null @tile", "reduce_parts overwrite", "reduce_parts accumulate",
               "reduce_jobs", "post_link"},
    "linear": {FN, FB, F4, fk(False, True, True), fk(False, True), fk(False, False), "fwd R = 0 no stats", BSPLIT, bk(True, 4), bk(True, 1),
               bk(False, 4), bk(False, 1), "bwd R = 0", B16, B64} | _NV | {"bias", "out_relu"} | _at(("mask", "want_db", "no db")) |
              {"gx = null @tile", "gx = null @persistent", "reduce_parts overwrite", "reduce_parts accumulate", "reduce_jobs", "post_link"},
    "qkv": {fk(False, True, True), fk(False, False), FN, FB, F4, BSPLIT, bk(False, 4), bk(False, 1), B16, B64} | _NV |
           _at(("no db", "gx_accumulate")) | {"reduce_parts overwrite", "reduce_parts accumulate", "reduce_jobs"},
    "sign_sum": {"k_masked_affine residual", "repeat(2, 1)"},
    "gin_layer": {FT, FB, F4, fk(True, True, True), fk(True, False), N32, N128, BSPLIT, bk(False, 4), bk(False, 1), bk(True, 1), B16, B64,
                  "gin_aggregate", "gin_aggregate doubled plan", "nvalid K > 1", "bias", "in_scale + in_relu", "k_tbn_apply relu",
                  "k_tbn_apply residual"} | _FIN | _at(_LINK2 + ("dot_x",)) |
                 {"want_db @persistent", "want_db @tile", "no db @split", "no db @tile"} | REDUCTIONS,
    "gine_layer": {FT, FB, N32, bk(True, 1), bk(False, 1), B16, "gine_aggregate", "gine_aggregate [L,E,C] block", "nvalid null", "nvalid K = 1",
                   "bias", "in_scale + in_relu", "k_tbn_apply relu", "k_tbn_apply residual"} | _FIN |
                  _at(_LINK2 + ("dot_x", "want_db", "no db"), ("tile",)) | REDUCTIONS,
    "scalar_mlp": {N32, N128, "k_smlp", "k_smlp negate_second", "k_smlp accumulate true", "k_smlp accumulate false"},
    "raw_link": {FN, FB, F4, fk(False, True), fk(False, False), bk(False, 1), BSPLIT, bk(False, 4), B16, B64, "in_scale", "in_relu",
                 "in_scale + in_relu", "bias", "out_relu", "x_state @tile", "SN_REQUIRE x_relu needs x_scale", "x_state + x_relu @tile", "x_state + x_relu @split", "x_state + x_relu @persistent",
                 "mask @tile", "want_db @tile", "want_db @split", "no db @tile", "no db @persistent", "reduce_parts overwrite", "ldx > d_in"} | _NV,
}


if __name__ == "__main__":
    for c in TABLE:
        print(c.id, "\n   ", branch_of(c))
