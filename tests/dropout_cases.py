"""The mask contract of sn_dropout_f32 restated in numpy, and the case tables of tests/test_dropout_gpu.py.

    i    = base + r*C + c
    w    = philox4x32_10(counter = (lo32(i>>2), hi32(i>>2), site, lo32(step)), key = (lo32(seed), hi32(seed)))
    keep = w[i & 3] >= floor(p * 2^32)

Philox4x32-10 is restated from Salmon, Moraes, Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11) and checked against
the Random123 known answers in tests/test_dropout_cases_cpu.py.  Pure numpy: no GPU, no torch.
"""
from collections import namedtuple

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two ints.  Returns the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK32) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]          # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        hi0, lo0 = p0 >> s32, p0 & m32
        hi1, lo1 = p1 >> s32, p1 & m32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0 = (k0 + W0) & MASK32
        k1 = (k1 + W1) & MASK32
    return [v.astype(np.uint32) for v in c]


def threshold_of(p):
    """floor(p * 2^32) in double precision (p < 1)."""
    return int(np.floor(np.float64(p) * np.float64(4294967296.0)))


def scale_of(p):
    return np.float32(1.0 / (1.0 - np.float64(p)))


def words(n, seed, step, site, base=0):
    """The uint32 word of each of the n logical indices base .. base + n - 1 (one generator call per aligned group of four)."""
    if n == 0:
        return np.zeros(0, np.uint32)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    g = np.arange(base >> 2, ((base + n - 1) >> 2) + 1, dtype=np.uint64)
    w = philox4x32_10((g & np.uint64(MASK32), g >> np.uint64(32), int(site) & MASK32, int(step) & MASK32), (seed & MASK32, seed >> 32))
    return np.stack(w, axis=-1).ravel()[base & 3:(base & 3) + n]


def keep_mask(R, C, p, seed, step, site, base=0):
    """bool [R, C]: the elements sn_dropout_f32 keeps."""
    return (words(R * C, seed, step, site, base) >= np.uint32(threshold_of(p))).reshape(R, C)


# ----------------------------------------------------------------------------- dispatch, restated from csrc/dropout.hip
MAX_BLOCKS = 2048
ONE_PASS_GROUPS = MAX_BLOCKS * 256          # more groups than this: the grid strides


def vector_path(C, base, lds, pointers):
    """The host's predicate: one generator call per 128-bit access."""
    return C % 4 == 0 and base % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(p % 16 == 0 for p in pointers)


def n_groups(R, C, base, vector):
    total = R * C
    if total == 0:
        return 0
    return total // 4 if vector else ((base + total - 1) >> 2) - (base >> 2) + 1


# ----------------------------------------------------------------------------- case tables
Case = namedtuple("Case", "id R C ld offset residual base p path")
# ld: None = plain (ld = C) or the row stride of x, residual and y;  offset: pointers 4 bytes off a 16-byte boundary;
# path: the branch the row must reach ('vector' / 'scalar' / 'none' for R = 0)

SHAPES = [(1, 1, None), (3, 5, None), (7, 4, None), (2, 128, None), (33, 77, None), (5, 68, 72), (0, 8, None)]
BIG = (2049, 1024)           # 2049 * 256 groups > ONE_PASS_GROUPS: the last row is the grid's second pass
PS = [0.1, 0.5, 0.9]
P_TINY = 2.0 ** -33          # threshold 0: keeps everything
BASES = [0, 3, (1 << 34) - 6]
SEED, STEP, SITE = 0x1234_5678_9ABC_DEF1, 41, 7


def _path(R, C, ld, offset, base):
    if R == 0:
        return "none"
    ldv = ld or C
    return "vector" if vector_path(C, base, [ldv], [4 if offset else 0]) else "scalar"


def _cases():
    out = []
    for k, (R, C, ld) in enumerate(SHAPES):
        p = PS[k % 3]
        for layout, (ldv, off) in {"plain": (ld, False), "strided": ((ld or C) + (4 if C % 4 == 0 else 3), False),
                                   "offset": (ld, True)}.items():
            for res in (False, True):
                out.append(Case(f"{R}x{C}-{layout}{'-res' if res else ''}-p{p}", R, C, ldv, off, res, 0, p, _path(R, C, ldv, off, 0)))
    # a strided layout whose stride is NOT a multiple of 4 under a C that is: falls to the scalar path
    out.append(Case("7x4-ld5", 7, 4, 5, False, True, 0, 0.5, "scalar"))
    for base in BASES[1:]:
        # 16 elements; 2^34 - 6 crosses into the counter's high word at its 7th element
        out.append(Case(f"2x8-base{base}", 2, 8, None, False, True, base, 0.5, _path(2, 8, None, False, base)))
    out.append(Case("2x8-base8", 2, 8, None, False, False, 8, 0.5, "vector"))
    out.append(Case("2x8-base2^34", 2, 8, None, False, False, 1 << 34, 0.5, "vector"))
    for p in PS:
        out.append(Case(f"33x77-p{p}", 33, 77, None, False, True, 0, p, "scalar"))
        out.append(Case(f"2x128-p{p}", 2, 128, None, False, True, 0, p, "vector"))
    out.append(Case("33x77-ptiny", 33, 77, None, False, True, 0, P_TINY, "scalar"))
    out.append(Case("2x128-ptiny", 2, 128, None, False, False, 0, P_TINY, "vector"))
    out.append(Case("big-vector", BIG[0], BIG[1], None, False, True, 0, 0.5, "vector"))
    out.append(Case("big-scalar", BIG[0], BIG[1], None, True, False, 0, 0.5, "scalar"))
    return out


CASES = _cases()
