"""An index-exact emulation of csrc/poly_filter.hip's slice and step schedule in numpy (the style of tests/evd_emulation.py): the same
slice width by N, grid and block shape, the same two LDS buffers per workgroup with the new iterate overwriting the one two steps back,
the same flat addresses into x / the stacks / y / dot_part (every access asserted in bounds, LDS included), the same ragged last slice,
and the dot products reduced thread -> wave (xor-shuffle tree) -> waves in order.  Arithmetic in float64, as the kernel's iterates are (it
rounds only what it stores to global memory), so the result can be held against the dense float64 polynomials: what this checks is the
schedule and the addressing, without a GPU.
"""
import numpy as np

MAX_THREADS, MAX_NODES, WAVE = 1024, 8192, 64


def slice_width_log2(N):
    return 2 if N <= MAX_NODES // 4 else (1 if N <= MAX_NODES // 2 else 0)


def launch_shape(N, d):
    """(workgroups, threads, LDS doubles) as launch_shape() in the .hip computes them."""
    csl = slice_width_log2(N)
    total = N << csl
    nt = min(-(-total // WAVE) * WAVE, MAX_THREADS)
    return -(-d // (1 << csl)), nt, 2 * total + MAX_THREADS // WAVE


class _Mem:
    """A flat array whose every access is bounds-checked (what the kernel would fault on)."""

    def __init__(self, a, name):
        self.a, self.name = a, name

    def _chk(self, idx):
        idx = np.asarray(idx)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < self.a.size), f"{self.name}: address out of bounds"
        return idx

    def rd(self, idx):
        return self.a[self._chk(idx)]

    def wr(self, idx, v):
        self.a[self._chk(idx)] = v


def _apply_s(rowptr, col, w, nnz, diag_add, scale, prev, N, csl, idx):
    """apply_s for the vector of elements idx: a row's entries in CSR order, columns outside [0, N) skipped, rowptr clamped."""
    cs = 1 << csl
    out = np.empty(idx.size, dtype=prev.a.dtype)
    for n, ix in enumerate(idx):
        i, ch = ix >> csl, ix & (cs - 1)
        e0 = min(max(int(rowptr[i]), 0), nnz)
        e1 = min(max(int(rowptr[i + 1]), e0), nnz)
        acc = prev.a.dtype.type(0)
        for e in range(e0, e1):
            j = int(col[e])
            if 0 <= j < N:
                acc = w[e] * prev.rd((j << csl) + ch) + acc
        out[n] = scale * acc + diag_add * prev.rd(ix)
    return out


def _block_sum(per_thread):
    """block_sum(): 64-lane xor-shuffle tree per wave, then the waves in order."""
    v = per_thread.reshape(-1, WAVE).copy()
    o = 32
    while o > 0:
        v = v + v[:, np.arange(WAVE) ^ o]
        o >>= 1
    t = per_thread.dtype.type(0)
    for wv in range(v.shape[0]):
        t = t + v[wv, 0]
    return t


def basis(x, rowptr, col, w, diag_add, scale, K, cheb, B=None, b_sk=0, b_ld=0, g=None, g_sk=0, g_ld=0, g_reverse=False, dtype=np.float64):
    """k_poly_basis over every workgroup.  x [N, d]; B / g flat arrays addressed as the kernel addresses them.  Returns dot_part
    [slices, K+1] (or None); B is written in place."""
    N, d = x.shape
    csl = slice_width_log2(N)
    cs, total = 1 << csl, N << csl
    nblk, nt, lds_floats = launch_shape(N, d)
    xm = _Mem(np.ascontiguousarray(x, dtype=dtype).reshape(-1), "x")
    Bm = None if B is None else _Mem(B, "B")
    gm = None if g is None else _Mem(g, "g")
    w = np.asarray(w, dtype=dtype)
    dot_part = None if g is None else np.zeros((nblk, K + 1), dtype=dtype)
    for blk in range(nblk):
        lds = np.zeros(lds_floats, dtype=dtype)
        assert 2 * total <= lds.size
        bufs = (_Mem(lds[:total], "lds buf0"), _Mem(lds[total:2 * total], "lds buf1"))
        c0 = blk << csl
        cw = min(cs, d - c0)
        for k in range(K + 1):
            cur, prev = bufs[k & 1], bufs[1 - (k & 1)]
            dots = np.zeros(nt, dtype=dtype)
            new = np.empty(total, dtype=dtype)
            for tid in range(min(nt, total)):
                idx = np.arange(tid, total, nt)
                i, ch = idx >> csl, idx & (cs - 1)
                ok = ch < cw
                if k == 0:
                    v = np.zeros(idx.size, dtype=dtype)
                    v[ok] = xm.rd(i[ok] * d + c0 + ch[ok])
                else:
                    v = _apply_s(rowptr, col, w, len(col), diag_add, scale, prev, N, csl, idx)
                    if cheb and k >= 2:
                        v = 2.0 * v - cur.rd(idx)
                new[idx] = v
                if Bm is not None:
                    Bm.wr(k * b_sk + i[ok] * b_ld + c0 + ch[ok], v[ok])
                if gm is not None:
                    kk = K - k if g_reverse else k
                    gv = gm.rd(kk * g_sk + i[ok] * g_ld + c0 + ch[ok])
                    acc = dtype(0)
                    for a, b in zip(v[ok], gv):            # the thread's elements in idx order
                        acc = a * b + acc
                    dots[tid] = acc
            # every thread wrote only its own elements of `cur` and read `prev` (and its own element of `cur`): apply after the step
            cur.wr(np.arange(total), new)
            if dot_part is not None:
                dot_part[blk, k] = _block_sum(dots)
    return dot_part


def combine(a, a_sk, a_ld, a_reverse, N, d, rowptr, col, w, diag_add, scale, K, cheb, c=None, dtype=np.float64):
    """k_poly_combine over every workgroup; `a` a flat array addressed as the kernel addresses it.  Returns y [N, d]."""
    csl = slice_width_log2(N)
    cs, total = 1 << csl, N << csl
    nblk, nt, lds_floats = launch_shape(N, d)
    am = _Mem(a, "a")
    w = np.asarray(w, dtype=dtype)
    y = _Mem(np.full(N * d, np.nan, dtype=dtype), "y")
    for blk in range(nblk):
        lds = np.full(lds_floats, np.nan, dtype=dtype)        # Horner never reads a buffer before writing it: NaN would show
        if cheb:
            lds[:2 * total] = 0.0
        bufs = (_Mem(lds[:total], "lds buf0"), _Mem(lds[total:2 * total], "lds buf1"))
        c0 = blk << csl
        cw = min(cs, d - c0)
        for k in range(K, -1, -1):
            cur, prev = bufs[(K - k) & 1], bufs[1 - ((K - k) & 1)]
            kk = K - k if a_reverse else k
            ck = dtype(1) if c is None else dtype(c[k])
            idx = np.arange(total)
            i, ch = idx >> csl, idx & (cs - 1)
            ok = ch < cw
            v = np.zeros(total, dtype=dtype)
            v[ok] = ck * am.rd(kk * a_sk + i[ok] * a_ld + c0 + ch[ok])
            if k < K:
                s = _apply_s(rowptr, col, w, len(col), diag_add, scale, prev, N, csl, idx)
                if not cheb:
                    v = v + s
                else:
                    v = v + (2.0 * s - cur.rd(idx) if k > 0 else s - cur.rd(idx))
            if k > 0:
                cur.wr(idx, v)
            else:
                y.wr(i[ok] * d + c0 + ch[ok], v[ok])
    assert not np.isnan(y.a).any(), "an element of y was never written"
    return y.a.reshape(N, d)
