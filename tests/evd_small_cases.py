"""The degenerate graphs of 1 .. 64 nodes the register Jacobi kernel (csrc/evd.hip, sn_laplacian_evd_f32) is checked on — shared by
tests/test_evd_small_gpu.py and tests/test_evd_small_cpu.py (dispatch coverage, float32 emulation of the method).  Each case:
(name, edge_index [2,E] int64 numpy with local node ids, n).  Every case runs under norm=None and norm='sym'.

The table puts a graph on each side of every row-count threshold of the kernel's dispatch (8|9, 16|17, 24|25, 32|33, 40|41, 48|49,
56|57, 64), the upper side always an odd n (a padding column: m = n + 1), and covers what the molecule generator never produces:
null spaces of dimension 2 .. 64 (components, isolated nodes, no edges at all) and eigenvalues of multiplicity up to 63 (K_n, stars,
K_{a,b}, cycles, hypercubes, grids)."""
import numpy as np

from evd_large_cases import collate  # noqa: F401  (re-exported: the sharing batches below are collated with it)

NORMS = (None, "sym")
WAVES = 4                 # EVD_WV of evd.hip


def _arr(pairs):
    return np.array(pairs, dtype=np.int64).reshape(-1, 2).T.copy()


def empty(n):
    return np.zeros((2, 0), np.int64)


def path(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)]).astype(np.int64)


def cycle(n):
    return np.concatenate([path(n), [[n - 1], [0]]], 1).astype(np.int64)


def star(n):
    return np.stack([np.zeros(n - 1, np.int64), np.arange(1, n)]).astype(np.int64)


def complete(n):
    return np.stack(np.triu_indices(n, 1)).astype(np.int64)


def bipartite(a, b):
    return _arr([(i, a + j) for i in range(a) for j in range(b)])


def cube(d):
    return _arr([(v, v | (1 << b)) for v in range(1 << d) for b in range(d) if not v & (1 << b)])


def grid(r, c):
    e = []
    for y in range(r):
        for x in range(c):
            if x + 1 < c:
                e.append((y * c + x, y * c + x + 1))
            if y + 1 < r:
                e.append((y * c + x, (y + 1) * c + x))
    return _arr(e)


def cases():
    p64 = path(64)
    return [
        ("single1", empty(1), 1),
        ("edge2", path(2), 2),
        ("empty5", empty(5), 5),                                         # amax = 0: L = 0 (None), L = I (sym)
        ("path3", path(3), 3),
        ("tri_tri_iso7", np.concatenate([cycle(3), cycle(3) + 3], 1), 7),  # two triangles and node 6 alone: three zero eigenvalues
        ("K8", complete(8), 8),
        ("cycle9", cycle(9), 9),
        ("star16", star(16), 16),
        ("K16", complete(16), 16),
        ("K17", complete(17), 17),
        ("cycle24", cycle(24), 24),
        ("star25", star(25), 25),
        ("K32", complete(32), 32),
        ("cube5", cube(5), 32),                                           # multiplicities 1, 5, 10, 10, 5, 1
        ("K33", complete(33), 33),
        ("star40", star(40), 40),
        ("cycle41", cycle(41), 41),
        ("grid6x8", grid(6, 8), 48),
        ("star49", star(49), 49),
        ("K16_16_plus_24_isolated", bipartite(16, 16), 56),               # null space of dimension 25 (None)
        ("cycle57", cycle(57), 57),
        ("path63", path(63), 63),
        ("K64", complete(64), 64),                                        # eigenvalue 64 (None) of multiplicity 63
        ("star64", star(64), 64),
        ("cycle64", cycle(64), 64),
        ("cube6", cube(6), 64),
        ("grid8x8", grid(8, 8), 64),
        ("K32_32", bipartite(32, 32), 64),
        ("two_paths_30_34", np.concatenate([p64[:, :29], p64[:, 30:]], 1), 64),   # two-dimensional null space
        ("path40_plus_24_isolated", p64[:, :39], 64),
        ("empty64", empty(64), 64),
    ]


CASE_NAMES = ["single1", "edge2", "empty5", "path3", "tri_tri_iso7", "K8", "cycle9", "star16", "K16", "K17", "cycle24", "star25", "K32",
              "cube5", "K33", "star40", "cycle41", "grid6x8", "star49", "K16_16_plus_24_isolated", "cycle57", "path63", "K64", "star64",
              "cycle64", "cube6", "grid8x8", "K32_32", "two_paths_30_34", "path40_plus_24_isolated", "empty64"]


def case(name):
    """(edge_index, n) of a case of the table."""
    return next((e, n) for nm, e, n in cases() if nm == name)


# ---- the dispatch of evd.hip, restated
# k_evd_prep:    n <= 16 -> class 16 (four graphs per workgroup), n <= 32 -> class 32 (two), n <= 64 -> class 64 (one); n = 0 is not listed.
# evd_jacobi:    nmax = the workgroup's largest n rounded up to even, rows = ceil(nmax / 4) live rows per wave, RMAX = NR / 4;
#                rows > 14 -> RW 16, > 12 -> 14, > 10 -> 12, > 8 -> 10   (RMAX >= 16: class 64 only)
#                rows > 6 -> RW 8, > 4 -> 6                               (RMAX >= 8:  classes 32 and 64)
#                rows > 2 -> RW 4                                         (RMAX >= 4:  every class)
#                otherwise RW 2.
# So: class 16 -> RW 2 (n <= 8), 4 (9 .. 16); class 32 -> RW 6 (17 .. 24), 8 (25 .. 32); class 64 -> RW 10 (33 .. 40), 12 (41 .. 48),
# 14 (49 .. 56), 16 (57 .. 64).
def size_class(n):
    assert 1 <= n <= 64, n
    return 16 if n <= 16 else (32 if n <= 32 else 64)


def rows_per_wave(nmax):
    """RW of the evd_jacobi_rows<NR, 4, RW> a workgroup runs whose largest graph has nmax nodes."""
    rmax = size_class(nmax) // WAVES
    rows = (((nmax + 1) & ~1) + WAVES - 1) // WAVES
    if rmax >= 16:
        for bound, rw in ((14, 16), (12, 14), (10, 12), (8, 10)):
            if rows > bound:
                return rw
    if rmax >= 8:
        for bound, rw in ((6, 8), (4, 6)):
            if rows > bound:
                return rw
    if rmax >= 4 and rows > 2:
        return 4
    return 2


def instantiation(sizes):
    """(NR, RW) of the ONE workgroup the graphs of these sizes share (they must be of one class and fit one workgroup)."""
    cls = {size_class(n) for n in sizes}
    assert len(cls) == 1 and len(sizes) <= 64 // min(cls), sizes
    return min(cls), rows_per_wave(max(sizes))


INSTANTIATIONS = [(16, 2), (16, 4), (32, 6), (32, 8), (64, 10), (64, 12), (64, 14), (64, 16)]
LOWER_BOUND = {(16, 2): 1, (16, 4): 9, (32, 6): 17, (32, 8): 25, (64, 10): 33, (64, 12): 41, (64, 14): 49, (64, 16): 57}


# ---- batches whose workgroup composition is certain whatever order k_evd_prep's LDS counter lists the graphs in: at most four class-16
# and at most two class-32 graphs per batch, so each class fills exactly one workgroup (a class-64 graph has its own anyway).
# name -> (case names, {class: (NR, RW) of that class's workgroup})
SHARING = {
    "four_m_one_workgroup": (["single1", "edge2", "cycle9", "K16"], {16: (16, 4)}),            # m = 2, 2, 10, 16: RW 4 because of the largest
    "dead_fourth_slot": (["path3", "K8", "empty5"], {16: (16, 2)}),
    "m18_beside_m32": (["K17", "K32"], {32: (32, 8)}),
    "half_the_lanes_dead": (["star25"], {32: (32, 8)}),
    # an EVEN m below mmax: the graph's last column is a real one, so a step it must sit out (step >= m - 1) would rotate real data — with
    # an odd n (K17 above) the column that such a step pairs up is the zero padding column, which never rotates
    "m24_beside_m32": (["cycle24", "K32"], {32: (32, 8)}),
    "m8_beside_m16": (["K8", "path3", "star16"], {16: (16, 4)}),
    "three_classes": (["K64", "K17", "cycle24", "edge2", "cycle9", "star16", "tri_tri_iso7", "cycle41"],
                      {16: (16, 4), 32: (32, 6), 64: None}),                                   # K64 and cycle41: a workgroup each, (64, 16) and (64, 12)
}


def sharing_batch(name):
    """(edge_index with batch-wide ids, sizes, case names) of a forced-sharing batch."""
    names = SHARING[name][0]
    ei, sizes = collate([case(nm) for nm in names])
    return ei, sizes, names
