"""The graphs of 65 .. 128 nodes the mid-size Jacobi kernel (csrc/evd_large.hip) is checked on — shared by tests/test_evd_large_gpu.py,
tests/test_evd_large_cpu.py (float32 emulation of the method) and profiles/scripts/evd_large.py.  Each case: (name, edge_index [2,E]
int64 numpy with local node ids, n)."""
import numpy as np


def _path(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)]).astype(np.int64)


def molecule(n):
    from signnet_basisnet_amd import synth
    return synth.make_batch(1, seed=100 + n, sizes=[n]).edge_index.numpy().astype(np.int64)


def cases():
    out = [(f"molecule{n}", molecule(n), n) for n in (65, 70, 96, 127, 128)]
    n = 128
    path = _path(n)
    out.append(("path128", path, n))
    out.append(("cycle128", np.concatenate([path, [[n - 1], [0]]], 1), n))                 # every eigenvalue but two is double
    out.append(("star128", np.stack([np.zeros(n - 1, np.int64), np.arange(1, n)]), n))     # eigenvalue 1 of multiplicity 126
    out.append(("K80", np.stack(np.triu_indices(80, 1)).astype(np.int64), 80))
    r, c = 8, 16
    e = []
    for y in range(r):
        for x in range(c):
            if x + 1 < c:
                e.append((y * c + x, y * c + x + 1))
            if y + 1 < r:
                e.append((y * c + x, (y + 1) * c + x))
    out.append(("grid8x16", np.array(e, dtype=np.int64).T, 128))
    out.append(("two_paths_60_68", np.concatenate([path[:, :59], path[:, 60:]], 1), n))    # two-dimensional null space
    out.append(("path101_plus_27_isolated", path[:, :100], n))
    return out


CASE_NAMES = ["molecule65", "molecule70", "molecule96", "molecule127", "molecule128", "path128", "cycle128", "star128", "K80",
              "grid8x16", "two_paths_60_68", "path101_plus_27_isolated"]


def collate(graphs):
    """[(edge_index, n), ...] -> (edge_index [2,E] int64 numpy with batch-wide node ids, sizes)."""
    eis, sizes, off = [], [], 0
    for ei, n in graphs:
        eis.append(np.asarray(ei, dtype=np.int64).reshape(2, -1) + off)
        sizes.append(int(n))
        off += n
    return np.ascontiguousarray(np.concatenate(eis, 1)), sizes
