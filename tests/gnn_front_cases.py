"""Batches for the GINE stage's front record tests: the smallest graphs that reach every branch of the front workgroup and of the
stage kernel's record prologue — 1, 16, 17 and 64 nodes (row-tile counts 1, 1, 2, 4), nodes with 0, exactly 4 and 9 in-edges, a graph
with exactly 192 in-edges, two bond types present out of the table's values — and the two batches a record cannot describe (a
65-node graph, an atom id outside its table)."""
import types

import numpy as np
import torch

from signnet_basisnet_amd import synth


def _sym(und):
    und = sorted(set((min(a, b), max(a, b)) for a, b in und if a != b))
    src = [a for a, b in und] + [b for a, b in und]
    dst = [b for a, b in und] + [a for a, b in und]
    ei = np.array([src, dst], dtype=np.int64).reshape(2, -1)
    return ei[:, np.lexsort((ei[1], ei[0]))]


def g_single():
    return 1, np.zeros((2, 0), dtype=np.int64)


def g_star16():
    """16 nodes: node 0 has 9 in-edges, node 10 exactly 4, node 15 none."""
    und = [(0, j) for j in range(1, 10)] + [(10, j) for j in range(11, 15)]
    return 16, _sym(und)


def g_tree(n, chords, seed):
    rng = np.random.default_rng(seed)
    und = set((int(rng.integers(0, i)), i) for i in range(1, n))
    while len(und) < n - 1 + chords:
        a, b = (int(v) for v in rng.integers(0, n, size=2))
        if a != b:
            und.add((min(a, b), max(a, b)))
    return n, _sym(und)


def collate(graphs, seed=0, bonds=(1, 3)):
    eis, evals, evecs, batch, sizes = [], [], [], [], []
    off = 0
    for b, (n, ei) in enumerate(graphs):
        D, V = synth.sym_laplacian_eigh(ei, n)
        eis.append(ei + off)
        evals.append(D)
        evecs.append(V.reshape(-1))
        batch.append(np.full(n, b, dtype=np.int64))
        sizes.append(n)
        off += n
    edge_index = torch.from_numpy(np.ascontiguousarray(np.concatenate(eis, axis=1)))
    g = torch.Generator().manual_seed(seed)
    E = edge_index.shape[1]
    data = types.SimpleNamespace(
        x=torch.randint(0, 28, (off, 1), generator=g, dtype=torch.long),
        edge_index=edge_index,
        edge_attr=torch.tensor(bonds, dtype=torch.long)[torch.randint(0, len(bonds), (E,), generator=g)] if E else torch.zeros(0, dtype=torch.long),
        batch=torch.from_numpy(np.concatenate(batch)), eigen_values=torch.cat(evals), eigen_vectors=torch.cat(evecs),
        num_graphs=len(graphs), num_nodes=off)
    data.sizes = sizes
    return data


def batch_one():
    return collate([g_single()], seed=1)


def batch_three():
    """16 nodes | 17 nodes | 64 nodes with 96 undirected edges = 192 in-edges."""
    return collate([g_star16(), g_tree(17, 2, 5), g_tree(64, 33, 6)], seed=2)


def batch_oversize():
    return collate([g_star16(), g_tree(65, 3, 7), g_tree(17, 2, 5)], seed=3)


def batch_bad_atom():
    d = collate([g_star16(), g_tree(17, 2, 5)], seed=4)
    d.x[3, 0] = 1000          # outside the 500-row table: nn.Embedding raises IndexError
    return d


def batch_wide_bond():
    """Bond ids inside the table but past the 32-value class mask: served by the stage kernel's own prologue, not by records."""
    return collate([g_star16(), g_tree(17, 2, 5), g_tree(40, 4, 8)], seed=5, bonds=(1, 40))
