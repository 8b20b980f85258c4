"""What tests/test_store_cpu.py and tests/test_store_gpu.py share: the pool of graphs, its per-graph samples and the HOST collate the
store's gather is compared with — written out here: torch.cat with node offsets, in index order (what the reference's DataLoader
does per batch)."""
import types

import torch

SIZES = [1, 2, 9, 37, 64, 16, 5, 33, 1, 12]
ZERO_EDGE = len(SIZES)                 # index of the zero-edge graph added by hand
G = len(SIZES) + 1


def pool(features):
    """-> (samples, y): SIZES from synth.make_batch, cut with dist.slice_graphs, plus a 3-node graph without edges; y [G, 2]."""
    from signnet_basisnet_amd import dist, synth
    batch = synth.make_batch(len(SIZES), seed=11, features=features, sizes=SIZES)
    samples = [dist.slice_graphs(batch, i, i + 1) for i in range(len(SIZES))]
    n = 3
    D, V = synth.sym_laplacian_eigh(torch.zeros(2, 0, dtype=torch.long).numpy(), n)
    samples.append(types.SimpleNamespace(
        x=batch.x[:n].clone(), edge_index=torch.zeros(2, 0, dtype=torch.long),
        edge_attr=batch.edge_attr[:0].clone(), batch=torch.zeros(n, dtype=torch.long), eigen_values=D, eigen_vectors=V.reshape(-1),
        num_graphs=1, num_nodes=n, sizes=[n]))
    y = torch.randn(G, 2, generator=torch.Generator().manual_seed(5))
    return samples, y


def host_collate(samples, idx, y=None):
    """The host collate of samples[i] for i in idx, in index order."""
    sel = [samples[i] for i in idx]
    off, eis, batch = 0, [], []
    for b, s in enumerate(sel):
        eis.append(s.edge_index + off)
        batch.append(torch.full((s.x.shape[0],), b, dtype=torch.long))
        off += s.x.shape[0]
    out = types.SimpleNamespace(
        x=torch.cat([s.x for s in sel]), edge_index=torch.cat(eis, 1).contiguous(), edge_attr=torch.cat([s.edge_attr for s in sel]),
        batch=torch.cat(batch), eigen_values=torch.cat([s.eigen_values for s in sel]),
        eigen_vectors=torch.cat([s.eigen_vectors for s in sel]), num_graphs=len(sel), num_nodes=off)
    out.sizes = [int(s.x.shape[0]) for s in sel]
    if y is not None:
        out.y = y[torch.as_tensor(list(idx), dtype=torch.long)]
    return out


def dgl_samples(samples, y, K, with_e=True, with_snorm=True):
    """The same pool in the DGL layout: per-graph (Graph, h [n], pos_enc [n, K], e [E] or None, snorm_n [n, 1] or None, target [1])."""
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    out = []
    for i, s in enumerate(samples):
        n = int(s.x.shape[0])
        out.append((Graph(s.edge_index[0], s.edge_index[1], [n]), s.x.reshape(-1).long(), synth.dgl_pos_enc(s, K),
                    s.edge_attr.reshape(-1).long() if with_e else None,
                    torch.full((n, 1), 1.0 / n).sqrt() if with_snorm else None, y[i, :1]))
    return out


def dgl_host_collate(dsamples, idx):
    """-> (Graph, h, p, e, snorm_n, targets [B, 1]) of dsamples[i] for i in idx, in index order."""
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    sel = [dsamples[i] for i in idx]
    off, src, dst = 0, [], []
    for g, h, *_ in sel:
        s, d = g.edges()
        src.append(s + off)
        dst.append(d + off)
        off += h.shape[0]
    cat = lambda i: None if sel[0][i] is None else torch.cat([s[i] for s in sel])
    g = Graph(torch.cat(src), torch.cat(dst), [int(s[1].shape[0]) for s in sel], [int(s[0].edges()[0].numel()) for s in sel])
    return g, cat(1), cat(2), cat(3), cat(4), torch.cat([s[5] for s in sel]).reshape(-1, 1)
