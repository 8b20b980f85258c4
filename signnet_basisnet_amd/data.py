"""Device-resident graph stores: a whole dataset lives on the GPU and a training batch is gathered out of it in ONE launch.

The reference's loops take each batch from a DataLoader (GINESignNetPyG/core/train.py:55-66, Alchemy/main_alchemy.py:99-110,
GraphPrediction/train/train_ZINC_graph_regression.py:54-88): a per-sample Python collate — seven tensors concatenated, edge ids
re-based, the eigenvector blocks laid end to end — and seven host-to-device copies per step.  The molecule sets fit on the device many
times over (ZINC-full with all eigenvectors: ~0.5 GB), so here the selection, offsetting and padding of a batch is sn_store_gather
(csrc/collate.hip): from B graph indices on the device straight into the capacity buffers the captured step reads.

    store = GraphStore.from_samples(samples, "cuda")            # or from_batch(collated, y, "cuda");  DGLGraphStore likewise
    loader = IndexLoader(store.num_graphs, 128, shuffle=True, seed=0)
    step = BucketedStep(model, flat_adam, max_graphs=128)
    every = [loader.permutation(e)[i:i + 128] for e in range(epochs) for i in range(0, store.num_graphs, 128)]
    bucket = store.covering_bucket(every, step.granule, model.max_k)                        # one capture for the whole run
    for epoch in range(epochs):
        loader.epoch(epoch)                                     # ONE upload of the permutation
        for idx in loader:                                      # (host indices, device view of the permutation)
            loss = step.step_from(store, idx, bucket=bucket)
    model.eval(); y = model(store.collate(test_idx))            # exact-size batch, no padding

Per step the host adds up B integers from its own copies of the size tables; it reads nothing from the device and copies nothing to it.
"""
from __future__ import annotations

import types

import numpy as np
import torch

from . import ops
from ._lib import require_cuda

_PYG_GRANULE = dict(N=64, E=128, S=4096, K=8)          # the defaults of train_graph.BucketedStep
_DGL_GRANULE = dict(N=256, E=512)                      # the defaults of train_graph.DGLBucketedStep


def _round_up(v, g):
    g = max(int(g), 1)
    return -(-int(v) // g) * g


def _device(device):
    """The store's device, or the package's 'GPU only' error."""
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        require_cuda(torch.empty(0))                   # raises: signnet_basisnet_amd ops run on the GPU only
    return dev


def _host_index(idx):
    return np.ascontiguousarray(np.asarray(idx.cpu() if torch.is_tensor(idx) else idx, dtype=np.int64).reshape(-1))


def _ptr(counts):
    out = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=out[1:])
    return out


class GraphSizes:
    """The host half of a store: per-graph node and edge counts (numpy int64) and the offset tables built from them.  Everything the
    training loop decides per step — totals, the capacity bucket — comes from here, without a device."""

    dgl = False

    def __init__(self, n_nodes, n_edges, dgl=False):
        self.n_nodes = np.ascontiguousarray(np.asarray(n_nodes, dtype=np.int64).reshape(-1))
        self.n_edges = np.ascontiguousarray(np.asarray(n_edges, dtype=np.int64).reshape(-1))
        if self.n_nodes.shape != self.n_edges.shape or (self.n_nodes < 0).any() or (self.n_edges < 0).any():
            raise ValueError("GraphSizes: one non-negative node count and edge count per graph")
        self.dgl = bool(dgl)
        self.num_graphs = int(self.n_nodes.size)
        self.node_ptr, self.edge_ptr = _ptr(self.n_nodes), _ptr(self.n_edges)
        self.eig_ptr = None if self.dgl else _ptr(self.n_nodes * self.n_nodes)

    # ---- constructors (host only)
    @classmethod
    def from_samples(cls, samples, dgl=False):
        if dgl:
            return cls([int(s[1].shape[0]) for s in samples], [int(s[0].edges()[0].numel()) for s in samples], dgl=True)
        return cls([int(s.x.shape[0]) for s in samples],
                   [int(s.edge_index.shape[1]) if s.edge_index.numel() else 0 for s in samples])

    @classmethod
    def from_batch(cls, batch, dgl=False):
        if dgl:
            g = batch[0]
            n = _host_index(torch.as_tensor(g.batch_num_nodes()))
            bne = getattr(g, "batch_num_edges", lambda: None)()
            e = _host_index(torch.as_tensor(bne)) if bne is not None else _edge_counts(g.edges()[0], n)
            return cls(n, e, dgl=True)
        B = int(batch.num_graphs)
        n = np.asarray(batch.sizes, dtype=np.int64) if hasattr(batch, "sizes") else torch.bincount(batch.batch, minlength=B).cpu().numpy()
        ei = batch.edge_index
        return cls(n, _edge_counts(ei[0] if ei.numel() else ei.new_zeros(0), n))

    # ---- per step
    def totals(self, idx):
        """(N, E, S, largest graph) of the graphs `idx` (host indices); an index outside [0, num_graphs) counts as an empty graph,
        as on the device."""
        idx = _host_index(idx)
        if idx.size and (int(idx.min()) < 0 or int(idx.max()) >= self.num_graphs):
            idx = idx[(idx >= 0) & (idx < self.num_graphs)]
        n = self.n_nodes[idx]
        return (int(n.sum()), int(self.n_edges[idx].sum()), 0 if self.dgl else int((n * n).sum()), int(n.max()) if n.size else 0)

    def bucket_of(self, idx, granule=None, max_k=None, _totals=None):
        """The capacity bucket of the batch `idx`: the rounding of BucketedStep.bucket_of (a Bucket) or, for a DGL store, of
        DGLBucketedStep.bucket_of (a DGLBucket).  Host only."""
        from .train_graph import Bucket, DGLBucket
        N, E, S, nmax = _totals or self.totals(idx)
        g = dict(_DGL_GRANULE if self.dgl else _PYG_GRANULE)
        g.update(granule or {})
        if self.dgl:
            return DGLBucket(_round_up(N + 1, g["N"]), _round_up(max(E, 1), g["E"]))
        K = int(max_k) if max_k else _round_up(max(nmax, 1), g["K"])
        return Bucket(_round_up(N + 1, g["N"]), _round_up(max(E, 1), g["E"]), _round_up(max(S, 1), g["S"]), K)

    def covering_bucket(self, batches, granule=None, max_k=None):
        """The ONE bucket that holds every batch of `batches` (an epoch's index lists; an IndexLoader's host indices): the
        component-wise maximum of their buckets.  With it one capture serves a whole run — a real shuffle otherwise produces more
        distinct buckets than the captures the LRU keeps."""
        bs = [self.bucket_of(b[0] if isinstance(b, tuple) else b, granule, max_k) for b in batches]
        if not bs:
            raise ValueError("covering_bucket: no batches")
        return type(bs[0])(*(max(c) for c in zip(*bs)))


def _edge_counts(src, n_nodes):
    """Edges per graph of a collated edge list (global source ids): the edges of a graph are contiguous and in graph order."""
    G = len(n_nodes)
    src = torch.as_tensor(src).cpu().long()
    ptr = torch.from_numpy(_ptr(n_nodes))
    graph = torch.bucketize(src, ptr[1:], right=True)
    if src.numel() and (int(src.min()) < 0 or int(graph.max()) >= G or bool((graph[1:] < graph[:-1]).any())):
        raise ValueError("the edges of a collated batch must be grouped by graph, in graph order, with endpoints inside the batch")
    return torch.bincount(graph, minlength=G).numpy()


def _resolve(idx, dev):
    """-> (host indices, device indices): an (host, device view) pair of an IndexLoader as it is, host indices uploaded."""
    if isinstance(idx, tuple) and len(idx) == 2 and torch.is_tensor(idx[1]) and idx[1].is_cuda:
        return _host_index(idx[0]), idx[1]
    if isinstance(idx, tuple) and len(idx) == 2 and idx[1] is None:
        idx = idx[0]
    if torch.is_tensor(idx) and idx.is_cuda:
        raise TypeError("a store takes host indices or an IndexLoader's (host indices, device view) pair: the host sizes its "
                        "batches without reading the device")
    h = _host_index(idx)
    return h, torch.from_numpy(h).to(dev)


class _Store(GraphSizes):
    """What GraphStore and DGLGraphStore share: the device tables, the cached parameter block per destination, collate / gather_into."""

    def _init_tables(self, dev):
        self.device = dev
        self.d_node_ptr, self.d_edge_ptr = (torch.from_numpy(p).to(dev) for p in (self.node_ptr, self.edge_ptr))
        self.d_eig_ptr = None if self.eig_ptr is None else torch.from_numpy(self.eig_ptr).to(dev)

    def tables(self):
        return self.d_node_ptr, self.d_edge_ptr, self.d_eig_ptr

    def _args(self, out, exact=False):
        cached = getattr(out, "_gather_args", None)
        if cached is None or cached[0] is not self:
            out.gather_status = torch.zeros(4, dtype=torch.int32, device=self.device)
            a = ops.store_gather_args(self.tables(), self.num_graphs, (out.N_cap, out.E_cap, out.B_cap, getattr(out, "S_cap", 0)),
                                      self.segments(out), out.gather_status, getattr(out, "counts", None),
                                      getattr(out, "count_error", None), exact)
            cached = out._gather_args = (self, a)
        return cached[1]

    def gather_into(self, idx, pad, _totals=None):
        """Fill the capacity buffers `pad` (train_graph.PaddedBatch / DGLPaddedBatch) with the graphs `idx`, in index order, in ONE
        launch: what ops.bucket_pack / bucket_pack_dgl writes for the host-collated batch, byte for byte.  The host computes N, E, S from
        its size arrays and raises ValueError before any launch if the batch does not fit; an index out of range becomes an empty graph
        and sets pad.gather_status[0] & 1 (the step's check() raises IndexError).  -> (N, E, B, S)."""
        hidx, didx = _resolve(idx, self.device)
        N, E, S, _ = _totals or self.totals(hidx)
        B = int(hidx.size)
        if N >= pad.N_cap or E > pad.E_cap or B >= pad.B_cap or S > getattr(pad, "S_cap", 0):
            raise ValueError(f"gather_into: batch (N {N}, E {E}, B {B}, S {S}) does not fit the bucket (N_cap {pad.N_cap} > N, E_cap "
                             f"{pad.E_cap}, B_cap {pad.B_cap} > B, S_cap {getattr(pad, 'S_cap', 0)})")
        ops.store_gather(self._args(pad), didx, B, (N, E, S))
        return N, E, B, S

    def _exact(self, idx, out):
        """The exact-size gather of collate(): indices are checked on the host (IndexError at once: nothing is deferred in eval)."""
        hidx, didx = _resolve(idx, self.device)
        if hidx.size and (int(hidx.min()) < 0 or int(hidx.max()) >= self.num_graphs):
            raise IndexError(ops.STORE_INDEX_ERROR)
        N, E, S, _ = self.totals(hidx)
        B = int(hidx.size)
        o = out(N, E, B, S)
        o.N_cap, o.E_cap, o.B_cap, o.S_cap = N, E, B, S
        ops.store_gather(self._args(o, exact=True), didx, B, (N, E, S))
        return hidx, o


class GraphStore(_Store):
    """The PyG layout on the device: x [N, ...], edge_index [2, E] with graph-LOCAL node ids, edge_attr [E, ...], eigen_values [N],
    eigen_vectors [sum n^2], y [G, n_out] (float32), and the int64 offset tables node_ptr / edge_ptr / eig_ptr [G + 1]."""

    def __init__(self, sizes, x, edge_index, edge_attr, eigen_values, eigen_vectors, y, device):
        dev = _device(device)
        GraphSizes.__init__(self, sizes.n_nodes, sizes.n_edges)
        N, E, S = int(self.node_ptr[-1]), int(self.edge_ptr[-1]), int(self.eig_ptr[-1])
        if x.shape[0] != N or eigen_values.numel() != N or edge_attr.shape[0] != E or eigen_vectors.numel() != S or \
                tuple(edge_index.shape) != (2, E):
            raise ValueError(f"GraphStore: arrays do not match the size tables (N {N}, E {E}, S {S})")
        self.x, self.edge_attr = x.to(dev).contiguous(), edge_attr.to(dev).contiguous()
        self.edge_index = edge_index.to(dev).long().contiguous()
        self.eigen_values = eigen_values.to(dev).float().contiguous()
        self.eigen_vectors = eigen_vectors.to(dev).float().reshape(-1).contiguous()
        self.y = None if y is None else torch.as_tensor(y).to(dev).float().reshape(self.num_graphs, -1).contiguous()
        self._init_tables(dev)

    @classmethod
    def from_samples(cls, samples, device, y=None):
        """`samples`: per-graph objects with x, edge_index (local ids), edge_attr, eigen_values, eigen_vectors and — unless `y` [G, ...]
        is given — y."""
        _device(device)
        sizes = GraphSizes.from_samples(samples)
        cat = lambda f, d=0: torch.cat([getattr(s, f) for s in samples], d)
        ei = torch.cat([s.edge_index.reshape(2, -1) for s in samples], 1)
        if y is None and all(hasattr(s, "y") for s in samples):
            y = torch.stack([torch.as_tensor(s.y).reshape(-1) for s in samples])
        return cls(sizes, cat("x"), ei, cat("edge_attr"), cat("eigen_values"), torch.cat([s.eigen_vectors.reshape(-1) for s in samples]),
                   y, device)

    @classmethod
    def from_batch(cls, batch, y, device):
        """`batch`: a collated batch in the layout of SURVEY §8(b) (edge ids batch-global); sizes from batch.sizes, else bincount."""
        _device(device)
        sizes = GraphSizes.from_batch(batch)
        ei = batch.edge_index.reshape(2, -1).long()
        first = torch.from_numpy(np.repeat(sizes.node_ptr[:-1], sizes.n_edges)).to(ei.device)
        return cls(sizes, batch.x, ei - first, batch.edge_attr, batch.eigen_values, batch.eigen_vectors, y, device)

    def proto(self):
        """(data, target) prototypes a new capture sizes its buffers from: dtypes and row shapes, no rows."""
        if self.y is None:
            raise ValueError("GraphStore: a training step needs targets (the store was built without y)")
        return types.SimpleNamespace(x=self.x[:0], edge_attr=self.edge_attr[:0], batch=self.d_node_ptr[:0], num_graphs=1), self.y[:1]

    def segments(self, out):
        S = ops
        segs = [(self.x, out.x, S.STORE_NODE, S.GATHER_COPY, 0),
                (self.edge_index[0], out.edge_index[0], S.STORE_EDGE, S.GATHER_ENDPOINT, 0),
                (self.edge_index[1], out.edge_index[1], S.STORE_EDGE, S.GATHER_ENDPOINT, 0),
                (self.edge_attr, out.edge_attr, S.STORE_EDGE, S.GATHER_COPY, 0),
                (None, out.batch, S.STORE_NODE, S.GATHER_GRAPH_ID, 0),
                (self.eigen_values, out.eigen_values, S.STORE_NODE, S.GATHER_COPY, 0),
                (self.eigen_vectors, out.eigen_vectors, S.STORE_EIG, S.GATHER_COPY, 0)]
        if getattr(out, "target", None) is not None:
            if self.y is None:
                raise ValueError("GraphStore: the destination has a target buffer, the store was built without y")
            segs.append((self.y, out.target, S.STORE_GRAPH, S.GATHER_COPY, 0))
        for name, kind in (("node_valid", S.STORE_NODE), ("edge_valid", S.STORE_EDGE), ("graph_valid", S.STORE_GRAPH)):
            if getattr(out, name, None) is not None:
                segs.append((None, getattr(out, name), kind, S.GATHER_CONST, 1))
        return segs

    def collate(self, idx):
        """The exact-size batch of the graphs `idx` for model(data) in eval mode: a namespace with the §8(b) fields, num_graphs,
        num_nodes, sizes (host) and y.  ONE launch, no padding, no spare graph."""
        dev = self.device

        def out(N, E, B, S):
            e = lambda like, n: torch.empty((n,) + tuple(like.shape[1:]), dtype=like.dtype, device=dev)
            return types.SimpleNamespace(
                x=e(self.x, N), edge_index=torch.empty(2, E, dtype=torch.int64, device=dev), edge_attr=e(self.edge_attr, E),
                batch=torch.empty(N, dtype=torch.int64, device=dev), eigen_values=torch.empty(N, dtype=torch.float32, device=dev),
                eigen_vectors=torch.empty(S, dtype=torch.float32, device=dev), target=None if self.y is None else e(self.y, B))
        hidx, o = self._exact(idx, out)
        return types.SimpleNamespace(x=o.x, edge_index=o.edge_index, edge_attr=o.edge_attr, batch=o.batch, eigen_values=o.eigen_values,
                                     eigen_vectors=o.eigen_vectors, num_graphs=o.B_cap, num_nodes=o.N_cap,
                                     sizes=self.n_nodes[hidx].tolist(), y=o.target)


class DGLGraphStore(_Store):
    """The DGL layout on the device: src / dst [E] with graph-LOCAL node ids, atom ids h [N], bond ids e [E] or None, pos_enc p [N, K],
    snorm_n [N] or None, target [G], and the int64 offset tables node_ptr / edge_ptr [G + 1]."""

    def __init__(self, sizes, src, dst, h, e, p, snorm_n, target, device):
        dev = _device(device)
        GraphSizes.__init__(self, sizes.n_nodes, sizes.n_edges, dgl=True)
        N, E = int(self.node_ptr[-1]), int(self.edge_ptr[-1])
        if h.numel() != N or p.shape[0] != N or p.dim() != 2 or src.numel() != E or dst.numel() != E or \
                (e is not None and e.numel() != E) or (snorm_n is not None and snorm_n.numel() != N):
            raise ValueError(f"DGLGraphStore: arrays do not match the size tables (N {N}, E {E})")
        i64 = lambda t: None if t is None else t.to(dev).long().reshape(-1).contiguous()
        self.src, self.dst, self.h, self.e = i64(src), i64(dst), i64(h), i64(e)
        self.p = p.to(dev).float().contiguous()
        self.K = int(p.shape[1])
        self.snorm_n = None if snorm_n is None else snorm_n.to(dev).float().reshape(-1).contiguous()
        self.target = None if target is None else torch.as_tensor(target).to(dev).float().reshape(-1).contiguous()
        if self.target is not None and self.target.numel() != self.num_graphs:
            raise ValueError("DGLGraphStore: one float32 score per graph")
        self._init_tables(dev)

    @staticmethod
    def _refuse_full_graph(g):
        ed = getattr(g, "edata", None)
        try:
            flagged = ed is not None and "real" in ed
        except TypeError:
            flagged = False
        if flagged:
            raise NotImplementedError("DGLGraphStore does not carry the edge flag edata['real'] of a full graph (TransformerNet with "
                                      "full_graph=True) through its gather: collate such batches with ops.make_full_graph")

    @classmethod
    def from_samples(cls, samples, device):
        """`samples`: per-graph tuples (g, h, p, e or None, snorm_n or None, target) — g's edges carry local node ids."""
        for s in samples:
            cls._refuse_full_graph(s[0])
        _device(device)
        sizes = GraphSizes.from_samples(samples, dgl=True)
        flat = lambda i: None if samples[0][i] is None else torch.cat([torch.as_tensor(s[i]).reshape(-1) for s in samples])
        src = torch.cat([s[0].edges()[0].reshape(-1) for s in samples])
        dst = torch.cat([s[0].edges()[1].reshape(-1) for s in samples])
        return cls(sizes, src, dst, flat(1), flat(3), torch.cat([s[2] for s in samples]), flat(4), flat(5), device)

    @classmethod
    def from_batch(cls, batch, y, device):
        """`batch`: (g, h, p, e or None, snorm_n or None) of a collated DGL batch (only g.edges() and g.batch_num_nodes() — and
        batch_num_edges() where g has it — are read); y: the targets [G, 1]."""
        g, h, p, e, snorm_n = batch[:5]
        cls._refuse_full_graph(g)
        _device(device)
        sizes = GraphSizes.from_batch(batch, dgl=True)
        src, dst = (t.reshape(-1).long() for t in g.edges())
        first = torch.from_numpy(np.repeat(sizes.node_ptr[:-1], sizes.n_edges)).to(src.device)
        return cls(sizes, src - first, dst - first, h, e, p, snorm_n, y, device)

    def proto(self):
        """The (g, h, p, e, snorm_n, targets) prototype a new capture sizes its buffers from (which optional arrays exist)."""
        if self.target is None:
            raise ValueError("DGLGraphStore: a training step needs targets (the store was built without them)")
        return None, self.h[:0], None, self.e, self.snorm_n, None

    def segments(self, out):
        S = ops
        if out.K != self.K:
            raise ValueError(f"DGLGraphStore: the store holds pos_enc of {self.K} columns, the destination of {out.K}")
        for name in ("e", "snorm_n"):
            if (getattr(self, name) is None) != (getattr(out, name, None) is None):
                raise ValueError(f"DGLGraphStore: {name} is {'missing' if getattr(self, name) is None else 'present'} in the store, "
                                 f"the destination was built {'with' if getattr(self, name) is None else 'without'} it")
        segs = [(self.src, out.src, S.STORE_EDGE, S.GATHER_ENDPOINT, 0), (self.dst, out.dst, S.STORE_EDGE, S.GATHER_ENDPOINT, 0),
                (self.h, out.h, S.STORE_NODE, S.GATHER_COPY, 0)]
        if self.e is not None:
            segs.append((self.e, out.e, S.STORE_EDGE, S.GATHER_COPY, 0))
        segs.append((self.p, out.p, S.STORE_NODE, S.GATHER_COPY, 0))
        if self.snorm_n is not None:
            segs.append((self.snorm_n, out.snorm_n.view(-1), S.STORE_NODE, S.GATHER_COPY, 0))
        if getattr(out, "target", None) is not None:
            if self.target is None:
                raise ValueError("DGLGraphStore: the destination has a target buffer, the store was built without targets")
            segs.append((self.target, out.target.view(-1), S.STORE_GRAPH, S.GATHER_COPY, 0))
        if getattr(out, "batch_num_nodes", None) is not None:
            segs.append((None, out.batch_num_nodes, S.STORE_GRAPH, S.GATHER_NODE_COUNT, 0))
        for name, kind, val in (("node_valid", S.STORE_NODE, 1), ("edge_valid", S.STORE_EDGE, 1), ("graph_valid", S.STORE_GRAPH, 1),
                                ("node_slots", S.STORE_NODE, self.K)):
            if getattr(out, name, None) is not None:
                segs.append((None, getattr(out, name), kind, S.GATHER_CONST, val))
        return segs

    def collate(self, idx):
        """The exact-size batch of the graphs `idx`: (dgl_deepsigns.Graph, h, p, e, snorm_n, targets) — what the DGL nets take in eval
        mode (p: the raw pos_enc [N, K]; snorm_n [N, 1]; targets [B, 1]; the graph's node counts are host values).  ONE launch."""
        from .dgl_deepsigns import Graph
        dev = self.device

        def out(N, E, B, S):
            i64, f32 = dict(dtype=torch.int64, device=dev), dict(dtype=torch.float32, device=dev)
            return types.SimpleNamespace(
                src=torch.empty(E, **i64), dst=torch.empty(E, **i64), h=torch.empty(N, **i64),
                e=None if self.e is None else torch.empty(E, **i64), p=torch.empty(N, self.K, **f32),
                snorm_n=None if self.snorm_n is None else torch.empty(N, 1, **f32),
                target=None if self.target is None else torch.empty(B, 1, **f32), K=self.K)
        hidx, o = self._exact(idx, out)
        g = Graph(o.src, o.dst, torch.from_numpy(self.n_nodes[hidx]), torch.from_numpy(self.n_edges[hidx]))
        return g, o.h, o.p, o.e, o.snorm_n, o.target


class IndexLoader:
    """The index half of a DataLoader: a seeded permutation of range(num_graphs) per epoch, uploaded to the device ONCE per epoch, cut
    into batches.  Iteration yields (host indices [numpy int64], device view of the same slice) — what step_from / gather_into /
    collate take: a step copies nothing to the device.  The order is a pure function of (seed, epoch); every graph appears exactly once
    per epoch; the last batch is ragged unless drop_last.  Iterating runs the epoch chosen by epoch(e) (0 at first) and then moves on to
    the next one, as a DataLoader reshuffles.  Without a visible GPU (host-side planning, tests) the device view is None."""

    def __init__(self, num_graphs, batch_size, shuffle=True, seed=0, drop_last=False, device="cuda"):
        if int(num_graphs) < 0 or int(batch_size) < 1:
            raise ValueError("IndexLoader: num_graphs >= 0 and batch_size >= 1")
        self.num_graphs, self.batch_size = int(num_graphs), int(batch_size)
        self.shuffle, self.seed, self.drop_last = bool(shuffle), int(seed), bool(drop_last)
        self.device = torch.device(device) if torch.cuda.is_available() and torch.device(device).type == "cuda" else None
        self._e, self._perm, self._dperm = 0, None, None

    def permutation(self, e):
        """The host permutation of epoch `e` (no upload)."""
        if not self.shuffle:
            return np.arange(self.num_graphs, dtype=np.int64)
        return np.random.default_rng([self.seed, int(e)]).permutation(self.num_graphs).astype(np.int64)

    def epoch(self, e):
        """Select epoch `e`: returns its host permutation and uploads it (one pinned copy)."""
        self._e, self._perm = int(e), self.permutation(e)
        if self.device is not None:
            self._dperm = torch.from_numpy(self._perm).pin_memory().to(self.device, non_blocking=True)
        return self._perm

    def __len__(self):
        return self.num_graphs // self.batch_size if self.drop_last else -(-self.num_graphs // self.batch_size)

    def __iter__(self):
        if self._perm is None:
            self.epoch(self._e)
        perm, dperm, bs = self._perm, self._dperm, self.batch_size
        self._e, self._perm = self._e + 1, None                 # the next iteration runs the next epoch
        for i in range(len(self)):
            lo, hi = i * bs, min((i + 1) * bs, self.num_graphs)
            yield perm[lo:hi], (None if dperm is None else dperm[lo:hi])
