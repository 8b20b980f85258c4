"""-m gpu: the device-resident graph store (data.GraphStore / DGLGraphStore) and sn_store_gather.  Data movement: every comparison is
torch.equal.  The gather into capacity buffers equals ops.bucket_pack / bucket_pack_dgl of the HOST-collated batch (store_cases.py:
torch.cat with node offsets, in index order) — validity, counts and padding included; collate() equals the host collate and the models
give the same outputs on both; no write leaves a destination (sentinel words around every array) whatever the indices and totals are;
training steps from the store equal steps on the host-collated batches bit for bit; one covering bucket means one capture."""
import types

import numpy as np
import pytest
import torch

import store_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# descending and repeated, the 64-node graph alone, one-node graphs only, the zero-edge graph alone, all ten
IDX_CASES = ([0], [9, 3, 3, 0], [4], [8, 0], [SC.ZERO_EDGE], list(range(10)))
PYG_FIELDS = ("x", "edge_index", "edge_attr", "batch", "eigen_values", "eigen_vectors", "target", "node_valid", "edge_valid",
              "graph_valid", "counts")
DGL_FIELDS = ("src", "dst", "h", "e", "p", "snorm_n", "target", "batch_num_nodes", "node_valid", "node_slots", "edge_valid",
              "graph_valid", "counts", "count_error")


@pytest.fixture(scope="module")
def pools():
    return {f: SC.pool(f) for f in ("zinc", "alchemy")}


@pytest.fixture(scope="module")
def stores(pools):
    from signnet_basisnet_amd.data import GraphStore
    out = {}
    for f, (samples, y) in pools.items():
        out[f] = GraphStore.from_samples(samples, DEV, y=y)
    return out


def _to(d, dev=DEV):
    from signnet_basisnet_amd import synth
    return synth.batch_to(d, dev)


def _gdev(g):
    """A host-collated Graph with its edge list on the device and its node counts on the host (as the DGL tests build it)."""
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    return Graph(g.src.to(DEV), g.dst.to(DEV), g.batch_num_nodes().tolist())


def _scribble(pad, fields):
    """Every word of the capacity buffers must be WRITTEN by the call under test: start from a pattern that is no valid content."""
    for f in fields:
        t = getattr(pad, f, None)
        if t is not None:
            t.view(torch.int32 if t.element_size() % 8 else torch.int64).fill_(0x5A5A5A5A)


def _same(a, b, fields, what):
    for f in fields:
        ta, tb = getattr(a, f, None), getattr(b, f, None)
        assert (ta is None) == (tb is None), (what, f)
        if ta is not None:
            assert ta.dtype == tb.dtype and torch.equal(ta, tb), (what, f)


def _pyg_caps(mode, sizes, idx):
    from signnet_basisnet_amd.train_graph import Bucket
    N, E, S, _ = sizes.totals(idx)
    if mode == "exact":                   # capacities that fit exactly: one padding node, nothing else
        return Bucket(N + 1, max(E, 1), S, 8), len(idx) + 1
    return sizes.bucket_of(idx, None, 8), 17


# ----------------------------------------------------------------------------- padded gather against the pack
@pytest.mark.parametrize("mode", ["exact", "granules"])
@pytest.mark.parametrize("features", ["zinc", "alchemy"])
def test_padded_gather_equals_the_pack_of_the_host_collated_batch(pools, stores, features, mode):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import PaddedBatch
    samples, y = pools[features]
    store = stores[features]
    assert tuple(store.x.shape[1:]) == ((1,) if features == "zinc" else (6,))      # 8-byte and 24-byte node rows
    for idx in IDX_CASES:
        host = _to(SC.host_collate(samples, idx, y))
        bucket, B_cap = _pyg_caps(mode, store, idx)
        ref, got = (PaddedBatch(bucket, B_cap, host, host.y, DEV) for _ in range(2))
        _scribble(ref, PYG_FIELDS)
        _scribble(got, PYG_FIELDS)
        totals = ops.bucket_pack(host, host.y, ref)
        assert store.gather_into(idx, got) == totals
        _same(ref, got, PYG_FIELDS, (features, mode, idx))
        N, E, B, S = totals
        assert got.gather_status.tolist() == [0, N, E, S]
        assert got.counts.tolist() == [N, E, B, S] and int(got.node_valid.sum()) == N and got.batch[N:].eq(B_cap - 1).all()


def test_stores_built_from_samples_and_from_a_collated_batch_are_equal(pools, stores):
    from signnet_basisnet_amd.data import GraphStore
    for f, (samples, y) in pools.items():
        whole = SC.host_collate(samples, range(SC.G))
        a, b = stores[f], GraphStore.from_batch(whole, y, DEV)
        del whole.sizes
        c = GraphStore.from_batch(_to(whole), y.to(DEV), DEV)               # a batch already on the device, sizes from bincount
        for other in (b, c):
            for t in ("x", "edge_index", "edge_attr", "eigen_values", "eigen_vectors", "y", "d_node_ptr", "d_edge_ptr", "d_eig_ptr"):
                assert torch.equal(getattr(a, t), getattr(other, t)), (f, t)
        assert a.edge_index.numel() == 0 or int(a.edge_index.max()) < 64         # graph-local node ids


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("with_snorm", [False, True])
@pytest.mark.parametrize("with_e", [False, True])
def test_dgl_padded_gather_equals_the_dgl_pack(pools, with_e, with_snorm, K):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.data import DGLGraphStore
    from signnet_basisnet_amd.train_graph import DGLBucket, DGLPaddedBatch
    samples, y = pools["zinc"]
    ds = SC.dgl_samples(samples, y, K, with_e, with_snorm)
    store = DGLGraphStore.from_samples(ds, DEV)
    g, h, p, e, sn, t = SC.dgl_host_collate(ds, range(SC.G))
    other = DGLGraphStore.from_batch((g, h, p, e, sn), t, DEV)
    for f in ("src", "dst", "h", "e", "p", "snorm_n", "target", "d_node_ptr", "d_edge_ptr"):
        a, b = getattr(store, f), getattr(other, f)
        assert (a is None and b is None) or torch.equal(a, b), f
    for idx in IDX_CASES:
        g, h, p, e, sn, t = SC.dgl_host_collate(ds, idx)
        dev = lambda v: None if v is None else v.to(DEV)
        N, E, _, _ = store.totals(idx)
        for bucket, B_cap in ((DGLBucket(N + 1, max(E, 1)), len(idx) + 1), (store.bucket_of(idx), 17)):
            ref, got = (DGLPaddedBatch(bucket, B_cap, K, with_e, with_snorm, DEV) for _ in range(2))
            _scribble(ref, DGL_FIELDS)
            _scribble(got, DGL_FIELDS)
            ops.bucket_pack_dgl(_gdev(g), dev(h), dev(p), dev(e), dev(sn), dev(t), ref)
            assert store.gather_into(idx, got) == (N, E, len(idx), 0)
            _same(ref, got, DGL_FIELDS, (with_e, with_snorm, K, idx, bucket))
            assert got.gather_status.tolist() == [0, N, E, 0] and int(got.batch_num_nodes.sum()) == bucket.N
            assert int(got.count_error[0]) == 0


# ----------------------------------------------------------------------------- collate(idx) against the host collate
@pytest.mark.parametrize("features", ["zinc", "alchemy"])
def test_collate_equals_the_host_collate(pools, stores, features):
    samples, y = pools[features]
    loader_like = (np.asarray([9, 3, 3, 0]), torch.tensor([7, 9, 3, 3, 0, 1], device=DEV)[1:5])     # (host, device VIEW) pair
    for idx in IDX_CASES + (loader_like,):
        host = SC.host_collate(samples, idx[0].tolist() if isinstance(idx, tuple) else idx, y)
        got = stores[features].collate(idx)
        for f in ("x", "edge_index", "edge_attr", "batch", "eigen_values", "eigen_vectors", "y"):
            a, b = getattr(host, f), getattr(got, f).cpu()
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), (features, idx, f)
        assert (got.num_graphs, got.num_nodes, got.sizes) == (host.num_graphs, host.num_nodes, host.sizes)
    with pytest.raises(IndexError, match="out of range"):
        stores[features].collate([0, SC.G])
    with pytest.raises(TypeError, match="host indices"):
        stores[features].collate(torch.tensor([0, 1], device=DEV))


@pytest.mark.parametrize("variant", ["gine", "alchemy"])
def test_the_model_gives_the_same_output_on_collate_and_on_the_host_collate(pools, stores, variant):
    from signnet_basisnet_amd.pyg import SignNetGNN
    features = "zinc" if variant == "gine" else "alchemy"
    torch.manual_seed(1)
    m = SignNetGNN(*((None, None) if variant == "gine" else (6, 4)), 32, 1, 3, 2, variant=variant, max_k=8).to(DEV).eval()
    idx = [9, 3, 3, 0, SC.ZERO_EDGE, 4]
    with torch.no_grad():
        a = m(_to(SC.host_collate(pools[features][0], idx)))
        b = m(stores[features].collate(idx))
    assert a.shape == (len(idx), 1) and torch.equal(a, b)


def _dgl_net(name="gin", seed=3, **over):
    from signnet_basisnet_amd import dgl_configs, dgl_nets
    cls, p = dgl_configs.net_params(name, DEV)
    p.update(over)
    torch.manual_seed(seed)
    return getattr(dgl_nets, cls)(p).to(DEV)


def test_ginnet_gives_the_same_output_on_collate_and_on_the_host_collate(pools):
    from signnet_basisnet_amd.data import DGLGraphStore
    samples, y = pools["zinc"]
    net = _dgl_net(L=4).eval()
    ds = SC.dgl_samples(samples, y, net.pos_enc_dim, True, False)
    store = DGLGraphStore.from_samples(ds, DEV)
    idx = [9, 3, 3, 0, 4]
    g, h, p, e, sn, t = SC.dgl_host_collate(ds, idx)
    cg, ch, cp, ce, csn, ct = store.collate(idx)
    assert csn is None and torch.equal(ch.cpu(), h) and torch.equal(cp.cpu(), p) and torch.equal(ce.cpu(), e) and torch.equal(ct.cpu(), t)
    assert torch.equal(cg.edges()[0].cpu(), g.edges()[0]) and torch.equal(cg.edges()[1].cpu(), g.edges()[1])
    assert cg.batch_num_nodes().tolist() == g.batch_num_nodes().tolist() and cg.batch_num_edges().tolist() == g.batch_num_edges().tolist()

    def fwd(g, h, p, e):
        with torch.no_grad():
            return net(g, h, net.sign_inv_net(g, p.unsqueeze(-1)).squeeze(-1), e, None)[0]
    assert torch.equal(fwd(_gdev(g), h.to(DEV), p.to(DEV), e.to(DEV)), fwd(cg, ch, cp, ce))


# ----------------------------------------------------------------------------- guard check
SENTINEL = 0x7E7E7E7E


def _carved(like):
    """A copy of the capacity buffers `like` (a PaddedBatch) carved out of ONE allocation, two sentinel words before and after every
    array (8-byte aligned arrays, most of them not 16-byte aligned).  -> (namespace, the allocation, mask of the sentinel words)."""
    names = [f for f in PYG_FIELDS]
    words = {f: getattr(like, f).numel() * getattr(like, f).element_size() // 4 for f in names}
    total = 2 + sum(-(-w // 2) * 2 + 2 for w in words.values())
    big = torch.full((total,), SENTINEL, dtype=torch.int32, device=DEV)
    guard = torch.ones(total, dtype=torch.bool, device=DEV)
    out = types.SimpleNamespace(N_cap=like.N_cap, E_cap=like.E_cap, B_cap=like.B_cap, S_cap=like.S_cap, K=like.K)
    off = 2
    for f in names:
        t = getattr(like, f)
        setattr(out, f, big[off:off + words[f]].view(t.dtype).view(t.shape))
        guard[off:off + words[f]] = False
        off += -(-words[f] // 2) * 2 + 2
    return out, big, guard


def _intact(big, guard):
    return bool((big[guard] == SENTINEL).all())


@pytest.mark.parametrize("features", ["zinc", "alchemy"])
def test_no_write_leaves_a_destination_and_the_status_block_says_why(pools, stores, features):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import Bucket, PaddedBatch
    samples, y = pools[features]
    store = stores[features]
    idx = [9, 3, 3, 0]
    host = _to(SC.host_collate(samples, idx, y))
    N, E, S, _ = store.totals(idx)
    ref = PaddedBatch(Bucket(N + 3, E + 5, S + 7, 8), 6, host, host.y, DEV)
    ops.bucket_pack(host, host.y, ref)
    out, big, guard = _carved(ref)
    assert out.x.data_ptr() % 16 == 8                                         # (the unaligned-destination path is exercised)
    # valid indices
    store.gather_into(idx, out)
    _same(ref, out, PYG_FIELDS, "carved")
    assert _intact(big, guard) and out.gather_status.tolist() == [0, N, E, S]
    # indices out of range: empty graphs, flag 1, the rest of the batch as if they were not there
    bad = [9, SC.G, 3, -1]
    n2, e2, s2, _ = store.totals([9, 3])
    assert store.totals(bad) == store.totals([9, 3])
    assert store.gather_into(bad, out) == (n2, e2, 4, s2)
    two = _to(SC.host_collate(samples, [9, 3], y))
    assert _intact(big, guard) and out.gather_status.tolist() == [ops.GATHER_BAD_INDEX, n2, e2, s2]
    assert out.counts.tolist() == [n2, e2, 4, s2] and out.graph_valid.tolist() == [1, 1, 1, 1, 0, 0]
    assert torch.equal(out.x[:n2], two.x) and torch.equal(out.edge_index[:, :e2], two.edge_index)
    assert torch.equal(out.eigen_vectors[:s2], two.eigen_vectors) and not out.eigen_vectors[s2:].any()
    assert out.batch[:n2].tolist() == [0] * 12 + [2] * 37 and out.batch[n2:].eq(5).all()
    assert torch.equal(out.target[0], two.y[0]) and torch.equal(out.target[2], two.y[1]) and not out.target[[1, 3, 4, 5]].any()
    # host totals passed too small through the raw op: flag 2, the device's totals reported, the whole batch padding
    args = ops.store_gather_args(store.tables(), store.num_graphs, (out.N_cap, out.E_cap, out.B_cap, out.S_cap), store.segments(out),
                                 out.gather_status, out.counts)
    didx = torch.tensor(idx, device=DEV)
    for wrong in ((N - 1, E, S), (N, E - 2, S), (N, E, S - 1)):
        ops.store_gather(args, didx, len(idx), wrong)
        assert _intact(big, guard) and out.gather_status.tolist() == [ops.GATHER_MISMATCH, N, E, S]
        assert out.counts.tolist() == [0, 0, 0, 0] and not out.node_valid.any() and not out.edge_valid.any() and not out.graph_valid.any()
        assert not out.x.any() and out.batch.eq(5).all() and int(out.edge_index.max()) < out.N_cap
    # graphs on the device that are LARGER than the capacities (the host was told about graph 0, the device view names the 64-node
    # graph and all ten): flag 2 again, nothing written past a capacity
    small = PaddedBatch(Bucket(2, 1, 1, 8), 11, host, host.y, DEV)
    out, big, guard = _carved(small)
    out.gather_status = torch.zeros(4, dtype=torch.int32, device=DEV)
    args = ops.store_gather_args(store.tables(), store.num_graphs, (2, 1, 11, 1), store.segments(out), out.gather_status, out.counts)
    for didx, B in ((torch.tensor([4], device=DEV), 1), (torch.arange(10, device=DEV), 10)):
        ops.store_gather(args, didx, B, (1, 0, 1))
        tn, te, ts, _ = store.totals(didx.tolist())
        assert _intact(big, guard) and out.gather_status.tolist() == [ops.GATHER_MISMATCH, tn, te, ts]
        assert out.counts.tolist() == [0, 0, 0, 0]
    ops.store_gather(args, torch.tensor([0], device=DEV), 1, (1, 0, 1))
    assert _intact(big, guard) and out.gather_status.tolist() == [0, 1, 0, 1] and out.counts.tolist() == [1, 0, 1, 1]
    # a batch that does not fit raises before any launch: the buffers and the status block keep their content
    before = big.clone()
    for too_big in ([4], [1], list(range(11))):
        with pytest.raises(ValueError, match="does not fit"):
            store.gather_into(too_big, out)
    assert torch.equal(big, before) and out.gather_status.tolist() == [0, 1, 0, 1]


# ----------------------------------------------------------------------------- steps from the store against steps on host batches
def _index_lists(pool_ids, n=6, seed=2):
    rng = np.random.default_rng(seed)
    return [rng.choice(pool_ids, size=int(rng.integers(2, 5)), replace=True).tolist() for _ in range(n)]


def _pyg_model(variant, max_k, sd=None):
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(7)
    m = SignNetGNN(*((None, None) if variant == "gine" else (6, 4)), 32, 1, 3, 2, variant=variant, max_k=max_k)
    if sd is not None:
        m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.attn_dropout = 0.0
    return m, optim.FlatAdam(m.parameters(), lr=1e-3)


@pytest.mark.parametrize("max_k", [8, None])
@pytest.mark.parametrize("variant", ["gine", "alchemy"])
def test_steps_from_the_store_equal_steps_on_host_collated_batches_bit_for_bit(pools, variant, max_k):
    from signnet_basisnet_amd.data import GraphStore
    from signnet_basisnet_amd.train_graph import BucketedStep
    samples, y = pools["zinc" if variant == "gine" else "alchemy"]
    store = GraphStore.from_samples(samples, DEV, y=y[:, :1])
    # (all-eigenvector mode: without the 64-node graph, K_cap = 40)
    lists = _index_lists([i for i in range(SC.G) if max_k or i != 4])
    bucket = store.covering_bucket(lists, dict(N=16, E=32, S=256, K=8), max_k)
    m1, o1 = _pyg_model(variant, max_k)
    m2, o2 = _pyg_model(variant, max_k, {k: v.clone() for k, v in m1.state_dict().items()})
    s1, s2 = BucketedStep(m1, o1, max_graphs=8), BucketedStep(m2, o2, max_graphs=8)
    la, lb = [], []
    for idx in lists:
        la.append(s1.step_from(store, idx, bucket=bucket).clone())
        host = _to(SC.host_collate(samples, idx, y[:, :1]))
        lb.append(s2.step(host, host.y, bucket=bucket).clone())
    s1.check()
    s2.check()
    assert s1.captures == s2.captures == 1 and s1.hits == s2.hits == len(lists) - 1
    for a, b in zip(la, lb):
        assert torch.equal(a, b), (la, lb)
    assert torch.equal(o1.flat_p, o2.flat_p)
    for (n, p), (_, q) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(p, q), n
    for (n, p), (_, q) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(p, q), n


def test_dgl_steps_from_the_store_equal_steps_on_host_collated_batches_bit_for_bit(pools):
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.data import DGLGraphStore
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    samples, y = pools["zinc"]
    n1 = _dgl_net(L=4).train()
    n2 = _dgl_net(L=4, seed=9).train()
    n2.load_state_dict({k: v.clone() for k, v in n1.state_dict().items()})
    ds = SC.dgl_samples(samples, y, n1.pos_enc_dim, True, False)
    store = DGLGraphStore.from_samples(ds, DEV)
    lists = _index_lists(list(range(SC.G)))
    bucket = store.covering_bucket(lists, dict(N=32, E=64))
    o1, o2 = optim.FlatAdam(n1.parameters(), lr=1e-3), optim.FlatAdam(n2.parameters(), lr=1e-3)
    s1, s2 = DGLBucketedStep(n1, o1, max_graphs=8), DGLBucketedStep(n2, o2, max_graphs=8)
    la, lb = [], []
    for idx in lists:
        la.append(s1.step_from(store, idx, bucket=bucket).clone())
        g, h, p, e, sn, t = SC.dgl_host_collate(ds, idx)
        lb.append(s2.step(_gdev(g), h.to(DEV), p.to(DEV), e.to(DEV), None, t.to(DEV), bucket=bucket).clone())
    s1.check()
    s2.check()
    assert s1.captures == s2.captures == 1 and s1.hits == s2.hits == len(lists) - 1
    for a, b in zip(la, lb):
        assert torch.equal(a, b), (la, lb)
    assert torch.equal(o1.flat_p, o2.flat_p)
    for (n, p), (_, q) in zip(n1.named_buffers(), n2.named_buffers()):
        assert torch.equal(p, q), n
    with pytest.raises(TypeError, match="DGLGraphStore"):
        s1.step_from(types.SimpleNamespace(dgl=False), [0])


# ----------------------------------------------------------------------------- capture count and the deferred error
def test_one_covering_bucket_means_one_capture_and_a_bad_index_raises_at_check(pools):
    from signnet_basisnet_amd.data import GraphStore, IndexLoader
    from signnet_basisnet_amd.train_graph import BucketedStep
    samples, y = pools["zinc"]
    store = GraphStore.from_samples(samples, DEV, y=y[:, :1])
    loader = IndexLoader(store.num_graphs, 4, shuffle=True, seed=1, device=DEV)
    gran = dict(N=16, E=32, S=256)
    every = [loader.permutation(e)[i:i + 4] for e in range(3) for i in range(0, store.num_graphs, 4)]
    assert len({store.bucket_of(b, gran, 8) for b in every}) > 4                  # (more buckets than the LRU keeps captures)
    bucket = store.covering_bucket(every, gran, 8)
    m, o = _pyg_model("gine", 8)
    s = BucketedStep(m, o, max_graphs=4, granule=gran)
    seen = []
    for e in range(3):
        perm = loader.epoch(e)
        for host_idx, dev_idx in loader:
            assert dev_idx.is_cuda and dev_idx.tolist() == host_idx.tolist()
            s.step_from(store, (host_idx, dev_idx), bucket=bucket)
            seen.append(host_idx)
        assert np.array_equal(np.concatenate(seen[-3:]), perm)
    s.check()
    assert s.captures == 1 and s.hits == 8 and s.buckets == [bucket]
    with pytest.raises(TypeError, match="GraphStore"):
        s.step_from(types.SimpleNamespace(dgl=True), [0])
    with pytest.raises(ValueError, match="max_graphs"):
        s.step_from(store, [0, 1, 2, 3, 5], bucket=bucket)
    # an index outside the store: the step runs (that graph is empty), check() raises; the next good step clears it; a step() on a
    # host batch does not look at the gather's stale status
    s.step_from(store, [0, store.num_graphs, 2], bucket=bucket)
    with pytest.raises(IndexError, match="graph index out of range"):
        s.check()
    s.step_from(store, [0, 2], bucket=bucket)
    s.check()
    s.step_from(store, [0, -1], bucket=bucket)
    host = _to(SC.host_collate(samples, [0, 2], y[:, :1]))
    s.step(host, host.y, bucket=bucket)
    s.check()
    assert s.captures == 1


# ----------------------------------------------------------------------------- call rejection
def test_calls_the_kernel_is_not_built_for_are_refused(pools, stores):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import Bucket, PaddedBatch
    samples, y = pools["zinc"]
    store = stores["zinc"]
    limit = ops.store_gather_max_graphs()
    assert limit >= 1024
    host = _to(SC.host_collate(samples, [0], y))
    pad = PaddedBatch(Bucket(limit + 64, 8, limit + 64, 8), limit + 2, host, host.y, DEV)
    # exactly the limit is served; one more is SN_ERR_UNSUPPORTED naming the limit
    assert store.gather_into([0] * limit, pad) == (limit, 0, limit, limit)
    assert pad.gather_status.tolist() == [0, limit, 0, limit] and int(pad.batch[limit - 1]) == limit - 1
    with pytest.raises(RuntimeError, match=r"code -3.*at most %d" % limit):
        store.gather_into([0] * (limit + 1), pad)
    caps = (pad.N_cap, pad.E_cap, pad.B_cap, pad.S_cap)
    segs = store.segments(pad)
    # wrong dtype / row shape / row count: ValueError from the binding, before the library is called
    for i, wrong in ((0, pad.x.float()), (0, torch.zeros(pad.N_cap, 2, dtype=torch.int64, device=DEV)), (0, pad.x[:-1]),
                     (4, pad.batch.int()), (8, pad.node_valid.float())):
        s = list(segs)
        s[i] = (s[i][0], wrong) + s[i][2:]
        with pytest.raises(ValueError, match="segment %d" % i):
            ops.store_gather_args(store.tables(), store.num_graphs, caps, s, pad.gather_status, pad.counts)
    with pytest.raises(ValueError, match="int64"):
        ops.store_gather_args((store.d_node_ptr.int(), store.d_edge_ptr, store.d_eig_ptr), store.num_graphs, caps, segs,
                              pad.gather_status, pad.counts)
    # a misaligned array (torch makes none: the parameter block is edited): SN_ERR_ARG from the library's host-side checks
    args = ops.store_gather_args(store.tables(), store.num_graphs, caps, segs, pad.gather_status, pad.counts)
    args.seg[4].dst += 4
    with pytest.raises(RuntimeError, match="code -1.*8-byte aligned"):
        ops.store_gather(args, torch.tensor([0], device=DEV), 1, (1, 0, 1))
    with pytest.raises(ValueError, match="index must be contiguous int64"):
        ops.store_gather(store._args(pad), torch.tensor([0], device=DEV, dtype=torch.int32), 1, (1, 0, 1))
