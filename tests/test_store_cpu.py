"""CPU: the host half of the device-resident graph store (signnet_basisnet_amd/data.py) — offset tables, bucket policy, the index
loader — and the entry point sn_store_gather (declared, bound, argument checks on the host before any launch).  No GPU needed."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

import store_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pool():
    return SC.pool("zinc")


def test_offset_tables_of_both_constructors_agree(pool):
    from signnet_basisnet_amd.data import GraphSizes
    samples, y = pool
    a = GraphSizes.from_samples(samples)
    whole = SC.host_collate(samples, range(SC.G))
    b = GraphSizes.from_batch(whole)
    del whole.sizes                                        # (then from bincount)
    c = GraphSizes.from_batch(whole)
    sizes = SC.SIZES + [3]
    assert a.n_nodes.tolist() == sizes and a.n_edges[SC.ZERO_EDGE] == 0 and a.num_graphs == SC.G
    assert a.node_ptr.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert a.eig_ptr.tolist() == np.concatenate([[0], np.cumsum(np.square(sizes))]).tolist()
    assert int(a.edge_ptr[-1]) == whole.edge_index.shape[1]
    for other in (b, c):
        for t in ("node_ptr", "edge_ptr", "eig_ptr"):
            assert getattr(a, t).dtype == np.int64 and np.array_equal(getattr(a, t), getattr(other, t)), t
    # the DGL layout: no eigenvector table; edge counts from batch_num_edges() or from the edge list
    ds = SC.dgl_samples(samples, y, 8)
    d1 = GraphSizes.from_samples(ds, dgl=True)
    g, h, p, e, sn, t = SC.dgl_host_collate(ds, range(SC.G))
    d2 = GraphSizes.from_batch((g, h, p, e, sn), dgl=True)
    g._bne = None
    d3 = GraphSizes.from_batch((g, h, p, e, sn), dgl=True)
    for other in (d1, d2, d3):
        assert other.eig_ptr is None and other.dgl
        assert np.array_equal(a.node_ptr, other.node_ptr) and np.array_equal(a.edge_ptr, other.edge_ptr)


def test_edges_out_of_graph_order_are_refused(pool):
    from signnet_basisnet_amd.data import GraphSizes
    whole = SC.host_collate(pool[0], [2, 3])
    whole.edge_index = whole.edge_index.flip(1)
    with pytest.raises(ValueError, match="grouped by graph"):
        GraphSizes.from_batch(whole)


def _pyg_step(max_k, **kw):
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.pyg import SignNetGNN
    from signnet_basisnet_amd.train_graph import BucketedStep
    m = SignNetGNN(None, None, 16, 1, 2, 1, variant="gine", max_k=max_k)
    return BucketedStep(m, optim.FlatAdam(m.parameters(), lr=1e-3), **kw)


def _dgl_step(**kw):
    from signnet_basisnet_amd import dgl_configs, dgl_nets, optim
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    cls, p = dgl_configs.net_params("gatedgcn", "cpu")
    net = getattr(dgl_nets, cls)(p)
    return DGLBucketedStep(net, optim.FlatAdam(net.parameters(), lr=1e-3), **kw)


def _index_lists(n=50):
    rng = np.random.default_rng(3)
    return [rng.integers(0, SC.G, size=int(rng.integers(1, 9))).tolist() for _ in range(n)]


def test_bucket_of_equals_the_steps_bucket_of_the_host_collated_batch(pool):
    from signnet_basisnet_amd.data import GraphSizes
    samples, y = pool
    sizes = GraphSizes.from_samples(samples)
    ds = SC.dgl_samples(samples, y, 8)
    dsizes = GraphSizes.from_samples(ds, dgl=True)
    gran = dict(N=16, E=32, S=256, K=8)
    steps = [(_pyg_step(8, max_graphs=16, granule=gran), 8, gran), (_pyg_step(None, max_graphs=16, granule=gran), None, gran),
             (_pyg_step(8, max_graphs=16), 8, None)]
    dstep, ddefault = _dgl_step(max_graphs=16, granule=dict(N=32, E=64)), _dgl_step(max_graphs=16)
    for idx in _index_lists():
        host = SC.host_collate(samples, idx)
        for step, max_k, g in steps:
            assert sizes.bucket_of(idx, g, max_k) == step.bucket_of(host), (idx, max_k)
        dh = SC.dgl_host_collate(ds, idx)
        assert dsizes.bucket_of(idx, dict(N=32, E=64)) == dstep.bucket_of(dh[0], dh[1]), idx
        assert dsizes.bucket_of(idx) == ddefault.bucket_of(dh[0], dh[1])


def test_covering_bucket_is_the_componentwise_maximum(pool):
    from signnet_basisnet_amd.data import GraphSizes
    from signnet_basisnet_amd.train_graph import Bucket, DGLBucket
    samples, y = pool
    for sizes, kw in ((GraphSizes.from_samples(samples), dict(granule=dict(N=16, E=32, S=256), max_k=None)),
                      (GraphSizes.from_samples(samples), dict(max_k=8)),
                      (GraphSizes.from_samples(SC.dgl_samples(samples, y, 8), dgl=True), dict(granule=dict(N=32, E=64)))):
        lists = _index_lists(20)
        cover = sizes.covering_bucket(lists, **kw)
        each = [sizes.bucket_of(i, **kw) for i in lists]
        assert isinstance(cover, DGLBucket if sizes.dgl else Bucket)
        assert all(c >= v for b in each for c, v in zip(cover, b))
        assert tuple(cover) == tuple(max(c) for c in zip(*each))
        assert len(set(each)) > 1
    with pytest.raises(ValueError, match="no batches"):
        sizes.covering_bucket([])


def test_totals_count_an_index_out_of_range_as_an_empty_graph(pool):
    from signnet_basisnet_amd.data import GraphSizes
    sizes = GraphSizes.from_samples(pool[0])
    assert sizes.totals([4, SC.G, -1, 0]) == sizes.totals([4, 0])
    assert sizes.totals([4, 0])[0] == 65 and sizes.totals([4, 0])[2] == 64 * 64 + 1 and sizes.totals([4, 0])[3] == 64
    assert sizes.totals([]) == (0, 0, 0, 0)


def test_index_loader_is_a_pure_function_of_seed_and_epoch():
    from signnet_basisnet_amd.data import IndexLoader
    a, b = IndexLoader(37, 8, seed=4), IndexLoader(37, 8, seed=4)
    for e in (0, 1, 5):
        pa = a.epoch(e)
        assert np.array_equal(pa, b.permutation(e)) and pa.dtype == np.int64
        assert sorted(pa.tolist()) == list(range(37))                               # every graph exactly once
    assert not np.array_equal(a.permutation(0), a.permutation(1))
    assert not np.array_equal(a.permutation(0), IndexLoader(37, 8, seed=5).permutation(0))
    # iteration: the epoch chosen by epoch(e), a ragged last batch, then the next epoch
    a.epoch(2)
    got = [h for h, _ in a]
    assert [len(h) for h in got] == [8, 8, 8, 8, 5] and len(a) == 5
    assert np.array_equal(np.concatenate(got), b.permutation(2))
    assert np.array_equal(np.concatenate([h for h, _ in a]), b.permutation(3))
    # drop_last; no shuffle
    d = IndexLoader(37, 8, seed=4, drop_last=True)
    got = [h for h, _ in d]
    assert [len(h) for h in got] == [8, 8, 8, 8] and len(d) == 4 and np.array_equal(np.concatenate(got), b.permutation(0)[:32])
    assert np.concatenate([h for h, _ in IndexLoader(10, 4, shuffle=False)]).tolist() == list(range(10))
    with pytest.raises(ValueError):
        IndexLoader(10, 0)


def test_building_a_store_without_a_device_raises_gpu_only(pool):
    from signnet_basisnet_amd.data import DGLGraphStore, GraphStore
    samples, y = pool
    for dev in ("cpu",) if torch.cuda.is_available() else ("cpu", "cuda"):
        with pytest.raises(RuntimeError, match="GPU only"):
            GraphStore.from_samples(samples, dev, y=y)
        with pytest.raises(RuntimeError, match="GPU only"):
            GraphStore.from_batch(SC.host_collate(samples, range(SC.G)), y, dev)
        with pytest.raises(RuntimeError, match="GPU only"):
            DGLGraphStore.from_samples(SC.dgl_samples(samples, y, 8), dev)


def test_the_entry_point_is_declared_bound_and_validates_on_the_host():
    from signnet_basisnet_amd import build
    build.build()
    from signnet_basisnet_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "signnet_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for name in ("sn_store_gather", "sn_store_gather_max_graphs"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.sn_version() == 3
    assert L.sn_store_gather_max_graphs() >= 1024
    # the ctypes mirrors have the header's field order and the C layout
    for cname, mirror in (("sn_store_seg", ops._StoreSegC), ("sn_store_gather_args", ops._StoreGatherC)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        fields = [f for f in re.findall(r"\*?\s*(\w+)\s*(?:\[\w+\])?\s*(?=[;,])", body)]
        assert [f for f, _ in mirror._fields_] == fields, cname
    assert C.sizeof(ops._StoreSegC) == 40
    assert C.sizeof(ops._StoreGatherC) == 13 * 8 + 8 + 12 * 40 + 4 * 8
    assert int(re.search(r"#define SN_STORE_MAX_SEGS (\d+)", hdr).group(1)) == ops.STORE_MAX_SEGS
    for name in ("STORE_NODE", "STORE_EDGE", "STORE_EIG", "STORE_GRAPH", "GATHER_COPY", "GATHER_ENDPOINT", "GATHER_GRAPH_ID",
                 "GATHER_CONST", "GATHER_NODE_COUNT"):
        assert int(re.search(r"#define SN_%s (\d+)" % name, hdr).group(1)) == getattr(ops, name), name
    # argument checks before any launch
    assert L.sn_store_gather(None, None) == -1 and b"sn_store_gather" in L.sn_last_error()
    buf = (C.c_int64 * 64)()
    base = C.addressof(buf)
    a = ops._StoreGatherC()
    a.node_ptr = a.edge_ptr = a.index = a.status = base
    a.B, a.B_cap, a.N, a.N_cap = 1, 2, 10, 10                  # N_cap must exceed N (the spare graph's node)
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"does not fit" in L.sn_last_error()
    a.N_cap = 11
    a.B, a.B_cap = 1025, 1026
    assert L.sn_store_gather(C.byref(a), None) == -3 and b"1024" in L.sn_last_error()          # SN_ERR_UNSUPPORTED names the limit
    a.B, a.B_cap = 1, 2
    a.exact = 1
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"exact" in L.sn_last_error()
    a.exact, a.nseg = 0, 1
    s = a.seg[0]
    s.src, s.dst, s.row_bytes, s.kind, s.op = base, base + 64, 6, ops.STORE_NODE, ops.GATHER_COPY
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"whole 4-byte words" in L.sn_last_error()
    s.row_bytes, s.dst = 8, base + 66
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"aligned" in L.sn_last_error()
    s.dst, s.op = base + 68, ops.GATHER_GRAPH_ID                                               # int64 rows: 8-byte aligned
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"8-byte aligned" in L.sn_last_error()
    s.dst, s.op, s.src = base + 64, ops.GATHER_COPY, None
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"null source" in L.sn_last_error()
    s.src, s.kind = base, ops.STORE_EIG
    a.S_cap = 4
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"eig_ptr" in L.sn_last_error()
    s.kind = 7
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"kind" in L.sn_last_error()
    a.nseg = 13
    assert L.sn_store_gather(C.byref(a), None) == -1 and b"segments" in L.sn_last_error()
