"""CPU: the bucket policy of train_graph.DGLBucketedStep (capacity rounding, B_cap, LRU order, refusals) and its pack entry point
sn_bucket_pack_dgl (declared in include/signnet_hip.h, bound in _lib.py, argument checks on the host before any launch).  No GPU needed."""
import ctypes as C
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(name="gatedgcn", **over):
    from signnet_basisnet_amd import dgl_configs, dgl_nets
    cls, p = dgl_configs.net_params(name, "cpu")
    p.update(over)
    torch.manual_seed(0)
    return getattr(dgl_nets, cls)(p)


def _step(net=None, **kw):
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    net = net if net is not None else _net()
    return DGLBucketedStep(net, optim.FlatAdam(net.parameters(), lr=1e-3), **kw)


def _fake(N, E, B, sizes=None):
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    if sizes is None:                      # B graphs holding the N nodes
        sizes = [N // B + (1 if i < N % B else 0) for i in range(B)]
    g = Graph(torch.zeros(E, dtype=torch.long), torch.zeros(E, dtype=torch.long), torch.tensor(sizes, dtype=torch.long))
    return g, torch.zeros(N, dtype=torch.long)


def test_capacities_round_up_to_their_granules_with_a_spare_node_and_graph():
    from signnet_basisnet_amd.train_graph import DGLBucket
    s = _step(max_graphs=128, granule=dict(N=256, E=512))
    assert s.B_cap == 129 and s.K == 8
    assert s.bucket_of(*_fake(274, 592, 12)) == DGLBucket(512, 1024)
    assert s.bucket_of(*_fake(256, 512, 12)) == DGLBucket(512, 512)       # N_cap > N: the spare graph has a node
    assert s.bucket_of(*_fake(0, 0, 0)) == DGLBucket(256, 512)
    b = s.bucket_of(*_fake(255, 1, 1))
    assert (b.N, b.E) == (256, 512)
    assert _step(_net("gatedgcn_mask")).K == 37


def test_more_graphs_than_max_graphs_is_refused():
    s = _step(max_graphs=16)
    s.bucket_of(*_fake(100, 10, 16))
    with pytest.raises(ValueError, match="max_graphs"):
        s.bucket_of(*_fake(100, 10, 17))
    g, h = _fake(100, 10, 17)
    with pytest.raises(ValueError, match="max_graphs"):
        s.step(g, h, torch.zeros(100, 8), None, None, torch.zeros(17, 1), bucket=(128, 128))
    assert s.captures == 0 and s.hits == 0 and s.buckets == []


def test_pos_enc_must_be_n_by_pos_enc_dim():
    s = _step()
    g, h = _fake(30, 40, 2)
    for bad in (torch.zeros(30, 7), torch.zeros(30, 8, 1), torch.zeros(29, 8)):
        with pytest.raises(ValueError, match="pos_enc_dim"):
            s.step(g, h, bad, None, None, torch.zeros(2, 1))
    assert s.buckets == []


def test_host_node_counts_that_do_not_sum_to_n_are_refused_before_any_launch():
    """The eager step's ValueError (dgl_nets / dgl_deepsigns _plan) for batch_num_nodes() on the host that does not describe the N
    feature rows: raised by step() and by the pack op before anything reaches the device (the padded node -> graph vector is built
    from these counts)."""
    from signnet_basisnet_amd import ops
    s = _step()
    for sizes in ([10, 10, 9], [10, 10, 11], [31, -1, 0]):
        g, h = _fake(30, 40, 3, sizes=sizes)
        with pytest.raises(ValueError, match="batch_num_nodes does not sum to the number of feature rows"):
            s.step(g, h, torch.zeros(30, 8), None, None, torch.zeros(3, 1))
        with pytest.raises(ValueError, match="batch_num_nodes does not sum to the number of feature rows"):
            ops.bucket_pack_dgl(g, h, torch.zeros(30, 8), None, None, torch.zeros(3, 1), types.SimpleNamespace(h=h))
    assert s.captures == 0 and s.hits == 0 and s.buckets == []
    ops.check_node_total([10, 10, 10], 30)
    ops.check_node_total(torch.tensor([30]), 30)


def test_lru_keeps_max_captures_and_evicts_the_least_recently_used():
    from signnet_basisnet_amd.train_graph import DGLBucket
    s = _step(max_captures=2)

    class _G:
        def __init__(self):
            self.was_reset = False

        def reset(self):
            self.was_reset = True

    caps = {}
    for b in (DGLBucket(256, 512), DGLBucket(512, 512)):
        assert not s._admit(b)
        caps[b] = s._lru[b] = types.SimpleNamespace(graph=_G())
    a, b = list(caps)
    assert s._admit(a)                      # a is now the most recent
    assert s.buckets == [b, a]
    c = DGLBucket(768, 512)
    assert not s._admit(c)                  # evicts b (least recently used), frees its graph
    assert caps[b].graph.was_reset and not caps[a].graph.was_reset
    assert s.buckets == [a]
    s.release()
    assert s.buckets == [] and caps[a].graph.was_reset


def test_constructor_refusals():
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.pyg import SignNetGNN
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    net = _net()
    with pytest.raises(TypeError, match="FlatAdam"):
        DGLBucketedStep(net, torch.optim.Adam(net.parameters()))
    m = SignNetGNN(None, None, 16, 1, 2, 1, variant="gine", max_k=8)
    with pytest.raises(TypeError, match="dgl_nets"):
        DGLBucketedStep(m, optim.FlatAdam(m.parameters(), lr=1e-3))
    o = optim.FlatAdam(net.parameters(), lr=1e-3)
    o.dist = object()
    with pytest.raises(ValueError, match="data-parallel"):
        DGLBucketedStep(net, o)
    o.dist = None
    with pytest.raises(ValueError, match="granule"):
        DGLBucketedStep(net, o, granule=dict(S=3))
    with pytest.raises(ValueError, match="granule"):
        DGLBucketedStep(net, o, granule=dict(N=0))
    net.lap_method = "sign_flip"
    with pytest.raises(ValueError, match="lap_method"):
        DGLBucketedStep(net, o)
    net.lap_method = "sign_inv"
    net.use_lapeig_loss = True
    with pytest.raises(ValueError, match="use_lapeig_loss"):
        DGLBucketedStep(net, o)
    net.use_lapeig_loss = False
    net.sign_inv_net = None
    with pytest.raises(ValueError, match="sign_inv_net"):
        DGLBucketedStep(net, o)
    for name in ("gin", "gat", "pna", "transformer"):        # every dgl_nets base network is taken
        _step(_net(name))


def test_pack_entry_point_is_declared_bound_and_validates_on_the_host():
    from signnet_basisnet_amd import build
    build.build()
    from signnet_basisnet_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "signnet_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    assert re.search(r"\bsn_bucket_pack_dgl\s*\(", hdr)
    assert "sn_bucket_pack_dgl" in _lib.SIGNATURES and hasattr(L, "sn_bucket_pack_dgl")
    # the ctypes mirror has the header's field order and no padding (all members 8 bytes)
    body = re.search(r"typedef struct sn_bucket_pack_dgl_args \{(.*?)\} sn_bucket_pack_dgl_args;", hdr, re.S).group(1)
    fields = re.findall(r"\*?\s*(\w+)\s*(?=[;,])", body)
    assert [f for f, _ in ops._BucketPackDglC._fields_] == fields
    assert C.sizeof(ops._BucketPackDglC) == 8 * len(fields)
    assert L.sn_bucket_pack_dgl(None, None) == -1 and b"sn_bucket_pack_dgl" in L.sn_last_error()
    a = ops._BucketPackDglC()
    a.N, a.N_cap, a.B, a.B_cap, a.K = 10, 10, 1, 2, 8          # N_cap must exceed N (the spare graph's node)
    assert L.sn_bucket_pack_dgl(C.byref(a), None) == -1
    err = L.sn_last_error()
    assert b"sn_bucket_pack_dgl" in err and b"does not fit" in err
    a.N_cap = 11                                               # fits, but no arrays: refused before any launch
    assert L.sn_bucket_pack_dgl(C.byref(a), None) == -1 and b"sn_bucket_pack_dgl: null" in L.sn_last_error()
    assert "count_error" in fields                             # (the device-side node-count check reports there)
