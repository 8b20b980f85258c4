"""-m gpu: the eigendecomposition of graphs of 65 .. 128 nodes on the device (sn_laplacian_evd_large_f32, csrc/evd_large.hip) against
numpy's float32 eigh at the project's EVD tolerance (tests/test_evd_gpu.py: 4e-6), its status words, its wire format as the forward
reads it, and the routing of transform.evd_laplacian_batch: no library call for a graph of up to 128 nodes."""
import types

import numpy as np
import pytest
import torch

import evd_large_cases as C
import parity_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 4e-6
ST_CROSS, ST_OVERSIZE, ST_NOCONV, ST_SPACE = 1, 2, 4, 8
SMALL = [(7, 12), (8, 37), (9, 64)]           # (seed, n) of the small graphs that share a batch with the mid-size ones


def _gptr(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)


def _dev(ei):
    return torch.from_numpy(np.ascontiguousarray(ei)).to(DEV)


def _check_batch(ei, sizes, norm, D, V):
    from oracle import evd as OE
    off = o2 = 0
    worst = {}
    for n in sizes:
        sel = (ei[0] >= off) & (ei[0] < off + n)
        L = OE.dense_laplacian(ei[:, sel] - off, n, norm)
        dr, vr = OE.evd_laplacian(ei[:, sel] - off, n, norm)
        r = OE.compare_decompositions(D[off:off + n], V[o2:o2 + n * n].reshape(n, n), dr, vr, L, TOL)
        print(f"    n={n} norm={norm}: " + " ".join(f"{k}={v:.2e}" for k, v in r.items() if k != "ok"))
        assert r["ok"], (n, norm, r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0), v)
        off += n
        o2 += n * n
    return worst


def _raw(ei, sizes, norm=None, k=0, skip=1):
    """Both entry points, low level: (val, vec, pe, evoff, status of the 64-node call, status of the mid-size call)."""
    from signnet_basisnet_amd import ops
    N, total = sum(sizes), sum(n * n for n in sizes)
    val, vec, evoff, pe, st = ops.laplacian_evd(_dev(ei), _gptr(sizes), N, total, norm, k, skip)
    stl = ops.laplacian_evd_large(_dev(ei), _gptr(sizes), N, total, evoff, val, vec, pe, norm, k, skip)
    return val, vec, pe, evoff, st, stl


def _small_graph(seed, n):
    from signnet_basisnet_amd import synth
    return synth.make_batch(1, seed=seed, sizes=[n]).edge_index.numpy(), n


def _mixed(sizes, seed=41):
    """A synth batch (host) of the given sizes: built BEFORE torch.linalg.eigh is patched (synth fills its own host eigen-data)."""
    from signnet_basisnet_amd import synth
    return synth.make_batch(len(sizes), seed=seed, sizes=list(sizes))


@pytest.mark.parametrize("norm", [None, "sym"])
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_case_alone(name, norm):
    """Every case of the list as a batch of one graph."""
    from signnet_basisnet_amd import transform as T
    ei, n = next((e, n) for nm, e, n in C.cases() if nm == name)
    val, vec, _, _, st, stl = _raw(ei, [n], norm)
    assert int(st[0]) == ST_OVERSIZE and int(stl[0]) == 0, (st.tolist(), stl.tolist())
    print(f"  {name} norm={norm}: sweeps {int(stl[1])}")
    D, V, _ = T.evd_laplacian_batch(_dev(ei), ptr=_gptr([n]), norm=norm)
    assert torch.equal(D, val) and torch.equal(V, vec)
    _check_batch(ei, [n], norm, D.cpu().numpy(), V.cpu().numpy())


@pytest.mark.parametrize("norm", [None, "sym"])
def test_all_cases_in_one_batch_with_small_graphs(norm):
    from signnet_basisnet_amd import transform as T
    cases = C.cases()
    assert [nm for nm, _, _ in cases] == C.CASE_NAMES
    graphs = [(e, n) for _, e, n in cases]
    small = [_small_graph(s, n) for s, n in SMALL]
    graphs = [small[0]] + graphs[:5] + [small[1]] + graphs[5:] + [small[2]]
    ei, sizes = C.collate(graphs)
    *_, stl = _raw(ei, sizes, norm)
    assert int(stl[0]) == 0, stl.tolist()
    print(f"  one batch norm={norm}: largest sweep count {int(stl[1])}")
    D, V, _ = T.evd_laplacian_batch(_dev(ei), ptr=_gptr(sizes), norm=norm)
    _check_batch(ei, sizes, norm, D.cpu().numpy(), V.cpu().numpy())


def test_no_library_call_up_to_128_nodes(monkeypatch):
    from signnet_basisnet_amd import transform as T
    host = _mixed([10, 70, 12, 128, 65, 37])
    big = _mixed([130, 70, 20], seed=42)
    real = torch.linalg.eigh

    def boom(*a, **k):
        raise AssertionError("torch.linalg.eigh called for a graph of at most 128 nodes")
    monkeypatch.setattr(torch.linalg, "eigh", boom)
    ei = host.edge_index.numpy()
    for norm in (None, "sym"):
        D, V, _ = T.evd_laplacian_batch(host.edge_index.to(DEV), ptr=_gptr(host.sizes), norm=norm)
        _check_batch(ei, host.sizes, norm, D.cpu().numpy(), V.cpu().numpy())
    calls = []

    def counting(*a, **k):
        calls.append(tuple(a[0].shape))
        return real(*a, **k)
    monkeypatch.setattr(torch.linalg, "eigh", counting)
    D, V, _ = T.evd_laplacian_batch(big.edge_index.to(DEV), ptr=_gptr(big.sizes), norm="sym")
    assert calls == [(130, 130)]
    _check_batch(big.edge_index.numpy(), big.sizes, "sym", D.cpu().numpy(), V.cpu().numpy())


def test_other_graphs_are_not_touched():
    """Values, vectors and positional encodings of every graph with n <= 64 or n > 128 are the same bits before and after the
    mid-size call on the same buffers."""
    from signnet_basisnet_amd import ops
    host = _mixed([10, 70, 12, 128, 64, 65, 130, 37, 1])
    sizes, N, total = host.sizes, sum(host.sizes), sum(n * n for n in host.sizes)
    ei = host.edge_index.to(DEV)
    k = 6
    val, vec, evoff, pe, st = ops.laplacian_evd(ei, _gptr(sizes), N, total, "sym", k, 1)
    val[sum(sizes[:6]):sum(sizes[:7])] = 7.0          # the 130-node graph's values are uninitialised memory: make them comparable
    v0, w0, p0 = val.clone(), vec.clone(), pe.clone()
    stl = ops.laplacian_evd_large(ei, _gptr(sizes), N, total, evoff, val, vec, pe, "sym", k, 1)
    assert int(stl[0]) == ST_OVERSIZE                 # the 130-node graph is flagged, nothing else
    n0 = o2 = 0
    for n in sizes:
        same = (torch.equal(val[n0:n0 + n], v0[n0:n0 + n]) and torch.equal(vec[o2:o2 + n * n], w0[o2:o2 + n * n])
                and torch.equal(pe[n0:n0 + n], p0[n0:n0 + n]))
        assert same == (not 64 < n <= 128), n
        n0 += n
        o2 += n * n
    # and the order of the two calls does not matter: the mid-size call clears its own blocks
    val2, vec2 = torch.full_like(val, 3.0), torch.full_like(vec, 3.0)
    pe2 = torch.full_like(pe, 3.0)
    ops.laplacian_evd_large(ei, _gptr(sizes), N, total, evoff, val2, vec2, pe2, "sym", k, 1)
    n0 = o2 = 0
    for n in sizes:
        if 64 < n <= 128:
            assert torch.equal(val2[n0:n0 + n], val[n0:n0 + n]) and torch.equal(vec2[o2:o2 + n * n], vec[o2:o2 + n * n])
            assert torch.equal(pe2[n0:n0 + n], pe[n0:n0 + n])
        else:
            assert bool((val2[n0:n0 + n] == 3.0).all()) and bool((vec2[o2:o2 + n * n] == 3.0).all()) and bool((pe2[n0:n0 + n] == 3.0).all())
        n0 += n
        o2 += n * n


def test_status_of_the_mid_size_entry_point():
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd import transform as T
    host = _mixed([70, 5, 100])
    *_, stl = _raw(host.edge_index.numpy(), host.sizes)
    assert int(stl[0]) == 0 and 1 <= int(stl[1]) < 24
    host = _mixed([129, 5, 70])
    *_, stl = _raw(host.edge_index.numpy(), host.sizes)
    assert int(stl[0]) == ST_OVERSIZE
    # `total` one float short: the last block (a mid-size graph's) does not fit
    host = _mixed([5, 70])
    sizes, N, total = host.sizes, 75, 25 + 4900
    ei = host.edge_index.to(DEV)
    val, vec, evoff, pe, st = ops.laplacian_evd(ei, _gptr(sizes), N, total)
    stl = ops.laplacian_evd_large(ei, _gptr(sizes), N, total - 1, evoff, val, vec)
    assert int(stl[0]) & ST_SPACE
    # an edge between a mid-size graph and its neighbour, in either direction, through the wrapper
    host = _mixed([70, 5])
    for s, d in ((3, 72), (72, 3), (69, 70)):
        bad = torch.cat([host.edge_index, torch.tensor([[s], [d]])], 1)
        with pytest.raises(RuntimeError, match="leaves its graph"):
            T.evd_laplacian_batch(bad.to(DEV), ptr=_gptr(host.sizes))
        *_, st, stl = _raw(bad.numpy(), host.sizes)
        assert int(stl[0]) & ST_CROSS and int(st[0]) & ST_CROSS
    # a crossing edge between two SMALL graphs is the 64-node entry point's to report, not this one's
    host = _mixed([70, 5, 6])
    bad = torch.cat([host.edge_index, torch.tensor([[71], [76]])], 1)
    *_, st, stl = _raw(bad.numpy(), host.sizes)
    assert int(stl[0]) == 0 and int(st[0]) & ST_CROSS


def test_edge_order_and_direction_do_not_matter():
    from signnet_basisnet_amd import transform as T
    host = _mixed([90, 20, 128, 65])
    ei = host.edge_index
    g = torch.Generator().manual_seed(0)
    perm = torch.randperm(ei.shape[1], generator=g)
    half = ei[:, ei[0] < ei[1]]
    a = T.evd_laplacian_batch(ei.to(DEV), ptr=_gptr(host.sizes), norm="sym")
    b = T.evd_laplacian_batch(ei[:, perm].to(DEV), ptr=_gptr(host.sizes), norm="sym")
    c = T.evd_laplacian_batch(half[:, torch.randperm(half.shape[1], generator=g)].to(DEV), ptr=_gptr(host.sizes), norm="sym")
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1], x[1])           # same dense Laplacian -> bit-identical run


def test_check_false_fills_the_mid_size_graphs_without_a_status_read(monkeypatch):
    from signnet_basisnet_amd import transform as T
    host = _mixed([10, 70, 12, 128, 65, 37])
    ei, gp = host.edge_index.to(DEV), _gptr(host.sizes)
    torch.cuda.synchronize()

    def no_read(self, *a, **k):
        raise AssertionError("host read of a device tensor")
    with monkeypatch.context() as mp:
        for name in ("item", "tolist", "cpu", "numpy"):
            mp.setattr(torch.Tensor, name, no_read)
        D, V, _ = T.evd_laplacian_batch(ei, ptr=gp, sizes=list(host.sizes), check=False)
    assert bool(torch.isfinite(D).all()) and bool(torch.isfinite(V).all())
    _check_batch(host.edge_index.numpy(), host.sizes, None, D.cpu().numpy(), V.cpu().numpy())


def test_positional_encoding_of_a_batch_with_a_90_node_graph():
    from signnet_basisnet_amd import transform as T
    host = _mixed([20, 90, 33, 5])
    ei, gp = host.edge_index.to(DEV), _gptr(host.sizes)
    k = 10
    D, V, pe = T.evd_laplacian_batch(ei, ptr=gp, norm="sym", pos_enc_dim=k, skip=1)
    pe2 = T.lap_positional_encoding_batch(ei, ptr=gp, pos_enc_dim=k)
    assert torch.equal(pe, pe2) and pe.shape == (sum(host.sizes), k)
    V, pe = V.cpu().numpy(), pe.cpu().numpy()
    off = o2 = 0
    for n in host.sizes:
        blk = V[o2:o2 + n * n].reshape(n, n)
        kk = min(k, n - 1)
        assert np.array_equal(pe[off:off + n, :kk], blk[:, 1:1 + kk])
        assert not pe[off:off + n, kk:].any()
        off += n
        o2 += n * n
    # zero padding written by the mid-size call itself (k beyond n - skip), into a buffer that was not cleared for it
    from signnet_basisnet_amd import ops
    host = _mixed([66])
    val, vec, evoff, pe, st = ops.laplacian_evd(host.edge_index.to(DEV), _gptr([66]), 66, 66 * 66, "sym", 70, 1)
    pe.fill_(5.0)
    ops.laplacian_evd_large(host.edge_index.to(DEV), _gptr([66]), 66, 66 * 66, evoff, val, vec, pe, "sym", 70, 1)
    assert torch.equal(pe[:, :65], vec.view(66, 66)[:, 1:]) and not bool(pe[:, 65:].any())


def test_end_to_end_device_evd_into_the_forward(monkeypatch):
    """BatchEVDTransform('sym') on sizes [20, 90, 33], then the default (strict) forward — layer path for the 90-node graph, stage
    kernels for the other two — against the oracle fed the SAME device eigen-data: the wire format is what the forward reads."""
    from oracle import pyg_signnet as O
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd import transform as T
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(2)
    ctor = (None, None, 32, 1, 2, 2)
    model = SignNetGNN(*ctor, variant="gine", max_k=8)
    host = _mixed([20, 90, 33], seed=4)
    sd = {k: v.clone() for k, v in model.state_dict().items()}

    def boom(*a, **k):
        raise AssertionError("torch.linalg.eigh called")
    monkeypatch.setattr(torch.linalg, "eigh", boom)
    model = model.cuda().eval()
    dd = synth.batch_to(host, DEV)
    dd.eigen_values = dd.eigen_vectors = None
    T.BatchEVDTransform("sym")(dd)
    assert model.strict
    with torch.no_grad():
        y = model(dd)
    model.check_last()
    fed = types.SimpleNamespace(**vars(host))
    fed.eigen_values, fed.eigen_vectors = dd.eigen_values.cpu(), dd.eigen_vectors.cpu()
    _check_batch(host.edge_index.numpy(), host.sizes, "sym", fed.eigen_values.numpy(), fed.eigen_vectors.numpy())
    cfg = O.make_cfg("gine", *ctor)
    with torch.no_grad():
        y32 = O.signnet_gnn(sd, cfg, fed, training=False, max_k=8)
        y64 = O.signnet_gnn(PU.to_f64(sd), cfg, PU.data_f64(fed), training=False, max_k=8)
    PU.close(y, y32, "forward on the device eigen-data", ref64=y64)
