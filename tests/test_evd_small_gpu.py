"""-m gpu: the 64-node eigendecomposition kernel (sn_laplacian_evd_f32, csrc/evd.hip) on the degenerate graphs of
tests/evd_small_cases.py — every row-count instantiation on both sides of its threshold, shared and partly filled workgroups, null spaces
and large multiplicities, more than 256 graphs, empty graphs, one- and two-node graphs under a wider positional encoding, self loops and
duplicate edges, out-of-range node ids and a short eigen_vectors buffer — against numpy's float32 eigh through
oracle.evd.compare_decompositions at the project's EVD tolerance (tests/test_evd_gpu.py: 4e-6; projectors 1e3 x that).
tests/test_evd_small_cpu.py asserts, without a GPU, that the table reaches the instantiations it names, that a float32 emulation of the
method stays inside the same tolerance, and that no cluster decision of the comparison sits on its threshold.

Measured on an MI355X, worst over all cases, batches and both norms (bound 4e-6; projector 4e-3): eigenvalues 3.9e-7 (star49, None),
residual 5.4e-7 (K64, sym), orthogonality 6.3e-7 (grid8x8, sym), projector 1.3e-5 (grid6x8, sym); no eigenvalue pair out of order.  Most
sweeps: 11 (path63, both norms; cycle64, two_paths_30_34 and path40_plus_24_isolated take up to 10) under the cap of 16; the
three-class batch and the 600-graph batch report 9 and 10.  Every graph of every sharing batch has the bits it gets alone.

What a one-line change of evd.hip does to these tests, tried on scratch builds: the rank's tie-break `i < j` turned into `i > j` fails
test_a_graph_without_edges_comes_out_as_the_identity (the decomposition stays valid, only the order inside a tie changes, so nothing
else can notice).  Dropping `fminf(lo, hi) > athr` fails nothing, here or in a float32 emulation of all 62 runs: without the guard the
null-space columns, which hold rounding noise, are orthogonalised like any other column — the result stays inside the tolerance and
costs one or two more sweeps; the guard saves time, it does not decide correctness.  `step < mm1` turned into `step <= mm1` (emulated
per lane in numpy, not run on the device) lets a graph with m < mmax pair its last column with itself at step m - 1: harmless when n is
odd (that column is the zero padding column), garbage when n is even — edge2 in four_m_one_workgroup and three_classes, cycle24 in
m24_beside_m32, K8 in m8_beside_m16.

Run with -s for the figures of every graph."""
import functools

import numpy as np
import pytest
import torch

import evd_small_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 4e-6
ST_CROSS, ST_OVERSIZE, ST_NOCONV, ST_SPACE = 1, 2, 4, 8
SENTINEL = -123.0


def _gptr(sizes):
    return torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device=DEV)


def _dev(ei):
    return torch.from_numpy(np.ascontiguousarray(ei)).to(DEV)


def _raw(ei, sizes, norm=None, k=0, skip=1):
    """ops.laplacian_evd on a collated batch: (val, vec, evoff, pe, status)."""
    from signnet_basisnet_amd import ops
    return ops.laplacian_evd(_dev(ei), _gptr(sizes), sum(sizes), sum(n * n for n in sizes), norm, k, skip)


def _blocks(sizes):
    """(node offset, block offset, n) per graph."""
    out, off, o2 = [], 0, 0
    for n in sizes:
        out.append((off, o2, n))
        off += n
        o2 += n * n
    return out


@functools.lru_cache(maxsize=None)
def _ref(name, norm):
    """The float32 reference of a case of the table, computed once: (L, eigenvalues, eigenvectors).  Read only."""
    from oracle import evd as OE
    ei, n = C.case(name)
    L = OE.dense_laplacian(ei, n, norm)
    dr, vr = OE.evd_laplacian(ei, n, norm)
    for a in (L, dr, vr):
        a.setflags(write=False)
    return L, dr, vr


@functools.lru_cache(maxsize=None)
def _alone(name, norm):
    """A case as a batch of one graph, run once: (val, vec, status as a list)."""
    ei, n = C.case(name)
    val, vec, _, _, st = _raw(ei, [n], norm)
    return val, vec, st.tolist()


def _compare(label, n, norm, D, V, ref):
    from oracle import evd as OE
    L, dr, vr = ref
    r = OE.compare_decompositions(D, V.reshape(n, n), dr, vr, L, TOL)
    print(f"    {label} n={n} norm={norm}: " + " ".join(f"{k}={v:.2e}" for k, v in r.items() if k != "ok"))
    assert r["ok"], (label, n, norm, r)
    return r


def _check_cases(names, sizes, norm, val, vec):
    """Every graph of a batch made of table cases against its cached reference."""
    D, V = val.cpu().numpy(), vec.cpu().numpy()
    for nm, (off, o2, n) in zip(names, _blocks(sizes)):
        _compare(nm, n, norm, D[off:off + n], V[o2:o2 + n * n], _ref(nm, norm))


def _check_graphs(ei, sizes, norm, val, vec, verbose=True):
    """Every non-empty graph of an arbitrary collated batch against numpy's float32 eigh of its own Laplacian; worst figures."""
    from oracle import evd as OE
    D, V = val.cpu().numpy(), vec.cpu().numpy()
    worst = {}
    for g, (off, o2, n) in enumerate(_blocks(sizes)):
        if n == 0:
            continue
        sel = (ei[0] >= off) & (ei[0] < off + n)
        loc = ei[:, sel] - off
        L = OE.dense_laplacian(loc, n, norm)
        dr, vr = np.linalg.eigh(L)
        r = OE.compare_decompositions(D[off:off + n], V[o2:o2 + n * n].reshape(n, n), dr, vr, L, TOL)
        if verbose:
            print(f"    graph {g} n={n} norm={norm}: " + " ".join(f"{k}={v:.2e}" for k, v in r.items() if k != "ok"))
        assert r["ok"], (g, n, norm, r)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0), v)
    return worst


# ---- a. each case alone
@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_case_alone(name, norm):
    """Every case of the table as a batch of one graph: no status bit (NOCONV, CROSS, OVERSIZE, SPACE all clear), the decomposition
    against numpy's float32 eigh, and the wrapper returning the raw call's bits.  The sweep count is printed, not bounded: the
    kernel's own NOCONV flag is the bound."""
    from signnet_basisnet_amd import transform as T
    ei, n = C.case(name)
    val, vec, st = _alone(name, norm)
    assert st[0] == 0, st
    print(f"  {name} norm={norm} ({C.size_class(n)}, RW {C.rows_per_wave(n)}): sweeps {st[1]}")
    _check_cases([name], [n], norm, val, vec)
    D, V, _ = T.evd_laplacian_batch(_dev(ei), ptr=_gptr([n]), norm=norm)
    assert torch.equal(D, val) and torch.equal(V, vec)


@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("name", ["single1", "empty5", "empty64"])
def test_a_graph_without_edges_comes_out_as_the_identity(name, norm):
    """L = 0 (None) or L = I ('sym'): nothing rotates (athr = 0 under None), every Rayleigh quotient is the same number, and the rank's
    tie-break by column index keeps the columns where they are — eigenvalues exactly 0 / 1 and V exactly the identity, in one sweep."""
    _, n = C.case(name)
    val, vec, st = _alone(name, norm)
    assert st[0] == 0 and st[1] == 1, st
    assert torch.equal(val, torch.full((n,), 0.0 if norm is None else 1.0, device=DEV))
    assert torch.equal(vec.view(n, n), torch.eye(n, device=DEV))


# ---- b. forced-sharing batches
@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("batch", list(C.SHARING))
def test_sharing_batch(batch, norm):
    """Graphs of different m in one workgroup (and dead slots beside them): the same assertions per graph as alone."""
    from signnet_basisnet_amd import transform as T
    ei, sizes, names = C.sharing_batch(batch)
    val, vec, _, _, st = _raw(ei, sizes, norm)
    st = st.tolist()
    assert st[0] == 0, st
    print(f"  {batch} norm={norm}: largest sweep count {st[1]}")
    _check_cases(names, sizes, norm, val, vec)
    D, V, _ = T.evd_laplacian_batch(_dev(ei), ptr=_gptr(sizes), norm=norm)
    assert torch.equal(D, val) and torch.equal(V, vec)


# ---- c. neighbour independence
@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("batch", list(C.SHARING))
def test_result_does_not_depend_on_the_neighbours(batch, norm):
    """A graph's eigenvalues and eigenvectors inside a sharing batch are the SAME BITS it gets alone, although the workgroup then runs
    another RW, more steps per sweep and more sweeps.  Derived from the code — a graph's rotation sequence depends only on its own
    columns, steps beyond m - 1 are inactive, padding rows add exact zeros to every partial sum whatever RW, a graph that does not
    rotate beside one that does is updated with s = tau = 0, and sweeps forced by a neighbour rotate nothing — and it HOLDS on the
    device for every graph of every batch under both norms: no defect, no exception by design."""
    ei, sizes, names = C.sharing_batch(batch)
    val, vec, _, _, st = _raw(ei, sizes, norm)
    assert int(st[0]) == 0
    for nm, (off, o2, n) in zip(names, _blocks(sizes)):
        v1, w1, _ = _alone(nm, norm)
        assert torch.equal(val[off:off + n], v1), (batch, nm, norm, "eigenvalues")
        assert torch.equal(vec[o2:o2 + n * n], w1), (batch, nm, norm, "eigenvectors")


# ---- d. more than 256 graphs: the prefix scan's carry across 256-graph chunks
def _many_graphs():
    builders = (C.path, lambda n: C.cycle(n) if n >= 3 else C.path(n), C.complete, C.empty, C.star)
    graphs = []
    for i in range(600):
        n = i % 6 + 1
        graphs.append((builders[(i // 6) % len(builders)](n), n))
    for pos, nm in ((255, "K17"), (256, "K33"), (511, "cycle64")):       # the last of chunk 0, the first of chunk 1, the last of chunk 1
        graphs[pos] = C.case(nm)
    return C.collate(graphs)


@pytest.mark.parametrize("norm", C.NORMS)
def test_more_than_256_graphs(norm):
    ei, sizes = _many_graphs()
    assert len(sizes) == 600 and (sizes[255], sizes[256], sizes[511]) == (17, 33, 64)
    val, vec, evoff, _, st = _raw(ei, sizes, norm)
    st = st.tolist()
    assert st[0] == 0, st
    want = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64) ** 2)])
    got = evoff.cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, want)
    worst = _check_graphs(ei, sizes, norm, val, vec, verbose=False)
    print(f"  600 graphs norm={norm}: sweeps {st[1]} worst " + " ".join(f"{k}={v:.2e}" for k, v in worst.items() if k != "ok"))


# ---- e. empty graphs inside a batch
@pytest.mark.parametrize("norm", C.NORMS)
def test_empty_graphs_inside_a_batch(norm):
    """graph_ptr = [0, 3, 3, 8, 8, 8, 10]: the scatter's binary search must land on the non-empty graph among equal offsets."""
    sizes = [3, 0, 5, 0, 0, 2]
    ei = np.concatenate([C.path(3), C.cycle(5) + 3, C.path(2) + 8], 1)
    val, vec, evoff, _, st = _raw(ei, sizes, norm)
    st = st.tolist()
    assert st[0] == 0, st
    assert evoff.cpu().tolist() == [0, 9, 9, 34, 34, 34, 38]
    assert val.shape == (10,) and vec.shape == (38,)
    _check_graphs(ei, sizes, norm, val, vec)
    # the same three graphs without the empty ones between them: the same bits
    val2, vec2, _, _, _ = _raw(ei, [3, 5, 2], norm)
    assert torch.equal(val, val2) and torch.equal(vec, vec2)


# ---- f. edge-list hygiene
@pytest.mark.parametrize("norm", C.NORMS)
def test_self_loops_and_duplicate_edges_change_nothing(norm):
    """The mixed batch with self loops on several nodes of every kind of graph and every edge present twice and once reversed, shuffled:
    the same bits as the clean list (the scatter returns on s == d and coalesces by overwriting)."""
    ei, sizes, _ = C.sharing_batch("three_classes")
    N = sum(sizes)
    # K64 0 5 63, K17 64 80, cycle24 81, both nodes of edge2, cycle9 107, the hub of star16, a triangle node and the isolated node, cycle41
    loops = np.array([0, 5, 63, 64, 80, 81, 105, 106, 107, 116, 132, 138, N - 1], dtype=np.int64)
    assert loops.max() < N
    dirty = np.concatenate([ei, np.stack([loops, loops]), ei, ei[::-1], np.stack([loops[:3], loops[:3]])], 1)
    dirty = dirty[:, np.random.default_rng(0).permutation(dirty.shape[1])]
    a = _raw(ei, sizes, norm)
    b = _raw(dirty, sizes, norm)
    assert a[4].tolist()[0] == 0 and b[4].tolist()[0] == 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- g. positional-encoding layout at the small end
@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("k,skip", [(4, 1), (3, 0), (1, 1), (1, 0)])
def test_positional_encoding_wider_than_the_graph(k, skip, norm):
    """pe[:, c] is column c + skip of the graph's V block where that column exists and exactly zero elsewhere: with k = 4, skip = 1 a
    whole zero row for the one-node graph, three zero columns for the edge, two for the path."""
    from signnet_basisnet_amd import transform as T
    names = ["single1", "edge2", "path3", "cycle9"]
    ei, sizes = C.collate([C.case(nm) for nm in names])
    val, vec, _, pe, st = _raw(ei, sizes, norm, k, skip)
    assert int(st[0]) == 0 and pe.shape == (sum(sizes), k)
    val0, vec0, _, pe0, _ = _raw(ei, sizes, norm)
    assert pe0 is None and torch.equal(val, val0) and torch.equal(vec, vec0)         # asking for the encoding changes nothing else
    _check_cases(names, sizes, norm, val, vec)
    for off, o2, n in _blocks(sizes):
        blk = vec[o2:o2 + n * n].view(n, n)
        kk = max(0, min(k, n - skip))
        assert torch.equal(pe[off:off + n, :kk], blk[:, skip:skip + kk]), (n, k, skip)
        assert not bool(pe[off:off + n, kk:].any()), (n, k, skip)
    D, V, pe2 = T.evd_laplacian_batch(_dev(ei), ptr=_gptr(sizes), norm=norm, pos_enc_dim=k, skip=skip)
    assert torch.equal(pe2, pe) and torch.equal(D, val) and torch.equal(V, vec)
    if norm == "sym" and skip == 1:
        assert torch.equal(T.lap_positional_encoding_batch(_dev(ei), ptr=_gptr(sizes), pos_enc_dim=k), pe)


# ---- h. status words
@pytest.mark.parametrize("bad", [(-1, 2), (2, -1), (29, 0), (0, 29)])
def test_out_of_range_node_id_is_flagged_and_dropped(bad):
    """A node id of -1 or N in either row sets the CROSS bit and nothing else (k_evd_scatter checks 0 <= id < N before it uses the id);
    the edge is dropped, so every graph comes out with the bits of the clean list."""
    from signnet_basisnet_amd import transform as T
    names = ["path3", "cycle9", "K17"]
    ei, sizes = C.collate([C.case(nm) for nm in names])
    assert sum(sizes) == 29
    mid = ei.shape[1] // 2
    dirty = np.concatenate([ei[:, :mid], np.array([[bad[0]], [bad[1]]], dtype=np.int64), ei[:, mid:]], 1)
    val0, vec0, *_ = _raw(ei, sizes, "sym")
    val, vec, _, _, st = _raw(dirty, sizes, "sym")
    assert int(st[0]) == ST_CROSS, st.tolist()
    _check_cases(names, sizes, "sym", val, vec)
    assert torch.equal(val, val0) and torch.equal(vec, vec0)
    with pytest.raises(RuntimeError, match="out of range"):
        T.evd_laplacian_batch(_dev(dirty), ptr=_gptr(sizes), norm="sym")


@pytest.mark.parametrize("names", [["cycle9", "K17", "cycle41", "path3", "star16"], ["path3", "K17", "star16", "cycle41"]],
                         ids=["last_shares_a_workgroup", "last_has_its_own"])
def test_short_eigen_vectors_buffer(names):
    """`total` one float short of the last graph's block, through the C entry point on an allocation of total + 64 floats filled with a
    sentinel: the SPACE bit and nothing else; every graph whose block fits is decomposed; of the last graph's block only the clearing
    memset is seen (total - 1 floats: zeros, then the sentinel), its eigenvalues are not written, and the 64 floats behind stay."""
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    ei, sizes = C.collate([C.case(nm) for nm in names])
    B, N, total = len(sizes), sum(sizes), sum(n * n for n in sizes)
    eid, gp = _dev(ei), _gptr(sizes)
    val = torch.full((N,), SENTINEL, device=DEV)
    vec = torch.full((total + 64,), SENTINEL, device=DEV)
    evoff = torch.empty(B + 1, dtype=torch.int64, device=DEV)
    work = torch.empty(int(lib().sn_evd_work_ints(B)), dtype=torch.int32, device=DEV)
    status = torch.empty(4, dtype=torch.int32, device=DEV)
    check(lib().sn_laplacian_evd_f32(ptr(eid), ei.shape[1], ptr(gp), B, N, 0, ptr(evoff), ptr(val), ptr(vec), total - 1, None, 0, 1,
                                     ptr(work), ptr(status), stream()), "sn_laplacian_evd_f32")
    assert int(status[0]) == ST_SPACE, status.tolist()
    assert evoff.cpu().tolist() == np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64) ** 2)]).tolist()
    last = sizes[-1]
    _check_cases(names[:-1], sizes[:-1], None, val[:N - last], vec[:total - last * last])
    blk = vec[total - last * last:total]
    assert not bool(blk[:-1].any()) and float(blk[-1]) == SENTINEL
    assert bool((val[N - last:] == SENTINEL).all())
    assert bool((vec[total:] == SENTINEL).all())
    # and with the right `total` the same buffers hold the same bits for the graphs that fitted before
    val1, vec1 = val.clone(), vec.clone()
    check(lib().sn_laplacian_evd_f32(ptr(eid), ei.shape[1], ptr(gp), B, N, 0, ptr(evoff), ptr(val), ptr(vec), total, None, 0, 1,
                                     ptr(work), ptr(status), stream()), "sn_laplacian_evd_f32")
    assert int(status[0]) == 0
    assert torch.equal(val[:N - last], val1[:N - last]) and torch.equal(vec[:total - last * last], vec1[:total - last * last])
    _check_cases(names, sizes, None, val, vec[:total])
    assert bool((vec[total:] == SENTINEL).all())
