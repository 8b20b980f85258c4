"""CPU: the case table of the 64-node eigendecomposition kernel (tests/evd_small_cases.py) reaches every row-count instantiation of
csrc/evd.hip's dispatch on both sides of its thresholds; a float32 emulation of the method (tests/evd_emulation.py) reaches the
project's EVD tolerance on every case within the kernel's own sweep cap; and no decision of the comparison
(oracle.evd.compare_decompositions) sits on its cluster threshold for any case."""
import os
import re

import numpy as np
import pytest

import evd_small_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 4e-6              # tests/test_evd_gpu.py: the project's EVD tolerance
MAX_SWEEPS = 16         # EVD_MAX_SWEEPS of csrc/evd.hip
CLUSTER_SEP = 1e-3      # oracle.evd.compare_decompositions cuts the spectrum into clusters at gaps above this
CLUSTER_MARGIN = 2e-5   # no gap of a case's float64 spectrum lies this close to the cut


def test_the_table_is_the_list_of_names():
    cases = C.cases()
    assert [nm for nm, _, _ in cases] == C.CASE_NAMES and len(set(C.CASE_NAMES)) == len(C.CASE_NAMES) == 31
    for nm, ei, n in cases:
        assert ei.dtype == np.int64 and ei.shape[0] == 2 and 1 <= n <= 64, nm
        assert ei.size == 0 or (0 <= ei.min() and ei.max() < n), nm
        assert not (ei[0] == ei[1]).any(), nm
        key = ei.min(0) * n + ei.max(0)
        assert len(np.unique(key)) == ei.shape[1], nm           # a clean list: one entry per undirected edge


def test_restated_constants_are_the_kernel_s():
    src = open(os.path.join(ROOT, "signnet_basisnet_amd", "csrc", "evd.hip")).read()
    assert re.search(r"constexpr int EVD_MAX_SWEEPS = %d;" % MAX_SWEEPS, src)
    assert re.search(r"constexpr int EVD_WV = %d;" % C.WAVES, src)
    assert "n <= 16 ? 0 : (n <= 32 ? 1 : 2)" in src
    for bound, rw in ((14, 16), (12, 14), (10, 12), (8, 10), (6, 8), (4, 6), (2, 4)):
        assert re.search(r"if \(rows > %d\) return evd_jacobi_rows<NR, WV, %d>" % (bound, rw), src), (bound, rw)


def test_dispatch_restatement_over_every_size():
    want = {}
    for lo, hi, inst in ((1, 8, (16, 2)), (9, 16, (16, 4)), (17, 24, (32, 6)), (25, 32, (32, 8)), (33, 40, (64, 10)), (41, 48, (64, 12)),
                         (49, 56, (64, 14)), (57, 64, (64, 16))):
        assert C.LOWER_BOUND[inst] == lo
        for n in range(lo, hi + 1):
            want[n] = inst
    for n in range(1, 65):
        assert (C.size_class(n), C.rows_per_wave(n)) == want[n], n
        # the live rows cover the padded graph: 4 waves x RW rows >= m = n rounded up to even
        assert C.WAVES * C.rows_per_wave(n) >= ((n + 1) & ~1)


@pytest.mark.parametrize("inst", C.INSTANTIATIONS)
def test_every_instantiation_is_named_by_the_table(inst):
    hit = [(nm, n) for nm, _, n in C.cases() if (C.size_class(n), C.rows_per_wave(n)) == inst]
    assert len(hit) >= 2, (inst, hit)
    assert any(n == C.LOWER_BOUND[inst] for _, n in hit), (inst, hit)         # a graph at the instantiation's lower size bound
    assert any(n & 1 for _, n in hit), (inst, hit)                            # an odd n: a padding column


def test_every_threshold_has_a_graph_on_each_side():
    sizes = {n for _, _, n in C.cases()}
    for below in (8, 16, 24, 32, 40, 48, 56):
        assert below in sizes and below + 1 in sizes, below
    assert 64 in sizes and 1 in sizes and 2 in sizes


@pytest.mark.parametrize("name", list(C.SHARING))
def test_sharing_batches_reach_what_they_claim(name):
    names, claim = C.SHARING[name]
    sizes = [C.case(nm)[1] for nm in names]
    by_class = {}
    for n in sizes:
        by_class.setdefault(C.size_class(n), []).append(n)
    # one workgroup per class whatever the listing order: at most 4 class-16 and 2 class-32 graphs
    assert len(by_class.get(16, [])) <= 4 and len(by_class.get(32, [])) <= 2
    assert set(by_class) == set(claim)
    for cls, ns in by_class.items():
        if cls == 64:
            continue
        assert C.instantiation(ns) == claim[cls], (name, cls, ns)
    _, coll_sizes, _ = C.sharing_batch(name)
    assert coll_sizes == sizes
    if name == "four_m_one_workgroup":
        assert sorted((n + 1) & ~1 for n in sizes) == [2, 2, 10, 16] and len(sizes) == 4
    if name == "dead_fourth_slot":
        assert len(sizes) == 3
    if name == "m18_beside_m32":
        assert [(n + 1) & ~1 for n in sizes] == [18, 32]
    if name == "three_classes":
        assert {(C.size_class(n), C.rows_per_wave(n)) for n in by_class[64]} == {(64, 16), (64, 12)}


@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_float32_emulation_reaches_the_tolerance_within_the_sweep_cap(name, norm):
    import evd_emulation as EM
    from oracle import evd as OE
    ei, n = C.case(name)
    L = OE.dense_laplacian(ei, n, norm)
    D, V, sweeps = EM.jacobi(L, max_sweeps=MAX_SWEEPS)
    dr, vr = np.linalg.eigh(L)
    r = OE.compare_decompositions(D, V, dr, vr, L, TOL)
    print(f"  {name} norm={norm}: sweeps {sweeps} " + " ".join(f"{k}={v:.2e}" for k, v in r.items() if k != "ok"))
    assert r["ok"], (name, norm, sweeps, r)
    assert sweeps < MAX_SWEEPS, (name, norm, sweeps)             # stopped on its own: a sweep that rotated nothing


@pytest.mark.parametrize("norm", C.NORMS)
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_no_cluster_decision_sits_on_its_threshold(name, norm):
    from oracle import evd as OE
    ei, n = C.case(name)
    w = np.linalg.eigvalsh(OE.dense_laplacian(ei, n, norm, np.float64))
    gaps = np.diff(w)
    near = np.abs(gaps - CLUSTER_SEP) <= CLUSTER_MARGIN
    assert not near.any(), (name, norm, gaps[near])
    # and the float32 reference cuts the spectrum where float64 does
    w32 = np.linalg.eigvalsh(OE.dense_laplacian(ei, n, norm))
    assert OE.clusters(w32, CLUSTER_SEP) == OE.clusters(w, CLUSTER_SEP), (name, norm)
