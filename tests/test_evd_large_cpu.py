"""CPU: the entry points of the mid-size (65 .. 128 nodes) eigendecomposition are declared, exported and bound; they validate their
arguments on the host; and a float32 emulation of the method (tests/evd_emulation.py) reaches the project's EVD tolerance at these
sizes (the tolerance tests/test_evd_large_gpu.py holds the kernel to)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sn_laplacian_evd_large_f32", "sn_evd_large_max_nodes", "sn_evd_large_work_ints")
TOL = 4e-6          # tests/test_evd_gpu.py


@pytest.fixture(scope="module")
def lib():
    from signnet_basisnet_amd import build
    build.build()
    from signnet_basisnet_amd import _lib
    return _lib.lib()


def test_entry_points_are_declared_exported_and_bound(lib):
    from signnet_basisnet_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "signnet_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in signnet_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
    assert len(_lib.SIGNATURES["sn_laplacian_evd_large_f32"]) == len(_lib.SIGNATURES["sn_laplacian_evd_f32"]) == 16
    assert lib.sn_evd_large_max_nodes() == 128 == ops.EVD_LARGE_MAX_NODES
    assert lib.sn_evd_large_work_ints(128) >= 128 + 1            # the list of mid-size graphs and its length
    assert lib.sn_evd_large_work_ints(1 << 33) > (1 << 33)       # an int64 result


def test_null_pointer_call_is_rejected_on_the_host(lib):
    rc = lib.sn_laplacian_evd_large_f32(None, 0, None, 0, 0, 0, None, None, None, 0, None, 0, 0, None, None, None)
    assert rc == -1 and b"sn_laplacian_evd_large_f32" in lib.sn_last_error()
    # the 64-node entry point's message is its own
    rc = lib.sn_laplacian_evd_f32(None, 0, None, 0, 0, 0, None, None, None, 0, None, 0, 0, None, None, None)
    assert rc == -1 and b"sn_laplacian_evd_f32" in lib.sn_last_error() and b"large" not in lib.sn_last_error()


@pytest.mark.parametrize("name", ["molecule70", "cycle128", "star128", "two_paths_60_68"])
@pytest.mark.parametrize("norm", [None, "sym"])
def test_float32_emulation_of_the_method_reaches_the_tolerance(name, norm):
    import evd_emulation as EM
    import evd_large_cases as C
    from oracle import evd as OE
    ei, n = next((e, n) for nm, e, n in C.cases() if nm == name)
    L = OE.dense_laplacian(ei, n, norm)
    D, V, sweeps = EM.jacobi(L)
    dr, vr = np.linalg.eigh(L)
    r = OE.compare_decompositions(D, V, dr, vr, L, TOL)
    assert r["ok"] and sweeps < 20, (name, norm, sweeps, r)
