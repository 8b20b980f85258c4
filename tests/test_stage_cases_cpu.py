"""No GPU: the conditions under which the stage grid (tests/test_stage_grid_gpu.py) can tell a right stage kernel from a wrong one, checked
on every row of tests/stage_cases.py.

  branch        the restated dispatch, evaluated on the row's actual batch (graph sizes, slot count, edge and edge-class counts), returns
                the row's `branch`; the rows reach every name of the branch sets, and no name listed as unreachable
  coverage      the widths, slot counts, layer counts and batches the grid was written for are in the tables
  conditioning  per row and stage the float32 oracle is within parity_util.REL of the float64 oracle under `close` and under
                `elementwise`, so the GPU rule is never decided by the reference's own error
  cost          both oracle passes of a row take under two seconds
"""
import time

import pytest
import torch

import parity_util as PU
import stage_cases as SC


def ids(cases):
    return [c.id for c in cases]


def test_ids_are_unique():
    i = ids(SC.ALL)
    assert len(i) == len(set(i)), sorted(x for x in i if i.count(x) > 1)


@pytest.mark.parametrize("case", SC.ALL, ids=ids(SC.ALL))
def test_row_takes_the_branch_it_names(case):
    assert (SC.pyg_branch if case.op == "pyg" else SC.dgl_branch)(case.p) == case.branch


def test_rows_cover_every_reachable_branch_and_no_unreachable_one():
    seen = SC.branches_of(SC.PYG)
    assert seen == SC.PYG_BRANCHES, f"not reached {sorted(SC.PYG_BRANCHES - seen)}, not declared {sorted(seen - SC.PYG_BRANCHES)}"
    assert not (seen & SC.UNREACHABLE) and not (SC.PYG_BRANCHES & SC.UNREACHABLE)
    seen = SC.branches_of(SC.DGL)
    assert seen == SC.DGL_BRANCHES, f"not reached {sorted(SC.DGL_BRANCHES - seen)}, not declared {sorted(seen - SC.DGL_BRANCHES)}"


def test_unreachable_names_are_the_natural_register_attention_at_the_other_six_tile_counts():
    """dispatch_rho<true, ONE>(nt) exists for nt 1..8; natural register attention needs d / 4 heads to be a multiple of 16: d = 64, 128"""
    assert SC.UNREACHABLE == {f"k_rho_fused<{nt},reg,{o}>" for nt in (1, 2, 3, 5, 6, 7) for o in ("ONE", "!ONE")}
    for d in range(4, 129, 4):
        for k in (1, 16):
            p = dict(variant="gine", hid=d, max_k=k, nl_rho=1, sizes=(20,))
            name = SC.rho_branch(p)
            assert (name in SC.UNREACHABLE) is False and (("HP" in name) == (d not in (64, 128)))


def test_named_branches_are_all_in_the_tables():
    """the list the grid was written for, spelled out"""
    seen = SC.branches_of(SC.ALL)
    want = {"k_rho_fused<4,reg,ONE,HP16>", "k_rho_fused<8,reg,!ONE,HP32>", "k_rho_wide<8,!ONE,COLS>", "k_rho_wide<4,ONE,!COLS>",
            "k_phi_fused<6,HID1> columns", "k_phi_fused<5,!HID1> slabs", "k_phi_fused<1,HID1> slabs", "k_rho_fused<5,lds,ONE>",
            "k_rho_fused<6,lds,!ONE>", "k_rho_fused<4,lds,ONE>", "k_rho_fused<8,lds,!ONE>", "gnn<8> T=3 use_ee", "gnn<8> T=1 gather",
            "gnn<5> use_tab", "gnn<6> gather", "gnn<4> no layers", "k_phi_fused<3,!HID1,DGL>", "k_phi_fused<7,!HID1,DGL>", "k_mlp_chain<8>",
            "k_mlp_chain<3> masked"}
    assert want <= seen, sorted(want - seen)


def rows(**kw):
    return [c for c in SC.PYG if all(c.p[k] == v for k, v in kw.items())]


def test_the_tables_hold_the_shapes_the_grid_was_written_for():
    default = dict(sizes=SC.DEFAULT_SIZES, keep_edges=None, complete=False)
    assert SC.DEFAULT_SIZES == (64, 1, 17, 33, 16, 5, 48, 2, 32, 49)
    # phi: widths x variants x columns (7, 16) / slabs, 2 layers; one row with 8
    for variant in ("gine", "alchemy"):
        for hid in (4, 16, 20, 32, 48, 64, 80, 96, 108, 112, 128):
            for k in (7, 16, None):
                assert rows(variant=variant, hid=hid, max_k=k, nl_phi=2, nl_gnn=2, **default), (variant, hid, k)
    assert rows(nl_phi=8)
    # rho: every register-attention width with ONE, !ONE from two layers without an encoder and !ONE from the eigenvalue encoder
    for hid in SC.RHO_HP16 + SC.RHO_HP32 + SC.RHO_NATURAL:
        for kw in (dict(variant="gine", nl_rho=1), dict(variant="gine", nl_rho=2), dict(variant="alchemy")):
            assert [c for c in rows(hid=hid, **kw, **default) if c.p["max_k"] in (7, 16)], (hid, kw)
    assert (SC.RHO_HP16, SC.RHO_HP32, SC.RHO_NATURAL) == ((4, 20, 48, 60), (68, 80, 96, 112, 124), (64, 128))
    for hid in (20, 32, 48, 60, 80, 96, 108, 124):          # LDS attention with more than 16 slots at every tile count
        for variant in ("gine", "alchemy"):
            assert rows(variant=variant, hid=hid, max_k=None, **default), (variant, hid)
    for hid in (80, 64):                                    # the 16 / 17 boundary
        for variant in ("gine", "alchemy"):
            assert rows(variant=variant, hid=hid, max_k=16, **default) and rows(variant=variant, hid=hid, max_k=17, **default)
            assert rows(variant=variant, hid=hid, max_k=None, sizes=SC.MAX16) and rows(variant=variant, hid=hid, max_k=None, sizes=SC.MAX17)
    assert max(SC.MAX16) == 16 and max(SC.MAX17) == 17
    # GINE: one graph per row-tile form at 128, both feature kinds, layer counts 0 / many, n_out 12 (the alchemy rows)
    assert {c.p["sizes"] for c in rows(variant="gine", hid=128) if len(c.p["sizes"]) == 1} == {(n,) for n in (16, 17, 32, 33, 48, 49, 64)}
    assert rows(nl_gnn=0) and rows(variant="gine", hid=128, nl_gnn=14, **default)
    assert 14 * 3 > SC.gnn_ee_rows(8, 1) >= 13 * 3          # the fewest layers at which three bond classes leave the class table
    for hid in (128, 96):                                   # a continuous-feature graph with ee_rows and with ee_rows + 1 in-edges
        c, = rows(variant="alchemy", hid=hid, keep_edges=SC.ee_batch(hid)[1])
        R = SC.gnn_ee_rows(SC.cdiv(hid, 16), 4)
        stats = SC.graph_edge_stats(SC.batch_of(c))
        assert stats[0] == (R, R) and stats[1] == (R + 1, R + 1) and R + 1 <= SC.GNN_EMAX
    # DGL: both nets at every padded width with K = 1, 8, 37, 64
    assert sorted(set(SC.DGL_HIDDEN.values())) == [48, 64, 80, 96, 112]
    for kind in ("gin", "masked_gin"):
        assert {(SC.dgl_widths(c.p)[0], c.p["K"]) for c in SC.DGL if c.p["kind"] == kind} == {(w, K) for w in (48, 64, 80, 96, 112) for K in SC.DGL_K}


def test_restated_ee_rows():
    """csrc/gnn_front.hpp gnn_ee_rows at the widths and edge-word counts of the tables (capped at GNN_EEMAX = 96 rows)"""
    assert [SC.gnn_ee_rows(nt, 1) for nt in range(1, 9)] == [96, 96, 96, 96, 96, 72, 53, 39]
    assert [SC.gnn_ee_rows(nt, 4) for nt in range(1, 9)] == [96, 96, 96, 96, 92, 66, 48, 34]


def test_reordered_batch_is_the_same_graphs():
    case = SC.PYG[0]
    data = SC.batch_of(case)
    order = list(range(len(data.sizes)))[::-1]
    rev, perm = SC.reorder(data, order)
    back, perm2 = SC.reorder(rev, order)
    assert torch.equal(perm[perm2], torch.arange(perm.numel()))
    for k in ("x", "batch", "eigen_values", "eigen_vectors", "edge_index", "edge_attr"):
        assert torch.equal(getattr(back, k), getattr(data, k)), k
    assert rev.sizes == list(data.sizes)[::-1] and SC.graph_edge_stats(rev) == SC.graph_edge_stats(data)[::-1]


def within_rel(case, what, a32, a64):
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and a32.shape == a64.shape
    assert bool(torch.isfinite(a64).all()) and a64.abs().max().item() > 0, f"{case.id} {what}"
    PU.close(a32, a64, f"{case.id} {what}: float32 oracle vs float64")
    PU.elementwise(a32, a64, f"{case.id} {what}: float32 oracle vs float64, element-wise")


@pytest.mark.parametrize("case", SC.PYG, ids=ids(SC.PYG))
def test_float32_oracle_is_within_rel_of_float64_and_quick(case):
    t0 = time.perf_counter()
    sd, o32, o64, mask = SC.reference(case)
    dt = time.perf_counter() - t0
    assert dt < 2.0, f"{case.id}: both oracle passes took {dt:.2f} s"
    p = case.p
    N, K = sum(p["sizes"]), SC.slot_count(p)
    assert mask.shape == (N, K) and o32["phi"].shape == (N, K, p["hid"]) and o32["rho_sum"].shape == (N, p["hid"])
    assert o32["y"].shape == (len(p["sizes"]), 1 if p["variant"] == "gine" else 12)
    assert not bool(o64["phi"][~mask].any()), "the oracle leaves invalid slots at zero"
    within_rel(case, "phi (valid slots)", o32["phi"][mask], o64["phi"][mask])
    within_rel(case, "rho_sum", o32["rho_sum"], o64["rho_sum"])
    within_rel(case, "y", o32["y"], o64["y"])


@pytest.mark.parametrize("case", SC.DGL, ids=ids(SC.DGL))
def test_float32_dgl_oracle_is_within_rel_of_float64_and_quick(case):
    t0 = time.perf_counter()
    sd, x, y32, y64 = SC.dgl_reference(case)
    dt = time.perf_counter() - t0
    assert dt < 2.0, f"{case.id}: both oracle passes took {dt:.2f} s"
    assert x.shape == (sum(case.p["sizes"]), case.p["K"], 1) and y32.shape == x.shape
    within_rel(case, "y", y32, y64)


@pytest.mark.parametrize("stage", ["phi", "rho_sum", "y"])
def test_the_elementwise_rule_sees_one_wrong_entry_the_max_norm_rule_lets_through(stage):
    """why the grid asserts both rules: an error of 0.9e-5 of the tensor's largest entry in one small entry (a wrong channel of one rho
    head, one bad slot row of phi) passes `attributed` and fails `elementwise`"""
    case = next(c for c in SC.PYG if c.name == "gine-h80-k16-rho1")
    sd, o32, o64, mask = SC.reference(case)
    r32, r64 = (o32[stage][mask], o64[stage][mask]) if stage == "phi" else (o32[stage], o64[stage])
    bad = r32.clone().view(-1)
    i = int(r64.abs().view(-1).argmin())
    bad[i] += 0.9e-5 * r64.abs().max().item()
    bad = bad.view(r32.shape)
    PU.attributed(bad, r32, r64, f"{stage}: one entry off by 0.9e-5 of the largest")
    with pytest.raises(AssertionError, match="farther from the float64 value"):
        PU.elementwise(bad, r32, stage, ref64=r64)
