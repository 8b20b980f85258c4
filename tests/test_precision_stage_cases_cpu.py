"""No GPU: the conditions under which the reduced-precision stage grid (tests/test_precision_stage_grid_gpu.py) can tell a right `high` /
`medium` stage kernel from a wrong one, checked on every row of tests/precision_stage_cases.py.

  coverage   every reduced instance of phi (12), rho (22) and the DGL pair is reached by some row, and each row's branch string is the
             restated dispatch on its actual batch
  folding    emulated_dgl_oracle(folded=True) restates the BatchNorm folding of dgl_deepsigns._FusedDeepSigns: with plain float64
             products on the unrounded W' it is the float64 oracle to 1e-12
  the rule   the float32 emulation (same planes, same products, float32 arithmetic) in the part of the GPU satisfies
             R(emu32_m, emu64_m) <= gap_m / 8 per row, stage, reduced mode, for the whole tensor, for every graph and (SignNetGNN) for
             every 16-channel tile — half of what the GPU test allows a kernel, so the rule is never decided by fp32 arithmetic as such
"""
import pytest
import torch

import precision_stage_cases as PC
import stage_cases as SC
from signnet_basisnet_amd import fused


def ids(cases):
    return [c.id for c in cases]


def test_ids_are_unique_and_salts_name_rows():
    i = ids(PC.PYG + PC.DGL)
    assert len(i) == len(set(i))
    assert set(PC.SALT) <= set(i), sorted(set(PC.SALT) - set(i))
    assert all(c.p.get("salt", 0) == PC.SALT.get(c.id, c.p.get("salt", 0)) for c in PC.PYG + PC.DGL)


@pytest.mark.parametrize("case", PC.PYG + PC.DGL, ids=ids(PC.PYG + PC.DGL))
def test_row_takes_the_branch_it_names(case):
    if case.op == "pyg":
        assert SC.pyg_branch(case.p) == case.branch and PC.stage_branch(case) == " | ".join(case.branch.split(" | ")[:2])
        assert SC.cdiv(case.p["hid"], 16) in fused.REDUCED_TILES
    else:
        assert SC.dgl_branch(case.p) == case.branch and SC.dgl_widths(case.p)[0] // 16 in fused.REDUCED_TILES_DGL


def test_rows_reach_every_reduced_instance():
    assert len(PC.PHI_BRANCHES) == 12 and len(PC.RHO_BRANCHES) == 22
    assert PC.PHI_BRANCHES <= SC.PHI_BRANCHES and PC.RHO_BRANCHES <= SC.RHO_BRANCHES and not (PC.RHO_BRANCHES & SC.UNREACHABLE)
    phi, rho = {SC.phi_branch(c.p) for c in PC.PYG}, {SC.rho_branch(c.p) for c in PC.PYG}
    assert phi == PC.PHI_BRANCHES, f"not reached {sorted(PC.PHI_BRANCHES - phi)}, not declared {sorted(phi - PC.PHI_BRANCHES)}"
    assert rho == PC.RHO_BRANCHES, f"not reached {sorted(PC.RHO_BRANCHES - rho)}, not declared {sorted(rho - PC.RHO_BRANCHES)}"
    pairs = [PC.stage_branch(c) for c in PC.PYG]
    assert len(pairs) == len(set(pairs)), "one row per (phi, rho) pair: the GINE stage stays at highest and is no reason for a row"
    seen = SC.branches_of(PC.DGL)
    assert seen == PC.DGL_BRANCHES, f"not reached {sorted(PC.DGL_BRANCHES - seen)}, not declared {sorted(seen - PC.DGL_BRANCHES)}"
    assert PC.DGL_BRANCHES == ({f"k_phi_fused<{nt},!HID1,DGL>" for nt in (4, 5, 6)} | {f"k_mlp_chain<{nt}>" for nt in (4, 5, 6, 7, 8)} |
                               {f"k_mlp_chain<{nt}> masked" for nt in (4, 5, 6)})
    # every stage_cases row at a reduced tile count takes a (phi, rho) pair some row here has: nothing was dropped but GINE variety
    for c in SC.PYG:
        if SC.cdiv(c.p["hid"], 16) in fused.REDUCED_TILES:
            assert " | ".join(c.branch.split(" | ")[:2]) in pairs, c.id


def test_refused_widths_are_the_tile_counts_without_reduced_kernels():
    tiles = {SC.cdiv(h, 16) for h in PC.REFUSED_HIDDEN}
    assert tiles | set(fused.REDUCED_TILES) == set(range(1, 9)) and not (tiles & set(fused.REDUCED_TILES))
    widths = {SC.dgl_widths(dict(kind="gin", hidden=h, out=4, K=8, layers=2))[0] for h in PC.REFUSED_DGL_HIDDEN}
    assert widths == {48, 112} and not ({w // 16 for w in widths} & set(fused.REDUCED_TILES_DGL))


@pytest.mark.parametrize("case", PC.DGL, ids=ids(PC.DGL))
def test_dgl_folding_is_algebra(case):
    y64 = SC.dgl_reference(case)[3]
    y = PC.dgl_folding_alone(case)
    assert y.dtype == torch.float64 and y.shape == y64.shape
    err = (y - y64).abs().max().item() / y64.abs().max().item()
    assert err <= 1e-12, f"{case.id}: folded restatement vs float64 oracle {err:.2e}"


def _hold(case, stage, mode, whole, worst, g):
    print(f"\n{case.id} [{PC.stage_branch(case) if case.op == 'pyg' else case.branch}] {mode} {stage}: R(emu32, emu64) / gap whole {whole:.4f}, "
          f"worst graph {worst:.4f} (graph {g}, {case.p['sizes'][g]} nodes); allowed {1 / PC.CPU_FACTOR}", end="")
    assert whole <= 1 / PC.CPU_FACTOR, f"{case.id} {mode} {stage}: the float32 emulation is {whole:.4f} of the mode gap (whole tensor)"
    assert worst <= 1 / PC.CPU_FACTOR, f"{case.id} {mode} {stage}: the float32 emulation is {worst:.4f} of the mode gap on graph {g}"


@pytest.mark.parametrize("case", PC.PYG, ids=ids(PC.PYG))
def test_float32_emulation_is_within_an_eighth_of_the_mode_gap(case):
    mask = SC.reference(case)[3]
    e64, e32 = PC.emulations(case), PC.emulations32(case)
    for mode in PC.REDUCED:
        for stage in ("phi", "rho_sum"):
            assert e32[mode][stage].dtype == torch.float32 and e64[mode][stage].dtype == torch.float64
            m = mask if stage == "phi" else None
            _hold(case, stage, mode, *PC.rule_ratios(e32[mode][stage], e64, mode, stage, case.p["sizes"], m))
            tile, t = PC.tile_ratios(e32[mode][stage], e64, mode, stage, m)
            print(f"; worst 16-channel tile {tile:.4f} (tile {t})", end="")
            assert tile <= 1 / PC.CPU_FACTOR, f"{case.id} {mode} {stage}: the float32 emulation is {tile:.4f} of the mode gap in channel tile {t}"


@pytest.mark.parametrize("case", PC.DGL, ids=ids(PC.DGL))
def test_float32_dgl_emulation_is_within_an_eighth_of_the_mode_gap(case):
    e64, e32 = PC.dgl_emulations(case), PC.dgl_emulations32(case)
    for mode in PC.REDUCED:
        assert e32[mode].dtype == torch.float32 and e64[mode].dtype == torch.float64
        _hold(case, "y", mode, *PC.rule_ratios(e32[mode], e64, mode, "y", case.p["sizes"]))


def test_the_rule_counts_a_neighbouring_mode_as_wrong():
    """fed the neighbouring mode's emulation, the rule's ratio is >= 1 by construction: four times the allowed"""
    case = PC.PYG[0]
    e64 = PC.emulations(case)
    for mode in PC.REDUCED:
        for n in PC.NEIGHBOURS[mode]:
            whole, worst, _ = PC.rule_ratios(e64[n]["rho_sum"], e64, mode, "rho_sum", case.p["sizes"])
            assert whole >= 1.0 and worst >= 1.0
