"""No GPU: the conditions under which the BasisNet grid (tests/test_basisnet_grid_gpu.py) can tell a right kernel from a wrong one, checked
on every row of every table of tests/basisnet_cases.py.

  branch        the host restatement of the dispatch returns the row's `branch`, and the rows of an op reach every branch its predicate
                can return
  conditioning  the reference's own float32 arithmetic is within parity_util.REL of float64 for every compared tensor (the contraction
                ops: every output column on its own) — a row where it is not cannot separate a right kernel from a wrong one at 1e-5
  references    the integer grouping and the IGN head restatements equal the oracle's (oracle/basisnet.py), which restates the reference
                project's statements
"""
import pytest
import torch

import basisnet_cases as BC
import parity_util as PU


def ids(cases):
    return [c.id for c in cases]


def test_ids_are_unique():
    i = ids(BC.ALL + BC.IGN_MLP_UNSUPPORTED + [BC.DEEPSETS_OVER_LIMIT])
    assert len(i) == len(set(i)), sorted(x for x in i if i.count(x) > 1)


@pytest.mark.parametrize("case", BC.ALL, ids=ids(BC.ALL))
def test_row_takes_the_branch_it_names(case):
    assert BC.OPS[case.op].predicate(case.p) == case.branch


@pytest.mark.parametrize("name", sorted(BC.OPS))
def test_rows_cover_every_branch(name):
    op = BC.OPS[name]
    seen = BC.branches_of(op.cases)
    assert seen == op.branches, f"{name}: not reached {sorted(op.branches - seen)}, not declared {sorted(seen - op.branches)}"


def test_named_branches_are_all_in_the_tables():
    """the list the grid was written for"""
    seen = BC.branches_of(BC.ALL)
    want = ({f"{k}, {pn}, strip {s}" for k in ("scalar", "v4") for pn in ("1 panel", "2 panels") for s in (64, 128)} |
            {"scalar (misaligned X)"} |
            {"proj_pass<2>", "proj_pass<4>", "proj_pass<8>", "proj_pass<32>", "2 passes", "3 passes", "ldv > N"} |
            {f"k_ign_mlp<{H},{T}>" for H in (16, 32) for T in (1, 2, 4, 8)} |
            {f"split0 = {s}, use_bn = {u}" for s in (0, 1) for u in (0, 1)} |
            {"run spans >= 3 chunks", "run starts at t * per", "all distinct", "all equal", "N = 1", "edge values", "decimals 0", "decimals 7"})
    assert want <= seen, sorted(want - seen)


def test_the_tables_hold_the_sizes_the_grid_was_written_for():
    assert {(c.p["b"], c.p["n"]) for c in BC.CONTRACT} >= {(3, 1), (2, 4), (3, 37), (2, 64), (2, 65), (1, 1027), (1, 1028), (64, 512), (52, 513), (2, 100)}
    assert {sum(c.p["mults"]) for c in BC.GROUP if c.p["values"] is None} >= {1, 5, 255, 256, 257, 300, 8192}
    assert {sum(c.p["mults"]) for c in BC.PROJECTORS} == {70, 200, 300}
    assert BC.PROJECTOR_MULTS <= {m for c in BC.PROJECTORS for m in c.p["mults"]}
    assert {c.p["n"] for c in BC.IGN_MLP} == BC.IGN_MLP_N and {c.p["O"] for c in BC.IGN_MLP} == BC.IGN_MLP_O
    assert {c.p["b"] for c in BC.IGN_MLP} == {1, 3} and any(c.p.get("no_fc2_bias") for c in BC.IGN_MLP)
    for H in (16, 32):          # every hidden width sees one output tile, a second tile with lanes past O, and two full tiles
        Os = {c.p["O"] for c in BC.IGN_MLP if c.p["H"] == H}
        assert any(o <= 16 for o in Os) and any(17 <= o <= 31 for o in Os) and 32 in Os
    assert {(c.p["n"], c.p["H"], c.p["O"]) for c in BC.IGN_MLP_UNSUPPORTED} == {(1025, 16, 2), (20, 8, 3), (20, 64, 3), (20, 16, 33)}
    assert all(c.branch == "not supported" for c in BC.IGN_MLP_UNSUPPORTED)
    assert {c.p["n"] for c in BC.DEEPSETS} == {1, 31, 32, 33, 1023, 1024, 512}
    assert {len(c.p["widths"]) for c in BC.DEEPSETS} >= {2, BC.DS_MAX_LAYERS}
    assert {1, 10, 31, 32} <= {w for c in BC.DEEPSETS for w in c.p["widths"]}
    ws = [c.p["widths"] for c in BC.DEEPSETS]
    assert any(w == sorted(w) and len(set(w)) == len(w) and len(w) > 2 for w in ws)                      # growing
    assert any(w[:-1] == sorted(w[:-1], reverse=True) and len(set(w[:-1])) == len(w) - 1 and len(w) > 3 for w in ws)      # shrinking
    assert any(w[-1] > max(w[:-1]) and c.p["n"] * w[-1] > BC.DS_BUF for c, w in zip(BC.DEEPSETS, ws))    # last layer wider than the LDS-resident ones
    assert any(c.p["n"] * max(c.p["widths"][:-1]) == BC.DS_BUF and c.p["n"] == 512 and max(c.p["widths"]) == 32 for c in BC.DEEPSETS)
    o = BC.DEEPSETS_OVER_LIMIT
    assert o.branch == "not supported" and (o.p["n"], max(o.p["widths"])) == (513, 32)


def within_rel(case, what, a32, a64):
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and a32.shape == a64.shape
    assert bool(torch.isfinite(a64).all())
    scale = a64.abs().max().item()
    assert scale > 0, f"{case.id} {what}: identically zero"
    err = (a32.double() - a64).abs().max().item()
    assert err <= PU.REL * scale, f"{case.id} {what}: |cpu32 - f64| {err / scale:.2e} of max|f64| {scale:.3e}"


@pytest.mark.parametrize("case", BC.CONTRACT, ids=ids(BC.CONTRACT))
def test_contraction_float32_restatement_is_within_rel_of_float64_per_column(case):
    X = BC.contract_gen(case)
    r32, r64 = BC.contractions_2to1(X), BC.contractions_2to1(X.double())
    for c, name in enumerate(BC.COLUMNS):
        within_rel(case, name, r32[..., c], r64[..., c])
    # every column is a different function of the row, and the matrices of a batch differ
    assert len({round(r64[0, 0, c].item(), 6) for c in range(5)}) == (5 if case.p["n"] > 1 else 1)
    if case.p["b"] > 1:
        assert not torch.equal(r64[0], r64[1])


@pytest.mark.parametrize("case", BC.GROUP, ids=ids(BC.GROUP))
def test_grouping_reference_gives_the_multiplicities_the_row_states(case):
    ev = BC.group_gen(case)
    assert ev.numel() == sum(case.p["mults"]) and bool((ev[1:] >= ev[:-1]).all())
    ref = BC.group_reference(ev, case.p["decimals"])
    assert ref["space_mult"].tolist() == case.p["mults"]
    assert ref["space_of"].tolist() == [s for s, m in enumerate(case.p["mults"]) for _ in range(m)]
    assert sorted(ref["space_slot"].tolist()) == list(range(ref["n_spaces"]))


@pytest.mark.parametrize("case", [c for c in BC.GROUP if sum(c.p["mults"]) <= 300], ids=lambda c: c.id)
def test_grouping_reference_is_the_oracles(case):
    """oracle/basisnet.py::group_eigenspaces on the identity as eigenvectors: P_s is the indicator of the eigenspace's columns, so the
    stack it returns per multiplicity spells out counts, order and slots"""
    from oracle import basisnet as OB
    ev = BC.group_gen(case)
    N = ev.numel()
    ref = BC.group_reference(ev, case.p["decimals"])
    groups, counts = OB.group_eigenspaces(ev, torch.eye(N), case.p["decimals"])
    assert counts.tolist() == ref["space_mult"].tolist() and sorted(groups) == ref["mults"]
    stack = torch.cat([groups[m][:, 0] for m in ref["mults"]], 0)                    # the multiplicity-major stack
    assert [groups[m].shape[0] for m in ref["mults"]] == ref["counts"]
    mine = BC.projectors(torch.eye(N), ref, BC.F32)
    assert torch.equal(stack, mine)


@pytest.mark.parametrize("case", BC.PROJECTORS, ids=ids(BC.PROJECTORS))
def test_projector_float32_restatement_is_within_rel_of_float64(case):
    ev, V = BC.projector_gen(case)
    ref = BC.group_reference(ev, 5)
    assert ref["space_mult"].tolist() == case.p["mults"]
    P32, P64 = BC.projectors(V, ref, BC.F32), BC.projectors(V, ref, BC.F64)
    within_rel(case, "projectors", P32, P64)
    c32, c64 = BC.contractions_2to1(P32), BC.contractions_2to1(P64)
    for c, name in enumerate(BC.COLUMNS):
        within_rel(case, name, c32[..., c], c64[..., c])


@pytest.mark.parametrize("case", BC.IGN_MLP + BC.IGN_MLP_UNSUPPORTED, ids=ids(BC.IGN_MLP + BC.IGN_MLP_UNSUPPORTED))
def test_ign_head_float32_restatement_is_within_rel_of_float64(case):
    o, sd = BC.ign_mlp_gen(case)
    y32, y64 = BC.ign_head(o, sd, BC.F32), BC.ign_head(o, sd, BC.F64)
    assert y64.shape == (case.p["b"], case.p["O"], case.p["n"])
    within_rel(case, "y", y32, y64)
    if case.p["b"] > 1:
        assert not torch.equal(y64[0], y64[1])


def test_ign_head_restatement_is_the_oracles():
    """contractions + head on one small projector stack == oracle/basisnet.py::ign2to1 (IGN2to1.forward of the reference) in float64"""
    from oracle import basisnet as OB
    case = BC.PROJECTORS[1]
    ev, V = BC.projector_gen(case)
    X = BC.projectors(V, BC.group_reference(ev, 5), BC.F64)                              # [7, 70, 70]
    _, sd = BC.ign_mlp_gen(BC.IGN_MLP[2])
    sd64 = PU.to_f64(sd)
    eq = [(sd64[f"equi_layers.{i}.coeffs"], sd64[f"equi_layers.{i}.bias"]) for i in range(3)]
    want = OB.ign2to1(sd64, eq, X.unsqueeze(1), training=False)
    o = BC.contractions_2to1(X)
    assert (o - OB.contractions_2_to_1(X.unsqueeze(1))[:, 0].transpose(1, 2)).abs().max().item() <= 1e-12
    got = BC.ign_head(o, sd, BC.F64)
    assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()


@pytest.mark.parametrize("case", BC.DEEPSETS + [BC.DEEPSETS_OVER_LIMIT], ids=ids(BC.DEEPSETS + [BC.DEEPSETS_OVER_LIMIT]))
def test_deepsets_float32_restatement_is_within_rel_of_float64(case):
    x, layers = BC.deepsets_gen(case)
    y32, y64 = BC.eq_deepsets(x, layers, BC.F32), BC.eq_deepsets(x, layers, BC.F64)
    assert y64.shape == (case.p["n"], case.p["widths"][-1])
    within_rel(case, "y", y32, y64)
    # the first layer as the caller of the kernel forms it (either form) is the restatement's first layer
    z = BC.deepsets_first_layer(x, layers[0], case.p["split0"]).double()
    w = case.p["widths"][0]
    h0 = z[:, :w] + z[:, w:].mean(0, keepdim=True) if case.p["split0"] else z
    L0 = {k: v.double() for k, v in layers[0].items()}
    want = x.double() @ L0["w1"].t() + L0["b1"] + x.double().mean(0, keepdim=True) @ L0["w2"].t() + L0["b2"]
    assert (h0 - want).abs().max().item() <= PU.REL * want.abs().max().item()


def test_deepsets_restatement_is_the_oracles():
    from oracle import basisnet as OB
    case = BC.DEEPSETS[4]
    x, layers = BC.deepsets_gen(case)
    sd = {}
    for i, L in enumerate(layers):
        sd.update({f"lins1.{i}.weight": L["w1"], f"lins1.{i}.bias": L["b1"], f"lins2.{i}.weight": L["w2"], f"lins2.{i}.bias": L["b2"]})
        if "gamma" in L:
            sd.update({f"bns.{i}.weight": L["gamma"], f"bns.{i}.bias": L["beta"]})
    want = OB.eq_deepsets(PU.to_f64(sd), x.double(), len(layers), True)
    got = BC.eq_deepsets(x, layers, BC.F64)
    assert (got - want).abs().max().item() <= 1e-12 * want.abs().max().item()
