"""No GPU: the conditions under which the forward-primitive grid (tests/test_ops_grid_gpu.py) can tell a right kernel from a wrong one,
checked on every row of every table of tests/ops_cases.py.

  branch        the host restatement of the dispatch returns the row's `branch`, and the rows of an op reach every name its predicate
                can return; rows not marked cu_dependent take the same branch on 64, 256 and 304 CUs
  conditioning  the reference's own float32 arithmetic is within parity_util.REL of float64 on the row's inputs — a row where it is not
                cannot separate a right kernel from a wrong one at 1e-5
  fixtures      the hand-built batch, the masks and the segment lengths hold the features their rows are named for
"""
import pytest
import torch

import ops_cases as OC
import parity_util as PU

ALL = [c for op in OC.OPS.values() for c in op.cases]


def test_ids_are_unique():
    ids = [c.id for c in ALL]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_row_takes_the_branch_it_names(case):
    pred = OC.OPS[case.op].predicate
    assert pred(case.p) == case.branch
    if not case.p.get("cu_dependent"):
        for cus in (64, 256, 304):
            assert pred(case.p, cus) == case.branch, f"{case.id}: another branch on {cus} CUs"


@pytest.mark.parametrize("name", sorted(OC.OPS))
def test_rows_cover_every_branch(name):
    op = OC.OPS[name]
    seen = set().union(*[OC.names(c.branch) for c in op.cases])
    assert seen == op.branches, f"{name}: not reached {sorted(op.branches - seen)}, not declared {sorted(seen - op.branches)}"


def test_statistics_rows_keep_the_branches_they_were_written_for():
    by_id = {c.id: c for c in OC.COLSTATS + OC.BN_STATS}
    for cid, branch in OC.STATS_PINNED.items():
        assert by_id[cid].branch == branch, cid


def test_clause_rows_falsify_exactly_one_clause():
    alone = [c for c in OC.LINEAR if c.p.get("alone")]
    assert len(alone) == 11
    seen = set()
    for c in alone:
        fx, fy = OC.false_clauses(c.p)
        assert len(fx) + len(fy) == 1, c.id
        seen |= set(fx) | set(fy)
    assert seen == {"ldx % 4", "x", "ldy % 4", "y", "bias", "scale", "shift", "residual", "ldr % 4", "bbias", "ldbb % 4"}


def _kernel_of(case):
    k = case.branch.split(" | ")[0]
    return "lds" if "lds" in k else "ksplit" if "ksplit" in k else "plain"


def test_every_linear_kernel_sees_every_epilogue_and_every_mask():
    """the epilogue exists in three copies: the covering set of epilogues and the masking cases run in each of them"""
    epis, masks = {}, {}
    for c in OC.LINEAR:
        epis.setdefault(_kernel_of(c), set()).add("bb" if c.p["epi"] == "bb_bias" else c.p["epi"])
        masks.setdefault(_kernel_of(c), set()).add(c.p["mask"])
    for k in ("lds", "ksplit", "plain"):
        assert epis[k] == {"none", "pyg", "dgl", "leaky_res", "respre", "bb"}, (k, epis[k])
        assert masks[k] == {None, "k7", "k1"}, (k, masks[k])


def test_linear_masks_hold_a_dead_tile_and_a_partial_tile():
    for mode in ("k7", "k1"):
        for R in (47 if mode == "k1" else 48, 4097):
            nv, K, valid = OC.mask_rows(mode, R, OC.rng(f"m{mode}{R}"))
            assert nv.numel() == OC.cdiv(R, K) and int(nv.max()) <= K and int(nv.min()) >= 0
            tiles = [valid[i:i + 16] for i in range(0, R, 16)]
            if R >= 48:
                assert any(not bool(t.any()) for t in tiles)
            assert any(bool(t.any()) and not bool(t.all()) for t in tiles)
            if R >= 512:          # a k_linear_lds workgroup (at most four consecutive tiles per wave round, 64 .. 255 spans three of them)
                assert not bool(valid[64:256].any())


def test_rejected_flag_pairs():
    assert {f for f, _ in OC.LINEAR_REJECTED.values()} == {OC.EPI_RELU | OC.EPI_LEAKY, OC.EPI_RESIDUAL | OC.EPI_RESIDUAL_PRE}


def test_aggregation_batch_has_the_named_features():
    batch, ei, sizes = OC.agg_batch()
    rowptr, col, eperm, gp = OC.agg_csr(batch, ei, sizes)
    N = batch.numel()
    deg = rowptr[1:] - rowptr[:-1]
    assert N % 2 == 1 and N % 512 != 0 and N > 512
    assert 0 not in ei.tolist()[0] + ei.tolist()[1]                                       # node 0: no edge at all
    assert [int(deg[i]) for i in (0, 1, 2, 3, 4)] == [0, 1, 3, 5, 2]
    assert col[rowptr[4]:rowptr[5]].tolist() == [5, 5]                                    # a multi-edge
    assert col[rowptr[6]:rowptr[7]].tolist() == [6]                                       # a self loop
    assert 70 in sizes and 0 in sizes and max(sizes) == 70
    assert bool((batch[ei[0]] == batch[ei[1]]).all())
    assert not bool((ei[1][1:] >= ei[1][:-1]).all())                                      # edge ids are not in destination order
    assert torch.equal(ei[1][eperm], torch.sort(ei[1])[0]) and torch.equal(ei[0][eperm], col)
    for i in range(N):                                                                    # in-edges of a node in edge-id order
        e = eperm[rowptr[i]:rowptr[i + 1]]
        assert bool((e[1:] > e[:-1]).all())


def test_aggregation_restatement_is_the_plain_sum():
    """the rounds of agg_ref against a dense index_add in float64"""
    batch, ei, sizes = OC.agg_batch()
    csr = OC.agg_csr(batch, ei, sizes)
    g = OC.rng("agg-plain")
    x, ea = torch.randn(batch.numel(), 5, generator=g, dtype=OC.F64), torch.randn(ei.shape[1], 5, generator=g, dtype=OC.F64)
    eps = torch.tensor(0.25, dtype=OC.F32)
    want = torch.zeros_like(x).index_add_(0, ei[1], x[ei[0]]) + 1.25 * x
    assert (OC.agg_ref(x, csr, OC.F64, eps) - want).abs().max().item() < 1e-12
    want = torch.zeros_like(x).index_add_(0, ei[1], (x[ei[0]] + ea).clamp_min(0)) + x
    assert (OC.agg_ref(x, csr, OC.F64, None, ea=ea) - want).abs().max().item() < 1e-12


def test_pool_segments():
    for C, rl in ((1, 256), (20, 8), (256, 1), (300, 1)):
        assert OC.pool_rl(C) == rl
        lens = OC.pool_lens(C)
        assert {0, 1, 8 * rl - 1, 8 * rl, 8 * rl + 1, 24 * rl + 3} <= set(lens)


# ---------------------------------------------------------------------------- conditioning
def within_rel(case, what, a32, a64):
    assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and a32.shape == a64.shape
    assert bool(torch.isfinite(a64).all())
    scale = a64.abs().max().item()
    if scale == 0:
        assert not bool(a32.any()), f"{case.id} {what}: zero in float64, not in float32"
        return
    err = (a32.double() - a64).abs().max().item()
    assert err <= PU.REL * scale, f"{case.id} {what}: |cpu32 - f64| {err / scale:.2e} of max|f64| {scale:.3e}"


@pytest.mark.parametrize("case", OC.LINEAR, ids=lambda c: c.id)
def test_linear_float32_is_within_rel_of_float64(case):
    t = OC.linear_gen(case)
    flags = OC.EPIS[case.p["epi"]][0]
    within_rel(case, "y", OC.linear_ref(flags, t, OC.F32), OC.linear_ref(flags, t, OC.F64))


@pytest.mark.parametrize("case", OC.LINEAR_BN, ids=lambda c: c.id)
def test_linear_bn_float32_is_within_rel_of_float64(case):
    t = OC.linear_bn_gen(case)
    (z32, s32), (z64, s64) = OC.linear_bn_ref(t, OC.F32), OC.linear_bn_ref(t, OC.F64)
    within_rel(case, "z", z32, z64)
    for k in s64:
        within_rel(case, k, s32[k], s64[k])
    assert torch.equal(s32["count"].double(), s64["count"])


@pytest.mark.parametrize("case", OC.COLSTATS + OC.BN_STATS, ids=lambda c: c.id)
def test_statistics_float32_is_within_rel_of_float64(case):
    t = OC.stats_gen(case)
    valid = t["mask"][2]
    s32, s64 = (OC.stats_ref(t["x"], valid, dt, t["gamma"], t["beta"], t["rmean"], t["rvar"]) for dt in (OC.F32, OC.F64))
    for k in s64:
        within_rel(case, k, s32[k], s64[k])
    assert int(s64["count"]) == int(valid.sum())


@pytest.mark.parametrize("case", OC.GIN + OC.GIN_ADD + OC.SLAB + OC.GINE, ids=lambda c: c.id)
def test_aggregation_float32_is_within_rel_of_float64(case):
    batch, ei, sizes = OC.agg_batch()
    csr = OC.agg_csr(batch, ei, sizes)
    t = OC.agg_gen(case, batch.numel(), ei.shape[1])
    kw = dict(eps=t["eps"], ea=t.get("ea"), negate=bool(case.p.get("negate")), plus=t.get("plus"))
    within_rel(case, "out", OC.agg_ref(t["x"], csr, OC.F32, **kw), OC.agg_ref(t["x"], csr, OC.F64, **kw))


@pytest.mark.parametrize("case", OC.POOL, ids=lambda c: c.id)
def test_pool_float32_is_within_rel_of_float64(case):
    x, lens = OC.pool_gen(case)
    a64 = OC.pool_ref(x, lens, case.p["mode"], OC.F64)
    within_rel(case, "out", OC.pool_ref(x, lens, case.p["mode"], OC.F32), a64)
    assert not bool(a64[[i for i, n in enumerate(lens) if n == 0]].any())


def test_named_branches_are_all_in_the_tables():
    """the list the grid was written for"""
    by_id = {c.id: c for c in ALL}
    for what, cid, name in OC.NAMED:
        assert cid in by_id, f"{what}: no row {cid}"
        assert name in OC.names(by_id[cid].branch), f"{what}: {cid} takes [{by_id[cid].branch}]"
