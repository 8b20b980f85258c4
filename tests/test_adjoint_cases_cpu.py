"""No GPU: the conditions under which the adjoint grid (tests/test_adjoint_grid_gpu.py) can tell a right kernel from a wrong one, checked
on every row of every table of tests/adjoint_cases.py.

  branch        the host restatement of the dispatch returns the row's `branch`, and the rows of an op reach every branch its predicate
                can return
  conditioning  the reference's own float32 arithmetic is within parity_util.REL of float64 for the forward and every gradient — a
                row where it is not cannot separate a right kernel from a wrong one at 1e-5
  ReLU margin   min |pre-activation| over the valid elements >= MARGIN * rms (float64): no ReLU decision can fall on different sides
                in float32 and float64
"""
import math

import pytest
import torch

import adjoint_cases as AC
import parity_util as PU

ALL = [c for op in AC.OPS.values() for c in op.cases]


def test_ids_are_unique():
    ids = [c.id for c in ALL + AC.ADAM]
    assert len(ids) == len(set(ids)), sorted(i for i in ids if ids.count(i) > 1)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_row_takes_the_branch_it_names(case):
    assert AC.OPS[case.op].predicate(case.p) == case.branch


@pytest.mark.parametrize("name", sorted(AC.OPS))
def test_rows_cover_every_branch(name):
    op = AC.OPS[name]
    seen = {b for c in op.cases for b in c.branch.split(" | ")}
    assert seen == op.branches, f"{name}: not reached {sorted(op.branches - seen)}, not declared {sorted(seen - op.branches)}"


def test_named_branches_are_all_in_the_tables():
    """the list the grid was written for"""
    seen = {b for c in ALL for b in c.branch.split(" | ")}
    want = ({f"k_attn16_{d}<{w}>" for d in ("fwd", "bwd") for w in (16, 32, 64)} |
            {"k_set_attention_bwd", "k_set_attention_bwd raised LDS", "k_layernorm_bwd"} | {f"k_layernorm_bwd_v4<{l}>" for l in (8, 16, 32, 64)} |
            {"k_wgrad vec", "k_wgrad scalar", "rpb 128", "rpb 256", "fused bias reduction, sum_parts tmp stage",
             "fused bias reduction, sum_parts single stage", "k_sum_strided x2", "sum_parts tmp stage", "sum_parts single stage",
             "bn_bwd_blocks capped at 2048", "chunk block 64", "chunk block 128", "chunk block 256", "chunk LDS raised", "k_gated_fwd_v4",
             "k_gated_fwd"})
    assert want <= seen, sorted(want - seen)


def test_the_rejected_attention_shape_is_the_one_the_host_refuses():
    r = AC.ATTENTION_REJECTED
    assert AC.attention_branch(r["K"], r["dk"]) == "k_set_attention raised LDS | SN_REQUIRE bwd: LDS > 160 KiB"


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.id)
def test_float32_restatement_is_within_rel_of_float64(case):
    op = AC.OPS[case.op]
    leaves, aux = op.gen(case.p)
    o64, g64 = AC.reference(case, AC.F64, leaves, aux)
    o32, g32 = AC.reference(case, AC.F32, leaves, aux)
    for what, a32, a64 in [(f"output {i}", a, b) for i, (a, b) in enumerate(zip(o32, o64))] + \
                          [(f"grad {i}", a, b) for i, (a, b) in enumerate(zip(g32, g64))]:
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64
        assert bool(torch.isfinite(a64).all())
        scale = a64.abs().max().item()
        if scale == 0:          # exactly zero in exact arithmetic AND in float64 (the softmax over a single slot): float32 must agree
            assert not bool(a32.any()), f"{case.id} {what}: zero in float64, not in float32"
            continue
        err = (a32.double() - a64).abs().max().item()
        assert err <= PU.REL * scale, f"{case.id} {what}: |cpu32 - f64| {err / scale:.2e} of max|f64| {scale:.3e}"
    if case.op in AC.HAS_RELU and AC.HAS_RELU[case.op](case.p):
        pre = op.pre(case.p, aux, *[t.double() for t in leaves])
        m = AC.relu_margin(pre, aux["valid"])
        assert m >= AC.MARGIN, f"{case.id}: min |pre-activation| {m:.2e} of its rms"


@pytest.mark.parametrize("case", AC.ADAM, ids=lambda c: c.id)
def test_adam_float32_reference_is_sane(case):
    """torch.optim.Adam in float32 against the written-out float64 step: the moments at REL; the update as the float32 parameter allows
    (p_new is rounded to the parameter's own ulp: that, not the arithmetic, bounds what `p_new - p_old` can resolve)."""
    p = case.p
    par, grad, m, v = AC.adam_gen(p)
    u64, m64, v64 = AC.adam_f64(p, par, grad, m, v)
    u32, m32, v32 = AC.adam_torch32(p, par, grad, m, v)
    for what, a, b in (("m", m32, m64), ("v", v32, v64)):
        s = b.abs().max().item()
        assert (a.double() - b).abs().max().item() <= PU.REL * s, (case.id, what)
    ulp = 2.0 ** (math.floor(math.log2(max(par.abs().max().item(), 1e-30))) - 23)
    assert (u32 - u64).abs().max().item() <= PU.REL * u64.abs().max().item() + ulp, case.id
