"""No GPU: the conditions under which the training-link grid (tests/test_train_stage_grid_gpu.py) can tell a right kernel from a wrong one,
checked on every row of tests/train_stage_cases.py.

  branch        the host restatement of the dispatch (256 CUs) gives the kernels and workgroup-count rules the row names, and the rows of
                an op reach exactly the branches and runtime arms declared for it
  conditioning  the restatement's own float32 arithmetic is within parity_util.REL of float64 for the output and every gradient, under
                one backward pass and under the two accumulated passes of the direct structures; a gradient that is exactly zero in
                float64 is exactly zero in float32
  ReLU margin   min |pre-activation| over the valid elements >= MARGIN * rms (float64)
"""
import pytest
import torch

import parity_util as PU
import train_stage_cases as TC

ALL = TC.TABLE
IDS = [c.id for c in ALL]


def test_ids_are_unique():
    assert len(IDS) == len(set(IDS)), sorted(i for i in IDS if IDS.count(i) > 1)


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_row_takes_the_branch_it_names(case):
    assert " | ".join(TC.kernel_level(TC.trace(case, cus=256).atoms)) == case.branch


@pytest.mark.parametrize("name", sorted(TC.OPS))
def test_rows_cover_every_branch(name):
    seen = {a for c in TC.BY_OP[name] for a in TC.trace(c, cus=256).atoms}
    want = TC.BRANCHES[name]
    assert seen == want, f"{name}: not reached {sorted(want - seen)}, not declared {sorted(seen - want)}"


def test_every_declared_atom_is_reached_by_some_op():
    seen = {a for c in ALL for a in TC.trace(c, cus=256).atoms}
    assert seen == TC.DECLARED, f"not reached {sorted(TC.DECLARED - seen)}, not declared {sorted(seen - TC.DECLARED)}"
    assert set().union(*TC.BRANCHES.values()) == TC.DECLARED


def test_named_branches_are_all_in_the_tables():
    """the list the grid was written for: what no op-level test reached before it"""
    seen = {a for c in ALL for a in TC.trace(c, cus=256).atoms}
    want = {"k_tlin_fwd<8,8,true,true>", "k_tlin_fwd<8,8,false,true>",                    # full width, the weight view not aligned / ldw % 4 != 0
            "k_tlin_fwd<8,8,false,false>", "k_tlin_fwd<8,8,false,true,SPLIT>",            # persistent without statistics
            "k_tlin_bwd<8,8,true,4>", "gx = null @persistent",                             # full width, persistent, gx == nullptr
            "k_tlin_bwd<8,8,true,1>", "gx = null @tile",                                   # want_dx = False in tile mode
            "fwd R = 0 memset", "fwd R = 0 no stats", "bwd R = 0",
            "fwd blocks capped at CUs/G", "bwd blocks capped at CUs/G",
            "bn_bwd_blocks R/32", "bn_bwd_blocks R/128", "bn_bwd_blocks capped at 2·CUs/G",
            "in_relu", "in_scale",                                                         # the `else if (a.in_relu)` arm; in_scale alone
            "nvalid K = 1", "k_tbn_finish C % 16 != 0", "k_tbn_bwd_finish C % 16 != 0",
            "reduce_parts accumulate", "reduce_jobs", "post_link", "post_link + bn finish", "post_link + dot", "dot_finish", "dot_jobs"}
    want |= {f"{a} @{k}" for a in ("coef", "merge", "mask", "x_state + x_relu", "x_mean + sums_part", "gx_accumulate", "dot_x", "want_db", "no db")
             for k in ("tile", "persistent", "split")}
    assert want <= seen, sorted(want - seen)
    assert {c.p["G"] for c in ALL if c.op == "mlp2_bn"} >= {1, 2, 3, 4}                    # a G other than 1 and 2
    # one direct structure with the fused finish (MERGE_COEF off) and one without deferral per backward kernel
    for kind in ("tile", "persistent", "split"):
        for v in ("direct-nomerge", "direct-nodefer"):
            assert any(v in c.p.get("variants", ()) and f"x_mean + sums_part @{kind}" in TC.trace(c).atoms for c in ALL), (kind, v)


def test_the_switches_sit_where_the_rows_say():
    assert TC.tile_mode(8192, 1) and not TC.tile_mode(8193, 1) and TC.tile_mode(4096, 2) and not TC.tile_mode(4097, 2)
    assert TC.tile_mode(2720, 3) and not TC.tile_mode(2721, 3)
    assert (TC.fwd_blocks(8209, 2), TC.bwd_blocks(8209, 2)) == (128, 128) and TC.fwd_blocks(8193, 2) == 128 and TC.bwd_blocks(8192 + 1, 1) == 129
    assert TC.bn_bwd_blocks(16385, 4) == 128 and TC.bn_bwd_blocks(16384, 4) == 128 and TC.bn_bwd_blocks(8193, 1) == 65
    assert TC.fwd_blocks(0, 2) == 1 and TC.bwd_blocks(0, 1) == 1 and TC.bn_bwd_blocks(0, 3) == 1
    assert TC.fwd_blocks(8209, 2, cus=304) == 129          # the cap moves with the device: the GPU test asks the library with its own count


def test_masks_are_what_the_rows_say():
    kinds = {}
    for c in ALL:
        if c.op in ("gin_layer", "gine_layer") or c.p.get("R", 1) == 0:
            continue
        _, aux = TC.OPS[c.op][0](c.p)
        nv, K = aux["nv"], aux["K"]
        if c.p["mask"] == "ragged" and K > 1:
            assert int(nv.max()) == K and int(nv.min()) == 1, c.id
            kinds["ragged"] = True
        if c.p["mask"] in ("rows", "last"):
            assert K == 1 and set(nv.tolist()) == {0, 1}, c.id
        if c.p["mask"] == "last":
            R = c.p["R"]
            first = int(aux["valid"].nonzero()[0])
            assert first >= (R - 1) // 16 * 16 and TC.tile_mode(R, c.p["G"]), c.id      # one 16-row tile per workgroup, the last one
            kinds["last"] = True
    assert kinds == {"ragged": True, "last": True}


def _compare(case, npass, L, aux):
    o64, g64, _, pre = TC.reference(case, TC.F64, L, aux, npass)
    o32, g32, _, _ = TC.reference(case, TC.F32, L, aux, npass)
    gmax = max([v.abs().max().item() for v in g64.values() if v.numel()] + [0.0])
    zero = TC.zero_bias(case)
    for what, a32, a64 in [(f"output {i}", a, b) for i, (a, b) in enumerate(zip(o32, o64))] + [(f"d{k}", g32[k], g64[k]) for k in g64]:
        assert a32.dtype == torch.float32 and a64.dtype == torch.float64 and a32.shape == a64.shape
        assert bool(torch.isfinite(a64).all()), f"{case.id} {what}"
        scale = a64.abs().max().item() if a64.numel() else 0.0
        if what[1:] in zero:          # a bias in front of a batch-statistics BatchNorm: true gradient 0, rounding in both precisions
            assert scale <= 1e-9 * gmax and a32.abs().max().item() <= 1e-5 * gmax, f"{case.id} {what}"
            continue
        if scale == 0:
            assert not bool(a32.any()), f"{case.id} {what}: zero in float64, not in float32"
            continue
        err = (a32.double() - a64).abs().max().item()
        assert err <= PU.REL * scale, f"{case.id} {what} ({npass} pass): |cpu32 - f64| {err / scale:.2e} of max|f64| {scale:.3e}"
    return pre


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_float32_restatement_is_within_rel_of_float64(case):
    L, aux = TC.OPS[case.op][0](case.p)
    pre = _compare(case, 1, L, aux)
    if any(v.startswith("direct") for v in case.p.get("variants", ())):
        _compare(case, 2, L, aux)
    vv = aux["valid"]
    for a in pre:
        if a.shape[0] == 0:
            continue
        v = vv.repeat(a.shape[0] // vv.numel())
        av = a[v]
        m = (av.abs().min() / av.pow(2).mean().sqrt()).item()
        assert m >= TC.MARGIN, f"{case.id}: min |pre-activation| {m:.2e} of its rms"
    # the convention of train_stage.py: inputs zero on invalid rows (the raw rows carry data there on purpose: the kernel masks them)
    if case.op != "raw_link" and vv.numel():
        x = L["x"].reshape(-1, vv.numel(), *L["x"].shape[1:]) if L["x"].dim() > 1 else L["x"].reshape(-1, vv.numel())
        assert not bool(x[:, ~vv].any()), case.id
