"""-m gpu: every dispatch branch of the eval stage kernels — phi (sn_phi_fused_f32), rho (sn_rho_fused_f32), GINE (sn_gnn_fused_f32) and the
DGL pair (sn_deepsigns_phi_f32 + sn_mlp_chain_f32) — against float64, stage by stage.

One parametrized test over the rows of tests/stage_cases.py.  A SignNetGNN row runs `forward(data, return_stages=True)`, which returns
every fused stage computed from the layer path's inputs, and holds each stage output to the float64 oracle value of that stage with the
two rules of tests/parity_util.py, no new tolerance:

    attributed    |hip - f64| <= max(REL * scale, 2 |cpu32 - f64| + ATTR * scale),   scale = max |f64|      (the rule of the other grids)
    elementwise   |hip - cpu32| <= REL |cpu32| + REL rms(cpu32) per element, or no farther from float64 than cpu32 is (+ the same term)

(phi: over the valid slots — the invalid ones are compared with zero exactly), so that an error in one small row or channel is not
hidden by the tensor's largest entry.  rho and GINE are also held against the layer path of the same call.  Then each stage runs once
more, directly, into a buffer between sentinel guards: the guards must be untouched, phi must leave every invalid slot row at the
sentinel bit pattern and write every valid one, and the result must repeat the first run bit for bit.  The row's graphs in reversed order
must give, per graph, the same stage rows within the same rules (errors tied to a bin position), the span recorder must show the three
stage entry points, and the default forward must leave check_last() clean.

tests/test_stage_cases_cpu.py asserts, without a GPU, that every row reaches the branches it names and that float32 itself is within REL.
"""
import pytest
import torch

import parity_util as PU
import stage_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1024          # floats on either side: several rows of the widest output (128 channels)
SENTINEL = 0x7FA5A5A5          # a NaN with a payload no kernel produces
WORST = {}


def ids(cases):
    return [c.id for c in cases]


def guarded(shape):
    """(buffer, view of `shape`): the output between two guards, every word the sentinel"""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf.view(torch.float32)[GUARD:GUARD + numel].view(*shape)


def check_guards(buf, what):
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()), f"{what}: written in front of the output"
    assert bool((buf[-GUARD:] == SENTINEL).all()), f"{what}: written behind the output"


def written(t, what):
    assert not bool((t.contiguous().view(torch.int32) == SENTINEL).any()), f"{what}: output elements not written"
    assert bool(torch.isfinite(t).all()), f"{what}: not finite"


def accept(case, stage, branch, hip, r32, r64, what=""):
    label = f"{case.id} [{branch}] {stage}{what}"
    e = PU.attributed(hip, r32, r64, label)
    n = PU.elementwise(hip, r32, label + " (element-wise)", ref64=r64)
    key = (stage, branch)
    WORST[key] = max(WORST.get(key, (0.0, 0.0, "")), (*e, case.id))
    w = WORST[key]
    print(f"\n{label}: |hip - f64| {e[0]:.2e}, |cpu32 - f64| {e[1]:.2e}, {n} elements attributed; worst of {stage} [{branch}] so far "
          f"{w[0]:.2e} / {w[1]:.2e} ({w[2]})", end="")


def stage_branches(case):
    p = case.p
    return {"phi": SC.phi_branch(p), "rho_sum": SC.rho_branch(p), "y": f"gnn<{SC.cdiv(p['hid'], 16)}>"}


def compare_stages(case, st, o32, o64, mask, what=""):
    """the three fused stage outputs of one return_stages call against the oracle's (rows already in the call's graph order)"""
    br = stage_branches(case)
    phi = st["phi_fused"].cpu()
    assert not bool(phi[~mask].any()), f"{case.id}{what}: phi left a nonzero in an invalid slot of a zero-filled buffer"
    accept(case, "phi", br["phi"], phi[mask], o32["phi"][mask], o64["phi"][mask], what)
    accept(case, "rho_sum", br["rho_sum"], st["rho_sum_fused"], o32["rho_sum"], o64["rho_sum"], what)
    accept(case, "y", br["y"], st["y_gnn_fused"], o32["y"], o64["y"], what)
    # ... and against the layer path of the same call (same inputs: what differs is the stage kernel alone)
    PU.close(st["rho_sum_fused"], st["rho_sum"], f"{case.id}{what}: fused rho slot sum vs layer kernels", ref64=o64["rho_sum"])
    PU.close(st["y_gnn_fused"], st["y"], f"{case.id}{what}: fused GINE output vs layer kernels", ref64=o64["y"])


@pytest.mark.parametrize("case", SC.PYG, ids=ids(SC.PYG))
def test_signnet_stage_row(case):
    from signnet_basisnet_amd import ops, synth
    p = case.p
    sd, o32, o64, mask = SC.reference(case)
    data = SC.batch_of(case)
    dd = synth.batch_to(data, DEV)
    model = SC.build_model(case).to(DEV).eval()
    B, N, K, d = len(p["sizes"]), sum(p["sizes"]), SC.slot_count(p), p["hid"]
    rec = ops.KernelTimer()
    with rec, torch.no_grad():
        _, st = model(dd, return_stages=True)
    ran = {s[0] for s in rec.spans}
    assert {"sn_batch_plan", "sn_phi_fused_f32", "sn_rho_fused_f32", "sn_gnn_fused_f32"} <= ran, sorted(ran)
    assert st["phi_fused"].shape == (N, K, d) and st["rho_sum_fused"].shape == (N, d) and st["y_gnn_fused"].shape == o32["y"].shape
    compare_stages(case, st, o32, o64, mask)

    # ---- every stage once more, into guarded sentinel buffers (the stage entry points themselves, on the same inputs)
    P = model._prep
    plan = ops.build_plan(dd.batch, dd.edge_index, B, p["max_k"] or 0, bins=True)
    assert torch.equal(plan.nvalid.cpu().long(), mask.sum(1)), "the plan's valid slots are the oracle's mask"
    dmask = mask.to(DEV)
    with torch.no_grad():
        buf, out = guarded((N, K, d))
        P["phi_fused"].run(plan, dd.eigen_vectors, K, out=out)
        check_guards(buf, f"{case.id} phi")
        assert bool((out.view(torch.int32)[~dmask] == SENTINEL).all()), f"{case.id}: phi wrote into an invalid slot"
        written(out[dmask], f"{case.id} phi (valid slots)")
        assert torch.equal(out[dmask], st["phi_fused"][dmask]), f"{case.id}: two runs of phi differ"

        ev = dd.eigen_values if SC.has_eig_encoder(p) else None
        buf, out = guarded((N, d))
        P["rho_fused"].run(plan, st["phi"].contiguous().view(N * K, d), ev, K, out=out)
        check_guards(buf, f"{case.id} rho")
        written(out, f"{case.id} rho")
        assert torch.equal(out, st["rho_sum_fused"]), f"{case.id}: two runs of rho differ"

        buf, out = guarded(tuple(o32["y"].shape))
        P["gnn_fused"].run(plan, dd.x, dd.edge_attr, st["rho_sum"], out=out)
        check_guards(buf, f"{case.id} GINE")
        written(out, f"{case.id} GINE")
        assert torch.equal(out, st["y_gnn_fused"]), f"{case.id}: two runs of the GINE stage differ"
        flags = plan.check()
        assert flags[3] == 0 and flags[1] == max(p["sizes"]), flags

        # ---- the default forward (plan + three stage launches): in-limit rows leave no flag behind
        y = model(dd)
        model.check_last()
    accept(case, "forward", f"{p['variant']} forward", y, o32["y"], o64["y"])

    # ---- the same graphs in reversed order: per graph the same rows
    if B > 1:
        rev, perm = SC.reorder(data, list(range(B))[::-1])
        with torch.no_grad():
            _, st_r = model(synth.batch_to(rev, DEV), return_stages=True)
        flip = lambda o: {"phi": o["phi"][perm], "rho_sum": o["rho_sum"][perm], "y": o["y"].flip(0)}
        compare_stages(case, st_r, flip(o32), flip(o64), mask[perm], " (reversed)")


def test_out_buffers_of_rho_and_gine_are_validated_before_the_launch():
    """the `out=` argument the guarded runs use: a buffer of another shape, dtype or layout is refused, never written"""
    from signnet_basisnet_amd import ops, synth
    case = next(c for c in SC.PYG if c.name == "gine-h64-k16-rho1")
    p = case.p
    dd = synth.batch_to(SC.batch_of(case), DEV)
    model = SC.build_model(case).to(DEV).eval()
    with torch.no_grad():
        _, st = model(dd, return_stages=True)
    P, B, N, K, d = model._prep, len(p["sizes"]), sum(p["sizes"]), SC.slot_count(p), p["hid"]
    plan = ops.build_plan(dd.batch, dd.edge_index, B, p["max_k"], bins=True)
    x = st["phi"].contiguous().view(N * K, d)
    for bad in (torch.empty(N + 1, d, device=DEV), torch.empty(N, d, device=DEV, dtype=torch.float64), torch.empty(d, N, device=DEV).t(),
                torch.empty(N, d)):
        with pytest.raises(ValueError, match="fused rho: out"):
            P["rho_fused"].run(plan, x, None, K, out=bad)
    for bad in (torch.empty(B, 2, device=DEV), torch.empty(B, 1, device=DEV, dtype=torch.float16), torch.empty(B + 1, 1, device=DEV)[::2][:B]):
        with pytest.raises(ValueError, match="fused gnn: out"):
            P["gnn_fused"].run(plan, dd.x, dd.edge_attr, st["rho_sum"], out=bad)


@pytest.mark.parametrize("case", SC.DGL, ids=ids(SC.DGL))
def test_deepsigns_stage_row(case):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import ops
    p = case.p
    sd, x, y32, y64 = SC.dgl_reference(case)
    data = SC.batch_of(case)
    net = SC.build_dgl(case).to(DEV).eval()

    def run(batch, xin):
        ei = batch.edge_index
        g = DS.Graph(ei[0].to(DEV), ei[1].to(DEV), torch.tensor(batch.sizes))
        rec = ops.KernelTimer()
        with rec, torch.no_grad():
            y = net(g, xin.to(DEV))
        ran = {s[0] for s in rec.spans}
        assert {"sn_deepsigns_phi_f32", "sn_mlp_chain_f32"} <= ran, sorted(ran)
        return y

    y = run(data, x)
    assert y.shape == y32.shape
    phi_name, chain_name = case.branch.split(" | ")
    accept(case, "deepsigns y", phi_name, y, y32, y64)
    accept(case, "deepsigns y", chain_name, y, y32, y64)
    assert torch.equal(run(data, x), y), f"{case.id}: two runs differ"
    rev, perm = SC.reorder(data, list(range(len(data.sizes)))[::-1])
    accept(case, "deepsigns y", phi_name, run(rev, x[perm]), y32[perm], y64[perm], " (reversed)")
