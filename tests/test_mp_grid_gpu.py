"""-m gpu: the message-passing kernels of csrc/dgl_layers.hip and their adjoints against float64, on a batch whose in-edge CSR and
flipped-edge CSR differ (tests/mp_cases.py: a hub of 39 in-edges, nodes without in-edges and without out-edges, self loops, duplicate
and directed-only edges, a shuffled edge list) and on a small molecule batch.

One parametrized test per op over its table.  A row runs the HIP path, the float32 CPU autograd and the float64 CPU autograd of the
restatement on the same inputs and the same seeded cotangents, and holds the forward value and every input gradient to the project's
attribution rule (parity_util.attributed):

    |hip - f64| <= max(REL * scale, 2 |cpu32 - f64| + ATTR * scale),   scale = max |f64|

Two exceptions, both taken from tests/test_dgl_basisnet_gpu.py: the std columns of the PNA forward are held to the bound derived there
(the rounding of E[x^2] through the square root: mp_cases.pna_std_bound), and dmsg of the PNA adjoint run with the cotangent that is
non-zero ONLY on the std columns keeps the bounds of the adjoint test there (2e-3 of the largest entry, 5e-4 on edges into nodes of
in-degree >= 3).  The run with the cotangent that is zero on the std columns is under `attributed` like everything else.

Besides: a node without in-edges gets exact zeros (PNA, edge attention) or act(bias) (GAT); a node without out-edges gets exact zeros in
dK / dV and in the adjoint of the source gather; a second run gives the same bits (no atomics).  tests/test_mp_cases_cpu.py asserts,
without a GPU, that every row reaches the kernel it names and that no discontinuous decision sits within rounding of its threshold.

Measured on an MI355X, largest |hip - f64| / max |f64| per op (the fp32 CPU reference's own distance beside it): pna 1.2e-7 (1.3e-7),
its std columns at 0.28 of their bound and dmsg under the std-only cotangent at 6.9e-4 (1.6e-5 where in-degree >= 3); pna_gather 1.6e-7
(1.6e-7); edge attention 1.3e-6 (6.2e-7), strided forward 2.5e-7 (2.5e-7); gat_aggregate 1.1e-5 (1.5e-5) for the 128-wide head and
9.6e-6 (2.5e-6) for the 64-wide one, both on d attn_r; gather_rows 1.8e-7 (1.8e-7).  Run with -s for the figures of every row.
"""
import functools

import pytest
import torch

import mp_cases as MP
import parity_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ids(rows):
    return [r.id for r in rows]


@functools.lru_cache(maxsize=None)
def plans(name):
    """(the batch plan, the plan of the flipped edge list) of a graph of mp_cases"""
    from signnet_basisnet_amd import ops
    g = MP.graph(name)
    B = int(g.batch.max()) + 1
    batch = g.batch.to(DEV)
    return ops.build_plan(batch, g.ei.contiguous().to(DEV), B, 0), ops.build_plan(batch, g.ei.flip(0).contiguous().to(DEV), B, 0)


def dev(t):
    return t.to(DEV).detach().requires_grad_(True)


class Report:
    """holds a row's tensors to parity_util.attributed and prints the worst distance next to the fp32 CPU reference's own"""

    def __init__(self, row):
        self.row, self.worst = row, (0.0, 0.0, "")

    def hold(self, what, hip, r32, r64):
        assert hip is not None, f"{self.row.id} {what}: no gradient"
        assert tuple(hip.shape) == tuple(r64.shape), f"{self.row.id} {what}: shape {tuple(hip.shape)} vs {tuple(r64.shape)}"
        e = PU.attributed(hip, r32, r64, f"{self.row.id} [{self.row.branch}] {what}")
        self.note(what, *e)

    def note(self, what, e_hip, e_cpu):
        self.worst = max(self.worst, (e_hip, e_cpu, what))

    def done(self):
        print(f"\n{self.row.id}: worst |hip - f64| {self.worst[0]:.2e}, |cpu32 - f64| there {self.worst[1]:.2e} ({self.worst[2]})", end="")


def same_bits(a, b, what):
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y), f"{what}: a second run gives other bits"


# ---------------------------------------------------------------------------- PNA aggregation
def _pna_autograd(row, aux, leaves, plan):
    from signnet_basisnet_amd import autograd as AG
    xs = [dev(t) for t in leaves]
    out = AG.pna_aggregate(xs[0], xs[1], plan, MP.AVG_LOG)
    return out.detach(), {name: list(torch.autograd.grad(out, xs, cot[0].float().to(DEV), retain_graph=True)) for name, cot in aux["cots"].items()}


def _pna_entry_points(row, aux, leaves, plan):
    """sn_pna_aggregate_f32 / sn_pna_aggregate_bwd_f32 with message rows ldm apart and / or without hself"""
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    p, g = row.p, aux["g"]
    C, ldm, c0 = p["C"], p["ldm"] or p["C"], aux["c0"]
    wide = aux["wide"].to(DEV)
    msg = wide[:, c0:c0 + C]                                       # a view: rows ldm floats apart
    assert wide.shape == (g.E, ldm) and msg.data_ptr() == wide.data_ptr() + 4 * c0
    hself = leaves[1].to(DEV) if p["hself"] else None
    W = MP.pna_width(C, p["hself"])
    out = torch.full((g.N, W), 7.0, dtype=torch.float32, device=DEV)
    check(lib().sn_pna_aggregate_f32(ptr(msg), ldm, ptr(hself), C, C, g.N, ptr(plan.rowptr), ptr(plan.eperm), MP.AVG_LOG, ptr(out), W, stream()),
          "sn_pna_aggregate_f32")
    grads = {}
    for name, cot in aux["cots"].items():
        go = cot[0].float().to(DEV)
        dmsg = torch.full((g.E, C), 7.0, dtype=torch.float32, device=DEV)      # every edge has a destination: every row is written
        dself = torch.full((g.N, C), 7.0, dtype=torch.float32, device=DEV) if p["hself"] else None
        check(lib().sn_pna_aggregate_bwd_f32(ptr(msg), ldm, C, g.N, ptr(plan.rowptr), ptr(plan.eperm), MP.AVG_LOG, ptr(go), W, ptr(dmsg), ptr(dself),
                                             stream()), "sn_pna_aggregate_bwd_f32")
        grads[name] = [dmsg] + ([dself] if p["hself"] else [])
    assert torch.equal(wide.cpu(), aux["wide"])
    return out, grads


def _pna_forward_checks(rep, row, aux, out, o32, o64, own_columns):
    """everything but the std columns under `attributed`; those within the derived bound; exact zeros for a node without in-edges"""
    std, bound = MP.pna_std(row)
    rep.hold("forward (mean, max, min, own row)", out[:, ~std], o32[:, ~std], o64[:, ~std])
    err = (out.cpu().double() - o64)[:, std].abs()
    assert bool((err <= bound).all()), f"{row.id} std columns: worst |hip - f64| / bound {(err / bound).max().item():.2f}"
    print(f"\n{row.id}: std columns at most {(err / bound).max().item():.2f} of their bound "
          f"(cpu32: {((o32.double() - o64)[:, std].abs() / bound).max().item():.2f})", end="")
    lone = aux["g"].deg_in == 0
    assert bool(lone.any()) == (aux["g"].name == "topo")
    assert not bool(out.cpu()[lone][:, ~own_columns].any()), f"{row.id}: a node without in-edges must get exact zeros"


@pytest.mark.parametrize("row", MP.PNA, ids=ids(MP.PNA))
def test_pna_aggregate(row):
    p = row.p
    leaves, aux = MP.inputs(row)
    g, C = aux["g"], p["C"]
    plan, _ = plans(g.name)
    run = _pna_autograd if row.branch.endswith("autograd.pna_aggregate") else _pna_entry_points
    out, grads = run(row, aux, leaves, plan)
    (o32, g32), (o64, g64) = MP.references(row)
    rep = Report(row)
    own = torch.zeros(out.shape[1], dtype=torch.bool)
    own[:C if p["hself"] else 0] = True
    _pna_forward_checks(rep, row, aux, out, o32[0], o64[0], own)
    names = ["dmsg", "dself"][:len(leaves)]
    for what, h, a32, a64 in zip(names, grads["std-free"], g32["std-free"], g64["std-free"]):
        rep.hold(f"{what} (cotangent zero on the std columns)", h, a32, a64)
    # the cotangent that is non-zero only on the std columns: d std = (x - mean) / (D std) with std^2 = relu(E[x^2] - E[x]^2) + 1e-5 computed
    # in fp32 — compared at the level that cancellation allows, as test_pna_and_edge_attention_adjoints_vs_fp64_autograd does
    dmsg, r64 = grads["std-only"][0].cpu().double(), g64["std-only"][0]
    scale = r64.abs().max().item()
    err = (dmsg - r64).abs()
    well = g.deg_in[g.dst] >= 3
    print(f"\n{row.id}: dmsg (std-only cotangent) {err.max().item() / scale:.2e} of the largest entry, {err[well].max().item() / scale:.2e} where "
          f"in-degree >= 3 (cpu32: {(g32['std-only'][0].double() - r64).abs().max().item() / scale:.2e})", end="")
    assert err.max().item() <= 2e-3 * scale, f"{row.id} dmsg (std-only cotangent): {err.max().item() / scale:.2e} of the largest entry"
    assert err[well].max().item() <= 5e-4 * scale, f"{row.id} dmsg (std-only cotangent), in-degree >= 3: {err[well].max().item() / scale:.2e}"
    if p["hself"]:
        assert not bool(grads["std-only"][1].any())                # no std column is the node's own row
    out2, grads2 = run(row, aux, leaves, plan)
    same_bits([out] + grads["std-free"] + grads["std-only"], [out2] + grads2["std-free"] + grads2["std-only"], row.id)
    rep.done()


@pytest.mark.parametrize("row", MP.PNA_GATHER, ids=ids(MP.PNA_GATHER))
def test_pna_aggregate_gather_forward(row):
    from signnet_basisnet_amd import ops
    p = row.p
    leaves, aux = MP.inputs(row)
    C, it = p["C"], p["tower"]
    plan, _ = plans(aux["g"].name)
    psd, qe, hself = (t.to(DEV) for t in leaves)
    if p["qe_layer"] is not None:
        qe = aux["qe_all"].to(DEV)
    out = ops.pna_aggregate_gather(psd, qe, hself, plan, MP.AVG_LOG, tower_width=it, qe_layer=p["qe_layer"])
    (o32, _), (o64, _) = MP.references(row)
    rep = Report(row)
    own = torch.zeros(1, 13 * C, dtype=torch.bool)
    own[:, :C] = True
    _pna_forward_checks(rep, row, aux, out, o32[0], o64[0], MP.tower_major(own, C, it)[0] if it else own[0])
    same_bits([out], [ops.pna_aggregate_gather(psd, qe, hself, plan, MP.AVG_LOG, tower_width=it, qe_layer=p["qe_layer"])], row.id)
    rep.done()


# ---------------------------------------------------------------------------- sparse edge attention
def _edge_attention_run(row, aux, leaves, plan, rplan):
    from signnet_basisnet_amd import autograd as AG
    xs = [dev(t) for t in leaves]
    out = AG.edge_attention(*xs, plan, rplan, row.p["H"])
    out.backward(aux["cots"][""][0].float().to(DEV))
    return out.detach(), [x.grad for x in xs]


@pytest.mark.parametrize("row", MP.EDGE_ATTENTION, ids=ids(MP.EDGE_ATTENTION))
def test_edge_attention(row):
    from signnet_basisnet_amd import ops
    p = row.p
    leaves, aux = MP.inputs(row)
    g, H, d = aux["g"], p["H"], p["H"] * p["dk"]
    plan, rplan = plans(g.name)
    (o32, g32), (o64, g64) = MP.references(row)
    rep = Report(row)
    lone, sink = g.deg_in == 0, g.deg_out == 0
    if p["layer"] is not None:
        # the fused projections: Q | K | V side by side, the layer's E block between the other layers' blocks
        Q, K, V, Ee = (t.to(DEV) for t in leaves)
        qkv = torch.cat([Q, K, V], 1).contiguous()
        Ee_all = aux["other"].to(DEV).clone()
        Ee_all[:, p["layer"] * d:(p["layer"] + 1) * d] = Ee
        out = ops.edge_attention_fused(qkv, Ee_all, p["layer"], plan, H)
        rep.hold("forward (strided)", out, o32[0], o64[0])
        assert torch.equal(out, ops.edge_attention(Q, K, V, Ee, plan, H)), f"{row.id}: the strided entry point runs the same kernel on the same values"
        assert not bool(out[lone.to(DEV)].any())
        rep.done()
        return
    out, grads = _edge_attention_run(row, aux, leaves, plan, rplan)
    rep.hold("forward", out, o32[0], o64[0])
    for what, h, a32, a64 in zip(("dQ", "dK", "dV", "dE"), grads, g32[""], g64[""]):
        rep.hold(what, h, a32, a64)
    dQ, dK, dV, dE = (t.cpu() for t in grads)
    assert not bool(out.cpu()[lone].any()) and not bool(dQ[lone].any()), f"{row.id}: a node without in-edges must get exact zeros"
    assert not bool(dK[sink].any()) and not bool(dV[sink].any()), f"{row.id}: a node without out-edges must get exact zeros in dK / dV"
    assert bool(lone.any()) == bool(sink.any()) == (g.name == "topo")
    # where the forward clamped the score the adjoint passes nothing to it: dE of such an (edge, head) is exactly zero.  The only other
    # exact zeros are single in-edges, whose weight s / (s + 1e-6) rounds to 1 in fp32: out is then V[src] to the bit and d score vanishes
    s = MP.edge_scores(g, H, *(t.double() for t in (leaves[0], leaves[1], leaves[3])))
    dead, clamped = (dE.view(g.E, H, p["dk"]) == 0).all(-1), s.abs() > 5
    assert bool(dead[clamped].all()), f"{row.id}: {int((clamped & ~dead).sum())} of {int(clamped.sum())} clamped scores got a gradient"
    assert bool((g.deg_in[g.dst] == 1)[(dead & ~clamped).any(1)].all()), f"{row.id}: dE vanishes on an unclamped score of a node with several in-edges"
    out2, grads2 = _edge_attention_run(row, aux, leaves, plan, rplan)
    same_bits([out] + grads, [out2] + grads2, row.id)
    rep.done()


# ---------------------------------------------------------------------------- GAT aggregation
def _gat_run(row, aux, leaves, plan, rplan):
    from signnet_basisnet_amd import autograd as AG
    p = row.p
    xs = [dev(t) for t in leaves]
    out = AG.gat_aggregate(xs[0], xs[1], xs[2], xs[3] if p["bias"] else None, plan, rplan, p["H"], MP.SLOPE, p["relu"])
    out.backward(aux["cots"][""][0].float().to(DEV))
    return out.detach(), [x.grad for x in xs]


@pytest.mark.parametrize("row", MP.GAT, ids=ids(MP.GAT))
def test_gat_aggregate(row):
    from signnet_basisnet_amd import ops
    p = row.p
    leaves, aux = MP.inputs(row)
    g, H, C = aux["g"], p["H"], p["C"]
    plan, rplan = plans(g.name)
    (o32, g32), (o64, g64) = MP.references(row)
    out, grads = _gat_run(row, aux, leaves, plan, rplan)
    rep = Report(row)
    rep.hold("forward", out, o32[0], o64[0])
    for what, h, a32, a64 in zip(("d feat", "d attn_l", "d attn_r", "d bias"), grads, g32[""], g64[""]):
        rep.hold(what, h, a32, a64)
    # a node without in-edges: out = act(bias) to the bit and lse = 0, the value the adjoint reads for it
    lone = g.deg_in == 0
    assert bool(lone.any()) == (g.name == "topo")
    b = leaves[3] if p["bias"] else torch.zeros(H * C)
    want = torch.relu(b) if p["relu"] else b
    assert torch.equal(out.cpu()[lone], want[None, :].expand(int(lone.sum()), -1)), f"{row.id}: a node without in-edges must get act(bias)"
    feat, al, ar = (t.to(DEV) for t in leaves[:3])
    out_f, lse = ops.gat_aggregate(feat, al, ar, b.to(DEV) if p["bias"] else None, plan, H, MP.SLOPE, relu=p["relu"], want_lse=True)
    assert torch.equal(out_f, out) and not bool(lse.cpu()[lone].any()) and bool(torch.isfinite(lse).all())
    out2, grads2 = _gat_run(row, aux, leaves, plan, rplan)
    same_bits([out] + grads, [out2] + grads2, row.id)
    rep.done()


# ---------------------------------------------------------------------------- node rows gathered onto edges
def _gather_run(row, aux, leaves, plan, idx):
    from signnet_basisnet_amd import autograd as AG
    h = dev(leaves[0])
    out = AG.gather_rows(h, idx, plan)
    out.backward(aux["cots"][""][0].float().to(DEV))
    return out.detach(), [h.grad]


@pytest.mark.parametrize("row", MP.GATHER_ROWS, ids=ids(MP.GATHER_ROWS))
def test_gather_rows_and_edge_rows_sum(row):
    p = row.p
    leaves, aux = MP.inputs(row)
    g = aux["g"]
    by_dst = p["side"] == "dst"
    plan = plans(g.name)[0 if by_dst else 1]
    idx, deg = (g.dst, g.deg_in) if by_dst else (g.src, g.deg_out)
    (o32, g32), (o64, g64) = MP.references(row)
    out, grads = _gather_run(row, aux, leaves, plan, idx.to(DEV))
    rep = Report(row)
    rep.hold("forward", out, o32[0], o64[0])
    rep.hold("dh", grads[0], g32[""][0], g64[""][0])
    assert not bool(grads[0].cpu()[deg == 0].any()), f"{row.id}: a node that no edge reads must get exact zeros"
    out2, grads2 = _gather_run(row, aux, leaves, plan, idx.to(DEV))
    same_bits([out] + grads, [out2] + grads2, row.id)
    rep.done()
