"""-m gpu: every instance of the DGL tree's one-launch net kernels — GIN (sn_gin_net_fused_f32: k_gnn_coop<4|6|8, 1>), Transformer
(sn_transformer_net_fused_f32: k_gnn_coop<4, 2>) and GatedGCN (sn_gatedgcn_fused_f32: k_gatedgcn_net<3|4|5|6>) — against float64.

One parametrized test per table of tests/dgl_stage_cases.py.  A row runs `net(g, h, p, e, None)` in eval mode on its explicit edge lists,
with a seeded random positional encoding (no sign-invariant net in front: only the stage kernel is under test), asserts that the row's
kernel was launched exactly once (layer-path rows: not at all) and that check_last() is clean, and holds the scores to the float64
oracle with the two rules of tests/parity_util.py, no new tolerance:

    attributed    |hip - f64| <= max(REL * scale, 2 |cpu32 - f64| + ATTR * scale),   scale = max |f64|
    elementwise   |hip - cpu32| <= REL |cpu32| + REL rms(cpu32) per element, or no farther from float64 than cpu32 is (+ the same term)

and to the layer path of the same net (fused_stages = False) with `close(..., ref64=)`.  A second run must repeat the first bit for bit
(GatedGCN consumes its edge buffer: the forward rebuilds it), and the row's graphs in reversed order must give, per graph, scores within
the same rules.  The persistent-loop rows of the GatedGCN table launch B = CUs + 40 graphs — eight distinct ones, so 40 workgroups take
a second graph, and the order makes that second graph the one AFTER the workgroup's first (reversed: the one before): its tables, images,
node, edge and pass counts all differ from what the first left in LDS (no edge -> two passes, two passes -> one, more nodes -> fewer,
edges -> none; asserted with the device's own CU count).  Every copy of a graph must get the same bits, which are also the bits it gets
in a batch of the eight.
The guard rows hand each kernel a graph with one in-edge more than it holds in a batch without per-graph edge counts: that graph's score
is NaN, every other score is bit for bit what the batch without it gives, and check_last() raises with the class's wording of the limit.
Of the device-side guards that is status[3] bit 2 alone: bit 1 (more than 64 nodes) and bit 8 (a graph without nodes) cannot be reached
through the nets — a graph object always carries its node counts and _DGLNet._stage filters on them — and stay covered on the host only.

The launch check counts spans of the ENTRY POINT (sn_gatedgcn_fused_f32 ...): which template instance ran is inferred — from the restated
switch, the packing widths the CPU test records and sn_gatedgcn_max_edges — not observed; the per-instance edits below are what shows
that the rows tell the instances apart.

tests/test_dgl_stage_cases_cpu.py asserts, without a GPU, that every row reaches the branches it names and that float32 itself is within REL.

Worst measured |hip - f64| / |cpu32 - f64| (relative to max |f64|) per kernel instance on an MI355X, over the rows and their reversed runs:

    k_gnn_coop<4,1>        5.93e-07 / 2.01e-07   (gin-h40-L2-mean-small)
    k_gnn_coop<6,1>        6.53e-07 / 2.40e-07   (gin-h95-L16-mean-small)
    k_gnn_coop<8,1>        5.78e-07 / 8.38e-07   (gin-h128-L2-max-topology)
    k_gnn_coop<4,2>        5.52e-07 / 5.54e-07   (tf-h64-L1-mean-add-sizes)
    k_gatedgcn_net<3>      3.21e-07 / 1.90e-07   (gated-h12-L2-sum-topology)
    k_gatedgcn_net<4>      3.40e-07 / 1.75e-07   (gated-h64-L2-max-edges)
    k_gatedgcn_net<5>      1.08e-06 / 8.77e-07   (gated-h68-L16-mean-small)
    k_gatedgcn_net<6>      1.01e-06 / 3.01e-07   (gated-h96-L2-sum-edges)
    layer-path rows        GIN 1.70e-07 / 1.09e-07, GatedGCN 4.88e-07 / 1.52e-07, Transformer 1.35e-06 / 1.15e-06 (17 layers)

No element needed the element-wise attribution clause and no row found a defect; the 63 tests take 4 s.  What the rows notice was tried
on the device with value-only edits, one build: the aggregation's 1e-6 changed at NT = 4 alone (exactly the six <4> rows fail), the
next graph's weight prefetch restarted at the last layer instead of layer 0 (exactly the four persistent-loop rows fail), the mean
readout's divisor off by one for <6,1> and <4,2> (exactly their mean rows fail); and, for what a workgroup's first graph leaves behind, the
in-edge ranges of a workgroup's rows kept from its first graph (stale but in bounds; right by accident whenever the second graph is the
first again): exactly the four persistent-loop rows fail.
"""
import ctypes
import re

import pytest
import torch

import dgl_stage_cases as DC
import parity_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


def ids(cases):
    return [c.id for c in cases]


def cu_count():
    from signnet_basisnet_amd._lib import check, lib
    cus = ctypes.c_int(0)
    check(lib().sn_device_info(ctypes.byref(cus), None, None), "sn_device_info")
    assert cus.value > 0
    return cus.value


def forward(net, case, b, counts=True):
    """-> (scores [B, 1], launches of the row's one-launch kernel) of one eval forward on a fresh graph object"""
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import ops
    g = DS.Graph(b["src"].to(DEV), b["dst"].to(DEV), b["sizes"], b["edge_counts"] if counts else None)
    p = b["p"].to(DEV) if case.p["pe"] == "lap_pe" else None
    rec = ops.KernelTimer()
    with rec, torch.no_grad():
        y = net(g, b["h"].to(DEV), p, b["e"].to(DEV), None)[0].clone()
    torch.cuda.synchronize()
    return y, sum(1 for s in rec.spans if s[0] == DC.KERNEL[case.op])


def instance_of(case):
    if not DC.one_launch(case):
        return f"{DC.NET_CLASS[case.op]} layer path"
    return next(w for w in case.branch.split(" ") if w.startswith("k_"))


def accept(case, hip, r32, r64, what=""):
    label = f"{case.id} [{instance_of(case)}]{what}"
    e = PU.attributed(hip, r32, r64, label)
    n = PU.elementwise(hip, r32, label + " (element-wise)", ref64=r64)
    key = instance_of(case)
    WORST[key] = max(WORST.get(key, (0.0, 0.0, "")), (*e, case.id))
    w = WORST[key]
    print(f"\n{label}: |hip - f64| {e[0]:.2e}, |cpu32 - f64| {e[1]:.2e}, {n} elements attributed; worst of {key} so far "
          f"{w[0]:.2e} / {w[1]:.2e} ({w[2]})", end="")


def run_row(case):
    from signnet_basisnet_amd._lib import lib
    p = case.p
    fused = DC.one_launch(case)
    if case.op == "gated":
        assert int(lib().sn_gatedgcn_max_edges(p["hidden"])) == DC.gated_max_edges(p["hidden"]), "the restated EMAX is the library's"
    sd, y32, y64 = DC.reference(case)
    net = DC.build_net(case).to(DEV).eval()
    order = DC.batch_order(case, cu_count())
    r32, r64 = y32[order], y64[order]
    y, n = forward(net, case, DC.assemble(case, order=order))
    assert n == (1 if fused else 0), f"{case.id}: {DC.KERNEL[case.op]} launched {n} times"
    net.check_last()
    assert y.shape == r32.shape and bool(torch.isfinite(y).all())
    accept(case, y, r32, r64)

    # ---- the layer path of the same net
    net.fused_stages = False
    y_layer, n = forward(net, case, DC.assemble(case, order=order))
    net.fused_stages = True
    assert n == 0
    PU.close(y, y_layer, f"{case.id}: one launch vs the layer path", ref64=r64)

    # ---- a second run: the same bits
    y2, n = forward(net, case, DC.assemble(case, order=order))
    assert n == (1 if fused else 0) and torch.equal(y2, y), f"{case.id}: two runs differ"

    # ---- the same graphs in reversed order: per graph the same scores
    rev = order[::-1]
    y_r, _ = forward(net, case, DC.assemble(case, order=rev))
    accept(case, y_r, y32[rev], y64[rev], " (reversed)")

    # ---- the persistent loop: whichever workgroup and iteration evaluated a copy, the same bits — those of a batch of the eight
    if p.get("repeat_beyond_cus"):
        k = len(p["graphs"])
        assert len(order) == cu_count() + 40
        DC.check_second_graphs(case, order, cu_count())          # with this device's grid no workgroup runs the same graph twice
        DC.check_second_graphs(case, rev, cu_count(), reverse=True)
        y8, n = forward(net, case, DC.assemble(case))
        assert n == 1
        idx = torch.tensor(order, device=DEV)
        for j in range(k):
            copies = y[idx == j]
            assert copies.shape[0] >= 2 and bool((copies == copies[0]).all()), f"{case.id}: copies of graph {j} differ"
            assert torch.equal(copies[0], y8[j]), f"{case.id}: graph {j} in the long batch vs among its own eight"
        rcopies = y_r[torch.tensor(rev, device=DEV) == 0]
        assert bool((rcopies == y8[0]).all()), f"{case.id}: graph 0 in the reversed long batch"


@pytest.mark.parametrize("case", DC.GIN, ids=ids(DC.GIN))
def test_gin_net_row(case):
    run_row(case)


@pytest.mark.parametrize("case", DC.GATED, ids=ids(DC.GATED))
def test_gatedgcn_net_row(case):
    run_row(case)


@pytest.mark.parametrize("case", DC.TF, ids=ids(DC.TF))
def test_transformer_net_row(case):
    run_row(case)


GUARDS = [("gin", 64), ("tf", 64), ("gated", 48), ("gated", 64), ("gated", 68), ("gated", 96)]


@pytest.mark.parametrize("op,hidden", GUARDS, ids=[f"{op}-h{h}" for op, h in GUARDS])
def test_graph_beyond_the_kernel_without_edge_counts_is_refused_on_the_device(op, hidden):
    """The kernels' designed refusal: a batch object without per-graph edge counts reaches the kernel, whose own guard hands back NaN for
    the graph it cannot hold (193 in-edges; GatedGCN: max_edges + 1), leaves every other graph's score untouched and raises status[3]."""
    from signnet_basisnet_amd._lib import lib
    table = {"gin": DC.GIN, "tf": DC.TF, "gated": DC.GATED}[op]
    case = next(c for c in table if c.p["hidden"] == hidden and DC.one_launch(c) and not c.p.get("repeat_beyond_cus"))
    limit = int(lib().sn_gatedgcn_max_edges(hidden)) if op == "gated" else DC.GNN_EMAX
    net = DC.build_net(case).to(DEV).eval()
    y_without, n = forward(net, case, DC.assemble(case))
    assert n == 1
    net.check_last()
    b = DC.assemble(case, extra=[DC.oversize_graph(case, limit + 1)])
    y_host, n = forward(net, case, b)                         # with the counts the host decides: the layer path, every score finite
    assert n == 0 and bool(torch.isfinite(y_host).all())
    net.check_last()
    y, n = forward(net, case, b, counts=False)
    assert n == 1
    assert bool(torch.isnan(y[-1]).all()), "the oversize graph's score"
    assert torch.equal(y[:-1], y_without), "the graphs beside the refused one"
    with pytest.raises(RuntimeError, match=re.escape(net._limit_text)):
        net.check_last()
    net.check_last()                                          # reported once
