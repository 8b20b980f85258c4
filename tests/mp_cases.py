"""Case tables, input generators and dtype-generic torch restatements for the message-passing grid of the DGL base nets: the ops of
csrc/dgl_layers.hip (PNA aggregation, sparse edge attention, GAT aggregation, rows gathered onto edges) and their adjoints.
tests/test_mp_grid_gpu.py runs the HIP kernels on the rows, tests/test_mp_cases_cpu.py checks the conditions that make that comparison
mean something.  Importable without a GPU: nothing here touches a device or the package's library.

Graphs.  `adjoint_cases.topology_batch()` (203 nodes, 646 directed edges: a hub with 39 in-edges, nodes without in-edges and without
out-edges, self loops, duplicate edges, directed-only edges, a shuffled edge list) is where the in-edge CSR and the CSR of the flipped
edge list differ in degrees and neighbour sets — a source-side adjoint that walked the wrong one of the two cannot pass on it — and one
small `synth.make_batch` molecule batch is the ordinary case.

Restatements are written from the formulas of include/signnet_hip.h (the f3 message-passing block), generic in dtype: torch.autograd over
them is the exact adjoint in float64 and the reference's own in float32.  The PNA restatement reduces a padded mailbox [N, Dmax, C] in
edge-id order with torch.max(dim) / torch.min(dim), which return — and differentiate through — the FIRST extremum, as the kernel does;
scatter_reduce(amax) would split a tie.

Discontinuities.  Four decisions in these ops are discontinuous in the inputs: the clamp of an attention score at +-5, the LeakyReLU of
a GAT logit, the ReLU of the GAT output, and which in-edge is the maximum / minimum of a PNA channel.  A value within rounding of
such a decision falls on different sides in fp32 and float64 and moves a gradient entry by a whole term.  The generators keep every
decision `PUSH` of the tensor's rms away (the CPU test asserts `MARGIN`), both taken from adjoint_cases: conditions on the inputs,
not tolerances on the kernels.  The `ties` rows are the opposite case on purpose: message rows that are bit-identical in fp32, where
the decision is exact in every precision and only the tie RULE (first in edge order) is left to check.
"""
import functools
import types

import torch

import adjoint_cases as AC
from adjoint_cases import F32, F64, MARGIN, PUSH, cotangent, rng

INF = float("inf")
AVG_LOG = 1.3                 # avg_d['log'] of the existing op tests
SLOPE = 0.2                   # GATConv's negative_slope (gat_net.py:62-66)
MOLECULE_SEED = 29
L_FUSED = 3                   # layers side by side in the fused E / Qe projections
TOPOLOGY_FACTS = dict(N=203, E=646, zero_in=17, zero_out=13, max_in=39)


class Row(AC.Case):
    """a case of adjoint_cases plus the hazard the row exists for"""

    def __init__(self, op, branch, hazard, **p):
        super().__init__(op, branch, **p)
        self.hazard = hazard


# ============================================================================ graphs
@functools.lru_cache(maxsize=None)
def graph(name):
    """-> ei [2, E], batch [N], src, dst, deg_in, deg_out, mail [N, Dmax] (the in-edge ids of a node in edge-id order, -1 padded: the order
    the destination-sorted CSR of sn_batch_plan walks them in)"""
    if name == "topo":
        ei, batch, _ = AC.topology_batch()
    else:
        from signnet_basisnet_amd import synth
        data = synth.make_batch(6, seed=MOLECULE_SEED)
        ei, batch = data.edge_index, data.batch
    src, dst = ei[0], ei[1]
    N, E = batch.numel(), ei.shape[1]
    deg_in, deg_out = torch.bincount(dst, minlength=N), torch.bincount(src, minlength=N)
    order = torch.sort(dst, stable=True).indices                   # edge ids grouped by destination, ascending within a group
    start = torch.cumsum(deg_in, 0) - deg_in
    slot = torch.arange(E) - start[dst[order]]
    mail = torch.full((N, max(int(deg_in.max()), 2)), -1, dtype=torch.long)
    mail[dst[order], slot] = order
    return types.SimpleNamespace(name=name, ei=ei, batch=batch, src=src, dst=dst, N=N, E=E, deg_in=deg_in, deg_out=deg_out, mail=mail)


def graph_facts(g):
    pairs = set(zip(g.src.tolist(), g.dst.tolist()))
    return dict(N=g.N, E=g.E, zero_in=int((g.deg_in == 0).sum()), zero_out=int((g.deg_out == 0).sum()), max_in=int(g.deg_in.max()),
                duplicates=g.E - len(pairs), self_loops=int((g.src == g.dst).sum()),
                directed_only=sum((d, s) not in pairs for s, d in pairs), sorted=bool((g.dst[1:] >= g.dst[:-1]).all()))


def duplicate_groups(g):
    """edge ids that share (src, dst), as lists of two or more in edge order"""
    seen = {}
    for e, (s, d) in enumerate(zip(g.src.tolist(), g.dst.tolist())):
        seen.setdefault((s, d), []).append(e)
    return [v for v in seen.values() if len(v) > 1]


# ============================================================================ PNA aggregation
def pna_width(C, hself):
    return (13 if hself else 12) * C


def std_columns(C, hself):
    """bool [width]: the three std blocks, columns off + (4s + 3) C .. off + (4s + 4) C"""
    off = C if hself else 0
    m = torch.zeros(pna_width(C, hself), dtype=torch.bool)
    for s in range(3):
        m[off + (4 * s + 3) * C:off + (4 * s + 4) * C] = True
    return m


def pna_restate(g, msg, hself, avg_log=AVG_LOG):
    """sn_pna_aggregate_f32: out[n, off + (4 s + a) C + c], a in {mean, max, min, std}, s in {1, log(D+1)/avg_log, avg_log/log(D+1)} over
    the in-edges of n in edge-id order; the node's own row in front when hself is given; zeros for a node without in-edges"""
    ok = (g.mail >= 0)[:, :, None]
    M = msg[g.mail.clamp(min=0)]                                   # [N, Dmax, C]
    zero = torch.zeros((), dtype=msg.dtype)
    D = g.deg_in.clamp(min=1).to(msg.dtype)[:, None]
    mean = torch.where(ok, M, zero).sum(1) / D
    ex2 = torch.where(ok, M * M, zero).sum(1) / D
    sd = torch.sqrt(torch.relu(ex2 - mean * mean) + 1e-5)
    mx = M.masked_fill(~ok, -INF).max(dim=1).values
    mn = M.masked_fill(~ok, INF).min(dim=1).values
    agg = torch.where((g.deg_in > 0)[:, None], torch.cat([mean, mx, mn, sd], 1), zero)
    logd = torch.log(D + 1.0)
    out = torch.cat([agg, agg * (logd / avg_log), agg * (avg_log / logd)], 1)
    return out if hself is None else torch.cat([hself, out], 1)


def pna_std_bound(g, msg):
    """The bound the forward's std columns are held to, as tests/test_dgl_basisnet_gpu.py::test_pna_aggregate_and_edge_attention_vs_fp64
    derives it: std = sqrt(relu(E[x^2] - E[x]^2) + 1e-5) cancels in fp32 — in the reference too — so the variance carries an absolute
    error of a few fp32 roundings of E[x^2], which the square root turns into 4e-7 E[x^2] / (2 std); + 1e-6, times two.  The amplified
    and attenuated blocks carry that error times their scaler.  msg: the float64 cast of the messages -> [N, 3 C], block by block"""
    C = msg.shape[1]
    deg = g.deg_in.clamp(min=1).double()[:, None]
    ex2 = torch.zeros(g.N, C, dtype=F64).index_add_(0, g.dst, msg.double() ** 2) / deg
    mean = torch.zeros(g.N, C, dtype=F64).index_add_(0, g.dst, msg.double()) / deg
    sd = torch.sqrt(torch.relu(ex2 - mean * mean) + 1e-5)
    tol = (4e-7 * ex2 / (2 * sd) + 1e-6) * 2.0
    logd = torch.log(deg + 1.0)
    return torch.cat([tol, tol * (logd / AVG_LOG), tol * (AVG_LOG / logd)], 1)


def pna_gaps(g, msg):
    """float64 -> (gap between the maximum and the runner-up, the same for the minimum) per (node, channel), inf where in-degree < 2;
    0 where the extremum is attained twice"""
    ok = (g.mail >= 0)[:, :, None]
    M = msg.double()[g.mail.clamp(min=0)]
    two = (g.deg_in >= 2)[:, None]
    hi = M.masked_fill(~ok, -INF).topk(2, dim=1)
    lo = (-M).masked_fill(~ok, -INF).topk(2, dim=1)
    inf = torch.full((), INF, dtype=F64)
    return (torch.where(two, hi.values[:, 0] - hi.values[:, 1], inf), torch.where(two, lo.values[:, 0] - lo.values[:, 1], inf),
            hi.indices[:, 0], lo.indices[:, 0])


def pna_margins(g, msg):
    """-> dict: smallest non-zero gap at the maximum / minimum in units of rms(msg), and the number of (node, channel) pairs tied there"""
    gmax, gmin, _, _ = pna_gaps(g, msg)
    rms = msg.double().pow(2).mean().sqrt()
    out = {}
    for k, gap in (("max", gmax), ("min", gmin)):
        out["ties_" + k] = int((gap == 0).sum())
        rest = gap[(gap > 0) & torch.isfinite(gap)]
        out["gap_" + k] = (rest.min() / rms).item() if rest.numel() else INF
    return out


def push_extrema(g, msg, iters=8):
    """Where the unique maximum (minimum) of a (node, channel) is within PUSH * rms of the runner-up, move it outward by 3 * PUSH * rms.
    (The extremum, not the runner-up: moving it outward cannot bring it close to a third value, and it is never one of a tied set of
    rows, which therefore stay bit-identical.)"""
    for _ in range(iters):
        m64 = msg.double()
        rms = m64.pow(2).mean().sqrt()
        gmax, gmin, imax, imin = pna_gaps(g, msg)
        moved = False
        for gap, slot, sgn in ((gmax, imax, 1.0), (gmin, imin, -1.0)):
            n, c = ((gap > 0) & (gap < PUSH * rms)).nonzero(as_tuple=True)
            if n.numel():
                m64[g.mail[n, slot[n, c]], c] += sgn * 3 * PUSH * rms
                moved = True
        if not moved:
            return msg
        msg = m64.float()
    raise AssertionError("push_extrema: gaps below PUSH remain")


TIE_SHARE = 3                 # every third in-edge of the hub carries the same message row


def tie_groups(g):
    """sets of in-edges of ONE node that get bit-identical message rows: every group of duplicate edges, and every TIE_SHARE-th in-edge
    of the hub"""
    hub = int(g.deg_in.argmax())
    return duplicate_groups(g) + [g.mail[hub, :int(g.deg_in[hub])][::TIE_SHARE].tolist()]


def impose_ties(g, msg, gen):
    """Channel c of a group's shared row: c % 3 == 0 above every other in-edge of the node (a tie at the maximum), c % 3 == 1 below (a
    tie at the minimum), c % 3 == 2 wherever the draw falls (a tie in the interior, which must not matter)."""
    msg = msg.clone()
    C = msg.shape[1]
    c = torch.arange(C)
    for grp in tie_groups(g):
        n = int(g.dst[grp[0]])
        assert all(int(g.dst[e]) == n for e in grp)
        others = [e for e in g.mail[n, :int(g.deg_in[n])].tolist() if e not in grp]
        v = torch.randn(C, generator=gen)
        if others:
            far = 0.5 + torch.randn(C, generator=gen).abs()
            v = torch.where(c % 3 == 0, msg[others].max(0).values + far, v)
            v = torch.where(c % 3 == 1, msg[others].min(0).values - far, v)
        msg[grp] = v
    return msg


def pna_branch(hself, ldm, C):
    """sn_pna_aggregate_f32 / sn_pna_aggregate_bwd_f32 launch one kernel each, whatever the shape; autograd.pna_aggregate always passes
    hself and contiguous messages, so the other two argument forms are reached through the entry points"""
    via = "autograd.pna_aggregate" if hself and (ldm or C) == C else "entry points"
    return " | ".join(["k_pna_aggregate", "k_pna_aggregate_bwd", "hself" if hself else "no hself", "ldm > C" if (ldm or C) > C else "ldm = C", via])


PNA_BRANCHES = {"k_pna_aggregate", "k_pna_aggregate_bwd", "hself", "no hself", "ldm > C", "ldm = C", "autograd.pna_aggregate", "entry points"}


def _pna(C, hself, hazard, ldm=None, ties=False, graph="topo"):
    return Row("pna", pna_branch(hself, ldm, C), hazard, C=C, hself=hself, ldm=ldm, ties=ties, graph=graph)


PNA = (
    [_pna(C, hs, "hub of 39 in-edges, nodes without in-edges, shuffled edge list" + ("" if hs else "; off = 0 in both kernels"))
     for C in (1, 14, 70) for hs in (True, False)]                 # 203 * 70 = 14 210 threads: 56 workgroups, the last one partial
    + [_pna(14, True, "message rows ldm apart: a column slice of a wider matrix", ldm=20),
       _pna(70, False, "message rows ldm apart, no hself", ldm=77),
       _pna(1, True, "one channel of a three-column matrix", ldm=3)]
    + [_pna(14, True, "ties at the maximum / minimum: the first in edge order takes the gradient", ties=True),
       _pna(70, False, "ties, more than one workgroup, no hself", ties=True),
       _pna(14, False, "ties behind a row stride", ldm=20, ties=True)]
    + [_pna(14, True, "the ordinary case: symmetric sorted molecule edges", graph="mol")]
)


def pna_gen(p):
    g = graph(p["graph"])
    C, ldm = p["C"], p["ldm"] or p["C"]
    gen = rng(21, C, ldm, p["hself"], p["ties"])
    wide = torch.randn(g.E, ldm, generator=gen)
    c0 = (ldm - C + 1) // 2                                        # the slice starts inside the wider matrix (and off a 16-byte boundary)
    msg = wide[:, c0:c0 + C].contiguous()
    if p["ties"]:
        msg = impose_ties(g, msg, gen)
    msg = push_extrema(g, msg)
    wide[:, c0:c0 + C] = msg
    leaves = [msg] + ([torch.randn(g.N, C, generator=gen)] if p["hself"] else [])
    cot = cotangent(0, (g.N, pna_width(C, p["hself"])))
    std = std_columns(C, p["hself"]).to(F64)
    return leaves, dict(g=g, wide=wide, c0=c0, cots={"std-free": [cot * (1 - std)], "std-only": [cot * std]})


def pna_ref(p, aux, msg, hself=None):
    return (pna_restate(aux["g"], msg, hself),)


# ---------------------------------------------------------------------------- PNA with the message formed in the kernel (forward only)
def pna_gather_branch(tower, qe_layer):
    return " | ".join(["k_pna_aggregate_gather", "tower-major" if tower else "block-major", "Qe [E, L*C]" if qe_layer is not None else "Qe [E, C]"])


PNA_GATHER_BRANCHES = {"k_pna_aggregate_gather", "tower-major", "block-major", "Qe [E, L*C]", "Qe [E, C]"}


def _pg(C, tower, qe_layer, hazard, graph="topo"):
    return Row("pna_gather", pna_gather_branch(tower, qe_layer), hazard, C=C, tower=tower, qe_layer=qe_layer, graph=graph)


PNA_GATHER = [
    _pg(14, 0, None, "Ps[src] + Pd[dst] + Qe[e]: src and dst differ in degree on this batch; four in-edges in flight, in-degrees 0 .. 39"),
    _pg(70, 0, None, "more than one workgroup"),
    _pg(1, 0, None, "one channel"),
    _pg(12, 4, None, "tower-major output columns [tower][13 blocks][it]"),
    _pg(70, 14, 0, "tower-major, the first layer's block of Qe [E, L*C]"),
    _pg(70, 70, L_FUSED - 1, "one tower as wide as the layer (it = C), the last layer's block"),
    _pg(14, 0, 1, "block-major from the middle block of Qe [E, L*C]"),
    _pg(12, 4, L_FUSED - 1, "the ordinary case", graph="mol"),
]


def pna_gather_gen(p):
    g = graph(p["graph"])
    C = p["C"]
    gen = rng(22, C, p["tower"], -1 if p["qe_layer"] is None else p["qe_layer"])
    psd, hself = torch.randn(g.N, 2 * C, generator=gen), torch.randn(g.N, C, generator=gen)
    L = 1 if p["qe_layer"] is None else L_FUSED
    qe_all = torch.randn(g.E, L * C, generator=gen)
    lay = p["qe_layer"] or 0
    return [psd, qe_all[:, lay * C:(lay + 1) * C].contiguous(), hself], dict(g=g, qe_all=qe_all, cots={})


def tower_major(out, C, it):
    """block-major [13][C] columns -> tower-major [C / it][13][it]"""
    return out.view(-1, 13, C // it, it).permute(0, 2, 1, 3).reshape(-1, 13 * C)


def pna_gather_ref(p, aux, psd, qe, hself):
    g, C = aux["g"], p["C"]
    out = pna_restate(g, (psd[g.src, :C] + psd[g.dst, C:]) + qe, hself)
    return (tower_major(out, C, p["tower"]) if p["tower"] else out,)


# ============================================================================ sparse edge attention
def edge_scores(g, H, Q, K, Ee):
    dk = Q.shape[1] // H
    Qh, Kh, Eh = (t.view(-1, H, dk) for t in (Q, K, Ee))
    return ((Kh[g.src] * Qh[g.dst]) / dk ** 0.5 * Eh).sum(-1)     # [E, H]


def edge_attention_restate(g, H, Q, K, V, Ee):
    """sn_edge_attention_f32: out[i,h,:] = sum_{j->i} s V[j,h,:] / (sum s + 1e-6), s = exp(clamp(score, -5, 5))"""
    dk = Q.shape[1] // H
    s = torch.exp(edge_scores(g, H, Q, K, Ee).clamp(-5, 5))
    z = torch.zeros(g.N, H, dtype=Q.dtype).index_add(0, g.dst, s)
    wV = torch.zeros(g.N, H, dk, dtype=Q.dtype).index_add(0, g.dst, s[:, :, None] * V.view(-1, H, dk)[g.src])
    return (wV / (z[:, :, None] + 1e-6)).reshape(g.N, H * dk)


def clamp_stats(g, H, Q, K, Ee):
    """float64 -> (min ||score| - 5| in units of rms(score), share of the scores outside [-5, 5])"""
    s = edge_scores(g, H, Q.double(), K.double(), Ee.double())
    return ((s.abs() - 5).abs().min() / s.pow(2).mean().sqrt()).item(), (s.abs() > 5).double().mean().item()


def push_scores(g, H, Q, K, Ee, iters=8):
    """A score within PUSH * rms of +-5 is moved 3 * PUSH * rms further to the side it is on by rescaling the edge's own E[e, h, :], in
    which the score is linear and which no other score reads."""
    dk = Q.shape[1] // H
    for _ in range(iters):
        s = edge_scores(g, H, Q.double(), K.double(), Ee.double())
        rms = s.pow(2).mean().sqrt()
        near = ((s.abs() - 5).abs() < PUSH * rms)
        if not bool(near.any()):
            return Ee
        out = torch.where(s.abs() >= 5, 1.0, -1.0).double()
        f = torch.where(near, 1 + out * 3 * PUSH * rms / s.abs(), torch.ones((), dtype=F64))
        Ee = (Ee.double().view(-1, H, dk) * f[:, :, None]).reshape(Ee.shape).float()
    raise AssertionError("push_scores: scores near the clamp remain")


def edge_attention_branch(layer):
    """sn_edge_attention_f32 and sn_edge_attention_strided_f32 launch the same kernel with the row strides d, d and 3 d, L d"""
    if layer is None:
        return "k_edge_attention | k_edge_attention_bwd_dst | k_edge_attention_bwd_src"
    return "k_edge_attention strided"


EDGE_ATTENTION_BRANCHES = {"k_edge_attention", "k_edge_attention_bwd_dst", "k_edge_attention_bwd_src", "k_edge_attention strided"}
HEAD_SHAPES = ((4, 6), (2, 32), (3, 1), (8, 8))
SHAPE_HAZARD = {(4, 6): "the width of the existing tests", (2, 32): "the widest head the kernel supports: q[32], go[32], aq[32] all live",
                (3, 1): "one channel per head", (8, 8): "N * H = 1624 threads: seven workgroups, the last one partial"}


def _ea(H, dk, scale, layer=None, graph="topo"):
    hz = SHAPE_HAZARD[(H, dk)] + ("; scores mostly inside the clamp" if scale == 1 else "; a share of the scores clamped: no gradient there")
    if layer is not None:
        hz += f"; Q | K | V and E of layer {layer} read in place from the fused projections"
    return Row("edge_attention", edge_attention_branch(layer), hz, H=H, dk=dk, scale=scale, layer=layer, graph=graph)


EDGE_ATTENTION = (
    [_ea(H, dk, sc) for H, dk in HEAD_SHAPES for sc in (1, 3)]
    + [_ea(H, dk, sc, layer=lay) for i, (H, dk) in enumerate(HEAD_SHAPES) for sc, lay in ((1, 0), (3, L_FUSED - 1))]
    + [_ea(4, 6, 3, graph="mol"), _ea(4, 6, 3, layer=L_FUSED - 1, graph="mol")]
)


def edge_attention_gen(p):
    g = graph(p["graph"])
    H, dk = p["H"], p["dk"]
    gen = rng(23, H, dk, p["scale"])                               # (the strided rows read the inputs of the contiguous row of their shape)
    Q, K, V = (torch.randn(g.N, H * dk, generator=gen) for _ in range(3))
    Q = Q * p["scale"]
    Ee = push_scores(g, H, Q, K, torch.randn(g.E, H * dk, generator=gen))
    other = torch.randn(g.E, L_FUSED * H * dk, generator=gen)      # the other layers' blocks of the fused E projection
    cots = {} if p["layer"] is not None else {"": [cotangent(0, (g.N, H * dk))]}
    return [Q, K, V, Ee], dict(g=g, other=other, cots=cots)


def edge_attention_ref(p, aux, Q, K, V, Ee):
    return (edge_attention_restate(aux["g"], p["H"], Q, K, V, Ee),)


# ============================================================================ GAT aggregation
def gat_parts(g, H, relu, feat, al, ar, bias):
    """sn_gat_aggregate_f32 -> (logits before the LeakyReLU [E, H], output before the ReLU [N, H*C]): a = softmax over a node's in-edges
    of leaky_relu(feat_j . attn_l[h] + feat_i . attn_r[h]); out = sum_j a_ij feat[j,h,:] + bias; a node without in-edges gets bias"""
    C = feat.shape[1] // H
    f = feat.view(g.N, H, C)
    el, er = (f * al.view(1, H, C)).sum(-1), (f * ar.view(1, H, C)).sum(-1)
    pre = el[g.src] + er[g.dst]
    e = torch.nn.functional.leaky_relu(pre, SLOPE)
    m = torch.full((g.N, H), -INF, dtype=feat.dtype).scatter_reduce(0, g.dst[:, None].expand(-1, H), e.detach(), "amax")
    w = torch.exp(e - m[g.dst])                                    # (the shift by a constant per node leaves value and gradient unchanged)
    z = torch.zeros(g.N, H, dtype=feat.dtype).index_add(0, g.dst, w)
    out = torch.zeros(g.N, H, C, dtype=feat.dtype).index_add(0, g.dst, (w / z[g.dst])[:, :, None] * f[g.src]).flatten(1)
    return pre, (out if bias is None else out + bias)


def gat_branch(C):
    """sn_gat_aggregate_f32 / sn_gat_aggregate_bwd_f32: C <= 64 -> the one-channel-per-lane forward and the 64-register adjoints, else
    two channels per lane with float64 logits and the 128-register adjoints with renormalised weights"""
    return ("k_gat_aggregate_wave<1> | k_gat_bwd_dst<64> | k_gat_bwd_src<64>" if C <= 64 else
            "k_gat_aggregate_wave<2> | k_gat_bwd_dst<128> | k_gat_bwd_src<128>")


GAT_BRANCHES = {"k_gat_aggregate_wave<1>", "k_gat_bwd_dst<64>", "k_gat_bwd_src<64>", "k_gat_aggregate_wave<2>", "k_gat_bwd_dst<128>",
                "k_gat_bwd_src<128>"}
GAT_SHAPES = ((4, 12), (3, 64), (2, 65), (1, 128), (3, 1))
GAT_HAZARD = {(4, 12): "lanes 12 .. 63 of every wave idle", (3, 64): "the widest head of the one-channel-per-lane kernels",
              (2, 65): "the narrowest head of the two-channel kernels: one lane holds a second channel",
              (1, 128): "the widest head supported: go[128], acc[128] all live", (3, 1): "one channel per head"}
GAT_SEED0, GAT_TRIES = 100, 64


def _gat(H, C, relu, bias, graph="topo"):
    hz = GAT_HAZARD[(H, C)] + "; nodes without in-edges get act(bias) and lse = 0, which the adjoint reads; hub of 39 in-edges"
    return Row("gat", gat_branch(C), hz, H=H, C=C, relu=relu, bias=bias, graph=graph)


GAT = ([_gat(H, C, relu, bias) for H, C in GAT_SHAPES for relu in (True, False) for bias in (True, False)]
       + [_gat(2, 65, True, True, graph="mol"), _gat(4, 12, True, True, graph="mol")])


def gat_draw(g, H, C, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(g.N, H * C, generator=gen), torch.randn(1, H, C, generator=gen), torch.randn(1, H, C, generator=gen),
            torch.randn(H * C, generator=gen)]


def logit_margin(pre):
    return (pre.abs().min() / pre.pow(2).mean().sqrt()).item()


def gat_gen(p):
    """Seeds are walked from a fixed start until no logit is within MARGIN * rms of the LeakyReLU's kink.  (The logits are computed in
    float64 from the float32 inputs the kernel gets: nothing is cast after the check, so MARGIN itself is what is established.)"""
    g = graph(p["graph"])
    H, C = p["H"], p["C"]
    for t in range(GAT_TRIES):
        seed = GAT_SEED0 + 1000 * (H * 131 + C) + t
        feat, al, ar, b = gat_draw(g, H, C, seed)
        pre, out = gat_parts(g, H, p["relu"], feat.double(), al.double(), ar.double(), b.double() if p["bias"] else None)
        if logit_margin(pre) >= MARGIN:
            break
    else:
        raise AssertionError(f"gat_gen: no seed in {GAT_TRIES} tries keeps the logits off zero")
    cot = cotangent(0, out.shape)
    near = torch.zeros_like(out, dtype=torch.bool)
    if p["relu"]:
        # (out == 0 exactly — a node without in-edges and no bias — is no rounding question: the sum is empty in every precision)
        near = (out.abs() < MARGIN * out.pow(2).mean().sqrt()) & (out != 0)
        cot = cot * (~near).to(F64)
    return [feat, al, ar] + ([b] if p["bias"] else []), dict(g=g, seed=seed, near=near, cots={"": [cot]})


def gat_ref(p, aux, feat, al, ar, bias=None):
    out = gat_parts(aux["g"], p["H"], p["relu"], feat, al, ar, bias)[1]
    return (torch.relu(out) if p["relu"] else out,)


# ============================================================================ node rows gathered onto edges
def _gr(C, side, graph="topo"):
    return Row("gather_rows", "k_edge_rows_sum " + ("plan" if side == "dst" else "flipped plan"),
               "h[dst]: the adjoint sums over the in-edge CSR" if side == "dst" else
               "h[src]: the adjoint sums over the CSR of the flipped edge list, which differs from the in-edge CSR on this batch",
               C=C, side=side, graph=graph)


GATHER_ROWS = [_gr(C, side) for C in (1, 10, 70) for side in ("dst", "src")] + [_gr(10, "src", graph="mol")]
GATHER_ROWS_BRANCHES = {"k_edge_rows_sum plan", "k_edge_rows_sum flipped plan"}


def gather_rows_gen(p):
    g = graph(p["graph"])
    return [torch.randn(g.N, p["C"], generator=rng(25, p["C"]))], dict(g=g, cots={"": [cotangent(0, (g.E, p["C"]))]})


def gather_rows_ref(p, aux, h):
    g = aux["g"]
    return (h[g.dst if p["side"] == "dst" else g.src],)


def pna_std(row):
    """-> (bool [width]: the std columns of the row's output, [N, 3 C]: pna_std_bound in the order of out[:, mask])"""
    p = row.p
    leaves, aux = inputs(row)
    g, C = aux["g"], p["C"]
    if row.op == "pna":
        mask, msg, it = std_columns(C, p["hself"]), leaves[0].double(), 0
    else:
        psd, qe = leaves[0].double(), leaves[1].double()
        mask, msg, it = std_columns(C, True), (psd[g.src, :C] + psd[g.dst, C:]) + qe, p["tower"]
    full = torch.zeros(g.N, mask.numel(), dtype=F64)
    full[:, mask] = pna_std_bound(g, msg)
    if it:
        mask, full = tower_major(mask[None, :], C, it)[0], tower_major(full, C, it)
    return mask, full[:, mask]


# ============================================================================ registry
OPS = {
    "pna": AC.Op(PNA, pna_gen, pna_ref, lambda p: pna_branch(p["hself"], p["ldm"], p["C"]), PNA_BRANCHES),
    "pna_gather": AC.Op(PNA_GATHER, pna_gather_gen, pna_gather_ref, lambda p: pna_gather_branch(p["tower"], p["qe_layer"]), PNA_GATHER_BRANCHES,
                        grads=False),
    "edge_attention": AC.Op(EDGE_ATTENTION, edge_attention_gen, edge_attention_ref, lambda p: edge_attention_branch(p["layer"]),
                            EDGE_ATTENTION_BRANCHES),
    "gat": AC.Op(GAT, gat_gen, gat_ref, lambda p: gat_branch(p["C"]), GAT_BRANCHES),
    "gather_rows": AC.Op(GATHER_ROWS, gather_rows_gen, gather_rows_ref,
                         lambda p: "k_edge_rows_sum " + ("plan" if p["side"] == "dst" else "flipped plan"), GATHER_ROWS_BRANCHES),
}
ALL = [r for op in OPS.values() for r in op.cases]


@functools.lru_cache(maxsize=None)
def _inputs(row_id):
    row = next(r for r in ALL if r.id == row_id)
    return OPS[row.op].gen(row.p)


def inputs(row):
    """(leaves, aux) of a row, generated once per process and never modified by the tests"""
    return _inputs(row.id)


def reference(row, dtype):
    """-> (outputs, {cotangent name: gradients of the leaves}) of the restatement in `dtype`; one backward pass per named cotangent"""
    leaves, aux = inputs(row)
    xs = [t.detach().to(dtype).requires_grad_(bool(aux["cots"])) for t in leaves]
    outs = OPS[row.op].ref(row.p, aux, *xs)
    grads = {}
    for name, cot in aux["cots"].items():
        gs = torch.autograd.grad(outs, xs, [c.to(dtype) for c in cot], retain_graph=True)
        grads[name] = list(gs)
    return [o.detach() for o in outs], grads


@functools.lru_cache(maxsize=None)
def _references(row_id):
    row = next(r for r in ALL if r.id == row_id)
    return reference(row, F32), reference(row, F64)


def references(row):
    """((outputs, gradients) in float32, the same in float64), computed once per process"""
    return _references(row.id)
