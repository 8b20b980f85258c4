"""Case tables, dispatch predicates and references of the eval stage-kernel grid (tests/test_stage_grid_gpu.py runs the HIP stage kernels
on them, tests/test_stage_cases_cpu.py checks the conditions that make that comparison mean something).  Importable without a GPU:
models are built on the CPU (parameter holders only) and nothing here touches a device or the package's library.

The whole-stage kernels of the eval forward pick a template instance or a code path from the model (hidden width, layer counts, variant),
the slot count and the batch (graph sizes, edge counts, edge-feature classes):

  phi    sn_phi_fused_f32    csrc/fused_phi.hip   dispatch_phi: NT = ceil(d / 16) x HID1; the plan lays out columns (max_k) or slabs
  rho    sn_rho_fused_f32    csrc/fused_rho.hip   rho_launch + fused.RhoPlan.run: head-padded / natural register attention, k_rho_wide,
                                                  LDS attention, each x ONE
  GINE   sn_gnn_fused_f32    csrc/fused_gnn.hip   gnn_fused_impl: NT; k_gnn_coop: the row-tile form at NT = 8; gnn_graph: the edge-embedding
                                                  mode of every graph (class table / per-edge staging / direct gather)
  DGL    sn_deepsigns_phi_f32 + sn_mlp_chain_f32  dispatch_phi_dgl / dispatch_mlp: the padded widths of dgl_deepsigns._FusedDeepSigns

A row is one (model, batch); its `branch` string joins the names of everything its launches take with " | ", and the `*_branch`
functions restate the host and kernel code (model, batch -> names).  The CPU test asserts predicate(row) == row.branch on the row's actual
batch and that the rows reach every name of the branch sets below.

References: `oracle.pyg_signnet.signnet_gnn(..., out=)` / `oracle.dgl_deepsigns` in float32 and float64 on the same weights, computed
once per row (`reference`) and never modified.
"""
import functools
import types
import zlib

import torch

F32, F64 = torch.float32, torch.float64
DEFAULT_SIZES = (64, 1, 17, 33, 16, 5, 48, 2, 32, 49)      # the 64-node limit, one node, both sides of every 16-row tile edge


class Case:
    def __init__(self, op, name, branch, **p):
        self.op, self.name, self.branch, self.p = op, name, branch, p

    @property
    def id(self):
        return f"{self.op}-{self.name}"

    def __repr__(self):
        return self.id


def cdiv(a, b):
    return (a + b - 1) // b


def seed_of(case, salt=0):
    """one seed per row and use; a row's own `salt` moves its draws (set where a draw left the float32 oracle itself outside REL)"""
    return (zlib.crc32(case.id.encode()) + 7919 * salt + 104729 * case.p.get("salt", 0)) % (2 ** 31)


def branches_of(cases):
    return {b for c in cases for b in c.branch.split(" | ")}


# ============================================================================ batches
def molecule_edges(n):
    """directed edges of synth.make_batch's n-node graph when every chord is placed: a tree plus round(n / 8) chords, both directions"""
    return 2 * ((n - 1) + (int(round(n / 8)) if n > 2 else 0))


@functools.lru_cache(maxsize=None)
def _batch(sizes, features, keep_edges, complete):
    """synth.make_batch(sizes=...); keep_edges ((graph, ne), ...): only the first ne edges of that graph stay; complete: every graph's
    edge set is replaced by all ordered pairs of its nodes (the eigenvectors stay the molecule's: they are an input like any other)"""
    from signnet_basisnet_amd import synth
    data = synth.make_batch(len(sizes), seed=4211 + len(sizes), sizes=list(sizes), features=features)
    if complete:
        ei, off = [], 0
        for n in sizes:
            a = torch.arange(n).repeat_interleave(n)
            b = torch.arange(n).repeat(n)
            ei.append(torch.stack([a[a != b], b[a != b]]) + off)
            off += n
        data.edge_index = torch.cat(ei, 1).contiguous()
        E, g = data.edge_index.shape[1], torch.Generator().manual_seed(977)
        data.edge_attr = torch.randint(1, 4, (E,), generator=g) if features == "zinc" else torch.rand(E, 4, generator=g)
    if keep_edges:
        gid = data.batch[data.edge_index[1]]
        keep = torch.ones(gid.numel(), dtype=torch.bool)
        for g, ne in keep_edges:
            idx = (gid == g).nonzero().view(-1)
            assert idx.numel() >= ne, f"graph {g} has {idx.numel()} edges, {ne} wanted"
            keep[idx[ne:]] = False
        data.edge_index = data.edge_index[:, keep].contiguous()
        data.edge_attr = data.edge_attr[keep].contiguous()
    return data


def batch_of(case):
    """the row's host batch (shared between the rows of one batch: never modified)"""
    p = case.p
    return _batch(tuple(p["sizes"]), "alchemy" if p["variant"] == "alchemy" else "zinc", tuple(sorted((p.get("keep_edges") or {}).items())),
                  bool(p.get("complete")))


def reorder(data, order):
    """-> (the same batch with its graphs in `order`, perm): node row i of the new batch is node row perm[i] of `data`"""
    sizes = list(data.sizes)
    B = len(sizes)
    start = [sum(sizes[:g]) for g in range(B)]
    vstart = [sum(s * s for s in sizes[:g]) for g in range(B)]
    perm = torch.cat([torch.arange(start[g], start[g] + sizes[g]) for g in order])
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.numel())
    out = types.SimpleNamespace(**vars(data))
    out.sizes = [sizes[g] for g in order]
    out.x, out.eigen_values = data.x[perm].contiguous(), data.eigen_values[perm].contiguous()
    out.eigen_vectors = torch.cat([data.eigen_vectors[vstart[g]:vstart[g] + sizes[g] ** 2] for g in order])
    out.batch = torch.repeat_interleave(torch.arange(B), torch.tensor(out.sizes))
    if data.edge_index.numel():
        gid = data.batch[data.edge_index[1]]
        eperm = torch.cat([(gid == g).nonzero().view(-1) for g in order])
        out.edge_index = inv[data.edge_index[:, eperm]].contiguous()
        out.edge_attr = data.edge_attr[eperm].contiguous()
    return out, perm


# ============================================================================ dispatch predicates
N_HEAD = 4
GNN_ROWS, GNN_EMAX, GNN_CLS, GNN_EEMAX, SP_IMAGE = 64, 192, 16, 96, 52224


def gnn_ee_rows(nt, edge_words):
    """csrc/gnn_front.hpp: rows of the stage kernel's LDS edge-embedding area at width 16 * nt"""
    LD = 16 * nt + 4
    base = 2 * SP_IMAGE + (GNN_ROWS + 1) * LD * 4 + (GNN_ROWS + 4 + GNN_EMAX * (3 + edge_words) + GNN_CLS) * 4
    cap = 160 * 1024 - 512
    room = cap - base if base < cap else 0
    return max(0, min(room // (LD * 4) - 1, GNN_EEMAX))


def phi_branch(p):
    """dispatch_phi: launch_phi<NT, HID1>, NT = ceil(d / 16), HID1 = the first hidden width is 1 (GINESignNetPyG's Linear(1, 1); Alchemy's
    first Linear is [d, 1]).  sn_batch_plan packs phi's bins into columns when kmax > 0 and into slabs with all eigenvectors."""
    return f"k_phi_fused<{cdiv(p['hid'], 16)},{'HID1' if p['variant'] == 'gine' else '!HID1'}> {'columns' if p['max_k'] else 'slabs'}"


def has_eig_encoder(p):
    return p["variant"] == "alchemy"


def slot_count(p):
    """K of the forward: max_k, or the largest graph with all eigenvectors"""
    return p["max_k"] or max(p["sizes"])


def rho_branch(p):
    """fused.RhoPlan.run + rho_launch"""
    d, K, kmax = p["hid"], slot_count(p), p["max_k"] or 0
    kcap = min(kmax, K) if kmax > 0 else K
    one = "ONE" if (p["nl_rho"] == 1 and not has_eig_encoder(p)) else "!ONE"
    dk = d // N_HEAD
    head_pad = 0 if dk % 16 == 0 else 16 * cdiv(dk, 16)
    if head_pad and kcap <= 16:                       # RhoPlan.run picks the head-padded packing
        return f"k_rho_fused<{4 if head_pad == 16 else 8},reg,{one},HP{head_pad}>"
    regattn = kcap <= 16 and dk % 16 == 0
    if not regattn and d in (64, 128):
        return f"k_rho_wide<{d // 16},{one},{'COLS' if kmax == 0 else '!COLS'}>"
    return f"k_rho_fused<{cdiv(d, 16)},{'reg' if regattn else 'lds'},{one}>"


def graph_edge_stats(data):
    """per graph: (in-edges, distinct edge-feature tuples among them)"""
    B = len(data.sizes)
    if not data.edge_index.numel():
        return [(0, 0)] * B
    gid = data.batch[data.edge_index[1]]
    ea = data.edge_attr.reshape(gid.numel(), -1)
    out = []
    for g in range(B):
        rows = ea[gid == g]
        out.append((rows.shape[0], int(torch.unique(rows, dim=0).shape[0]) if rows.shape[0] else 0))
    return out


def gnn_branches(p, data):
    """gnn_fused_impl (NT), k_gnn_coop (row-tile form at NT = 8) and gnn_graph (edge-embedding mode) for every graph of the batch"""
    nt, L = cdiv(p["hid"], 16), p["nl_gnn"]
    discrete = p["variant"] == "gine"
    ee_rows = gnn_ee_rows(nt, (1 if discrete else 4) if L > 0 else 0) if L > 0 else 0
    names = {f"gnn {'discrete' if discrete else 'continuous'} n_out={1 if discrete else 12}"}
    for n, (ne, ncls) in zip(data.sizes, graph_edge_stats(data)):
        assert 1 <= n <= GNN_ROWS and ne <= GNN_EMAX, "beyond the stage's limits"
        if L == 0:
            mode = "no layers"
        elif ncls <= GNN_CLS and L * ncls <= ee_rows:
            mode = "use_tab"
        elif ne <= ee_rows:
            mode = "use_ee"
        else:
            mode = "gather"
        names.add(f"gnn<{nt}>{f' T={(n + 15) >> 4}' if nt == 8 else ''} {mode}")
    return names


def pyg_branch(p):
    return " | ".join([phi_branch(p), rho_branch(p)] + sorted(gnn_branches(p, batch_of(types.SimpleNamespace(p=p)))))


ONES = ("ONE", "!ONE")
PHI_BRANCHES = {f"k_phi_fused<{nt},{h}> {lay}" for nt in range(1, 9) for h in ("HID1", "!HID1") for lay in ("columns", "slabs")}
RHO_BRANCHES = ({f"k_rho_fused<4,reg,{o},HP16>" for o in ONES} | {f"k_rho_fused<8,reg,{o},HP32>" for o in ONES} |
                {f"k_rho_fused<{nt},reg,{o}>" for nt in (4, 8) for o in ONES} |
                {f"k_rho_wide<{nt},{o},{c}>" for nt in (4, 8) for o in ONES for c in ("COLS", "!COLS")} |
                {f"k_rho_fused<{nt},lds,{o}>" for nt in range(1, 9) for o in ONES})
# dispatch_rho<true, ...>(nt) is natural register attention: d / 4 a multiple of 16.  With the four heads the modules are built with
# that is d = 64 or 128 only (nt 4 and 8); every other width with <= 16 slots takes the head-padded packing (RhoPlan.run).
UNREACHABLE = {f"k_rho_fused<{nt},reg,{o}>" for nt in (1, 2, 3, 5, 6, 7) for o in ONES}
GNN_MODES = ("use_tab", "use_ee", "gather")
GNN_BRANCHES = ({f"gnn<{nt}> {m}" for nt in range(1, 8) for m in GNN_MODES} | {f"gnn<8> T={T} {m}" for T in (1, 2, 3, 4) for m in GNN_MODES} |
                {"gnn<4> no layers", "gnn discrete n_out=1", "gnn continuous n_out=12"})
PYG_BRANCHES = PHI_BRANCHES | RHO_BRANCHES | GNN_BRANCHES


# ============================================================================ the SignNetGNN table
def _r(variant, hid, max_k, nl_rho=None, nl_phi=2, nl_gnn=2, sizes=DEFAULT_SIZES, keep_edges=None, complete=False, tag="", salt=0):
    if nl_rho is None:
        nl_rho = 1 if variant == "gine" else 2
    p = dict(variant=variant, hid=hid, max_k=max_k, nl_rho=nl_rho, nl_phi=nl_phi, nl_gnn=nl_gnn, sizes=tuple(sizes), keep_edges=keep_edges,
             complete=complete, salt=salt)
    name = f"{variant}-h{hid}-k{max_k or 'all'}-rho{nl_rho}" + (f"-phi{nl_phi}" if nl_phi != 2 else "") + (f"-gnn{nl_gnn}" if nl_gnn != 2 else "") + \
           (f"-{tag}" if tag else "")
    return Case("pyg", name, pyg_branch(p), **p)


PHI_WIDTHS = (4, 16, 20, 32, 48, 64, 80, 96, 108, 112, 128)
RHO_HP16, RHO_HP32, RHO_NATURAL = (4, 20, 48, 60), (68, 80, 96, 112, 124), (64, 128)
RHO_LDS = (20, 32, 48, 60, 80, 96, 108, 124)
MAX16, MAX17 = (16, 1, 9, 5, 16, 12), (17, 1, 9, 5, 16, 12)


def ee_batch(hid, edge_words=4):
    """graphs whose in-edge count sits on both sides of the width's ee_rows (row-tile forms 2, 2, 3, 4 at d = 128)"""
    R = gnn_ee_rows(cdiv(hid, 16), edge_words)
    n0 = min(n for n in range(2, 65) if molecule_edges(n) >= R + 1)
    return (n0, n0, 40, 64), {0: R, 1: R + 1, 2: R, 3: R}


def _pyg_rows():
    rows = []
    # phi: every tile count, full and part-filled last tile x HID1 / !HID1 x columns (max_k 7, 16) / slabs.  The same rows give rho's
    # head-padded, natural and LDS-attention kernels with ONE (gine: one layer, no encoder) and !ONE (alchemy: eigenvalue encoder) and
    # every NT of the GINE stage with discrete and continuous features
    for variant in ("gine", "alchemy"):
        for hid in PHI_WIDTHS:
            for k in (7, 16, None):
                rows.append(_r(variant, hid, k))
    rows.append(_r("gine", 128, 16, nl_phi=8))
    # rho widths the phi list does not have, and !ONE from two layers without an eigenvalue encoder at every register-attention width
    for hid in (60, 68, 124):
        rows += [_r("gine", hid, 16), _r("alchemy", hid, 7)]
    for hid in RHO_HP16 + RHO_HP32 + RHO_NATURAL:
        rows.append(_r("gine", hid, 16, nl_rho=2))
    # LDS attention at 4 and 8 tiles (64 / 128 take k_rho_wide).  (salt: with the first draw of gine-h60-kall the float32 oracle's own y
    # is 1.8e-5 from float64 — test_stage_cases_cpu.py would fail, and the row could not hold a kernel to 1e-5)
    for hid in (60, 124):
        rows += [_r("gine", hid, None, salt=int(hid == 60)), _r("alchemy", hid, None)]
    # k_rho_wide: per-graph bins (16 < max_k < n) with ONE / !ONE; COLS x ONE / !ONE are the all-eigenvector rows above
    for hid in (64, 128):
        rows += [_r("gine", hid, 20), _r("alchemy", hid, 20), _r("gine", hid, None, nl_rho=2)]
    # the kcap 16 / 17 boundary: max_k 17 next to the max_k 16 rows above, and all eigenvectors with a largest graph of 16 / 17 nodes
    for hid in (80, 64):
        rows += [_r("gine", hid, 17), _r("alchemy", hid, 17)]
        for sizes, tag in ((MAX16, "max16"), (MAX17, "max17")):
            rows += [_r("gine", hid, None, sizes=sizes, tag=tag), _r("alchemy", hid, None, sizes=sizes, tag=tag)]
    # GINE at d = 128: one graph per row-tile form, both sides of every 16-row edge
    for n in (16, 17, 32, 33, 48, 49, 64):
        rows.append(_r("gine", 128, 16, sizes=(n,), tag=f"n{n}"))
    # continuous features around ee_rows (per-edge staging / direct gather), also with 33-48 and 49-64 nodes
    for hid in (128, 96):
        sizes, keep = ee_batch(hid)
        rows.append(_r("alchemy", hid, 16, sizes=sizes, keep_edges=keep, tag="ee"))
    # discrete features with n_layers * ncls > ee_rows (no class table), thinned graphs for the staging mode at every row-tile form
    rows.append(_r("gine", 128, 16, nl_gnn=14))
    R1 = gnn_ee_rows(8, 1)
    rows.append(_r("gine", 128, 16, nl_gnn=14, sizes=(16, 17, 40, 64), keep_edges={2: R1, 3: R1 - 1}, tag="ee"))
    # (below 8 tiles ee_rows >= 53 > 16 layers x the 3 bond classes: discrete features always take the class table there)
    # direct gather in the one-row-tile form: more in-edges than ee_rows on <= 16 nodes needs graphs denser than molecules
    rows += [_r("alchemy", 128, 7, sizes=(8, 12, 14), complete=True, tag="complete"),
             _r("gine", 128, 7, nl_gnn=14, sizes=(8, 12, 14), complete=True, tag="complete")]
    rows.append(_r("gine", 64, 16, nl_gnn=0))
    return rows


PYG = _pyg_rows()


# ---------------------------------------------------------------------------- models and references
def ctor_of(p):
    if p["variant"] == "gine":
        return (None, None, p["hid"], 1, p["nl_phi"], p["nl_gnn"])
    return (6, 4, p["hid"], 12, p["nl_phi"], p["nl_gnn"])


def randomize(model, seed):
    """no identity anywhere: BatchNorm running statistics (parity_util.bn_randomize's draws) and affine, LayerNorm affine, GIN / GINE eps"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, mod in model.named_modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(torch.randn(mod.running_mean.shape, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.running_var.shape, generator=g) + 0.5)
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
            elif isinstance(mod, torch.nn.LayerNorm):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
        for name, prm in model.named_parameters():
            if name.endswith(".eps") and prm.numel() == 1:
                prm.copy_(0.6 * torch.rand(1, generator=g) - 0.3)


def build_model(case):
    """the row's SignNetGNN on the CPU (parameter holders; .cuda() runs it).  The reference constructors fix the rho depth (1 / 4); a
    row that names another depth gets a SetTransformer of that depth, as the fused stage takes any depth up to 8."""
    from signnet_basisnet_amd import pyg
    p = case.p
    torch.manual_seed(seed_of(case))
    m = pyg.SignNetGNN(*ctor_of(p), variant=p["variant"], max_k=p["max_k"])
    if p["nl_rho"] != m.nl_rho:
        m.sign_net.rho = pyg.SetTransformer(p["hid"], p["nl_rho"], p["variant"])
        m.nl_rho = p["nl_rho"]
    randomize(m, seed_of(case, 1))
    return m.eval()


def oracle_cfg(p):
    from oracle import pyg_signnet as O
    cfg = O.make_cfg(p["variant"], *ctor_of(p))
    cfg["nl_rho"] = p["nl_rho"]
    return cfg


def to_f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def data_f64(data):
    out = types.SimpleNamespace(**vars(data))
    for k, v in vars(data).items():
        if torch.is_tensor(v) and v.is_floating_point():
            setattr(out, k, v.double())
    return out


STAGES = ("phi", "rho_sum", "y")


@functools.lru_cache(maxsize=4)
def reference(case):
    """-> (state_dict, {stage: float32 value}, {stage: float64 value}, mask [N, K]) of the row, from oracle.pyg_signnet; phi [N, K, d],
    rho_sum [N, d], y [B, n_out]"""
    from oracle import pyg_signnet as O
    p = case.p
    sd = {k: v.detach().clone() for k, v in build_model(case).state_dict().items()}
    cfg, data = oracle_cfg(p), batch_of(case)
    o32, o64 = {}, {}
    with torch.no_grad():
        O.signnet_gnn(sd, cfg, data, training=False, max_k=p["max_k"], out=o32)
        O.signnet_gnn(to_f64(sd), cfg, data_f64(data), training=False, max_k=p["max_k"], out=o64)
    assert o32["phi"].shape[1] == slot_count(p), "rows keep max_k <= the largest graph: the oracle's K is the forward's"
    return sd, {s: o32[s] for s in STAGES}, {s: o64[s] for s in STAGES}, o32["mask"]


# ============================================================================ the DGL DeepSigns table
def dgl_widths(p):
    """dgl_deepsigns._FusedDeepSigns: the padded width of the phi stage and of the rho chain"""
    hidden, out, K = p["hidden"], p["out"], p["K"]
    dp = max(48, 16 * cdiv(max(hidden, out), 16))
    rdims = [out if p["kind"] == "masked_gin" else K * out] + [hidden] * (p["layers"] - 1) + [K]
    rp = max(48, 16 * cdiv(max(rdims), 16))
    return dp, rp


def dgl_branch(p):
    """dispatch_phi_dgl: launch_phi<dp / 16, false, DGL>; dispatch_mlp: launch_mlp<rp / 16> (with the masked slot sum in front for
    MaskedGINDeepSigns)"""
    dp, rp = dgl_widths(p)
    assert 48 <= dp <= 112 and rp <= 128 and p["K"] <= 64, "the layer path would serve this row"
    return f"k_phi_fused<{dp // 16},!HID1,DGL> | k_mlp_chain<{rp // 16}>{' masked' if p['kind'] == 'masked_gin' else ''}"


def _d(kind, hidden, out, K, layers=2):
    p = dict(kind=kind, hidden=hidden, out=out, K=K, layers=layers, sizes=DEFAULT_SIZES, variant="gine")
    return Case("dgl", f"{kind}-h{hidden}-c{out}-k{K}", dgl_branch(p), **p)


DGL_K = (1, 8, 37, 64)
DGL_HIDDEN = {40: 48, 64: 64, 67: 80, 95: 96, 100: 112}          # hidden width -> the width it pads to
DGL = ([_d("gin", h, 2 if K > 37 else (3 if K == 37 else 4), K) for h in DGL_HIDDEN for K in DGL_K] +      # (k * phi_out <= 128)
       [_d("masked_gin", h, c, K) for h, c in ((40, 40), (64, 4), (67, 67), (95, 17), (100, 100)) for K in DGL_K])
DGL_BRANCHES = ({f"k_phi_fused<{nt},!HID1,DGL>" for nt in range(3, 8)} | {f"k_mlp_chain<{nt}>" for nt in range(3, 9)} |
                {f"k_mlp_chain<{nt}> masked" for nt in range(3, 8)})


def build_dgl(case):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    p = case.p
    torch.manual_seed(seed_of(case))
    net = DS.get_sign_inv_net(dict(sign_inv_net=p["kind"], hidden_dim=p["hidden"], phi_out_dim=p["out"], sign_inv_layers=p["layers"],
                                   pos_enc_dim=p["K"], dropout=0.0, sign_inv_activation="relu", device="cpu"))
    randomize(net, seed_of(case, 1))
    return net.eval()


@functools.lru_cache(maxsize=4)
def dgl_reference(case):
    """-> (state_dict, pos_enc [N, K, 1], y float32, y float64) from oracle.dgl_deepsigns"""
    from oracle import dgl_deepsigns as OD
    from signnet_basisnet_amd import synth
    p = case.p
    data = batch_of(case)
    sd = {k: v.detach().clone() for k, v in build_dgl(case).state_dict().items()}
    x = synth.dgl_pos_enc(data, p["K"]).unsqueeze(-1)
    ei, sizes = data.edge_index, torch.tensor(data.sizes)
    with torch.no_grad():
        if p["kind"] == "gin":
            y32 = OD.gin_deepsigns(sd, ei[0], ei[1], x, p["layers"], p["K"])
            y64 = OD.gin_deepsigns(to_f64(sd), ei[0], ei[1], x.double(), p["layers"], p["K"])
        else:
            y32 = OD.masked_gin_deepsigns(sd, ei[0], ei[1], sizes, x, p["layers"], p["K"])
            y64 = OD.masked_gin_deepsigns(to_f64(sd), ei[0], ei[1], sizes, x.double(), p["layers"], p["K"])
    return sd, x, y32, y64


ALL = PYG + DGL
