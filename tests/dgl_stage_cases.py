"""Case tables, dispatch predicates and references of the DGL one-launch net grid (tests/test_dgl_stage_grid_gpu.py runs the three
eval-mode kernels on them, tests/test_dgl_stage_cases_cpu.py checks the conditions that make that comparison mean something).  Importable
without a GPU: nets are built on the CPU (parameter holders only) and nothing here touches a device or the package's library.

  GIN          sn_gin_net_fused_f32          k_gnn_coop<4|6|8, MODE=1>  csrc/fused_gnn.hip, fused_gnn_graph.hpp   dgl_nets._FusedGin
  Transformer  sn_transformer_net_fused_f32  k_gnn_coop<4, MODE=2>      the same files                            dgl_nets._FusedTransformer
  GatedGCN     sn_gatedgcn_fused_f32         k_gatedgcn_net<3|4|5|6>    csrc/fused_gated.hip                      dgl_nets._FusedGated

A row is one (net, batch).  Its batch is a tuple of graph specs (kind, n, ne) — node and in-edge count stated literally, "EMAX" for
sn_gatedgcn_max_edges(d) — built as explicit, shuffled, directed edge lists; every graph's edges, atom / bond types and positional
encoding are drawn from (row, graph index) alone, so the same graph is the same data wherever it stands in a batch (reversed order,
the cyclic repeats of the persistent-loop rows).  `branch` joins the names of everything the row's launch takes with " | "; the
`*_branch` functions restate the host code (net, batch -> names): the packers' `ok` rules and padded widths, the switches of the two
entry points, `_DGLNet._stage`'s limits and the kernels' own per-graph choices (row-tile count, edge passes).

References: oracle.dgl_nets.gin_net / gatedgcn_net / transformer_net on the row's state_dict in float32 and float64, computed once per
row (`reference`) and never modified.  The positional encoding is a seeded random [N, pos_enc_dim] tensor handed to the net directly
(lap_method 'none': no sign_inv_net is built), so only the stage kernel is under test.
"""
import functools

import numpy as np
import torch

import parity_util as PU
from stage_cases import Case, branches_of, cdiv, seed_of

F32, F64 = torch.float32, torch.float64
CUS = 256                    # the CU count the persistent-loop rows are written for (MI355X); the GPU test takes the device's own
ROWS, GNN_EMAX, GNN_MAX_LAYERS = 64, 192, 16          # _DGLNet._stage / fused.GNN_MAX_LAYERS (SN_GNN_MAX_LAYERS)
N_ATOM, N_BOND = 28, 4


# ============================================================================ graphs and batches
def gated_max_edges(d):
    """csrc/fused_gated.hip GGCfg<NT>::EMAX (sn_gatedgcn_max_edges): what is left of 160 KB of LDS behind the three-chunk weight ring
    (fused_common.hpp WRing<NT>: 3 x (3 ceil(NT / 2) + SN_SPLIT_EPI) KB), the Bh | Dh | Eh image and the readout scratch, per in-edge a
    gate row and 6 bytes of tables; capped at 192, else rounded down to 16.  The GPU test asserts the library returns the same."""
    nt = max(3, cdiv(d, 16))
    if nt > 6:
        return 0
    D = 16 * nt
    ring = 3 * (3 * ((nt + 1) // 2) + 3) * 1024
    raw = (160 * 1024 - ring - ROWS * (3 * D + 4) * 4 - (4 * D * 4 + 1024)) // ((D + 4) * 4 + 6)
    return 192 if raw > 192 else raw // 16 * 16


def resolve(spec, emax):
    kind, n, ne = spec
    return kind, n, (emax if ne == "EMAX" else ne)


def graph_edges(kind, n, ne, rng):
    """[ne, 2] (src, dst) local, directed, shuffled.  none: no edge; cycle: i -> i + 1 mod n; star: hub 0 and n - 1 leaves, both
    directions (n - 1 in-edges at the hub); rand: ne random ordered pairs — a multigraph — with a self loop at node 0, one repeated
    edge and a self loop at the LAST node (in CSR order it stands in the last edge pass with source row n - 1)."""
    if kind == "none":
        e = np.zeros((0, 2), dtype=np.int64)
    elif kind == "cycle":
        e = np.array([(i, (i + 1) % n) for i in range(n)], dtype=np.int64)
    elif kind == "star":
        a = np.array([(0, i) for i in range(1, n)], dtype=np.int64).reshape(-1, 2)
        e = np.concatenate([a, a[:, ::-1]], 0)
    else:
        assert kind == "rand", kind
        e = rng.integers(0, n, size=(ne, 2)).astype(np.int64)
        if ne >= 1:
            e[0] = (0, 0)
        if ne >= 4:
            e[2] = e[1]
        if ne >= 2:
            e[-1] = (n - 1, n - 1)
    assert e.shape[0] == ne, f"{kind}: {e.shape[0]} edges built, {ne} stated"
    return e[rng.permutation(e.shape[0])]


@functools.lru_cache(maxsize=None)
def _graph(case, j, emax):
    """graph j of the row: (n, edges [ne, 2], atom types [n], bond types [ne], positional encoding [n, K] float32)"""
    kind, n, ne = resolve(case.p["graphs"][j], emax)
    rng = np.random.default_rng(seed_of(case, 3) + 31 * j)
    e = graph_edges(kind, n, ne, rng)
    return (n, torch.from_numpy(np.ascontiguousarray(e)), torch.from_numpy(rng.integers(0, N_ATOM, n)), torch.from_numpy(rng.integers(0, N_BOND, ne)),
            torch.from_numpy(rng.standard_normal((n, case.p["K"])).astype(np.float32)))


def default_emax(case):
    return gated_max_edges(case.p["hidden"]) if case.op == "gated" else None


def assemble(case, order=None, emax=None, extra=()):
    """-> dict(src, dst [E], sizes, edge_counts [B], h [N], e [E], p [N, K]): the row's graphs in `order` (indices into the row's specs,
    default: as stated), then `extra` graphs given as _graph tuples"""
    emax = default_emax(case) if emax is None else emax
    order = range(len(case.p["graphs"])) if order is None else order
    gs = [_graph(case, j, emax) for j in order] + list(extra)
    off, src, dst = 0, [], []
    for n, e, *_ in gs:
        src.append(e[:, 0] + off)
        dst.append(e[:, 1] + off)
        off += n
    return dict(src=torch.cat(src), dst=torch.cat(dst), sizes=torch.tensor([g[0] for g in gs]), edge_counts=torch.tensor([g[1].shape[0] for g in gs]),
                h=torch.cat([g[2] for g in gs]), e=torch.cat([g[3] for g in gs]), p=torch.cat([g[4] for g in gs]))


def oversize_graph(case, ne):
    """a 20-node random graph with `ne` in-edges (the guard rows: one more than the kernel holds), drawn like the row's own"""
    rng = np.random.default_rng(seed_of(case, 5))
    n = 20
    return (n, torch.from_numpy(graph_edges("rand", n, ne, rng)), torch.from_numpy(rng.integers(0, N_ATOM, n)), torch.from_numpy(rng.integers(0, N_BOND, ne)),
            torch.from_numpy(rng.standard_normal((n, case.p["K"])).astype(np.float32)))


def batch_order(case, cus=CUS):
    """the order of the row's launch: the stated graphs once, or — persistent-loop rows — B = CUs + 40 graphs: the first CUs cyclically,
    then, at index w + CUs (the second graph of workgroup w: launch_gated's grid is min(B, CUs), the kernel strides by it), the graph
    AFTER the one at index w — so no workgroup meets in its second graph the tables, images and counts its first one left in LDS,
    whatever the CU count; in reversed order a workgroup goes from graph j + 1 to graph j"""
    k = len(case.p["graphs"])
    if not case.p.get("repeat_beyond_cus"):
        return list(range(k))
    return [i % k for i in range(cus)] + [(w % k + 1) % k for w in range(case.p["repeat_beyond_cus"])]


def second_graphs(order, cus):
    """[(first graph, second graph)] of every workgroup that takes two: indices into the row's specs (grid = cus, stride = cus)"""
    assert cus < len(order) <= 2 * cus
    return [(order[w], order[w + cus]) for w in range(len(order) - cus)]


def check_second_graphs(case, order, cus, reverse=False):
    """what the persistent-loop rows are for: every second graph differs from the first, and the transitions go from no edge to more
    than one 64-edge pass, from two passes to one, from more nodes to fewer (reversed order: the opposite directions)"""
    specs = [resolve(s, default_emax(case)) for s in case.p["graphs"]]
    pairs = second_graphs(order, cus)
    assert len(pairs) == case.p["repeat_beyond_cus"] and all(a != b for a, b in pairs), pairs
    ne = [(specs[b][2], specs[a][2]) if reverse else (specs[a][2], specs[b][2]) for a, b in pairs]
    nn = [(specs[b][1], specs[a][1]) if reverse else (specs[a][1], specs[b][1]) for a, b in pairs]
    assert any(a == 0 and b > 64 for a, b in ne) and any(a > 64 and 0 < b < 64 for a, b in ne) and any(a > 0 and b == 0 for a, b in ne), ne
    assert any(a > b for a, b in nn) and any(a < b for a, b in nn), nn


# ============================================================================ dispatch predicates
# dgl_nets._DGLNet._stage (dgl_nets.py:277-289): no graph above 64 nodes, none with more in-edges than 192 (GatedGCN: max_edges)
def within_stage(p, emax, limit):
    gs = [resolve(s, emax) for s in p["graphs"]]
    return 0 < max(n for _, n, _ in gs) <= ROWS and max(ne for _, _, ne in gs) <= limit


def gin_dp(p):
    """dgl_nets._FusedGin.__init__ (dgl_nets.py:324-337) -> (ok, dp, kp): the widest of hidden, every conv's two Linears, the readout's
    hidden widths and kp pads to 64 | 96 | 128; ok False above 128 or with more than 16 layers"""
    hid, out, L = p["hidden"], p["out_dim"], p["L"]
    kp = 1 if p["pe"] == "no_pe" else p["K"]
    dmax = max([hid, out, out // 2, out // 4, kp])
    ok = dmax <= 128 and 1 <= L <= GNN_MAX_LAYERS
    return ok, (64 if dmax <= 64 else (96 if dmax <= 96 else 128)), kp


def coop_graph_names(nt, mode, p, emax=None):
    """gnn_graph<NT, MODE> (fused_gnn_graph.hpp) per graph: T = ceil(n / 16) row tiles of the 64-row image; no in-edge; all 192 staged"""
    k = f"k_gnn_coop<{nt},{mode}>"
    names = set()
    for _, n, ne in (resolve(s, emax) for s in p["graphs"]):
        names.add(f"{k} T={cdiv(n, 16)}")
        if ne == 0:
            names.add(f"{k} ne=0")
        if ne == GNN_EMAX:
            names.add(f"{k} ne=192")
    return names


def gin_branch(p):
    """_FusedGin + sn_gin_net_fused_f32's switch (fused_gnn.hip:489-493: ceil(dp / 16) <= 4 -> <4,1>, 5..6 -> <6,1>, else <8,1>)"""
    ok, dp, kp = gin_dp(p)
    if p["L"] > GNN_MAX_LAYERS:
        return "layer path: more than 16 layers"
    if not ok:
        return "layer path: wider than 128"
    if not within_stage(p, None, GNN_EMAX):
        return "layer path: a graph beyond 64 nodes / 192 in-edges"
    nt = 4 if cdiv(dp, 16) <= 4 else (6 if cdiv(dp, 16) <= 6 else 8)
    return " | ".join(sorted(coop_graph_names(nt, 1, p) | {f"k_gnn_coop<{nt},1> kp={'1 (no_pe)' if p['pe'] == 'no_pe' else 'K'}"}))


GIN_BRANCHES = ({f"k_gnn_coop<{nt},1> T={T}" for nt in (4, 6, 8) for T in (1, 2, 3, 4)} |
                {f"k_gnn_coop<{nt},1> {e}" for nt in (4, 6, 8) for e in ("ne=0", "ne=192", "kp=K", "kp=1 (no_pe)")} |
                {"layer path: more than 16 layers", "layer path: wider than 128", "layer path: a graph beyond 64 nodes / 192 in-edges"})


def gated_dp(p):
    """dgl_nets._FusedGated.__init__ (dgl_nets.py:554-565) -> (why not | None, dp): hidden a multiple of 4 in [4, 96], every layer
    hidden -> hidden but the last, whose out_dim may be anything up to dp = max(48, 16 ceil(d / 16)); readout widths <= 128"""
    d, out = p["hidden"], p["out_dim"]
    dp = max(48, 16 * cdiv(d, 16))
    if d > 96:
        return "hidden above 96", dp
    if d < 4 or d % 4:
        return "hidden not a multiple of 4", dp
    if p["L"] > 32:
        return "more than 32 layers", dp
    if out > dp:
        return "out_dim above the padded width", dp
    return None, dp


def gated_branch(p, cus=CUS):
    """_FusedGated + sn_gatedgcn_fused_f32's switch (fused_gated.hip:344, 357-362: NT = max(3, ceil(d / 16))) + k_gatedgcn_net's per-graph
    edge passes (npass = ceil(ne / 64); ne = 0: the A|B|D|E GEMM prefetches the next layer's weights instead of wc) + launch_gated's
    grid = min(B, CUs) (a workgroup whose graph index + grid < B takes a second graph)"""
    why, dp = gated_dp(p)
    if why:
        return f"layer path: {why}"
    d = p["hidden"]
    emax = gated_max_edges(d)
    if not within_stage(p, emax, emax):
        return "layer path: a graph beyond 64 nodes / max_edges in-edges"
    k = f"k_gatedgcn_net<{dp // 16}>"
    names = set()
    for _, n, ne in (resolve(s, emax) for s in p["graphs"]):
        names.add(f"{k} ne=0" if ne == 0 else f"{k} npass={cdiv(ne, 64)}")
        if ne == emax:
            names.add(f"{k} ne=EMAX")
    if p.get("repeat_beyond_cus"):
        names.add(f"{k} second graph")
    if d < 48:
        names.add("hidden below 48: zero-padded")
    elif d % 16:
        names.add("hidden cuts the last 16-column tile")
    out = p["out_dim"]
    names.add("d_out = d" if out == d else ("d_out < d" if out < d else "d_out in (d, dp]"))
    names.add("residual" if p["residual"] else "no residual")
    return " | ".join(sorted(names))


GATED_BRANCHES = ({f"k_gatedgcn_net<{nt}> {e}" for nt in (3, 4, 5, 6) for e in ("ne=0", "npass=1", "npass=2", "ne=EMAX", "second graph")} |
                  {f"k_gatedgcn_net<{nt}> npass=3" for nt in (3, 4, 5)} |          # (EMAX = 112 at 96 columns: two passes at most)
                  {"hidden below 48: zero-padded", "hidden cuts the last 16-column tile", "d_out = d", "d_out < d", "d_out in (d, dp]", "residual",
                   "no residual"} |
                  {f"layer path: {w}" for w in ("hidden above 96", "hidden not a multiple of 4", "out_dim above the padded width",
                                                "more than 32 layers", "a graph beyond 64 nodes / max_edges in-edges")})


def tf_branch(p):
    """dgl_nets._FusedTransformer.__init__ (dgl_nets.py:1038-1049: hidden = out = 64, 8 heads, BatchNorm, residual, <= 16 layers, kp <= 64)
    + TransformerNet._stage / _fusable (:1154-1162: not full_graph, every layer hidden -> hidden) + sn_transformer_net_fused_f32 (<4,2>)"""
    assert not p.get("full_graph") and p["residual"], "the sparse residual net: what oracle.dgl_nets.transformer_net restates"
    if p["hidden"] != 64 or p["out_dim"] != 64:
        return "layer path: hidden is not 64"
    if p["n_heads"] != 8:
        return "layer path: not 8 heads"
    if p["L"] > GNN_MAX_LAYERS:
        return "layer path: more than 16 layers"
    if not within_stage(p, None, GNN_EMAX):
        return "layer path: a graph beyond 64 nodes / 192 in-edges"
    return " | ".join(sorted(coop_graph_names(4, 2, p)))


TF_BRANCHES = ({f"k_gnn_coop<4,2> T={T}" for T in (1, 2, 3, 4)} | {"k_gnn_coop<4,2> ne=0", "k_gnn_coop<4,2> ne=192"} |
               {f"layer path: {w}" for w in ("hidden is not 64", "not 8 heads", "more than 16 layers", "a graph beyond 64 nodes / 192 in-edges")})

BRANCH_OF = {"gin": gin_branch, "gated": gated_branch, "tf": tf_branch}
KERNEL = {"gin": "sn_gin_net_fused_f32", "gated": "sn_gatedgcn_fused_f32", "tf": "sn_transformer_net_fused_f32"}


def one_launch(case):
    return not case.branch.startswith("layer path")


# ============================================================================ the tables
# both sides of every 16-row tile edge; in-edge counts below, at and above a 64-edge pass
SIZES = (("rand", 1, 2), ("rand", 16, 40), ("rand", 17, 31), ("rand", 32, 64), ("rand", 33, 70), ("rand", 48, 100), ("rand", 49, 90), ("rand", 64, 150))
# a graph without edges, a directed cycle, a multigraph with self loops, a 39-in-edge star, exactly 192 in-edges
TOPOLOGY = (("none", 5, 0), ("cycle", 17, 17), ("rand", 9, 46), ("star", 40, 78), ("rand", 33, 192))
SMALL = (("rand", 12, 30), ("cycle", 5, 5), ("star", 7, 12), ("rand", 20, 47))
BEYOND = SMALL + (("rand", 30, 193),)
# GatedGCN: n in {1, 16, 17, 64} x ne in {0, 1, 63, 64, 65, 128, EMAX}; at 96 columns EMAX is 112 and a 128-edge graph is beyond the kernel
EDGES = (("none", 16, 0), ("rand", 1, 1), ("rand", 17, 63), ("rand", 64, 64), ("rand", 16, 65), ("rand", 64, 128), ("rand", 64, "EMAX"), ("none", 1, 0))
EDGES_96 = tuple(s for s in EDGES if s[2] != 128)
# the size and topology batches within the smallest EMAX (112)
G_SIZES = (("rand", 1, 2), ("rand", 16, 40), ("rand", 17, 31), ("rand", 64, 100), ("rand", 33, 70), ("rand", 48, 66))
G_TOPOLOGY = (("none", 5, 0), ("cycle", 17, 17), ("rand", 9, 46), ("star", 40, 78), ("rand", 64, 112))
# the persistent loop: eight distinct graphs of <= 8 nodes, without edges, below and above one 64-edge pass
EIGHT = (("none", 3, 0), ("rand", 8, 70), ("cycle", 5, 5), ("rand", 6, 30), ("star", 8, 14), ("rand", 1, 2), ("rand", 8, 100), ("rand", 7, 64))


def _row(op, fn, name, **p):
    return Case(op, name, fn(p), **p)


def _gin(hidden, graphs, tag, readout="mean", L=2, pe="lap_pe", salt=0):
    p = dict(hidden=hidden, out_dim=hidden, L=L, readout=readout, K=8, pe=pe, residual=True, graphs=graphs, salt=salt)
    return _row("gin", gin_branch, f"h{hidden}-L{L}-{readout}-{tag}", **p)


GIN_WIDTHS = {40: 64, 64: 64, 68: 96, 95: 96, 100: 128, 128: 128}          # hidden -> dp
READOUTS = ("sum", "mean", "max")


def _gin_rows():
    rows = []
    for i, (hid, dp) in enumerate(GIN_WIDTHS.items()):
        # per dp: the size batch at one width, the topology batch at the other; the three readouts spread over both
        rows.append(_gin(hid, SIZES if i % 2 == 0 else TOPOLOGY, "sizes" if i % 2 == 0 else "topology", readout=READOUTS[i % 3]))
    for hid, ro in ((64, "max"), (40, "mean"), (95, "mean"), (68, "sum"), (128, "mean"), (100, "sum")):
        rows.append(_gin(hid, SMALL, "small", readout=ro))
    rows += [_gin(64, SMALL, "small", L=1), _gin(95, SMALL, "small", L=16), _gin(40, TOPOLOGY, "nope", pe="no_pe"),
             _gin(95, SMALL, "nope", pe="no_pe"), _gin(128, SMALL, "nope", pe="no_pe"),
             _gin(132, SMALL, "wide"), _gin(64, SMALL, "deep", L=17), _gin(64, BEYOND, "beyond")]
    return rows


def _gated(hidden, graphs, tag, readout="mean", L=2, out_dim=None, residual=True, repeat=0, salt=0):
    p = dict(hidden=hidden, out_dim=out_dim or hidden, L=L, readout=readout, K=8, pe="lap_pe", residual=residual, graphs=graphs,
             repeat_beyond_cus=repeat, pe_aggregate="add", salt=salt)
    name = f"h{hidden}" + (f"-o{out_dim}" if out_dim else "") + f"-L{L}-{readout}" + ("" if residual else "-nores") + f"-{tag}"
    return _row("gated", gated_branch, name, **p)


GATED_WIDTHS = {12: 3, 44: 3, 48: 3, 52: 4, 64: 4, 68: 5, 80: 5, 84: 6, 96: 6}          # hidden -> instance


def _gated_rows():
    rows = []
    for i, (hid, nt) in enumerate(GATED_WIDTHS.items()):
        rows.append(_gated(hid, G_SIZES if i % 2 else G_TOPOLOGY, "sizes" if i % 2 else "topology", readout=READOUTS[i % 3]))
    for hid, ro in ((48, "sum"), (64, "max"), (68, "max"), (96, "sum")):          # per instance: the edge-pass batch, the persistent loop
        rows.append(_gated(hid, EDGES_96 if hid > 80 else EDGES, "edges", readout=ro))
    for hid, ro in ((44, "max"), (52, "sum"), (80, "mean"), (84, "max")):
        rows.append(_gated(hid, EIGHT, "persistent", readout=ro, repeat=40))
    rows += [_gated(64, SMALL, "small", out_dim=40), _gated(52, SMALL, "small", out_dim=60), _gated(68, EDGES, "edges", residual=False),
             _gated(48, SMALL, "small", L=1), _gated(68, SMALL, "small", L=16),
             _gated(50, SMALL, "small"), _gated(100, SMALL, "small"), _gated(52, SMALL, "small", out_dim=68), _gated(48, SMALL, "deep", L=33),
             _gated(64, BEYOND, "beyond")]
    return rows


def _tf(graphs, tag, readout="sum", L=2, hidden=64, n_heads=8, pe_aggregate="add"):
    p = dict(hidden=hidden, out_dim=hidden, L=L, readout=readout, K=16, pe="lap_pe", residual=True, graphs=graphs, n_heads=n_heads,
             pe_aggregate=pe_aggregate, full_graph=False)
    return _row("tf", tf_branch, f"h{hidden}-L{L}-{readout}-{pe_aggregate}-{tag}" + (f"-{n_heads}heads" if n_heads != 8 else ""), **p)


def _tf_rows():
    return [_tf(SIZES, "sizes", "sum", L=3), _tf(TOPOLOGY, "topology", "mean", L=3, pe_aggregate="concat"), _tf(SMALL, "small", "max", L=1),
            _tf(SMALL, "small", "mean", L=10, pe_aggregate="concat"), _tf(TOPOLOGY, "topology", "max", L=2), _tf(SIZES, "sizes", "mean", L=1),
            _tf(SMALL, "small", hidden=56), _tf(SMALL, "small", n_heads=4), _tf(SMALL, "small", L=17), _tf(BEYOND, "beyond")]


GIN, GATED, TF = _gin_rows(), _gated_rows(), _tf_rows()
ALL = GIN + GATED + TF


# ============================================================================ nets and references
def net_params(case, device="cpu"):
    p = case.p
    q = dict(num_atom_type=N_ATOM, num_bond_type=N_BOND, in_feat_dropout=0.0, dropout=0.0, batch_norm=True, residual=p["residual"], edge_feat=True,
             pe_init=p["pe"], lap_method="none", lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4, device=device,
             hidden_dim=p["hidden"], out_dim=p["out_dim"], L=p["L"], readout=p["readout"], pos_enc_dim=p["K"],
             pe_aggregate=p.get("pe_aggregate", "add"))
    if case.op == "tf":
        q.update(n_heads=p["n_heads"], full_graph=p["full_graph"], layer_norm=True)
    return q


NET_CLASS = {"gin": "GINNet", "gated": "GatedGCNNet", "tf": "TransformerNet"}


def build_net(case):
    """the row's net on the CPU (parameter holders; .to(device) runs it): no identity anywhere — BatchNorm running statistics
    (parity_util.bn_randomize), BatchNorm affine, the GIN layers' eps"""
    from signnet_basisnet_amd import readout_models          # (the classes that take every readout; sum and mean are the base classes')
    torch.manual_seed(seed_of(case))
    net = getattr(readout_models, NET_CLASS[case.op])(net_params(case))
    PU.bn_randomize(net, seed_of(case, 1))
    g = torch.Generator().manual_seed(seed_of(case, 2))
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.weight.copy_(1.0 + 0.2 * torch.randn(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
        for name, buf in net.named_buffers():
            if name.endswith(".eps") and buf.numel() == 1:
                buf.copy_(0.6 * torch.rand(1, generator=g) - 0.3)
    return net.eval()


def oracle_scores(case, sd, b, dtype):
    """oracle.dgl_nets on the batch `b` (assemble) with the weights in `dtype` -> scores [B, 1]"""
    from oracle import dgl_nets as O
    p = case.p
    sd = PU.to_f64(sd) if dtype == F64 else sd
    pe = b["p"].to(dtype) if p["pe"] == "lap_pe" else None
    sizes = b["sizes"].tolist()
    with torch.no_grad():
        if case.op == "gin":
            return O.gin_net(sd, b["src"], b["dst"], sizes, b["h"], pe, p["L"], p["readout"])
        if case.op == "gated":
            return O.gatedgcn_net(sd, b["src"], b["dst"], sizes, b["h"], pe, b["e"], p["L"], p["pe_aggregate"], p["readout"], residual=p["residual"])
        return O.transformer_net(sd, b["src"], b["dst"], sizes, b["h"], pe, b["e"], p["L"], p["n_heads"], p["pe_aggregate"], p["readout"])


@functools.lru_cache(maxsize=4)
def reference(case, emax=None):
    """-> (state_dict, y float32 [k, 1], y float64 [k, 1]) of the row's k stated graphs, in the stated order"""
    sd = {k: v.detach().clone() for k, v in build_net(case).state_dict().items()}
    b = assemble(case, emax=emax)
    return sd, oracle_scores(case, sd, b, F32), oracle_scores(case, sd, b, F64)
