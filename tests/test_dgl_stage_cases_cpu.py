"""No GPU: the conditions under which the DGL one-launch net grid (tests/test_dgl_stage_grid_gpu.py) can tell a right kernel from a wrong
one, checked on every row of tests/dgl_stage_cases.py.

  branch        the restated dispatch, evaluated on the row's stated batch, returns the row's `branch`; each table reaches every name its
                predicate can return
  batches       every stated node and in-edge count is what the generator built; the topologies the grid was written for are there
                (directed-only edges, repeated edges, self loops, nodes without in-edges, an edge with source row 63 in the last pass)
  coverage      the widths, readouts, layer counts and batches the grid was written for are in the tables
  conditioning  per row the float32 oracle is within parity_util.REL of the float64 oracle under `close` and `elementwise`
  host rules    dgl_nets._FusedGin / _FusedGated / _FusedTransformer, TransformerNet._fusable and _DGLNet._stage decide as the predicates
                do: the packers are constructed on CPU nets with the device packing calls replaced by shape recorders
"""
import time
import types

import numpy as np
import pytest
import torch

import dgl_stage_cases as DC
import parity_util as PU


def ids(cases):
    return [c.id for c in cases]


def test_ids_are_unique():
    i = ids(DC.ALL)
    assert len(i) == len(set(i)), sorted(x for x in i if i.count(x) > 1)


@pytest.mark.parametrize("case", DC.ALL, ids=ids(DC.ALL))
def test_row_takes_the_branch_it_names(case):
    assert DC.BRANCH_OF[case.op](case.p) == case.branch


def test_rows_cover_every_branch_the_predicates_can_return():
    for rows, full in ((DC.GIN, DC.GIN_BRANCHES), (DC.GATED, DC.GATED_BRANCHES), (DC.TF, DC.TF_BRANCHES)):
        seen = DC.branches_of(rows)
        assert seen == full, f"not reached {sorted(full - seen)}, not declared {sorted(seen - full)}"


def test_named_branches_are_all_in_the_tables():
    """the list the grid was written for, spelled out"""
    seen = DC.branches_of(DC.ALL)
    want = {"k_gnn_coop<6,1> T=3", "k_gnn_coop<8,1> T=1", "k_gnn_coop<4,1> ne=0", "k_gnn_coop<8,1> ne=192", "k_gnn_coop<4,1> kp=1 (no_pe)",
            "k_gnn_coop<4,2> T=4", "k_gnn_coop<4,2> ne=0", "k_gatedgcn_net<4> npass=2", "k_gatedgcn_net<6> ne=0", "k_gatedgcn_net<3> ne=EMAX",
            "k_gatedgcn_net<6> second graph", "k_gatedgcn_net<5> npass=3", "d_out in (d, dp]", "no residual", "layer path: wider than 128",
            "layer path: hidden not a multiple of 4", "layer path: hidden is not 64"}
    assert want <= seen, sorted(want - seen)


def test_restated_max_edges():
    """csrc/fused_gated.hip GGCfg<3..6>::EMAX (176 at hidden 68: dgl_nets._DGLNet._stage's docstring); widths below 48 run on <3>"""
    assert [DC.gated_max_edges(d) for d in (12, 48, 64, 68, 80, 96, 100)] == [192, 192, 192, 176, 176, 112, 0]


# ---------------------------------------------------------------------------- batches
def csr_order(e, n):
    """positions of the graph's edges in destination-sorted (CSR) order, edge-id order within a destination"""
    return np.argsort(e[:, 1].numpy(), kind="stable")


@pytest.mark.parametrize("case", DC.ALL, ids=ids(DC.ALL))
def test_stated_sizes_and_edge_counts_are_what_the_generator_built(case):
    emax = DC.default_emax(case)
    b = DC.assemble(case)
    specs = [DC.resolve(s, emax) for s in case.p["graphs"]]
    assert b["sizes"].tolist() == [n for _, n, _ in specs] and b["edge_counts"].tolist() == [ne for _, _, ne in specs]
    N, E = int(b["sizes"].sum()), int(b["edge_counts"].sum())
    assert b["src"].shape == b["dst"].shape == b["e"].shape == (E,) and b["h"].shape == (N,) and b["p"].shape == (N, case.p["K"])
    # every edge inside its graph, the edges of a graph contiguous (as a DGL batch holds them)
    start = torch.cumsum(b["sizes"], 0) - b["sizes"]
    gid = torch.repeat_interleave(torch.arange(len(specs)), b["edge_counts"])
    for t in (b["src"], b["dst"]):
        assert bool(((t >= start[gid]) & (t < (start + b["sizes"])[gid])).all())
    assert int(b["h"].max()) < DC.N_ATOM and (E == 0 or int(b["e"].max()) < DC.N_BOND)
    # reversed order and cyclic repeats hold the same graphs
    rev = DC.assemble(case, order=list(range(len(specs)))[::-1])
    assert rev["sizes"].tolist() == b["sizes"].tolist()[::-1] and rev["edge_counts"].tolist() == b["edge_counts"].tolist()[::-1]
    assert torch.equal(rev["p"][:specs[-1][1]], b["p"][N - specs[-1][1]:])
    if case.p.get("repeat_beyond_cus"):
        order = DC.batch_order(case)
        assert len(order) == DC.CUS + 40 and order[:9] == [0, 1, 2, 3, 4, 5, 6, 7, 0] and max(n for _, n, _ in specs) <= 8
        assert set(order) == set(range(8)) and all(order.count(j) >= 2 for j in range(8))
        # a workgroup's second graph is never its first (else whatever the first left in LDS would be right for the second): at the
        # MI355X's CU count and at any other, forward and reversed
        for cus in (DC.CUS, 255, 257, 304, 64):
            o = DC.batch_order(case, cus)
            assert len(o) == cus + 40
            DC.check_second_graphs(case, o, cus)
            DC.check_second_graphs(case, o[::-1], cus, reverse=True)
        assert all(order[w] != order[w + DC.CUS] for w in range(40))
        assert {0} < {ne for _, _, ne in specs} and any(0 < ne < 64 for _, _, ne in specs) and any(ne > 64 for _, _, ne in specs)


def test_the_batches_hold_the_topologies_the_grid_was_written_for():
    case = next(c for c in DC.GATED if c.name == "h64-L2-max-edges")
    emax = DC.default_emax(case)
    seen_63 = 0
    for j, spec in enumerate(case.p["graphs"]):
        n, e, *_ = DC._graph(case, j, emax)
        ne = e.shape[0]
        if ne >= 4:
            pairs = {tuple(x) for x in e.tolist()}
            assert len(pairs) < ne, "a repeated edge"
            assert (0, 0) in pairs and (n - 1, n - 1) in pairs, "self loops"
            assert any((b, a) not in pairs for a, b in pairs if a != b), "directed-only edges"
        if n == 64 and ne:
            last = csr_order(e, n)[64 * ((ne - 1) // 64):]          # the edges of the last 64-edge pass
            assert 63 in e[last, 0].tolist(), f"graph {j}: no edge with source row 63 in the last pass"
            seen_63 += 1
    assert seen_63 >= 3 and {DC.resolve(s, emax)[2] for s in case.p["graphs"]} == {0, 1, 63, 64, 65, 128, emax}
    assert {s[1] for s in case.p["graphs"]} == {1, 16, 17, 64}
    # the topology batch: no edges, a directed cycle, a multigraph with self loops, a 39-in-edge star, exactly 192 in-edges;
    # nodes without in-edges (the Transformer's z = 0)
    case = next(c for c in DC.TF if c.name.endswith("topology"))
    b = DC.assemble(case)
    assert b["edge_counts"].tolist() == [0, 17, 46, 78, 192]
    indeg = torch.bincount(b["dst"], minlength=int(b["sizes"].sum()))
    assert int(indeg.max()) >= 39 and int((indeg == 0).sum()) >= 5
    assert {s[1] for s in DC.SIZES} == {1, 16, 17, 32, 33, 48, 49, 64}


# ---------------------------------------------------------------------------- coverage
def rows(table, **kw):
    return [c for c in table if all(c.p.get(k) == v for k, v in kw.items())]


def test_the_tables_hold_the_shapes_the_grid_was_written_for():
    assert DC.GIN_WIDTHS == {40: 64, 64: 64, 68: 96, 95: 96, 100: 128, 128: 128}
    for hid, dp in DC.GIN_WIDTHS.items():
        assert rows(DC.GIN, hidden=hid, L=2) and DC.gin_dp(rows(DC.GIN, hidden=hid)[0].p)[1] == dp
    for dp in (64, 96, 128):
        at = [c for c in DC.GIN if DC.one_launch(c) and DC.gin_dp(c.p)[1] == dp]
        assert {c.p["readout"] for c in at} == set(DC.READOUTS), dp
        assert any(c.p["graphs"] == DC.SIZES for c in at) and any(c.p["graphs"] == DC.TOPOLOGY for c in at), dp
    assert rows(DC.GIN, L=1) and rows(DC.GIN, L=16) and rows(DC.GIN, pe="no_pe") and rows(DC.GIN, hidden=132) and rows(DC.GIN, L=17)
    assert DC.GATED_WIDTHS == {12: 3, 44: 3, 48: 3, 52: 4, 64: 4, 68: 5, 80: 5, 84: 6, 96: 6}
    for hid, nt in DC.GATED_WIDTHS.items():
        r = [c for c in rows(DC.GATED, hidden=hid, L=2, out_dim=hid) if DC.one_launch(c)]
        assert r and all(f"k_gatedgcn_net<{nt}>" in c.branch for c in r), hid
    for nt in (3, 4, 5, 6):
        at = [c for c in DC.GATED if f"k_gatedgcn_net<{nt}>" in c.branch]
        assert {c.p["readout"] for c in at} == set(DC.READOUTS), nt
        assert any(c.p["graphs"] in (DC.EDGES, DC.EDGES_96) for c in at) and any(c.p.get("repeat_beyond_cus") == 40 for c in at), nt
    assert rows(DC.GATED, hidden=50) and rows(DC.GATED, hidden=100) and rows(DC.GATED, hidden=64, out_dim=40) and rows(DC.GATED, hidden=52, out_dim=60)
    assert rows(DC.GATED, residual=False) and rows(DC.GATED, L=1) and rows(DC.GATED, L=16)
    fused = [c for c in DC.TF if DC.one_launch(c)]
    assert {c.p["L"] for c in fused} == {1, 2, 3, 10} and {c.p["readout"] for c in fused} == set(DC.READOUTS)
    assert {c.p["pe_aggregate"] for c in fused} == {"add", "concat"} and rows(DC.TF, hidden=56)
    assert any(c.p["graphs"] == DC.SIZES for c in fused) and any(c.p["graphs"] == DC.TOPOLOGY for c in fused)
    assert all(len(c.p["graphs"]) <= 12 for c in DC.ALL)


# ---------------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("case", DC.ALL, ids=ids(DC.ALL))
def test_float32_oracle_is_within_rel_of_float64_and_quick(case):
    t0 = time.perf_counter()
    sd, y32, y64 = DC.reference(case)
    print(f"\n{case.id}: both oracle passes took {time.perf_counter() - t0:.2f} s", end="")
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64 and y32.shape == y64.shape == (len(case.p["graphs"]), 1)
    assert bool(torch.isfinite(y64).all()) and y64.abs().max().item() > 0
    assert torch.unique(y64).numel() == y64.numel(), f"{case.id}: distinct graphs with the same score (a dead net is no reference)"
    PU.close(y32, y64, f"{case.id}: float32 oracle vs float64")
    PU.elementwise(y32, y64, f"{case.id}: float32 oracle vs float64, element-wise")


def test_scores_of_a_graph_do_not_depend_on_its_batch():
    """what the reversed-order and persistent-loop comparisons rest on: in eval mode the oracle's score of a graph is the same in any batch"""
    for case in (DC.GIN[0], next(c for c in DC.GATED if c.p.get("repeat_beyond_cus")), DC.TF[0]):
        sd, y32, y64 = DC.reference(case)
        k = len(case.p["graphs"])
        order = [i % k for i in range(k + 3)][::-1]
        y = DC.oracle_scores(case, sd, DC.assemble(case, order=order), DC.F64)
        assert torch.allclose(y, y64[order], rtol=0, atol=1e-12 * y64.abs().max().item())


# ---------------------------------------------------------------------------- host rules
@pytest.fixture
def recorded_packing(monkeypatch):
    """The packers of dgl_nets on CPU nets: every device packing call replaced by a recorder of the shapes it was given.  The `ok`
    rules, the padded widths and the parameter block are host code and run as they are."""
    from signnet_basisnet_amd import dgl_deepsigns, dgl_nets, ops
    shapes = []

    def pack_split(W, *vecs):
        shapes.append(tuple(W.shape))
        return torch.zeros(16, dtype=torch.uint8)

    def bn_fold(bn, c_pad=None):
        c = bn.num_features if c_pad is None else int(c_pad)
        return torch.ones(c), torch.zeros(c)

    monkeypatch.setattr(ops, "pack_split", pack_split)
    monkeypatch.setattr(ops, "bn_fold", bn_fold)
    monkeypatch.setattr(dgl_nets, "_fold_bn_before", lambda lin, site: (lin.weight.detach(), lin.bias.detach()))
    monkeypatch.setattr(dgl_nets, "lib", lambda: types.SimpleNamespace(sn_gatedgcn_max_edges=DC.gated_max_edges))
    return shapes


@pytest.mark.parametrize("case", DC.ALL, ids=ids(DC.ALL))
def test_host_packers_decide_as_the_predicates_do(case, recorded_packing):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    p = case.p
    net = DC.build_net(case)
    fz = net._stage_cls(net)
    b = DC.assemble(case)
    g = DS.Graph(b["src"], b["dst"], b["sizes"], b["edge_counts"])
    assert (net._stage(g) is not None) == DC.one_launch(case), "the host's choice of path"
    if case.op == "gin":
        ok, dp, kp = DC.gin_dp(p)
        assert fz.ok == ok
        if ok:
            assert (fz.params.d, fz.kp, fz.params.n_layers) == (dp, kp, p["L"]) and set(recorded_packing) == {(dp, dp)}
            assert fz.pool_mean == {"sum": 0, "mean": 1, "max": 2}[p["readout"]]
    elif case.op == "gated":
        why, dp = DC.gated_dp(p)
        assert fz.ok == (why is None)
        if fz.ok:
            P = fz.params
            assert (P.d, P.d_out, P.n_layers, P.readout_mean) == (p["hidden"], p["out_dim"], p["L"], {"sum": 0, "mean": 1, "max": 2}[p["readout"]])
            assert set(recorded_packing) == {(4 * dp, dp), (dp, dp)}, "A|B|D|E and C are packed at the instance's width"
            assert fz.max_edges == DC.gated_max_edges(p["hidden"])
            want = [int(p["residual"] and (l < p["L"] - 1 or p["out_dim"] == p["hidden"])) for l in range(p["L"])]
            assert [P.layers[l].residual for l in range(p["L"])] == want
    else:
        fusable = p["hidden"] == p["out_dim"]          # TransformerNet._fusable: every layer hidden -> hidden
        assert net._fusable() == fusable
        assert fz.ok == (p["hidden"] == 64 and p["out_dim"] == 64 and p["n_heads"] == 8 and p["L"] <= DC.GNN_MAX_LAYERS)
        if fz.ok:
            assert (fz.params.d, fz.kp, fz.params.n_layers) == (64, p["K"], p["L"])


def test_a_graph_without_edge_counts_reaches_the_kernel(recorded_packing):
    """_DGLNet._stage: without batch_num_edges() the host cannot know; the kernels' own guards decide (the GPU test's guard rows)"""
    from signnet_basisnet_amd import dgl_deepsigns as DS
    for case in (DC.GIN[0], DC.GATED[0], DC.TF[0]):
        net = DC.build_net(case)
        b = DC.assemble(case, extra=[DC.oversize_graph(case, 193)])
        assert net._stage(DS.Graph(b["src"], b["dst"], b["sizes"], b["edge_counts"])) is None
        assert net._stage(DS.Graph(b["src"], b["dst"], b["sizes"])) is not None
