"""CPU: full-graph attention from the bond graph — what can be checked without a GPU.

  restatement   the bond form (expand the bonds with FC.make_full_graph_ref, then FC.full_attention_ref) equals the edge form in
                float64 on every case of tests/bond_attention_cases.py
  fixtures      the three fixtures' bond lists reproduce their stored full_src / full_dst / real / e_full exactly
  case tables   every case lands on the branch it names: the staging limits (answered by the library as well), the clamp, the
                patterns, the empty graph
  surface       the property full_graph_input, the refusals that stay and the ones that are lifted"""
import pytest
import torch

import bond_attention_cases as BC
import full_graph_cases as FC


def _id(case):
    return " ".join(f"{k}={v}" for k, v in sorted(case.items()) if k != "sizes") + (f" sizes={len(case['sizes'])}" if "sizes" in case else "")


@pytest.mark.parametrize("case", BC.CASES, ids=_id)
def test_bond_form_equals_the_edge_form(case):
    inp = BC.bond_inputs(**case)
    ex = BC.expand(inp)
    # the expansion of the bonds is the case's own edge list (same pairs in the same order, same flags and classes) ...
    assert torch.equal(ex.src, inp.src) and torch.equal(ex.dst, inp.dst) and torch.equal(ex.codes, inp.codes)
    assert int((inp.codes & 1).sum()) == inp.bsrc.numel()
    # ... so the two restatements are one function
    a = FC.to_dtype(inp, torch.float64)
    edge = FC.full_attention_ref(a.Q, a.K, a.V, a.Q2, a.K2, a.Tr, a.Tf, a.codes, a.gamma, a.src, a.dst, a.heads)
    assert torch.equal(BC.bond_attention_ref(inp), edge)
    # a one-node graph has no pair: exact zeros
    off = 0
    for n in inp.sizes:
        if n == 1:
            assert not bool(edge[off].any())
        off += n


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_fixture_bonds_reproduce_the_stored_full_graph(name):
    fx = FC.fixture(name)
    sizes = [int(s) for s in fx.inp["sizes"]]
    ei = fx.inp["edge_index"]
    fs, fd, real, ef = FC.make_full_graph_ref(sizes, ei[0], ei[1], fx.inp["edge_attr"].reshape(-1))
    for got, key in ((fs, "full_src"), (fd, "full_dst"), (real, "real"), (ef, "e_full")):
        assert torch.equal(got, fx.inp[key]), key
    # the bonds are well-formed for the bond kernel: no self loop, no repeated (u, v), none between two graphs
    assert not bool((ei[0] == ei[1]).any())
    N = sum(sizes)
    assert torch.unique(ei[0] * N + ei[1]).numel() == ei.shape[1]
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    assert torch.equal(batch[ei[0]], batch[ei[1]])


def test_staging_limits_are_the_librarys():
    from signnet_basisnet_amd import build
    build.build()
    from signnet_basisnet_amd import ops
    for dk in (1, 3, 4, 8, 10, 16, 24, 32):
        for bwd in (False, True):
            n = BC.staged_nodes(dk, bwd)
            assert ops.bond_attention_staged_nodes(dk, bwd) == n
            assert BC.path_of(n, dk, bwd) == "staged" and BC.path_of(n + 1, dk, bwd) == "global"
    assert ops.bond_attention_staged_nodes(33) == 0 and ops.bond_attention_staged_nodes(0) == 0


def test_case_tables_land_on_their_branches():
    # the grid: at every shape the forward stages every graph and the adjoint every graph up to 33 nodes; up to a head width of 16 the
    # adjoint stages all of them, at 24 and 32 its two largest graphs take the global path next to staged ones in one launch
    for heads, dk in BC.SHAPES:
        assert all(BC.path_of(n, dk, False) == "staged" for n in FC.GRID_SIZES)
        assert all(BC.path_of(n, dk, True) == "staged" for n in FC.GRID_SIZES if n <= 33 or dk <= 16)
        if dk >= 24:
            assert BC.path_of(65, dk, True) == BC.path_of(70, dk, True) == "global"
    assert {h for h, _ in BC.SHAPES} == set(range(1, 9)) and {3, 4, 8, 10, 16, 24, 32} <= {k for _, k in BC.SHAPES}
    assert 1 in FC.GRID_SIZES and max(FC.GRID_SIZES) < 128          # (one destination per thread of the 128-thread workgroup)
    # the limit case: d = 128; per pass the largest staged graph and the first one that is not
    dk = BC.LIMIT_CASE["dk"]
    assert BC.LIMIT_CASE["heads"] * dk == 128
    a, b, c, d = BC.LIMIT_SIZES
    assert (BC.path_of(a, dk, True), BC.path_of(b, dk, True)) == ("staged", "global") and b == a + 1
    assert (BC.path_of(c, dk, False), BC.path_of(d, dk, False)) == ("staged", "global") and d == c + 1
    assert BC.path_of(c, dk, True) == "global" and BC.path_of(b, dk, False) == "staged"     # (the passes' limits differ)
    # the huge case: the byte table alone does not fit a workgroup's 160 KiB, and the workgroup's threads take several nodes each
    n = max(BC.HUGE_CASE["sizes"])
    assert n == 450 and n * n > 160 * 1024 and n > 3 * 128
    assert BC.path_of(n, BC.HUGE_CASE["dk"], False) == BC.path_of(n, BC.HUGE_CASE["dk"], True) == "global"
    assert BC.path_of(3, BC.HUGE_CASE["dk"], True) == "staged"
    # the empty graph sits in the middle, next to a one-node graph
    s = BC.EMPTY_CASE["sizes"]
    assert 0 in s[1:-1] and 1 in s and BC.path_of(0, 5, False) == "skip"


def test_patterns_gamma_arms_and_clamp_meet_their_conditions():
    for p in BC.PATTERNS:
        inp = BC.bond_inputs(3, 5, pattern=p, gamma=0.6, seed=2)
        real = (inp.codes & 1).bool()
        pairs = sum(n * (n - 1) for n in inp.sizes)
        assert inp.src.numel() == pairs
        if p == "all_real":
            assert bool(real.all()) and inp.bsrc.numel() == pairs
        elif p == "none_real":
            assert not bool(real.any()) and inp.bsrc.numel() == 0
        elif p == "one_direction":
            assert torch.equal(real, inp.src < inp.dst) and bool((inp.bsrc < inp.bdst).all())
        else:
            assert 0 < int(real.sum()) < pairs
            rev = set(zip(inp.bdst.tolist(), inp.bsrc.tolist()))
            assert set(zip(inp.bsrc.tolist(), inp.bdst.tolist())) == rev                  # both directions of every bond
        if p == "shuffled":
            m = BC.bond_inputs(3, 5, pattern="molecule", gamma=0.6, seed=2)
            assert not torch.equal(m.bsrc, inp.bsrc) and sorted(zip(m.bsrc.tolist(), m.bdst.tolist(), m.bcls.tolist())) == \
                sorted(zip(inp.bsrc.tolist(), inp.bdst.tolist(), inp.bcls.tolist()))
    assert any(g < 0 for g in BC.GAMMAS) and any(0 < g < 1 for g in BC.GAMMAS) and any(g > 1 for g in BC.GAMMAS)
    # the clamp is live in the bond form of FC.CLAMP_CASE too: real and fake scores beyond +5 and beyond -5, none within 1e-3 of +-5
    rp, fp, rm, fm, near = FC.clamp_conditions(BC.bond_inputs(**BC.CLAMP_CASE))
    print("clamp conditions (real > 5, fake > 5, real < -5, fake < -5, near):", rp, fp, rm, fm, near)
    assert rp >= 1 and fp >= 1 and rm >= 1 and fm >= 1 and near == 0, (rp, fp, rm, fm, near)


def test_full_graph_input_is_an_opt_in_property():
    from signnet_basisnet_amd import dgl_nets, dropout_models
    fx = FC.fixture(FC.FIXTURES[0])
    net = dgl_nets.TransformerNet(FC.net_params(fx))
    keys = list(net.state_dict().keys())
    assert net.full_graph_input == "edges"
    net.full_graph_input = "bonds"
    assert net.full_graph_input == "bonds" and list(net.state_dict().keys()) == keys == [str(k) for k in fx.meta["sd_keys"]]
    net.load_state_dict(fx.sd, strict=True)
    with pytest.raises(ValueError, match="full_graph_input"):
        net.full_graph_input = "pairs"
    assert net.full_graph_input == "bonds"
    net.full_graph_input = "edges"
    sparse = dgl_nets.TransformerNet(FC.net_params(fx, full_graph=False))
    assert sparse.full_graph_input == "edges"
    with pytest.raises(ValueError, match="full_graph=True"):
        sparse.full_graph_input = "bonds"
    sub = dropout_models.TransformerNet(FC.net_params(fx))
    sub.full_graph_input = "bonds"
    assert sub.full_graph_input == "bonds" and dgl_nets.TransformerNet(FC.net_params(fx)).full_graph_input == "edges"


def test_refusals_stay_for_the_edge_form_and_for_flagged_graphs():
    from signnet_basisnet_amd import data, dgl_nets, serving, train_graph
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    fx = FC.fixture(FC.FIXTURES[0])
    net = dgl_nets.TransformerNet(FC.net_params(fx))
    with pytest.raises(NotImplementedError, match=r"DGLBucketedStep does not carry the edge flag edata\['real'\]"):
        train_graph.DGLBucketedStep(net, None)
    with pytest.raises(NotImplementedError, match=r"GraphedDGLForward does not carry the edge flag edata\['real'\]"):
        serving.GraphedDGLForward(net.eval(), None, None, None)
    full = Graph(fx.inp["full_src"], fx.inp["full_dst"], fx.inp["sizes"])
    full.edata["real"] = fx.inp["real"]
    with pytest.raises(NotImplementedError, match=r"DGLGraphStore does not carry the edge flag edata\['real'\]"):
        data.DGLGraphStore.from_batch((full, fx.inp["x"], fx.inp["pos_enc"], fx.inp["e_full"], None), None, "cpu")
    # a bond-form net passes the first gate of both wrappers (the next one is the optimizer's type / the graph) ...
    net.full_graph_input = "bonds"
    with pytest.raises(TypeError, match="FlatAdam"):
        train_graph.DGLBucketedStep(net.train(), None)
    # ... but not with a graph that carries the flag
    with pytest.raises(NotImplementedError, match=r"GraphedDGLForward does not carry the edge flag edata\['real'\]"):
        serving.GraphedDGLForward(net.eval(), full, None, None)
    assert train_graph.carries_real_flag(full) and not train_graph.carries_real_flag(Graph(fx.inp["edge_index"][0], fx.inp["edge_index"][1],
                                                                                         fx.inp["sizes"]))
