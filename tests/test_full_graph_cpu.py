"""CPU: full-graph attention for TransformerNet (full_graph=True) — what can be checked without a GPU.

  restatement   tests/full_graph_cases.py's torch form of the op (inside the net) reproduces the reference's own runs stored in
                tests/golden/fullgraph_*.npz: eval y / h_last, train-mode y and every parameter gradient, in float32 and float64
  make_full_graph  its restatement gives the fixtures' full edge lists, flags and classes, and networkx's edge order
  state_dict    key order equals the reference's; a reference checkpoint loads with strict=True; full_graph=False nets keep their keys
  refusals      DGLBucketedStep, GraphedDGLForward, DGLGraphStore and a graph without edata['real']"""
import pytest
import torch

import full_graph_cases as FC
import parity_util as PU


def _sd(fx, dtype, grad=False):
    out = {}
    for k, v in fx.sd.items():
        if v.is_floating_point():
            v = v.to(dtype).clone()
            if grad and "running" not in k:
                v.requires_grad_(True)
        out[k] = v
    return out


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_restatement_reproduces_the_reference_runs(name):
    fx = FC.fixture(name)
    for dtype, tag, rel in ((torch.float64, "64", 1e-9), (torch.float32, "", 1e-5)):
        out = {}
        with torch.no_grad():
            y = FC.full_transformer_net(_sd(fx, dtype), fx, False, out)
        assert PU.relerr(y, fx.out["eval/y" + tag]) <= rel and PU.relerr(out["h_last"], fx.out["eval/h_last" + tag]) <= rel
    # train mode and the gradients of the L1 loss, float64 (float32 repeats the same arithmetic at its own precision)
    sd = _sd(fx, torch.float64, grad=True)
    y = FC.full_transformer_net(sd, fx, True)
    assert PU.relerr(y, fx.out["train/y64"]) <= 1e-9
    (y - fx.inp["target"].double()).abs().mean().backward()
    ref = {k[len("train/grad64/"):]: v for k, v in fx.out.items() if k.startswith("train/grad64/")}
    gmax = max(float(v.abs().max()) for v in ref.values())
    assert any(k.endswith(".gamma") for k in ref) and any(".Q_2." in k for k in ref) and any(".E_2." in k for k in ref)
    for k, g in ref.items():
        got = sd[k].grad if sd[k].grad is not None else torch.zeros_like(g)
        assert (got - g).abs().max().item() <= 1e-8 * gmax, k
    hidden, L, k_, heads = (int(v) for v in fx.meta["params"])
    for l, gm in enumerate(fx.meta["gamma"]):
        g = ref[f"layers.{l}.gamma"]
        if not 0.0 <= float(gm) <= 1.0:
            assert float(g) == 0.0            # the clamped arms: exactly 0
        else:
            assert float(g) != 0.0


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_make_full_graph_restatement_gives_the_fixture_and_networkx_order(name):
    nx = pytest.importorskip("networkx")
    fx = FC.fixture(name)
    sizes = [int(s) for s in fx.inp["sizes"]]
    ei = fx.inp["edge_index"]
    fs, fd, real, ef = FC.make_full_graph_ref(sizes, ei[0], ei[1], fx.inp["edge_attr"].reshape(-1))
    for got, key in ((fs, "full_src"), (fd, "full_dst"), (real, "real"), (ef, "e_full")):
        assert torch.equal(got, fx.inp[key]), key
    assert int(real.sum()) == ei.shape[1]
    off, pairs = 0, []
    for n in sizes:
        pairs += [(off + u, off + v) for u, v in nx.complete_graph(n).to_directed().edges()]
        off += n
    assert pairs == list(zip(fs.tolist(), fd.tolist()))


@pytest.mark.parametrize("name", FC.FIXTURES)
def test_state_dict_key_order_and_strict_load(name):
    from signnet_basisnet_amd import dgl_nets
    fx = FC.fixture(name)
    net = dgl_nets.TransformerNet(FC.net_params(fx))
    want = [str(k) for k in fx.meta["sd_keys"]]
    assert list(net.state_dict().keys()) == want
    assert "layers.0.gamma" in want and "layers.0.attention_h.gamma" in want
    i = want.index("layers.0.attention_h.Q.weight")
    assert [k.split(".")[3] for k in want[i:i + 7]] == ["Q", "K", "E", "Q_2", "K_2", "E_2", "V"]
    net.load_state_dict(fx.sd, strict=True)
    for l, gm in enumerate(fx.meta["gamma"]):
        assert net.layers[l].gamma is net.layers[l].attention_h.gamma and net.layers[l].gamma.item() == pytest.approx(float(gm))


def test_sparse_nets_keep_their_keys():
    from signnet_basisnet_amd import dgl_nets
    fx = FC.fixture(FC.FIXTURES[0])
    net = dgl_nets.TransformerNet(FC.net_params(fx, full_graph=False))
    full = [str(k) for k in fx.meta["sd_keys"]]
    keys = list(net.state_dict().keys())
    assert keys == [k for k in full if "_2." not in k]
    assert not any("_2" in k for k in keys) and net._stage_cls is not None and not net.full_graph


def test_out_of_scope_paths_refuse_a_full_graph_net():
    from signnet_basisnet_amd import data, dgl_nets, serving, train_graph
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    fx = FC.fixture(FC.FIXTURES[0])
    net = dgl_nets.TransformerNet(FC.net_params(fx))
    with pytest.raises(NotImplementedError, match="full_graph"):
        train_graph.DGLBucketedStep(net, None)
    with pytest.raises(NotImplementedError, match="full_graph"):
        serving.GraphedDGLForward(net.eval(), None, None, None)
    g = Graph(fx.inp["full_src"], fx.inp["full_dst"], fx.inp["sizes"])
    g.edata["real"] = fx.inp["real"]
    with pytest.raises(NotImplementedError, match="full_graph"):
        data.DGLGraphStore.from_batch((g, fx.inp["x"], fx.inp["pos_enc"], fx.inp["e_full"], None), None, "cpu")
    with pytest.raises(NotImplementedError, match="full_graph"):
        data.DGLGraphStore.from_samples([(g, None, None, None, None, None)], "cpu")
    # a graph without the flag: a clear error before anything is launched
    bare = Graph(fx.inp["full_src"], fx.inp["full_dst"], fx.inp["sizes"])
    with pytest.raises(ValueError, match=r"edata\['real'\]"):
        net(bare, fx.inp["x"].reshape(-1), fx.inp["pos_enc"], fx.inp["e_full"], None)
    # still refused as before
    with pytest.raises(NotImplementedError):
        dgl_nets.TransformerNet(FC.net_params(fx, edge_feat=False))
    with pytest.raises(NotImplementedError):
        dgl_nets.TransformerNet(FC.net_params(fx, readout="max"))
    with pytest.raises(NotImplementedError):
        dgl_nets.TransformerNet(FC.net_params(fx, lap_lspe=True))
    with pytest.raises(NotImplementedError, match="edge features"):
        dgl_nets.BatchedTransformerLayer(16, 16, 4, True, use_edge=False)


def test_graph_carries_edata_and_ndata():
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    g = Graph(torch.tensor([0, 1]), torch.tensor([1, 0]), torch.tensor([2]))
    assert g.edata == {} and g.ndata == {}
    g.edata["real"] = torch.tensor([1, 0])
    g.ndata["feat"] = torch.tensor([3, 4])
    h = g.to("cpu")
    assert h is not g and torch.equal(h.edata["real"], g.edata["real"]) and torch.equal(h.ndata["feat"], g.ndata["feat"])


def test_clamp_case_inputs_meet_their_conditions():
    """The op grid's clamp-live input set (tests/test_full_graph_gpu.py): in float64 at least one real and one fake score beyond +5, one
    of each beyond -5, none within 1e-3 of +-5."""
    rp, fp, rm, fm, near = FC.clamp_conditions(FC.op_inputs(**FC.CLAMP_CASE))
    assert rp >= 1 and fp >= 1 and rm >= 1 and fm >= 1 and near == 0, (rp, fp, rm, fm, near)
