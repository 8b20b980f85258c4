"""CPU: readout='max' — the restatement of tests/readout_max_cases.py against the reference's fixtures, the fixtures' gap rule, the
opt-in classes of readout_models.py, the drop-in table and the C ABI's argument checks.  No launches."""
import pytest
import torch

import readout_max_cases as RC

NETS = ["GINNet", "GatedGCNNet", "PNANet", "TransformerNet", "GATNet"]


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_restatement_reproduces_the_reference_pooled_rows(name):
    fx = RC.fixture(name)
    sizes = [int(s) for s in fx.inp["sizes"]]
    for mode in ("eval", "train"):
        for tag in ("", "64"):
            h, hg = fx.out[f"{mode}/h_last{tag}"], fx.out[f"{mode}/hg{tag}"]
            out, arg = RC.segment_max_ref(h, sizes)
            assert torch.equal(out.to(hg.dtype), hg), (name, mode, tag)
            # the adjoint's one non-zero per (graph, channel) sits where the maximum is
            dx = RC.segment_max_bwd_ref(torch.ones_like(out), arg, sizes, h.shape[0])
            assert int((dx != 0).sum()) == out.numel()
            assert torch.equal(h.double()[dx != 0].sort().values, out.reshape(-1).sort().values)


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_fixture_gaps_clear_the_rule(name):
    fx = RC.fixture(name)
    sizes = [int(s) for s in fx.inp["sizes"]]
    for mode in ("eval", "train"):
        gap = torch.from_numpy(fx.meta[f"gap_{mode}"])
        h = fx.out[f"{mode}/h_last"].double()
        assert gap.shape == (len(sizes), h.shape[1])
        # recomputed from the stored node features
        scale, r = h.abs().amax(0), 0
        for b, n in enumerate(sizes):
            top = h[r:r + n].topk(2, dim=0).values
            assert torch.equal(gap[b], (top[0] - top[1]) / scale), (name, mode, b)
            r += n
        print(f"{name} {mode}: smallest gap {float(gap.min()):.2e}")
        assert float(gap.min()) >= RC.MIN_GAP
        # float32 and float64 pick the same rows
        assert torch.equal(RC.segment_max_ref(fx.out[f"{mode}/h_last"], sizes)[1], RC.segment_max_ref(fx.out[f"{mode}/h_last64"], sizes)[1])


def test_restatement_rules():
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[1.0, -inf, 2.0], [3.0, -inf, nan], [3.0, -inf, nan], [0.5, 7.0, 1.0]])
    out, arg = RC.segment_max_ref(x, [0, 3, 0, 1, 0])
    assert torch.equal(arg, torch.tensor([[-1] * 3, [1, 0, 1], [-1] * 3, [3, 3, 3], [-1] * 3], dtype=torch.int32))
    assert torch.equal(out[[0, 2, 4]], torch.zeros(3, 3, dtype=torch.float64))
    assert out[1].tolist()[:2] == [3.0, -inf] and bool(torch.isnan(out[1, 2])) and out[3].tolist() == [0.5, 7.0, 1.0]
    dx = RC.segment_max_bwd_ref(torch.tensor([[9.0] * 3, [1.0, 2.0, 3.0], [9.0] * 3, [4.0, 5.0, 6.0], [9.0] * 3]), arg, [0, 3, 0, 1, 0], 4)
    assert torch.equal(dx, torch.tensor([[0, 2.0, 0], [1.0, 0, 3.0], [0, 0, 0], [4.0, 5.0, 6.0]], dtype=torch.float64))


def test_table_covers_what_it_claims():
    sizes = {n for l in RC.SIZE_LISTS for n in l}
    assert sizes == {0, 1, 2, 15, 16, 17, 64, 65, 300, 2100}
    first, last = RC.SIZE_LISTS[0][0], RC.SIZE_LISTS[0][-1]
    assert first == 0 and last == 0 and 0 in RC.SIZE_LISTS[0][1:-1]
    assert RC.WIDTHS == [1, 3, 4, 64, 77, 95, 128, 260]


# ----------------------------------------------------------------------------- the classes
def test_base_classes_still_refuse_max():
    from signnet_basisnet_amd import dgl_nets, dropout_models, dropout_signinv
    for name in RC.FIXTURES[:5]:
        fx = RC.fixture(name)
        cls = RC.CLS[str(fx.meta["net"])]
        for mod in (dgl_nets, dropout_models, dropout_signinv):
            with pytest.raises(NotImplementedError, match="readout"):
                getattr(mod, cls)(RC.net_params(fx))


@pytest.mark.parametrize("name", RC.FIXTURES)
def test_readout_models_construct_with_the_keys_of_their_bases(name):
    from signnet_basisnet_amd import dropout_signinv, readout_models
    fx = RC.fixture(name)
    cls = RC.CLS[str(fx.meta["net"])]
    m = getattr(readout_models, cls)(RC.net_params(fx))
    assert m.readout == "max" and m._max_readout and issubclass(type(m), getattr(dropout_signinv, cls))
    assert [str(k) for k in fx.meta["sd_keys"]] == list(m.state_dict().keys())          # the reference's keys, in its order
    base = getattr(dropout_signinv, cls)(RC.net_params(fx, readout="mean"))
    assert list(base.state_dict().keys()) == list(m.state_dict().keys())
    m.load_state_dict(fx.sd, strict=True)
    assert sorted(readout_models.NETS) == sorted(NETS)
    # one attribute apart: nothing else is defined on the subclass
    assert {k for k in vars(type(m)) if not k.startswith("__")} == {"_max_readout"}
    # dropout and max together
    both = getattr(readout_models, cls)(RC.net_params(fx, dropout=0.1))
    assert both.p_drop == 0.1 and both.readout == "max"
    with pytest.raises(NotImplementedError):
        getattr(readout_models, cls)(RC.net_params(fx, lap_lspe=True))


# ----------------------------------------------------------------------------- the drop-in table
_NET_MODULES = ["nets.ZINC_graph_regression." + m for m in ("gin_net", "gatedgcn_net", "pna_net", "transformer_net", "gat_net")]


def test_dropin_table_with_and_without_max_readout():
    from signnet_basisnet_amd import dropin
    pkg = "signnet_basisnet_amd.dropin"
    plain = dropin.AliasFinder("graphprediction").table
    assert plain == dropin.ALIASES["graphprediction"]
    for m in _NET_MODULES:
        assert plain[m] == f"{pkg}.graphprediction.{m}"
    sd = dropin.AliasFinder("graphprediction", sign_inv_dropout=True).table
    assert all(sd[m] == pkg + ".signinv_dropout_nets" for m in _NET_MODULES)
    mx = dropin.AliasFinder("graphprediction", max_readout=True).table
    assert all(mx[m] == pkg + ".max_readout_nets" for m in _NET_MODULES)
    assert mx["nets.ZINC_graph_regression.sign_inv_net"] == pkg + ".signinv_dropout_nets"          # implies sign_inv_dropout
    assert mx["layers.deepsigns"] == plain["layers.deepsigns"]
    for tree in ("alchemy", "gine_pyg", "learningfilters"):
        assert dropin.AliasFinder(tree, max_readout=True).table == dropin.AliasFinder(tree, sign_inv_dropout=True).table


def _resolve(finder, name):
    import importlib
    spec = finder.find_spec(name)
    assert spec is not None, name
    return importlib.import_module(spec.origin)


def test_dropin_install_rebinds_the_five_names():
    """What `dropin.run --max-readout main_ZINC_graph_regression.py --config ... --readout max` imports."""
    from signnet_basisnet_amd import dgl_deepsigns, dgl_nets, dropin, dropout_signinv, readout_models
    dropin.uninstall("graphprediction")
    try:
        f = dropin.install("graphprediction", sign_inv_dropout=True)
        assert _resolve(f, _NET_MODULES[1]).GatedGCNNet is dropout_signinv.GatedGCNNet
        assert dropin.install("graphprediction", max_readout=True) is f          # extends the installed finder in place
        for m, cls in zip(_NET_MODULES, NETS):
            assert getattr(_resolve(f, m), cls) is getattr(readout_models, cls)
        assert _resolve(f, "nets.ZINC_graph_regression.sign_inv_net").get_sign_inv_net is dropout_signinv.get_sign_inv_net
        dropin.install("graphprediction", sign_inv_dropout=True)                # a later call with less takes nothing away
        assert _resolve(f, _NET_MODULES[0]).GINNet is readout_models.GINNet
        assert f.find_spec("nets.ZINC_graph_regression.load_net") is None         # everything else stays the tree's
    finally:
        dropin.uninstall("graphprediction")
    f = dropin.install("graphprediction")          # without the flag every name resolves as before, and max is refused as before
    try:
        mod = _resolve(f, _NET_MODULES[1])
        assert mod.GatedGCNNet is dgl_nets.GatedGCNNet
        assert _resolve(f, "nets.ZINC_graph_regression.sign_inv_net").get_sign_inv_net is dgl_deepsigns.get_sign_inv_net
        with pytest.raises(NotImplementedError, match="readout"):
            mod.GatedGCNNet(RC.net_params(RC.fixture("readout_max_gatedgcn")))
    finally:
        dropin.uninstall("graphprediction")


def test_runner_flag(monkeypatch, tmp_path):
    from signnet_basisnet_amd import dropin
    from signnet_basisnet_amd.dropin import run
    seen = {}
    monkeypatch.setattr(run, "install", lambda tree, **kw: seen.update(tree=tree, **kw))
    script = tmp_path / "main_ZINC_graph_regression.py"
    script.write_text("import sys\nARGS = list(sys.argv)\n")
    argv = list(__import__("sys").argv)
    path = list(__import__("sys").path)
    try:
        run.main(["--max-readout", str(script), "--readout", "max"])
    finally:
        __import__("sys").argv[:] = argv
        __import__("sys").path[:] = path
    assert seen == dict(tree="graphprediction", baselines=False, gnn_types=False, feature_dropout=True, sign_inv_dropout=True, max_readout=True)
    assert "--max-readout" in run.__doc__ and "MAX_READOUT_OVERRIDES" in dropin.install.__doc__


# ----------------------------------------------------------------------------- the C ABI
def test_c_abi_exports_and_argument_errors():
    from signnet_basisnet_amd import _lib
    L = _lib.lib()
    one = 16          # any non-NULL address: the checks run on the host before any launch
    for args in ((None, 1, 4, one, one, one, None), (one, 1, 0, one, one, one, None), (one, 1, -3, one, one, one, None),
                 (one, -1, 4, one, one, one, None), (one, 1, 4, None, one, one, None), (one, 1, 4, one, None, one, None)):
        assert L.sn_segment_max_f32(*args) == -1 and b"sn_segment_max_f32" in L.sn_last_error(), args
    for args in ((None, one, 1, 4, one, one, None), (one, None, 1, 4, one, one, None), (one, one, 1, 0, one, one, None),
                 (one, one, -1, 4, one, one, None), (one, one, 1, 4, None, one, None), (one, one, 1, 4, one, None, None)):
        assert L.sn_segment_max_bwd_f32(*args) == -1 and b"sn_segment_max_bwd_f32" in L.sn_last_error(), args
    # B == 0: nothing to do, no launch (arg may be NULL)
    assert L.sn_segment_max_f32(one, 0, 4, one, one, None, None) == 0
    assert L.sn_segment_max_bwd_f32(one, one, 0, 4, one, one, None) == 0
    hdr = open(__import__("os").path.join(__import__("os").path.dirname(_lib._HERE), "include", "signnet_hip.h")).read()
    for name, v in (("SN_READOUT_SUM", 0), ("SN_READOUT_MEAN", 1), ("SN_READOUT_MAX", 2)):
        assert f"#define {name} {v}\n" in hdr
    from signnet_basisnet_amd import dgl_nets
    assert dgl_nets._READOUT_MODE == {"sum": 0, "mean": 1, "max": 2}
