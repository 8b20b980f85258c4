"""CPU: the restatements of tests/deepsigns_variant_cases.py against the reference's own outputs (tests/golden/ds_*.npz) at the 1e-6 of
tests/test_oracle_golden.py; the modules' keys and shapes; the factory and the drop-in; what the modules refuse."""
import pytest
import torch

import deepsigns_variant_cases as C
import golden_util as G
import parity_util as PU
from test_oracle_golden import TOL_BS

ALL = C.GCN_CASES + C.TF_CASES
TOL = 1e-6


def _rel(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-300)


@pytest.mark.parametrize("name", ALL)
def test_restatement_reproduces_the_reference(name):
    fx = G.load(name)
    assert _rel(C.module_ref(fx, torch.float32), fx.out["eval/y"]) <= TOL
    buffers = {}
    yt = C.module_ref(fx, torch.float32, training=True, buffers=buffers)
    # train mode: rho's batch-statistic BatchNorm runs over the batch's ~40 node rows — the tolerance test_oracle_golden.py keeps for
    # the train mode of the DGL modules (TOL_BS), and both fp32 evaluations as close to the float64 value as each other
    torch.testing.assert_close(yt, fx.out["train/y"], **TOL_BS)
    y64 = C.module_ref(fx, torch.float64, training=True)
    PU.attributed(yt, fx.out["train/y"], y64, f"{name}: train y")
    want = {k[len("train/buffers/"):]: v for k, v in fx.out.items() if k.startswith("train/buffers/")}
    assert set(buffers) == set(want)
    for k, v in want.items():
        if k.endswith("num_batches_tracked"):
            assert int(buffers[k]) == int(v), k
        else:
            assert _rel(buffers[k], v) <= TOL, k
    # the GCN encoder runs twice per forward: its BatchNorms count two batches, rho's one
    tracked = {k: int(v) - int(fx.sd[k]) for k, v in want.items() if k.endswith("num_batches_tracked")}
    assert all(n == (2 if k.startswith("enc.") else 1) for k, n in tracked.items()), tracked


@pytest.mark.parametrize("name", ALL)
def test_restatement_gradients_in_float64_agree_with_the_reference(name):
    fx = G.load(name)
    _, g32 = C.module_ref(fx, torch.float32, training=True, grads=True)
    _, g64 = C.module_ref(fx, torch.float64, training=True, grads=True)
    want = {k[len("grad/"):]: v for k, v in fx.out.items() if k.startswith("grad/")}
    assert set(g64) == set(want) == set(g32)
    for k, v in want.items():
        # the formula: the reference's fp32 autograd gradient is the float64 one up to fp32 conditioning (TOL_BS's relative part) ...
        assert _rel(v, g64[k]) <= TOL_BS["rtol"], (k, _rel(v, g64[k]))
        # ... and the restatement in fp32 is as close to it as the reference itself
        PU.attributed(g32[k], v, g64[k], f"{name}: d {k}")


@pytest.mark.parametrize("name", ALL)
def test_keys_and_shapes(name):
    fx = G.load(name)
    net = C.build(fx)
    sd = net.state_dict()
    assert sorted(sd) == sorted(str(k) for k in fx.meta["sd_keys"])
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(fx.sd[k].shape), k
        assert torch.equal(v, fx.sd[k]), k
    assert type(net).__name__ == C.CLASSES[name]


def test_op_restatements_agree_with_each_other():
    for gname in C.PROP_GRAPHS:
        N, src, dst = C.prop_graph(gname)
        x = torch.randn(N, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        b = torch.randn(3, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
        ref = C.gcn_propagate_ref(x.view(N, 2, 3), src, dst, b).reshape(N, 6)
        assert _rel(ref, C.gcn_dense_operator(src, dst, N) @ x + b.repeat(2)) <= 1e-12 or not src.numel()
    # a one-node set attends to itself only
    q, k, v = (torch.randn(3, 4) for _ in range(3))
    assert torch.equal(C.graph_attention_ref(q, k, v, [1], 3, 2), v)


def _params(kind):
    return dict(sign_inv_net=kind, hidden_dim=16, phi_out_dim=4, sign_inv_layers=3, pos_enc_dim=5, dropout=0.0,
                sign_inv_activation="relu", device="cpu")


def test_factory_builds_all_four_kinds():
    from signnet_basisnet_amd import dgl_deepsigns as DS
    want = {"gcn": DS.GCNDeepSigns, "gin": DS.GINDeepSigns, "masked_gin": DS.MaskedGINDeepSigns, "transformer": DS.TransformerDeepSigns}
    for kind, cls in want.items():
        net = DS.get_sign_inv_net(_params(kind))
        assert type(net) is cls and net.k == 5
    with pytest.raises(ValueError, match="Invalid sign inv net"):
        DS.get_sign_inv_net(_params("gat"))
    # the reference's argument lists: rho of the transformer is a 4-layer MLP over hidden * k, phi_out_dim unused
    tf = DS.get_sign_inv_net(_params("transformer"))
    assert len(tf.rho.lins) == 4 and tf.rho.lins[0].weight.shape == (16, 16 * 5) and len(tf.enc.layers) == 3
    gcn = DS.get_sign_inv_net(_params("gcn"))
    assert len(gcn.rho.lins) == 3 and gcn.rho.lins[0].weight.shape == (16, 4 * 5) and gcn.enc.layers[-1].weight.shape == (16, 4)
    assert len(gcn.enc.bns) == 2


def test_odd_hidden_width_builds():
    from signnet_basisnet_amd import dgl_deepsigns as DS
    tf = DS.TransformerDeepSigns(1, 95, 4, 2, 8, use_bn=True, dropout=0.0)
    m = tf.enc.layers[0].mha
    assert m.proj_q.weight.shape == (94, 95) and m.proj_o.weight.shape == (95, 94) and m.ffn[0].weight.shape == (94, 95)


def test_dropin_resolves_the_new_names():
    import importlib
    from signnet_basisnet_amd import dgl_deepsigns as DS
    mod = importlib.import_module("signnet_basisnet_amd.dropin.graphprediction.layers.deepsigns")
    for n in ("GCNDeepSigns", "TransformerDeepSigns", "GCN", "GINDeepSigns", "MaskedGINDeepSigns", "GIN", "MLP"):
        assert getattr(mod, n) is getattr(DS, n), n


@pytest.mark.parametrize("cls", ["GCNDeepSigns", "TransformerDeepSigns"])
def test_refusals(cls):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    K = getattr(DS, cls)
    with pytest.raises(NotImplementedError, match="dropout"):
        K(1, 16, 4, 3, 5, use_bn=True, dropout=0.1)
    with pytest.raises(ValueError):
        K(1, 16, 4, 3, 5, use_bn=True, dropout=0.0, activation="tanh")
    with pytest.raises(ValueError):
        K(1, 16, 4, 3, 5, use_bn=True, use_ln=True, dropout=0.0)
    net = K(1, 16, 4, 3, 5, use_bn=True, dropout=0.0)
    assert net.matmul_precision == "highest"
    net.matmul_precision = "highest"
    for mode in ("high", "medium"):
        with pytest.raises(ValueError, match="matmul_precision"):
            net.matmul_precision = mode
    assert net.matmul_precision == "highest"
    assert not hasattr(net, "fused_stages")


@pytest.mark.parametrize("name", [C.GCN_CASES[0], C.TF_CASES[0]])
@pytest.mark.parametrize("train", [False, True])
def test_host_tensors_raise_gpu_only(name, train):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    fx = G.load(name)
    net = C.build(fx).train(train)
    ei = fx.inp["edge_index"]
    g = DS.Graph(ei[0], ei[1], fx.inp["sizes"])
    with pytest.raises(RuntimeError, match="GPU only"):
        net(g, fx.inp["pos_enc"].unsqueeze(-1))
