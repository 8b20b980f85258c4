"""-m gpu: train-mode dropout in the models.  Fixtures tests/golden/dropout_*.npz hold the reference's own modules run in train mode with
dropout 0.25 on the masks of the counter-based generator (tests/golden/make_dropout.py), in float32 and in float64.

  eval identity   a model built with dropout > 0 is, in eval mode, the dropout = 0 model bit for bit, launch for launch
  fixture parity  train mode without autograd (value path) and under autograd (differentiable path): outputs, BatchNorm buffers and every
                  parameter gradient, by the rules the p = 0 tests of the same fixture family use (tests/test_gnn_types_gpu.py,
                  tests/test_pyg_baselines_gpu.py: parity_util.close_conditioned for a train-mode output, close for a buffer, attributed
                  for a gradient) with the fixture's float64 run as the yardstick
  step behaviour  consecutive forwards draw other masks; seed_dropout makes them repeat; a backward uses its own forward's masks
  state           no state_dict key, no buffer
  refusals        what stays unbuilt still says so
Every figure is printed before it is asserted."""
import functools

import pytest
import torch

import golden_util as G
import parity_util as PU
from parity_util import attributed, close, close_conditioned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLAIN = ["dropout_plain_gnn_gine_h16_l2_add", "dropout_plain_gnn_gcn_h16_l2_mean"]
DGL = ["gatedgcn", "gin", "pna", "transformer", "gat"]
DGL_FX = {f"dropout_{n}_nope": n for n in DGL}
ALL = PLAIN + list(DGL_FX)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return G.load(name)


def _plain_gnn(fx, dropout):
    """dropout > 0: the opt-in class of dropout_models.py; 0: the class every other test builds."""
    from signnet_basisnet_amd import dropout_models, pyg_gnn_types
    GNN = dropout_models.GNN if dropout else pyg_gnn_types.GNN
    nhid, nlayer = (int(v) for v in fx.meta["nhid_nlayer"])
    m = GNN(None, None, nhid, 1, nlayer, str(fx.meta["gnn_type"]), dropout, str(fx.meta["pooling"]), res=True)
    m.load_state_dict(G.full_state_dict(fx), strict=True)
    return m.to(DEV)


def _dgl_net(net, fx, on):
    import test_lap_baselines_cpu as LC
    from test_lap_baselines_gpu import _params_of
    from signnet_basisnet_amd import dgl_nets, dropout_models
    cfg = _params_of(net, fx)
    cfg.update(pe_init="no_pe", lap_method="none", pe_aggregate="none")
    p_in, p_drop = (float(v) for v in fx.meta["p_in_feat_p_drop"])
    if on:
        cfg.update(in_feat_dropout=p_in, dropout=p_drop)
    m = getattr(dropout_models if on else dgl_nets, LC._CLS[net])(cfg)
    if on and net == "transformer":          # as the reference: the net never hands `dropout` to its layers (tests/golden/make_dropout.py)
        for L in m.layers:
            L.dropout = p_drop
    m.load_state_dict(fx.sd, strict=True)
    return m.to(DEV)


def build(name, on):
    fx = fixture(name)
    return _dgl_net(DGL_FX[name], fx, on) if name in DGL_FX else _plain_gnn(fx, 0.25 if on else 0)


def _data(name):
    from signnet_basisnet_amd import synth
    fx = fixture(name)
    if name in DGL_FX:
        from test_lap_baselines_gpu import _inputs
        return _inputs(fx)          # (a fresh graph object: a batch plan is cached on it by the first forward that sees it)
    return synth.batch_to(G.as_data(fx.inp), DEV)


def run(name, model):
    d = _data(name)
    if name in DGL_FX:
        g, h, e, sn = d
        return model(g, h, None, e, sn)[0]
    return model(d)


def _seed(model, fx):
    """The fixture's forward is step `dropout_step`: a train-mode forward advances the step first."""
    model.seed_dropout(int(fx.meta["dropout_seed"]), int(fx.meta["dropout_step"]) - 1)
    return float(fx.meta["dropout_p"])


def _names(name, model):
    from signnet_basisnet_amd import ops
    rec = ops.KernelTimer()
    with rec, torch.no_grad():
        y = run(name, model)
    return y, [s[0] for s in rec.spans]


# ----------------------------------------------------------------------------- eval identity
@pytest.mark.parametrize("name", ALL)
def test_eval_mode_is_the_dropout_free_model(name):
    fx = fixture(name)
    y0, n0 = _names(name, build(name, False).eval())
    y1, n1 = _names(name, build(name, True).eval())
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
    assert n0 == n1 and n1 and "sn_dropout_f32" not in n1
    close(y1, fx.out["eval/y"], f"{name}: eval y")
    # and train mode with p = 0 launches no dropout either
    _, nt = _names(name, build(name, False).train())
    assert "sn_dropout_f32" not in nt


# ----------------------------------------------------------------------------- fixture parity
def _check_buffers(model, fx, what):
    sd = model.state_dict()
    n = 0
    for k, ref in fx.out.items():
        if not k.startswith("train/buffers/"):
            continue
        key = k[len("train/buffers/"):]
        if key.endswith("num_batches_tracked"):
            assert int(sd[key]) == int(ref), f"{what}: {key}"
        else:
            close(sd[key], ref, f"{what}: {key}")
        n += 1
    assert n


def _check_gradients(model, fx, name):
    g32 = {k[len("train/grad/"):]: v for k, v in fx.out.items() if k.startswith("train/grad/")}
    g64 = {k[len("train/grad64/"):]: v for k, v in fx.out.items() if k.startswith("train/grad64/")}
    assert g32 and set(g32) == set(g64)
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    used = {k for k, g in g64.items() if bool(g.any()) and ".layer.nn." not in k and ".lin_dst." not in k}
    assert used <= set(got), sorted(used - set(got))
    # (a bias in front of a batch-statistics BatchNorm has the gradient 0 and float64 returns its rounding noise: compared together with
    #  its Linear's weight gradient, as tests/test_gnn_types_gpu.py does)
    gmax = max(float(g.abs().max()) for g in g64.values())
    paired = {k for k in used if k.endswith(".bias") and float(g64[k].abs().max()) <= 1e-12 * gmax and k[:-4] + "weight" in used}
    for k in sorted(used):
        print(f"{name} d {k}: |hip - f64| {PU.relerr(got[k], g64[k]):.2e}  |ref32 - f64| {PU.relerr(g32[k], g64[k]):.2e}")
    for k in sorted(used - paired):
        attributed(got[k], g32[k], g64[k], f"{name}: d {k}")
    for k in sorted(paired):
        w = k[:-4] + "weight"
        both = lambda g: torch.cat([g[w].detach().cpu().reshape(-1), g[k].detach().cpu().reshape(-1)])          # noqa: E731
        attributed(both(got), both(g32), both(g64), f"{name}: d ({w} | {k})")
    for k in set(got) - used:
        assert not bool(got[k].any()), k


@pytest.mark.parametrize("name", PLAIN)
def test_train_mode_against_the_reference_fixture(name):
    fx = fixture(name)
    y32, y64 = fx.out["train/y"], fx.out["train/y64"]
    # value path: train mode without autograd
    model = build(name, True).train()
    assert _seed(model, fx) == model.dropout
    yv, names = _names(name, model)
    assert names.count("sn_dropout_f32") == len(fx.meta["dropout_site_shapes"])
    print(f"{name} train y: |hip - ref| {PU.relerr(yv, y32):.2e}  |hip - f64| {PU.relerr(yv, y64):.2e}  |ref - f64| {PU.relerr(y32, y64):.2e}")
    close_conditioned(yv, y32, y64, f"{name}: train y")
    _check_buffers(model, fx, f"{name} (train, no autograd)")
    # and it is not the dropout-free output
    with torch.no_grad():
        y0 = run(name, build(name, False).train())
    assert PU.relerr(y0, y64) > 1e-3
    # differentiable path
    model = build(name, True).train()
    _seed(model, fx)
    yg = run(name, model)
    print(f"{name} train y (autograd): |hip - f64| {PU.relerr(yg, y64):.2e}")
    close_conditioned(yg, y32, y64, f"{name}: train y (autograd)")
    (yg * fx.inp["cotangent"].to(DEV)).sum().backward()
    _check_buffers(model, fx, f"{name} (train, autograd)")
    _check_gradients(model, fx, name)


@pytest.mark.parametrize("name", list(DGL_FX))
def test_dgl_net_train_mode_against_the_reference_fixture(name):
    """The tolerances of the p = 0 tests of the same nets on the sibling baseline_<net>_nope fixtures (tests/test_lap_baselines_gpu.py):
    TRAIN_TOL for the scores, _check_param_grads at GRAD_TOL for the gradients against float64; buffers by parity_util.close."""
    from test_dgl_basisnet_gpu import _check_param_grads
    from test_lap_baselines_gpu import GRAD_TOL, TRAIN_TOL
    net = DGL_FX[name]
    fx = fixture(name)
    y32, y64 = fx.out["train/y"], fx.out["train/y64"]
    rtol, atol = TRAIN_TOL[net]
    model = build(name, True).train()
    _seed(model, fx)
    yv, names = _names(name, model)
    assert names.count("sn_dropout_f32") == len(fx.meta["dropout_site_shapes"]), names
    print(f"{name} train y: |hip - ref| {PU.relerr(yv, y32):.2e}  |hip - f64| {PU.relerr(yv, y64):.2e}  |ref - f64| {PU.relerr(y32, y64):.2e}")
    torch.testing.assert_close(yv.cpu(), y32, rtol=rtol, atol=atol)
    if any(k.startswith("train/buffers/") for k in fx.out):
        _check_buffers(model, fx, f"{name} (train, no autograd)")
    with torch.no_grad():
        y0 = run(name, build(name, False).train())
    assert PU.relerr(y0, y64) > 1e-3
    model = build(name, True).train()
    _seed(model, fx)
    yg = run(name, model)
    assert yg.requires_grad
    print(f"{name} train y (autograd): |hip - f64| {PU.relerr(yg, y64):.2e}")
    torch.testing.assert_close(yg.detach().cpu(), y32, rtol=rtol, atol=atol)
    (yg * fx.inp["cotangent"].to(DEV)).sum().backward()
    if any(k.startswith("train/buffers/") for k in fx.out):
        _check_buffers(model, fx, f"{name} (train, autograd)")
    sd64 = {}
    for k, v in fx.sd.items():
        if v.is_floating_point() and "running" not in k:
            t = v.double().requires_grad_(True)
            t.grad = fx.out.get("train/grad64/" + k)
            sd64[k] = t
    for k, p_ in model.named_parameters():
        if k in sd64 and sd64[k].grad is not None and p_.grad is not None:
            print(f"{name} d {k}: |hip - f64| {PU.relerr(p_.grad, sd64[k].grad):.2e}")
    _check_param_grads(model, sd64, name, tol=GRAD_TOL[net])


# ----------------------------------------------------------------------------- step behaviour
@pytest.mark.parametrize("name", ALL)
def test_steps_differ_repeat_after_seeding_and_a_backward_uses_its_own_masks(name):
    fx = fixture(name)
    model = build(name, True).train()
    model.seed_dropout(7, 0)
    with torch.no_grad():
        a1, a2 = run(name, model), run(name, model)
    assert not torch.equal(a1, a2)
    model.seed_dropout(7, 0)
    with torch.no_grad():
        b1, b2 = run(name, model), run(name, model)
    assert torch.equal(a1.view(torch.int32), b1.view(torch.int32)) and torch.equal(a2.view(torch.int32), b2.view(torch.int32))
    # the differentiable path draws the same masks as the value path
    model.seed_dropout(7, 0)
    yA = run(name, model)
    # (other masks move the output by O(1); the same masks leave fp32 rounding through a BatchNorm over the few pooled rows)
    assert PU.relerr(yA, a1) < 1e-2, PU.relerr(yA, a1)

    def grads():
        g = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        return g

    # forward A, forward B, backward B, backward A: A's gradients are those of A's own masks
    cot = fx.inp["cotangent"].to(DEV)
    model.seed_dropout(7, 0)
    yA = run(name, model)
    yB = run(name, model)
    (yB * cot).sum().backward()
    gB = grads()
    (yA * cot).sum().backward()
    gA = grads()
    model.seed_dropout(7, 0)
    (run(name, model) * cot).sum().backward()
    gA_alone = grads()
    model.seed_dropout(7, 1)
    (run(name, model) * cot).sum().backward()
    gB_alone = grads()
    assert set(gA) == set(gA_alone)
    for k in gA:
        if bool(gA_alone[k].any()):
            close(gA[k], gA_alone[k], f"{name}: d {k} of forward A after an interleaved forward")
            close(gB[k], gB_alone[k], f"{name}: d {k} of forward B")
    assert max(PU.relerr(gA[k], gB[k]) for k in gA if bool(gB[k].any())) > 1e-2


def test_default_seed_follows_torch_manual_seed():
    name = PLAIN[0]
    outs = []
    for _ in range(2):
        torch.manual_seed(4321)
        model = build(name, True).train()
        with torch.no_grad():
            outs.append(run(name, model))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert model.dropout_state(torch.device(DEV)).t.tolist() == [4321, 1]


# ----------------------------------------------------------------------------- the state stays out of the module
@pytest.mark.parametrize("name", ALL)
def test_the_state_is_no_buffer_and_no_state_dict_key(name):
    m0, m1 = build(name, False).train(), build(name, True).train()
    with torch.no_grad():
        run(name, m0), run(name, m1)
    assert list(m0.state_dict().keys()) == list(m1.state_dict().keys())
    assert len(list(m0.buffers())) == len(list(m1.buffers()))
    assert len(list(m0.parameters())) == len(list(m1.parameters()))
    m1.seed_dropout(3, 5)
    assert m1.dropout_state(torch.device(DEV)).t.tolist() == [3, 5]


# ----------------------------------------------------------------------------- the captured step
def test_dgl_bucketed_step_replays_draw_the_eager_steps_masks():
    """GatedGCN NoPE, dropout 0.25: replay j of the captured step equals eager step j from the same seed (j = 1, 2), by the eager-vs-
    bucketed loss check of tests/test_dgl_bucketed_step_gpu.py (_close_losses; this net reads no continuous input, so its sensitivity
    term is zero and every loss is held to 1e-6 relative) — which it could not if the capture's warm-up forwards had consumed steps."""
    from test_dgl_bucketed_step_gpu import _close_losses
    from test_lap_baselines_gpu import _inputs, _params_of
    from signnet_basisnet_amd import dropout_models, optim
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    fx = fixture("dropout_gatedgcn_nope")
    g, h, e, sn = _inputs(fx)
    t = torch.randn(len(fx.inp["sizes"]), 1, generator=torch.Generator().manual_seed(9)).to(DEV)

    def net():
        cfg = _params_of("gatedgcn", fx)
        cfg.update(pe_init="no_pe", lap_method="none", pe_aggregate="none", in_feat_dropout=0.25, dropout=0.25)
        torch.manual_seed(3)
        m = dropout_models.GatedGCNNet(cfg).to(DEV).train()
        return m, optim.FlatAdam(m.parameters(), lr=1e-4)

    def eager(step0, n=2):
        m, o = net()
        m.seed_dropout(11, step0)
        losses = []
        for _ in range(n):
            o.zero_grad()
            loss = m.loss(m(g, h, None, e, sn)[0], t)
            loss.backward()
            o.step()
            losses.append(loss.item())
        return losses

    want = eager(0)
    m2, o2 = net()
    m2.seed_dropout(11, 0)
    s = DGLBucketedStep(m2, o2, max_graphs=8, warmup=2)
    padded = [s.step(g, h, None, e, sn, t).item() for _ in range(2)]
    s.check()
    assert s.captures == 1 and s.hits == 1
    shifted = eager(2)                   # what the replays would follow had the two warm-up forwards counted
    print(f"eager {want}  padded {padded}  eager from step 2 {shifted}")
    assert padded[0] != padded[1]
    _close_losses(want, want, padded)
    assert abs(shifted[0] - want[0]) > 1e-3 * abs(want[0])
    assert m2.dropout_state(torch.device(DEV)).t.tolist() == [11, 2]
    assert list(m2.state_dict().keys()) == list(net()[0].state_dict().keys())
    s.release()
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- refusals that stay
def test_what_stays_unbuilt_still_refuses():
    from signnet_basisnet_amd import basisnet, dgl_deepsigns, dropout_models, filter_baselines, learning_filters
    with pytest.raises(NotImplementedError, match="dropout"):          # sign_inv with dropout > 0: refused at get_sign_inv_net
        fx = fixture("dropout_gatedgcn_nope")
        from test_lap_baselines_gpu import _params_of
        dropout_models.GatedGCNNet(dict(_params_of("gatedgcn", fx), pe_init="lap_pe", lap_method="sign_inv", pe_aggregate="add",
                                        sign_inv_net="gin", sign_inv_layers=3, sign_inv_activation="relu", phi_out_dim=4, dropout=0.1))
    for cls in ("GINDeepSigns", "MaskedGINDeepSigns", "GCNDeepSigns", "TransformerDeepSigns"):
        with pytest.raises(NotImplementedError, match=r"dropout=0.1 is not implemented by the HIP modules \(the shipped configs use 0.0\)"):
            args = (1, 8, 4, 3, 6, None) if cls == "MaskedGINDeepSigns" else (1, 8, 4, 3, 6)
            getattr(dgl_deepsigns, cls)(*args, use_bn=True, dropout=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        dgl_deepsigns.get_sign_inv_net(dict(sign_inv_net="gin", hidden_dim=8, phi_out_dim=4, sign_inv_layers=3, pos_enc_dim=6, dropout=0.1,
                                            sign_inv_activation="relu", device=DEV))
    with pytest.raises(NotImplementedError, match="MLP: dropout > 0 is not built"):
        learning_filters.MLP(4, dropout=0.1)
    with pytest.raises(NotImplementedError, match="Transformer: dropout > 0 is not built"):
        learning_filters.Transformer(4, dropout=0.1)
    with pytest.raises(NotImplementedError, match="EqDeepSetsEncoder: dropout > 0 is not built"):
        basisnet.EqDeepSetsEncoder(4, dropout=0.1)
    with pytest.raises(NotImplementedError, match="GATConv: dropout != 0 is not built"):
        filter_baselines.GATConv(8, 8, dropout=0.5)
    with pytest.raises(NotImplementedError, match="ARMAConv: dropout != 0 is not built"):
        filter_baselines.ARMAConv(8, 8, dropout=0.5)
