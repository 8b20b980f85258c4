"""-m gpu: the PyG trees' baselines on the device — the Set2Set kernel (sn_set2set_f32 / sn_set2set_bwd_f32) against the float64
restatement of tests/pyg_baseline_cases.py under the rules of tests/parity_util.py (values: close(rel=1e-5, ref64); gradients:
attributed()), NetGINE and the plain GINE GNN against the reference's own outputs (tests/golden/netgine_*.npz, plain_gnn_*.npz) and
their float64 restatements, and SignNetGNN untouched by all of it.  Every figure is printed before it is asserted."""
import functools

import pytest
import torch

import golden_util as G
import parity_util as PU
import pyg_baseline_cases as C
from parity_util import attributed, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def offset_view(t):
    """a contiguous device copy of t that starts 4 bytes into a 16-byte aligned buffer"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def graph_ptr(sizes):
    return torch.tensor([0] + list(sizes), dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)


@functools.lru_cache(maxsize=None)
def set2set_refs(case):
    """(inputs, (out32, grads32), (out64, grads64)): computed once per case, shared, never modified."""
    inp = C.set2set_inputs(case)
    return inp, C.set2set_ref_grads(inp, torch.float32), C.set2set_ref_grads(inp, torch.float64)


def run_set2set(inp):
    from signnet_basisnet_amd import autograd as AG
    x = (offset_view(inp.x) if inp.offset else inp.x.to(DEV)).detach().requires_grad_(True)
    lstm = {k: v.to(DEV).requires_grad_(True) for k, v in inp.lstm.items()}
    out = AG.set2set(x, graph_ptr(inp.sizes), *lstm.values(), inp.T)
    out.backward(offset_view(inp.gout) if inp.offset else inp.gout.to(DEV))
    return out.detach(), {"x": x.grad, **{k: v.grad for k, v in lstm.items()}}


# ----------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("case", list(C.SET2SET_CASES))
def test_set2set_forward_and_backward_against_float64(case):
    from signnet_basisnet_amd import ops
    inp, (o32, g32), (o64, g64) = set2set_refs(case)
    x = offset_view(inp.x) if inp.offset else inp.x.to(DEV)
    eval_out = ops.set2set(x, graph_ptr(inp.sizes), *(v.to(DEV) for v in inp.lstm.values()), inp.T)      # no tape
    out, grads = run_set2set(inp)
    assert out.shape == (len(inp.sizes), 2 * inp.d) and bool(torch.isfinite(out).all())
    for what, o in (("eval", eval_out), ("train", out)):
        print(f"{case} {what}: |hip - f64| {PU.relerr(o, o64):.2e}  |cpu32 - f64| {PU.relerr(o32, o64):.2e}  |hip - cpu32| {PU.relerr(o, o32):.2e}")
    for what, o in (("eval", eval_out), ("train", out)):
        close(o, o32, f"{case}: q* ({what})", rel=1e-5, ref64=o64)
        for b, n in enumerate(inp.sizes):
            if n == 0:
                assert not bool(o[b, inp.d:].any()), f"{case}: r of the empty graph {b} ({what})"
    for k in g64:
        assert grads[k].shape == g64[k].shape, k
        e_hip, e_cpu = (grads[k].cpu().double() - g64[k]).abs().max().item(), (g32[k].double() - g64[k]).abs().max().item()
        s = max(g64[k].abs().max().item(), 1e-300)          # (T = 1: the cell's input and state are 0, both weight gradients vanish)
        print(f"{case} d {k}: |hip - f64| {e_hip / s:.2e}  |cpu32 - f64| {e_cpu / s:.2e}")
    for k in g64:
        attributed(grads[k], g32[k], g64[k], f"{case}: d {k}")


@pytest.mark.parametrize("case", ["d100_T6", "empty_ends"])
def test_set2set_gradients_are_bit_reproducible(case):
    inp = set2set_refs(case)[0]
    (o1, g1), (o2, g2) = run_set2set(inp), run_set2set(inp)
    assert torch.equal(o1, o2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


# ----------------------------------------------------------------------------- NetGINE
def _netgine(fx):
    from signnet_basisnet_amd.pyg_baselines import NetGINE
    m = NetGINE(int(fx.meta["dim"]))
    m.load_state_dict(fx.sd, strict=True)
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def netgine_refs64(name):
    """float64: eval output, the gradients of the first step, the L1 losses of the first two Adam steps (torch.optim.Adam), the output
    after those two steps."""
    fx = G.load(name)
    data = PU.data_f64(G.as_data(fx.inp))
    sd = C.leaf_state_dict(fx.sd, torch.float64)
    lr, wd = (float(v) for v in fx.meta["lr_wd"])
    opt = torch.optim.Adam(list(sd.values()), lr=lr, weight_decay=wd)
    with torch.no_grad():
        y = C.netgine_ref(sd, data)
    losses, grads = [], None
    for step in range(2):
        opt.zero_grad()
        loss = torch.nn.functional.l1_loss(C.netgine_ref(sd, data), fx.inp["y_target"].double())
        loss.backward()
        if step == 0:
            grads = {k: v.grad.detach().clone() for k, v in sd.items()}
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        y_after = C.netgine_ref(sd, data)
    return y, grads, torch.stack(losses), y_after


@pytest.mark.parametrize("name", C.NETGINE_CASES)
def test_netgine_on_the_reference_fixtures(name):
    from signnet_basisnet_amd import optim, synth
    fx, gr = G.load(name), G.load(name + "_grads")
    assert 1 in fx.inp["sizes"].tolist()
    y64, g64, l64, _ = netgine_refs64(name)
    data = synth.batch_to(G.as_data(fx.inp), DEV)
    target = fx.inp["y_target"].to(DEV)
    model = _netgine(fx).eval()
    with torch.no_grad():
        y = model(data)
    print(f"{name} eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, y64):.2e}")
    close(y, fx.out["eval/y"], f"{name}: eval y", ref64=y64)
    model.train()
    lr, wd = (float(v) for v in fx.meta["lr_wd"])
    opt = optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
    losses = []
    for step in range(2):
        opt.zero_grad()
        loss = torch.nn.functional.l1_loss(model(data), target)
        loss.backward()
        if step == 0:
            grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
        opt.step()
        losses.append(loss.detach())
    losses = torch.stack(losses)
    print(f"{name} losses: hip {losses.tolist()}  ref {fx.out['loss'].tolist()}  f64 {l64.tolist()}")
    close(losses[0], fx.out["loss"][0], f"{name}: loss", ref64=l64[0])
    assert set(grads) == set(fx.sd) == {k[len("grad/"):] for k in gr.out}
    for k in grads:
        print(f"{name} d {k}: |hip - ref| {PU.relerr(grads[k], gr.out['grad/' + k]):.2e}  |hip - f64| {PU.relerr(grads[k], g64[k]):.2e}  "
              f"|ref - f64| {PU.relerr(gr.out['grad/' + k], g64[k]):.2e}")
    for k in grads:          # the fixture's gradients are the reference's own autograd
        attributed(grads[k], gr.out["grad/" + k], g64[k], f"{name}: d {k}")
    close(losses[1], fx.out["loss"][1], f"{name}: loss at the second Adam step", ref64=l64[1])


def _adam_steps(model, args, target, n=2, lr=1e-3, wd=1e-5):
    from signnet_basisnet_amd import optim
    opt = optim.Adam(model.parameters(), lr=lr, weight_decay=wd)
    model.train()
    for _ in range(n):
        opt.zero_grad()
        torch.nn.functional.l1_loss(model(*args), target).backward()
        opt.step()


@pytest.mark.parametrize("stay_in_train_mode", [False, True])
def test_netgine_forward_after_optimiser_steps_uses_the_new_weights(stay_in_train_mode):
    """The device optimiser writes parameters through raw pointers: the eval forward's packed weights must not outlive it.  Forward
    without autograd (eval mode, or train mode under no_grad), two optim.Adam steps, the same forward again: float64 after the same
    two steps, and bit for bit what a fresh module holding the trained state_dict computes."""
    from signnet_basisnet_amd import synth
    name = "netgine_d16"
    fx = G.load(name)
    y64, _, _, y64_after = netgine_refs64(name)
    data = synth.batch_to(G.as_data(fx.inp), DEV)
    lr, wd = (float(v) for v in fx.meta["lr_wd"])
    model = _netgine(fx).train(stay_in_train_mode)
    with torch.no_grad():
        close(model(data), fx.out["eval/y"], "before the steps", ref64=y64)
    _adam_steps(model, (data,), fx.inp["y_target"].to(DEV), lr=lr, wd=wd)
    model.train(stay_in_train_mode)
    with torch.no_grad():
        y = model(data)
    print(f"after two steps: |hip - f64| {PU.relerr(y, y64_after):.2e}; the steps moved y by {PU.relerr(y64, y64_after):.2e}")
    assert PU.relerr(y64, y64_after) > 1e-4          # the steps are visible at the tolerance: stale weights cannot pass
    close(y, y64_after.float(), "after two Adam steps", ref64=y64_after)
    fresh = _netgine(fx)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh.eval()(data), y)


def test_plain_gnn_eval_after_optimiser_steps_uses_the_new_weights():
    from signnet_basisnet_amd import synth
    fx = G.load("plain_gnn_h32_l2_mean_pe")
    data = synth.batch_to(G.as_data(fx.inp), DEV)
    pe = fx.inp["additional_x"].to(DEV)
    model = _plain_gnn(fx).eval()
    with torch.no_grad():
        y0 = model(data, pe)
    _adam_steps(model, (data, pe), _cotangent(y0.shape).to(DEV))
    model.eval()
    with torch.no_grad():
        y = model(data, pe)
    fresh = _plain_gnn(fx)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh.eval()(data, pe), y)
    assert PU.relerr(y, y0) > 1e-4


# ----------------------------------------------------------------------------- plain GINE GNN
def _gnn_meta(fx):
    nhid, nlayer = (int(v) for v in fx.meta["nhid_nlayer"])
    return nhid, nlayer, str(fx.meta["pooling"])


def _plain_gnn(fx):
    from signnet_basisnet_amd.dropin.baseline_core_model import GNN
    nhid, nlayer, pooling = _gnn_meta(fx)
    m = GNN(None, None, nhid, 1, nlayer, "GINEConv", 0, pooling, res=True)
    m.load_state_dict(G.full_state_dict(fx), strict=True)
    return m.to(DEV)


def _cotangent(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(5))


@functools.lru_cache(maxsize=None)
def plain_gnn_refs(name):
    """(eval y in float64, train-mode y in float64, train-mode gradients of sum(y * cotangent) in float32 and float64)."""
    fx = G.load(name)
    _, nlayer, pooling = _gnn_meta(fx)
    pe = fx.inp.get("additional_x")
    outs = {}
    for dtype in (torch.float32, torch.float64):
        data = G.as_data(fx.inp) if dtype == torch.float32 else PU.data_f64(G.as_data(fx.inp))
        sd = C.leaf_state_dict(fx.sd, dtype)
        p = None if pe is None else pe.to(dtype)
        with torch.no_grad():
            y_eval = C.plain_gnn_ref(sd, nlayer, pooling, data, p, False)
        y = C.plain_gnn_ref(sd, nlayer, pooling, data, p, True)
        (y * _cotangent(y.shape).to(dtype)).sum().backward()
        outs[dtype] = (y_eval, y.detach(), {k: v.grad for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point() and v.grad is not None})
    return outs


def _check_buffers(model, fx, what):
    sd = model.state_dict()
    for k, ref in fx.out.items():
        if not k.startswith("train/buffers/"):
            continue
        key = k[len("train/buffers/"):]
        if key.endswith("num_batches_tracked"):
            assert int(sd[key]) == int(ref), f"{what}: {key}"
        else:
            close(sd[key], ref, f"{what}: {key}")


@pytest.mark.parametrize("name", C.PLAIN_GNN_CASES)
def test_plain_gnn_on_the_reference_fixtures(name):
    from signnet_basisnet_amd import synth
    fx = G.load(name)
    refs = plain_gnn_refs(name)
    (_, _, g32), (y64_eval, y64_train, g64) = refs[torch.float32], refs[torch.float64]
    data = synth.batch_to(G.as_data(fx.inp), DEV)
    pe = fx.inp.get("additional_x")
    pe = None if pe is None else pe.to(DEV)
    model = _plain_gnn(fx).eval()
    with torch.no_grad():
        y = model(data, pe)
    print(f"{name} eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, y64_eval):.2e}")
    close(y, fx.out["eval/y"], f"{name}: eval y", ref64=y64_eval)
    # train mode without autograd: batch statistics, running statistics moved as the reference moves them
    model.train()
    with torch.no_grad():
        yt = model(data, pe)
    print(f"{name} train y: |hip - ref| {PU.relerr(yt, fx.out['train/y']):.2e}  |hip - f64| {PU.relerr(yt, y64_train):.2e}  "
          f"|ref - f64| {PU.relerr(fx.out['train/y'], y64_train):.2e}")
    close(yt, fx.out["train/y"], f"{name}: train y", ref64=y64_train)
    _check_buffers(model, fx, f"{name} (train, no autograd)")
    # train mode under autograd: the same forward, gradients against float64
    model = _plain_gnn(fx).train()
    yg = model(data, pe)
    close(yg, fx.out["train/y"], f"{name}: train y (autograd)", ref64=y64_train)
    (yg * _cotangent(yg.shape).to(DEV)).sum().backward()
    _check_buffers(model, fx, f"{name} (train, autograd)")
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    used = {k for k, g in g64.items() if bool(g.any())}
    assert used <= set(got), sorted(used - set(got))
    for k in sorted(used):
        print(f"{name} d {k}: |hip - f64| {PU.relerr(got[k], g64[k]):.2e}  |cpu32 - f64| {PU.relerr(g32[k], g64[k]):.2e}")
    for k in sorted(used):
        attributed(got[k], g32[k], g64[k], f"{name}: d {k}")
    for k in set(got) - used:          # a parameter the forward does not use (or whose gradient is exactly 0) gets no gradient
        assert not bool(got[k].any()), k


# ----------------------------------------------------------------------------- nothing shared was disturbed
_UNTOUCHED = r"""
import sys
import torch
import golden_util as G
from signnet_basisnet_amd import synth
from signnet_basisnet_amd.pyg import SignNetGNN
NEW = ("signnet_basisnet_amd.pyg_baselines", "signnet_basisnet_amd.dropin.baseline_core_model")
fx = G.load("gine_d16")
c = [None if v < 0 else int(v) for v in fx.meta["ctor"]]
model = SignNetGNN(*c, variant=str(fx.meta["variant"]))
model.load_state_dict(G.full_state_dict(fx))
model = model.to("cuda:0").eval()
data = synth.batch_to(G.as_data(fx.inp), "cuda:0")
before = model(data).clone()
before_layers = model(data, return_stages=True)[0].clone()
assert not any(m in sys.modules for m in NEW), "the outputs above were to be taken before the new modules are imported"
from signnet_basisnet_amd.dropin.baseline_core_model import GNN
from signnet_basisnet_amd.pyg_baselines import NetGINE
bfx = G.load("netgine_d16")
net = NetGINE(int(bfx.meta["dim"]))
net.load_state_dict(bfx.sd)
net.to("cuda:0").train()(synth.batch_to(G.as_data(bfx.inp), "cuda:0")).sum().backward()
bfx = G.load("plain_gnn_h32_l2_mean_pe")
gnn = GNN(None, None, 32, 1, 2, "GINEConv", 0, "mean")
gnn.load_state_dict(G.full_state_dict(bfx))
gnn.to("cuda:0").train()(synth.batch_to(G.as_data(bfx.inp), "cuda:0"), bfx.inp["additional_x"].to("cuda:0")).sum().backward()
assert torch.equal(model(data), before)
assert torch.equal(model(data, return_stages=True)[0], before_layers)
print("UNTOUCHED " + str(float((before.cpu() - fx.out["eval/y"]).abs().max() / fx.out["eval/y"].abs().max())))
"""


def test_signnet_gnn_is_untouched_by_the_baselines():
    """In a fresh interpreter (in this one the new modules are long imported): SignNetGNN's outputs on an existing fixture, taken before
    the baseline modules are imported, are `torch.equal` to its outputs after they were imported and both models trained a step."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", _UNTOUCHED], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "UNTOUCHED " in out.stdout, out.stdout + out.stderr
    assert float(out.stdout.split("UNTOUCHED ")[1].split()[0]) <= 1e-4          # (and the model did run: its output is the fixture's)
