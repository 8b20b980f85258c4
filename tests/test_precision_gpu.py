"""-m gpu: the matmul-precision modes of the fused eval stages (`matmul_precision` = "highest" | "high" | "medium").

Reference: tests/precision_emulation.py — the three product sets of the exact bf16 split evaluated in float64, exact at GEMM level, and
the float64 oracles with their weight GEMMs replaced by it at model level.  Every tolerance below is derived there or is
parity_util.close_conditioned's factor 4; none comes from what the kernels give.
"""
import copy

import pytest
import torch

import parity_util as PU
import precision_emulation as PE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REDUCED = ("high", "medium")


# ------------------------------------------------------------------------------------------------ 1. GEMM level
@pytest.mark.parametrize("K", [48, 64, 80, 96, 112, 128])          # every dispatch_mlp<PREC> tile count: 3 .. 8
def test_a_mode_computes_exactly_its_product_set(K):
    """One Linear + bias, [4096, K] x [K, K], through ops.mlp_chain (sn_mlp_chain_prec_f32, one layer).  With
    d = ((y_gpu - b) - emu_mm(mode)) / mag elementwise:  (i) |d| <= K * 2^-23 — twice the worst case of a round-to-nearest fp32
    accumulation of K exact products (the matrix pipe's rounding inside a K = 32 block is not documented); nothing else differs between
    kernel and emulation — hence |y_gpu - b - y_f64| <= (C_MODE + K * 2^-23) * mag;  (ii) rms(d) <= rms(emu(mode) - emu(neighbour)) / 16:
    fails when a mode runs another mode's products (a float32 matmul of the same planes on the CPU gives rms(d) ~ 1e-8 against mode gaps
    of 4e-6 and 1e-3: a factor ~300 to the nearer one)."""
    from signnet_basisnet_amd import ops
    g = torch.Generator().manual_seed(K)
    x = torch.randn(4096, K, generator=g)
    w = torch.randn(K, K, generator=g) / K ** 0.5
    b = torch.randn(K, generator=g)
    y64 = x.double() @ w.double().t()
    mag = x.double().abs() @ w.double().abs().t()
    emu = {m: PE.emu_mm(x, w, m) for m in PE.MODES}
    wp = ops.pack_split(w.to(DEV), b.to(DEV))
    xd = x.to(DEV)

    def rms(t):
        return t.pow(2).mean().sqrt().item()

    for i, mode in enumerate(PE.MODES):
        y = ops.mlp_chain(xd, [wp], K, K, precision=mode).cpu().double()
        acc = y - b.double()
        d = (acc - emu[mode]) / mag
        gaps = [rms((emu[mode] - emu[PE.MODES[j]]) / mag) for j in (i - 1, i + 1) if 0 <= j < len(PE.MODES)]
        print(f"K={K} {mode}: max|d| {d.abs().max().item():.3e} (bound {K * 2.0 ** -23:.3e}), rms(d) {rms(d):.3e}, "
              f"mode gaps rms {', '.join(f'{v:.3e}' for v in gaps)}, max|y - f64|/mag {((acc - y64).abs() / mag).max().item():.3e}")
        assert bool((d.abs() <= K * 2.0 ** -23).all()), f"{mode}: kernel and emulation differ by more than an fp32 accumulation"
        assert bool(((acc - y64).abs() <= (PE.C_MODE[mode] + K * 2.0 ** -23) * mag).all()), f"{mode}: derived bound against float64"
        for gap in gaps:
            assert rms(d) <= gap / 16, f"{mode}: the kernel is not closer to its own product set than to a neighbouring mode's"
    assert torch.equal(ops.mlp_chain(xd, [wp], K, K), ops.mlp_chain(xd, [wp], K, K, precision="highest"))
    with pytest.raises(ValueError):
        ops.mlp_chain(xd, [wp], K, K, precision="bf16")


def test_unknown_precision_is_an_error_of_the_library():
    """The C entry point refuses a value outside SN_PREC_*: the usual error code with a message."""
    import ctypes as C
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd._lib import lib, ptr, stream
    x = torch.randn(64, 64, device=DEV)
    wp = ops.pack_split(torch.randn(64, 64, device=DEV))
    y = torch.empty(64, 64, device=DEV)
    ws = (C.c_void_p * 1)(ptr(wp))
    rc = lib().sn_mlp_chain_prec_f32(ptr(x), 64, 64, 64, None, 0, ws, 1, 64, ptr(y), 64, 64, 3, stream())
    assert rc < 0 and b"precision" in lib().sn_last_error()


# ------------------------------------------------------------------------------------------------ model cases
CASES = {
    "gine128_k16": dict(variant="gine", ctor=(None, None, 128, 1, 4, 6), max_k=16, batch=dict(num_graphs=32, seed=5)),
    "gine64_all": dict(variant="gine", ctor=(None, None, 64, 1, 4, 6), max_k=None, batch=dict(num_graphs=24, seed=5)),
    "alchemy108": dict(variant="alchemy", ctor=(6, 4, 108, 12, 8, 16), max_k=None,
                       batch=dict(num_graphs=32, seed=5, n_lo=6, n_hi=14, features="alchemy")),
}


def _case(name):
    from oracle import pyg_signnet as O
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.pyg import SignNetGNN
    c = CASES[name]
    torch.manual_seed(0)
    model = SignNetGNN(*c["ctor"], variant=c["variant"], max_k=c["max_k"])
    PU.bn_randomize(model, 1)
    data = synth.make_batch(**c["batch"])
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model, data, sd, O.make_cfg(c["variant"], *c["ctor"]), c["max_k"]


@pytest.mark.parametrize("name", list(CASES))
def test_default_is_untouched(name):
    """`highest` is the forward of a model on which the property was never set, bit for bit; and again after high -> highest."""
    from signnet_basisnet_amd import synth
    model, data, _, _, _ = _case(name)
    other = copy.deepcopy(model)
    model, other = model.to(DEV).eval(), other.to(DEV).eval()
    dd = synth.batch_to(data, DEV)
    with torch.no_grad():
        y0 = model(dd).clone()
        other.matmul_precision = "highest"
        assert torch.equal(other(dd), y0)
        other.matmul_precision = "high"
        prep = other._prep
        y_high = other(dd).clone()
        assert other._prep is prep, "nothing is repacked when the mode changes"
        assert not torch.equal(y_high, y0)
        other.matmul_precision = "highest"
        assert torch.equal(other(dd), y0)
    other.check_last()
    model.check_last()


@pytest.mark.parametrize("name", list(CASES))
def test_model_accuracy_follows_the_emulation(name, monkeypatch):
    """phi_fused, rho_sum_fused and y in the two reduced modes: e = max|. - f64| / max|f64| of the GPU and of the emulated oracle
    satisfy e_gpu <= 4 e_emu + 1e-6 and e_gpu >= e_emu / 4 (the lower bound shows that the cheaper product set really runs; where
    e_emu is below 30 x the fp32 oracle's own distance from float64 it cannot be told from fp32 noise, and `differs from highest`
    stands in for it).  `highest` passes parity_util.close as ever."""
    from oracle import pyg_signnet as O
    from signnet_basisnet_amd import synth
    model, data, sd, cfg, max_k = _case(name)
    o32, o64 = {}, {}
    with torch.no_grad():
        y32 = O.signnet_gnn(sd, cfg, data, training=False, max_k=max_k, out=o32)
        y64 = O.signnet_gnn(PU.to_f64(sd), cfg, PU.data_f64(data), training=False, max_k=max_k, out=o64)
    ref32 = dict(phi=o32["phi"], rho_sum=o32["rho_sum"], y=y32)
    ref64 = dict(phi=o64["phi"], rho_sum=o64["rho_sum"], y=y64)
    model = model.to(DEV).eval()
    dd = synth.batch_to(data, DEV)

    def gpu(mode):
        model.matmul_precision = mode
        with torch.no_grad():
            y = model(dd).clone()
            model.check_last()
            _, st = model(dd, return_stages=True)
        return dict(phi=st["phi_fused"].cpu(), rho_sum=st["rho_sum_fused"].cpu(), y=y.cpu())

    top = gpu("highest")
    for k in ("phi", "rho_sum", "y"):
        PU.close(top[k], ref32[k], f"{name} highest {k}", ref64=ref64[k])
    for mode in REDUCED:
        ye, oe = PE.emulated_oracle(mode, monkeypatch, sd, cfg, data, max_k)
        emu = dict(phi=oe["phi"], rho_sum=oe["rho_sum"], y=ye)
        got = gpu(mode)
        for k in ("phi", "rho_sum", "y"):
            e_gpu, e_emu, e_32 = PE.relmax(got[k], ref64[k]), PE.relmax(emu[k], ref64[k]), PE.relmax(ref32[k], ref64[k])
            print(f"{name} {mode} {k}: e_gpu {e_gpu:.3e}  e_emu {e_emu:.3e}  fp32 oracle {e_32:.3e}")
            assert e_gpu <= 4 * e_emu + 1e-6, f"{name} {mode} {k}: e_gpu {e_gpu:.3e} > 4 x e_emu {e_emu:.3e} + 1e-6"
            if e_emu >= 30 * e_32:
                assert e_gpu >= e_emu / 4, f"{name} {mode} {k}: e_gpu {e_gpu:.3e} < e_emu {e_emu:.3e} / 4: is the cheaper product set running?"
            else:
                assert not torch.equal(got[k], top[k]), f"{name} {mode} {k}: same bits as highest"
    model.matmul_precision = "highest"


@pytest.mark.parametrize("mode", PE.MODES)
def test_sign_invariance_is_bit_exact_in_every_mode(mode):
    """Truncation is symmetric in the sign: flipping a random subset of eigenvector columns leaves phi(x) + phi(-x) and y unchanged."""
    from signnet_basisnet_amd import synth
    model, data, _, _, _ = _case("gine128_k16")
    g = torch.Generator().manual_seed(9)
    flipped = copy.copy(data)
    ev, off = data.eigen_vectors.clone(), 0
    for n in data.sizes:
        s = (torch.rand(n, generator=g) < 0.5).float().mul(2).sub(1)
        ev[off:off + n * n] = (ev[off:off + n * n].view(n, n) * s[None, :]).reshape(-1)
        off += n * n
    flipped.eigen_vectors = ev
    assert not torch.equal(ev, data.eigen_vectors)
    model = model.to(DEV).eval()
    model.matmul_precision = mode
    with torch.no_grad():
        a, b = synth.batch_to(data, DEV), synth.batch_to(flipped, DEV)
        ya, yb = model(a).clone(), model(b).clone()
        _, sa = model(a, return_stages=True)
        _, sb = model(b, return_stages=True)
    assert torch.equal(sa["phi_fused"], sb["phi_fused"]) and torch.equal(ya, yb)


def test_training_is_untouched():
    """The differentiable train-mode path runs its own kernels at full precision: loss and every parameter gradient of a step with
    matmul_precision = "medium" are the bits of the same step with "highest"."""
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    model = SignNetGNN(None, None, 64, 1, 3, 3, variant="gine", max_k=8).to(DEV)
    dd = synth.batch_to(synth.make_batch(8, seed=21), DEV)
    target = torch.randn(8, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    start = copy.deepcopy(model.state_dict())

    def step(mode):
        model.load_state_dict(start)
        model.train()
        model.matmul_precision = mode
        model.zero_grad(set_to_none=True)
        torch.cuda.manual_seed(1234)             # the attention dropout draws from the device generator
        loss = (model(dd) - target).abs().mean()
        loss.backward()
        return loss.detach().clone(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}

    l0, g0 = step("highest")
    l1, g1 = step("medium")
    assert torch.equal(l0, l1)
    assert any(v is not None for v in g0.values())
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None) and (g0[k] is None or torch.equal(g0[k], g1[k])), k


def test_mixed_batch_serves_the_oversize_graph_at_highest():
    """Strict mode, sizes [10, 70, 12] at `high`: the 70-node graph goes layer by layer (highest: the bits of the `highest` run), the
    graphs around it through the stage kernels at `high` (the bits of their one-graph forwards at `high`)."""
    from signnet_basisnet_amd import dist as D
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(2)
    model = SignNetGNN(None, None, 64, 1, 2, 2, variant="gine", max_k=8).to(DEV).eval()
    assert model.strict
    dd = synth.batch_to(synth.make_batch(3, seed=4, sizes=[10, 70, 12]), DEV)
    with torch.no_grad():
        y_top = model(dd).clone()
        model.matmul_precision = "high"
        y = model(dd).clone()
        y_first, y_last = model(D.slice_graphs(dd, 0, 1)).clone(), model(D.slice_graphs(dd, 2, 3)).clone()
    assert torch.isfinite(y).all()
    assert torch.equal(y[1:2], y_top[1:2])
    assert torch.equal(y[0:1], y_first) and torch.equal(y[2:3], y_last)
    assert not torch.equal(y[0:1], y_top[0:1]) and not torch.equal(y[2:3], y_top[2:3])


# ------------------------------------------------------------------------------------------------ DGL DeepSigns
@pytest.mark.parametrize("kind,k,hidden,c", [("gin", 8, 95, 4), ("gin", 16, 64, 4), ("masked_gin", 37, 67, 67)])
def test_deepsigns_modes(kind, k, hidden, c, monkeypatch):
    """The three shipped DeepSigns shapes: default bits unchanged; the reduced modes follow the emulated float64 oracle within the
    factor 4 in both directions.  (The kernels truncate the BatchNorm-folded weights, the emulation the unfolded ones: covered by the
    factor.)  No residual or LayerNorm damps the error over the 8 layers: `medium` on the masked k = 37 net is a 5 % answer."""
    from oracle import dgl_deepsigns as OD
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import synth
    torch.manual_seed(0)
    net = DS.get_sign_inv_net(dict(sign_inv_net=kind, hidden_dim=hidden, phi_out_dim=c, sign_inv_layers=8, pos_enc_dim=k,
                                   dropout=0.0, sign_inv_activation="relu", device=DEV))
    PU.bn_randomize(net, 3)
    data = synth.make_batch(12, seed=41)
    x = synth.dgl_pos_enc(data, k).unsqueeze(-1)
    sd = {kk: v.detach().clone() for kk, v in net.state_dict().items()}
    ei, sizes = data.edge_index, torch.tensor(data.sizes)
    with torch.no_grad():
        if kind == "gin":
            r32 = OD.gin_deepsigns(sd, ei[0], ei[1], x, 8, k)
            r64 = OD.gin_deepsigns(PU.to_f64(sd), ei[0], ei[1], x.double(), 8, k)
        else:
            r32 = OD.masked_gin_deepsigns(sd, ei[0], ei[1], sizes, x, 8, k)
            r64 = OD.masked_gin_deepsigns(PU.to_f64(sd), ei[0], ei[1], sizes, x.double(), 8, k)
    other = copy.deepcopy(net).to(DEV).eval()
    net = net.to(DEV).eval()
    g = DS.Graph(ei[0].to(DEV), ei[1].to(DEV), sizes)
    xd = x.to(DEV)
    with torch.no_grad():
        y0 = other(g, xd).clone()
        net.matmul_precision = "highest"
        y_top = net(g, xd).clone()
        assert torch.equal(y_top, y0)
        PU.close(y_top, r32, f"{kind} highest", ref64=r64)
        e_32 = PE.relmax(r32, r64)
        for mode in REDUCED:
            net.matmul_precision = mode
            y = net(g, xd).clone()
            emu = PE.emulated_dgl_oracle(mode, monkeypatch, kind, sd, ei[0], ei[1], sizes, x, 8, k)
            e_gpu, e_emu = PE.relmax(y, r64), PE.relmax(emu, r64)
            print(f"{kind} k={k} hidden={hidden} {mode}: e_gpu {e_gpu:.3e}  e_emu {e_emu:.3e}  fp32 oracle {e_32:.3e}")
            assert e_gpu <= 4 * e_emu + 1e-6, f"{mode}: e_gpu {e_gpu:.3e} > 4 x e_emu {e_emu:.3e} + 1e-6"
            if e_emu >= 30 * e_32:
                assert e_gpu >= e_emu / 4, f"{mode}: e_gpu {e_gpu:.3e} < e_emu {e_emu:.3e} / 4: is the cheaper product set running?"
            else:
                assert not torch.equal(y, y_top)
        net.matmul_precision = "highest"
        assert torch.equal(net(g, xd), y0)


# ------------------------------------------------------------------------------------------------ refusal, not substitution
def test_a_width_without_reduced_kernels_refuses_them():
    """Hidden 32 (two 16-channel tiles) has no reduced instantiation: the property raises, the library refuses the launch with its
    usual error, and the forward at `highest` still works."""
    from signnet_basisnet_amd import ops, synth
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    model = SignNetGNN(None, None, 32, 1, 2, 2, variant="gine", max_k=8).to(DEV).eval()
    for name in REDUCED:
        with pytest.raises(ValueError, match="16-channel tiles"):
            model.matmul_precision = name
    assert model.matmul_precision == "highest"
    dd = synth.batch_to(synth.make_batch(6, seed=3), DEV)
    with torch.no_grad():
        y = model(dd)
        model.check_last()
        assert torch.isfinite(y).all()
        # the stage launch itself, asked for `high` behind the property's back: refused, nothing substituted
        P = model._prep["phi_fused"]
        plan = ops.build_plan(dd.batch, dd.edge_index, dd.num_graphs, 8, bins=True)
        with pytest.raises(RuntimeError, match="matmul precision"):
            P.run(plan, dd.eigen_vectors, 8, precision=1)
