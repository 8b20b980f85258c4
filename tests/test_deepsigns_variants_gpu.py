"""-m gpu: the 'gcn' and 'transformer' sign-invariant nets of the DGL tree (signnet_basisnet_amd.dgl_deepsigns.GCNDeepSigns /
TransformerDeepSigns) and their two kernels.  sn_gcn_propagate_f32 and its adjoint against a dense float64 operator on directed
graphs with multi-edges, self loops and empty rows, every vector / scalar layout; sn_graph_attention_f32 and its backward against
float64 on one batch with every size class of a set; the modules on the reference's fixtures (eval, train value, BatchNorm buffers,
every parameter gradient, sign invariance, launch counts); and behind the base networks: eager and captured training, recorded
serving, the zero-in-degree check."""
import functools
import types

import pytest
import torch

import deepsigns_variant_cases as C
import golden_util as G
import parity_util as PU
from parity_util import attributed, close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _randn(shape, seed, dtype=torch.float32):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


def _layout(t, layout):
    """The same values on the device as a contiguous matrix, as rows of a matrix four floats wider, or as a view one float into a buffer."""
    R, Cc = t.shape
    if layout in ("contiguous", "packed"):
        return t.to(DEV).contiguous()
    if layout == "strided":
        buf = torch.zeros(R, Cc + 4, device=DEV)
        buf[:, :Cc] = t.to(DEV)
        return buf[:, :Cc]
    buf = torch.zeros(R * Cc + 1, device=DEV)
    buf[1:] = t.to(DEV).reshape(-1)
    v = buf[1:].view(R, Cc)
    assert v.data_ptr() % 16 == 4
    return v


# ----------------------------------------------------------------------------- sn_gcn_propagate_f32
@functools.lru_cache(maxsize=None)
def _prop_plans(gname):
    from signnet_basisnet_amd import ops
    N, src, dst = C.prop_graph(gname)
    batch = torch.zeros(N, dtype=torch.long, device=DEV)
    ei = torch.stack([src, dst]).to(DEV)
    plan, rplan = ops.build_plan(batch, ei, 1, 0), ops.build_plan(batch, ei.flip(0).contiguous(), 1, 0)
    plan.check()
    return N, src, dst, plan, rplan, C.gcn_dense_operator(src, dst, N)


@pytest.mark.parametrize("Cc", C.PROP_WIDTHS)
@pytest.mark.parametrize("gname", C.PROP_GRAPHS)
def test_gcn_propagate_and_its_adjoint_against_the_dense_operator(gname, Cc):
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import ops
    N, src, dst, plan, rplan, A = _prop_plans(gname)
    width = 4 if Cc % 4 == 0 else Cc
    x, g, b = _randn((N, Cc), 1), _randn((N, Cc), 2), _randn((width,), 3)
    bt = b.repeat(Cc // width)
    y64, y64b = A @ x.double(), A @ x.double() + bt.double()
    dx64 = A.t() @ g.double()
    x32 = x.clone().requires_grad_(True)
    y32 = C.gcn_propagate_ref(x32, src, dst)
    (y32 * g).sum().backward()
    for layout in C.PROP_LAYOUTS:
        xd, gd = _layout(x, layout), _layout(g, layout)
        y = ops.gcn_propagate(xd, plan, rplan)
        yb = ops.gcn_propagate(xd, plan, rplan, b.to(DEV), width)
        dx = ops.gcn_propagate(gd, rplan, plan)
        e = attributed(y, y32.detach(), y64, f"{gname} C={Cc} {layout}: propagate")
        attributed(yb, y32.detach() + bt, y64b, f"{gname} C={Cc} {layout}: propagate + bias")
        e2 = attributed(dx, x32.grad, dx64, f"{gname} C={Cc} {layout}: adjoint")
        print(f"{gname} C={Cc} {layout}: |hip - f64| {e[0]:.1e} (cpu32 {e[1]:.1e})  adjoint {e2[0]:.1e} (cpu32 {e2[1]:.1e})")
        assert torch.equal(y, ops.gcn_propagate(xd, plan, rplan)) and torch.equal(dx, ops.gcn_propagate(gd, rplan, plan))
        zero_in = torch.bincount(dst, minlength=N) == 0
        assert torch.equal(yb.cpu()[zero_in], bt.expand(int(zero_in.sum()), Cc)), "a row without in-edges is the bias"
        assert not bool(y.cpu()[zero_in].any())
    # the autograd node: d x on the flipped plan, d bias the ordered column sums
    xa, ba = x.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    (AG.gcn_propagate(xa, plan, rplan, ba, width) * g.to(DEV)).sum().backward()
    attributed(xa.grad, x32.grad, dx64, f"{gname} C={Cc}: autograd d x")
    db64 = g.double().view(-1, width).sum(0)
    attributed(ba.grad, g.view(-1, width).sum(0), db64, f"{gname} C={Cc}: autograd d bias")


# ----------------------------------------------------------------------------- sn_graph_attention_f32
def _graph_ptr(sizes):
    return torch.tensor([0] + list(torch.tensor(sizes).cumsum(0)), dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dh", C.ATT_WIDTHS)
@pytest.mark.parametrize("S", C.ATT_SLOTS)
def test_graph_attention_and_its_backward_against_float64(S, dh):
    from signnet_basisnet_amd import ops
    sizes, H = C.ATT_SIZES, C.ATT_HEADS
    N, D = sum(sizes), C.ATT_HEADS * dh
    R = N * S
    qkv, go = _randn((R, 3 * D), 10 + dh), _randn((R, D), 11 + dh)
    gp = _graph_ptr(sizes)

    def ref(dtype):
        q, k, v = (qkv[:, i * D:(i + 1) * D].clone().to(dtype).requires_grad_(True) for i in range(3))
        out, lse = C.graph_attention_ref(q, k, v, sizes, S, H, want_lse=True)
        (out * go.to(dtype)).sum().backward()
        return out.detach(), lse.detach(), torch.cat([q.grad, k.grad, v.grad], dim=1)
    (o32, l32, g32), (o64, l64, g64) = ref(torch.float32), ref(torch.float64)
    for layout in C.ATT_LAYOUTS:
        t = _layout(qkv, layout)
        q, k, v = t[:, :D], t[:, D:2 * D], t[:, 2 * D:]
        out, lse = ops.graph_attention(q, k, v, gp, N, S, H)
        e = attributed(out, o32, o64, f"S={S} dh={dh} {layout}: out")
        attributed(lse, l32, l64, f"S={S} dh={dh} {layout}: lse")
        assert torch.equal(out[:S], v[:S]), "a one-node set returns its v row"
        gd = go.to(DEV)
        g = ops.graph_attention_bwd(q, k, v, out, lse, gd, gp, N, S, H)
        for i, n in enumerate(("dq", "dk", "dv")):
            eg = attributed(g[:, i * D:(i + 1) * D], g32[:, i * D:(i + 1) * D], g64[:, i * D:(i + 1) * D], f"S={S} dh={dh} {layout}: {n}")
            print(f"S={S} dh={dh} {layout} {n}: |hip - f64| {eg[0]:.1e} (cpu32 {eg[1]:.1e})")
        print(f"S={S} dh={dh} {layout} out: |hip - f64| {e[0]:.1e} (cpu32 {e[1]:.1e})")
        assert torch.equal(out, ops.graph_attention(q, k, v, gp, N, S, H)[0])
        assert torch.equal(g, ops.graph_attention_bwd(q, k, v, out, lse, gd, gp, N, S, H))


def test_graph_attention_refuses_wide_heads_before_any_launch():
    from signnet_basisnet_amd import ops
    sizes, S, H, dh = [3, 2], 1, 2, 65
    t = _randn((5, 3 * H * dh), 1).to(DEV)
    D = H * dh
    rec = ops.KernelTimer()
    with rec, pytest.raises(RuntimeError, match=r"code -3.*head width 65"):
        ops.graph_attention(t[:, :D], t[:, D:2 * D], t[:, 2 * D:], _graph_ptr(sizes), 5, S, H)
    out, lse = torch.zeros(5, D, device=DEV), torch.zeros(5, H, device=DEV)
    with pytest.raises(RuntimeError, match=r"code -3.*head width 65"):
        ops.graph_attention_bwd(t[:, :D], t[:, D:2 * D], t[:, 2 * D:], out, lse, out, _graph_ptr(sizes), 5, S, H)
    torch.cuda.synchronize()          # (nothing was queued: nothing can fault)


# ----------------------------------------------------------------------------- the modules on the reference's fixtures
@functools.lru_cache(maxsize=None)
def _refs(name):
    fx = G.load(name)
    y64_eval = C.module_ref(fx, torch.float64)
    y64_train, g64 = C.module_ref(fx, torch.float64, training=True, grads=True)
    return fx, y64_eval, y64_train, g64


def _graph(fx):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    ei = fx.inp["edge_index"]
    return DS.Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"])


def _check_buffers(model, fx, what):
    sd = model.state_dict()
    n = 0
    for key, ref in fx.out.items():
        if not key.startswith("train/buffers/"):
            continue
        k = key[len("train/buffers/"):]
        n += 1
        if k.endswith("num_batches_tracked"):
            assert int(sd[k]) == int(ref), f"{what}: {k}"
        else:
            close(sd[k], ref, f"{what}: {k}")
    assert n


def _spans(fn):
    from signnet_basisnet_amd import ops
    fn()
    rec = ops.KernelTimer()
    with rec:
        y = fn()
    return y, [n for n, _, _ in rec.spans]


@pytest.mark.parametrize("name", C.GCN_CASES + C.TF_CASES)
def test_modules_on_the_reference_fixtures(name):
    fx, y64_eval, y64_train, g64 = _refs(name)
    p = C.params(fx)
    g, x = _graph(fx), fx.inp["pos_enc"].unsqueeze(-1).to(DEV)
    model = C.build(fx, DEV).eval()
    with torch.no_grad():
        y = model(g, x)
    print(f"{name} eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, y64_eval):.2e}")
    close(y, fx.out["eval/y"], f"{name}: eval y", ref64=y64_eval)
    # sign invariance, bit for bit: a flipped eigenvector column swaps two rows of the merged sign axis, nothing else
    flips = torch.tensor([1.0, -1.0] * p.k)[:p.k].view(1, p.k, 1).to(DEV)
    with torch.no_grad():
        assert torch.equal(model(g, x * flips), y) and torch.equal(model(g, -x), y)
    # launches: one propagation / attention launch per encoder layer, whatever k
    kernel = "sn_gcn_propagate_f32" if p.cls == "GCNDeepSigns" else "sn_graph_attention_f32"

    def run():
        with torch.no_grad():
            return model(g, x)
    _, names = _spans(run)
    assert names.count(kernel) == p.layers, names
    # train mode without autograd: batch statistics, running statistics moved as the reference moves them
    model.train()
    with torch.no_grad():
        yt = model(g, x)
    ref_err = PU.relerr(fx.out["train/y"], y64_train)
    print(f"{name} train y: |hip - ref| {PU.relerr(yt, fx.out['train/y']):.2e}  |hip - f64| {PU.relerr(yt, y64_train):.2e}  "
          f"|ref - f64| {ref_err:.2e}")
    if ref_err > PU.REL:          # the reference's own fp32 output is farther than 1e-5 from float64: the case's conditioning sets the bar
        PU.close_conditioned(yt, fx.out["train/y"], y64_train, f"{name}: train y")
    else:
        close(yt, fx.out["train/y"], f"{name}: train y", ref64=y64_train)
    _check_buffers(model, fx, f"{name} (train, no autograd)")
    # train mode under autograd: the same forward, every parameter gradient against the reference's and float64
    model = C.build(fx, DEV).train()
    yg = model(g, x)
    if ref_err > PU.REL:
        PU.close_conditioned(yg, fx.out["train/y"], y64_train, f"{name}: train y (autograd)")
    else:
        close(yg, fx.out["train/y"], f"{name}: train y (autograd)", ref64=y64_train)
    (yg * fx.inp["cotangent"].to(DEV)).sum().backward()
    _check_buffers(model, fx, f"{name} (train, autograd)")
    got = {k: q.grad for k, q in model.named_parameters()}
    assert set(got) == set(g64) and all(v is not None for v in got.values())
    for k in sorted(got):
        print(f"{name} d {k}: |hip - f64| {PU.relerr(got[k], g64[k]):.2e}  |ref32 - f64| {PU.relerr(fx.out['grad/' + k], g64[k]):.2e}")
    for k in sorted(got):
        attributed(got[k], fx.out["grad/" + k], g64[k], f"{name}: d {k}")


# ----------------------------------------------------------------------------- behind the base networks
BASES = {"GINNet": "dgl_ginnet_k6", "GatedGCNNet": "dgl_gatedgcn_concat_k6"}


def _base_net(cls, kind, seed=3, lr=1e-4):
    from signnet_basisnet_amd import dgl_nets, optim
    fx = G.load(BASES[cls])
    hidden, L, k = (int(v) for v in fx.meta["params"])
    params = dict(num_atom_type=28, num_bond_type=4, hidden_dim=hidden, out_dim=hidden, in_feat_dropout=0.0, dropout=0.0, L=L,
                  readout="mean", batch_norm=True, residual=True, edge_feat=True, device=DEV, pe_init="lap_pe", lap_method="sign_inv",
                  lap_lspe=False, use_lapeig_loss=False, lambda_loss=1, alpha_loss=1e-4, pos_enc_dim=k, sign_inv_net=kind,
                  sign_inv_layers=3, sign_inv_activation="relu", phi_out_dim=4,
                  pe_aggregate=str(fx.meta["pe_aggregate"]) if "pe_aggregate" in fx.meta else "add")
    torch.manual_seed(seed)
    net = getattr(dgl_nets, cls)(params)
    with torch.no_grad():                               # GraphConv's bias is zero-initialised: make it count
        for n_, p_ in net.sign_inv_net.named_parameters():
            if kind == "gcn" and n_.startswith("enc.layers.") and n_.endswith(".bias"):
                p_.copy_(0.1 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(5)))
    net = net.to(DEV)
    return net, optim.FlatAdam(net.parameters(), lr=lr), k


def _batch(k, sizes, seed):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import synth
    data = synth.make_batch(len(sizes), seed=seed, sizes=sizes)
    src, dst = data.edge_index
    return types.SimpleNamespace(
        g=DS.Graph(src.to(DEV), dst.to(DEV), data.sizes), h=data.x.squeeze(-1).to(DEV), p=synth.dgl_pos_enc(data, k).to(DEV),
        e=data.edge_attr.to(DEV), sn=None, t=torch.randn(len(sizes), 1, generator=torch.Generator().manual_seed(seed + 100)).to(DEV),
        N=data.batch.numel(), E=data.edge_index.shape[1], B=len(sizes), data=data)


SHAPES = ([5, 9, 12, 7, 3], [8, 4, 11, 6, 10, 2, 7])          # two batches of different node, edge and graph counts


@pytest.mark.parametrize("kind", ["gcn", "transformer"])
@pytest.mark.parametrize("cls", list(BASES))
def test_eval_eager_step_and_recorded_serving(cls, kind):
    from signnet_basisnet_amd import serving
    net, opt, k = _base_net(cls, kind)
    b = _batch(k, SHAPES[0], seed=5)
    net.eval()
    with torch.no_grad():
        p = net.sign_inv_net(b.g, b.p.unsqueeze(-1)).squeeze(-1)
        y, _ = net(b.g, b.h, p, b.e, None)
    assert p.shape == (b.N, k) and y.shape == (b.B, 1) and torch.isfinite(y).all() and torch.isfinite(p).all()
    pe = b.p.unsqueeze(-1)
    fwd = serving.GraphedDGLForward(net, b.g, b.h, pe, b.e)
    for _ in range(2):
        assert torch.equal(fwd(b.g, b.h, pe, b.e), y), "the recorded forward replays the eager eval output"
    fwd.check()
    del fwd
    # one eager training step moves every parameter of the sign-invariant net
    net.train()
    before = {n: q.detach().clone() for n, q in net.sign_inv_net.named_parameters()}
    opt.zero_grad()
    p = net.sign_inv_net(b.g, b.p.unsqueeze(-1)).squeeze(-1)
    loss = net.loss(net(b.g, b.h, p, b.e, None)[0], b.t)
    loss.backward()
    assert all(q.grad is not None for q in net.sign_inv_net.parameters())
    opt.step()
    same = [n for n, q in net.sign_inv_net.named_parameters() if torch.equal(q.detach(), before[n])]
    assert not same, same


@pytest.mark.parametrize("kind", ["gcn", "transformer"])
@pytest.mark.parametrize("cls", list(BASES))
def test_bucketed_step_follows_the_eager_steps(cls, kind):
    """Two differently shaped batches through ONE capacity bucket: losses, first-step gradients and Adam's parameters against the eager
    loop, at the bounds tests/test_dgl_bucketed_step_gpu.py holds the GIN sign-invariant net to (its helpers, unchanged)."""
    import test_dgl_bucketed_step_gpu as T
    lr = 1e-4
    k = _base_net(cls, kind)[2]
    batches = [_batch(k, s, seed=5 + i) for i, s in enumerate(SHAPES)]
    bucket = (max(b.N for b in batches) + 9, max(b.E for b in batches) + 14)
    m1, o1, _ = _base_net(cls, kind, lr=lr)
    eager, ge, _ = T._eager(m1.train(), o1, batches)
    mn, on, _ = _base_net(cls, kind, lr=lr)
    noisy, gn, _ = T._eager(mn.train(), on, T._perturbed(batches))
    m2, o2, _ = _base_net(cls, kind, lr=lr)
    s, padded, gp, _ = T._bucketed(m2.train(), o2, batches, bucket=bucket)
    assert s.captures == 1 and s.hits == 1
    s.check()
    print(f"{cls} {kind}: eager {eager}  noisy {noisy}  padded {padded}")
    T._close_losses(eager, noisy, padded)
    T._close_grads(ge[0], gn[0], gp[0])
    T._close_params(o1, on, o2, len(batches), lr)
    assert getattr(m2.sign_inv_net, "_bucket", None) is None, "the switch does not outlive the step"
    T._release(s)


@pytest.mark.parametrize("cls", list(BASES))
def test_gcn_zero_in_degree_raises_eagerly_and_through_check(cls):
    from signnet_basisnet_amd import serving
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    net, opt, k = _base_net(cls, "gcn")
    b = _batch(k, [5, 1, 9, 7], seed=8)          # the one-node graph has no edge
    net.eval()
    with torch.no_grad(), pytest.raises(ValueError, match="0-in-degree"):
        net.sign_inv_net(b.g, b.p.unsqueeze(-1))
    fwd = serving.GraphedDGLForward(net, b.g, b.h, b.p.unsqueeze(-1), b.e)
    fwd()                                        # (check() reads what the last REPLAY flagged on the device)
    with pytest.raises(ValueError, match="0-in-degree"):
        fwd.check()
    del fwd
    net.train()
    with pytest.raises(ValueError, match="0-in-degree"):
        net.sign_inv_net(b.g, b.p.unsqueeze(-1))
    s = DGLBucketedStep(net, opt, max_graphs=8)
    with pytest.raises(ValueError, match="0-in-degree"):          # the capture's own check() reads the deferred flag of its warm-up
        s.step(b.g, b.h, b.p, b.e, None, b.t)
    s.release()
    torch.cuda.synchronize()
