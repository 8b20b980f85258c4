"""-m gpu: the plain GNN for every model.gnn_type on the device.  The three launches of csrc/simplified_pna.hip and the GCNConv propagation
of csrc/pyg_gcn.hip against the float64 restatements of tests/gnn_type_cases.py; the four modules on the reference's own fixtures
(tests/golden/gnn_types_*.npz) in eval mode, train mode without autograd and train mode under autograd; the launch structure of a
SimplifiedPNAConv layer; the errors; and nothing shared disturbed.  Rules of tests/parity_util.py only: close(ref64=) at REL for forward
values, attributed() for gradients, close_conditioned() where a BatchNorm runs over a handful of rows.  Every figure is printed before it
is asserted."""
import functools

import pytest
import torch

import gnn_type_cases as C
import golden_util as G
import parity_util as PU
from parity_util import attributed, close, close_conditioned

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FEW_ROWS = ("n1_e2", "n3_e2")          # the cases whose BatchNorm sees two rows


def plans(ei, batch, B):
    from signnet_basisnet_amd import ops
    ei, batch = ei.to(DEV), batch.to(DEV)
    return ops.build_plan(batch, ei, B, 0), ops.build_plan(batch, ei.flip(0).contiguous(), B, 0)


def laid_out(shape, ld, offset, fill=None):
    """(buffer, view): a [R, C] device block with row stride ld that starts 16 bytes (offset: 20 bytes) into a NaN-poisoned buffer with 16
    more bytes behind it; `fill` is copied in."""
    R, Cc = shape
    buf = torch.full((R * ld + 9,), float("nan"), dtype=torch.float32, device=DEV)
    start = 5 if offset else 4
    v = buf.as_strided((R, Cc), (ld, 1), start)
    assert v.data_ptr() % 16 == (4 if offset else 0)
    if fill is not None:
        v.copy_(fill)
    return buf, v


def guards_intact(buf, v, what):
    """Every element of the view was written, and nothing else of its buffer was."""
    assert not bool(torch.isnan(v).any()), f"{what}: unwritten output elements"
    mask = torch.ones_like(buf, dtype=torch.bool)
    R, Cc = v.shape
    start = (v.data_ptr() - buf.data_ptr()) // 4
    if R and Cc:
        idx = (start + torch.arange(R, device=DEV)[:, None] * v.stride(0) + torch.arange(Cc, device=DEV)[None, :]).reshape(-1)
        mask[idx] = False
    assert bool(torch.isnan(buf[mask]).all()), f"{what}: a write outside the output block"


@functools.lru_cache(maxsize=None)
def kernel_refs(name):
    """Inputs and the float32 / float64 references of one kernel case: computed once, shared, never modified."""
    x = C.kernel_inputs(name)
    out = {"x": x}
    for dtype in (torch.float32, torch.float64):
        t = lambda v: v.to(dtype)          # noqa: E731
        ops_ = (t(x.A), t(x.B_), t(x.Q), x.ei)
        r = types_ns()
        # eval: the folded running statistics, computed once in float64 and handed to both sides as float32
        scale = (x.gamma.double() / (x.running_var.double() + C.BN_EPS).sqrt()).float()
        shift = (x.beta.double() - x.running_mean.double() * scale.double()).float()
        r.scale, r.shift = scale, shift
        r.eval_r, r.eval_g = C.spna_eval_ref(*ops_, t(scale), t(shift), t(x.dr))
        if "train" in x.modes:
            r.st = C.spna_stats_ref(*ops_, t(x.gamma), t(x.beta), t(x.running_mean), t(x.running_var))
            r.train_r, r.train_g = C.spna_train_ref(*ops_, t(x.gamma), t(x.beta), t(x.dr))
        out[dtype] = r
    return out


def types_ns():
    import types
    return types.SimpleNamespace()


def run_kernels(x, mode, scale=None, shift=None):
    """One forward and one adjoint of the case on the device, every operand and output laid out as the case says."""
    from signnet_basisnet_amd import ops
    plan, rplan = plans(x.ei, x.batch, x.B)
    ins = [laid_out(t.shape, x.ld, x.offset, t)[1] for t in (x.A, x.B_, x.Q, x.dr)]
    a, b, q, dr = ins
    res = types_ns()
    rbuf, r = laid_out((x.N, x.C), x.ld, x.offset)
    outs = [laid_out(s, x.ld, x.offset) for s in ((x.N, x.C), (x.N, x.C), (x.E, x.C))]
    if mode == "train":
        bn = torch.nn.BatchNorm1d(x.C).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(x.gamma), bn.bias.copy_(x.beta), bn.running_mean.copy_(x.running_mean), bn.running_var.copy_(x.running_var)
        res.state, res.count = ops.spna_stats(a, b, q, plan, bn)
        res.bn = bn
        ops.spna_mean(a, b, q, plan, res.state[3], res.state[4], out=r)
        _, _, _, res.dgamma, res.dbeta = ops.spna_bwd(a, b, q, plan, rplan, dr, state=res.state, gamma=bn.weight.detach(),
                                                      out=tuple(v for _, v in outs))
    else:
        ops.spna_mean(a, b, q, plan, scale.to(DEV), shift.to(DEV), out=r)
        ops.spna_bwd(a, b, q, plan, rplan, dr, scale=scale.to(DEV), shift=shift.to(DEV), out=tuple(v for _, v in outs))
    torch.cuda.synchronize()
    guards_intact(rbuf, r, f"{x.name} {mode}: r")
    for (buf, v), k in zip(outs, ("dA", "dB", "dQ")):
        guards_intact(buf, v, f"{x.name} {mode}: {k}")
    res.r, (res.dA, res.dB, res.dQ) = r, (v for _, v in outs)
    assert plan.check()[0] == 0
    return res


# ----------------------------------------------------------------------------- 1. the kernels of csrc/simplified_pna.hip
@pytest.mark.parametrize("name", [n for n, c in C.KERNEL_CASES.items() if "eval" in c[4]])
def test_spna_eval_mean_and_adjoint_against_float64(name):
    refs = kernel_refs(name)
    x, r32, r64 = refs["x"], refs[torch.float32], refs[torch.float64]
    got = run_kernels(x, "eval", r32.scale, r32.shift)
    print(f"{name} eval r: |hip - f64| {PU.relerr(got.r, r64.eval_r):.2e}  |cpu32 - f64| {PU.relerr(r32.eval_r, r64.eval_r):.2e}")
    if x.E == 0:
        assert not bool(got.r.any()) and not bool(got.dA.any()) and not bool(got.dB.any())
        return
    close(got.r, r32.eval_r, f"{name}: r (eval)", ref64=r64.eval_r)
    deg = torch.bincount(x.ei[1], minlength=x.N)
    assert not bool(got.r[(deg == 0).to(DEV)].any())
    for k in ("dA", "dB", "dQ"):
        print(f"{name} eval {k}: |hip - f64| {PU.relerr(getattr(got, k), r64.eval_g[k]):.2e}  |cpu32 - f64| {PU.relerr(r32.eval_g[k], r64.eval_g[k]):.2e}")
    for k in ("dA", "dB", "dQ"):
        attributed(getattr(got, k), r32.eval_g[k], r64.eval_g[k], f"{name}: {k} (eval)")


@pytest.mark.parametrize("name", [n for n, c in C.KERNEL_CASES.items() if "train" in c[4]])
def test_spna_train_statistics_mean_and_adjoint_against_float64(name):
    refs = kernel_refs(name)
    x, r32, r64 = refs["x"], refs[torch.float32], refs[torch.float64]
    got = run_kernels(x, "train")
    chk = close_conditioned if name in FEW_ROWS else (lambda a, b32, b64, what: close(a, b32, what, ref64=b64))
    names = ("mean", "var", "rstd", "scale", "shift")
    for i, k in enumerate(names):
        print(f"{name} {k}: |hip - f64| {PU.relerr(got.state[i], getattr(r64.st, k)):.2e}  |cpu32 - f64| {PU.relerr(getattr(r32.st, k), getattr(r64.st, k)):.2e}")
    print(f"{name} train r: |hip - f64| {PU.relerr(got.r, r64.train_r):.2e}  |cpu32 - f64| {PU.relerr(r32.train_r, r64.train_r):.2e}")
    assert float(got.count) == x.E == r64.st.count
    for i, k in enumerate(names):
        chk(got.state[i], getattr(r32.st, k), getattr(r64.st, k), f"{name}: {k}")
    for k, t in (("running_mean", got.bn.running_mean), ("running_var", got.bn.running_var)):
        chk(t, getattr(r32.st, k), getattr(r64.st, k), f"{name}: {k}")
    assert int(got.bn.num_batches_tracked) == 1
    chk(got.r, r32.train_r, r64.train_r, f"{name}: r (train)")
    grads = dict(dA=got.dA, dB=got.dB, dQ=got.dQ, dgamma=got.dgamma, dbeta=got.dbeta)
    for k, g in grads.items():
        print(f"{name} train {k}: |hip - f64| {PU.relerr(g, r64.train_g[k]):.2e}  |cpu32 - f64| {PU.relerr(r32.train_g[k], r64.train_g[k]):.2e}")
    for k, g in grads.items():
        if name in FEW_ROWS:
            close_conditioned(g, r32.train_g[k], r64.train_g[k], f"{name}: {k} (train)")
        else:
            attributed(g, r32.train_g[k], r64.train_g[k], f"{name}: {k} (train)")


@pytest.mark.parametrize("name", ["c12_offset", "c48_ld64", "c384"])
def test_spna_launches_are_bit_reproducible(name):
    x = kernel_refs(name)["x"]
    a, b = run_kernels(x, "train"), run_kernels(x, "train")
    for k in ("state", "r", "dA", "dB", "dQ", "dgamma", "dbeta"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.bn.running_var, b.bn.running_var)
    r32 = kernel_refs(name)[torch.float32]
    a, b = run_kernels(x, "eval", r32.scale, r32.shift), run_kernels(x, "eval", r32.scale, r32.shift)
    for k in ("r", "dA", "dB", "dQ"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_spna_train_mode_refuses_a_single_edge_row():
    from signnet_basisnet_amd import ops
    x = C.kernel_inputs("n2_e1")
    plan, _ = plans(x.ei, x.batch, x.B)
    bn = torch.nn.BatchNorm1d(x.C).to(DEV).train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.spna_stats(x.A.to(DEV), x.B_.to(DEV), x.Q.to(DEV), plan, bn)
    assert int(bn.num_batches_tracked) == 0


# ----------------------------------------------------------------------------- 2. GCNConv's propagation in PyG's normalisation
@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("Cc", [12, 15])
def test_gcn_pyg_propagate_and_adjoint_against_the_dense_float64_operator(symmetric, Cc):
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import ops
    ei, batch, B = C.kernel_graph("degrees")          # directed, with input self loops and multi-edges
    if symmetric:
        ei = torch.cat([ei, ei.flip(0)], 1).contiguous()
    N = batch.numel()
    g = torch.Generator().manual_seed(Cc)
    x, cot = torch.randn(N, Cc, generator=g), torch.randn(N, Cc, generator=g)
    S64 = C.gcn_norm_dense(ei, N, torch.float64)
    assert symmetric == bool(torch.allclose(S64, S64.t(), rtol=1e-12, atol=1e-14))
    y64, dx64 = S64 @ x.double(), S64.t() @ cot.double()
    S32 = C.gcn_norm_dense(ei, N, torch.float32)
    y32, dx32 = S32 @ x, S32.t() @ cot
    plan, rplan = plans(ei, batch, B)
    dis = ops.gcn_pyg_coef(plan)
    xd = x.to(DEV).requires_grad_(True)
    y = AG.gcn_pyg_propagate(xd, plan, rplan, dis)
    y.backward(cot.to(DEV))
    print(f"gcn C={Cc} symmetric={symmetric}: y |hip - f64| {PU.relerr(y, y64):.2e} |cpu32 - f64| {PU.relerr(y32, y64):.2e}; "
          f"dx |hip - f64| {PU.relerr(xd.grad, dx64):.2e} |cpu32 - f64| {PU.relerr(dx32, dx64):.2e}")
    close(dis, S64.diagonal().sqrt().float(), "dis", ref64=S64.diagonal().sqrt())          # S_ii = dis_i^2: every node has exactly one unit loop
    close(y, y32, "D^-1/2 (A+I) D^-1/2 x", ref64=y64)
    attributed(xd.grad, dx32, dx64, "the adjoint")
    y2 = ops.gcn_pyg_propagate(x.to(DEV), plan, dis)
    assert torch.equal(y2, y.detach())


# ----------------------------------------------------------------------------- 3. the four modules on the reference's fixtures
def _meta(fx):
    nhid, nlayer = (int(v) for v in fx.meta["nhid_nlayer"])
    return str(fx.meta["gnn_type"]), nhid, nlayer, str(fx.meta["pooling"])


def _model(fx):
    from signnet_basisnet_amd.pyg_gnn_types import GNN
    kind, nhid, nlayer, pooling = _meta(fx)
    m = GNN(None, None, nhid, 1, nlayer, kind, 0, pooling, res=True)
    m.load_state_dict(G.full_state_dict(fx), strict=True)
    return m.to(DEV)


def _cotangent(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(5))


@functools.lru_cache(maxsize=None)
def module_refs(name):
    """(eval y, train-mode y, train-mode gradients of sum(y * cotangent)) of the restatement in float32 and float64."""
    fx = G.load(name)
    kind, _, nlayer, pooling = _meta(fx)
    pe = fx.inp.get("additional_x")
    outs = {}
    for dtype in (torch.float32, torch.float64):
        data = G.as_data(fx.inp)
        sd = C.leaf_state_dict(G.full_state_dict(fx), dtype)
        p = None if pe is None else pe.to(dtype)
        with torch.no_grad():
            y_eval = C.gnn_ref(sd, kind, nlayer, pooling, data, p, False)
        y = C.gnn_ref(sd, kind, nlayer, pooling, data, p, True)
        (y * _cotangent(y.shape).to(dtype)).sum().backward()
        outs[dtype] = (y_eval, y.detach(), {k: v.grad for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point() and v.grad is not None})
    return outs


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


@pytest.mark.parametrize("name", list(C.FIXTURES))
def test_modules_on_the_reference_fixtures(name):
    from signnet_basisnet_amd import synth
    fx = G.load(name)
    refs = module_refs(name)
    (_, _, g32), (y64_eval, y64_train, g64) = refs[torch.float32], refs[torch.float64]
    data = synth.batch_to(G.as_data(fx.inp), DEV)
    pe = fx.inp.get("additional_x")
    pe = None if pe is None else pe.to(DEV)
    model = _model(fx).eval()
    with torch.no_grad():
        y = model(data, pe)
    print(f"{name} eval y: |hip - ref| {PU.relerr(y, fx.out['eval/y']):.2e}  |hip - f64| {PU.relerr(y, y64_eval):.2e}  "
          f"|ref - f64| {PU.relerr(fx.out['eval/y'], y64_eval):.2e}")
    close(y, fx.out["eval/y"], f"{name}: eval y", ref64=y64_eval)
    # train mode without autograd: batch statistics, running statistics moved as the reference moves them
    model.train()
    with torch.no_grad():
        yt = model(data, pe)
    print(f"{name} train y: |hip - ref| {PU.relerr(yt, fx.out['train/y']):.2e}  |hip - f64| {PU.relerr(yt, y64_train):.2e}  "
          f"|ref - f64| {PU.relerr(fx.out['train/y'], y64_train):.2e}")
    close_conditioned(yt, fx.out["train/y"], y64_train, f"{name}: train y")          # (BatchNorm over the 5 pooled rows / the node rows)
    _check_buffers(model, fx, f"{name} (train, no autograd)")
    # train mode under autograd: the same forward, gradients against float64
    model = _model(fx).train()
    yg = model(data, pe)
    close_conditioned(yg, fx.out["train/y"], y64_train, f"{name}: train y (autograd)")
    (yg * _cotangent(yg.shape).to(DEV)).sum().backward()
    _check_buffers(model, fx, f"{name} (train, autograd)")
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    used = {k for k, g in g64.items() if bool(g.any()) and ".layer.nn." not in k and ".lin_dst." not in k}
    assert used <= set(got), sorted(used - set(got))
    # A bias directly in front of a batch-statistics BatchNorm (GINConv's nn.layers.1.bias) has the gradient 0: float64 returns its own
    # rounding noise (1e-17 of the other gradients), which is no scale to compare against.  Such a bias is compared together with its
    # Linear's weight gradient, as one tensor (weight | bias), so the Linear's gradient sets the scale.
    gmax = max(float(g.abs().max()) for g in g64.values())
    paired = {k for k in used if k.endswith(".bias") and float(g64[k].abs().max()) <= 1e-12 * gmax and k[:-4] + "weight" in used}
    for k in sorted(used):
        print(f"{name} d {k}: |hip - f64| {PU.relerr(got[k], g64[k]):.2e}  |cpu32 - f64| {PU.relerr(g32[k], g64[k]):.2e}"
              + ("  (zero to float64 rounding: compared with its weight)" if k in paired else ""))
    for k in sorted(used - paired):
        attributed(got[k], g32[k], g64[k], f"{name}: d {k}")
    for k in sorted(paired):
        w = k[:-4] + "weight"
        both = lambda g: torch.cat([g[w].detach().cpu().reshape(-1), g[k].detach().cpu().reshape(-1)])          # noqa: E731
        attributed(both(got), both(g32), both(g64), f"{name}: d ({w} | {k})")
    for k in set(got) - used:          # a parameter the forward does not use (or whose gradient is exactly 0) gets no gradient
        assert not bool(got[k].any()), k
    unused = [k for k, _ in model.named_parameters() if "edge_encoders" in k or ".norms.1." in k and "convs" in k]
    if _meta(fx)[0] != "SimplifiedPNAConv":
        assert all(k not in got or not bool(got[k].any()) for k in unused if "edge_encoders" in k)
    assert all(k not in got or not bool(got[k].any()) for k in unused if ".norms.1." in k)


@pytest.mark.parametrize("kind", ["GCNConv", "GATConv"])
def test_a_batch_of_more_than_20000_nodes(kind):
    """No 8 192-node limit: eval on one large batch against the float64 restatement."""
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.pyg_gnn_types import GNN
    data = C.odd_edges(synth.make_batch(900, seed=11, n_lo=20, n_hi=27))
    assert data.num_nodes > 20000
    torch.manual_seed(3)
    model = GNN(None, None, 16, 1, 2, kind, 0, "mean")
    PU.bn_randomize(model, 4)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        y32 = C.gnn_ref(sd, kind, 2, "mean", data, None, False)
        y64 = C.gnn_ref(PU.to_f64(sd), kind, 2, "mean", data, None, False)
        y = model.to(DEV).eval()(synth.batch_to(data, DEV))
    print(f"{kind}, {data.num_nodes} nodes: |hip - f64| {PU.relerr(y, y64):.2e}  |cpu32 - f64| {PU.relerr(y32, y64):.2e}")
    close(y, y32, f"{kind} on {data.num_nodes} nodes", ref64=y64)


# ----------------------------------------------------------------------------- 4. launch structure
def test_a_pna_layer_is_one_new_launch_in_eval_and_two_in_the_train_forward():
    from signnet_basisnet_amd import ops, synth
    fx = G.load("gnn_types_pna_h16_l2_add")
    nlayer = _meta(fx)[2]
    data = synth.batch_to(G.as_data(fx.inp), DEV)
    model = _model(fx)
    for train, new in ((False, ["sn_spna_mean_f32"]), (True, ["sn_spna_stats_f32", "sn_spna_mean_f32"])):
        model.train(train)
        rec = ops.KernelTimer()
        with rec, torch.no_grad():
            model(data)
        names = [s[0] for s in rec.spans]
        gemm = "sn_masked_linear_f32"
        starts = [i for i, n in enumerate(names) if n == new[0]]
        assert len(starts) == nlayer, names
        for i in starts:
            # ... A|B GEMM, edge embedding, Q GEMM | the new launches | W2 GEMM ...
            assert names[i - 3:i] == [gemm, "sn_embedding_sum_f32", gemm], names[i - 3:i + 3]
            assert names[i:i + len(new)] == new and names[i + len(new)] == gemm, names[i:i + 3]
        assert sum(n.startswith("sn_spna_") for n in names) == nlayer * len(new), names


# ----------------------------------------------------------------------------- 5. errors
def test_index_errors_are_the_references():
    import types
    from signnet_basisnet_amd.pyg_gnn_types import GNN
    N = 202
    star = torch.stack([torch.arange(1, N), torch.zeros(N - 1, dtype=torch.long)])          # 201 in-edges at node 0
    data = types.SimpleNamespace(x=torch.zeros(N, 1, dtype=torch.long), edge_index=star, edge_attr=torch.ones(N - 1, dtype=torch.long),
                                 batch=torch.zeros(N, dtype=torch.long), num_graphs=1, num_nodes=N)
    data = types.SimpleNamespace(**{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in vars(data).items()})
    torch.manual_seed(0)
    pna = GNN(None, None, 16, 1, 1, "SimplifiedPNAConv").to(DEV).eval()
    with torch.no_grad(), pytest.raises(IndexError):
        pna(data)
    data.edge_index = star[:, :199].contiguous().to(DEV)          # in-degree 199: the last row of the table
    data.edge_attr = data.edge_attr[:199].contiguous()
    with torch.no_grad():
        assert bool(torch.isfinite(pna(data)).all())
    gcn = GNN(None, None, 16, 1, 1, "GCNConv").to(DEV).eval()
    with torch.no_grad():
        assert bool(torch.isfinite(gcn(data)).all())
        data.edge_attr = data.edge_attr.clone()
        data.edge_attr[7] = 500          # one past the edge encoder's table
        with pytest.raises(IndexError):
            gcn(data)


# ----------------------------------------------------------------------------- 6. parameters move
@pytest.mark.parametrize("name", ["gnn_types_gin_h16_l2_add", "gnn_types_gcn_h16_l2_mean", "gnn_types_gat_h16_l2_add", "gnn_types_pna_h32_l3_add_pe"])
def test_eval_after_optimiser_steps_uses_the_new_weights(name):
    from signnet_basisnet_amd import optim, synth
    fx = G.load(name)
    data = synth.batch_to(G.as_data(fx.inp), DEV)
    pe = fx.inp.get("additional_x")
    pe = None if pe is None else pe.to(DEV)
    model = _model(fx).eval()
    with torch.no_grad():
        y0 = model(data, pe)
    opt = optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-5)
    model.train()
    target = _cotangent(y0.shape).to(DEV)
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.l1_loss(model(data, pe), target).backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        y = model(data, pe)
    fresh = _model(fx)
    fresh.load_state_dict(model.state_dict())
    with torch.no_grad():
        assert torch.equal(fresh.eval()(data, pe), y)
    assert PU.relerr(y, y0) > 1e-4


# ----------------------------------------------------------------------------- 7. nothing shared was disturbed
_UNTOUCHED = r"""
import sys
import torch
import golden_util as G
from signnet_basisnet_amd import synth
from signnet_basisnet_amd.pyg import SignNetGNN
from signnet_basisnet_amd.dropin.baseline_core_model import GNN as PlainGNN
NEW = ("signnet_basisnet_amd.pyg_gnn_types", "signnet_basisnet_amd.dropin.gnn_types_core_model")
fx = G.load("gine_d16")
c = [None if v < 0 else int(v) for v in fx.meta["ctor"]]
model = SignNetGNN(*c, variant=str(fx.meta["variant"]))
model.load_state_dict(G.full_state_dict(fx))
model = model.to("cuda:0").eval()
data = synth.batch_to(G.as_data(fx.inp), "cuda:0")
before = model(data).clone()
bfx = G.load("plain_gnn_h32_l2_mean_pe")
plain = PlainGNN(None, None, 32, 1, 2, "GINEConv", 0, "mean")
plain.load_state_dict(G.full_state_dict(bfx))
plain = plain.to("cuda:0")
bdata, bpe = synth.batch_to(G.as_data(bfx.inp), "cuda:0"), bfx.inp["additional_x"].to("cuda:0")
with torch.no_grad():
    plain_eval = plain.eval()(bdata, bpe).clone()
assert not any(m in sys.modules for m in NEW), "the outputs above were to be taken before the new modules are imported"
from signnet_basisnet_amd.dropin.gnn_types_core_model import GNN
for name in ("gnn_types_pna_h16_l2_add", "gnn_types_gcn_h16_l2_add", "gnn_types_gat_h16_l2_add", "gnn_types_gin_h16_l2_add"):
    nfx = G.load(name)
    net = GNN(None, None, 16, 1, 2, str(nfx.meta["gnn_type"]), 0, "add")
    net.load_state_dict(G.full_state_dict(nfx))
    net.to("cuda:0").train()(synth.batch_to(G.as_data(nfx.inp), "cuda:0")).sum().backward()
assert torch.equal(model(data), before)
with torch.no_grad():
    assert torch.equal(plain.eval()(bdata, bpe), plain_eval)
# the same GINEConv net through the new class: the same launches, bit for bit
same = GNN(None, None, 32, 1, 2, "GINEConv", 0, "mean")
same.load_state_dict(G.full_state_dict(bfx))
with torch.no_grad():
    assert torch.equal(same.to("cuda:0").eval()(bdata, bpe), plain_eval)
print("UNTOUCHED " + str(float((before.cpu() - fx.out["eval/y"]).abs().max() / fx.out["eval/y"].abs().max())))
"""


def test_signnet_gnn_and_the_gine_plain_gnn_are_untouched_by_the_new_modules():
    """In a fresh interpreter: the outputs of SignNetGNN and of the GINEConv plain GNN, taken before the new modules are imported, are
    `torch.equal` to their outputs after those were imported and each new net ran a training step."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, "-c", _UNTOUCHED], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "UNTOUCHED " in out.stdout, out.stdout + out.stderr
    assert float(out.stdout.split("UNTOUCHED ")[1].split()[0]) <= 1e-4          # (and the model did run: its output is the fixture's)
