"""-m gpu: every dispatch branch and every launch structure of the training link kernels (csrc/train.hip) against float64.

One parametrized test over the rows of tests/train_stage_cases.py.  A row runs the public function of train_stage.py (the raw rows: the
entry points themselves, on poisoned buffers), the float32 CPU autograd and the float64 CPU autograd of the restatement on the same inputs
and the same seeded cotangents, under every launch structure the row lists:

  autograd   plain parameters, one backward pass
  direct*    every parameter owns a zeroed .grad the kernels accumulate into (`_sn_direct_grad`, as optim.FlatAdam marks them): TWO forward
             and backward passes with different cotangents, nothing zeroed in between, flush_deferred() after each — the accumulated
             gradients against the float64 sum of the two passes; MERGE_COEF / DEFER_DW switched per structure

and checks the output, every input gradient and every parameter gradient with the family's attribution rule (parity_util.attributed),
exact zeros on invalid rows, the BatchNorm running statistics after all sequential updates, bitwise reproducibility of a second run, and
— with a counter on the library handle — that the structure ran the reduction / finish entry points the host restatement says it runs.
tests/test_train_stage_cases_cpu.py asserts, without a GPU, that the rows reach every branch and are well conditioned.
"""
import types
from collections import Counter

import pytest
import torch

import parity_util as PU
import train_stage_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c.id for c in TC.TABLE]
PARAM_PREFIX = ("W", "b", "g", "eps")          # leaves that are parameters (b*, be*: biases and BatchNorm shifts)
SKIPPED = []                                    # rows whose `capped` atoms differ on a device without 256 CUs


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------------------- dispatch pin
@pytest.mark.parametrize("case", TC.TABLE, ids=IDS)
def test_block_counts_are_the_restatement_s(case):
    from signnet_basisnet_amd._lib import lib
    cus = _cus()
    fn = {"fwd": (lib().sn_train_linear_blocks, TC.fwd_blocks), "bwd": (lib().sn_train_linear_bwd_blocks, TC.bwd_blocks),
          "bn": (lib().sn_train_bn_bwd_blocks, TC.bn_bwd_blocks)}
    for kind, R, G in TC.trace(case, cus).shapes:
        assert int(fn[kind][0](R, G)) == fn[kind][1](R, G, cus), (kind, R, G, cus)
    if cus != TC.CUS and set(TC.trace(case, cus).atoms) != set(TC.trace(case).atoms):
        SKIPPED.append(case.id)
        pytest.skip(f"{cus} CUs: the row's capped atoms are written for {TC.CUS}")


def test_rows_skipped_for_the_cu_count():
    """(runs after the pin: same module, definition order)"""
    print(f"\nrows skipped for the CU count ({_cus()} CUs): {len(SKIPPED)}", end="")
    assert _cus() != TC.CUS or not SKIPPED


# ---------------------------------------------------------------------------- running a row
def _is_param(name):
    return name.startswith(PARAM_PREFIX)


class Counted:
    """counts the calls of the reduction / finish entry points on the library handle"""

    def __enter__(self):
        from signnet_basisnet_amd._lib import lib
        self.L, self.calls, self.orig = lib(), Counter(), {}
        for name in TC.COUNTED:
            self.orig[name] = getattr(self.L, name)
            setattr(self.L, name, self._wrap(name))
        return self.calls

    def _wrap(self, name):
        orig = self.orig[name]

        def counted(*a):
            self.calls[name] += 1
            return orig(*a)
        return counted

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(self.L, name, fn)


def _weight_view(W, how):
    """a weight that is a view of a leaf: ldw = d_in + 1, or one float off a 16-byte boundary -> (view, leaf, gradient of the view)"""
    d_out, d_in = W.shape
    if how == "ld":
        leaf = torch.zeros(d_out, d_in + 1, device=DEV)
        leaf[:, :d_in] = W
        leaf.requires_grad_(True)
        view = leaf[:, :d_in]
        assert view.stride(0) % 4 == 1
        return view, leaf, lambda: leaf.grad[:, :d_in]
    leaf = torch.zeros(W.numel() + 4, device=DEV)
    leaf[1:1 + W.numel()] = W.reshape(-1)
    leaf.requires_grad_(True)
    view = leaf[1:1 + W.numel()].view(d_out, d_in)
    assert view.data_ptr() % 16 == 4
    return view, leaf, lambda: leaf.grad[1:1 + W.numel()].view(d_out, d_in)


class Device:
    """the leaves of a row on the device, the modules built over them, and where each leaf's gradient ends up"""

    def __init__(self, case, L, direct):
        self.t, self.grad_of, self.bns = {}, {}, {}
        for k, v in L.items():
            if _is_param(k) and k.startswith("W") and case.p.get("wview"):
                self.t[k], _, self.grad_of[k] = _weight_view(v, case.p["wview"])
                continue
            t = torch.nn.Parameter(v.to(DEV)) if _is_param(k) else v.to(DEV).requires_grad_(TC.wants_grad(case, k))
            if direct and _is_param(k):          # parameters whose .grad the optimiser owns (optim.FlatAdam): the adjoints add into them
                t.grad = torch.zeros_like(t)
                t._sn_direct_grad = True
            self.t[k] = t
            if t.requires_grad:
                self.grad_of[k] = (lambda t=t: t.grad)

    def lin(self, key):
        return types.SimpleNamespace(weight=self.t["W" + key], bias=self.t.get("b" + key))

    def bn(self, key):
        if key not in self.bns:
            bn = torch.nn.BatchNorm1d(self.t["g" + key].numel(), eps=TC.BN_EPS).to(DEV).train()
            bn.weight, bn.bias = self.t["g" + key], self.t["be" + key]
            self.bns[key] = bn
        return self.bns[key]


def _nv(aux):
    return None if aux["nv"] is None else aux["nv"].to(DEV)


@torch.no_grad()
def _plans(aux, G):
    from signnet_basisnet_amd import ops
    gr = aux["gr"]
    batch, ei = gr.batch.to(DEV), gr.ei.to(DEV)
    plan = ops.build_plan(batch, ei, len(gr.sizes), aux.get("K", 0) or 0)
    rplan = ops.build_plan(batch, ei.flip(0).contiguous(), len(gr.sizes), 0)
    plan.check()
    return (ops.doubled_plan(plan), ops.doubled_plan(rplan), plan) if G == 2 else (plan, rplan, plan)


def forward(case, aux, D):
    """the public function of the row -> tuple of outputs"""
    from signnet_basisnet_amd import train_stage as T
    p, t, op = case.p, D.t, case.op
    nv, K = _nv(aux), aux["K"]
    if op == "mlp2_bn":
        return (T.mlp2_bn(t["x"], D.lin("1"), D.bn("1"), D.lin("2"), D.bn("2") if p["bn2"] else None, nv, K, p["G"], residual=t.get("res"),
                          relu_out=p["relu_out"]),)
    if op == "lin_bn":
        return (T.lin_bn(t["x"], D.lin(""), D.bn(""), nv, K, relu=p["relu"], residual=t.get("res")),)
    if op == "linear":
        if p["wview"]:
            return (T.linear(t["x"], t["W"], t.get("b"), nv, K, relu=p["relu"]),)
        return (T.linear_module(t["x"], D.lin(""), nv, K, relu=p["relu"]),)
    if op == "qkv":
        return T.qkv(t["x"], *(types.SimpleNamespace(weight=t["W" + k], bias=None) for k in "qkv"), nv, K)
    if op == "sign_sum":
        return (T.sign_sum(t["x"], nv, K),)
    if op == "scalar_mlp":
        return (T.scalar_mlp(t["x"], D.lin("1"), D.bn("1"), D.lin("2"), D.bn("2"), nv, K, G=p["G"], negate_second=(p["G"] == 2)),)
    if op == "gin_layer":
        plan, rplan, base = _plans(aux, p["G"])
        assert torch.equal(base.nvalid.cpu(), aux["nv"])          # the generator's nvalid is the plan's
        return (T.gin_layer(t["x"], t["eps"], D.lin("1"), D.bn("1"), D.lin("2"), D.bn("2"), plan, rplan, nv, K, p["G"]),)
    if op == "gine_layer":
        plan, rplan, _ = _plans(aux, 1)
        h, e = t["x"], t["e"]
        if p["block"]:
            e._sn_gbuf = torch.full_like(e, 7.0)          # (autograd.embedding_sum_layers: empty_like — every plane is written by its layer)
        for l in range(aux["layers"]):
            h = T.gine_layer(h, e, t[f"eps{l}"], D.lin(f"{l}a"), D.bn(f"{l}a"), D.lin(f"{l}b"), D.bn(f"{l}b"), plan, rplan,
                             layer=l if p["block"] else -1, nvalid=nv, K=K)
        return (h,)
    raise KeyError(op)


def run(case, L, aux, variant, monkeypatch):
    """-> (outputs of the first pass, {leaf: gradient}, BatchNorm modules, counted calls, passes)"""
    from signnet_basisnet_amd import train_stage as T
    direct, merge, defer = TC.VARIANTS[variant]
    monkeypatch.setattr(T, "MERGE_COEF", merge or not direct)          # (autograd: the module default, which plain parameters do not take)
    monkeypatch.setattr(T, "DEFER_DW", defer or not direct)
    npass = 2 if direct else 1
    D = Device(case, L, direct)
    vv = aux["valid"]
    first = None
    with Counted() as calls:
        for i in range(npass):
            outs = forward(case, aux, D)
            rows = vv.repeat(outs[0].shape[0] // max(vv.numel(), 1)) if vv.numel() else vv
            torch.autograd.backward(outs, [TC.cots(case, i, j, o.shape, rows).float().to(DEV) for j, o in enumerate(outs)])
            T.flush_deferred()
            first = first or [o.detach() for o in outs]
        torch.cuda.synchronize()
    grads = {k: f() for k, f in D.grad_of.items()}
    return first, grads, D.bns, calls, npass


def compare(case, what, hip, r32, r64, gmax, zero):
    assert hip is not None, f"{case.id} {what}: no gradient"
    assert tuple(hip.shape) == tuple(r64.shape), f"{case.id} {what}: shape {tuple(hip.shape)} vs {tuple(r64.shape)}"
    if r64.numel() == 0:
        return 0.0, 0.0
    scale = r64.abs().max().item()
    if zero:            # a bias in front of a batch-statistics BatchNorm: true gradient 0 (float64 <= 1e-9 of the largest gradient)
        assert scale <= 1e-9 * gmax and hip.abs().max().item() <= 1e-5 * gmax, f"{case.id} {what}"
        return 0.0, 0.0
    if scale == 0:
        assert not bool(hip.any()), f"{case.id} {what}: exactly zero in float64"
        return 0.0, 0.0
    return PU.attributed(hip, r32, r64, f"{case.id} {what}")


def check_variant(case, L, aux, variant, monkeypatch):
    outs, grads, bns, calls, npass = run(case, L, aux, variant, monkeypatch)
    o64, g64, st64, _ = TC.reference(case, TC.F64, L, aux, npass)
    o32, g32, _, _ = TC.reference(case, TC.F32, L, aux, npass)
    assert len(outs) == len(o64) and set(grads) == set(g64), (sorted(grads), sorted(g64))
    gmax = max([v.abs().max().item() for v in g64.values() if v.numel()] + [0.0])
    zero, vv = TC.zero_bias(case), aux["valid"]
    worst = (0.0, 0.0, "")
    for what, h, a32, a64 in [(f"output {i}", *t) for i, t in enumerate(zip(outs, o32, o64))] + [("d" + k, grads[k], g32[k], g64[k]) for k in g64]:
        worst = max(worst, (*compare(case, f"[{variant}] {what}", h, a32, a64, gmax, what[1:] in zero), what))
        if (what.startswith("output") or what in ("dx", "dres")) and vv.numel() and h.dim() == 2 and h.shape[0] % vv.numel() == 0:
            inv = ~vv.repeat(h.shape[0] // vv.numel())
            assert not bool(h.detach().cpu()[inv].any()), f"{case.id} [{variant}] {what}: invalid rows must be exactly 0"
    # running statistics: one update per group and pass, in order (momentum 0.1, unbiased variance); the batch counter
    G = aux["G"]
    for key, bn in bns.items():
        rm, rv = torch.zeros(bn.num_features, dtype=torch.float64), torch.ones(bn.num_features, dtype=torch.float64)
        for _ in range(npass):
            for mean, var in st64.get("bn" + key, []):
                rm, rv = 0.9 * rm + 0.1 * mean, 0.9 * rv + 0.1 * var
        PU.close(bn.running_mean, rm, f"{case.id} [{variant}] bn{key}.running_mean", rel=2e-5)
        PU.close(bn.running_var, rv, f"{case.id} [{variant}] bn{key}.running_var", rel=2e-5)
        assert int(bn.num_batches_tracked) == npass * G, (key, int(bn.num_batches_tracked))
    # the launch structure ran what the restatement says
    want = TC.trace(case, _cus()).calls.get(variant, Counter())
    assert {k: calls[k] for k in TC.COUNTED} == {k: npass * want[k] for k in TC.COUNTED}, f"{case.id} [{variant}]"
    # bit-for-bit on a second run (no atomics)
    outs2, grads2, _, _, _ = run(case, L, aux, variant, monkeypatch)
    for a, b in list(zip(outs, outs2)) + [(grads[k], grads2[k]) for k in grads]:
        assert torch.equal(a, b), f"{case.id} [{variant}]: not reproducible"
    print(f"\n{case.id} [{variant}]: worst |hip - f64| {worst[0]:.2e}, |cpu32 - f64| there {worst[1]:.2e} ({worst[2]})", end="")


# ---------------------------------------------------------------------------- the raw entry points on poisoned buffers
def _poisoned(rows, ld, cols, value=None, at=0):
    buf = torch.full((rows, ld), 7.0, dtype=torch.float32, device=DEV)
    if value is not None:
        buf[:, at:at + cols] = value.to(DEV)
    return buf, buf[:, at:at + cols]


def run_raw(case, L, aux):
    import ctypes as C
    from signnet_basisnet_amd import train_stage as T
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    p = case.p
    (d_in, d_out), R, G, K = p["d"], p["R"], p["G"], aux["K"]
    rows, im = G * R, p["in_mode"] or ""
    ldx = p["ldx"] or d_in
    X, x = _poisoned(rows, ldx, d_in, L["x"], 4 if ldx - d_in >= 4 else 0)
    if p["wview"]:
        Wb, W = _poisoned(d_out, d_in + 1, d_in, L["W"])
    else:
        W = L["W"].to(DEV)
    b = L["b"].to(DEV) if "b" in L else None
    nv = _nv(aux)
    s, t = (aux["s"].to(DEV), aux["t"].to(DEV)) if "scale" in im else (None, None)
    bs, bt = (aux["s"].to(DEV), aux["t"].to(DEV)) if im else (None, None)          # in_relu alone: the backward takes it as x_scale = 1, x_shift = 0
    Y, y = _poisoned(rows, d_out + 4, d_out)
    a = T._LinArgs(ptr(x), ldx, R, G, d_in, d_out, ptr(W), W.stride(0), ptr(b), ptr(nv), K, ptr(s), ptr(t), int("relu" in im), int(p["out_relu"]),
                   ptr(y), d_out + 4, None)
    check(lib().sn_train_linear_f32(C.byref(a), stream()), "sn_train_linear_f32")
    DY, dy = _poisoned(rows, d_out + 8, d_out, TC.cots(case, 0, 0, (rows, d_out), aux["valid"].repeat(G)).float(), 4)
    GX, gx = _poisoned(rows, d_in + 4, d_in)
    nblk = int(lib().sn_train_linear_bwd_blocks(R, G))
    stride = d_out * d_in + (d_out if b is not None else 0)
    part = torch.full((G * nblk * stride + 16,), 7.0, dtype=torch.float32, device=DEV)
    one, nul = torch.ones(G, d_out, device=DEV), torch.zeros(G, d_out, device=DEV)
    q = T._BwdArgs(R, G, ptr(nv), K, d_in, d_out, ptr(dy), d_out + 8, ptr(y) if p["out_relu"] else None, d_out + 4 if p["out_relu"] else 0,
                   None, None, None, ptr(one) if p["out_relu"] else None, ptr(nul) if p["out_relu"] else None,
                   ptr(x), ldx, ptr(bs), ptr(bt), int("relu" in im), None, ptr(W), W.stride(0), ptr(gx), d_in + 4, None, ptr(part),
                   int(b is not None), 0, None, 0, None)
    if im == "relu":          # x_relu without x_scale / x_shift: refused before any launch, nothing written
        q.x_scale = q.x_shift = None
        with pytest.raises(RuntimeError, match="x_relu needs x_scale"):
            check(lib().sn_train_linear_bwd_f32(C.byref(q), stream()), "sn_train_linear_bwd_f32")
        torch.cuda.synchronize()
        assert bool((GX == 7.0).all()) and bool((part == 7.0).all())
        q.x_scale, q.x_shift = ptr(bs), ptr(bt)
    check(lib().sn_train_linear_bwd_f32(C.byref(q), stream()), "sn_train_linear_bwd_f32")
    out = torch.full((stride + 8,), 7.0, dtype=torch.float32, device=DEV)
    check(lib().sn_train_reduce_parts_f32(ptr(part), G * nblk, stride, stride, ptr(out), 0, stream()), "sn_train_reduce_parts_f32")
    torch.cuda.synchronize()
    # what the entry points were not asked to write is still 7.0
    cx = 4 if ldx - d_in >= 4 else 0
    keep = torch.ones(ldx, dtype=torch.bool)
    keep[cx:cx + d_in] = False
    assert bool((X[:, keep.to(DEV)] == 7.0).all()) and bool((Y[:, d_out:] == 7.0).all()) and bool((GX[:, d_in:] == 7.0).all())
    assert bool((DY[:, :4] == 7.0).all()) and bool((DY[:, 4 + d_out:] == 7.0).all())
    assert bool((part[G * nblk * stride:] == 7.0).all()) and bool((out[stride:] == 7.0).all())
    grads = {"x": gx, "W": out[:d_out * d_in].view(d_out, d_in)}
    if b is not None:
        grads["b"] = out[d_out * d_in:stride]
    return [y], grads


def check_raw(case, L, aux):
    outs, grads = run_raw(case, L, aux)
    o64, g64, _, _ = TC.reference(case, TC.F64, L, aux)
    o32, g32, _, _ = TC.reference(case, TC.F32, L, aux)
    assert set(grads) == set(g64)
    inv = ~aux["valid"].repeat(case.p["G"])
    for what, h, a32, a64 in [("output 0", outs[0], o32[0], o64[0])] + [("d" + k, grads[k], g32[k], g64[k]) for k in g64]:
        compare(case, what, h, a32, a64, 0.0, False)
        if what in ("output 0", "dx"):
            assert not bool(h.cpu()[inv].any()), f"{case.id} {what}: invalid rows must be exactly 0"
    outs2, grads2 = run_raw(case, L, aux)
    assert torch.equal(outs[0], outs2[0]) and all(torch.equal(grads[k], grads2[k]) for k in grads), f"{case.id}: not reproducible"


# ---------------------------------------------------------------------------- the grid
@pytest.mark.parametrize("case", TC.TABLE, ids=IDS)
def test_row_vs_float64(case, monkeypatch):
    L, aux = TC.OPS[case.op][0](case.p)
    if case.op == "raw_link":
        check_raw(case, L, aux)
        return
    for variant in case.p.get("variants", ("autograd",)):
        check_variant(case, L, aux, variant, monkeypatch)


def test_no_rows_then_rows_on_the_same_modules(monkeypatch):
    """R = 0: linear_fwd with a BatchNorm leaves the running statistics untouched and counts the batch, the backward returns zero dW —
    and the next non-empty call on the same modules is still right."""
    from signnet_basisnet_amd import train_stage as T
    case = next(c for c in TC.BY_OP["lin_bn"] if c.p["d"] == (128, 4))
    L, aux = TC.OPS["lin_bn"][0](case.p)
    D = Device(case, L, False)
    lin, bn = D.lin(""), D.bn("")
    x0 = torch.zeros(0, 128, device=DEV, requires_grad=True)
    y0 = T.lin_bn(x0, lin, bn, None, 0, relu=False)
    assert y0.shape == (0, 4) and int(bn.num_batches_tracked) == 1
    assert not bool(bn.running_mean.any()) and bool((bn.running_var == 1).all())
    # (a materialised cotangent, as every producer hands one: the stride-0 gradient of `y0.sum()` is refused by the entry points' row checks)
    y0.backward(torch.zeros(0, 4, device=DEV))
    torch.cuda.synchronize()
    assert not bool(lin.weight.grad.any()) and not bool(lin.bias.grad.any()) and not bool(bn.weight.grad.any()) and not bool(bn.bias.grad.any())
    for t in (lin.weight, lin.bias, bn.weight, bn.bias):
        t.grad = None
    outs = forward(case, aux, D)
    torch.autograd.backward(outs, [TC.cots(case, 0, 0, outs[0].shape, aux["valid"]).float().to(DEV)])
    o64, g64, st64, _ = TC.reference(case, TC.F64, L, aux)
    o32, g32, _, _ = TC.reference(case, TC.F32, L, aux)
    gmax = max(v.abs().max().item() for v in g64.values())
    compare(case, "output", outs[0], o32[0], o64[0], gmax, False)
    for k in g64:
        compare(case, "d" + k, D.grad_of[k](), g32[k], g64[k], gmax, k in TC.zero_bias(case))
    mean, var = st64["bn"][0]
    PU.close(bn.running_mean, 0.1 * mean, "running_mean", rel=2e-5)
    PU.close(bn.running_var, 0.9 + 0.1 * var, "running_var", rel=2e-5)
    assert int(bn.num_batches_tracked) == 2
