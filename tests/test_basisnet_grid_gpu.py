"""-m gpu: every dispatch branch of the BasisNet / LearningFilters kernels (csrc/eigenspace.hip, csrc/ign_mlp.hip, the IGN contractions of
csrc/ops.hip) against float64.

One parametrized test per op over its table in tests/basisnet_cases.py.  A row runs the HIP entry point and the float32 and float64 CPU
restatements on the same inputs; floating-point outputs are checked with the project's attribution rule (parity_util.attributed):

    |hip - f64| <= max(REL * scale, 2 |cpu32 - f64| + ATTR * scale),   scale = max |f64|

(the contraction ops: every output column on its own), integer outputs with torch.equal.  Every output buffer sits between NaN-filled
guards that must still be NaN afterwards while the interior holds none, and every row runs twice and must repeat bit for bit (no float
atomics in these kernels).  tests/test_basisnet_cases_cpu.py asserts, without a GPU, that every row reaches the branch it names and that
float32 itself is within REL there.
"""
import ctypes as C

import pytest
import torch

import basisnet_cases as BC
import parity_util as PU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SN_ERR_ARG = -1
WORST = {}


def ids(cases):
    return [c.id for c in cases]


def guarded(numel, guard=GUARD):
    """(buffer, interior view): `numel` floats between two NaN-filled guards; the interior starts NaN-filled too"""
    assert guard >= GUARD and guard % 4 == 0
    buf = torch.full((guard + numel + guard,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[guard:guard + numel]


def check_guards(buf, numel, what, guard=GUARD, interior=True):
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:guard]).all()), f"{what}: written in front of the output"
    assert bool(torch.isnan(buf[guard + numel:]).all()), f"{what}: written behind the output"
    if interior:
        assert not bool(torch.isnan(buf[guard:guard + numel]).any()), f"{what}: output elements not written (or NaN)"


def offset_view(t):
    """a contiguous device copy of t that starts 4 bytes into a 16-byte aligned buffer"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def accept(case, hip, r32, r64, what):
    e = PU.attributed(hip, r32, r64, f"{case.id} [{case.branch}] {what}")
    w = WORST.get(case.op, (0.0, 0.0, ""))
    WORST[case.op] = max(w, (*e, f"{case.id} {what}"))
    print(f"\n{case.id} {what}: |hip - f64| {e[0]:.2e}, |cpu32 - f64| {e[1]:.2e}; worst of {case.op} so far {WORST[case.op][0]:.2e} / "
          f"{WORST[case.op][1]:.2e} ({WORST[case.op][2]})", end="")


def twice(run):
    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y), "two runs differ"
    return a


def refused(rc, match):
    from signnet_basisnet_amd._lib import lib
    assert rc == SN_ERR_ARG, rc
    msg = lib().sn_last_error().decode()
    assert match in msg, msg


# ---------------------------------------------------------------------------- sn_ign_contract_2to1_f32
@pytest.mark.parametrize("case", BC.CONTRACT, ids=ids(BC.CONTRACT))
def test_ign_contract_2to1(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    b, n = case.p["b"], case.p["n"]
    X = BC.contract_gen(case)
    Xd = offset_view(X) if case.p.get("misaligned") else X.to(DEV)
    assert case.p.get("misaligned") or Xd.data_ptr() % 16 == 0
    nscr = int(lib().sn_ign_contract_scratch_floats(b, n))

    def run():
        obuf, o = guarded(b * n * 5)
        sbuf, s = guarded(nscr)
        assert s.data_ptr() % 16 == 0
        check(lib().sn_ign_contract_2to1_f32(ptr(Xd), b, n, ptr(o), ptr(s), stream()), "sn_ign_contract_2to1_f32")
        check_guards(obuf, b * n * 5, f"{case.id} ops")
        check_guards(sbuf, nscr, f"{case.id} scratch", interior=False)          # (the 128-row strips leave part of the partials unused)
        return (o.view(b, n, 5).cpu(),)

    hip, = twice(run)
    r32, r64 = BC.contractions_2to1(X), BC.contractions_2to1(X.double())
    for c, name in enumerate(BC.COLUMNS):
        accept(case, hip[..., c], r32[..., c], r64[..., c], name)
    assert torch.equal(hip[..., 0], torch.diagonal(X, dim1=1, dim2=2))         # the diagonal is a copy


# ---------------------------------------------------------------------------- sn_eigenspace_group
GROUP_FIELDS = ("space_of", "space_start", "space_mult", "space_slot", "mult_list", "mult_count", "meta")


def group_raw(ev_dev, N, decimals):
    """the raw entry point on int32 regions carved out of one NaN-filled float buffer, a guard in front of, between and behind them
    -> (rc, {field: int32 view}, guard check)"""
    from signnet_basisnet_amd._lib import lib, ptr, stream
    M = max(N, 1)
    sizes = dict(space_of=M, space_start=M + 1, space_mult=M, space_slot=M, mult_list=M, mult_count=M, meta=4)
    buf = torch.full((GUARD + sum(s + GUARD for s in sizes.values()),), float("nan"), dtype=torch.float32, device=DEV)
    ints, views, off = buf.view(torch.int32), {}, GUARD
    spans = []
    for f in GROUP_FIELDS:
        views[f] = ints[off:off + sizes[f]]
        spans.append((off, sizes[f]))
        off += sizes[f] + GUARD
    rc = lib().sn_eigenspace_group(ptr(ev_dev), N, decimals, *[ptr(views[f]) for f in GROUP_FIELDS], stream())
    torch.cuda.synchronize()

    def guards_intact():
        keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
        for o, s in spans:
            keep[o:o + s] = False
        return bool(torch.isnan(buf[keep]).all())
    return rc, views, guards_intact, buf


@pytest.mark.parametrize("case", BC.GROUP, ids=ids(BC.GROUP))
def test_eigenspace_group(case):
    from signnet_basisnet_amd import ops
    ev = BC.group_gen(case)
    N, d = ev.numel(), case.p["decimals"]
    ref = BC.group_reference(ev, d)
    evd = ev.to(DEV)

    def run():
        rc, v, guards_intact, _ = group_raw(evd, N, d)
        assert rc == 0 and guards_intact(), f"{case.id}: rc {rc}, or written outside an output array"
        ns, nm, err, mmax = v["meta"].tolist()
        assert err == 0
        return (v["space_of"].cpu(), v["space_start"][:ns + 1].cpu(), v["space_mult"][:ns].cpu(), v["space_slot"][:ns].cpu(),
                v["mult_list"][:nm].cpu(), v["mult_count"][:nm].cpu(), v["meta"].cpu())

    space_of, space_start, space_mult, space_slot, mult_list, mult_count, meta = twice(run)
    assert meta.tolist() == [ref["n_spaces"], len(ref["mults"]), 0, ref["max_mult"]]
    for name, got in (("space_of", space_of), ("space_start", space_start), ("space_mult", space_mult), ("space_slot", space_slot)):
        assert got.dtype == torch.int32 and torch.equal(got, ref[name]), f"{case.id} [{case.branch}] {name}"
    assert mult_list.tolist() == ref["mults"] and mult_count.tolist() == ref["counts"]
    plan = ops.eigenspace_group(evd, d)                        # and what the wrapper makes of it
    assert (plan.N, plan.mults, plan.counts, plan.n_spaces, plan.max_mult) == (N, ref["mults"], ref["counts"], ref["n_spaces"], ref["max_mult"])
    assert torch.equal(plan.space_slot[:plan.n_spaces].cpu(), ref["space_slot"])


@pytest.mark.parametrize("r", BC.GROUP_REFUSED, ids=lambda r: f"N{r['N']}-decimals{r['decimals']}")
def test_eigenspace_group_refuses(r):
    ev = torch.zeros(max(r["N"], 1), device=DEV)
    rc, _, guards_intact, buf = group_raw(ev, r["N"], r["decimals"])
    refused(rc, r["match"])
    assert bool(torch.isnan(buf).all())                        # nothing was launched


@pytest.mark.parametrize("N,at", [(3, 1), (300, 151), (300, 200), (8192, 4096)])
def test_eigenspace_group_descending_input_raises(N, at):
    """a single descent, inside a thread's chunk and on a chunk boundary (per = 2: 200 = 100 * per; per = 32: 4096 = 128 * per)"""
    from signnet_basisnet_amd import ops
    ev = 0.01 * torch.arange(N, dtype=torch.float32)
    ev[at] = ev[at - 1] - 0.005
    with pytest.raises(ValueError, match="ascending"):
        ops.eigenspace_group(ev.to(DEV))
    assert ops.eigenspace_group(torch.sort(ev).values.to(DEV)).n_spaces == N            # the entry point serves the next call


# ---------------------------------------------------------------------------- sn_eigenspace_projectors_f32 / sn_ign_contract_eigvecs_f32
@pytest.mark.parametrize("case", BC.PROJECTORS, ids=ids(BC.PROJECTORS))
def test_eigenspace_projectors_and_contractions(case):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    ev, V = BC.projector_gen(case)
    N, pad = V.shape[0], case.p["pad"]
    ref = BC.group_reference(ev, 5)
    plan = ops.eigenspace_group(ev.to(DEV))
    ns = plan.n_spaces
    assert ns == ref["n_spaces"] and plan.max_mult == ref["max_mult"] and plan.mults == ref["mults"] and plan.counts == ref["counts"]
    assert torch.equal(plan.space_start[:ns + 1].cpu(), ref["space_start"]) and torch.equal(plan.space_slot[:ns].cpu(), ref["space_slot"])
    ldv = N + pad
    Vd = torch.full((N, ldv), float("nan"), dtype=torch.float32, device=DEV)          # the padding of the wider buffer holds NaN
    Vd[:, :N] = V.to(DEV)

    def run():
        pbuf, P = guarded(ns * N * N)
        check(lib().sn_eigenspace_projectors_f32(ptr(Vd), N, ldv, ptr(plan.space_start), ptr(plan.space_slot), ns, ptr(P), stream()),
              "sn_eigenspace_projectors_f32")
        check_guards(pbuf, ns * N * N, f"{case.id} projectors")
        cbuf, c = guarded(ns * N * 5)
        check(lib().sn_ign_contract_eigvecs_f32(ptr(Vd), N, ldv, ptr(plan.space_start), ptr(plan.space_slot), ns, plan.max_mult, ptr(c),
                                                stream()), "sn_ign_contract_eigvecs_f32")
        check_guards(cbuf, ns * N * 5, f"{case.id} contractions")
        return P.view(ns, N, N).clone(), c.view(ns, N, 5).clone()

    Pd, cd = twice(run)
    P, c = Pd.cpu(), cd.cpu()
    P32, P64 = BC.projectors(V, ref, BC.F32), BC.projectors(V, ref, BC.F64)
    accept(case, P, P32, P64, "projectors")
    c32, c64 = BC.contractions_2to1(P32), BC.contractions_2to1(P64)
    for k, name in enumerate(BC.COLUMNS):
        accept(case, c[..., k], c32[..., k], c64[..., k], f"eigvecs {name}")
    assert torch.equal(c[..., 2], c[..., 3])                      # row sums = column sums of a symmetric matrix: the same number stored twice
    # the stacking order is plan.group's: the eigenspaces of one multiplicity, in eigenvalue order, without going through the slots
    st, V64 = ref["space_start"].tolist(), V.double()
    c2 = ops.ign_contract_2to1(Pd)
    for m in plan.mults:
        spaces = [s for s in range(ns) if st[s + 1] - st[s] == m]
        want64 = torch.stack([V64[:, st[s]:st[s + 1]] @ V64[:, st[s]:st[s + 1]].T for s in spaces])
        want32 = torch.stack([V[:, st[s]:st[s + 1]] @ V[:, st[s]:st[s + 1]].T for s in spaces])
        got = plan.group(Pd, m).cpu()
        assert got.shape == want64.shape
        accept(case, got, want32, want64, f"plan.group(projectors, {m})")
        # and the projector-free contractions agree with the contraction kernel applied to the device-built projectors (the bound of
        # test_eigenspace_grouping_device_op_vs_reference_statements)
        dscale = torch.diagonal(want64, dim1=1, dim2=2).abs().max().item()
        diff = (plan.group(cd, m).double() - plan.group(c2, m).double()).abs().max().item()
        assert diff <= 2e-6 * dscale, f"{case.id} m={m}: eigvecs vs projector contractions differ by {diff:.2e} (diag scale {dscale:.2e})"


# ---------------------------------------------------------------------------- sn_ign_mlp_f32
def ign_module(case, sd):
    from signnet_basisnet_amd import basisnet as BN
    enc = BN.IGN2to1(1, case.p["H"], case.p["O"])
    res = enc.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("bns.3.") or k.endswith("num_batches_tracked") for k in res.missing_keys), res
    return enc.to(DEV).eval()


@pytest.mark.parametrize("case", BC.IGN_MLP, ids=ids(BC.IGN_MLP))
def test_ign_mlp(case):
    from signnet_basisnet_amd import basisnet as BN
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    b, n, H, O = (case.p[k] for k in "bnHO")
    assert lib().sn_ign_mlp_supported(n, H, O) == 1
    o, sd = BC.ign_mlp_gen(case)
    enc = ign_module(case, sd)
    prep = enc._prepare()
    params = prep["mlp"]
    if case.p.get("no_fc2_bias"):
        params = BN._IgnMlpParams(*[getattr(params, f) for f, _ in BN._IgnMlpParams._fields_])
        params.fc2_b = None
    od = o.to(DEV)
    guard = GUARD + 32 * n          # (a store of the output tile's lanes past O lands here, not outside the allocation)

    def run():
        buf, y = guarded(b * O * n, guard)
        check(lib().sn_ign_mlp_f32(ptr(od), b, n, H, O, C.byref(params), ptr(y), stream()), "sn_ign_mlp_f32")
        check_guards(buf, b * O * n, case.id, guard)
        return (y.view(b, O, n).clone(),)

    yd, = twice(run)
    accept(case, yd.cpu(), BC.ign_head(o, sd, BC.F32), BC.ign_head(o, sd, BC.F64), "y")
    if not case.p.get("no_fc2_bias"):
        with torch.no_grad():
            assert torch.equal(enc.forward_contractions(od), yd)          # the module takes this kernel


@pytest.mark.parametrize("case", BC.IGN_MLP_UNSUPPORTED, ids=ids(BC.IGN_MLP_UNSUPPORTED))
def test_ign_mlp_unsupported_shapes_take_the_layer_path_and_the_entry_point_refuses(case):
    from signnet_basisnet_amd._lib import lib, ptr, stream
    b, n, H, O = (case.p[k] for k in "bnHO")
    assert lib().sn_ign_mlp_supported(n, H, O) == 0
    o, sd = BC.ign_mlp_gen(case)
    enc = ign_module(case, sd)
    od = o.to(DEV)
    with torch.no_grad():
        y = enc.forward_contractions(od)
    accept(case, y.cpu(), BC.ign_head(o, sd, BC.F32), BC.ign_head(o, sd, BC.F64), "y (layer path)")
    buf, yraw = guarded(b * O * n)
    prep = enc._prepare()
    refused(lib().sn_ign_mlp_f32(ptr(od), b, n, H, O, C.byref(prep["mlp"]), ptr(yraw), stream()), "sn_ign_mlp_f32")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


# ---------------------------------------------------------------------------- sn_deepsets_tail_f32
def tail_params(layers, widths, use_bn, split0):
    from signnet_basisnet_amd import basisnet as BN
    P = BN._DeepSetsTailParams()
    P.n_layers, P.use_bn, P.eps, P.split0 = len(widths), use_bn, BC.BN_EPS, split0
    for i, w in enumerate(widths):
        P.width[i] = w
    for i in range(1, len(widths)):
        P.w1[i], P.b1[i], P.w2[i], P.b2[i] = (layers[i][k].data_ptr() for k in ("w1", "b1", "w2", "b2"))
        if use_bn:
            P.gamma[i - 1], P.beta[i - 1] = layers[i - 1]["gamma"].data_ptr(), layers[i - 1]["beta"].data_ptr()
    return P


@pytest.mark.parametrize("case", BC.DEEPSETS, ids=ids(BC.DEEPSETS))
def test_deepsets_tail(case):
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    p = case.p
    n, widths = p["n"], p["widths"]
    assert len(widths) <= BC.DS_MAX_LAYERS
    x, layers = BC.deepsets_gen(case)
    dev = [{k: v.to(DEV).contiguous() for k, v in L.items()} for L in layers]
    P = tail_params(dev, widths, p["use_bn"], p["split0"])
    z = BC.deepsets_first_layer(x, layers[0], p["split0"]).to(DEV)
    assert z.shape == (n, (2 if p["split0"] else 1) * widths[0])

    def run():
        buf, y = guarded(n * widths[-1])
        check(lib().sn_deepsets_tail_f32(ptr(z), n, C.byref(P), ptr(y), stream()), "sn_deepsets_tail_f32")
        check_guards(buf, n * widths[-1], case.id)
        return (y.view(n, widths[-1]).cpu(),)

    y, = twice(run)
    accept(case, y, BC.eq_deepsets(x, layers, BC.F32), BC.eq_deepsets(x, layers, BC.F64), "y")


def test_deepsets_tail_limit_in_the_module_and_the_entry_point():
    """n * widest == 16384 runs the kernel; one row more takes the layer path in the module and is refused by the entry point"""
    from signnet_basisnet_amd import basisnet as BN
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd._lib import lib, ptr, stream
    over = BC.DEEPSETS_OVER_LIMIT
    widths, fin = over.p["widths"], over.p["fin"]
    torch.manual_seed(5)
    enc = BN.EqDeepSetsEncoder(fin, hidden_channels=widths[0], num_layers=len(widths), out_channels=widths[-1], use_bn=True)
    with torch.no_grad():
        for bn in enc.bns:
            bn.weight.uniform_(0.7, 1.3); bn.bias.uniform_(0.2, 0.5)
    enc = enc.to(DEV).eval()
    layers = BC.layers_of(enc)
    for n, fused in ((over.p["n"] - 1, True), (over.p["n"], False)):
        assert BC.deepsets_supported(n, widths) == fused
        x = torch.randn(n, fin, generator=BC.rng(over, n))
        rec = ops.KernelTimer()
        with rec, torch.no_grad():
            y = enc(x.to(DEV))
        assert ("sn_deepsets_tail_f32" in [s[0] for s in rec.spans]) == fused
        accept(over, y.cpu(), BC.eq_deepsets(x, layers, BC.F32), BC.eq_deepsets(x, layers, BC.F64), f"module n={n}")
    dev = [{k: v.to(DEV).contiguous() for k, v in L.items()} for L in layers]
    z = BC.deepsets_first_layer(x, layers[0], 1).to(DEV)
    buf, y = guarded(over.p["n"] * widths[-1])
    refused(lib().sn_deepsets_tail_f32(ptr(z), over.p["n"], C.byref(tail_params(dev, widths, 1, 1)), ptr(y), stream()), "16384")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
