"""-m gpu: the counter source of the attention-dropout mask (sn_set_attention_drop_f32 / sn_set_attention_drop_bwd_f32,
SignNetGNN.attn_dropout_source = "counter") against the explicit-mask entry points fed the numpy restatement of the mask contract
(tests/attention_dropout_cases.py), against float64, and through GraphedStep / BucketedStep."""
import pytest
import torch

import adjoint_cases as AC
import attention_dropout_cases as ADC
import test_adjoint_grid_gpu as G
import test_bucketed_step_gpu as TB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = [c for c in AC.ATTENTION if c.p["drop"]]
SITE = ADC.SITE0 + 2


def _snap(seed, step):
    from signnet_basisnet_amd import ops
    return ops.DropoutState(seed, DEV, step).snapshot()


def _factors(p_case, p, seed, step, site=SITE):
    return torch.from_numpy(ADC.factors(p_case["N"], p_case["H"], p_case["K"], p, seed, step, site))


def _run(case, leaves, nvd, pm=None, drop=None):
    """forward + backward (the grid's seeded cotangent) of AG.set_attention on the row's inputs -> ([out], [dq, dk, dv])"""
    from signnet_basisnet_amd import autograd as AG
    p = case.p
    xs = [G.to_dev(t, p["offset"]) for t in leaves]
    out = AG.set_attention(*xs, p["N"], p["K"], p["H"], nvd, None if pm is None else pm.to(DEV), drop)
    G.backward([out], p["offset"])
    return [out.detach()], [x.grad for x in xs]


def _assert_same(a, b, what):
    for name, x, y in zip(("out", "dq", "dk", "dv"), a[0] + a[1], b[0] + b[1]):
        assert torch.equal(x, y), f"{what}: {name} differs in {int((x != y).sum())} of {x.numel()} elements, max {(x - y).abs().max().item():.3e}"


@pytest.mark.parametrize("p", ADC.PS)
@pytest.mark.parametrize("case", ROWS, ids=G.ids(ROWS))
def test_counter_kernels(case, p):
    leaves, aux = AC.attention_gen(case.p)
    nvd = G.nv_dev(aux)
    seed, step = ADC.SEED, ADC.STEP
    pm = _factors(case.p, p, seed, step)
    counter = _run(case, leaves, nvd, drop=(p, _snap(seed, step), SITE))
    # 1. bit equality with the explicit mask of the restated factors (forward, dq, dk, dv)
    _assert_same(counter, _run(case, leaves, nvd, pm=pm), f"{case.id} p={p} [{case.branch}] counter vs explicit mask")
    # 2. the grid's acceptance rule against float64 / float32 with aux["pm"] = the restated factors
    aux = dict(aux, pm=pm)
    G.check_case(case, lambda c, a, l: counter, leaves, aux)
    # 3. the same snapshot again: identical bits; the next step: another mask (a condition on the restatement) and another output
    _assert_same(counter, _run(case, leaves, nvd, drop=(p, _snap(seed, step), SITE)), f"{case.id} p={p} repeat")
    ok = (torch.arange(case.p["K"])[None, :] < aux["nv"][:, None])
    live = (ok[:, None, :, None] & ok[:, None, None, :]).expand_as(pm)
    pm_next = _factors(case.p, p, seed, step + 1)
    assert bool((pm_next != pm)[live].any()), "the restated masks of step and step + 1 agree on every valid element: choose another seed"
    nxt = _run(case, leaves, nvd, drop=(p, _snap(seed, step + 1), SITE))
    assert not torch.equal(nxt[0][0], counter[0][0])
    #    the extreme words: seed = 2^64 - 1, step = 2^32 - 1
    big = ((1 << 64) - 1, (1 << 32) - 1)
    _assert_same(_run(case, leaves, nvd, drop=(p, _snap(*big), SITE)), _run(case, leaves, nvd, pm=_factors(case.p, p, *big)),
                 f"{case.id} p={p} seed 2^64-1 step 2^32-1")
    # 4. rows at or beyond nvalid: exactly zero in the output and in every gradient
    dead = ~aux["valid"].to(DEV)
    for name, t in zip(("out", "dq", "dk", "dv"), counter[0] + counter[1]):
        assert not bool(t[dead].any()), f"{case.id} p={p}: {name} is not zero beyond nvalid"


@pytest.mark.parametrize("case", ROWS, ids=G.ids(ROWS))
def test_tiny_p_equals_the_launch_without_a_mask(case):
    leaves, aux = AC.attention_gen(case.p)
    nvd = G.nv_dev(aux)
    _assert_same(_run(case, leaves, nvd, drop=(ADC.P_TINY, _snap(ADC.SEED, ADC.STEP), SITE)), _run(case, leaves, nvd),
                 f"{case.id} p=2^-33 vs no mask")
    # p == 0 is the plain launch itself
    _assert_same(_run(case, leaves, nvd, drop=(0.0, _snap(ADC.SEED, ADC.STEP), SITE)), _run(case, leaves, nvd), f"{case.id} p=0")


def test_arguments():
    from signnet_basisnet_amd import autograd as AG
    from signnet_basisnet_amd import ops
    q = torch.randn(3 * 4, 32, device=DEV)
    snap = _snap(1, 1)
    with pytest.raises(ValueError, match="not both"):
        ops.set_attention(q, q, q, 3, 4, 2, None, torch.ones(3, 2, 4, 4, device=DEV), (0.1, snap, SITE))
    with pytest.raises(ValueError, match="probability"):
        AG.set_attention(q, q, q, 3, 4, 2, None, None, (1.0, snap, SITE))
    with pytest.raises(ValueError, match="snap"):
        ops.set_attention(q, q, q, 3, 4, 2, None, None, (0.1, snap.int(), SITE))


def test_backward_rejects_more_than_160k_of_lds_before_any_launch():
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd._lib import check, lib, ptr, stream
    r = AC.ATTENTION_REJECTED
    N, K, H, dk = r["N"], r["K"], r["H"], r["dk"]
    q, k, v, g = (torch.randn(N * K, H * dk, device=DEV) for _ in range(4))
    dq, dk_, dv = (torch.full_like(q, 7.0) for _ in range(3))
    thr, scale = ops.dropout_threshold(0.1)
    snap = _snap(1, 1)
    with pytest.raises(RuntimeError, match="LDS"):
        check(lib().sn_set_attention_drop_bwd_f32(ptr(q), ptr(k), ptr(v), ptr(g), N, K, H, dk, None, thr, scale, ptr(snap), SITE,
                                                  ptr(dq), ptr(dk_), ptr(dv), stream()), "sn_set_attention_drop_bwd_f32")
    torch.cuda.synchronize()
    for t in (dq, dk_, dv):
        assert bool((t == 7.0).all())
    test_tiny_p_equals_the_launch_without_a_mask(ROWS[1])          # the entry point serves the next call


# ----------------------------------------------------------------------------- module level
SEED, STEP = 0xC0FFEE, 5


def _model(variant, hid, max_k, source="generator", p=0.1):
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(7)
    if variant == "gine":
        m = SignNetGNN(None, None, hid, 1, 2, 2, variant="gine", max_k=max_k)
    else:
        m = SignNetGNN(6, 4, hid, 1, 2, 2, variant="alchemy", max_k=max_k)
    m = m.to(DEV).train()
    m.attn_dropout, m.attn_dropout_source = p, source
    return m.seed_dropout(SEED, STEP)


def _host(variant, graphs=7):
    from signnet_basisnet_amd import synth
    return synth.make_batch(graphs, seed=5, n_lo=3, n_hi=20, features="zinc" if variant == "gine" else "alchemy")


def _restated_masks(m, host, step):
    from signnet_basisnet_amd.pyg import N_HEAD
    N, K = int(host.batch.numel()), int(m.max_k or max(host.sizes))
    return [torch.from_numpy(ADC.factors(N, N_HEAD, K, m.attn_dropout, SEED, step, ADC.SITE0 + li)).to(DEV)
            for li in range(len(m.sign_net.rho.transformer_layers))]


def _train_step(m, d, target, grad=True):
    m.zero_grad(set_to_none=True)
    if not grad:
        with torch.no_grad():
            y = m(d)
        return [y.clone()] + [b.detach().clone() for b in m.buffers()]
    y = m(d)
    loss = (y - target).abs().mean()
    loss.backward()
    return [loss.detach().clone(), y.detach().clone()] + [b.detach().clone() for b in m.buffers()] + \
        [torch.zeros(()) if p.grad is None else p.grad.detach().clone() for p in m.parameters()]


def _equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("max_k", [8, None], ids=["k8", "all"])
@pytest.mark.parametrize("hid", [64, 20])
@pytest.mark.parametrize("variant", ["gine", "alchemy"])
def test_counter_mode_equals_injected_masks(variant, hid, max_k):
    from signnet_basisnet_amd import synth
    host = _host(variant)
    d = synth.batch_to(host, DEV)
    target = torch.randn(host.num_graphs, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    for path in ("stages", "per-op", "value"):
        mc, mg = _model(variant, hid, max_k, "counter"), _model(variant, hid, max_k, "generator")
        mc.train_stages = mg.train_stages = path == "stages"
        rng = torch.cuda.get_rng_state(DEV)
        got = _train_step(mc, d, target, grad=path != "value")
        assert torch.equal(torch.cuda.get_rng_state(DEV), rng), "a counter-mode train step moved torch's device generator"
        mg._attn_masks = _restated_masks(mg, host, STEP + 1)
        want = _train_step(mg, d, target, grad=path != "value")
        assert _equal(got, want), f"{variant} hid {hid} max_k {max_k} {path}: counter mode differs from the injected restated masks"
        # explicit masks win in counter mode too
        mc.seed_dropout(SEED, STEP + 7)
        mc._attn_masks = mg._attn_masks
        mc.load_state_dict(_model(variant, hid, max_k).state_dict())
        assert _equal(_train_step(mc, d, target, grad=path != "value"), want)


@pytest.mark.parametrize("variant,hid", [("gine", 64), ("alchemy", 20)])
def test_repeats_and_non_interference(variant, hid):
    from signnet_basisnet_amd import synth
    host = _host(variant)
    d = synth.batch_to(host, DEV)
    target = torch.randn(host.num_graphs, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    fresh = _model(variant, hid, 8)
    keys, nbuf = list(fresh.state_dict().keys()), len(list(fresh.buffers()))
    a, b = _model(variant, hid, 8, "counter"), _model(variant, hid, 8, "counter")
    ra, rb = _train_step(a, d, target), _train_step(b, d, target)
    assert _equal(ra, rb)                                            # the same (seed, step): identical
    b.load_state_dict(fresh.state_dict())
    rb2 = _train_step(b, d, target)                                  # the same weights and buffers, the next step: other masks
    assert not torch.equal(rb2[0], ra[0])
    b.load_state_dict(fresh.state_dict())
    assert _equal(_train_step(b.seed_dropout(SEED, STEP), d, target), ra)
    # no new state_dict key, no new buffer; the state is a plain attribute
    assert list(a.state_dict().keys()) == keys and len(list(a.buffers())) == nbuf
    assert not any("dropout" in k or "_sn_" in k for k in keys)
    assert all(n.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked") for n, _ in a.named_buffers())
    # eval reads none of it
    a.load_state_dict(fresh.state_dict())
    y_gen, y_cnt = fresh.eval()(d), a.eval()(d)
    assert torch.equal(y_gen, y_cnt)
    with pytest.raises(ValueError, match="attn_dropout_source"):
        a.attn_dropout_source = "philox"
    assert a._dropout_active() and not fresh._dropout_active()
    a.attn_dropout = 0.0
    assert not a._dropout_active()


@pytest.mark.parametrize("variant,hid", [("gine", 64), ("alchemy", 20)])
def test_graphed_step_replays_the_eager_counter_steps(variant, hid):
    """The criterion of tests/test_training_gpu.py::test_graphed_step_replays_the_eager_training_step_bit_for_bit: losses, parameters
    and buffers bit for bit — with no mask drawn, kept or copied outside the graph."""
    from signnet_basisnet_amd import optim, synth
    from signnet_basisnet_amd.train_graph import GraphedStep
    host = _host(variant)
    target = torch.randn(host.num_graphs, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    m1 = _model(variant, hid, 8, "counter")
    o1 = optim.FlatAdam(m1.parameters(), lr=2e-3)
    d = synth.batch_to(host, DEV)
    eager = []
    for _ in range(3):
        o1.zero_grad()
        loss = (m1(d) - target).abs().mean()
        loss.backward()
        o1.step()
        eager.append(loss.item())
    del loss
    m2 = _model(variant, hid, 8, "counter")
    o2 = optim.FlatAdam(m2.parameters(), lr=2e-3)
    rng = torch.cuda.get_rng_state(DEV)
    gs = GraphedStep(m2, o2, synth.batch_to(host, DEV), target.clone())
    assert gs._masks is None and gs._draw is None
    assert not any(torch.is_tensor(v) and v.dim() == 4 for v in vars(gs).values())
    graphed = [gs.step().item() for _ in range(3)]
    gs.check()
    assert graphed == eager, (graphed, eager)
    assert len(set(graphed)) == 3
    assert torch.equal(o1.flat_p, o2.flat_p)
    for b1, b2 in zip(m1.buffers(), m2.buffers()):
        assert torch.equal(b1, b2)
    assert torch.equal(m1.dropout_state(DEV).t, m2.dropout_state(DEV).t)          # both at (seed, step + 3)
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng)


def _bucket_model(variant, hid, max_k):
    from signnet_basisnet_amd import optim
    m = _model(variant, hid, max_k, "counter", p=0.1)
    return m, optim.FlatAdam(m.parameters(), lr=1e-3)


@pytest.mark.parametrize("max_k,K_cap", [(8, 8), (None, 24)], ids=["k8", "all"])
def test_padded_step_equals_the_eager_step_with_dropout_on(max_k, K_cap):
    """tests/test_bucketed_step_gpu.py switches the attention dropout off for this comparison (padded masks were other draws); with the
    counter source the padded step draws the unpadded step's masks: the same bounds hold at attn_dropout = 0.1."""
    from signnet_basisnet_amd import synth
    host = _host("gine", graphs=8)
    assert max(host.sizes) <= 20
    N, E, S = host.batch.numel(), host.edge_index.shape[1], host.eigen_vectors.numel()
    d = synth.batch_to(host, DEV)
    target = torch.randn(host.num_graphs, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    m1, o1 = _bucket_model("gine", 64, max_k)
    eager, ge, be = TB._eager(m1, o1, [d] * 3, [target] * 3)
    m2, o2 = _bucket_model("gine", 64, max_k)
    s, padded, gp, bp = TB._bucketed(m2, o2, [d] * 3, [target] * 3, bucket=(N + 37, E + 50, S + 100, K_cap))
    assert s.captures == 1 and s.hits == 2
    assert all(c._masks is None for c in s._lru.values())
    for a, b in zip(eager, padded):
        assert abs(a - b) <= 1e-6 * abs(a), (eager, padded)
    assert len(set(eager)) == 3
    TB._close_grads(ge[0], gp[0])
    TB._close_state(m1, m2, o1, o2, be, bp, 3)
    # another bucket serving the same batch: the same masks, the same loss
    m3, o3 = _bucket_model("gine", 64, max_k)
    _, other, g3, _ = TB._bucketed(m3, o3, [d], [target], bucket=(N + 101, E + 7, S + 500, K_cap + (0 if max_k else 8)))
    assert abs(other[0] - padded[0]) <= 1e-6 * abs(padded[0]), (other, padded)
    TB._close_grads(gp[0], g3[0])


@pytest.mark.parametrize("max_k", [8, None], ids=["k8", "all"])
def test_steps_from_the_store_draw_the_masks_of_steps_on_host_collated_batches(max_k):
    """BucketedStep.step_from in counter mode with the dropout on: the criterion of tests/test_store_gpu.py (which runs at p = 0) —
    losses, parameters and buffers bit for bit against step() on the host-collated batch."""
    import store_cases as SC
    from signnet_basisnet_amd import optim, synth
    from signnet_basisnet_amd.data import GraphStore
    from signnet_basisnet_amd.train_graph import BucketedStep
    samples, y = SC.pool("zinc")
    store = GraphStore.from_samples(samples, DEV, y=y[:, :1])
    lists = [[0, 2, 1], [3, 3, 1, 0], [2, 5]]
    bucket = store.covering_bucket(lists, dict(N=16, E=32, S=256, K=8), max_k)
    steps = []
    for _ in range(2):
        m = _model("gine", 32, max_k, "counter")
        steps.append((m, BucketedStep(m, optim.FlatAdam(m.parameters(), lr=1e-3), max_graphs=8)))
    (m1, s1), (m2, s2) = steps
    la, lb = [], []
    for idx in lists:
        la.append(s1.step_from(store, idx, bucket=bucket).clone())
        host = synth.batch_to(SC.host_collate(samples, idx, y[:, :1]), DEV)
        lb.append(s2.step(host, host.y, bucket=bucket).clone())
    s1.check()
    s2.check()
    assert s1.captures == s2.captures == 1 and all(c._masks is None for c in s1._lru.values())
    for a, b in zip(la, lb):
        assert torch.equal(a, b), (la, lb)
    assert torch.equal(s1.optimizer.flat_p, s2.optimizer.flat_p)
    for (n, p), (_, q) in zip(m1.named_buffers(), m2.named_buffers()):
        assert torch.equal(p, q), n
    assert torch.equal(m1.dropout_state(DEV).t, m2.dropout_state(DEV).t)
