"""-m gpu: the baseline PE rows of the DGL tree — sn_lap_pe_transform_f32 (handle_lap's network-free branches) against the reference's
own outputs and a torch restatement, the five nets at pe_init 'no_pe' against the reference's outputs and the float oracles, GatedGCN
behind sign_flip / abs_val / canonical end to end, and the captured / recorded paths (DGLBucketedStep, GraphedDGLForward) for the new
methods.  Fixtures: tests/golden/baseline_*.npz (tests/golden/make_baseline_pe.py)."""
import types

import pytest
import torch

import golden_util as G
import parity_util as PU
import store_cases as SC
from parity_util import close
from test_lap_baselines_cpu import fixture_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EXCLUDE = 1e-4          # margin below which a canonical (graph, column) pair is a rounding coin toss in the reference (see the CPU test)


# ----------------------------------------------------------------------------- the op
def _graph_ptr(sizes, extra=()):
    return torch.tensor([0] + list(sizes) + list(extra), dtype=torch.int64).cumsum(0).to(torch.int32).to(DEV)


def _canonical(p, sizes):
    """handle_lap's canonical branch (train_ZINC_graph_regression.py:26-43) restated on the host: per graph and column, times -1 if
    there are fewer non-negative than negative entries OR their sum is smaller than the negatives' absolute sum (both strict)."""
    out, r = p.clone(), 0
    for n in sizes:
        blk = p[r:r + n]
        flip = ((blk >= 0).sum(0) < (blk < 0).sum(0)) | (torch.where(blk >= 0, blk, 0 * blk).sum(0) < torch.where(blk < 0, -blk, 0 * blk).sum(0))
        out[r:r + n] = blk * torch.where(flip, -1.0, 1.0)
        r += n
    return out


def _assert_canonical(out, ref, p, sizes, margin, what):
    """Every pair whose margin is at least EXCLUDE equals the reference; an excluded pair is +column or -column exactly."""
    r = 0
    for b, n in enumerate(sizes):
        for c in range(p.shape[1]):
            got, col = out[r:r + n, c], p[r:r + n, c]
            if margin[b, c] >= EXCLUDE:
                assert torch.equal(got, ref[r:r + n, c]), (what, b, c)
            else:
                assert torch.equal(got, col) or torch.equal(got, -col), (what, b, c)
        r += n


@pytest.mark.parametrize("in_place", [False, True])
def test_transform_equals_the_reference_handle_lap(in_place):
    from signnet_basisnet_amd import ops
    fx = G.load("baseline_handle_lap_k8")
    p, sizes = fx.inp["pos_enc"], [int(s) for s in fx.inp["sizes"]]
    gp = _graph_ptr(sizes)

    def run(mode, **kw):
        src = p.to(DEV).clone()
        out = ops.lap_pe_transform(src, mode, out=src if in_place else None, **kw)
        assert (out is src) == in_place and (in_place or torch.equal(src.cpu(), p))          # out of place: the input is untouched
        return out.cpu()

    assert torch.equal(run("abs_val"), fx.out["abs_val"])
    assert torch.equal(run("none"), fx.out["none"]) and torch.equal(fx.out["none"], p)
    assert torch.equal(run("sign_flip", u=fx.inp["u"].to(DEV)), fx.out["sign_flip"])
    assert torch.equal(run(ops.LAP_ABS_VAL), fx.out["abs_val"])                              # (the SN_LAP_* integer)
    _assert_canonical(run("canonical", graph_ptr=gp), fx.out["canonical"], p, sizes, fx.meta["margin"], "fixture batch")


TIE_SIZES = [1, 1, 2, 3, 5, 9, 12, 17, 20, 33, 64, 70, 300]          # sizes {1, 2, 3, 5, 9, 12, 17, 20, 33, 64, 70, 300}; two one-node graphs
# column 0 of these graphs (position in TIE_SIZES) is written by hand: (entries, flips?)
TIE_CASES = {
    0: ([-0.5], True),                                                    # a one-node graph with a negative entry
    1: ([0.0], False),                                                    # a one-node graph with 0
    2: ([0.5, -0.5], False),                                              # count equality with sum equality
    3: ([0.75, -0.25, -0.25], True),                                      # count only: n_pos < n_neg, s_pos > s_neg
    4: ([0.25, 0.25, 0.25, -1.0, -0.5], True),                            # sum only
    5: ([0.125, 0.125] + [-1.0] * 7, True),                               # both
    6: ([0.5] * 6 + [-0.25] * 6, False),                                  # neither (count equality, s_pos > s_neg)
    7: ([0.0] * 17, False),                                               # an all-zero column
}


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("K", [1, 8, 37, 65])
def test_canonical_exact_ties_and_every_decision_branch(K, in_place):
    """Entries are multiples of 2^-8 in [-1, 1]: every sum is exact in any order, so the restatement has one answer for every pair."""
    from signnet_basisnet_amd import ops
    gen = torch.Generator().manual_seed(100 + K)
    N, tail, guard = sum(TIE_SIZES), 7, 16
    p = torch.randint(-256, 257, (N + tail, K), generator=gen).float() / 256.0
    starts = torch.tensor([0] + TIE_SIZES).cumsum(0).tolist()
    for b, (vals, _) in TIE_CASES.items():
        assert len(vals) == TIE_SIZES[b]
        p[starts[b]:starts[b + 1], 0] = torch.tensor(vals)
    want = _canonical(p[:N], TIE_SIZES)
    for b, (vals, flips) in TIE_CASES.items():                              # the restatement takes the branch the case was built for
        assert torch.equal(want[starts[b]:starts[b + 1], 0], torch.tensor(vals) * (-1.0 if flips else 1.0)), b
    buf = torch.full((guard + (N + tail) * K + guard,), 12345.0, device=DEV)
    out = buf[guard:guard + (N + tail) * K].view(N + tail, K)
    src = p.to(DEV)
    if in_place:
        out.copy_(src)
        src = out
    got = ops.lap_pe_transform(src, "canonical", graph_ptr=_graph_ptr(TIE_SIZES), out=out)
    torch.cuda.synchronize()
    assert torch.equal(got[:N].cpu(), want)
    assert torch.equal(got[N:].cpu(), p[N:])                                # rows beyond graph_ptr[B] come back unchanged
    assert bool((buf[:guard] == 12345.0).all()) and bool((buf[-guard:] == 12345.0).all())


def test_canonical_signs_do_not_depend_on_the_batch():
    from signnet_basisnet_amd import ops
    sizes = [1, 2, 3, 5, 9, 12, 17, 20, 33, 64, 70]
    N = sum(sizes)
    p = torch.randn(N, 8, generator=torch.Generator().manual_seed(0))
    margin = torch.full((len(sizes), 8), float("inf"), dtype=torch.float64)
    r = 0
    for b, n in enumerate(sizes):
        blk = p[r:r + n].double()
        r += n
        s_pos, s_neg = torch.where(blk >= 0, blk, 0 * blk).sum(0), torch.where(blk < 0, -blk, 0 * blk).sum(0)
        decide = ((blk >= 0).sum(0) >= (blk < 0).sum(0)) & (torch.maximum(s_pos, s_neg) > 0)
        margin[b, decide] = ((s_pos - s_neg).abs() / torch.maximum(s_pos, s_neg))[decide]
    print("smallest margin", float(margin.min()))
    assert float(margin.min()) >= 1e-3                                      # (2.2e-2 on this draw: no pair is excluded)
    pd = p.to(DEV)
    batched = ops.lap_pe_transform(pd, "canonical", graph_ptr=_graph_ptr(sizes))
    assert torch.equal(batched.cpu(), _canonical(p, sizes))
    r = 0
    for n in sizes:                                                         # each graph alone
        alone = ops.lap_pe_transform(pd[r:r + n].clone(), "canonical", graph_ptr=_graph_ptr([n]))
        assert torch.equal(alone, batched[r:r + n]), n
        r += n
    big = torch.zeros(N + 50, 8, device=DEV)                                # a capacity buffer: zero padding rows in one extra graph
    big[:N] = pd
    padded = ops.lap_pe_transform(big, "canonical", graph_ptr=_graph_ptr(sizes, extra=[50]))
    assert torch.equal(padded[:N], batched) and not bool(padded[N:].any())


# ----------------------------------------------------------------------------- the five nets at pe_init 'no_pe'
NETS = ["gin", "gatedgcn", "gat", "pna", "transformer"]
# train-mode tolerance of the sibling test of each net in tests/test_dgl_basisnet_gpu.py (test_dgl_*_base_net_golden)
TRAIN_TOL = {"gin": (5e-4, 5e-5), "gatedgcn": (1e-3, 1e-4), "gat": (1e-3, 1e-4), "pna": (1e-3, 1e-4), "transformer": (1e-3, 1e-4)}
# the coefficient of the sibling gradient test (test_dgl_{pna,gat,transformer}_net_parameter_gradients_match_oracle_autograd; GIN and
# GatedGCN have theirs in tests/test_training_gpu.py: 2e-3 and 3e-3 of the largest entry)
GRAD_TOL = {"gin": 2e-3, "gatedgcn": 3e-3, "gat": 1e-4, "pna": 5e-3, "transformer": 2e-3}


def _inputs(fx):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    ei = fx.inp["edge_index"]
    g = DS.Graph(ei[0].to(DEV), ei[1].to(DEV), fx.inp["sizes"])
    sn = fx.inp["snorm_n"].to(DEV) if "snorm_n" in fx.inp else None
    return g, fx.inp["x"].squeeze(-1).to(DEV), fx.inp["edge_attr"].to(DEV), sn


def _loaded(net, row="nope", mode="eval"):
    fx, m = fixture_net(net, row, DEV)
    m.load_state_dict(fx.sd, strict=True)
    return fx, m.to(DEV).train(mode == "train")


def _oracle(net, fx, sd, training):
    """The unchanged oracle of the lap_pe net with a zero embedding_p and p = 0 (GatedGCN / Transformer: its pe_aggregate 'add' path):
    the reference's NoPE forward."""
    from oracle import dgl_nets as ON
    ei, sizes, h, e = fx.inp["edge_index"], fx.inp["sizes"], fx.inp["x"].squeeze(-1), fx.inp["edge_attr"]
    hidden, L, k = (int(v) for v in fx.meta["hidden_L_k"])
    dt = sd["embedding_h.weight"].dtype
    sd = dict(sd, **{"embedding_p.weight": torch.zeros(hidden, k, dtype=dt), "embedding_p.bias": torch.zeros(hidden, dtype=dt)})
    p = torch.zeros(h.shape[0], k, dtype=dt)
    if net == "gin":
        return ON.gin_net(sd, ei[0], ei[1], sizes, h, p, L, "mean", training=training)
    if net == "gatedgcn":
        return ON.gatedgcn_net(sd, ei[0], ei[1], sizes, h, p, e, L, pe_aggregate="add", readout="mean", training=training)
    if net == "gat":
        return ON.gat_net(sd, ei[0], ei[1], sizes, h, p, L, int(fx.meta["n_heads"]), "mean")
    if net == "pna":
        return ON.pna_net(sd, ei[0], ei[1], sizes, h, p, e, fx.inp["snorm_n"].to(dt), L, int(fx.meta["towers"]), float(fx.meta["avg_d"][2]),
                          "sum", training=training)
    return ON.transformer_net(sd, ei[0], ei[1], sizes, h, p, e, L, int(fx.meta["n_heads"]), "add", "sum", training=training)


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("net", NETS)
def test_nope_net_equals_the_reference(net, mode):
    fx, m = _loaded(net, mode=mode)
    g, h, e, sn = _inputs(fx)
    with torch.no_grad():
        y, _ = m(g, h, None, e, sn)
    if mode == "eval":
        with torch.no_grad():
            y64 = _oracle(net, fx, PU.to_f64(fx.sd), False)
        close(y, fx.out["eval/y"], f"{net} NoPE scores", ref64=y64)
        if "eval/h_last" in fx.out and hasattr(m, "_h_last"):
            m.fused_stages = False                                          # (the one-launch kernels keep no node features)
            with torch.no_grad():
                m(g, h, None, e, sn)
            close(m._h_last, fx.out["eval/h_last"], f"{net} NoPE node features")
    else:
        rtol, atol = TRAIN_TOL[net]
        torch.testing.assert_close(y.cpu(), fx.out["train/y"], rtol=rtol, atol=atol)
    # p is not read at pe_init 'no_pe' (as in the reference): anything may be passed
    with torch.no_grad():
        y2, _ = _loaded(net, mode=mode)[1](g, h, torch.full((h.shape[0], 3), float("nan"), device=DEV), e, sn)
    assert torch.equal(y2, y)


def _grads(m):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}


@pytest.mark.parametrize("net", ["gin", "gat", "pna"])
def test_nope_net_is_the_lap_pe_net_with_a_zero_embedding_bit_for_bit(net):
    """GIN, GAT and PNA add the PE: h = embedding_h(h) + embedding_p(p).  With a zero embedding_p and p = 0 that sum adds an exact zero,
    so outputs (eval, train) and every shared parameter's gradient of the lap_pe net equal the NoPE net's bit for bit."""
    import test_lap_baselines_cpu as C
    from signnet_basisnet_amd import dgl_nets
    fx = G.load(f"baseline_{net}_nope")
    hidden, L, k = (int(v) for v in fx.meta["hidden_L_k"])
    g, h, e, sn = _inputs(fx)
    p0 = torch.zeros(h.shape[0], k, device=DEV)
    cot = torch.randn(len(fx.inp["sizes"]), 1, generator=torch.Generator().manual_seed(5)).to(DEV)

    def run(lap):
        cfg, sd = _params_of(net, fx), dict(fx.sd)
        if lap:
            cfg.update(pe_init="lap_pe", lap_method="none", pe_aggregate="add")
            sd.update({"embedding_p.weight": torch.zeros(hidden, k), "embedding_p.bias": torch.zeros(hidden)})
        else:
            cfg.update(pe_init="no_pe", lap_method="none", pe_aggregate="none")
        m = getattr(dgl_nets, C._CLS[net])(cfg)
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV)
        outs = {}
        with torch.no_grad():
            outs["eval"] = m.eval()(g, h, p0 if lap else None, e, sn)[0].clone()
            outs["train"] = m.train()(g, h, p0 if lap else None, e, sn)[0].clone()
        y, _ = m(g, h, p0 if lap else None, e, sn)
        assert y.requires_grad
        (y * cot).sum().backward()
        outs["grad_y"] = y.detach().clone()
        return outs, _grads(m)

    (o0, g0), (o1, g1) = run(False), run(True)
    for key in o0:
        assert torch.equal(o0[key], o1[key]), key
    assert set(g1) - set(g0) == {"embedding_p.weight", "embedding_p.bias"}
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None) and (g0[n] is None or torch.equal(g0[n], g1[n])), n


def _params_of(net, fx):
    """The constructor dictionary fixture_net builds (read back from a NoPE net of the fixture)."""
    import test_lap_baselines_cpu as C
    hidden, L, k = (int(v) for v in fx.meta["hidden_L_k"])
    p = dict(C._COMMON, hidden_dim=hidden, out_dim=hidden, L=L, pos_enc_dim=k, readout=C._READOUT[net], device=DEV)
    if net in ("gat", "transformer"):
        p["n_heads"] = int(fx.meta["n_heads"])
    if net == "transformer":
        p.update(full_graph=False, layer_norm=True)
    if net == "pna":
        a = fx.meta["avg_d"]
        p.update(graph_norm=True, aggregators="mean max min std", scalers="identity amplification attenuation",
                 towers=int(fx.meta["towers"]), divide_input_first=True, divide_input_last=True, edge_dim=int(fx.meta["edge_dim"]),
                 pretrans_layers=1, posttrans_layers=1, gru=False, avg_d=dict(lin=float(a[0]), exp=float(a[1]), log=float(a[2])))
    return p


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("net", NETS)
def test_nope_parameter_gradients_match_the_oracle(net, dtype):
    """Train mode with gradients enabled: every parameter gradient of the NoPE net against torch.autograd over the unchanged oracle
    (zero embedding_p, p = 0) in float64 and in float32, under the sibling gradient tests' comparison (_check_param_grads)."""
    from test_dgl_basisnet_gpu import _check_param_grads
    fx, m = _loaded(net, mode="train")
    g, h, e, sn = _inputs(fx)
    sd = {k: (v.to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k else v) for k, v in fx.sd.items()}
    yo = _oracle(net, fx, sd, True)
    cot = torch.randn(yo.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (yo * cot.to(dtype)).sum().backward()
    y, _ = m(g, h, None, e, sn)
    assert y.requires_grad
    torch.testing.assert_close(y.detach().cpu().double(), yo.detach().double(), rtol=2e-3, atol=2e-4)
    (y * cot.float().to(DEV)).sum().backward()
    _check_param_grads(m, sd, f"{net} NoPE ({dtype})", tol=GRAD_TOL[net])


def _spans(fn):
    from signnet_basisnet_amd import ops
    fn()
    rec = ops.KernelTimer()
    with rec:
        y = fn()
    return y, [n for n, _, _ in rec.spans]


@pytest.mark.parametrize("net,kernel", [("gin", "sn_gin_net_fused_f32"), ("gatedgcn", "sn_gatedgcn_fused_f32"),
                                        ("transformer", "sn_transformer_net_fused_f32")])
def test_nope_eval_takes_the_one_launch_path_and_matches_the_layer_path(net, kernel):
    """Where the lap_pe net's eval forward is one launch (the GIN net, the GatedGCN stack, the hidden-64 Transformer) the NoPE net's
    is too — the GIN / Transformer kernel adds a projection of the PE itself and gets a ZERO projection (packed on the host) of a
    one-column zero encoding — and gives what the layer path gives."""
    from signnet_basisnet_amd import dgl_nets
    fx = G.load(f"baseline_{net}_nope")
    if net == "transformer":                                                # the one-launch kernel is written for hidden 64 = 8 heads of 8
        torch.manual_seed(3)
        m = dgl_nets.TransformerNet(dict(_params_of(net, fx), hidden_dim=64, out_dim=64, n_heads=8, pe_init="no_pe", lap_method="none",
                                         pe_aggregate="none"))
        PU.bn_randomize(m, 4)
        m = m.to(DEV).eval()
    else:
        m = _loaded(net)[1]
    g, h, e, sn = _inputs(fx)

    def run():
        with torch.no_grad():
            return m(g, h, None, e, sn)[0].clone()
    y, names = _spans(run)
    assert names.count(kernel) == 1, names
    if net != "gatedgcn":                                                   # (GatedGCN: embeddings in front of the stack, as at lap_pe)
        assert names == [kernel] or (net == "transformer" and len(names) == 3), names      # + the edge embedding and its E projection
    m.check_last()
    m.fused_stages = False
    y_layers, names_l = _spans(run)
    assert kernel not in names_l
    assert torch.isfinite(y).all()
    close(y, y_layers, f"{net} NoPE one launch vs layer path")


# ----------------------------------------------------------------------------- GatedGCN behind handle_lap, end to end
@pytest.mark.parametrize("method", ["sign_flip", "abs_val", "canonical"])
def test_gatedgcn_lappe_rows_end_to_end(method):
    """dgl_nets.handle_lap then the net against the reference's handle_lap and net: p exact (canonical: the excluded-pair rule), y at
    the tolerances of test_dgl_gatedgcn_base_net_golden.  If an excluded (coin-toss) pair of the canonical row comes out with the other
    sign, the scores are those of another encoding: the net is then run on the reference's p, so that y is still held to the reference."""
    from signnet_basisnet_amd import dgl_nets
    for mode in ("eval", "train"):
        fx, m = _loaded("gatedgcn", method, mode)
        g, h, e, sn = _inputs(fx)
        pe = fx.inp["pos_enc"].to(DEV)
        seed = int(fx.meta["flip_seed"])
        if method == "sign_flip":
            torch.manual_seed(seed)
            assert torch.equal(torch.rand(pe.shape[1]), fx.inp["u"])        # host draws under the recorded seed: the stored uniforms
            torch.manual_seed(seed)
        with torch.no_grad():
            p = dgl_nets.handle_lap(m, pe, g, DEV)
            assert torch.equal(pe.cpu(), fx.inp["pos_enc"])                 # (out of place)
            if method == "canonical":
                sizes = [int(s) for s in fx.inp["sizes"]]
                _assert_canonical(p.cpu(), fx.out["p"], fx.inp["pos_enc"], sizes, fx.meta["margin"], "gatedgcn canonical")
                if not torch.equal(p.cpu(), fx.out["p"]):
                    p = fx.out["p"].to(DEV)
            else:
                assert torch.equal(p.cpu(), fx.out["p"])
            y, _ = m(g, h, p, e, sn)
        if mode == "eval":
            close(y, fx.out["eval/y"], f"GatedGCN {method} scores")
        else:
            torch.testing.assert_close(y.cpu(), fx.out["train/y"], rtol=1e-3, atol=1e-4)
    if method == "sign_flip":                                               # u= : a caller's uniforms, host or device
        u = fx.inp["u"]
        with torch.no_grad():
            assert torch.equal(dgl_nets.handle_lap(m, pe, g, u=u).cpu(), fx.out["p"])
            assert torch.equal(dgl_nets.handle_lap(m, pe, g, u=u.to(DEV)).cpu(), fx.out["p"])


# ----------------------------------------------------------------------------- the captured step
STEP_CASES = ["sign_flip", "abs_val", "canonical", "none", "no_pe"]        # GatedGCN with each new method; PNA at pe_init 'no_pe'
LISTS = [[0, 1, 2, 6], [3, 5], [2, 9, 0, 8], [4], [1, 6, 7], [3, 5]]       # shuffled small batches of the store_cases pool
GRANULE = dict(N=32, E=64)
LR, SEED = 1e-4, 7


@pytest.fixture(scope="module")
def pool():
    return SC.pool("zinc")


def _step_net(case, seed=3):
    """A small net of the fixtures' shapes with seeded random weights (train mode) + its FlatAdam."""
    from signnet_basisnet_amd import optim
    net, row = ("pna", "nope") if case == "no_pe" else ("gatedgcn", "nope" if case == "none" else case)
    fx = G.load(f"baseline_{net}_{row}")
    cfg = _params_of(net, fx)
    cfg.update(dict(pe_init="no_pe", lap_method="none", pe_aggregate="none") if case == "no_pe" else
               dict(pe_init="lap_pe", lap_method=case, pe_aggregate="add"))
    torch.manual_seed(seed)
    from signnet_basisnet_amd import dgl_nets
    m = getattr(dgl_nets, "PNANet" if net == "pna" else "GatedGCNNet")(cfg).to(DEV).train()
    return m, optim.FlatAdam(m.parameters(), lr=LR)


def _samples(pool, net):
    samples, y = pool
    return SC.dgl_samples(samples, y, net.pos_enc_dim, True, net.__class__.__name__ == "PNANet")


def _dev_batch(ds, idx):
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    g, h, p, e, sn, t = SC.dgl_host_collate(ds, idx)
    src, dst = g.edges()
    return types.SimpleNamespace(g=Graph(src.to(DEV), dst.to(DEV), g.batch_num_nodes()), h=h.to(DEV), p=p.to(DEV), e=e.to(DEV),
                                 sn=None if sn is None else sn.to(DEV), t=t.to(DEV))


def _eager_loop(net, o, batches):
    from signnet_basisnet_amd import dgl_nets
    torch.manual_seed(SEED)
    losses = []
    for b in batches:
        o.zero_grad()
        pe = dgl_nets.handle_lap(net, b.p, b.g, DEV) if net.pe_init == "lap_pe" else None      # (:73-76)
        y, _ = net(b.g, b.h, pe, b.e, b.sn)
        loss = net.loss(y, b.t)
        loss.backward()
        o.step()
        losses.append(loss.item())
    return losses


def _noisy(batches, case):
    """The eager loop's sensitivity probe of tests/test_dgl_bucketed_step_gpu.py: a 1e-6 relative perturbation of the continuous input
    — pos_enc; for the NoPE net (PNA), which does not read it, snorm_n."""
    from test_dgl_bucketed_step_gpu import NOISE
    gen = torch.Generator().manual_seed(11)
    out = []
    for b in batches:
        c = types.SimpleNamespace(**vars(b))
        if case == "no_pe":
            c.sn = b.sn * (1 + NOISE * torch.randn(b.sn.shape, generator=gen).to(DEV))
        else:
            c.p = b.p * (1 + NOISE * torch.randn(b.p.shape, generator=gen).to(DEV))
        out.append(c)
    return out


def _release(s):
    s.release()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", STEP_CASES)
def test_captured_step_follows_the_eager_loop(pool, case):
    """DGLBucketedStep over shuffled small batches (two or more buckets, an LRU hit) against the eager loop on the unpadded batches:
    the comparison and bounds of tests/test_dgl_bucketed_step_gpu.py::test_variable_shapes_follow_the_eager_loop.  sign_flip: the same
    torch.manual_seed on both sides gives the same flips (flip_rng 'host'), and every replay reads fresh uniforms."""
    from test_dgl_bucketed_step_gpu import _close_losses, _close_params
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    m1, o1 = _step_net(case)
    ds = _samples(pool, m1)
    batches = [_dev_batch(ds, idx) for idx in LISTS]
    eager = _eager_loop(m1, o1, batches)
    mn, on = _step_net(case)
    noisy = _eager_loop(mn, on, _noisy(batches, case))
    m2, o2 = _step_net(case)
    s = DGLBucketedStep(m2, o2, max_graphs=8, granule=GRANULE)
    torch.manual_seed(SEED)
    padded, us = [], []
    for b in batches:
        padded.append(s.step(b.g, b.h, None if case == "no_pe" else b.p, b.e, b.sn, b.t).item())
        if case == "sign_flip":
            us.append(s._last.u.cpu().clone())
    s.check()
    distinct = {s.bucket_of(b.g, b.h) for b in batches}
    assert len(distinct) >= 2 and s.captures == len(distinct) and s.hits == len(batches) - len(distinct) >= 1
    print(f"{case}: eager {eager}\n noisy {noisy}\n padded {padded}")
    _close_losses(eager, noisy, padded, rel=1e-5)
    _close_params(o1, on, o2, len(batches), LR)
    if case == "sign_flip":
        torch.manual_seed(SEED)
        draws = [torch.rand(m2.pos_enc_dim) for _ in batches]                # the reference's sequence: one torch.rand(k) per step
        for i, (u, d) in enumerate(zip(us, draws)):
            assert torch.equal(u, d), i
        for a, b, da, db in zip(us, us[1:], draws, draws[1:]):               # consecutive replays read different uniforms
            assert torch.equal(a, b) == torch.equal(da, db)
        assert not torch.equal(us[1], us[5])                                 # LISTS[1] == LISTS[5]: two replays of ONE capture
    assert getattr(m2, "_bucket", None) is None
    _release(s)


@pytest.mark.parametrize("case,flip_rng", [(c, "host") for c in STEP_CASES] + [("sign_flip", "device")])
def test_steps_from_the_store_equal_steps_on_host_collated_batches_bit_for_bit(pool, case, flip_rng):
    from signnet_basisnet_amd.data import DGLGraphStore
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    n1, o1 = _step_net(case)
    n2, o2 = _step_net(case)
    ds = _samples(pool, n1)
    if case == "no_pe":                                                      # any store: its pos_enc (another width) is gathered and ignored
        store = DGLGraphStore.from_samples(SC.dgl_samples(*pool, 5, True, True), DEV)
        assert store.K == 5 != n1.pos_enc_dim
    else:
        store = DGLGraphStore.from_samples(ds, DEV)
    bucket = store.covering_bucket(LISTS, GRANULE)
    s1 = DGLBucketedStep(n1, o1, max_graphs=8, flip_rng=flip_rng)
    s2 = DGLBucketedStep(n2, o2, max_graphs=8, flip_rng=flip_rng)
    la, lb = [], []
    for run in ("store", "host"):
        torch.manual_seed(SEED)                                              # (seeds the device generator too: flip_rng 'device')
        for idx in LISTS:
            if run == "store":
                la.append(s1.step_from(store, idx, bucket=bucket).clone())
            else:
                b = _dev_batch(ds, idx)
                lb.append(s2.step(b.g, b.h, None if case == "no_pe" else b.p, b.e, b.sn, b.t, bucket=bucket).clone())
    s1.check()
    s2.check()
    assert s1.captures == s2.captures == 1 and s1.hits == s2.hits == len(LISTS) - 1
    for a, b in zip(la, lb):
        assert torch.equal(a, b), (la, lb)
    assert torch.equal(o1.flat_p, o2.flat_p)
    for (n, p), (_, q) in zip(n1.named_buffers(), n2.named_buffers()):
        assert torch.equal(p, q), n
    if case != "no_pe":
        wrong = DGLGraphStore.from_samples(SC.dgl_samples(*pool, 5, True, False), DEV)
        with pytest.raises(ValueError, match="pos_enc"):
            s1.step_from(wrong, LISTS[0], bucket=bucket)
    _release(s1)
    _release(s2)


@pytest.mark.parametrize("case", STEP_CASES)
def test_padding_content_is_invisible(pool, monkeypatch, case):
    """Zero padding vs random padding content: bit-identical losses, buffers and parameters (the canonical transform may flip the
    spare graph's random columns: they stay padding)."""
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    pack = ops.bucket_pack_dgl
    gen = torch.Generator(device=DEV)

    def noisy_pack(g, h, p, e, snorm_n, target, out):
        N, E, B = pack(g, h, p, e, snorm_n, target, out)
        gen.manual_seed(N + E + B)
        out.h[N:] = torch.randint(0, 28, out.h[N:].shape, generator=gen, device=DEV)
        out.e[E:] = torch.randint(0, 4, out.e[E:].shape, generator=gen, device=DEV)
        out.p[N:] = torch.randn(out.p[N:].shape, generator=gen, device=DEV)
        if out.snorm_n is not None:
            out.snorm_n[N:] = torch.rand(out.snorm_n[N:].shape, generator=gen, device=DEV) + 0.5
        out.target[B:] = torch.randn(out.target[B:].shape, generator=gen, device=DEV)
        return N, E, B

    runs = []
    for noisy in (False, True):
        if noisy:
            monkeypatch.setattr(ops, "bucket_pack_dgl", noisy_pack)
        m, o = _step_net(case)
        ds = _samples(pool, m)
        s = DGLBucketedStep(m, o, max_graphs=8)
        torch.manual_seed(SEED)
        losses = []
        for idx in (LISTS[0], LISTS[2]):
            b = _dev_batch(ds, idx)
            losses.append(s.step(b.g, b.h, None if case == "no_pe" else b.p, b.e, b.sn, b.t, bucket=(96, 192)).item())
        torch.cuda.synchronize()
        runs.append((losses, [x.clone() for x in m.buffers()], o.flat_p.clone()))
        _release(s)
    (l0, b0, p0), (l1, b1, p1) = runs
    assert l0 == l1 and torch.equal(p0, p1)
    for x0, x1 in zip(b0, b1):
        assert torch.equal(x0, x1)


# ----------------------------------------------------------------------------- the recorded eval forward
@pytest.mark.parametrize("case", ["canonical", "no_pe", "sign_flip"])
def test_graphed_dgl_forward_replays_the_eager_forward(case):
    """serving.GraphedDGLForward for a canonical LapPE net and a NoPE net: the replay equals the eager eval forward bit for bit; a second
    batch of the same shape is served through the static buffers.  sign_flip: every call draws fresh uniforms (the reference flips at
    evaluation too), the CPU generator's sequence."""
    from signnet_basisnet_amd import dgl_nets, synth
    from signnet_basisnet_amd.serving import GraphedDGLForward
    from test_serving_gpu import _inputs as serving_inputs, _permuted
    fx = G.load("baseline_gatedgcn_nope" if case != "no_pe" else "baseline_gin_nope")
    net = "gatedgcn" if case != "no_pe" else "gin"
    cfg = _params_of(net, fx)
    cfg.update(dict(pe_init="no_pe", lap_method="none", pe_aggregate="none") if case == "no_pe" else
               dict(pe_init="lap_pe", lap_method=case, pe_aggregate="add"))
    torch.manual_seed(2)
    m = getattr(dgl_nets, "GINNet" if net == "gin" else "GatedGCNNet")(cfg)
    PU.bn_randomize(m, 3)
    m = m.to(DEV).eval()
    k = m.pos_enc_dim
    a = synth.make_batch(24, seed=11)
    b = _permuted(a, list(reversed(range(24))))
    (ga, ha, pa, ea, _), (gb, hb, pb, eb, _) = serving_inputs(a, k), serving_inputs(b, k)
    pa, pb = (None, None) if case == "no_pe" else (pa.squeeze(-1).contiguous(), pb.squeeze(-1).contiguous())

    def eager(g, h, p, e):
        with torch.no_grad():
            q = dgl_nets.handle_lap(m, p, g) if case != "no_pe" else None
            return m(g, h, q, e, None)[0].clone()

    torch.manual_seed(SEED)
    ya, yb, ya2 = eager(ga, ha, pa, ea), eager(gb, hb, pb, eb), eager(ga, ha, pa, ea)
    assert not torch.equal(ya, yb)
    torch.manual_seed(SEED)
    gf = GraphedDGLForward(m, ga, ha, pa, ea, None)                          # (the recording's own draw does not count)
    assert torch.equal(gf().clone(), ya)
    assert torch.equal(gf(gb, hb, pb, eb).clone(), yb)
    assert torch.equal(gf(ga, ha, pa, ea).clone(), ya2)
    if case == "sign_flip":
        assert not torch.equal(ya, ya2)                                      # other flips on the same batch
    gf.check()


# ----------------------------------------------------------------------------- GAT at the baseline configs' width
# GAT_ZINC_NoPE.json / GAT_ZINC_LapPE.json: hidden 65 with 4 heads of 65 channels — beyond the 64 the GATConv kernels took.  Head widths
# 65 .. 128 run two channels per lane (forward) and 128 channel registers per thread (adjoint); widths <= 64 run the kernels as before.
@pytest.mark.parametrize("heads,C", [(4, 65), (2, 100), (1, 128)])
def test_gat_aggregate_wide_heads_vs_fp64(heads, C):
    from test_dgl_basisnet_gpu import test_gat_aggregate_vs_fp64
    test_gat_aggregate_vs_fp64(heads, C)


@pytest.mark.parametrize("heads,C,relu", [(4, 65, True), (1, 128, False)])
def test_gat_aggregate_wide_heads_adjoint_vs_fp64_autograd(heads, C, relu):
    from test_dgl_basisnet_gpu import test_gat_aggregate_adjoint_vs_fp64_autograd
    test_gat_aggregate_adjoint_vs_fp64_autograd(heads, C, relu)


def test_gat_head_width_beyond_128_is_refused():
    from signnet_basisnet_amd import dgl_nets, ops
    with pytest.raises(ValueError, match="head width"):
        dgl_nets.GATConv(16, 129, 2)
    L = ops.lib()
    assert L.sn_gat_aggregate_f32(None, None, None, None, 4, 2, 129, 0.2, 1, None, None, None, None, None) == -1


@pytest.mark.parametrize("row", ["gat_nope", "gat_lappe"])
def test_gat_at_the_shipped_baseline_width_vs_oracle(row):
    """The shipped GAT baseline shape (hidden 65, 4 heads; 3 layers here) in eval and with gradients against the float64 oracle."""
    from oracle import dgl_nets as ON
    from signnet_basisnet_amd import dgl_configs, dgl_deepsigns as DS, dgl_nets, synth
    from test_dgl_basisnet_gpu import _check_param_grads
    cls, cfg = dgl_configs.net_params(row, DEV)
    cfg.update(L=3)
    torch.manual_seed(4)
    m = getattr(dgl_nets, cls)(cfg)
    with torch.no_grad():
        for n_, p_ in m.named_parameters():
            if n_.startswith("layers.") and n_.endswith(".bias") and n_.count(".") == 2:       # GATConv.bias (zero-initialised)
                p_.copy_(0.1 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(6)))
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    lap = cfg["pe_init"] == "lap_pe"
    data = synth.make_batch(6, seed=21, sizes=[5, 9, 12, 7, 3, 20])
    pe = synth.dgl_pos_enc(data, 8) if lap else torch.zeros(data.num_nodes, 8)
    if not lap:
        sd.update({"embedding_p.weight": torch.zeros(65, 8), "embedding_p.bias": torch.zeros(65)})
    ei, h = data.edge_index, data.x.squeeze(-1)
    g = DS.Graph(ei[0].to(DEV), ei[1].to(DEV), data.sizes)
    m = m.to(DEV)
    with torch.no_grad():
        y64 = ON.gat_net(PU.to_f64(sd), ei[0], ei[1], data.sizes, h, pe.double(), 3, 4, "mean")
        y = m.eval()(g, h.to(DEV), pe.to(DEV) if lap else None, data.edge_attr.to(DEV))[0]
    close(y, y64, f"{row} eval scores")
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    yo = ON.gat_net(sd64, ei[0], ei[1], data.sizes, h, pe.double(), 3, 4, "mean")
    cot = torch.randn(yo.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (yo * cot).sum().backward()
    yt, _ = m.train()(g, h.to(DEV), pe.to(DEV) if lap else None, data.edge_attr.to(DEV))
    (yt * cot.float().to(DEV)).sum().backward()
    _check_param_grads(m, sd64, row, tol=1e-4)
