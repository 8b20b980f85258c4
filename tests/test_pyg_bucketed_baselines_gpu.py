"""-m gpu: train_graph.BucketedStep for the baselines of the two PyG trees — pyg.GNN (variant='gine'), pyg_gnn_types.GNN for every
gnn_type, dropout_models.GNN and pyg_baselines.NetGINE.  The idiom and the bounds of tests/test_bucketed_step_gpu.py: the padded step
equals the eager step on the unpadded batch (loss 1e-6 relative, gradients 1e-5 * gmax + 1e-6, buffers and Adam's parameters through
_close_state), in adverse buckets too; the padding content cannot change a bit; the two new launches alone (the operator pair without
self loops, SimplifiedPNAConv's masked edge-row BatchNorm) against what the eager step builds / a float64 evaluation; dropout, shuffled
shapes, the store path, the deferred IndexError; and SignNetGNN's bucketed step records the launches it recorded before."""
import collections
import functools
import types

import pytest
import torch

import gnn_type_cases as C
import parity_util as PU
from parity_util import attributed, close
from test_bucketed_step_gpu import _bucketed, _close_grads, _close_state, _eager

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TYPES = ("GINEConv", "GINConv", "GCNConv", "GATConv", "SimplifiedPNAConv")
NETS = TYPES + ("NetGINE",)


def _model(kind, pooling="add", seed=7, lr=1e-3, dropout=0):
    from signnet_basisnet_amd import dropout_models, optim, pyg_baselines, pyg_gnn_types
    torch.manual_seed(seed)
    if kind == "NetGINE":
        m = pyg_baselines.NetGINE(16)
    elif dropout:
        m = dropout_models.GNN(None, None, 16, 1, 2, kind, dropout=dropout, pooling=pooling)
    else:
        m = pyg_gnn_types.GNN(None, None, 16, 1, 2, kind, pooling=pooling)
    m = m.to(DEV).train()
    return m, optim.FlatAdam(m.parameters(), lr=lr)


def _strip(host):
    """The batch as a loader of these models delivers it: no eigen fields."""
    return types.SimpleNamespace(**{k: v for k, v in vars(host).items() if not k.startswith("eigen")})


@functools.lru_cache(maxsize=None)
def _batch(kind, graphs=12, seed=5):
    """(device batch without eigen data, target): computed once per feature kind, shared, never modified."""
    from signnet_basisnet_amd import synth
    alchemy = kind == "NetGINE"
    host = _strip(synth.make_batch(graphs, seed=seed, features="alchemy" if alchemy else "zinc"))
    target = torch.randn(graphs, 12 if alchemy else 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    return synth.batch_to(host, DEV), target


def _check(kind, pooling, bucket_of, max_graphs=16, steps=3):
    d, target = _batch(kind)
    N, E = d.batch.numel(), d.edge_index.shape[1]
    m1, o1 = _model(kind, pooling)
    eager, ge, be = _eager(m1, o1, [d] * steps, [target] * steps)
    m2, o2 = _model(kind, pooling)
    s, padded, gp, bp = _bucketed(m2, o2, [d] * steps, [target] * steps, bucket=bucket_of(N, E), max_graphs=max_graphs)
    s.check()
    assert s.captures == 1 and s.hits == steps - 1
    print(f"{kind}/{pooling}: eager {eager} padded {padded}")
    for a, b in zip(eager, padded):
        assert abs(a - b) <= 1e-6 * abs(a), (eager, padded)
    _close_grads(ge[0], gp[0])
    _close_state(m1, m2, o1, o2, be, bp, steps)
    return s


CASES = [(k, "add") for k in NETS] + [(k, "mean") for k in ("GINEConv", "GCNConv", "SimplifiedPNAConv")]


@pytest.mark.parametrize("kind,pooling", CASES)
def test_padded_step_equals_the_eager_step(kind, pooling):
    s = _check(kind, pooling, lambda N, E: (N + 37, E + 50, 1, 1))
    assert s.B_cap == 17 and s.plain


def test_the_plain_gine_net_of_pyg_is_admitted_too():
    """pyg.GNN(variant='gine') itself (what train/zinc.py builds for the default gnn_type), granule rounding, no eigen fields."""
    from signnet_basisnet_amd import optim, pyg
    from signnet_basisnet_amd.train_graph import BucketedStep
    d, target = _batch("GINEConv")

    def build():
        torch.manual_seed(3)
        m = pyg.GNN(None, None, 16, 1, 2, "gine").to(DEV).train()
        return m, optim.FlatAdam(m.parameters(), lr=1e-3)

    m1, o1 = build()
    eager, _, _ = _eager(m1, o1, [d] * 2, [target] * 2)
    m2, o2 = build()
    s = BucketedStep(m2, o2, max_graphs=16)
    padded = [s.step(d, target).item() for _ in range(2)]
    assert s.bucket_of(d)[2:] == (1, 1) and s.captures == 1 and s.hits == 1
    for a, b in zip(eager, padded):
        assert abs(a - b) <= 1e-6 * abs(a), (eager, padded)


ADVERSE = {
    "one_padding_node": (lambda N, E: (N + 1, E + 300, 1, 1), 16),       # every padding edge on ONE node: in-degree 300
    "large_spare_graph": (lambda N, E: (N + 260, E + 50, 1, 1), 16),     # the spare graph has more nodes than size_embedder has rows
    "empty_graphs": (lambda N, E: (N + 37, E + 50, 1, 1), 16),           # 12 graphs, max_graphs 16: graphs 12..15 are empty
}


@pytest.mark.parametrize("bucket", sorted(ADVERSE))
@pytest.mark.parametrize("kind,pooling", [("GATConv", "add"), ("SimplifiedPNAConv", "add"), ("GINEConv", "mean")])
def test_adverse_buckets(kind, pooling, bucket):
    of, mg = ADVERSE[bucket]
    _check(kind, pooling, of, max_graphs=mg, steps=2)


@pytest.mark.parametrize("kind", NETS)
def test_padding_content_is_invisible(monkeypatch, kind):
    """Zero padding vs random padding content (random features, valid ids, random targets): bit-identical losses, gradients, buffers
    and parameters."""
    from signnet_basisnet_amd import ops
    d, target = _batch(kind)
    N, E, B = d.batch.numel(), d.edge_index.shape[1], d.num_graphs
    bucket = (N + 37, E + 50, 1, 1)
    pack = ops.bucket_pack
    g = torch.Generator(device=DEV)

    def noisy_pack(data, tgt, out):
        r = pack(data, tgt, out)
        g.manual_seed(int(out.counts.sum().item()))
        if out.x.dtype == torch.int64:
            out.x[N:] = torch.randint(0, 28, out.x[N:].shape, generator=g, device=DEV)
            out.edge_attr[E:] = torch.randint(0, 4, out.edge_attr[E:].shape, generator=g, device=DEV)
        else:
            out.x[N:] = torch.rand(out.x[N:].shape, generator=g, device=DEV) * 5
            out.edge_attr[E:] = torch.rand(out.edge_attr[E:].shape, generator=g, device=DEV) * 5
        out.target[B:] = torch.randn(out.target[B:].shape, generator=g, device=DEV)
        return r

    runs = []
    for noisy in (False, True):
        if noisy:
            monkeypatch.setattr(ops, "bucket_pack", noisy_pack)
        m, o = _model(kind)
        s, losses, grads, _ = _bucketed(m, o, [d] * 2, [target] * 2, bucket=bucket)
        runs.append((losses, grads, [b.clone() for b in m.buffers()], o.flat_p.clone()))
    (l0, g0, b0, p0), (l1, g1, b1, p1) = runs
    assert l0 == l1
    for n in g0[0]:
        for k in range(2):
            assert (g0[k][n] is None) == (g1[k][n] is None), n
            assert g0[k][n] is None or torch.equal(g0[k][n], g1[k][n]), n
    for a, b in zip(b0, b1):
        assert torch.equal(a, b)
    assert torch.equal(p0, p1)


# ----------------------------------------------------------------------------- the two new launches alone
def _padded(d, target, N_cap, E_cap, B_cap=17):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import Bucket, PaddedBatch
    pad = PaddedBatch(Bucket(N_cap, E_cap, 1, 1), B_cap, d, target, DEV)
    ops.bucket_pack(d, target, pad)
    return pad


@functools.lru_cache(maxsize=None)
def _odd_batch():
    """A 12-graph batch with two input self loops, a duplicated edge, an isolated node and a shuffled edge list."""
    from signnet_basisnet_amd import synth
    host = _strip(synth.make_batch(12, seed=5))
    N = host.batch.numel()
    ei = host.edge_index
    extra = torch.tensor([[3, 40, int(ei[0, 7])], [3, 40, int(ei[1, 7])]])          # loops on nodes 3 and 40, edge 7 once more
    ei = torch.cat([ei, extra], 1)
    perm = torch.randperm(ei.shape[1], generator=torch.Generator().manual_seed(4))
    host.edge_index = ei[:, perm].contiguous()
    host.edge_attr = torch.cat([host.edge_attr, torch.ones(3, dtype=torch.long)])[perm].contiguous()
    host.x = torch.cat([host.x, torch.zeros(1, 1, dtype=torch.long)])                # node N: no edge at all, in the last graph
    host.batch = torch.cat([host.batch, host.batch[-1:]])
    host.num_nodes = N + 1
    return synth.batch_to(host, DEV), torch.zeros(12, 1, device=DEV)


@pytest.mark.parametrize("dN,dE", [(1, 300), (37, 50)])
def test_operator_pair_without_self_loops_equals_the_eager_one(dN, dE):
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.pyg_gnn_types import _gat_operator
    d, target = _odd_batch()
    N, E = d.batch.numel(), d.edge_index.shape[1]
    want = _gat_operator(d, N)
    assert want.nnz == E - 2
    pad = _padded(d, target, N + dN, E + dE)
    plan = ops.build_plan(pad.batch, pad.edge_index, pad.B_cap, 0)
    rplan = ops.build_plan(pad.batch, pad.edge_index.flip(0).contiguous(), pad.B_cap, 0)
    a, b = ops.csr_drop_loops(plan, rplan), ops.csr_drop_loops(plan, rplan)
    torch.cuda.synchronize()
    assert plan.check()[0] == 0
    for got, again, ref in ((a, b, want), (a.t, b.t, want.t)):
        assert got.N == N + dN and got.nnz == E + dE                                  # capacities
        assert torch.equal(got.rowptr, again.rowptr) and torch.equal(got.col, again.col)      # identical bytes on a second call
        assert torch.equal(got.rowptr[:N + 1], ref.rowptr)
        assert torch.equal(got.col[:ref.nnz], ref.col)
        assert bool((got.rowptr[N:] == ref.nnz).all())                                # padding rows are empty
        assert not bool(got.col[ref.nnz:].any())


@pytest.mark.parametrize("Cc", [48, 51])
def test_masked_spna_statistics_and_adjoint_against_float64(Cc):
    """C = 48: the 16-byte path; C = 51: one channel per thread.  The valid rows against the float32 / float64 restatements of
    tests/gnn_type_cases.py on the UNPADDED batch, with the rules tests/test_gnn_types_gpu.py applies to the unmasked launches."""
    from signnet_basisnet_amd import ops
    d, target = _batch("GINEConv")
    N, E = d.batch.numel(), d.edge_index.shape[1]
    dN, dE = 5, 23
    pad = _padded(d, target, N + dN, E + dE)
    plan = ops.build_plan(pad.batch, pad.edge_index, pad.B_cap, 0)
    rplan = ops.build_plan(pad.batch, pad.edge_index.flip(0).contiguous(), pad.B_cap, 0)
    assert ops.spna_vector_path(Cc, (Cc,) * 4, (0,)) == (Cc == 48)
    g = torch.Generator().manual_seed(Cc)
    A, B_, dr = (torch.randn(N + dN, Cc, generator=g) for _ in range(3))               # (padding rows: random content too)
    Q = torch.randn(E + dE, Cc, generator=g)
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g)
    rm, rv = torch.randn(Cc, generator=g), torch.rand(Cc, generator=g) + 0.5
    bn = torch.nn.BatchNorm1d(Cc).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    a, b, q, drd = (t.to(DEV) for t in (A, B_, Q, dr))
    state, count = ops.spna_stats(a, b, q, plan, bn, pad.node_valid, pad.counts)
    r = ops.spna_mean(a, b, q, plan, state[3], state[4])
    dA, dB, dQ, dgamma, dbeta = ops.spna_bwd(a, b, q, plan, rplan, drd, state=state, gamma=bn.weight.detach(),
                                             node_valid=pad.node_valid, counts=pad.counts)
    torch.cuda.synchronize()
    assert float(count) == E
    ei = d.edge_index.cpu()
    ref = {}
    for dtype in (torch.float32, torch.float64):
        t = lambda v: v.to(dtype)          # noqa: E731
        ops_ = (t(A[:N]), t(B_[:N]), t(Q[:E]), ei)
        st = C.spna_stats_ref(*ops_, t(gamma), t(beta), t(rm), t(rv))
        rr, gr = C.spna_train_ref(*ops_, t(gamma), t(beta), t(dr[:N]))
        ref[dtype] = (st, rr, gr)
    (s32, r32, g32), (s64, r64, g64) = ref[torch.float32], ref[torch.float64]
    for i, k in enumerate(("mean", "var", "rstd", "scale", "shift")):
        print(f"C={Cc} {k}: |hip - f64| {PU.relerr(state[i], getattr(s64, k)):.2e}  |cpu32 - f64| {PU.relerr(getattr(s32, k), getattr(s64, k)):.2e}")
        close(state[i], getattr(s32, k), f"C={Cc}: {k}", ref64=getattr(s64, k))
    for k, tns in (("running_mean", bn.running_mean), ("running_var", bn.running_var)):
        close(tns, getattr(s32, k), f"C={Cc}: {k}", ref64=getattr(s64, k))
    close(r[:N], r32, f"C={Cc}: r", ref64=r64)
    got = dict(dA=dA[:N], dB=dB[:N], dQ=dQ[:E], dgamma=dgamma, dbeta=dbeta)
    for k, v in got.items():
        print(f"C={Cc} {k}: |hip - f64| {PU.relerr(v, g64[k]):.2e}  |cpu32 - f64| {PU.relerr(g32[k], g64[k]):.2e}")
    for k, v in got.items():
        attributed(v, g32[k], g64[k], f"C={Cc}: {k}")
    assert not bool(dA[N:].any()) and not bool(dB[N:].any()) and not bool(dQ[E:].any())       # padding rows: exactly zero


# ----------------------------------------------------------------------------- dropout, shuffled shapes, the store, errors
def test_dropout_draws_the_unpadded_steps_masks():
    d, target = _batch("GINConv")
    N, E = d.batch.numel(), d.edge_index.shape[1]
    m1, o1 = _model("GINConv", dropout=0.1)
    m1.seed_dropout(11, 0)
    eager, _, _ = _eager(m1, o1, [d] * 3, [target] * 3)
    m2, o2 = _model("GINConv", dropout=0.1)
    m2.seed_dropout(11, 0)
    s, padded, _, _ = _bucketed(m2, o2, [d] * 3, [target] * 3, bucket=(N + 37, E + 50, 1, 1))
    assert s.captures == 1 and s.hits == 2
    m0, o0 = _model("GINConv")
    plain, _, _ = _eager(m0, o0, [d], [target])
    assert abs(plain[0] - eager[0]) > 1e-4 * abs(eager[0])          # (the masks are drawn at all)
    for a, b in zip(eager, padded):
        assert abs(a - b) <= 1e-6 * abs(a), (eager, padded)


SHUFFLED = [(9, 1), (12, 2), (10, 3), (11, 4), (12, 5), (9, 6), (10, 7), (11, 8)]      # (graphs, seed)


def test_shuffled_shapes_follow_the_eager_loop():
    """Eight batches of 9 to 12 graphs through granule N = 64, E = 128: at most three captures, the eager loop's losses (the bound and
    the small learning rate of test_variable_shapes_follow_the_eager_loop in tests/test_bucketed_step_gpu.py)."""
    bt = [_batch("GINEConv", g, sd) for g, sd in SHUFFLED]
    batches, targets = [b for b, _ in bt], [t for _, t in bt]
    m1, o1 = _model("GINEConv", lr=1e-4)
    eager, _, _ = _eager(m1, o1, batches, targets)
    m2, o2 = _model("GINEConv", lr=1e-4)
    s, padded, _, _ = _bucketed(m2, o2, batches, targets, max_graphs=12, max_captures=4, granule=dict(N=64, E=128))
    distinct = {s.bucket_of(d) for d in batches}
    print("buckets", sorted(distinct))
    assert 2 <= len(distinct) == s.captures <= 3 and s.hits == len(batches) - s.captures
    for a, b in zip(eager, padded):
        assert abs(a - b) <= 1e-5 * abs(a), (eager, padded)


def test_steps_from_a_store_equal_steps_on_its_collated_batches():
    """A GraphStore of 40 graphs: its batches carry eigen data, which step_from gathers and the model ignores."""
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.data import GraphStore
    from signnet_basisnet_amd.train_graph import BucketedStep
    samples = []
    for i in range(40):
        h = synth.make_batch(1, seed=100 + i)
        h.x = h.x.reshape(-1, 1)
        samples.append(h)
    y = torch.randn(40, 1, generator=torch.Generator().manual_seed(9))
    store = GraphStore.from_samples(samples, DEV, y=y)
    order = torch.randperm(40, generator=torch.Generator().manual_seed(1)).tolist()
    lists = [order[i:i + 10] for i in range(0, 40, 10)]
    m1, o1 = _model("GINEConv")
    m2, o2 = _model("GINEConv")
    s1, s2 = BucketedStep(m1, o1, max_graphs=12), BucketedStep(m2, o2, max_graphs=12)
    la, lb = [], []
    for idx in lists:
        la.append(s1.step_from(store, idx).item())
        c = store.collate(idx)
        lb.append(s2.step(c, c.y).item())
    s1.check()
    s2.check()
    assert la == lb, (la, lb)
    assert torch.equal(o1.flat_p, o2.flat_p)


def test_an_index_out_of_range_raises_from_a_valid_row_only(monkeypatch):
    from signnet_basisnet_amd import ops, synth
    from signnet_basisnet_amd.train_graph import BucketedStep
    d, target = _batch("GINEConv")
    N = d.batch.numel()
    m, o = _model("GINEConv")
    s = BucketedStep(m, o, max_graphs=16)
    pack = ops.bucket_pack

    def bad_padding(data, tgt, out):
        r = pack(data, tgt, out)
        out.x[N:] = 1000                           # the same id in padding rows only
        return r

    monkeypatch.setattr(ops, "bucket_pack", bad_padding)
    s.step(d, target)
    s.check()                                      # nothing raised
    monkeypatch.setattr(ops, "bucket_pack", pack)
    bad = synth.batch_to(types.SimpleNamespace(**vars(d)), DEV)
    bad.x = d.x.clone()
    bad.x[3, 0] = 1000
    s.step(bad, target)                            # the same bucket: a replay
    assert s.hits == 1
    with pytest.raises(IndexError):
        s.check()


# ----------------------------------------------------------------------------- SignNetGNN's bucketed step is the one it was
class _Count:
    """Stands where ops.KernelTimer keeps its `only` set: counts every launch name the timer is asked about and records none (no
    event is placed, so the count also runs through the warm-up and the capture of a BucketedStep)."""

    def __init__(self):
        self.n = collections.Counter()

    def __contains__(self, name):
        self.n[name] += 1
        return False


# the launch names and counts of SignNetGNN's first bucketed step (two warm-up runs and the capture), recorded on the commit before the
# baseline models were admitted
SIGNNET_LAUNCHES = {
    "sn_batch_plan": 3, "sn_batch_plan_padded": 3, "sn_bucket_pack": 1, "sn_embedding_sum_bwd_layers_f32": 3,
    "sn_embedding_sum_f32": 3, "sn_embedding_sum_layers_f32": 3, "sn_gin_aggregate_add_f32": 6, "sn_gin_aggregate_f32": 9,
    "sn_gine_aggregate_bwd_add_f32": 6, "sn_gine_aggregate_f32": 6, "sn_linear_wgrad_f32": 6, "sn_masked_affine_f32": 3,
    "sn_masked_l1_bwd_f32": 3, "sn_masked_l1_f32": 3, "sn_masked_layernorm_bwd_f32": 6, "sn_masked_layernorm_f32": 6,
    "sn_masked_linear_f32": 12, "sn_pack_eig_f32": 3, "sn_segment_pool_f32": 3, "sn_set_attention_bwd_f32": 3,
    "sn_set_attention_f32": 3, "sn_slot_sum_f32": 3, "sn_train_bn_apply_f32": 18, "sn_train_bn_bwd_sums_f32": 18,
    "sn_train_bn_finish_f32": 30, "sn_train_dot_jobs_f64": 3, "sn_train_linear_bwd_f32": 48, "sn_train_linear_f32": 48,
    "sn_train_reduce_jobs_f32": 3, "sn_train_scalar_mlp_apply_f32": 3, "sn_train_scalar_mlp_bwd_f32": 3,
    "sn_train_scalar_mlp_stats_f32": 6,
}


def test_signnet_gnn_records_the_launches_it_recorded_before():
    from signnet_basisnet_amd import ops, synth
    from test_bucketed_step_gpu import _model as signnet_model
    host = synth.make_batch(12, seed=5)
    N, E = host.batch.numel(), host.edge_index.shape[1]
    d = synth.batch_to(host, DEV)
    target = torch.randn(12, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    m, o = signnet_model("gine", 8)
    from signnet_basisnet_amd.train_graph import BucketedStep
    s = BucketedStep(m, o, max_graphs=16)
    timer = ops.KernelTimer()
    timer.only = _Count()
    with timer:
        s.step(d, target, bucket=(N + 37, E + 50, host.eigen_vectors.numel() + 100, 8))
    torch.cuda.synchronize()
    got = dict(timer.only.n)
    print("launches", sorted(got.items()))
    assert not timer.spans
    assert got == SIGNNET_LAUNCHES
