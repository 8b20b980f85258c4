"""-m gpu: train_graph.BucketedStep — batches of any shape padded into capacity buckets, one capture per bucket.  The padded step
equals the eager step on the unpadded batch (losses, gradients, BatchNorm running statistics, Adam's parameters), the padding content
cannot change a bit of it, a shuffled sequence of shapes follows the eager loop, the all-eigenvector mode and the Alchemy variant are
covered, and an embedding index out of range in a valid row still raises."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(variant="gine", max_k=8, seed=7, lr=1e-3):
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(seed)
    if variant == "gine":
        m = SignNetGNN(None, None, 32, 1, 3, 2, variant="gine", max_k=max_k)
    else:
        m = SignNetGNN(6, 4, 32, 1, 3, 2, variant="alchemy", max_k=max_k)
    m = m.to(DEV).train()
    m.attn_dropout = 0.0          # padded masks are other draws: comparisons with the eager step run without dropout
    return m, optim.FlatAdam(m.parameters(), lr=lr)


def _grads(m):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}


def _buffers(m):
    return [b.detach().clone() for b in m.buffers()]


def _eager(m, o, batches, targets):
    losses, grads, bufs = [], [], []
    for d, t in zip(batches, targets):
        o.zero_grad()
        loss = (m(d) - t).abs().mean()
        loss.backward()
        grads.append(_grads(m))
        bufs.append(_buffers(m))
        o.step()
        losses.append(loss.item())
    return losses, grads, bufs


def _bucketed(m, o, batches, targets, bucket=None, max_graphs=16, **kw):
    from signnet_basisnet_amd.train_graph import BucketedStep
    s = BucketedStep(m, o, max_graphs=max_graphs, **kw)
    losses, grads, bufs = [], [], []
    for d, t in zip(batches, targets):
        losses.append(s.step(d, t, bucket=bucket).item())
        grads.append(_grads(m))
        bufs.append(_buffers(m))
    torch.cuda.synchronize()
    return s, losses, grads, bufs


def _close_grads(ga, gb):
    gmax = max(g.abs().max().item() for g in ga.values() if g is not None)
    for n in ga:
        a, b = ga[n], gb[n]
        if a is None or b is None:
            assert (a is None or a.abs().max().item() == 0) and (b is None or b.abs().max().item() == 0), n
            continue
        e = (a - b).abs().max().item()
        assert e <= 1e-5 * gmax + 1e-6, f"{n}: {e:.3e} (gmax {gmax:.3e})"


def _close_buffers(m, b1, b2, atol):
    for (n, _), x1, x2 in zip(m.named_buffers(), b1, b2):
        if x1.dtype == torch.int64:
            assert torch.equal(x1, x2), n                                   # num_batches_tracked
        else:
            e = (x1 - x2).abs().max().item()
            assert e <= 1e-5 * x1.abs().max().item() + atol, f"{n}: {e:.3e}"


def _close_state(m1, m2, o1, o2, b1, b2, steps, lr=1e-3):
    # step 1: the running statistics of the same batch statistics
    _close_buffers(m1, b1[0], b2[0], 1e-6)
    # Adam turns the rounding noise of a mathematically-zero gradient (a bias in front of a batch-statistics BatchNorm) into a step
    # of +-lr, which moves that BatchNorm's running mean by momentum x the step: after `steps` steps the parameters agree to rounding
    # except there, within a few steps' worth, and so do the running statistics
    _close_buffers(m1, b1[-1], b2[-1], 2 * lr * steps)
    d = (o1.flat_p - o2.flat_p).abs()
    assert d.max().item() <= 2 * lr * steps + 1e-6
    assert (d > 1e-5).float().mean().item() <= 0.02


def _check_padded_equals_eager(variant, max_k, host, bucket):
    from signnet_basisnet_amd import synth
    B = host.num_graphs
    target = torch.randn(B, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    d = synth.batch_to(host, DEV)
    m1, o1 = _model(variant, max_k)
    eager, ge, be = _eager(m1, o1, [d] * 3, [target] * 3)
    m2, o2 = _model(variant, max_k)
    s, padded, gp, bp = _bucketed(m2, o2, [d] * 3, [target] * 3, bucket=bucket)
    assert s.captures == 1 and s.hits == 2
    for a, b in zip(eager, padded):
        assert abs(a - b) <= 1e-6 * abs(a), (eager, padded)
    _close_grads(ge[0], gp[0])
    _close_state(m1, m2, o1, o2, be, bp, 3)
    return s


def test_padded_step_equals_the_eager_step():
    from signnet_basisnet_amd import synth
    host = synth.make_batch(12, seed=5)
    N, E = host.batch.numel(), host.edge_index.shape[1]
    s = _check_padded_equals_eager("gine", 8, host, (N + 37, E + 50, host.eigen_vectors.numel() + 100, 8))
    assert s.B_cap == 17


def test_all_eigenvector_padded_step_equals_the_eager_step():
    """max_k=None (the reference's default: every eigenvector, K = the largest graph) with K_cap above the largest graph — GraphedStep
    refuses this mode."""
    from signnet_basisnet_amd import synth
    host = synth.make_batch(12, seed=5)
    N, E = host.batch.numel(), host.edge_index.shape[1]
    assert max(host.sizes) < 40
    _check_padded_equals_eager("gine", None, host, (N + 37, E + 50, host.eigen_vectors.numel() + 100, 40))


def test_alchemy_padded_step_equals_the_eager_step():
    from signnet_basisnet_amd import synth
    host = synth.make_batch(12, seed=5, features="alchemy")
    N, E = host.batch.numel(), host.edge_index.shape[1]
    _check_padded_equals_eager("alchemy", 8, host, (N + 37, E + 50, host.eigen_vectors.numel() + 100, 8))


@pytest.mark.parametrize("variant", ["gine", "alchemy"])
def test_padding_content_is_invisible(monkeypatch, variant):
    """Zero padding vs random padding content (valid ids, random eigen data, random features and targets): bit-identical losses,
    gradients and buffers — padded rows are excluded from every statistic and every dW / d gamma / d beta / eps sum."""
    from signnet_basisnet_amd import ops, synth
    host = synth.make_batch(12, seed=5, features="zinc" if variant == "gine" else "alchemy")
    N, E, B, S = host.batch.numel(), host.edge_index.shape[1], host.num_graphs, host.eigen_vectors.numel()
    bucket = (N + 37, E + 50, S + 100, 8)
    d = synth.batch_to(host, DEV)
    target = torch.randn(B, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
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
        out.eigen_values[N:] = torch.rand(out.eigen_values[N:].shape, generator=g, device=DEV) * 3
        out.eigen_vectors[S:] = torch.randn(out.eigen_vectors[S:].shape, generator=g, device=DEV)
        out.target[B:] = torch.randn(out.target[B:].shape, generator=g, device=DEV)
        return r

    runs = []
    for noisy in (False, True):
        if noisy:
            monkeypatch.setattr(ops, "bucket_pack", noisy_pack)
        m, o = _model(variant, 8)
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


def test_variable_shapes_follow_the_eager_loop():
    """Eight batches of different shapes (128 graphs, one ragged batch of 100) through ONE BucketedStep: a capture per distinct
    bucket, replays for the rest, the eager loop's loss trajectory."""
    from signnet_basisnet_amd import synth
    hosts = [synth.make_batch(128 if seed != 2 else 100, seed=seed) for seed in range(1, 9)]      # (the ragged batch second: 28 empty graphs)
    batches = [synth.batch_to(h, DEV) for h in hosts]
    targets = [torch.randn(h.num_graphs, 1, generator=torch.Generator().manual_seed(h.num_graphs + i)).to(DEV)
               for i, h in enumerate(hosts)]
    # (a small learning rate: Adam turns the rounding noise of mathematically-zero gradient entries into +-lr steps, which the
    # later losses of an 8-step trajectory would otherwise carry at the 1e-5 level)
    m1, o1 = _model("gine", 8, lr=1e-4)
    eager, _, _ = _eager(m1, o1, batches, targets)
    m2, o2 = _model("gine", 8, lr=1e-4)
    s, padded, _, _ = _bucketed(m2, o2, batches, targets, max_graphs=128, max_captures=8, granule=dict(N=256, E=512, S=8192))
    distinct = {s.bucket_of(d) for d in batches}
    assert len(distinct) >= 2
    assert s.captures == len(distinct) and s.hits == len(batches) - len(distinct)
    assert set(s.buckets) == distinct
    for a, b in zip(eager, padded):
        assert abs(a - b) <= 1e-5 * abs(a), (eager, padded)
    d = (o1.flat_p - o2.flat_p).abs()
    assert d.max().item() <= 2e-4 * len(batches) and (d > 1e-5).float().mean().item() <= 0.02


def test_lru_eviction_recaptures_and_keeps_training():
    from signnet_basisnet_amd import synth
    hosts = [synth.make_batch(12, seed=s) for s in (1, 2, 1)]
    m, o = _model("gine", 8)
    target = torch.randn(12, 1, generator=torch.Generator().manual_seed(1)).to(DEV)
    from signnet_basisnet_amd.train_graph import BucketedStep
    s = BucketedStep(m, o, max_graphs=12, max_captures=1, granule=dict(N=8, E=8, S=8))
    assert len({s.bucket_of(h) for h in hosts}) == 2
    losses = [s.step(synth.batch_to(h, DEV), target).item() for h in hosts]
    assert s.captures == 3 and s.hits == 0 and len(s.buckets) == 1
    assert all(torch.isfinite(torch.tensor(losses)))


def test_embedding_index_out_of_range_in_a_valid_row_raises():
    from signnet_basisnet_amd import synth
    from signnet_basisnet_amd.train_graph import BucketedStep
    m, o = _model("gine", 8)
    s = BucketedStep(m, o, max_graphs=16)
    host = synth.make_batch(12, seed=5)
    target = torch.randn(12, 1, generator=torch.Generator().manual_seed(2)).to(DEV)
    s.step(synth.batch_to(host, DEV), target)
    s.check()                                  # padding ids are valid: nothing raised
    bad = synth.make_batch(12, seed=5)
    bad.x[3, 0] = 1000
    s.step(synth.batch_to(bad, DEV), target)   # the same bucket: a replay
    assert s.hits == 1
    with pytest.raises(IndexError):
        s.check()
