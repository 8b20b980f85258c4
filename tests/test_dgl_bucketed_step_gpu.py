"""-m gpu: train_graph.DGLBucketedStep — the DGL tree's training loop (train_ZINC_graph_regression.py:54-88) on batches of any shape,
padded into capacity buckets, one capture per bucket.  For every shipped sign-invariant config the padded step follows the eager step
on the unpadded batch (losses, gradients, BatchNorm running statistics, Adam's parameters; see NOISE below for the bounds); the padding
content cannot change a bit of it; the pack kernel writes exactly the padding convention; a shuffled sequence of shapes follows the
eager loop; the deferred host checks raise what the eager step raises; the switch on the net does not outlive the step."""
import types

import pytest
import torch

from signnet_basisnet_amd.dgl_configs import SHIPPED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _net(name, seed=3, lr=1e-3):
    from signnet_basisnet_amd import dgl_configs, dgl_nets, optim
    cls, p = dgl_configs.net_params(name, DEV)
    torch.manual_seed(seed)
    net = getattr(dgl_nets, cls)(p)
    if name.startswith("gat"):
        with torch.no_grad():                               # GATConv's bias is zero-initialised: make it count
            for n_, p_ in net.named_parameters():
                if n_.startswith("layers.") and n_.endswith(".bias") and n_.count(".") == 2:
                    p_.copy_(0.1 * torch.randn(p_.shape, generator=torch.Generator().manual_seed(5)))
    net = net.to(DEV).train()
    return net, optim.FlatAdam(net.parameters(), lr=lr)


def _batch(name, B, seed):
    from signnet_basisnet_amd import dgl_deepsigns as DS
    from signnet_basisnet_amd import synth
    data = synth.make_batch(B, seed=seed)
    k = SHIPPED[name]["pos_enc_dim"]
    src, dst = data.edge_index
    sn = torch.cat([torch.full((n, 1), 1.0 / n) for n in data.sizes]).sqrt()          # PNA's graph_norm input
    return types.SimpleNamespace(
        g=DS.Graph(src.to(DEV), dst.to(DEV), data.sizes), h=data.x.squeeze(-1).to(DEV), p=synth.dgl_pos_enc(data, k).to(DEV),
        e=data.edge_attr.to(DEV), sn=sn.to(DEV) if name.startswith("pna") else None,
        t=torch.randn(B, 1, generator=torch.Generator().manual_seed(seed + 100)).to(DEV),
        N=data.batch.numel(), E=data.edge_index.shape[1], B=B, data=data)


def _grads(m):
    return {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()}


def _buffers(m):
    return [b.detach().clone() for b in m.buffers()]


def _eager_loss(net, b):
    p = net.sign_inv_net(b.g, b.p.unsqueeze(-1)).squeeze(-1)
    y, _ = net(b.g, b.h, p, b.e, b.sn)
    return net.loss(y, b.t)


def _eager(net, o, batches):
    losses, grads, bufs = [], [], []
    for b in batches:
        o.zero_grad()
        loss = _eager_loss(net, b)
        loss.backward()
        grads.append(_grads(net))
        bufs.append(_buffers(net))
        o.step()
        losses.append(loss.item())
    return losses, grads, bufs


def _bucketed(net, o, batches, bucket=None, max_graphs=16, **kw):
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    s = DGLBucketedStep(net, o, max_graphs=max_graphs, **kw)
    losses, grads, bufs = [], [], []
    for b in batches:
        losses.append(s.step(b.g, b.h, b.p, b.e, b.sn, b.t, bucket=bucket).item())
        grads.append(_grads(net))
        bufs.append(_buffers(net))
    torch.cuda.synchronize()
    return s, losses, grads, bufs


def _release(s):
    s.release()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# The DGL sign-invariant nets are ill-conditioned in fp32: the first GIN layer's BatchNorm has channels that the ReLU in front of it
# leaves constant on a batch (variance 0: rstd = 1/sqrt(eps), about 316), which turn the last-bit differences of any other summation
# order — the padded batch has more rows, so its reductions are blocked differently — into visible differences of the encoding and of
# the first layers' gradients.  The eager step moves as much under a 1e-6 relative perturbation of pos_enc.  So beyond the first loss
# (strict), the padded step is held to the eager step within MARGIN times that measured sensitivity — an eager run of an identically
# seeded net on the perturbed batches — plus the absolute floors of tests/test_bucketed_step_gpu.py.  The parity test reports the
# sensitivity per config (`eager_noise`; printed with -s), asserts the constant channels that explain it, and caps it: the bounds
# cannot widen silently if the eager path became noisier.  Measured on the 12-graph batch, 3 steps at lr 1e-4: 3-13 constant channels
# per config; the loss moved by 8.6e-5 (gat) to 2.2e-2 (transformer) relative, the step-1 gradients by 9e-4 (transformer_mask) to
# 7.1e-2 (gin) of the largest one; the padded step stayed within 9.2x of that (losses, pna) and within 1x (gradients).
NOISE = 1e-6
MARGIN = 20.0
LOSS_NOISE_CAP, GRAD_NOISE_CAP = 0.05, 0.15     # (about twice the largest sensitivity measured over the 8 configs)


def _perturbed(batches):
    gen = torch.Generator().manual_seed(11)
    out = []
    for b in batches:
        c = types.SimpleNamespace(**vars(b))
        c.p = b.p * (1 + NOISE * torch.randn(b.p.shape, generator=gen).to(DEV))
        out.append(c)
    return out


def _close_losses(eager, noisy, padded, first=1e-6, rel=1e-6):
    assert abs(eager[0] - padded[0]) <= first * abs(eager[0]), (eager, padded)
    scale = 0.0
    for a, n, c in zip(eager, noisy, padded):
        scale = max(scale, abs(a - n))
        assert abs(a - c) <= rel * abs(a) + MARGIN * scale, (eager, noisy, padded)


def _close_grads(ge, gn, gp):
    gmax = max(g.abs().max().item() for g in ge.values() if g is not None)
    nmax = max((ge[n] - gn[n]).abs().max().item() for n in ge if ge[n] is not None)
    for n in ge:
        a, b = ge[n], gp[n]
        if a is None or b is None:
            assert (a is None or a.abs().max().item() == 0) and (b is None or b.abs().max().item() == 0), n
            continue
        e = (a - b).abs().max().item()
        noise = max((a - gn[n]).abs().max().item(), 0.05 * nmax)
        assert e <= 1e-5 * gmax + 1e-6 + MARGIN * noise, f"{n}: {e:.3e} (gmax {gmax:.3e}, eager noise {noise:.3e})"


def _close_buffers(m, be, bn, bp, atol):
    for (n, _), x1, xn, x2 in zip(m.named_buffers(), be, bn, bp):
        if x1.dtype == torch.int64:
            assert torch.equal(x1, x2), n                                   # num_batches_tracked
        else:
            e = (x1 - x2).abs().max().item()
            noise = (x1 - xn).abs().max().item()
            assert e <= 1e-5 * x1.abs().max().item() + atol + MARGIN * noise, f"{n}: {e:.3e} (eager noise {noise:.3e})"


def _close_params(oe, on, op, steps, lr):
    # Adam moves every parameter by at most ~lr per step, whatever the gradient: two runs differ by at most 2 lr per step
    d, dn = (oe.flat_p - op.flat_p).abs(), (oe.flat_p - on.flat_p).abs()
    assert d.max().item() <= 2 * lr * steps + 1e-6
    assert d.mean().item() <= MARGIN * dn.mean().item() + 1e-7, (d.mean().item(), dn.mean().item())


def _constant_bn_channels(net, b):
    """Channels of the sign-invariant net's first BatchNorm (after Linear(1, hidden) and ReLU, over all N*k slot rows of the eager
    batch) that are constant on this batch: the ReLU keeps every row negative.  Their rstd is 1/sqrt(eps)."""
    from signnet_basisnet_amd import ops
    sn = net.sign_inv_net
    conv = sn.enc.layers[0]
    lin = conv.apply_func.lins[0]
    with torch.no_grad():
        a = ops.gin_aggregate(b.p.contiguous(), sn._plan(b.g, b.N), conv.eps.detach())
        z = torch.relu(a.reshape(-1, 1) * lin.weight.view(1, -1) + lin.bias.view(1, -1))
        return int((z.var(0) == 0).sum())


@pytest.mark.parametrize("name", list(SHIPPED))
def test_padded_step_equals_the_eager_step(name, record_property):
    b = _batch(name, 12, seed=5)
    bucket = (b.N + 37, b.E + 50)
    lr = 1e-4      # (Adam turns rounding noise of near-zero gradient entries into +-lr steps: a small lr keeps 3 steps comparable)
    m1, o1 = _net(name, lr=lr)
    eager, ge, be = _eager(m1, o1, [b] * 3)
    mn, on = _net(name, lr=lr)
    noisy, gn, bn = _eager(mn, on, _perturbed([b] * 3))
    m2, o2 = _net(name, lr=lr)
    s, padded, gp, bp = _bucketed(m2, o2, [b] * 3, bucket=bucket)
    assert s.captures == 1 and s.hits == 2 and s.B_cap == 17
    s.check()
    # the sensitivity the bounds below scale with, measured on this config (reported; see NOISE above)
    gmax = max(g.abs().max().item() for g in ge[0].values() if g is not None)
    loss_noise = max(abs(a - n) / abs(a) for a, n in zip(eager, noisy))
    grad_noise = max((ge[0][n] - gn[0][n]).abs().max().item() for n in ge[0] if ge[0][n] is not None) / gmax
    const = _constant_bn_channels(mn, b)
    record_property("eager_noise", dict(loss=loss_noise, grad=grad_noise, constant_bn_channels=const))
    print(f"NOISE {name}: loss {loss_noise:.2e}  grad {grad_noise:.2e} of gmax  constant first-BN channels {const}  "
          f"padded: loss {max(abs(a - c) / abs(a) for a, c in zip(eager, padded)):.2e}  "
          f"grad {max((ge[0][n] - gp[0][n]).abs().max().item() for n in ge[0] if ge[0][n] is not None) / gmax:.2e}")
    assert const >= 1, "no constant channel in the first BatchNorm: the sensitivity-scaled bounds below are not explained"
    assert loss_noise <= LOSS_NOISE_CAP and grad_noise <= GRAD_NOISE_CAP, (loss_noise, grad_noise)
    _close_losses(eager, noisy, padded)
    _close_grads(ge[0], gn[0], gp[0])
    _close_buffers(m1, be[0], bn[0], bp[0], 1e-6)
    _close_buffers(m1, be[-1], bn[-1], bp[-1], 2 * lr * 3)
    _close_params(o1, on, o2, 3, lr)
    _release(s)


@pytest.mark.parametrize("name", ["gatedgcn", "gatedgcn_mask", "pna", "gat"])
def test_padding_content_is_invisible(monkeypatch, name):
    """Zero padding vs random padding content (valid atom / bond ids, random pos_enc, snorm_n, targets): bit-identical losses,
    gradients, buffers and parameters — padding rows are excluded from every statistic and every parameter gradient, and the
    aggregations never carry them into a valid row."""
    from signnet_basisnet_amd import ops
    b = _batch(name, 12, seed=5)
    N, E, B = b.N, b.E, b.B
    bucket = (N + 37, E + 50)
    pack = ops.bucket_pack_dgl
    gen = torch.Generator(device=DEV)

    def noisy_pack(g, h, p, e, snorm_n, target, out):
        r = pack(g, h, p, e, snorm_n, target, out)
        gen.manual_seed(int(out.counts.sum().item()))
        out.h[N:] = torch.randint(0, 28, out.h[N:].shape, generator=gen, device=DEV)
        out.e[E:] = torch.randint(0, 4, out.e[E:].shape, generator=gen, device=DEV)
        out.p[N:] = torch.randn(out.p[N:].shape, generator=gen, device=DEV)
        if out.snorm_n is not None:
            out.snorm_n[N:] = torch.rand(out.snorm_n[N:].shape, generator=gen, device=DEV) + 0.5
        out.target[B:] = torch.randn(out.target[B:].shape, generator=gen, device=DEV)
        return r

    runs = []
    for noisy in (False, True):
        if noisy:
            monkeypatch.setattr(ops, "bucket_pack_dgl", noisy_pack)
        m, o = _net(name)
        s, losses, grads, _ = _bucketed(m, o, [b] * 2, bucket=bucket)
        runs.append((losses, grads, [x.clone() for x in m.buffers()], o.flat_p.clone()))
        _release(s)
    (l0, g0, b0, p0), (l1, g1, b1, p1) = runs
    assert l0 == l1
    for n in g0[0]:
        for k in range(2):
            assert (g0[k][n] is None) == (g1[k][n] is None), n
            assert g0[k][n] is None or torch.equal(g0[k][n], g1[k][n]), n
    for x0, x1 in zip(b0, b1):
        assert torch.equal(x0, x1)
    assert torch.equal(p0, p1)


@pytest.mark.parametrize("pad_nodes,pad_edges", [(37, 50), (37, 10)])
def test_pack_writes_the_padding_convention(pad_nodes, pad_edges):
    """Every buffer of ops.bucket_pack_dgl equals a torch construction of the convention: valid rows first, padding edge E + i a
    self-loop on padding node N + i % (N_cap - N), zero padding, the padded per-graph node counts, validity, node slots, [N, E, B]."""
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.train_graph import DGLBucket, DGLPaddedBatch
    b = _batch("pna", 12, seed=7)
    N, E, B, K = b.N, b.E, b.B, 8
    Nc, Ec, Bc = N + pad_nodes, E + pad_edges, 17
    out = DGLPaddedBatch(DGLBucket(Nc, Ec), Bc, K, True, True, DEV)
    for t in (out.src, out.dst, out.h, out.e, out.p, out.snorm_n, out.target, out.batch_num_nodes, out.node_valid, out.edge_valid,
              out.graph_valid, out.node_slots, out.counts, out.count_error):
        t.fill_(-7)                                           # every element must be written
    ops.bucket_pack_dgl(b.g, b.h, b.p, b.e, b.sn, b.t, out)
    torch.cuda.synchronize()
    i64 = dict(dtype=torch.int64, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    pad_ep = N + torch.arange(Ec - E, **i64) % (Nc - N)
    src, dst = b.g.edges()
    z = lambda n, *s, dt=torch.float32: torch.zeros(n, *s, dtype=dt, device=DEV)
    want = dict(
        src=torch.cat([src, pad_ep]), dst=torch.cat([dst, pad_ep]), h=torch.cat([b.h, z(Nc - N, dt=torch.int64)]),
        e=torch.cat([b.e, z(Ec - E, dt=torch.int64)]), p=torch.cat([b.p, z(Nc - N, K)]), snorm_n=torch.cat([b.sn, z(Nc - N, 1)]),
        target=torch.cat([b.t, z(Bc - B, 1)]),
        batch_num_nodes=torch.cat([torch.tensor(b.data.sizes, **i64), z(Bc - 1 - B, dt=torch.int64), torch.tensor([Nc - N], **i64)]),
        node_valid=torch.cat([torch.ones(N, **i32), z(Nc - N, dt=torch.int32)]),
        edge_valid=torch.cat([torch.ones(E, **i32), z(Ec - E, dt=torch.int32)]),
        graph_valid=torch.cat([torch.ones(B, **i32), z(Bc - B, dt=torch.int32)]),
        node_slots=torch.cat([torch.full((N,), K, **i32), z(Nc - N, dt=torch.int32)]),
        counts=torch.tensor([N, E, B], **i32), count_error=z(1, dt=torch.int32))
    for k, v in want.items():
        assert torch.equal(getattr(out, k), v), k
    assert int(out.batch_num_nodes.sum()) == Nc


@pytest.mark.parametrize("delta", [1, -1])
def test_node_counts_that_do_not_sum_to_n_stay_in_bounds_and_raise(delta):
    """batch_num_nodes() that does not describe the N feature rows — the eager step's ValueError.  Counts on the device: the pack keeps
    the padded counts at N_cap (one graph holds every node, so the recorded repeat_interleave(..., output_size=N_cap) stays in bounds),
    flags the batch, and check() raises.  Counts on the host: step() raises before any launch."""
    from signnet_basisnet_amd import ops
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    from signnet_basisnet_amd.train_graph import DGLBucket, DGLBucketedStep, DGLPaddedBatch
    msg = "batch_num_nodes does not sum to the number of feature rows"
    b = _batch("gatedgcn", 12, seed=5)
    src, dst = b.g.edges()
    bad_sizes = list(b.data.sizes)
    bad_sizes[3] += delta
    bad_dev = Graph(src, dst, torch.tensor(bad_sizes, device=DEV))
    good_dev = Graph(src, dst, torch.tensor(b.data.sizes, device=DEV))
    bucket = (b.N + 37, b.E + 50)
    out = DGLPaddedBatch(DGLBucket(*bucket), 17, 8, True, False, DEV)
    ops.bucket_pack_dgl(bad_dev, b.h, b.p, b.e, None, b.t, out)
    want = torch.zeros(17, dtype=torch.int64, device=DEV)
    want[-1] = bucket[0]
    assert torch.equal(out.batch_num_nodes, want) and int(out.count_error[0]) == 1
    ops.bucket_pack_dgl(good_dev, b.h, b.p, b.e, None, b.t, out)
    assert int(out.count_error[0]) == 0 and out.batch_num_nodes[:12].tolist() == list(b.data.sizes)
    net, o = _net("gatedgcn")
    s = DGLBucketedStep(net, o, max_graphs=16)
    s.step(good_dev, b.h, b.p, b.e, None, b.t, bucket=bucket)
    s.check()
    loss = s.step(bad_dev, b.h, b.p, b.e, None, b.t, bucket=bucket)         # the same bucket: a replay of the captured step
    assert s.hits == 1 and torch.isfinite(loss).item()
    with pytest.raises(ValueError, match=msg):
        s.check()
    with pytest.raises(ValueError, match=msg):
        s.step(Graph(src, dst, bad_sizes), b.h, b.p, b.e, None, b.t, bucket=bucket)
    assert s.hits == 1 and s.captures == 1
    s.step(good_dev, b.h, b.p, b.e, None, b.t, bucket=bucket)
    s.check()                                                                # the next good batch is clean again
    _release(s)


def test_variable_shapes_follow_the_eager_loop():
    """Eight batches of 128 graphs (one ragged batch of 100) through ONE DGLBucketedStep: a capture per distinct bucket, replays for
    the rest, the eager loop's loss trajectory."""
    name = "gatedgcn"
    batches = [_batch(name, 128 if seed != 2 else 100, seed=seed) for seed in range(1, 9)]
    m1, o1 = _net(name, lr=1e-4)
    eager, _, _ = _eager(m1, o1, batches)
    mn, on = _net(name, lr=1e-4)
    noisy, _, _ = _eager(mn, on, _perturbed(batches))
    m2, o2 = _net(name, lr=1e-4)
    s, padded, _, _ = _bucketed(m2, o2, batches, max_graphs=128, max_captures=8, granule=dict(N=256, E=512))
    distinct = {s.bucket_of(b.g, b.h) for b in batches}
    assert len(distinct) >= 2
    assert s.captures == len(distinct) and s.hits == len(batches) - len(distinct)
    assert set(s.buckets) == distinct
    _close_losses(eager, noisy, padded, rel=1e-5)
    _close_params(o1, on, o2, len(batches), 1e-4)
    _release(s)


def test_atom_id_out_of_range_in_a_valid_row_raises_at_check():
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    net, o = _net("gatedgcn")
    s = DGLBucketedStep(net, o, max_graphs=16)
    b = _batch("gatedgcn", 12, seed=5)
    s.step(b.g, b.h, b.p, b.e, b.sn, b.t)
    s.check()                                  # padding ids are valid: nothing raised
    bad = _batch("gatedgcn", 12, seed=5)
    bad.h[3] = 1000
    s.step(bad.g, bad.h, bad.p, bad.e, bad.sn, bad.t)      # the same bucket: a replay
    assert s.hits == 1
    with pytest.raises(IndexError):
        s.check()
    _release(s)


def test_gat_zero_in_degree_node_in_a_valid_graph_raises_at_check():
    from signnet_basisnet_amd.dgl_deepsigns import Graph
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    net, o = _net("gat")
    s = DGLBucketedStep(net, o, max_graphs=16)
    b = _batch("gat", 12, seed=5)
    bucket = (b.N + 37, b.E + 10)              # 27 padding nodes get no self-loop: padding never trips the check
    s.step(b.g, b.h, b.p, b.e, b.sn, b.t, bucket=bucket)
    s.check()
    src, dst = b.g.edges()
    keep = dst != 5                            # node 5 of graph 0 loses its in-edges
    b.g = Graph(src[keep].contiguous(), dst[keep].contiguous(), b.data.sizes)
    s.step(b.g, b.h, b.p, b.e[keep].contiguous(), b.sn, b.t, bucket=bucket)
    assert s.hits == 1
    with pytest.raises(ValueError, match="0-in-degree nodes"):
        s.check()
    _release(s)


def test_the_switch_does_not_outlive_the_step():
    name = "gatedgcn_mask"
    net, o = _net(name)
    b = _batch(name, 12, seed=5)
    from signnet_basisnet_amd.train_graph import DGLBucketedStep
    s = DGLBucketedStep(net, o, max_graphs=16)
    s.step(b.g, b.h, b.p, b.e, b.sn, b.t)
    torch.cuda.synchronize()
    assert getattr(net, "_bucket", None) is None and getattr(net.sign_inv_net, "_bucket", None) is None
    twin, _ = _net(name)
    twin.load_state_dict(net.state_dict())
    b2 = _batch(name, 9, seed=11)
    assert _eager_loss(net, b2).item() == _eager_loss(twin, b2).item()
    _release(s)
