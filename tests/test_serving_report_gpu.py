"""The serving mode's status report (SignNetGNN.strict = False): a forward with a one-launch plan takes it from the plan launch's
pinned words (ops.EarlyReport, queued in `_pending`), every other forward from the GINE kernel's last workgroup — same verdicts, same
exceptions, outputs bit-equal to the strict mode's.

Batches are 3-6 graphs of 3-9 nodes (hidden 128, k = 4) unless a case needs otherwise; every fault is one the kernels flag and
survive (a NaN row, never an access outside the batch's arrays).  "The exception type strict mode raises": where strict mode serves
the batch instead of raising (a graph beyond the fused limits or without nodes goes layer by layer), the serving mode's documented
RuntimeError is expected."""
import time
import types

import numpy as np
import pytest
import torch

import gnn_front_cases as cases

pytestmark = pytest.mark.gpu

CTOR = (None, None, 128, 1, 2, 2)
SIZES = [9, 3, 7, 5]


def _make(max_k):
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    m = SignNetGNN(*CTOR, variant="gine", max_k=max_k).cuda().eval()
    m.strict = False
    return m


@pytest.fixture(scope="module")
def model():
    return _make(4)


@pytest.fixture(scope="module")
def model_all():
    return _make(None)


def _clean(seed=11, sizes=SIZES):
    from signnet_basisnet_amd import synth
    return synth.make_batch(len(sizes), seed=seed, sizes=sizes)


def _dense193():
    """15 nodes, 96 undirected edges + one more directed one: 193 in-edges (the fused GINE stage stages 192)."""
    pairs = [(a, b) for a in range(15) for b in range(a + 1, 15)]
    ei = cases._sym(pairs[:96])
    ei = np.concatenate([ei, np.array([[pairs[96][0]], [pairs[96][1]]], dtype=np.int64)], axis=1)
    assert ei.shape[1] == 193
    return 15, ei


def _vocab(model):
    g = model.gnn
    return int(g.input_encoder.embeddings[0].weight.shape[0]), int(g.edge_encoders[0].embeddings[0].weight.shape[0])


def _fault(name, model):
    d = _clean()
    if name == "unsorted":
        d.batch = d.batch.flip(0).contiguous()
    elif name == "edge_across":
        e = int((d.batch[d.edge_index[1]] == 1).nonzero()[0])      # an in-edge of graph 1 now starts in graph 0
        d.edge_index[0, e] = 0
    elif name == "node_id":
        d.x[SIZES[0], 0] = _vocab(model)[0]
    elif name == "edge_id":
        d.edge_attr[int((d.batch[d.edge_index[0]] == 2).nonzero()[0])] = _vocab(model)[1]
    elif name == "empty_graph":
        d = _clean(sizes=[5, 0, 7, 3])
    elif name == "nodes65":
        d = cases.collate([cases.g_tree(5, 1, 1), cases.g_tree(65, 3, 7), cases.g_tree(7, 1, 2)], seed=3)
    elif name == "edges193":
        d = cases.collate([cases.g_tree(5, 1, 1), _dense193(), cases.g_tree(7, 1, 2)], seed=3)
    else:
        raise KeyError(name)
    return d


def _strict_type(model, dd):
    """What strict mode raises for the batch (None: it serves it)."""
    model.strict = True
    try:
        with torch.no_grad():
            model(dd)
        return None
    except (ValueError, IndexError, RuntimeError) as e:
        return type(e)
    finally:
        model.strict = False


def _plans(model, dd):
    """One serving-mode forward -> (y, the plan it built, whether a pinned buffer went to the GINE kernel)."""
    from signnet_basisnet_amd import fused, ops
    build, got = ops.build_plan, []
    ops.build_plan = lambda *a, **k: got.append(build(*a, **k)) or got[-1]
    cls, hosts = fused.GnnPlan, []
    run = cls.run

    def spy(self, plan, x, ea, s, flags_host=None, out=None):
        hosts.append(flags_host)
        return run(self, plan, x, ea, s, flags_host, out)
    cls.run = spy
    try:
        with torch.no_grad():
            y = model(dd)
    finally:
        ops.build_plan, cls.run = build, run
    return y, got[-1], hosts[-1] is not None


def test_clean_batch_reports_from_the_plan_launch_and_equals_strict_mode(model):
    from signnet_basisnet_amd import ops, synth
    dd = synth.batch_to(_clean(), "cuda:0")
    model.check_last()
    y, plan, kernel_report = _plans(model, dd)
    assert plan.front is not None and not kernel_report, "a one-launch plan: the GINE kernel carries no report"
    assert len(model._pending) == 1 and isinstance(model._pending[0][1], ops.EarlyReport)
    model.check_last()
    assert not model._pending
    y = y.clone()
    model.strict = True
    with torch.no_grad():
        y_strict = model(dd)
    model.strict = False
    assert torch.isfinite(y).all() and torch.equal(y, y_strict)


@pytest.mark.parametrize("name", ["unsorted", "edge_across", "node_id", "edge_id", "empty_graph", "nodes65", "edges193"])
def test_each_fault_reaches_check_last_with_strict_modes_exception(model, name):
    from signnet_basisnet_amd import ops, synth
    dd = synth.batch_to(_fault(name, model), "cuda:0")
    expect = _strict_type(model, dd) or RuntimeError
    print(f"{name}: strict mode -> {expect.__name__}")
    assert expect is {"unsorted": ValueError, "edge_across": ValueError, "node_id": IndexError, "edge_id": IndexError}.get(name, RuntimeError)
    model.check_last()
    y, plan, kernel_report = _plans(model, dd)
    assert plan.front is not None and not kernel_report
    assert isinstance(model._pending[-1][1], ops.EarlyReport)
    with pytest.raises(expect) as ei:
        model.check_last()
    assert type(ei.value) is expect
    assert torch.isnan(y).any()
    model.check_last()                                             # reported once


def test_host_sizes_smaller_than_the_devices_largest_graph(model_all):
    from signnet_basisnet_amd import pyg, synth
    dd = synth.batch_to(_clean(), "cuda:0")
    liar = types.SimpleNamespace(**vars(dd))
    liar.sizes = [6, 6, 6, 6]                                      # adds up to the batch, largest 6, not 9
    assert sum(liar.sizes) == sum(SIZES) and pyg.host_max_nodes(liar) == 6
    assert _strict_type(model_all, liar) is ValueError
    with torch.no_grad():
        model_all(liar)
    with pytest.raises(ValueError, match="disagree"):
        model_all.check_last()
    with torch.no_grad():                                          # the all-eigenvector count of an honest batch passes
        y = model_all(dd).clone()
    model_all.check_last()
    bare = types.SimpleNamespace(**{k: v for k, v in vars(dd).items() if k != "sizes"})      # K from the report's largest-graph word
    with torch.no_grad():
        assert torch.equal(model_all(bare), y)
    model_all.check_last()


def test_eight_queued_forwards_with_the_fourth_faulty(model):
    from signnet_basisnet_amd import synth
    good = synth.batch_to(_clean(), "cuda:0")
    bad = synth.batch_to(_fault("node_id", model), "cuda:0")
    model.check_last()
    raised, blocked, watching = [], [], []
    wait_status = model._wait_status

    def watched(ev, host):
        if watching:
            blocked.append(not model._arrived(ev, host))
        return wait_status(ev, host)
    model._wait_status = watched
    try:
        with torch.no_grad():
            for i in range(8):
                try:
                    model(bad if i == 3 else good)                 # (a later forward's own check_last(wait=False) may be the one that raises)
                except IndexError as e:
                    assert i > 3
                    raised.append(e)
        assert len(model._pending) <= 4                            # (beyond four queued reports wait=False takes the oldest, as ever)
        watching.append(1)
        t0 = time.perf_counter()
        try:
            model.check_last(wait=False)                           # before any wait: looks at what has arrived, never blocks
        except IndexError as e:
            raised.append(e)
        dt = time.perf_counter() - t0
        watching.clear()
        assert not any(blocked), "check_last(wait=False) waited for a report that had not arrived"
        try:
            model.check_last()
        except IndexError as e:
            raised.append(e)
    finally:
        del model._wait_status
    print(f"check_last(wait=False): {dt * 1e6:.0f} us; raised {len(raised)} time(s)")
    assert len(raised) == 1 and not model._pending
    model.check_last()


def test_pinned_slots_are_pooled_and_arrive_zeroed(model):
    from signnet_basisnet_amd import ops, synth
    E = ops.EarlyReport
    dd = synth.batch_to(_clean(), "cuda:0")
    with torch.no_grad():
        model(dd)
    model.check_last()
    made0, pool0 = E._made, len(E._pool)
    with torch.no_grad():
        for _ in range(12):                                        # one in flight at a time: no new slot
            model(dd)
            model.check_last()
    assert E._made == made0 and len(E._pool) == pool0
    with torch.no_grad():
        for _ in range(3):                                         # up to three in flight
            model(dd)
        in_flight = len(model._pending)
        assert E._made - made0 <= in_flight and E._made - len(E._pool) == made0 - pool0 + in_flight
    model.check_last()
    assert E._made - len(E._pool) == made0 - pool0, "every slot is back in the pool"
    assert not getattr(model, "_limbo", [])
    assert E._pool[-1][1][8:12].all(), "the slot last released carries its launch's done words"
    r = E()
    assert not r.v.any(), "a recycled slot arrives zeroed"
    r.release()
    assert E._made - len(E._pool) == made0 - pool0


def test_reports_dropped_behind_an_error_wait_for_their_launch(model):
    """check_last() drops the reports queued behind a faulty one unread; their slots are pooled once their done words are set."""
    from signnet_basisnet_amd import ops, synth
    E = ops.EarlyReport
    good = synth.batch_to(_clean(), "cuda:0")
    bad = synth.batch_to(_fault("unsorted", model), "cuda:0")
    model.check_last()
    out0 = E._made - len(E._pool)
    model.check_last = lambda wait=True: None                      # (queue three without the forwards' own look at the first)
    try:
        with torch.no_grad():
            model(bad), model(good), model(good)
    finally:
        del model.check_last
    with pytest.raises(ValueError, match="malformed"):
        model.check_last()
    assert not model._pending
    assert len(model._limbo) <= 2 and all(isinstance(h, E) for h in model._limbo)      # (slots whose launch had not finished are parked)
    torch.cuda.synchronize()
    model.check_last()
    assert not model._limbo and E._made - len(E._pool) == out0


def test_beyond_the_one_launch_plan_the_gine_kernel_reports(model):
    """1025 graphs of 3 nodes: one graph past what sn_batch_plan_early_supported takes (N <= 4096, E <= 12288, B <= 1024) — the
    smallest batch it refuses.  Five-launch plan, no front records: the last workgroup of the GINE kernel reports."""
    from signnet_basisnet_amd import ops, synth
    host = _clean(seed=5, sizes=[3] * 1025)
    N, E, B = host.batch.numel(), host.edge_index.shape[1], 1025
    assert ops.early_supported(N, E, 1024) and not ops.early_supported(N, E, B)
    dd = synth.batch_to(host, "cuda:0")
    model.check_last()
    y, plan, kernel_report = _plans(model, dd)
    assert plan.front is None and kernel_report
    assert not isinstance(model._pending[-1][1], ops.EarlyReport) and model._pending[-1][0] is None
    model.check_last()
    y = y.clone()
    flags = plan.flags.cpu().tolist()
    assert flags[4] == B and flags[0] == 0 and flags[3] == 0 and flags[1] == 3
    model.strict = True
    with torch.no_grad():
        assert torch.equal(model(dd), y)
    model.strict = False
    for name, expect in (("node_id", IndexError), ("edge_across", ValueError), ("nodes65", RuntimeError)):
        bad = types.SimpleNamespace(**vars(host))
        bad.x, bad.edge_index = host.x.clone(), host.edge_index.clone()
        if name == "node_id":
            bad.x[7, 0] = _vocab(model)[0]
        elif name == "edge_across":
            bad.edge_index[0, int((host.batch[host.edge_index[1]] == 1).nonzero()[0])] = 0      # an in-edge of graph 1 from graph 0
        else:
            big = cases.collate([cases.g_tree(65, 3, 7)] + [cases.g_tree(3, 0, s) for s in range(1024)], seed=3)
            bad = big
            assert not ops.early_supported(bad.batch.numel(), bad.edge_index.shape[1], 1025)
        bd = synth.batch_to(bad, "cuda:0")
        _, plan, kernel_report = _plans(model, bd)
        assert plan.front is None and kernel_report
        with pytest.raises(expect) as ei:
            model.check_last()
        assert type(ei.value) is expect, name
    model.check_last()


def test_a_captured_forward_posts_nothing_to_the_host(model):
    from signnet_basisnet_amd import fused, ops, synth
    E = ops.EarlyReport
    dd = synth.batch_to(_clean(), "cuda:0")
    with torch.no_grad():
        y0 = model(dd).clone()
        model.check_last()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(dd)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        model.check_last()
        made, pool, free = E._made, len(E._pool), len(model._free_hosts)
        cls, hosts = fused.GnnPlan, []
        run = cls.run

        def spy(self, plan, x, ea, s, flags_host=None, out=None):
            hosts.append(flags_host)
            return run(self, plan, x, ea, s, flags_host, out)
        cls.run = spy
        try:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                y_cap = model(dd)
        finally:
            cls.run = run
        assert hosts == [None] and model._captured_plan.front is not None
        assert not model._pending and model._flags_host is None and model._early is None
        assert (E._made, len(E._pool), len(model._free_hosts)) == (made, pool, free)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y_cap, y0)
    model.check_captured()
    dd.x.add_(1000)                                                # a bad id in the static input: the captured plan's flags say so
    g.replay()
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        model.check_captured()
    dd.x.sub_(1000)
