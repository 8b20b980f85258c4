"""The GINE stage's front records (sn_batch_plan_front / sn_gnn_fused_front_f32): what the plan launch's front workgroups write
against the host restatement (signnet_basisnet_amd/gnn_front.py), and the forward that starts from the records against the one
whose stage kernel runs its own prologue — same library, records withheld — bit for bit."""
import numpy as np
import pytest
import torch

import gnn_front_cases as cases

pytestmark = pytest.mark.gpu

CTOR = (None, None, 128, 1, 2, 2)


@pytest.fixture(scope="module")
def model():
    from signnet_basisnet_amd.pyg import SignNetGNN
    torch.manual_seed(0)
    m = SignNetGNN(*CTOR, variant="gine", max_k=8).cuda().eval()
    m.strict = False          # serving mode: the flags stay on the device, a graph that cannot be served gets a NaN row
    return m


def _drain(model):
    """Serving mode: take the queued flag reports (their pinned buffers go back to the module's pool); what they say is compared
    through plan.flags."""
    try:
        model.check_last()
    except (RuntimeError, ValueError, IndexError):
        pass


def _forward(model, data, front):
    """(y, flags, plan) of one forward with / without the front records."""
    from signnet_basisnet_amd import ops, pyg, synth
    dd = synth.batch_to(data, "cuda:0")
    saved, build, plans = pyg._USE_FRONT, ops.build_plan, []
    pyg._USE_FRONT = front
    ops.build_plan = lambda *a, **k: plans.append(build(*a, **k)) or plans[-1]       # (the module drops its plan behind the forward)
    try:
        with torch.no_grad():
            y = model(dd).clone()
        torch.cuda.synchronize()
    finally:
        pyg._USE_FRONT, ops.build_plan = saved, build
    plan = plans[-1]
    _drain(model)
    assert (plan.front is not None) == front
    return y.cpu(), plan.flags.cpu().tolist(), plan


def _tables(model):
    g = model.gnn
    d = g.linear.weight.shape[0]
    return (g.input_encoder.embeddings[0].weight.detach().cpu(), [e.embeddings[0].weight.detach().cpu() for e in g.edge_encoders],
            g.linear.weight.detach().cpu()[:, :d].contiguous())


def _check_records(model, data, plan, expect_valid):
    from signnet_basisnet_amd import gnn_front as GF
    ntab, etabs, lin_a = _tables(model)
    recs = GF.decode(plan.front, data.num_graphs, len(etabs))
    assert [r["valid"] for r in recs] == expect_valid
    for g, r in enumerate(recs):
        h = GF.host_record(g, data.batch, data.edge_index, data.x, data.edge_attr, ntab, etabs, lin_a)
        assert h["valid"] == r["valid"], g
        if not r["valid"]:
            continue
        assert (r["n"], r["ne"], r["ncls"]) == (h["n"], h["ne"], h["ncls"])
        assert np.array_equal(r["info"], h["info"]), g                    # degree, packed first-four in-edges, erow of every row
        assert np.array_equal(r["esrc"], h["esrc"]) and np.array_equal(r["ecls"], h["ecls"]), g
        assert np.array_equal(r["ee"], h["ee"]), g                        # table rows: copies
        # the parked lin_a rows: six bf16 partial products per term, fp32 accumulate — against float64 within the worst case of
        # the 6 K accumulation roundings plus the dropped products (<= 2^-23 |x||w| per term): (6 K + 2) 2^-24 sum |x||w|
        err = (torch.from_numpy(r["x1"]).double() - h["x1"]).abs()
        bound = (6 * 128 + 2) * 2.0 ** -24 * h["x1_abs"]
        print(f"graph {g}: n={r['n']} ne={r['ne']} ncls={r['ncls']} max err / bound = {float((err / bound.clamp_min(1e-30)).max()):.3f}")
        assert bool((err <= bound).all()), g
        assert not r["x1"][r["n"]:].any()                                  # rows behind the graph in its last row tile: +0
    return recs


@pytest.mark.parametrize("name", ["batch_one", "batch_three"])
def test_records_match_the_host_restatement_and_y_is_bit_identical(model, name):
    data = getattr(cases, name)()
    y1, f1, plan = _forward(model, data, True)
    recs = _check_records(model, data, plan, [1] * data.num_graphs)
    if name == "batch_three":
        assert [r["n"] for r in recs] == [16, 17, 64] and recs[2]["ne"] == 192
        assert sorted(set(recs[0]["info"][:16, 0].tolist())) == [0, 1, 4, 9] and all(r["ncls"] == 2 for r in recs)
    y0, f0, _ = _forward(model, data, False)
    assert torch.isfinite(y0).all()
    assert torch.equal(y1, y0) and f1 == f0


@pytest.mark.parametrize("name,valid", [("batch_oversize", [1, 0, 1]), ("batch_bad_atom", [0, 1])])
def test_a_graph_the_record_cannot_describe_keeps_its_flags_and_nan_row(model, name, valid):
    data = getattr(cases, name)()
    y1, f1, plan = _forward(model, data, True)
    _check_records(model, data, plan, valid)
    y0, f0, _ = _forward(model, data, False)
    assert f1 == f0 and any(f0)
    assert torch.equal(torch.isnan(y1), torch.isnan(y0)) and bool(torch.isnan(y0).any())
    assert torch.equal(torch.nan_to_num(y1), torch.nan_to_num(y0))


def test_a_served_graph_without_a_record_runs_the_in_kernel_prologue_bit_identically(model):
    """In a launch with records a graph without a valid one runs the general row-tile form of the in-kernel prologue; without records
    it runs the compile-time row-tile form: the same products in the same order."""
    data = cases.batch_wide_bond()
    y1, f1, plan = _forward(model, data, True)
    _check_records(model, data, plan, [0, 0, 0])
    y0, f0, _ = _forward(model, data, False)
    assert torch.isfinite(y0).all() and not any(f0[:1] + f0[3:4])
    assert torch.equal(y1, y0) and f1 == f0


def test_capture_and_replay_with_front_records(model):
    from signnet_basisnet_amd import synth
    data = cases.batch_three()
    y0, _, _ = _forward(model, data, False)
    dd = synth.batch_to(data, "cuda:0")
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            model(dd)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        _drain(model)                                  # (a capturing forward must find a pinned flag buffer in the pool)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            y_cap = model(dd)
        assert model._captured_plan.front is not None
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(y_cap.cpu(), y0)
    model.check_captured()
