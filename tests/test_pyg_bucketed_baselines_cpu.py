"""CPU: the host side of train_graph.BucketedStep for the baselines of the two PyG trees — which models are admitted and what the
refusals say, bucket_of on a batch without eigen fields, and the deferral of the forward's status read (no GPU: nothing is launched)."""
import types

import pytest
import torch


def _step(model, **kw):
    from signnet_basisnet_amd import optim
    from signnet_basisnet_amd.train_graph import BucketedStep
    return BucketedStep(model, optim.FlatAdam(model.parameters(), lr=1e-3), **kw)


def _baselines():
    from signnet_basisnet_amd import dropout_models, pyg, pyg_baselines, pyg_gnn_types
    yield pyg.GNN(None, None, 16, 1, 2, "gine")
    for kind in pyg_gnn_types.GNN_TYPES:
        yield pyg_gnn_types.GNN(None, None, 16, 1, 2, kind)
    yield dropout_models.GNN(None, None, 16, 1, 2, "GINConv", dropout=0.1)
    yield pyg_baselines.NetGINE(16)


def test_the_baseline_models_are_admitted_next_to_signnet():
    from signnet_basisnet_amd.pyg import SignNetGNN
    for m in _baselines():
        assert _step(m).plain is True, type(m)
    assert _step(SignNetGNN(None, None, 16, 1, 2, 1, variant="gine", max_k=8)).plain is False


def test_refusals_name_the_accepted_classes():
    from signnet_basisnet_amd import pyg
    from signnet_basisnet_amd.optim import FlatAdam
    from signnet_basisnet_amd.train_graph import BucketedStep
    names = ("pyg.SignNetGNN", "pyg.GNN", "pyg_gnn_types.GNN", "dropout_models.GNN", "pyg_baselines.NetGINE")
    lin = torch.nn.Linear(4, 4)
    with pytest.raises(TypeError) as e:
        BucketedStep(lin, FlatAdam(lin.parameters(), lr=1e-3))
    assert all(n in str(e.value) for n in names) and "Linear" in str(e.value)
    # an object that merely carries the attribute the admission check used to look at
    fake = torch.nn.Linear(4, 4)
    fake.variant = "gine"
    with pytest.raises(TypeError):
        BucketedStep(fake, FlatAdam(fake.parameters(), lr=1e-3))
    # Alchemy's GNN is a parameter holder of SignNetGNN, no model of its own
    alch = pyg.GNN(6, 4, 16, 1, 2, "alchemy")
    with pytest.raises(TypeError, match="variant='alchemy' is no model of its own") as e:
        BucketedStep(alch, FlatAdam(alch.parameters(), lr=1e-3))
    assert all(n in str(e.value) for n in names)


def test_bucket_of_a_batch_without_eigen_fields():
    """Only N and E pick a capture: S and K are the smallest legal values, with or without eigen data on the batch."""
    from signnet_basisnet_amd import pyg_gnn_types, synth
    from signnet_basisnet_amd.train_graph import Bucket
    host = synth.make_batch(12, seed=5)
    N, E = host.batch.numel(), host.edge_index.shape[1]
    bare = types.SimpleNamespace(x=host.x, edge_index=host.edge_index, edge_attr=host.edge_attr, batch=host.batch, num_graphs=12)
    s = _step(pyg_gnn_types.GNN(None, None, 16, 1, 2, "GCNConv"), max_graphs=16, granule=dict(N=64, E=128))
    want = Bucket(-(-(N + 1) // 64) * 64, -(-E // 128) * 128, 1, 1)
    assert s.bucket_of(bare) == want == s.bucket_of(host)
    assert s.B_cap == 17
    with pytest.raises(ValueError, match="exceeds max_graphs"):
        _step(pyg_gnn_types.GNN(None, None, 16, 1, 2, "GCNConv"), max_graphs=8).bucket_of(bare)
    # a batch whose N + 1 is a multiple of the granule keeps one padding node
    empty = types.SimpleNamespace(x=host.x[:63], edge_index=host.edge_index[:, :0], edge_attr=host.edge_attr[:0], batch=host.batch[:63],
                                  num_graphs=3)
    assert s.bucket_of(empty) == Bucket(64, 128, 1, 1)


def test_the_status_read_is_deferred_under_the_switch(monkeypatch):
    from signnet_basisnet_amd import ops, pyg_baselines, pyg_gnn_types
    calls = []
    plan = types.SimpleNamespace(status=torch.zeros(8, dtype=torch.int32), check=lambda: calls.append("check"))
    m = pyg_gnn_types.GNN(None, None, 16, 1, 2, "GATConv")
    m._finish_train(plan)
    assert calls == ["check"] and getattr(m, "_train_status", None) is None          # the eager step: one host read, at once
    m._defer_status = True
    m._finish_train(plan)
    assert calls == ["check"] and m._train_status is plan.status                     # a captured step: handed over, not read
    seen = []
    monkeypatch.setattr(ops, "check_plan_status", lambda st: seen.append(st))
    for model in (m, pyg_baselines.NetGINE(16)):
        model._train_status = plan.status
        model.check_train()
        assert seen.pop() is plan.status and model._train_status is None
        model.check_train()                                                           # nothing pending: nothing read
        assert not seen


def test_the_deferred_status_raises_what_the_eager_check_raises():
    from signnet_basisnet_amd import ops, pyg_gnn_types
    m = pyg_gnn_types.GNN(None, None, 16, 1, 2, "GINConv")
    m._train_status = torch.tensor([0, 12, 3, 0, 0, 1, 0, 0], dtype=torch.int32)
    with pytest.raises(IndexError):
        m.check_train()
    m._train_status = torch.tensor([4, 12, 3, 0, 0, 0, 0, 0], dtype=torch.int32)
    with pytest.raises(ValueError, match="edge endpoint out of range"):
        m.check_train()
    assert ops.check_plan_status(torch.tensor([0, 12, 3, 0, 0, 0, 0, 0], dtype=torch.int32))[1] == 12
