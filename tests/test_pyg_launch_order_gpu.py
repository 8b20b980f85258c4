"""-m gpu: the ORDER of the launches of the PyG trees' plain models (pyg.GNN, pyg_gnn_types.GNN for every gnn_type and both link
forms, dropout_models.GNN, pyg_baselines.NetGINE), of SignNetGNN's differentiable forward and of two captured steps, against the
literals of tests/pyg_launch_orders.py.  The other suites pin outputs and a few launch counts; this one fails when a launch moves —
an edge-id check behind the GCN coefficients instead of in front of them, an encoder evaluated one layer early."""
import pytest

import pyg_launch_cases as L
from pyg_launch_orders import ORDERS

pytestmark = pytest.mark.gpu


def test_every_case_has_a_recorded_order():
    assert set(ORDERS) == set(L.CASES)
    assert all(ORDERS[n] for n in ORDERS)


@pytest.mark.parametrize("name", list(L.CASES))
def test_launches_are_the_recorded_ones(name):
    got, want = L.record(name), ORDERS[name]
    if isinstance(want, list):
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        assert got == want, f"{name}: {len(got)} launches, {len(want)} recorded; first difference at {first}: {got[first:first + 3]} vs {want[first:first + 3]}"
    assert got == want
