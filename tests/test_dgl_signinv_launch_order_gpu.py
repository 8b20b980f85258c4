"""-m gpu: the ORDER of the launches of the four sign-invariant encoders of the DGL tree (dgl_deepsigns, dropout_signinv,
activation_signinv: eval, the train-mode value, forward + backward; the layer path and a reduced-precision stage forward of the GIN
pair) and the launch counts of two captured DGLBucketedStep steps, against the literals of tests/dgl_signinv_launch_orders.py.  The
other suites pin outputs and a few launch counts; this one fails when a launch moves — a pack in front of the plan instead of behind
it, a dropout step advanced twice, a layer-path pack that changes place relative to the stage launches."""
import pytest

import dgl_signinv_launch_cases as L
from dgl_signinv_launch_orders import ORDERS

pytestmark = pytest.mark.gpu


def test_every_case_has_a_recorded_order():
    assert set(ORDERS) == set(L.CASES)
    assert all(ORDERS[n] for n in ORDERS)
    assert all(ORDERS[n].count(L.MARK) == 1 and ORDERS[n][0] != L.MARK and ORDERS[n][-1] != L.MARK for n in L.EAGER)


@pytest.mark.parametrize("name", list(L.CASES))
def test_launches_are_the_recorded_ones(name):
    got, want = L.record(name), ORDERS[name]
    if isinstance(want, list):
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        assert got == want, f"{name}: {len(got)} launches, {len(want)} recorded; first difference at {first}: {got[first:first + 3]} vs {want[first:first + 3]}"
    assert got == want
