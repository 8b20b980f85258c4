"""`models` of LearningFilters for `dropin.install('learningfilters', baselines=True)` (the runner's `--baselines`): everything
`dropin/learningfilters/models.py` provides, with the four polynomial-filter baselines of `training.py:9` — BernNet, GPRNet, ChebNet,
GcnNet — bound to the HIP classes of `signnet_basisnet_amd.filter_baselines`.  GatNet and ARMANet resolve as they do without the flag:
to the reference's own `models.py` when it imports, else to a placeholder that raises on construction."""
from signnet_basisnet_amd.dropin.learningfilters import models as _base
from signnet_basisnet_amd.dropin.learningfilters.models import EqDeepSetsEncoder, MLP, Transformer  # noqa: F401
from signnet_basisnet_amd.filter_baselines import BernNet, ChebNet, GcnNet, GPRNet  # noqa: F401

BASELINES = _base.BASELINES
HIP_BASELINES = ("BernNet", "GPRNet", "ChebNet", "GcnNet")


def __getattr__(name):
    return _base.__getattr__(name)
