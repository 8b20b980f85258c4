"""`models` of LearningFilters for `dropin.install('learningfilters', baselines="all")` (the runner's `--baselines=all`): everything
`dropin/baseline_filter_models.py` provides — the base models and the four polynomial-filter baselines — with the last two names of
`training.py:9`, GatNet and ARMANet, bound to the HIP classes of `signnet_basisnet_amd.filter_baselines` as well: all ten values of
`--net` then run on this stack."""
from signnet_basisnet_amd.dropin import baseline_filter_models as _base
from signnet_basisnet_amd.dropin.baseline_filter_models import (BernNet, ChebNet, EqDeepSetsEncoder, GcnNet, GPRNet, MLP,  # noqa: F401
                                                                Transformer)
from signnet_basisnet_amd.filter_baselines import ARMANet, GatNet  # noqa: F401

BASELINES = _base.BASELINES
HIP_BASELINES = _base.HIP_BASELINES + ("GatNet", "ARMANet")


def __getattr__(name):
    return _base.__getattr__(name)
