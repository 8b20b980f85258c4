#!/usr/bin/env python
"""Eigendecompositions of the at-size batches of tests/test_training_gpu.py (SIZE_CASES), stored so that the test feeds every machine
the same inputs.  The graphs, features and weights of those batches are seeded and identical everywhere; the fp32 eigenvectors that
synth.make_batch computes with the host's LAPACK are not (they differ in the last bits, and in sign, with the CPU's instruction set),
and the gradient test's fp32-vs-float64 comparison depends on every ReLU decision the inputs lead to.

    python tests/golden/make_size_cases_eig.py      # rewrites tests/golden/size_cases_eig.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from signnet_basisnet_amd import synth  # noqa: E402
from test_training_gpu import SIZE_CASES  # noqa: E402


def main():
    arrays = {}
    for name, c in SIZE_CASES.items():
        data = synth.make_batch(c["B"], seed=c["seed"], n_lo=c["lo"], n_hi=c["hi"], features=c["feat"])
        arrays[name + "/eigen_values"] = data.eigen_values.numpy()
        arrays[name + "/eigen_vectors"] = data.eigen_vectors.numpy()
    np.savez_compressed(os.path.join(HERE, "size_cases_eig.npz"), **arrays)


if __name__ == "__main__":
    main()
