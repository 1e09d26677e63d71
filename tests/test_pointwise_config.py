"""PointwiseEvaluator's host side: data preparation, refusals, exports, and the unchanged ABI version."""
import ctypes

import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd import evaluators
from multitreegp_amd.coefficients import CoefficientOptimiser


def test_prepare_transposes_and_pads():
    X, Y = np.arange(10, dtype=np.float32).reshape(5, 2), np.arange(15, dtype=np.float32).reshape(5, 3)
    ff = mt.PointwiseEvaluator()
    d = ff.prepare((X, Y))
    assert (d["M"], d["ld"], d["n_var"], d["n_out"]) == (5, 8, 2, 3)
    assert d["xt"].shape == (2, 8) and d["yt"].shape == (3, 8) and d["xt"].dtype == np.float32
    assert np.array_equal(d["xt"][:, :5], X.T) and np.array_equal(d["yt"][:, :5], Y.T) and not d["xt"][:, 5:].any()
    assert (ff.n_data(), ff.n_trees(), ff.max_fitness) == (2, 3, 1e4)
    assert ff.program_specs()[0] == [(0, 2, 0), (1, 2, 0), (2, 2, 0)]


@pytest.mark.parametrize("xs, ys, err", [((4, 9), (4, 1), NotImplementedError), ((4, 2), (4, 5), NotImplementedError),
                                         ((4, 2), (3, 1), ValueError), ((0, 2), (0, 1), ValueError)])
def test_refusals(xs, ys, err):
    with pytest.raises(err):
        mt.PointwiseEvaluator().prepare((np.zeros(xs, np.float32), np.zeros(ys, np.float32)))


def test_exports_abi_and_no_coefficient_optimisation():
    with pytest.raises(NotImplementedError):
        CoefficientOptimiser.check_evaluator(mt.PointwiseEvaluator())
    assert evaluators.PointwiseEvaluator is mt.PointwiseEvaluator and "PointwiseEvaluator" in evaluators.__all__
    assert nat.ABI_VERSION == 24
    lib = nat.load()
    pw, one = nat.MtgpPointwise(), np.zeros(4, np.int32)
    args = (one.ctypes.data, one.ctypes.data, 1, 4, 1, None)
    assert lib.mtgp_eval_pointwise(ctypes.byref(pw), *args) == nat.ERR_ARG  # no buffers: nothing launched
    assert lib.mtgp_eval_pointwise_jit(None, *args[:-1], None, None) == nat.ERR_ARG
