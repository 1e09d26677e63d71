"""PointwiseEvaluator(linear_scaling=True) on the host: the flag, prepare's exact sums, the new entries' refusals."""
import ctypes
import math

import numpy as np

import multitreegp_amd as mt
from multitreegp_amd import _native as nat


def test_flag_default_and_prepare_sums():
    rng = np.random.default_rng(0)
    X = rng.normal(size=(1001, 2)).astype(np.float32)
    Y = (rng.normal(size=(1001, 3)) * [1.0, 1e3, 1e-3] + [0.0, 4096.0, 1.0]).astype(np.float32)
    plain, scaled = mt.PointwiseEvaluator(), mt.PointwiseEvaluator(1e4, linear_scaling=True)
    assert plain.linear_scaling is False and scaled.linear_scaling is True
    d0, d1 = plain.prepare((X, Y)), scaled.prepare((X, Y))
    assert set(d0) == {"xt", "yt", "M", "ld", "n_var", "n_out"} and set(d1) == set(d0) | {"sy", "syy"}
    assert all(np.array_equal(d0[k], d1[k]) for k in d0)
    assert d1["sy"].dtype == d1["syy"].dtype == np.float64
    for k in range(3):
        y = [float(v) for v in Y[:, k]]
        assert d1["sy"][k] == math.fsum(y) and d1["syy"][k] == math.fsum(v * v for v in y)


def test_scaled_entries_refuse_missing_buffers():
    lib = nat.load()
    pw, sc, one = nat.MtgpPointwise(), nat.MtgpPointwiseScale(), np.zeros(4, np.int32)
    args = (one.ctypes.data, one.ctypes.data, 1, 4, 1)
    assert lib.mtgp_eval_pointwise_scaled(ctypes.byref(pw), ctypes.byref(sc), *args, None) == nat.ERR_ARG  # no buffers
    assert lib.mtgp_eval_pointwise_scaled_jit(None, ctypes.byref(sc), *args, None, None) == nat.ERR_ARG
    buf = np.zeros(64, np.float32)  # every buffer of MtgpPointwise present (a refusal precedes any device call)
    pw.xt = pw.yt = pw.nodes = pw.fitness = buf.ctypes.data + (-buf.ctypes.data) % 16
    pw.M, pw.ld, pw.n_var, pw.n_out, pw.max_fitness = nat.PW_SPAN + 1, nat.PW_SPAN + 4, 1, 1, 1.0
    assert lib.mtgp_eval_pointwise_scaled(ctypes.byref(pw), None, *args, None) == nat.ERR_ARG  # no scale arguments
    assert lib.mtgp_eval_pointwise_scaled(ctypes.byref(pw), ctypes.byref(sc), *args, None) == nat.ERR_ARG  # W = 2, no moments
