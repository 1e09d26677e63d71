"""PointwiseEvaluator on the GPU with more than two spans: W = 3, 6, 7 (M = 8193, 20481, 24577: a one-point last
span, zeros up to 4, 8 and 8 spans) through k_pointwise_mean's binary-counter stack and, scaled, through
k_pointwise_scaled_mean / pw_span_tree, on k_pointwise, k_pointwise_wide and the forced wide kernel.  float32 normal
tables: numpy float32 evaluates the same + - * tree node by node and the spec's sums (nothing is contracted), so
the comparison stays bit for bit, and tests/test_pointwise_reference.py shows that at W = 6 and 7 these tables
tell the span tree from a left fold."""
import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd.engine import DeviceEngine
from helpers import bits_equal
from test_gpu_pointwise import library, tree
from test_gpu_pointwise_scaled import within_bound
from test_pointwise_reference import SPAN_M, SPAN_N_OUT, SPAN_P, span_case

pytestmark = pytest.mark.gpu
f32, MAXF = np.float32, 1e4
KERNELS = {"narrow": (8, False), "wide": (17, False), "forced_wide": (8, True)}  # n_var, MTGP_PW_WIDE=1


def run(monkeypatch, kernel, M, scaled):
    n_var, forced = KERNELS[kernel]
    monkeypatch.setenv("MTGP_PW_WIDE", "1") if forced else monkeypatch.delenv("MTGP_PW_WIDE", raising=False)
    X, Y, exprs, want, ref = span_case(M, n_var)
    lib = library("+-*", n_var, SPAN_N_OUT)
    pop = np.stack([np.stack([tree(lib, e) for e in ex]) for ex in exprs])
    eng = DeviceEngine(mt.PointwiseEvaluator(MAXF, linear_scaling=scaled, wide=n_var > 8), lib, 0.0, "cuda:0")
    res = eng.evaluate(torch.from_numpy(pop).cuda(), (X, Y), trajectories=True)
    torch.cuda.synchronize()
    assert eng._pointwise_wide() == (kernel != "narrow") and DeviceEngine.jit_ok(res["_flat"])
    assert (eng._jit_mode() == nat.JIT_MODE_LDS) == (kernel != "narrow")
    return {k: res[k].cpu().numpy() for k in ("fitness", "pred") + (("scale",) if scaled else ())}


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("M", SPAN_M)
def test_span_sums_bitexact_and_within_f64_bound(monkeypatch, M, kernel):
    X, Y, _, want, ref = span_case(M, KERNELS[kernel][0])
    got = run(monkeypatch, kernel, M, scaled=False)
    assert bits_equal(got["pred"], want)
    assert bits_equal(got["fitness"], ref), (got["fitness"], ref)
    # the bound of test_gpu_pointwise.test_exact_programs_bitexact_and_within_f64_bound: W enters through the
    # height of the span tree
    W = -(-M // 4096)
    A = (-(-min(M, 4096) // 64) - 1) + 6 + (W - 1).bit_length() + SPAN_N_OUT
    ref64 = ((want.astype(np.float64) - Y.T.astype(np.float64)) ** 2).sum(axis=(1, 2)) / M
    print(M, kernel, np.abs(got["fitness"] - ref64) / ref64 * 2.0 ** 24, A + 2)
    assert np.all(np.abs(got["fitness"] - ref64) <= (A + 2) * 2.0 ** -24 * ref64), (got["fitness"], ref64)


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("M", SPAN_M)
def test_scaled_span_moments_against_float64_closed_form(monkeypatch, M, kernel):
    X, Y, _, want, _ = span_case(M, KERNELS[kernel][0])
    got = run(monkeypatch, kernel, M, scaled=True)
    assert bits_equal(got["pred"], want)
    for p, (_, _, a, b, bad, deg) in enumerate(within_bound(got["fitness"], want, Y)):
        ab = np.stack([a, b], axis=1)  # (2^-20 relative, as test_scaled_against_float64_closed_form of the wide tests)
        assert not bad.any() and not deg.any(), (p, bad, deg)
        assert np.all(np.abs(got["scale"][p] - ab) <= 2.0 ** -20 * np.abs(ab)), (p, got["scale"][p], ab)
    assert SPAN_P == len(got["fitness"])
