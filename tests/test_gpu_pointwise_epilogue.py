"""The end of the pointwise reductions on the GPU (pw_epilogue, pw_finish, pw_scaled_finish): the clip, a zero
ceiling, sums and means that overflow, a raw parsimony argument, non-finite targets and inputs, padding that must
not be used, and one invalid output next to a clean one -- each on k_pointwise, on the forced wide kernel
(MTGP_PW_WIDE=1) and on k_pointwise_wide with a 12-column table, at M = 70 (the main kernel finishes) and M = 4097
(k_pointwise_mean / k_pointwise_scaled_mean finish)."""
import math

import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd.engine import DeviceEngine
from helpers import bits_equal
from test_gpu_pointwise import fitness_ref, library, tree, value
from test_gpu_pointwise_scaled import reference, within_bound

pytestmark = pytest.mark.gpu
f32, MAXF, FLT_MAX = np.float32, 1e4, float(np.finfo(np.float32).max)
KERNELS = {"narrow": (3, False), "forced_wide": (3, True), "wide12": (12, False)}  # n_var, MTGP_PW_WIDE=1
kernels = pytest.mark.parametrize("kernel", list(KERNELS))
sizes = pytest.mark.parametrize("M", [70, 4097])
OPS = ["+", "-", "*", "/"]


def table(kernel, M, n_out, y=None, seed=3):
    """X uniform in [-1, 1); Y = y(X, normal noise) [M, n_out] (default: the noise)."""
    n_var = KERNELS[kernel][0]
    rng = np.random.default_rng(seed)
    X, E = rng.uniform(-1, 1, size=(M, n_var)).astype(f32), rng.normal(size=(M, n_out)).astype(f32)
    return X, (E if y is None else y(X, E)).astype(f32), f"x{n_var - 1}"


def evaluate(monkeypatch, kernel, exprs, X, Y, max_fitness=MAXF, scaled=False, parsimony=0.0, patch=None):
    """exprs [P][n_out] -> fitness, pred, nodes (and scale) of one evaluation; patch(prepared data) runs
    after a first evaluation, and the results are then those of a second one on the same data object."""
    n_var, forced = KERNELS[kernel]
    monkeypatch.setenv("MTGP_PW_WIDE", "1") if forced else monkeypatch.delenv("MTGP_PW_WIDE", raising=False)
    lib = library(OPS, n_var, Y.shape[1])
    pop = np.stack([np.stack([tree(lib, e) for e in ex]) for ex in exprs])
    ff = mt.PointwiseEvaluator(max_fitness, linear_scaling=scaled, wide=n_var > 8)
    eng = DeviceEngine(ff, lib, parsimony, "cuda:0")
    pt = torch.from_numpy(pop).cuda()
    res = eng.evaluate(pt, (X, Y), trajectories=True)
    if patch is not None:
        d = eng.prepare_data((X, Y))
        patch(d)
        assert eng.prepare_data((X, Y)) is d  # the cache is hit: the patched rows are evaluated
        res = eng.evaluate(pt, (X, Y), trajectories=True)
    torch.cuda.synchronize()
    assert eng._pointwise_wide() == (kernel != "narrow") and DeviceEngine.jit_ok(res["_flat"])
    out = {k: res[k].cpu().numpy() for k in ("fitness", "pred") + (("scale",) if scaled else ())}
    out["nodes"] = (pop[..., 0] != 0).sum(axis=(1, 2)).astype(f32)
    return out


def values(exprs, X):
    return np.stack([np.stack([value(e, X) for e in ex]) for ex in exprs])


def spec(want, Y, max_fitness=MAXF):
    with np.errstate(all="ignore"):
        return np.array([fitness_ref(w, Y, max_fitness) for w in want])


def mse64(want, Y):
    return ((want.astype(np.float64) - Y.T.astype(np.float64)) ** 2).sum(axis=(1, 2)) / Y.shape[0]


@kernels
@sizes
def test_clip_and_zero_ceiling(monkeypatch, kernel, M):
    X, Y, xl = table(kernel, M, 1, lambda X, E: X[:, :1] + f32(0.1) * E)
    far = [[("*", "x0", f32(8.0))], [("-", ("*", xl, f32(16.0)), "x0")]]
    near = [[("+", "x0", f32(0.125))], [("*", "x0", f32(0.75))], ["x0"]]
    want = values(far + near, X)
    m64 = mse64(want, Y)
    assert np.all(m64[:2] > 4.0) and np.all(m64[2:] < 0.25) and np.all(m64[2:] > 0)  # far above / below the ceiling 1
    got = evaluate(monkeypatch, kernel, far + near, X, Y, max_fitness=1.0)
    assert bits_equal(got["pred"], want)
    assert np.all(got["fitness"][:2] == f32(1.0)), got["fitness"]
    assert np.all(got["fitness"][2:] < f32(1.0)) and bits_equal(got["fitness"], spec(want, Y, 1.0)), got["fitness"]
    # a zero ceiling: every fitness is exactly 0, a pole's included, scaled and unscaled
    X = X.copy()
    X[3, 0] = 0.0
    exprs = far + near + [[("/", f32(1.0), "x0")]]
    for scaled in (False, True):
        got = evaluate(monkeypatch, kernel, exprs, X, Y, max_fitness=0.0, scaled=scaled)
        assert np.isinf(got["pred"][-1, 0, 3]) and np.array_equal(got["fitness"], np.zeros(len(exprs), f32)), got


@kernels
@sizes
def test_squared_error_overflows_to_the_ceiling(monkeypatch, kernel, M):
    """f stays finite, e e is inf: the f32 sum is inf, the mean is inf, the fitness max_fitness."""
    X, Y, xl = table(kernel, M, 1)
    X = (X * f32(0.5) + f32(2.0)).astype(f32)  # [1.5, 2.5)
    sq = ("*", "x0", "x0")
    exprs = [[("*", ("*", sq, sq), f32(1e19))], [("+", "x0", f32(0.5))]]
    want = values(exprs, X)
    assert np.all(np.isfinite(want)) and np.all(want[0].astype(np.float64) ** 2 > FLT_MAX)
    got = evaluate(monkeypatch, kernel, exprs, X, Y)
    assert bits_equal(got["pred"], want) and np.all(np.isfinite(got["pred"]))
    assert got["fitness"][0] == f32(MAXF) and got["fitness"][1] < f32(MAXF)
    assert bits_equal(got["fitness"], spec(want, Y)), got["fitness"]


@kernels
@sizes
@pytest.mark.parametrize("scale", [1e3, 1e30])  # the residual mean exceeds max_fitness / FLT_MAX
def test_scaled_mean_overflows_to_the_ceiling(monkeypatch, kernel, M, scale):
    """(float)(total / n) above max_fitness is clipped, above FLT_MAX it is inf: both score max_fitness, as the
    float64 reference clipped at max_fitness."""
    X, Y, xl = table(kernel, M, 1, lambda X, E: f32(scale) * E)
    exprs = [["x0"], [("*", "x0", xl)], [("+", ("*", "x0", "x0"), xl)]]
    want = values(exprs, X)
    y64 = Y[:, 0].astype(np.float64)
    floor = FLT_MAX if scale == 1e30 else MAXF
    for w in want[:, 0].astype(np.float64):  # the residual mean is var(y) (1 - r^2) > 0.75 var(y) > 2 floor
        assert abs(np.corrcoef(w, y64)[0, 1]) < 0.5 and 0.75 * y64.var() > 2 * floor
    got = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=True)
    assert bits_equal(got["pred"], want)
    for fit, bound, *_ in within_bound(got["fitness"], want, Y):  # (asserts == max_fitness where the reference is)
        assert fit == MAXF
    assert np.all(got["fitness"] == f32(MAXF)) and np.all(np.isfinite(got["scale"]))


@kernels
@sizes
def test_parsimony_is_added_after_the_clip(monkeypatch, kernel, M):
    """parsimony = 0.125 straight to DeviceEngine: fitness = clip(mean) + f32(0.125) * nodes, one f32 addition."""
    X, Y, xl = table(kernel, M, 1, lambda X, E: X[:, :1] * X[:, -1:] + f32(0.25) * E)
    exprs = [[("*", "x0", f32(1000.0))], [("+", "x0", ("*", xl, f32(0.5)))], [("*", "x0", xl)],
             [("+", ("*", ("-", "x0", xl), xl), f32(0.5))], [f32(1.5)]]
    want = values(exprs, X)
    ref = spec(want, Y)
    assert mse64(want, Y)[0] > 2 * MAXF and ref[0] == f32(MAXF) and np.all(ref[1:] < f32(MAXF))
    got = evaluate(monkeypatch, kernel, exprs, X, Y, parsimony=0.125)
    assert len(set(got["nodes"])) >= 4 and got["nodes"][0] == 3
    assert bits_equal(got["fitness"], ref + f32(0.125) * got["nodes"]), (got["fitness"], ref, got["nodes"])
    assert got["fitness"][0] == f32(10000.375)  # (adding before the clip would give 10000)
    # scaled: the raw value is the evaluation's own without parsimony (inside the float64 bound); the constant
    # tree's is known in bits: degenerate, sse = cyy from the exactly rounded sums of y and y y
    raw = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=True)
    within_bound(raw["fitness"], want, Y)
    y64 = Y[:, 0].astype(np.float64)
    sy, syy, n = math.fsum(y64), math.fsum(y64 * y64), float(M)
    assert raw["fitness"][4] == f32(max(syy - sy * sy / n, 0.0) / n) and np.all(raw["fitness"] < f32(MAXF))
    got = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=True, parsimony=0.125)
    assert bits_equal(got["fitness"], raw["fitness"] + f32(0.125) * got["nodes"]), (got["fitness"], raw["fitness"])
    assert bits_equal(got["scale"], raw["scale"])
    # scaled and clipped: the target's noise alone (variance 62500) is above max_fitness for every tree
    Y = (f32(1000.0) * Y).astype(f32)
    assert all(reference(w, Y)[0] == MAXF for w in want)
    got = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=True, parsimony=0.125)
    assert np.array_equal(got["fitness"], f32(MAXF) + f32(0.125) * got["nodes"]), got["fitness"]
    assert np.all(got["fitness"] > f32(MAXF))


@kernels
@sizes
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_target_scores_max_fitness(monkeypatch, kernel, M, scaled, bad):
    """One bad target in output 0 (output 1 is clean): every individual scores max_fitness -- with linear scaling
    too, where cyy is NaN and a clamp written as `sse > 0 ? sse : 0` would turn it into the best score, 0."""
    X, Y, xl = table(kernel, M, 2, lambda X, E: X[:, :2] + f32(0.25) * E)
    Y[5, 0] = bad
    exprs = [["x0", "x1"], [("*", "x0", xl), ("+", "x1", f32(0.5))], [f32(1.5), "x1"], [("-", xl, "x0"), f32(0.0)]]
    got = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=scaled)
    assert bits_equal(got["pred"], values(exprs, X))
    print(kernel, M, scaled, bad, got["fitness"])
    assert np.array_equal(got["fitness"], np.full(len(exprs), MAXF, f32)), got["fitness"]


@kernels
@sizes
@pytest.mark.parametrize("scaled", [False, True])
def test_non_finite_input_and_unused_padding(monkeypatch, kernel, M, scaled):
    X, Y, xl = table(kernel, M, 2, lambda X, E: X[:, :2] + f32(0.25) * E)
    assert xl != "x1"
    exprs = [["x0", "x1"], [("*", "x0", xl), ("+", "x0", f32(0.5))], [("-", xl, "x1"), ("*", "x1", "x1")]]
    clean = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=scaled)
    keys = [k for k in clean if k != "nodes"]
    assert bits_equal(clean["pred"], values(exprs, X)) and np.all(clean["fitness"] < f32(MAXF))
    # a NaN at a valid point: NaN predictions there and max_fitness for the trees that read it, nothing else moves
    Xn = X.copy()
    Xn[7, 0] = np.nan
    got = evaluate(monkeypatch, kernel, exprs, Xn, Y, scaled=scaled)
    assert bits_equal(got["pred"], values(exprs, Xn)) and np.isnan(got["pred"][:2, 0, 7]).all()
    assert np.all(got["fitness"][:2] == f32(MAXF)), got["fitness"]
    assert all(bits_equal(got[k][2], clean[k][2]) for k in keys)
    # NaN in the padding only (M = 70: ld = 72; M = 4097: ld = 4100): read, never used -- the same bits
    ld = (M + 3) // 4 * 4

    def patch(d):
        assert d["ld"] == ld > M and d["xt_dev"].shape[1] == ld == d["yt_dev"].shape[1]
        d["xt_dev"][:, M:] = float("nan")
        d["yt_dev"][:, M:] = float("nan")

    got = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=scaled, patch=patch)
    assert all(bits_equal(got[k], clean[k]) for k in keys) and np.all(np.isfinite(got["fitness"]))


@kernels
@sizes
def test_scaled_one_output_invalid_the_other_clean(monkeypatch, kernel, M):
    X, Y, xl = table(kernel, M, 2, lambda X, E: np.sin(3 * X[:, :1]) + f32(0.25) * E)
    X[3, 0] = 0.0
    exprs = [[("/", f32(1.0), "x0"), ("+", ("*", "x0", f32(2.0)), f32(1.0))], [("/", xl, "x0"), "x0"]]
    want = values(exprs, X)
    assert np.isinf(want[0, 0, 3]) and np.isfinite(want[:, 1]).all()
    got = evaluate(monkeypatch, kernel, exprs, X, Y, scaled=True)
    assert bits_equal(got["pred"], want)
    assert np.array_equal(got["fitness"], np.full(2, MAXF, f32)), got["fitness"]
    y64 = Y.astype(np.float64)
    for p in range(2):
        _, _, a, b, bad, deg = reference(want[p], Y)
        assert bad.tolist() == [True, False] and not deg.any()
        assert np.array_equal(got["scale"][p, 0], f32([math.fsum(y64[:, 0]) / M, 0.0])), got["scale"][p]
        ab = np.array([a[1], b[1]])
        assert np.all(np.abs(got["scale"][p, 1] - ab) <= 2.0 ** -20 * np.abs(ab)), (got["scale"][p], ab)
