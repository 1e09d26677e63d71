"""PointwiseEvaluator(linear_scaling=True) on the GPU against a two-pass centred closed form in float64, within
|fit - ref| <= 2^-22 ref + 2^-40 sum_d (Syy_d + b_d^2 Sff_d) / M: the one f32 rounding, the ~2^-46 sum chains."""
import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd.engine import DeviceEngine
from multitreegp_amd.sampling import sample_population
from helpers import bits_equal
from test_gpu_pointwise import exact_exprs, library, tree, value

pytestmark = pytest.mark.gpu
f32, MAXF = np.float32, 1e4


def reference(f, Y):
    """f [n_out, M] float32, Y [M, n_out] -> (fitness, bound, a, b, invalid, degenerate), the flags per output."""
    f, y, M = f.astype(np.float64), Y.T.astype(np.float64), f.shape[1]
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(f).all(axis=1)
        fc, yc = f - f.mean(axis=1, keepdims=True), y - y.mean(axis=1, keepdims=True)
        cff, cfy, cyy, Sff = (fc * fc).sum(1), (fc * yc).sum(1), (yc * yc).sum(1), (f * f).sum(1)
        deg = ~(cff > 2.0 ** -40 * Sff) & ~bad
        b = np.where(deg | bad, 0.0, cfy / cff)
        a = y.mean(axis=1) - np.where(b == 0.0, 0.0, b * f.mean(axis=1))
        fit = min(np.maximum(cyy - b * cfy, 0.0).sum() / M, MAXF) if not bad.any() else MAXF
        return fit, 2.0 ** -22 * fit + 2.0 ** -40 * ((y * y).sum(1) + b * b * Sff).sum() / M, a, b, bad, deg


def run(lib, pop, X, Y, scaled=True, jit=None, small_buffer=False):
    eng = DeviceEngine(mt.PointwiseEvaluator(MAXF, linear_scaling=scaled), lib, 0.0, "cuda:0", jit=jit)
    if small_buffer:  # a 16-byte code buffer: the kernel sees that the code does not fit and interprets
        arena = eng._arena
        eng._arena = lambda nbytes: (arena(nbytes)[0], 16)
    res = eng.evaluate(torch.from_numpy(pop).cuda(), (X, Y), trajectories=True)
    return [res[k].cpu().numpy() for k in (("fitness", "scale", "pred") if scaled else ("fitness", "pred"))]


def within_bound(fit, f, Y):
    refs = [reference(fp, Y) for fp in f]
    for p, (want, bound, *_) in enumerate(refs):
        print(p, fit[p], want, abs(fit[p] - want), bound)
        assert abs(float(fit[p]) - want) <= bound if want < MAXF else fit[p] == f32(MAXF), (p, fit[p], want, bound)
    return refs


@pytest.mark.parametrize("P", [1, 9])
@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("n_var", [1, 8])
@pytest.mark.parametrize("M", [1, 2, 63, 65, 4096, 4097])
def test_exact_programs(M, n_var, n_out, P):
    m = np.arange(M)[:, None]
    X = (((m * 7 + np.arange(n_var) * 3) % 32 - 16) / 8).astype(f32)
    Y = (((m * 5 + np.arange(n_out)) % 16 - 8) / 4).astype(f32)
    lib = library("+-*", n_var, n_out)
    exprs = [exact_exprs(p, n_var, n_out) for p in range(P)]
    pop = np.stack([np.stack([tree(lib, e) for e in ex]) for ex in exprs])
    fit, scale, pred = run(lib, pop, X, Y)
    want = np.stack([np.stack([value(e, X) for e in ex]) for ex in exprs])
    assert bits_equal(pred, want)
    within_bound(fit, want, Y)
    if M == 1:  # one point: degenerate
        assert not scale[:, :, 1].any() and np.array_equal(scale[:, :, 0], np.tile(Y, (P, 1))) and not fit.any()


@pytest.fixture(scope="module")
def general():
    lib = library(["+", "-", "*", "/", "sin", "cos", "exp", "log", "sqrt", "tanh", "abs"], 3, 2)
    pop = sample_population(23, lib, 16, 1, max_init_depth=4, max_nodes=16)[0]
    out = {}
    for M in (130, 4097):
        rng = np.random.default_rng(5)
        X, Y = rng.uniform(0.25, 2.0, size=(M, 3)).astype(f32), rng.normal(size=(M, 2)).astype(f32)
        out[M] = (X, Y, run(lib, pop, X, Y, jit=True))
    return lib, pop, out


@pytest.mark.parametrize("M", [130, 4097])
def test_general_operators_program_paths_and_unscaled(general, M):
    lib, pop, out = general
    X, Y, (fit, scale, pred) = out[M]
    refs = within_bound(fit, pred, Y)
    valid = np.isfinite(pred).all(axis=(1, 2))
    raw, _ = run(lib, pop, X, Y, scaled=False, jit=True)  # a = 0, b = 1 is admissible: scaling can only help
    assert np.all(fit[valid].astype(np.float64) <= raw[valid].astype(np.float64) * (1 + 2.0 ** -20)), (fit, raw)
    if M == 130:
        assert sum(not (bad.any() or deg.any()) for *_, bad, deg in refs) >= 8
        for kw in (dict(jit=False), dict(jit=True, small_buffer=True)):
            fit2, scale2, pred2 = run(lib, pop, X, Y, **kw)
            assert bits_equal(fit, fit2) and bits_equal(scale, scale2) and bits_equal(pred, pred2)


@pytest.mark.parametrize("case", ["affine", "constant", "pole", "offset"])
def test_edges(case):
    lib = library(["+", "*", "/"], 1, 1)
    X = (np.arange(70, dtype=f32)[:, None] - 35) / 8 if case != "offset" else np.linspace(-1, 1, 70, dtype=f32)[:, None]
    expr = {"affine": ("+", ("*", "x0", "x0"), "x0"), "constant": f32(1.5), "pole": ("/", f32(1.0), "x0"),
            "offset": ("+", "x0", f32(4096.0))}[case]
    Y = np.sin(3 * X).astype(f32)
    if case == "affine":
        Y = (2 - 3 * (X * X + X)).astype(f32)  # exact: multiples of 1/64 below 2^7
    fit, scale, pred = run(lib, tree(lib, expr)[None, None], X, Y)
    (want, bound, a, b, bad, deg), = within_bound(fit, pred, Y)
    assert (bad[0], deg[0]) == (case == "pole", case == "constant")
    assert {"affine": fit[0] <= bound and np.all(np.abs(scale[0, 0] - [2, -3]) <= 2.0 ** -20 * np.array([2, 3])),
            "constant": scale[0, 0, 1] == 0 and abs(want - Y.astype(np.float64).var()) <= bound,
            "pole": fit[0] == f32(MAXF), "offset": scale[0, 0, 1] != 0}[case]


@pytest.mark.parametrize("backend", ["native", "device"])
def test_through_genetic_programming(backend):
    X = np.random.default_rng(2).uniform(-1, 1, size=(100, 2)).astype(f32)
    Y = (f32(3.0) * X[:, :1] * X[:, 1:] + f32(0.5)).astype(f32)
    ops = [("+", None, 2, 0.5), ("-", None, 2, 0.1), ("*", None, 2, 0.5), ("sin", None, 1, 0.1)]
    ff = mt.PointwiseEvaluator(MAXF, linear_scaling=True)
    gp = mt.GeneticProgramming(3, 40, ff, ops, [["x0", "x1"]], [1], max_nodes=16, size_parsinomy=0.01, verbose=False,
                               evolve_backend=backend, device="cuda:0")
    pops = gp.initialize_population(7)
    for g in range(2):
        fit, pops = gp.evaluate_population(pops, (X, Y))
        flat = torch.as_tensor(pops).reshape(40, 1, 16, 4).float().cuda()
        raw = DeviceEngine(ff, gp.library, 0.0, "cuda:0").evaluate(flat, (X, Y))["fitness"].cpu().numpy()
        nodes = (flat[..., 0] != 0).sum(dim=(1, 2)).cpu().numpy().astype(f32)
        got = torch.as_tensor(fit).cpu().numpy().reshape(-1)
        assert np.array_equal(got, raw + f32(0.01) * nodes) and np.all(np.isfinite(got))
        assert gp.best_fitnesses[g] == got.min()  # best tracking ran
        pops = gp.evolve(pops, fit, g + 11)
