"""PointwiseEvaluator(wide=True) on the GPU: k_pointwise_wide (tables of 9 .. 64 columns, the data vector in LDS
for LDS-data JIT code) against the references of test_gpu_pointwise / test_gpu_pointwise_scaled, and against
k_pointwise itself (MTGP_PW_WIDE=1 at 8 columns)."""
import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd.engine import DeviceEngine
from multitreegp_amd.sampling import sample_population
from helpers import bits_equal
from test_gpu_pointwise import fitness_ref, library, tree, value
from test_gpu_pointwise_scaled import within_bound

pytestmark = pytest.mark.gpu
f32, MAXF = np.float32, 1e4


def run(lib, pop, X, Y, scaled=False, jit=None, small_buffer=False):
    """As test_gpu_pointwise.run with wide=True -> (engine, fitness, pred, flattened, scale or None)."""
    eng = DeviceEngine(mt.PointwiseEvaluator(MAXF, linear_scaling=scaled, wide=True), lib, 0.0, "cuda:0", jit=jit)
    if small_buffer:  # a 16-byte code buffer: the kernel sees that the code does not fit and interprets
        arena = eng._arena
        eng._arena = lambda nbytes: (arena(nbytes)[0], 16)
    res = eng.evaluate(torch.from_numpy(pop).cuda(), (X, Y), trajectories=True)
    torch.cuda.synchronize()
    if eng.use_jit:
        assert DeviceEngine.jit_ok(res["_flat"]) == (not small_buffer)
    scale = res["scale"].cpu().numpy() if scaled else None
    return eng, res["fitness"].cpu().numpy(), res["pred"].cpu().numpy(), res["_flat"], scale


def dyadic(M, n_var, n_out):
    """X: multiples of 1/8 in [-2, 2), Y: multiples of 1/4 in [-2, 2), as the narrow tests'."""
    m = np.arange(M)[:, None]
    return ((((m * 7 + np.arange(n_var) * 3) % 32 - 16) / 8).astype(f32),
            (((m * 5 + np.arange(n_out)) % 16 - 8) / 4).astype(f32))


def wide_exprs(p, n_var, n_out):
    """Exact in f32: the left-deep sum of every x_k (all slots, stack depth 2; |sum| < 128), a tree on the first
    and the last slot, then slots around the 16 preloads."""
    total = "x0"
    for k in range(1, n_var):
        total = ("+", total, f"x{k}")
    c, xl, xm = f32(0.25 * (p % 5 + 1)), f"x{n_var - 1}", f"x{min(16, n_var - 1)}"
    return [total, ("-", ("*", xl, f32(1.5)), "x0"), ("*", ("+", xm, c), ("-", xl, f32(2.0))),
            ("+", ("*", "x8", xl), c)][:n_out]


def population(lib, P, n_var, n_out, N=128):
    exprs = [wide_exprs(p, n_var, n_out) for p in range(P)]
    return exprs, np.stack([np.stack([tree(lib, e, N) for e in ex]) for ex in exprs])


@pytest.mark.parametrize("P", [1, 9])
@pytest.mark.parametrize("n_out", [1, 4])
@pytest.mark.parametrize("n_var", [9, 17, 64])
@pytest.mark.parametrize("M", [1, 65, "tile+1", 4097])
def test_exact_programs_bitexact_and_within_f64_bound(M, n_var, n_out, P):
    if M == "tile+1":  # chunks per tile: the largest of 4, 2, 1 within 64 KB of LDS
        M = 64 * next(T for T in (4, 2, 1) if 2 * T * (n_var + n_out) * 256 + 16384 <= 65536 or T == 1) + 1
    X, Y = dyadic(M, n_var, n_out)
    lib = library("+-*", n_var, n_out)
    exprs, pop = population(lib, P, n_var, n_out)
    _, fit, pred, _, _ = run(lib, pop, X, Y)
    want = np.stack([np.stack([value(e, X) for e in ex]) for ex in exprs])
    assert bits_equal(pred, want)
    ref = np.array([fitness_ref(w, Y) for w in want])
    assert bits_equal(fit, ref), (fit, ref)
    W = -(-M // 4096)  # the bound of test_gpu_pointwise: its derivation does not involve n_var
    A = (-(-min(M, 4096) // 64) - 1) + 6 + (W - 1).bit_length() + n_out
    ref64 = ((want.astype(np.float64) - Y.T.astype(np.float64)) ** 2).sum(axis=(1, 2)) / M
    assert np.all(np.abs(fit - ref64) <= (A + 2) * 2.0 ** -24 * ref64), (fit, ref64)


@pytest.fixture(scope="module")
def general():
    n_var, n_out, P, M = 12, 2, 16, 130
    lib = library(["+", "-", "*", "/", "sin", "cos", "exp", "log", "sqrt", "tanh", "abs"], n_var, n_out)
    pop = sample_population(3, lib, P, 1, max_init_depth=4, max_nodes=16)[0]
    rng = np.random.default_rng(5)
    X, Y = rng.normal(size=(M, n_var)).astype(f32), rng.normal(size=(M, n_out)).astype(f32)
    return lib, pop, X, Y, run(lib, pop, X, Y, jit=True)


def test_general_operators_match_eval_programs(general):
    lib, pop, X, Y, (eng, fit, pred, fl, _) = general
    want = eng.eval_programs(fl, torch.from_numpy(X).cuda()).cpu().numpy()
    assert bits_equal(pred, want)
    ref = np.array([fitness_ref(w, Y) for w in want])
    assert bits_equal(fit, ref), (fit, ref)


@pytest.mark.parametrize("path", ["interpreter", "small_buffer"])
def test_program_paths_give_identical_bits(general, path):
    lib, pop, X, Y, (_, fit, pred, _, _) = general
    _, fit2, pred2, _, _ = run(lib, pop, X, Y, jit=path != "interpreter", small_buffer=path == "small_buffer")
    assert bits_equal(fit, fit2) and bits_equal(pred, pred2)


@pytest.mark.parametrize("scaled", [False, True])
def test_wide_kernel_gives_the_narrow_kernels_bits(monkeypatch, scaled):
    n_var, n_out, M, P = 8, 3, 4097, 9
    X, Y = dyadic(M, n_var, n_out)
    lib = library("+-*", n_var, n_out)
    _, pop = population(lib, P, n_var, n_out)
    monkeypatch.delenv("MTGP_PW_WIDE", raising=False)
    _, fit, pred, _, scale = run(lib, pop, X, Y, scaled=scaled)
    monkeypatch.setenv("MTGP_PW_WIDE", "1")
    eng, fit2, pred2, fl, scale2 = run(lib, pop, X, Y, scaled=scaled)
    assert eng._jit_mode() == nat.JIT_MODE_LDS and fl.jit[4].next == 0  # the wide kernel's code
    assert bits_equal(fit, fit2) and bits_equal(pred, pred2) and (not scaled or bits_equal(scale, scale2))


@pytest.mark.parametrize("n_out", [1, 4])
@pytest.mark.parametrize("M", [65, 4097])
def test_scaled_against_float64_closed_form(M, n_out):
    n_var, P = 17, 9
    X, Y = dyadic(M, n_var, n_out)
    lib = library("+-*", n_var, n_out)
    exprs, pop = population(lib, P, n_var, n_out)
    _, fit, pred, _, scale = run(lib, pop, X, Y, scaled=True)
    want = np.stack([np.stack([value(e, X) for e in ex]) for ex in exprs])
    assert bits_equal(pred, want)
    for p, (_, _, a, b, bad, deg) in enumerate(within_bound(fit, want, Y)):
        ab = np.stack([a, b], axis=1)  # (2^-20 relative: the bound of test_gpu_pointwise_scaled.test_edges)
        assert not bad.any() and not deg.any() and np.all(np.abs(scale[p] - ab) <= 2.0 ** -20 * np.abs(ab)), (p, scale[p], ab)


@pytest.mark.parametrize("backend", ["native", "device"])
def test_through_genetic_programming(backend):
    X = np.random.default_rng(2).uniform(-1, 1, size=(100, 12)).astype(f32)
    Y = (X[:, :1] * X[:, 11:] + f32(0.5)).astype(f32)
    ops = [("+", None, 2, 0.5), ("-", None, 2, 0.1), ("*", None, 2, 0.5), ("sin", None, 1, 0.1)]
    ff = mt.PointwiseEvaluator(MAXF, wide=True)
    gp = mt.GeneticProgramming(3, 40, ff, ops, [[f"x{k}" for k in range(12)]], [1], max_nodes=16, size_parsinomy=0.01,
                               verbose=False, evolve_backend=backend, device="cuda:0")
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
