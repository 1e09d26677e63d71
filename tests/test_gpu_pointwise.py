"""PointwiseEvaluator on the GPU: k_pointwise against a literal float32 restatement of include/mtgp.h's
reduction order, float64, eval_programs, on its three program paths, and through GeneticProgramming."""
import functools

import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd.engine import DeviceEngine
from multitreegp_amd.sampling import sample_population
from helpers import bits_equal

pytestmark = pytest.mark.gpu
f32, MAXF = np.float32, 1e4


def fitness_ref(pred, Y, max_fitness=MAXF, left_fold=False):
    """The spec in np.float32: pred [n_out, M], Y [M, n_out] -> clipped fitness (no parsimony).
    left_fold: the span sums added one after the other instead -- NOT the spec: the order that
    test_pointwise_reference.py requires the span tests' inputs to tell from the right one."""
    e = pred[0] - Y[:, 0]
    sq = e * e
    for d in range(1, pred.shape[0]):
        e = pred[d] - Y[:, d]
        sq = sq + e * e
    parts = []
    for s in range(0, len(sq), 4096):  # one wave per span
        span = sq[s:s + 4096]
        rows = -(-len(span) // 64)
        pad = np.zeros(rows * 64, f32)
        pad[:len(span)] = span
        pad, has = pad.reshape(rows, 64), (np.arange(rows * 64) < len(span)).reshape(rows, 64)
        lane = pad[0].copy()  # the first term; +0 in a lane without a point
        for r in range(1, rows):
            lane = np.where(has[r], lane + pad[r], lane)
        for w in (1, 2, 4, 8, 16, 32):  # xor butterfly
            lane = lane + lane[np.arange(64) ^ w]
        parts.append(lane[0])
    v = np.array(parts + [0.0] * ((1 << (len(parts) - 1).bit_length()) - len(parts)), f32)
    if left_fold:
        v = np.array([functools.reduce(lambda a, b: a + b, parts)], f32)
    while len(v) > 1:  # span sums pairwise in span order
        v = v[0::2] + v[1::2]
    with np.errstate(all="ignore"):
        mean = v[0] / f32(len(sq))
    mean = f32(max_fitness) if not np.isfinite(mean) else mean
    return f32(min(max(mean, f32(0)), f32(max_fitness)))


def library(ops, n_var, n_out):
    return mt.NodeLibrary([(o, None, 1 if len(o) > 1 else 2, 0.1) for o in ops],
                          [[f"x{k}" for k in range(n_var)]], [n_out])


def tree(lib, expr, N=16):
    """Nested tuples (op, child[, child]) / variable names / constants -> [N, 4] rows, root last."""
    rows = []

    def walk(e):
        if isinstance(e, tuple):
            kids = [walk(k) for k in e[1:]] + [-1]
            rows.append((lib.string_to_node[e[0]], kids[0], kids[1], 0.0))
        elif isinstance(e, str):
            rows.append((lib.string_to_node[e], -1, -1, 0.0))
        else:
            rows.append((1, -1, -1, e))
        return len(rows) - 1

    walk(expr)
    out, s = np.tile(f32([0, -1, -1, 0]), (N, 1)), N - len(rows)
    for i, (f, a, b, v) in enumerate(rows):
        out[s + i] = (f, a + s if a >= 0 else -1, b + s if b >= 0 else -1, v)
    return out


def value(expr, X):
    if isinstance(expr, tuple):
        a, b = value(expr[1], X), value(expr[2], X)
        if expr[0] == "/":  # IEEE division, as the kernels' (x / 0 = +-inf, 0 / 0 = NaN)
            with np.errstate(all="ignore"):
                return a / b
        return a + b if expr[0] == "+" else a - b if expr[0] == "-" else a * b
    return X[:, int(expr[1:])] if isinstance(expr, str) else np.full(len(X), expr, f32)


def exact_exprs(p, n_var, n_out):
    """Output trees of individual p from + - * on dyadic values: every f_d(x_m) and e_d is exact."""
    c, xl = f32(0.25 * (p % 5 + 1)), f"x{n_var - 1}"
    return [("+", ("*", "x0", "x0"), c), ("-", ("*", xl, f32(1.5)), "x0"),
            ("*", ("+", "x0", c), ("-", xl, f32(2.0)))][:n_out]


def run(lib, pop, X, Y, parsimony=0.0, jit=None, small_buffer=False):
    eng = DeviceEngine(mt.PointwiseEvaluator(MAXF), lib, parsimony, "cuda:0", jit=jit)
    if small_buffer:  # a 16-byte code buffer: the kernel sees that the code does not fit and interprets
        arena = eng._arena
        eng._arena = lambda nbytes: (arena(nbytes)[0], 16)
    res = eng.evaluate(torch.from_numpy(pop).cuda(), (X, Y), trajectories=True)
    torch.cuda.synchronize()
    if eng.use_jit:
        assert DeviceEngine.jit_ok(res["_flat"]) == (not small_buffer)
    return eng, res["fitness"].cpu().numpy(), res["pred"].cpu().numpy(), res["_flat"]


@pytest.mark.parametrize("P", [1, 9])
@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("n_var", [1, 8])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 4096, 4097])
def test_exact_programs_bitexact_and_within_f64_bound(M, n_var, n_out, P):
    m = np.arange(M)[:, None]
    X = (((m * 7 + np.arange(n_var) * 3) % 32 - 16) / 8).astype(f32)
    Y = (((m * 5 + np.arange(n_out)) % 16 - 8) / 4).astype(f32)
    lib = library("+-*", n_var, n_out)
    exprs = [exact_exprs(p, n_var, n_out) for p in range(P)]
    pop = np.stack([np.stack([tree(lib, e) for e in ex]) for ex in exprs])
    _, fit, pred, _ = run(lib, pop, X, Y)
    want = np.stack([np.stack([value(e, X) for e in ex]) for ex in exprs])
    assert bits_equal(pred, want)
    ref = np.array([fitness_ref(w, Y) for w in want])
    assert bits_equal(fit, ref), (fit, ref)
    # f32 additions on the longest path: lane chain, butterfly, span tree, outputs; + product and division
    W = -(-M // 4096)
    A = (-(-min(M, 4096) // 64) - 1) + 6 + (W - 1).bit_length() + n_out
    ref64 = ((want.astype(np.float64) - Y.T.astype(np.float64)) ** 2).sum(axis=(1, 2)) / M
    assert np.all(np.abs(fit - ref64) <= (A + 2) * 2.0 ** -24 * ref64), (fit, ref64)


@pytest.fixture(scope="module")
def general():
    n_var, n_out, P, M = 3, 2, 16, 130
    lib = library(["+", "-", "*", "/", "sin", "cos", "exp", "log", "sqrt", "tanh", "abs"], n_var, n_out)
    pop = sample_population(3, lib, P, 1, max_init_depth=4, max_nodes=16)[0]
    rng = np.random.default_rng(5)
    X, Y = rng.normal(size=(M, n_var)).astype(f32), rng.normal(size=(M, n_out)).astype(f32)
    return lib, pop, X, Y, run(lib, pop, X, Y, jit=True)


def test_general_operators_match_eval_programs(general):
    lib, pop, X, Y, (eng, fit, pred, fl) = general
    want = eng.eval_programs(fl, torch.from_numpy(X).cuda()).cpu().numpy()
    assert bits_equal(pred, want)
    ref = np.array([fitness_ref(w, Y) for w in want])
    assert bits_equal(fit, ref), (fit, ref)


@pytest.mark.parametrize("path", ["interpreter", "small_buffer"])
def test_program_paths_give_identical_bits(general, path):
    lib, pop, X, Y, (_, fit, pred, _) = general
    _, fit2, pred2, _ = run(lib, pop, X, Y, jit=path != "interpreter", small_buffer=path == "small_buffer")
    assert bits_equal(fit, fit2) and bits_equal(pred, pred2)


def test_edge_values():
    lib = library(["/", "sin"], 1, 1)
    pop = np.stack([tree(lib, ("/", f32(1.0), "x0"))[None], tree(lib, ("sin", "x0"))[None]])
    X, Y = np.linspace(0.5, 2.0, 70, dtype=f32)[:, None], np.zeros((70, 1), f32)
    X[3, 0], X[68, 0] = 0.0, 3e5  # 1 / 0 at one point; a slow-reduction sin argument at another
    _, fit, pred, _ = run(lib, pop, X, Y, jit=True)
    assert fit[0] == f32(MAXF) and np.isinf(pred[0, 0, 3])
    _, fit2, pred2, _ = run(lib, pop, X, Y, jit=False)
    assert bits_equal(fit, fit2) and bits_equal(pred, pred2)


@pytest.mark.parametrize("backend", ["native", "device"])
def test_through_genetic_programming(backend):
    X = np.random.default_rng(2).uniform(-1, 1, size=(100, 2)).astype(f32)
    Y = (X[:, :1] * X[:, 1:] + f32(0.5)).astype(f32)
    ops = [("+", None, 2, 0.5), ("-", None, 2, 0.1), ("*", None, 2, 0.5), ("sin", None, 1, 0.1)]
    gp = mt.GeneticProgramming(3, 40, mt.PointwiseEvaluator(MAXF), ops, [["x0", "x1"]], [1], max_nodes=16,
                               size_parsinomy=0.01, verbose=False, evolve_backend=backend, device="cuda:0")
    pops = gp.initialize_population(7)
    for g in range(2):
        fit, pops = gp.evaluate_population(pops, (X, Y))
        flat = torch.as_tensor(pops).reshape(40, 1, 16, 4).float().cuda()
        eng = DeviceEngine(mt.PointwiseEvaluator(MAXF), gp.library, 0.0, "cuda:0")
        raw = eng.evaluate(flat, (X, Y))["fitness"].cpu().numpy()
        nodes = (flat[..., 0] != 0).sum(dim=(1, 2)).cpu().numpy().astype(f32)
        got = torch.as_tensor(fit).cpu().numpy().reshape(-1)
        assert np.array_equal(got, raw + f32(0.01) * nodes) and np.all(np.isfinite(got))
        assert gp.best_fitnesses[g] == got.min()  # best tracking ran
        pops = gp.evolve(pops, fit, g + 11)
