"""Program paths of the pointwise kernels that nothing else runs: unchained register-data code (MTGP_JIT_CHAIN=0:
pw_run's one call per output), the forced wide kernel on tables of 1 and 3 columns (fewer 16-byte pieces than
threads), and the general operators against the oracle's tree walk instead of another GPU kernel."""
import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd.engine import DeviceEngine
from multitreegp_amd.sampling import sample_population
from oracle import oracle as orc
from helpers import bits_equal
from test_gpu_pointwise import general as general_narrow  # noqa: F401  (fixtures: 3 and 12 columns, P = 16, M = 130)
from test_gpu_pointwise import library, tree
from test_gpu_pointwise_wide import general as general_wide  # noqa: F401

pytestmark = pytest.mark.gpu
f32, MAXF = np.float32, 1e4
GENERAL_OPS = ["+", "-", "*", "/", "sin", "cos", "exp", "log", "sqrt", "tanh", "abs"]  # test_gpu_pointwise.general's


def run(lib, pop, X, Y, scaled, jit=True):
    eng = DeviceEngine(mt.PointwiseEvaluator(MAXF, linear_scaling=scaled), lib, 0.0, "cuda:0", jit=jit)
    res = eng.evaluate(torch.from_numpy(pop).cuda(), (X, Y), trajectories=True)
    torch.cuda.synchronize()
    fl = res["_flat"]
    assert DeviceEngine.jit_ok(fl) == jit
    return eng, fl, [res[k].cpu().numpy() for k in ("fitness", "pred") + (("scale",) if scaled else ())]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n_out", [2, 4])
def test_unchained_code_gives_the_chained_and_interpreted_bits(monkeypatch, n_out, scaled):
    n_var, P, M = 3, 16, 130
    lib = library(GENERAL_OPS, n_var, n_out)
    pop = sample_population(3, lib, P, 1, max_init_depth=4, max_nodes=16)[0]
    rng = np.random.default_rng(5)
    X, Y = rng.normal(size=(M, n_var)).astype(f32), rng.normal(size=(M, n_out)).astype(f32)
    monkeypatch.delenv("MTGP_PW_WIDE", raising=False)
    monkeypatch.delenv("MTGP_JIT_CHAIN", raising=False)
    eng, fl, chained = run(lib, pop, X, Y, scaled)
    assert not eng._pointwise_wide() and fl.jit[4].next == (1 << (n_out - 1)) - 1
    _, _, interpreted = run(lib, pop, X, Y, scaled, jit=False)
    monkeypatch.setenv("MTGP_JIT_CHAIN", "0")
    eng, fl, unchained = run(lib, pop, X, Y, scaled)
    assert not eng._pointwise_wide() and eng._jit_mode() == nat.JIT_MODE_REGS and fl.jit[4].next == 0
    assert np.isfinite(chained[0]).all() and (chained[0] < f32(MAXF)).sum() >= P // 4  # not all at the ceiling
    for a, b, c in zip(chained, unchained, interpreted):
        assert bits_equal(a, b) and bits_equal(a, c)


def small_exprs(p, n_var, n_out):
    c, xl = f32(0.25 * (p % 5 + 1)), f"x{n_var - 1}"
    return [("+", ("*", "x0", "x0"), c), ("-", ("*", xl, f32(1.5)), "x0"), ("*", ("+", "x0", c), ("-", xl, f32(2.0))),
            ("-", c, ("*", xl, ("+", "x0", xl)))][:n_out]


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n_out", [1, 4])
@pytest.mark.parametrize("n_var", [1, 3])
@pytest.mark.parametrize("M", [1, 257, 4097])
def test_forced_wide_kernel_at_small_width_gives_the_narrow_bits(monkeypatch, M, n_var, n_out, scaled):
    P = 9
    rng = np.random.default_rng(13)
    X, Y = rng.normal(size=(M, n_var)).astype(f32), rng.normal(size=(M, n_out)).astype(f32)
    lib = library("+-*", n_var, n_out)
    pop = np.stack([np.stack([tree(lib, e) for e in small_exprs(p, n_var, n_out)]) for p in range(P)])
    monkeypatch.delenv("MTGP_PW_WIDE", raising=False)
    eng, _, narrow = run(lib, pop, X, Y, scaled)
    assert not eng._pointwise_wide()
    monkeypatch.setenv("MTGP_PW_WIDE", "1")
    eng, fl, wide = run(lib, pop, X, Y, scaled)
    assert eng._pointwise_wide() and eng._jit_mode() == nat.JIT_MODE_LDS and fl.jit[4].next == 0
    assert np.isfinite(narrow[0]).all()
    for a, b in zip(narrow, wide):
        assert bits_equal(a, b)


@pytest.mark.parametrize("columns", [3, 12])
def test_general_operators_match_the_oracle_tree_walk(columns, general_narrow, general_wide):
    """pred of the `general` populations against oracle.eval_tree per individual, tree and point (NaNs match NaNs)."""
    lib, pop, X, Y, (_, _, pred, *_) = general_narrow if columns == 3 else general_wide
    assert X.shape[1] == columns and pred.shape == (16, 2, 130)
    want = np.empty_like(pred)
    for p, t, m in np.ndindex(*pred.shape):
        want[p, t, m] = orc.eval_tree(pop[p, t], lib.fn_codes, lib.n_funcs, lib.var_start, X[m])
    assert np.isfinite(want).mean() > 0.5
    assert bits_equal(pred, want), np.argwhere(~((pred.view(np.uint32) == want.view(np.uint32)) | np.isnan(want)))[:8]
