"""Coefficient optimisation of dynamic policies with state_size 4..16 (mtgp.h ABI v21): the host
side.  CoefficientOptimiser.check_evaluator and GeneticProgramming(coefficient_optimisation=True)
accept the wide states, and the inputs of the GPU tests (tests/test_gpu_ctl_grad_wide.py) are
pinned by the oracle alone: every case differentiates without an error and moves at least five
candidates, so the bit-exact comparison there is never a comparison of zeros.

`wide_case` builds a case and its oracle reference once; the GPU tests share it.
"""
import functools

import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import coefficients as co
from oracle import oracle as orc

from helpers import CONTROL_OPS, dynamic_setup, oracle_model, oracle_rollouts

DOPRI5 = (1e-4, 1e-4, 0.001, 600)  # rtol, atol, dtmin, max_steps

# (env, state_size, solver, obs_noise): run-time state sizes at both ends and odd ones, every
# environment's n_var / parameter count, both solver templates, noise on and off, two parameter
# chunks (acrobot / 16)
WIDE_CASES = [("acrobot", 4, "rk4", 0.0), ("acrobot", 8, "rk4", 0.1), ("acrobot", 16, "rk4", 0.0),
              ("harmonic", 16, "rk4", 0.1), ("reactor", 6, "rk4", 0.0), ("acrobot", 5, "euler", 0.1),
              ("harmonic", 9, "euler", 0.0), ("acrobot", 4, "dopri5", 0.0), ("acrobot", 12, "dopri5", 0.1),
              ("harmonic", 16, "dopri5", 0.0)]


def wide_setup(env, state_size, solver, noise, P=12, R=6):
    e, lib, ff, data, pop = dynamic_setup(P=P, R=R, n_steps=30, depth=5, N=30, seed=11, state_size=state_size,
                                          obs_noise=noise, env=env, solver=DOPRI5 if solver == "dopri5" else None)
    if solver == "euler":
        ff = mt.DynamicEvaluator(e, state_size, ff.dt0, solver=mt.Euler())
    return lib, ff, data, pop


def oracle_reference(lib, ff, data, pop):
    """(loss [P], grad [P, K], rows) of the oracle on the evaluator's prepared data."""
    d = ff.prepare(data)
    return orc.ctl_grad(oracle_model(ff, d), pop, lib, oracle_rollouts(d))


@functools.lru_cache(maxsize=None)
def wide_case(env, state_size, solver, noise):
    """One case of WIDE_CASES with its oracle reference, computed once per session (read-only)."""
    lib, ff, data, pop = wide_setup(env, state_size, solver, noise)
    loss, grad, rows = oracle_reference(lib, ff, data, pop)
    for a in (pop, loss, grad):
        a.setflags(write=False)
    return lib, ff, data, pop, loss, grad, rows


def moved(grad):
    """Candidates with a non-zero gradient entry (NaN counts: it is not zero)."""
    return int(sum(np.count_nonzero(g) > 0 for g in grad))


@pytest.mark.parametrize("state_size,solver", [(4, "rk4"), (16, "rk4"), (8, "dopri5")])
def test_check_evaluator_accepts_wide_states(state_size, solver):
    kw = dict(solver=mt.RK4()) if solver == "rk4" else dict(
        solver=mt.Dopri5(), max_steps=600, stepsize_controller=mt.PIDController(rtol=1e-4, atol=1e-4, dtmin=0.001))
    ff = mt.DynamicEvaluator(mt.Acrobot(0.0, 0.0), state_size, 0.05, **kw)
    co.CoefficientOptimiser.check_evaluator(ff)


def test_genetic_programming_constructs_with_a_wide_state():
    e, lib, ff, data, pop = dynamic_setup(P=8, R=2, n_steps=10, depth=3, N=16, seed=2, state_size=8)
    # (population 8 needs a migration / elite share that gives whole, even counts: the constructor
    # asserts that before it reaches the evaluator check)
    gp = mt.GeneticProgramming(20, 8, ff, CONTROL_OPS, lib.variable_list, [8, 1], max_nodes=16,
                               migration_percentage=0.5, elite_percentage=0.0, coefficient_optimisation=True,
                               verbose=False)
    assert gp.coefficient_optimisation


@pytest.mark.parametrize("env,state_size,solver,noise", WIDE_CASES)
def test_oracle_differentiates_the_gpu_cases(env, state_size, solver, noise):
    lib, ff, data, pop, loss, grad, rows = wide_case(env, state_size, solver, noise)
    assert loss.shape == (pop.shape[0],) and not np.isnan(loss).any()
    assert moved([grad[p, : len(r)] for p, r in enumerate(rows)]) >= 5
