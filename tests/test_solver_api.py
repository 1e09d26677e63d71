"""The fixed-step solver family at the Python surface: Heun, Midpoint, Ralston, Bosh3 as classes and
strings, their MTGP_SOLVER_* codes, the refusals (adaptive use, coefficient optimisation)."""
import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd import evaluators as ev
from multitreegp_amd.coefficients import CoefficientOptimiser

NEW = [("Heun", "heun", 3), ("Midpoint", "midpoint", 4), ("Ralston", "ralston", 5), ("Bosh3", "bosh3", 6)]


def test_abi_version_and_codes():
    assert nat.ABI_VERSION == 24
    assert (nat.SOLVER_RK4, nat.SOLVER_DOPRI5, nat.SOLVER_EULER) == (0, 1, 2)
    assert (nat.SOLVER_HEUN, nat.SOLVER_MIDPOINT, nat.SOLVER_RALSTON, nat.SOLVER_BOSH3) == (3, 4, 5, 6)


@pytest.mark.parametrize("cls,kind,code", NEW)
def test_classes_exported_and_checked(cls, kind, code):
    assert getattr(mt, cls) is getattr(ev, cls) and cls in ev.__all__
    obj = getattr(mt, cls)()
    assert obj.name == cls and repr(obj) == f"{cls}()"
    for controller in (None, mt.ConstantStepSize()):
        assert ev._check_solver(obj, controller) == kind
        assert ev._check_solver(obj, controller, adaptive_ok=True) == kind
        assert ev._check_solver(kind, controller) == kind
        assert ev._check_solver(cls, controller) == kind
    with pytest.raises(NotImplementedError):
        ev._check_solver(obj, mt.PIDController(rtol=1e-4, atol=1e-4), adaptive_ok=True)
    with pytest.raises(NotImplementedError):
        ev._check_solver(kind, mt.PIDController(rtol=1e-4, atol=1e-4), adaptive_ok=True)
    assert ev._solver_fields(kind, None, 77)["solver"] == code


def test_old_kinds_unchanged():
    assert ev._check_solver(mt.RK4(), None) == "rk4" and ev._check_solver("euler", mt.ConstantStepSize()) == "euler"
    assert ev._solver_fields("rk4", None, 5)["solver"] == 0 and ev._solver_fields("euler", None, 5)["solver"] == 2
    with pytest.raises(NotImplementedError):
        ev._check_solver(mt.Dopri5(), mt.ConstantStepSize(), adaptive_ok=True)
    with pytest.raises(NotImplementedError):
        ev._check_solver("tsit5", None)


@pytest.mark.parametrize("cls,kind,code", NEW)
def test_prepare_yields_code_and_the_same_grid(cls, kind, code):
    solver = getattr(mt, cls)()
    env = mt.HarmonicOscillator(0.0, 0.0)
    data = mt.control_data(env, 3, 0.05, None, seed=1, n_steps=40, mode="Different")
    ts = np.asarray(data[1], np.float32)
    n_grid = len(ev.constant_step_grid(ts, 0.05, 16 ** 4)) - 1
    makers = (lambda s, **kw: mt.FeedforwardEvaluator(env, 0.05, solver=s, **kw),
              lambda s, **kw: mt.DynamicEvaluator(env, 2, 0.05, solver=s, **kw),
              lambda s, **kw: mt.DynamicEvaluator(env, 5, 0.05, solver=s, **kw))
    for i, make in enumerate(makers):
        ff = make(solver) if i < 2 else make(kind, stepsize_controller=mt.ConstantStepSize())
        assert ff.solver_kind == kind
        d = ff.prepare(data)
        ref = make(mt.RK4()).prepare(data)
        assert d["solver"] == code and d["max_steps"] == 16 ** 4
        assert (d["n_steps"], d["save_every"], d["n_save"]) == (ref["n_steps"], ref["save_every"], ref["n_save"])
        assert d["n_steps"] == n_grid
        assert (d["rtol"], d["atol"], d["dtmin"], d["dtmax"]) == (0.0, 0.0, 0.0, 0.0)
    sr = mt.SREvaluator(solver=solver, dt0=0.05)
    assert sr.solver_kind == kind
    x0 = np.array([[1.0, 0.0]], np.float32)
    ts = (np.arange(11, dtype=np.float32) * np.float32(0.2)).astype(np.float32)
    d = sr.prepare((x0, ts, np.zeros((1, 11, 2), np.float32), np.zeros((1, 2), np.uint32)))
    assert d["solver"] == code and d["n_steps"] == len(ev.constant_step_grid(ts, 0.05, 16 ** 4)) - 1
    with pytest.raises(NotImplementedError):
        mt.SREvaluator(solver=solver, dt0=0.05, stepsize_controller=mt.PIDController(rtol=1e-4, atol=1e-4))


@pytest.mark.parametrize("cls,kind,code", NEW)
def test_coefficient_optimiser_refuses(cls, kind, code):
    ff = mt.SREvaluator(solver=getattr(mt, cls)(), dt0=0.05)
    with pytest.raises(NotImplementedError, match=kind):
        CoefficientOptimiser.check_evaluator(ff)
    CoefficientOptimiser.check_evaluator(mt.SREvaluator(solver=mt.RK4(), dt0=0.05))
