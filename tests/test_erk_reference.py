"""The tableau-driven numpy restatement of the fixed-step explicit Runge-Kutta solvers
(tests/np_reference_erk.py), which pins the Heun / Midpoint / Ralston / Bosh3 kernels: tied to the
pinned Euler / RK4 restatement bit for bit, of the published orders, its tableaus distinguishable,
Bosh3 really FSAL."""
import numpy as np
import pytest

import np_reference as npr
import np_reference_erk as erk
from test_oracle import CS_GRIDS

f = np.float32

# rhs(t, s) on arrays of either precision; every constant is exact in float32
SYSTEMS = {
    "linear": (lambda t, s: np.array([s[1], s.dtype.type(0) - s[0]], s.dtype), (1.0, 0.0)),
    "vanderpol": (lambda t, s: np.array([s[1], s.dtype.type(0.5) * ((s.dtype.type(1) - s[0] * s[0]) * s[1]) - s[0]],
                                        s.dtype), (0.3, -0.7)),
    "blowup": (lambda t, s: np.array([s[0] * s[0], s[1]], s.dtype), (3.0, 1.0)),
}


def _event(s):
    return not np.all(np.isfinite(s))


def _same_bits(a, b):
    a, b = np.asarray(a, f), np.asarray(b, f)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("system", sorted(SYSTEMS))
@pytest.mark.parametrize("grid", sorted(CS_GRIDS))
def test_anchor_euler_and_rk4_equal_cs_solve(grid, system):
    """(a) with the euler and rk4 tableaus erk_solve is np_reference.cs_solve bit for bit in float32,
    the event's +inf fill included (the blow-up ends early on every grid that reaches t ~ 1/3)."""
    ts, dt0 = CS_GRIDS[grid]
    rhs, s0 = SYSTEMS[system]
    for solver in ("euler", "rk4"):
        want = npr.cs_solve(rhs, np.array(s0, f), ts, dt0, solver, f, event=_event)
        got = erk.erk_solve(rhs, np.array(s0, f), ts, dt0, solver, f, event=_event)
        assert _same_bits(got, want), (grid, system, solver)
    if system == "blowup" and ts[-1] > 1.0:
        assert np.all(np.isposinf(got[-1]))


@pytest.mark.parametrize("solver,p", [("heun", 2), ("midpoint", 2), ("ralston", 2), ("bosh3", 3)])
def test_order_of_convergence(solver, p):
    """(b) x'' = -x to t = 2 in float64: halving dt0 divides the error by 2^p, to a quarter of the gap
    to the neighbouring order."""
    ts = np.array([0.0, 2.0], f)
    exact = np.array([np.cos(2.0), -np.sin(2.0)])
    errs = []
    for dt0 in (0.0625, 0.03125, 0.015625):
        got = erk.erk_solve(SYSTEMS["linear"][0], np.array([1.0, 0.0]), ts, dt0, solver, np.float64)
        errs.append(np.max(np.abs(got[-1] - exact)))
    for e0, e1 in zip(errs, errs[1:]):
        assert abs(np.log2(e0 / e1) - p) < 0.25, (solver, errs)


def test_two_stage_tableaus_differ_on_a_nonlinear_system():
    """(c) Heun, Midpoint and Ralston coincide on the linear system (up to rounding they are the
    same quadratic in dt A), so only a non-linear one tells a mixed-up tableau: on Van der Pol they
    differ pairwise in float32."""
    ts, dt0 = CS_GRIDS["uniform_c3"]
    rhs, s0 = SYSTEMS["vanderpol"]
    out = {s: erk.erk_solve(rhs, np.array(s0, f), ts, dt0, s, f) for s in ("heun", "midpoint", "ralston")}
    for a, b in (("heun", "midpoint"), ("heun", "ralston"), ("midpoint", "ralston")):
        assert not _same_bits(out[a], out[b]), (a, b)
        assert np.max(np.abs(out[a] - out[b])) > 1e-5, (a, b)
    # (the linear system's step ends coincide; between them the dense outputs differ, their k1 being
    # the derivative at t + c dt -- so the comparison is at a save on the last step's end)
    lin, l0 = SYSTEMS["linear"]
    te = np.array([0.0, 2.0], f)
    lo = {s: erk.erk_solve(lin, np.array(l0), te, 0.0625, s, np.float64)[-1] for s in ("heun", "midpoint", "ralston")}
    assert np.allclose(lo["heun"], lo["midpoint"], rtol=0, atol=1e-12)
    assert np.allclose(lo["heun"], lo["ralston"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("solver,per_step,extra", [("heun", 2, 0), ("midpoint", 2, 0), ("ralston", 2, 0), ("bosh3", 3, 1),
                                                   ("rk4", 4, 0), ("euler", 1, 0)])
def test_rhs_evaluation_count(solver, per_step, extra):
    """(d) Bosh3 is FSAL: 3 steps + 1 evaluations; the two-stage solvers make 2 per step."""
    calls = []

    def rhs(t, s):
        calls.append(t)
        return SYSTEMS["linear"][0](t, s)

    ts = (np.arange(11, dtype=f) * f(0.1)).astype(f)
    n_steps = len(npr.cs_grid(ts, 0.1))
    erk.erk_solve(rhs, np.array([1.0, 0.0], f), ts, 0.1, solver, f)
    assert n_steps == 10 and len(calls) == per_step * n_steps + extra, (solver, len(calls))
    assert all(isinstance(t, np.float32) for t in calls)


def test_zero_entries_are_multiplied():
    """The zero rule of the spec: Midpoint's y1 = y + [0 f0; 1 f1] dt and Bosh3's stage 2 are NaN in a
    component whose f0 is infinite, where skipping the entry would leave them finite.  From
    x = (1, 0.25), dx0 = 1 / (x1 - 0.25) is +inf at stage 0 only.  Midpoint: x0 after the first step
    is NaN (skipped: 1 + 10 dt), seen in the second step's save (the first step's dense output is
    NaN either way, k0 = inf dt).  Bosh3: x0's stage-2 input is NaN, so f2 of x1 = 1 / NaN + 1 and
    with it x1's end state are NaN (skipped: every term of x1 finite)."""
    with np.errstate(all="ignore"):
        rhs = lambda t, s: np.array([f(1) / (s[1] - f(0.25)), f(1) / s[0] + f(1)], f)  # noqa: E731
        ts = np.array([0.0, 0.1, 0.2], f)
        got = erk.erk_solve(rhs, np.array([1.0, 0.25], f), ts, 0.1, "midpoint", f)
        assert np.isnan(got[2, 0])
        got = erk.erk_solve(rhs, np.array([1.0, 0.25], f), ts, 0.1, "bosh3", f)
        assert np.isnan(got[1, 1])
