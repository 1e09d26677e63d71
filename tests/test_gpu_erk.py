"""The fixed-step Heun / Midpoint / Ralston / Bosh3 kernels against the literal numpy restatement
(tests/np_reference_erk.py; the C oracle does not know these solvers): bit for bit where the
right-hand side is exact in float32, to the float64 tolerance of tests/test_oracle.py elsewhere,
every stage loop (JIT and interpreter, register-resident and wide, packed and unpacked lanes)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import multitreegp_amd as mt
import np_reference as npr
import np_reference_erk as erk
from helpers import SR_OPS, bits_equal, dynamic_setup, mismatch_report, static_setup, tree_from_expr
from multitreegp_amd import _native as nat
from multitreegp_amd.engine import DeviceEngine, to_reference_layout
from test_oracle import CS_GRIDS

pytestmark = pytest.mark.gpu

f = np.float32
SOLVERS = {"heun": mt.Heun, "midpoint": mt.Midpoint, "ralston": mt.Ralston, "bosh3": mt.Bosh3}
TRAJ = ("xs", "ys", "us", "acts")


def _event(s):
    return not np.all(np.isfinite(s))


def _evaluate(ff, lib, data, pop, traj=True, lanes=None, jit=None):
    eng = DeviceEngine(ff, lib, 0.0, "cuda:0", jit=jit, lanes=lanes)
    res = eng.evaluate(torch.from_numpy(np.ascontiguousarray(pop)).cuda(), data, trajectories=traj, rollout_fitness=True)
    torch.cuda.synchronize()
    P, R = pop.shape[0], res["rollout_fitness"].shape[1]
    out = {k: res[k].cpu().numpy() for k in ("fitness", "rollout_fitness")}
    for k in TRAJ:
        if traj and res.get(k) is not None:
            out[k] = to_reference_layout(res[k], P, R)
    return out


def _assert_same(a, b, keys, what):
    for k in keys:
        assert bits_equal(a[k], b[k]), (what, mismatch_report(a[k], b[k], k))


# ---------------------------------------------------------------- SR: right-hand sides exact in f32
# (expression for helpers.tree_from_expr, the same in numpy float32), n_var 2: k_sr
SR2 = [
    ([("x1"), ("-", 0.0, "x0")], lambda t, s: np.array([s[1], f(0) - s[0]], f)),
    ([("x1"), ("-", ("*", 0.5, ("*", ("-", 1.0, ("*", "x0", "x0")), "x1")), "x0")],
     lambda t, s: np.array([s[1], f(0.5) * ((f(1) - s[0] * s[0]) * s[1]) - s[0]], f)),
    ([("*", "x0", "x0"), "x1"], lambda t, s: np.array([s[0] * s[0], s[1]], f)),
    ([("/", "x1", ("+", 2.0, ("*", "x0", "x0"))), ("-", 0.0, "x0")],
     lambda t, s: np.array([s[1] / (f(2) + s[0] * s[0]), f(0) - s[0]], f)),
]
# n_var 5: k_sr_wide (a linear chain, and one with a blow-up in its first component)
SR5 = [
    ([("-", "x1", "x0"), ("-", "x2", "x1"), ("-", "x3", "x2"), ("-", "x4", "x3"), ("-", 0.0, "x4")],
     lambda t, s: np.array([s[1] - s[0], s[2] - s[1], s[3] - s[2], s[4] - s[3], f(0) - s[4]], f)),
    ([("*", "x0", "x0"), ("-", "x2", "x1"), ("*", 0.5, "x3"), ("-", "x4", "x3"), ("-", 0.0, "x0")],
     lambda t, s: np.array([s[0] * s[0], s[2] - s[1], f(0.5) * s[3], s[4] - s[3], f(0) - s[0]], f)),
]
X0 = {2: np.array([[1.0, 0.0], [0.3, -0.7], [3.0, 1.0]], f),
      5: np.array([[1.0, 0.0, -0.5, 0.25, 2.0], [3.0, 1.0, 0.5, -1.0, 0.125]], f)}


def _sr_problem(n_var):
    lib = mt.NodeLibrary(SR_OPS, [[f"x{i}" for i in range(n_var)]], [n_var])
    cands = SR2 if n_var == 2 else SR5
    pop = np.stack([np.stack([tree_from_expr(e, lib, 12) for e in exprs]) for exprs, _ in cands])
    return lib, pop, [rhs for _, rhs in cands], X0[n_var]


_REF = {}


def _sr_reference(n_var, solver, grid, max_steps=None):
    """erk_solve(float32) of every (candidate, rollout), computed once per case"""
    key = (n_var, solver, grid, max_steps)
    if key not in _REF:
        _, _, rhss, x0 = _sr_problem(n_var)
        ts, dt0 = CS_GRIDS[grid]
        _REF[key] = np.stack([np.stack([erk.erk_solve(rhs, x0[r], ts, dt0, solver, f, event=_event, max_steps=max_steps)
                                        for r in range(x0.shape[0])]) for rhs in rhss])
    return _REF[key]


def _sr_mse(xs, ys):
    """the kernel's sum in float32: per save point sum_d e^2, added in order, / S"""
    tot = f(0)
    with np.errstate(all="ignore"):
        for k in range(xs.shape[0]):
            e = xs[k] - ys[k]
            sq = e[0] * e[0]
            for dd in range(1, e.shape[0]):
                sq = sq + e[dd] * e[dd]
            tot = tot + sq
    return tot / f(xs.shape[0])


def _sr_check(n_var, solver, grid, max_steps=None):
    lib, pop, rhss, x0 = _sr_problem(n_var)
    ts, dt0 = CS_GRIDS[grid]
    kw = {} if max_steps is None else dict(max_steps=max_steps)
    ff = mt.SREvaluator(solver=SOLVERS[solver](), dt0=dt0, **kw)
    P, R, S = pop.shape[0], x0.shape[0], ts.shape[0]
    ys = (np.sin(np.arange(R * S * n_var, dtype=f)).reshape(R, S, n_var) * f(0.5)).astype(f)
    data = (x0, ts, ys, np.zeros((R, 2), np.uint32))
    want = _sr_reference(n_var, solver, grid, max_steps)
    got = _evaluate(ff, lib, data, pop)
    assert bits_equal(got["xs"], want), (solver, grid, mismatch_report(got["xs"], want, "xs"))
    mx = f(ff.max_fitness)
    for p in range(P):
        sub = []
        for r in range(R):
            mse = _sr_mse(want[p, r], ys[r])
            rf = got["rollout_fitness"][p, r]
            if np.isfinite(mse):
                assert np.isfinite(rf) and abs(float(rf) - float(mse)) <= 1e-6 * abs(float(mse)), (solver, grid, p, r, rf, mse)
                sub.append(float(mse))
            else:
                assert not np.isfinite(rf), (solver, grid, p, r, rf, mse)
                sub.append(float(mx))
        mean = min(max(float(np.mean(sub)), 0.0), float(mx))
        if all(v == float(mx) for v in sub):
            assert got["fitness"][p] == mx  # exactly the substituted value
        else:
            assert abs(float(got["fitness"][p]) - mean) <= 1e-6 * mean + 1e-30, (solver, grid, p)
    only = _evaluate(ff, lib, data, pop, traj=False)
    _assert_same(got, only, ("fitness",), (solver, grid, "fitness-only launch"))
    return want


@pytest.mark.parametrize("grid", sorted(CS_GRIDS))
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_sr_register_resident_bitexact(solver, grid):
    want = _sr_check(2, solver, grid)
    if CS_GRIDS[grid][0][-1] > 1.0:  # x0' = x0^2 from 3 blows up at t = 1/3: a non-finite row, then the +inf fill
        assert not np.all(np.isfinite(want[2, 2])) and np.all(np.isposinf(want[2, 2, -1]))


@pytest.mark.parametrize("grid", sorted(CS_GRIDS))
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_sr_wide_bitexact(solver, grid):
    want = _sr_check(5, solver, grid)
    if CS_GRIDS[grid][0][-1] > 1.0:  # the second candidate's x0' = x0^2 from 3 blows up at t = 1/3
        assert np.all(np.isposinf(want[1, 1, -1])) and np.all(np.isfinite(want[0]))


@pytest.mark.parametrize("n_var", [2, 5])
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_sr_evaluate_candidate(solver, n_var):
    """The public per-candidate calls (sr.py:47-55 / 30-45): evaluate_candidate's trajectories are
    erk_solve(float32) bit for bit, its fitness the rows' MSE, __call__ their clipped mean."""
    lib, pop, rhss, x0 = _sr_problem(n_var)
    ts, dt0 = CS_GRIDS["nonuniform"]
    ff = mt.SREvaluator(solver=SOLVERS[solver](), dt0=dt0)
    R, S = x0.shape[0], ts.shape[0]
    ys = (np.sin(np.arange(R * S * n_var, dtype=f)).reshape(R, S, n_var) * f(0.5)).astype(f)
    data = (x0, ts, ys, np.zeros((R, 2), np.uint32))
    te = mt.TreeEvaluator(lib, 12)
    want = _sr_reference(n_var, solver, "nonuniform")
    for p in range(pop.shape[0]):
        fit, pred = ff.evaluate_candidate(pop[p], data, te)
        assert bits_equal(pred, want[p]), (solver, p, mismatch_report(pred, want[p], "pred_ys"))
        sub = []
        for r in range(R):
            mse = _sr_mse(want[p, r], ys[r])
            if np.isfinite(mse):
                assert abs(float(fit[r]) - float(mse)) <= 1e-6 * abs(float(mse)), (solver, p, r)
            else:
                assert not np.isfinite(fit[r]), (solver, p, r)
            sub.append(float(mse) if np.isfinite(mse) else float(ff.max_fitness))
        mean = min(float(np.mean(sub)), float(ff.max_fitness))
        got = ff(pop[p][..., 3:], pop[p][..., :3], data, te)
        assert abs(got - mean) <= 1e-6 * mean, (solver, p, got, mean)


@pytest.mark.parametrize("n_var", [2, 5])
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_sr_max_steps_cut_fills_inf(solver, n_var):
    want = _sr_check(n_var, solver, "uniform_c3", max_steps=50)
    assert np.all(np.isfinite(want[0, 0, :50])) and np.all(np.isposinf(want[0, 0, 51:]))


# ---------------------------------------------------------------- control, exact arithmetic
@pytest.mark.parametrize("grid", ["off_multiple", "nonuniform"])
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_static_harmonic_exact_policy_bitexact(solver, grid):
    """HarmonicOscillator, static policy u = 0 - y2, no noise: xs and us bit for bit against the
    float32 restatement whose operation order is the C oracle's (np_reference_erk.ho_*)."""
    ts, dt0 = CS_GRIDS[grid]
    env, lib, _, data, _ = static_setup(P=1, R=3, n_steps=10, env="harmonic", h=dt0)
    ff = mt.FeedforwardEvaluator(env, dt0, solver=SOLVERS[solver]())
    data = (data[0], ts) + tuple(data[2:])
    pop = tree_from_expr(("-", 0.0, "y2"), lib, 8)[None, None]
    got = _evaluate(ff, lib, data, pop)
    d = ff.prepare(data)
    for r in range(3):
        omega, zeta = d["params"][r]
        xs = erk.erk_solve(erk.ho_static_rhs_f32(omega, zeta), d["x0"][r], ts, dt0, solver, f, event=_event)
        us = np.array([erk.ho_policy_f32(erk.ho_obs_f32(x)) for x in xs], f)[:, None]
        assert np.all(np.isfinite(xs))
        assert bits_equal(got["xs"][0, r], xs), (solver, grid, r, mismatch_report(got["xs"][0, r], xs, "xs"))
        assert bits_equal(got["us"][0, r], us), (solver, grid, r, mismatch_report(got["us"][0, r], us, "us"))


# ---------------------------------------------------------------- control, both program paths
def _ctl_case(case, solver):
    s = SOLVERS[solver]()
    if case == "dynamic_acrobot_noisy":
        env, lib, _, data, pop = dynamic_setup(P=8, R=3, n_steps=20, obs_noise=0.1)
        return env, lib, mt.DynamicEvaluator(env, 2, 0.05, solver=s), data, pop
    if case == "static_acrobot":
        env, lib, _, data, pop = static_setup(P=8, R=3, n_steps=20)
        return env, lib, mt.FeedforwardEvaluator(env, 0.05, solver=s), data, pop
    env, lib, _, data, pop = dynamic_setup(P=8, R=3, n_steps=20, env="harmonic", state_size=5)
    return env, lib, mt.DynamicEvaluator(env, 5, 0.05, solver=s), data, pop


@pytest.mark.parametrize("case", ["dynamic_acrobot_noisy", "static_acrobot", "dynamic_harmonic_ss5"])
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_control_paths_agree(solver, case, monkeypatch):
    """The JIT stage loops equal the interpreter's (MTGP_JIT=0), the packed lane set equals the
    default one, and the noise-free cases follow the float64 restatement."""
    env, lib, ff, data, pop = _ctl_case(case, solver)
    keys = ("fitness", "rollout_fitness") + tuple(k for k in TRAJ if k != "acts" or case != "static_acrobot")
    got = _evaluate(ff, lib, data, pop)
    packed = _evaluate(ff, lib, data, pop, lanes=0)
    _assert_same(got, packed, keys, (solver, case, "packed lanes"))
    only = _evaluate(ff, lib, data, pop, traj=False)
    _assert_same(got, only, ("fitness",), (solver, case, "fitness-only launch"))
    monkeypatch.setenv("MTGP_JIT", "0")
    interp = _evaluate(ff, lib, data, pop)
    _assert_same(got, interp, keys, (solver, case, "MTGP_JIT=0"))
    interp_packed = _evaluate(ff, lib, data, pop, lanes=0)
    _assert_same(got, interp_packed, keys, (solver, case, "MTGP_JIT=0 packed"))
    if case == "dynamic_acrobot_noisy":
        return
    d = ff.prepare(data)
    compared = tight = 0
    for p in range(pop.shape[0]):
        for r in range(d["R"]):
            x0 = d["x0"][r].astype(np.float64)
            if case == "static_acrobot":
                traj = erk.erk_solve(lambda t, s: npr.ff_rhs(pop[p], lib, s), x0, d["ts"], 0.05, solver)
                have = got["xs"][p, r]
            else:
                prm, tg = d["params"][r].astype(np.float64), float(d["targets"][r, 0])
                traj = erk.erk_solve(lambda t, s: npr.dyn_rhs_env("harmonic", pop[p], lib, s, 5, prm, tg, 2),
                                     np.concatenate([x0, np.zeros(5)]), d["ts"], 0.05, solver)
                have = np.concatenate([got["xs"][p, r], got["acts"][p, r]], -1)
            if not (np.all(np.isfinite(traj)) and np.all(np.abs(traj) < 1e3) and np.all(np.isfinite(have))):
                continue
            tight += bool(np.allclose(have, traj, rtol=2e-3, atol=2e-3))  # (tests/test_oracle.py's criterion)
            compared += 1
    assert compared >= 10 and tight >= 0.9 * compared, (solver, case, compared, tight)


# ---------------------------------------------------------------- noise keyed on the stage times
@pytest.mark.parametrize("solver", sorted(SOLVERS))
def test_static_noise_is_keyed_on_stage_times(solver):
    """Static Acrobot with observation noise against the float64 restatement whose noise is
    npr.obs_noise at the float32 stage time of every evaluation (erk_solve hands rhs that time);
    Bosh3 never evaluates at a later step's t: its reused f3 carries the draw of t + 1.0f dt."""
    env, lib, _, data, pop = static_setup(P=8, R=3, n_steps=20, obs_noise=0.1)
    ff = mt.FeedforwardEvaluator(env, 0.05, solver=SOLVERS[solver]())
    got = _evaluate(ff, lib, data, pop)
    d = ff.prepare(data)
    W = d["obs_w"].astype(np.float64)
    compared = tight = 0
    for p in range(pop.shape[0]):
        for r in range(d["R"]):
            key = d["obs_keys"][r]
            nz = lambda t: npr.obs_noise(key, t, W, False)  # noqa: E731
            traj = erk.erk_solve(lambda t, s: npr.ff_rhs(pop[p], lib, s, noise=nz(t)), d["x0"][r].astype(np.float64),
                                 d["ts"], 0.05, solver)
            ys_want = np.array([npr.acro_f_obs(traj[k, :4], nz(d["ts"][k])) for k in range(traj.shape[0])])
            have = got["xs"][p, r]
            if not (np.all(np.isfinite(traj)) and np.all(np.abs(traj) < 1e3) and np.all(np.isfinite(have))):
                continue
            tight += bool(np.allclose(have, traj, rtol=2e-3, atol=2e-3)
                          and np.allclose(got["ys"][p, r], ys_want, rtol=2e-3, atol=2e-3))
            compared += 1
    assert compared >= 10 and tight >= 0.9 * compared, (solver, compared, tight)
    res = got["ys"][..., 2:] - got["xs"][..., 2:]
    res = res[np.isfinite(res)]
    assert 0.05 < np.std(res) < 0.2  # the noise is really there


# ---------------------------------------------------------------- refusals
def _entry_args(model_id, solver):
    """An otherwise valid call with P = 0: every entry returns MTGP_OK for it after its argument
    checks and before any device work, so MTGP_ERR_ARG is the solver's refusal and nothing launches."""
    m = nat.MtgpModel()
    m.model, m.solver, m.h, m.n_save, m.max_steps = model_id, solver, 0.05, 4, 100
    if model_id == nat.MODEL_SR:
        m.n_var, m.prog_state = 2, 0
    else:
        m.env, m.n_var, m.n_obs, m.n_control, m.state_size = nat.ENV_ACROBOT, 4, 4, 1, 2
        m.prog_state, m.prog_readout, m.prog_readout_save = 0, 2, 2
    m.max_fitness = 1e4
    buf = np.zeros(64, np.int32)
    ro = nat.MtgpRollouts()
    ro.R = 4
    ro.x0 = ro.ts = ro.params = ro.ys_true = buf.ctypes.data
    return m, ro, buf


@pytest.mark.parametrize("model_id", [nat.MODEL_SR, nat.MODEL_DYNAMIC])
def test_refusals(model_id):
    lib = nat.load()
    n_prog = 2 if model_id == nat.MODEL_SR else 3

    def evaluate(solver):
        m, ro, buf = _entry_args(model_id, solver)
        out = nat.MtgpOutputs()
        out.fitness = buf.ctypes.data
        return lib.mtgp_eval_rk4(ctypes.byref(m), buf.ctypes.data, buf.ctypes.data, n_prog, 4, buf.ctypes.data, 0,
                                 ctypes.byref(ro), ctypes.byref(out), None)

    def grad(solver):
        m, ro, buf = _entry_args(model_id, solver)
        fn = lib.mtgp_sr_grad if model_id == nat.MODEL_SR else lib.mtgp_ctl_grad
        p = buf.ctypes.data
        return fn(ctypes.byref(m), p, n_prog, 4, 0, p, p, 1, ctypes.byref(ro), p, p, p, None)

    for solver in (nat.SOLVER_RK4, nat.SOLVER_EULER, 3, 4, 5, 6):
        assert evaluate(solver) == nat.OK, solver
    for solver in (7, 8, -1):
        assert evaluate(solver) == nat.ERR_ARG, solver
    for solver in (nat.SOLVER_RK4, nat.SOLVER_EULER):
        assert grad(solver) == nat.OK, solver
    for solver in (3, 4, 5, 6, 7):
        assert grad(solver) == nat.ERR_ARG, solver
