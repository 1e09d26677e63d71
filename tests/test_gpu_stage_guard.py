"""The dynamic JIT stage loop's merged guards, at the states where they can go wrong: bit-exact vs the oracle.

One wave-uniform range test of a stage's input state (csrc/mtgp_ab.h MTGP_STAGE_GUARD: both angles
below 2^15 in magnitude, both velocities finite) stands for the observation's finite test, the angle
wraps' |theta + pi| < 2^20 tests and the drift's trig-range and fastdiv tests; the drift's tests of
its two division numerators (div_safe) stay per stage, inside the guarded-out form too.  A wave
that fails a test runs the guarded code.  Each population is 4 individuals x 32 rollouts (2 waves
of 2 groups), 8 steps of h = 0.05, 24-node trees; a rollout is a lane of each group, so one special
start state sits in an otherwise ordinary wave once per group.  The special states straddle each threshold; the readout cases and a
rollout of large velocity push the drift's num / n1 out of [2^-40, 2^40) or to NaN.

Checked from the oracle alone (_assert_oracle): every special lane has the intended bits at save 0
and lies on the intended side of its threshold, the overflow lane is non-finite by the second save,
and the readout cases reach the division fallback at the first stage (num and n1 recomputed in
numpy from the first stage's state, which is save 0 wherever the first step stays finite; a lane
whose first step overflows has a non-finite save 0, and that is asserted instead)."""
import functools

import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd.engine import DeviceEngine, to_reference_layout
from oracle import oracle as orc
from helpers import CONTROL_OPS, bits_equal, mismatch_report, oracle_model, oracle_rollouts, tree_from_expr

pytestmark = pytest.mark.gpu

N_NODES = 24
N_STEPS = 8
H = 0.05
R = 32
LANE = 5  # the rollout that carries the special state

F = np.float32
T15, T17, T20 = F(2.0 ** 15), F(2.0 ** 17), F(2.0 ** 20)
B15 = np.nextafter(T15, F(0))  # 2^15 - 1 ulp
INF, NAN = F(np.inf), F(np.nan)

# (name, component, value, what the oracle-only check expects of it)
SPECIALS = []
for comp in (0, 1):
    for v, kind in ((B15, "below15"), (-B15, "below15"), (T15, "at15"), (-T15, "at15"), (T17, "at15"), (-T17, "at15")):
        SPECIALS.append((f"th{comp + 1}={float(v)!r}", comp, v, kind))
SPECIALS += [("th1=1048572", 0, F(1048572.0), "wrap_fast"), ("th2=1048573", 1, F(1048573.0), "wrap_slow"),
             ("th1=2^20", 0, T20, "wrap_slow"), ("th2=-0.0", 1, F(-0.0), "below15")]
SPECIALS += [(f"x{c}={n}", c, v, "nonfinite") for c in range(4) for n, v in (("inf", INF), ("nan", NAN))]
SPECIALS += [("thd1=3e38", 2, F(3e38), "overflow")]
# the static policy's loop is tested with angles below 2^15 only (its slow-trig defect, DESIGN.md "Round 7")
STATIC_SPECIALS = [s for s in SPECIALS if s[3] in ("below15", "nonfinite")]

# the drift's division fallbacks next to the stage guard: readouts (inf, 1e30, 0, NaN) of the individuals in
# group 0 of wave 0 and group 1 of wave 1; LANE starts with a velocity that puts |num| beyond 2^40
# whatever the control
READOUTS = {"inf": ("*", 1e30, 1e30), "1e30": 1e30, "tiny": ("*", 1e-30, 1e-30),
            "nan": ("-", ("*", 1e30, 1e30), ("*", 1e30, 1e30))}

ORDINARY = [[("-", ("sin", "y1"), "a1"), ("-", ("cos", "y2"), "a2"), ("+", "a1", "a2")],
            [("-", "y3", "a1"), ("*", "y4", "a2"), ("sin", ("+", "a1", "y1"))],
            [("cos", ("+", "y1", "y2")), ("-", "y2", "a2"), ("*", "a1", 0.5)],
            [("-", ("*", "y3", "y4"), "a1"), ("sin", "a1"), ("-", "a2", "a1")]]
STATIC = [("sin", ("+", "y1", "y2")), ("*", ("cos", "y1"), "y4"), ("-", "y3", "y4"), ("*", "y2", 0.5)]


@functools.lru_cache(maxsize=None)
def _base(policy, solver, noise):
    env = mt.Acrobot(0.0, noise)
    ys = [f"y{i + 1}" for i in range(env.n_obs)]
    sol = mt.Euler() if solver == "euler" else mt.RK4()
    if policy == "dynamic":
        lib = mt.NodeLibrary(CONTROL_OPS, [ys + ["a1", "a2", "u"], ["a1", "a2"]], [2, 1])
        ff = mt.DynamicEvaluator(env, 2, H, solver=sol)
    else:
        lib = mt.NodeLibrary(CONTROL_OPS, [ys], [1])
        ff = mt.FeedforwardEvaluator(env, H, solver=sol)
    data = tuple(mt.control_data(env, R, H, None, seed=11, n_steps=N_STEPS))
    return lib, ff, data


def _population(policy, lib, readout=None):
    if policy == "static":
        return np.ascontiguousarray(np.stack([tree_from_expr(e, lib, N_NODES)[None] for e in STATIC]), np.float32)
    trees = [list(t) for t in ORDINARY]
    if readout is not None:
        trees[0][2] = READOUTS[readout]  # wave 0, group 0
        trees[3][2] = READOUTS[readout]  # wave 1, group 1
    return np.ascontiguousarray(np.stack([np.stack([tree_from_expr(e, lib, N_NODES) for e in t]) for t in trees]),
                                np.float32)


def _x0(data, scenario):
    """The sampled start states with the scenario's special lanes written in: ("one", special),
    ("all",): special i in rollout i (every lane of both waves special), ("readout", name)."""
    x0 = np.array(data[0], np.float32, copy=True)
    if scenario[0] == "one":
        _, comp, v, _ = scenario[1]
        x0[LANE, comp] = v
    elif scenario[0] == "all":
        for r in range(R):
            _, comp, v, _ = SPECIALS[r % len(SPECIALS)]
            x0[r, comp] = v
    else:
        x0[LANE, 2] = F(1.0e7)
    return x0


def _scenarios(policy):
    if policy == "static":
        return [("one", s) for s in STATIC_SPECIALS]
    return [("one", s) for s in SPECIALS] + [("all",)] + [("readout", n) for n in READOUTS]


def _scenario_id(sc):
    return sc[1][0] if sc[0] == "one" else (sc[0] if sc[0] == "all" else f"readout-{sc[1]}")


_ORACLE = {}


def oracle_case(policy, solver, noise, scenario):
    """(lib, ff, data, pop, ref): the oracle's result with trajectories, computed once per population
    and start state on the host, shared by the trajectory and the fitness-only variant, read-only."""
    key = (policy, solver, noise, _scenario_id(scenario))
    if key not in _ORACLE:
        lib, ff, data = _base(policy, solver, noise)
        pop = _population(policy, lib, scenario[1] if scenario[0] == "readout" else None)
        data = (_x0(data, scenario),) + tuple(data[1:])
        d = ff.prepare(data)
        ref = orc.evaluate(oracle_model(ff, d), pop, lib, oracle_rollouts(d), trajectories=True)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _assert_oracle(ref, d, data[0], scenario, policy)
        _ORACLE[key] = (lib, ff, data, pop, ref)
    return _ORACLE[key]


def _div_safe(v):
    """the kernel's div_safe: |v| in [2^-40, 2^40) or NaN"""
    a = np.abs(v.astype(np.float32))
    return ~(a < F(9.094947e-13)) & ~(a >= F(1.0995116e12))


def _first_stage_num_n1(x, params, u):
    """the drift's num and n1 (acrobot.py:55-72) at state x [.., 4] and raw control u, in float32
    numpy (numpy's sin / cos: the magnitudes are what is checked, not the last bits)"""
    f = np.float32
    l1, l2, m1, m2 = (params[..., i].astype(f) for i in range(4))
    lc1, lc2, g = f(0.5) * l1, f(0.5) * l2, f(9.81)
    th1, th2, thd1, thd2 = (x[..., i].astype(f) for i in range(4))
    with np.errstate(all="ignore"):
        c = np.where(np.isnan(u), u, np.clip(u, f(-1), f(1))).astype(f)
        s2, c2 = np.sin(th2), np.cos(th2)
        d1 = m1 * lc1 ** 2 + m2 * (l1 ** 2 + lc2 ** 2 + f(2) * l1 * lc2 * c2) + f(1) + f(1)
        d2 = m2 * (lc2 ** 2 + l1 * lc2 * c2) + f(1)
        phi2 = m2 * lc2 * g * np.cos(th1 + th2 - f(np.pi / 2))
        phi1 = (-m2 * l1 * lc2 * thd2 ** 2 * s2 - f(2) * m2 * l1 * lc2 * thd2 * thd1 * np.sin(th1)
                + (m1 * lc1 + m2 * l1) * g * np.cos(th1 - f(np.pi / 2)) + phi2)
        num = c + d2 / d1 * phi1 - m2 * l1 * lc2 * thd1 ** 2 * s2 - phi2
        den = m2 * lc2 ** 2 + f(1) - d2 ** 2 / d1
        a2 = num / den
        n1 = -(d2 * a2 + phi1)
    return num.astype(f), n1.astype(f)


def _assert_oracle(ref, d, x0, scenario, policy):
    xs = ref["xs"]  # [P, R, S, 4]
    assert xs.shape[:2] == (4, R) and xs.shape[3] == 4
    lanes = [(LANE, scenario[1])] if scenario[0] == "one" else \
        [(r, SPECIALS[r % len(SPECIALS)]) for r in range(R)] if scenario[0] == "all" else []
    # save 0 (the first step's dense output at its start) is the start state bit for bit (-0.0
    # included) in every individual, except in the lanes whose first step leaves the finite range:
    # the non-finite and overflow specials and the readout cases' LANE, whose save 0 is not finite
    same = np.all(xs[:, :, 0, :].view(np.uint32) == np.broadcast_to(x0, (4, R, 4)).view(np.uint32), axis=-1)
    blown = ~np.all(np.isfinite(xs[:, :, 0, :]), axis=-1)
    assert np.all(same | blown)
    trouble = [r for r, s in lanes if s[3] in ("nonfinite", "overflow")]
    assert np.all(blown[:, [r for r, s in lanes if s[3] == "nonfinite"]])
    if scenario[0] != "readout":  # every other lane starts (and is saved) as given
        assert np.all(same[:, [r for r in range(R) if r not in trouble]])
    for r, (name, comp, v, kind) in lanes:
        s0 = x0[r, comp]  # (= save 0 where the lane is not blown, above)
        assert s0.view(np.uint32) == np.float32(v).view(np.uint32), name
        if kind == "below15":
            assert abs(s0) < T15 and (abs(s0) == B15 or s0 == 0)
        elif kind == "at15":
            assert T15 <= abs(s0) < np.inf
        elif kind == "wrap_fast":
            assert abs(s0) >= T15 and abs(np.float32(s0 + np.float32(np.pi))) < T20
        elif kind == "wrap_slow":
            assert np.isfinite(s0) and abs(np.float32(s0 + np.float32(np.pi))) >= T20
        elif kind == "nonfinite":
            assert not np.isfinite(s0)
        elif kind == "overflow":
            assert np.isfinite(s0) and not np.all(np.isfinite(xs[:, r, 1, :]), axis=-1).any(), name
    if policy == "static":  # the known defect's range is never entered: every finite angle stays below 2^15
        ang = xs[..., :2]
        assert np.all(np.abs(ang[np.isfinite(ang)]) < T15)
    if scenario[0] == "readout":
        u = {"inf": np.inf, "1e30": 1e30, "tiny": 0.0, "nan": np.nan}[scenario[1]]
        num, n1 = _first_stage_num_n1(x0, np.asarray(d["params"], np.float32).reshape(R, 4),
                                      np.full(R, u, np.float32))
        out = ~_div_safe(num) | ~_div_safe(n1) | np.isnan(num) | np.isnan(n1)
        if scenario[1] == "nan":  # a NaN control: every lane's num and n1 are NaN (div_safe passes a NaN,
            assert np.isnan(num).all() and np.isnan(n1).all()  # both quotients then give the NaN of `/`)
        else:  # LANE is outside [2^-40, 2^40), the ordinary lanes are inside
            assert not _div_safe(num[LANE]) or not _div_safe(n1[LANE]), (num[LANE], n1[LANE])
            assert not out[np.arange(R) != LANE].any()


# (policy, solver, trajectories, obs_noise)
VARIANTS = [("dynamic", "rk4", True, 0.0), ("dynamic", "rk4", False, 0.0), ("dynamic", "euler", True, 0.0),
            ("dynamic", "euler", False, 0.0), ("dynamic", "rk4", True, 0.1), ("static", "rk4", True, 0.0)]
CASES = [(*v, sc) for v in VARIANTS for sc in _scenarios(v[0])]


def _id(c):
    policy, solver, traj, noise, sc = c
    return f"{policy}_{solver}-{'traj' if traj else 'fit'}-nz{noise}-{_scenario_id(sc)}"


@functools.lru_cache(maxsize=None)
def _engine(policy, solver, noise):
    lib, ff, _ = _base(policy, solver, noise)
    return DeviceEngine(ff, lib, 0.0, "cuda:0", jit=True, lanes=0)  # lanes=0: 64 / Rp individuals per wave


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_stage_guard_bitexact(case):
    policy, solver, traj, noise, scenario = case
    lib, ff, data, pop, ref = oracle_case(policy, solver, noise, scenario)
    eng = _engine(policy, solver, noise)
    res = eng.evaluate(torch.from_numpy(pop).cuda(), data, trajectories=traj, rollout_fitness=True, schedule=False)
    torch.cuda.synchronize()
    assert DeviceEngine.jit_ok(res["_flat"])
    for k in ("fitness", "rollout_fitness"):
        got = res[k].cpu().numpy()
        assert bits_equal(got, ref[k]), mismatch_report(got, ref[k], k)
    if traj:
        for k in (["xs", "ys", "us", "acts"] if policy == "dynamic" else ["xs", "ys", "us"]):
            got = to_reference_layout(res[k], pop.shape[0], R)
            assert bits_equal(got, ref[k]), mismatch_report(got, ref[k], k)
