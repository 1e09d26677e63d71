"""Literal numpy restatement of diffrax's explicit Runge-Kutta solvers under ConstantStepSize,
driven by the tableau: Heun, Midpoint, Ralston, Bosh3 (and Euler / RK4, which tie it to
np_reference.cs_solve).  Written from the spec text of include/mtgp_cstep.h; it imports the time
grid of np_reference and nothing from the product.

* stage time t + c_i dt in float32 (the product rounds, then the sum);
* stage input y + (sum_j a_ij f_j) dt, ascending j, products and sums rounded separately;
* a zero tableau entry is multiplied: its term is a no-op when +-0 and makes the row NaN when NaN;
* Bosh3 is FSAL and "solution same as last stage input": y1 is the stage-3 input, f3 = f(t + dt, y1)
  is the next step's f0 (reused, not evaluated again);
* dense output: Euler linear, every other solver the cubic Hermite from k0 = f_first dt,
  k1 = f_last dt."""
import numpy as np

from np_reference import cs_grid

# c (stages 1..), a (lower rows), b (None: the solution is the last stage's input), fsal
TABLEAUS = {
    "euler": dict(c=[], a=[], b=[1.0], fsal=False),
    "heun": dict(c=[1.0], a=[[1.0]], b=[0.5, 0.5], fsal=False),
    "midpoint": dict(c=[0.5], a=[[0.5]], b=[0.0, 1.0], fsal=False),
    "ralston": dict(c=[0.75], a=[[0.75]], b=[1.0 / 3.0, 2.0 / 3.0], fsal=False),
    "bosh3": dict(c=[0.5, 0.75, 1.0], a=[[0.5], [0.0, 0.75], [2.0 / 9.0, 1.0 / 3.0, 4.0 / 9.0]], b=None, fsal=True),
    "rk4": dict(c=[0.5, 0.5, 1.0], a=[[0.5], [0.0, 0.5], [0.0, 0.0, 1.0]], b=[1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0],
                fsal=False),
}


def _row(coefs, fs, d):
    """sum_j coefs[j] * fs[j], ascending j: the non-zero entries' products summed in order, the zero
    entries' products z joined by the zero rule (NaN stays, +-0 is a no-op)."""
    v, z = None, None
    for cj, fj in zip(coefs, fs):
        term = d(cj) * fj
        if cj == 0.0:
            z = term if z is None else z + term
        else:
            v = term if v is None else v + term
    return v if z is None else np.where(np.isnan(z), z, v)


def erk_solve(rhs, s0, ts, dt0, solver, dtype=np.float64, event=None, max_steps=None):
    """diffeqsolve(solver, ConstantStepSize, SaveAt(ts)).  dtype float64 (semantics, to a tolerance)
    or float32 (literal rounding).  rhs(t, s) -> ds with t a float32 stage time.  event(s) -> True
    ends the solve after the step (its saves are kept); max_steps bounds the step count.
    -> saved [len(ts), n], +inf where nothing was saved."""
    d = dtype
    tab = TABLEAUS[solver]
    f32 = np.float32
    ts = np.asarray(ts, f32)
    S = ts.shape[0]
    y = np.array(s0, d)
    saved = np.full((S, y.shape[0]), np.inf, d)
    k = 0
    f_carry = None  # FSAL: the last step's last stage derivative
    with np.errstate(all="ignore"):
        for t, tn in cs_grid(ts, dt0, max_steps):
            dtf = f32(tn - t)
            dt = d(dtf)
            fs = [f_carry if (tab["fsal"] and f_carry is not None) else np.asarray(rhs(t, y), d)]
            yin = y
            for c, arow in zip(tab["c"], tab["a"]):
                yin = y + _row(arow, fs, d) * dt
                fs.append(np.asarray(rhs(f32(t + f32(c) * dtf), yin), d))
            y1 = yin if tab["b"] is None else y + _row(tab["b"], fs, d) * dt
            f_carry = fs[-1]
            while k < S and ts[k] <= tn:
                if t == tn:
                    th = d(0.0)
                elif d is np.float32:
                    th = f32(f32(ts[k] - t) / f32(tn - t))
                else:
                    th = (d(ts[k]) - d(t)) / (d(tn) - d(t))
                if solver == "euler":
                    saved[k] = y + th * (y1 - y)
                else:
                    k0, k1 = fs[0] * dt, fs[-1] * dt
                    a = ((k0 + k1) + d(2) * y) - d(2) * y1
                    b = (((d(-2) * k0) - k1) - d(3) * y) + d(3) * y1
                    v = d(0) * th + a
                    v = v * th + b
                    v = v * th + k0
                    saved[k] = v * th + y
                k += 1
            y = y1
            if event is not None and event(y):
                break
    return saved


# ---- the static policy on HarmonicOscillator in float32, operation order of the C oracle's text
# (oracle/mtgp_oracle.c: ctl_f_obs with C = I and no noise, ho_drift, the policy u = 0 - y2)
def ho_obs_f32(x):
    f = np.float32
    x = np.asarray(x, f)
    with np.errstate(all="ignore"):
        y0 = f(f(f(1) * x[0]) + f(f(0) * x[1])) + f(0)
        y1 = f(f(f(0) * x[0]) + f(f(1) * x[1])) + f(0)
    return np.array([y0, y1], f)


def ho_policy_f32(y):
    return np.float32(np.float32(0.0) - y[1])


def ho_static_rhs_f32(omega, zeta):
    f = np.float32
    omega, zeta = f(omega), f(zeta)

    def rhs(t, x):
        x = np.asarray(x, f)
        u = ho_policy_f32(ho_obs_f32(x))
        with np.errstate(all="ignore"):
            dx0 = f(f(f(0) * x[0]) + f(f(1) * x[1])) + f(f(0) * u)
            dx1 = f(f(f(-omega) * x[0]) + f(f(-zeta) * x[1])) + f(f(1) * u)
        return np.array([dx0, dx1], f)

    return rhs
