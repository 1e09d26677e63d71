"""mtgp_ctl_grad for dynamic policies with state_size 4..16 (k_ctl_grad_wide: every per-lane array
in LDS columns, csrc/mtgp_grad.hip) vs oracle_ctl_grad: loss and every coefficient's gradient bit
for bit -- every environment, RK4 / Euler / Dopri5 + PID, observation noise, two parameter chunks,
the rollout ceiling, the general Acrobot mask -- and GeneticProgramming's optimising generation
end to end.  The cases and their oracle references come from tests/test_coefficients_wide.py,
where the oracle alone pins them."""
import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd import coefficients as co
from multitreegp_amd.engine import DeviceEngine
from oracle import oracle as orc

from helpers import bits_equal, dynamic_setup, mismatch_report, oracle_model, oracle_rollouts
from test_coefficients_wide import WIDE_CASES, moved, oracle_reference, wide_case, wide_setup

pytestmark = pytest.mark.gpu


def _engine(ff, lib):
    return DeviceEngine(ff, lib, 0.0, torch.device("cuda", 0))


def _assert_grads(loss, grads, rl, rg, tag=""):
    assert bits_equal(loss, rl), (tag, mismatch_report(loss, rl, "loss"))
    for p, g in enumerate(grads):
        assert bits_equal(g, rg[p, : len(g)]), (tag, p, g, rg[p, : len(g)])


@pytest.mark.parametrize("env,state_size,solver,noise", WIDE_CASES)
def test_gpu_ctl_grad_wide_bitexact(env, state_size, solver, noise):
    lib, ff, data, pop, rl, rg, rows = wide_case(env, state_size, solver, noise)
    eng = _engine(ff, lib)
    opt = co.CoefficientOptimiser(eng)
    loss, grads = opt.loss_and_grad(pop, data)
    assert opt.last_jit_info is None  # wide states interpret: no code buffer was set up
    _assert_grads(loss, grads, rl, rg)
    fit = eng.evaluate(torch.from_numpy(np.array(pop)).cuda(), data)["fitness"].cpu().numpy()
    assert bits_equal(loss, fit), mismatch_report(loss, fit, "fitness")
    assert moved(grads) >= 5
    if (env, state_size) == ("acrobot", 16):  # the two-chunk path: more coefficients than parameter slots
        assert opt.param_cap(eng.ff.n_data()) < max(len(r) for r in rows)
    loss2, grads2 = co.CoefficientOptimiser(eng, jit=False).loss_and_grad(pop, data)
    _assert_grads(loss2, grads2, rl, rg, "jit=False")


def test_gpu_ctl_grad_wide_rollout_ceiling():
    """R = 64, the most rollouts the gradient kernels take: every lane set is K whole waves."""
    lib, ff, data, pop = wide_setup("acrobot", 8, "rk4", 0.0, P=4, R=64)
    rl, rg, rows = oracle_reference(lib, ff, data, pop)
    loss, grads = co.CoefficientOptimiser(_engine(ff, lib)).loss_and_grad(pop, data)
    _assert_grads(loss, grads, rl, rg)


OFFSET_DOPRI5 = (1e-5, 1e-5, 0.002, 600)  # as tests/test_coefficients.py OFFSET_CASES


@pytest.mark.parametrize("solver,t0", [(None, 1.0), (None, -0.35), (OFFSET_DOPRI5, 1.5), (OFFSET_DOPRI5, -0.4)])
def test_gpu_ctl_grad_wide_offset_ts_bitexact(solver, t0):
    """The general Acrobot mask (MtgpRollouts.fit_kof, cost prefixes kept behind the partials) with
    a wide state: a positive offset (the kept prefix lies behind the first success) and a negative
    one (it runs into the +inf fill)."""
    from test_gpu_acrobot_mask import _swing_data
    env, lib, ff, data, pop = dynamic_setup(P=10, R=8, n_steps=40, depth=4, N=24, seed=13, state_size=5,
                                            solver=solver)
    data = _swing_data(data, t0, seed=int(abs(t0) * 100) + 5)
    eng = _engine(ff, lib)
    d = eng.prepare_data(data)
    assert d.get("fit_kof") is not None
    rl, rg, rows = orc.ctl_grad(oracle_model(ff, d), pop, lib, oracle_rollouts(d))
    assert sum(len(r) for r in rows) > 5
    loss, grads = co.CoefficientOptimiser(eng).loss_and_grad(pop, data)
    _assert_grads(loss, grads, rl, rg)
    fit = eng.evaluate(torch.from_numpy(pop).cuda(), data)["fitness"].cpu().numpy()
    assert bits_equal(loss, fit), mismatch_report(loss, fit, "fitness")


def test_gpu_evaluate_population_optimises_wide_state_coefficients():
    """gp.py:418-422 with state_size 4 on the HarmonicOscillator: generation 14's 50 best candidates
    get gradient_steps Adam steps through mtgp_ctl_grad; fitness and population equal a CPU
    restatement of the loop driven by the oracle's loss and gradients."""
    e, lib, ff, data, pop = dynamic_setup(P=60, R=4, n_steps=30, depth=4, N=24, seed=12, state_size=4,
                                          env="harmonic")
    strategy = mt.GeneticProgramming(20, 60, ff, lib.operator_list, lib.variable_list, lib.layer_sizes, max_nodes=24,
                                     size_parsinomy=0.01, coefficient_optimisation=True, gradient_steps=3,
                                     verbose=False)
    strategy.current_generation = 14
    fit, newpop = strategy.evaluate_population(pop[None], data)
    d = ff.prepare(data)
    model, ro = oracle_model(ff, d), oracle_rollouts(d)
    raw = orc.evaluate(model, pop, lib, ro)["fitness"]
    idx = np.argsort(raw, kind="stable")[:50]
    cands = pop[idx].copy()
    rows = co.coefficient_rows(cands)
    opt = co.adam()
    states = [opt.init(c[r[:, 0], r[:, 1], 3]) for c, r in zip(cands, rows)]
    hist_c, hist_l = [], []
    for _ in range(3):
        loss, grad, _ = orc.ctl_grad(model, cands, lib, ro)
        hist_c.append(cands.copy())
        hist_l.append(loss)
        for b, r in enumerate(rows):
            v = cands[b][r[:, 0], r[:, 1], 3]
            u, states[b] = opt.update(grad[b, : len(r)], states[b], v)
            cands[b][r[:, 0], r[:, 1], 3] = (v + u).astype(np.float32)
    L = np.stack(hist_l)
    best = np.argmin(L, axis=0)
    want_pop = pop.copy()
    want_pop[idx] = np.stack([hist_c[e_][b] for b, e_ in enumerate(best)])
    want_raw = raw.copy()
    want_raw[idx] = L.min(axis=0)
    counts = (want_pop[..., 0] != 0).sum(axis=(1, 2)).astype(np.float32)
    want = (want_raw + np.float32(0.01) * counts).astype(np.float32)
    assert bits_equal(fit.reshape(-1), want)
    assert np.array_equal(newpop.reshape(pop.shape), want_pop)
    assert (L.min(axis=0) < L[0]).any()  # the optimisation improved some candidate


class _Tampered(co.CoefficientOptimiser):
    """Calls mtgp_ctl_grad itself with this case's buffers and one struct field overwritten; the
    return code is kept."""

    def __init__(self, engine, edit):
        super().__init__(engine, jit=False)
        self.edit, self.rc = edit, None

    def _grad_fn(self):
        native = self.engine.native.mtgp_ctl_grad

        def mtgp_ctl_grad(model, prog, n_prog, L, P, theta, nparam, K, ro, *rest):
            self.edit(model._obj, ro._obj)
            self.rc = native(model, prog, n_prog, L, P, theta, nparam, K, ro, *rest)
            return self.rc

        return mtgp_ctl_grad


@pytest.mark.parametrize("what", ["state_size", "R"])
def test_ctl_grad_refusals_stay(what):
    """state_size 17 and 65 rollouts are argument errors of the C entry: nothing launches."""
    lib, ff, data, pop, *_ = wide_case("acrobot", 4, "rk4", 0.0)

    def edit(model, ro):
        assert isinstance(model, nat.MtgpModel) and isinstance(ro, nat.MtgpRollouts)
        if what == "state_size":
            model.state_size = 17
        else:
            ro.R = 65

    opt = _Tampered(_engine(ff, lib), edit)
    with pytest.raises(RuntimeError, match="rejected the configuration"):
        opt.loss_and_grad(pop, data)
    assert opt.rc == nat.ERR_ARG
    torch.cuda.synchronize()
