"""Device optimise on the GPU: CoefficientOptimiser.optimise of a CUDA tensor (index, parameterise,
gradient, fused track + Adam, scatter, all on the device: csrc/mtgp_optim.hip) against optimise of
the same candidates as numpy from the same build -- the host loop, which tests/test_coefficients.py
pins to the oracle.  Fitness and candidates are compared as uint32 views (NaN as a class); every
case runs 6 epochs, so Adam and the best-epoch choice are exercised."""
import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import coefficients as co

from helpers import SR_OPS, bits_equal, dynamic_setup, mismatch_report, sr_setup, static_setup, tree_from_expr

pytestmark = pytest.mark.gpu
N_EPOCH = 6


def _optimiser(ff, lib):
    import torch
    from multitreegp_amd.engine import DeviceEngine
    return co.CoefficientOptimiser(DeviceEngine(ff, lib, 0.0, torch.device("cuda", 0)))


def _compare(opt, pop, data, optimiser=None, n_epoch=N_EPOCH):
    """optimise(numpy) and optimise(CUDA tensor) -> the reference (fitness, candidates); the
    device run must not enter the host loop (loss_and_grad)."""
    import torch
    ref_fit, ref_pop = opt.optimise(pop, data, n_epoch, optimiser)
    host_loop = opt.loss_and_grad

    def no_host_loop(*a, **k):
        raise AssertionError("the device loop called loss_and_grad")

    opt.loss_and_grad = no_host_loop
    try:
        fit, out = opt.optimise(torch.from_numpy(pop).cuda(), data, n_epoch, optimiser)
    finally:
        opt.loss_and_grad = host_loop
    assert fit.is_cuda and out.is_cuda and fit.dtype == torch.float32 and out.dtype == torch.float32
    assert tuple(out.shape) == pop.shape and tuple(fit.shape) == (pop.shape[0],)
    fit, out = fit.cpu().numpy(), out.cpu().numpy()
    assert bits_equal(fit, ref_fit), mismatch_report(fit, ref_fit, "fitness")
    assert bits_equal(out, ref_pop), mismatch_report(out, ref_pop, "candidates")
    return ref_fit, ref_pop


def _sr(P, R, seed, euler=False, dopri5=False, n_var=2):
    solver = (1e-6, 1e-6, 0.001, 500) if dopri5 else None
    env, lib, ff, data, pop = sr_setup(P=P, R=R, n_save=9, save_every=2, h=0.05, depth=4, N=20, seed=seed, n_var=n_var,
                                       solver=solver)
    if euler:
        ff = mt.SREvaluator(solver=mt.Euler(), dt0=0.05)
    return lib, ff, data, pop


@pytest.mark.parametrize("euler", [False, True], ids=["rk4", "euler"])
def test_sr_fixed_step(euler):
    """SR, n_var 2, B 6, N 20, R 4, 9 save points (the register kernel with dual-number code)."""
    lib, ff, data, pop = _sr(6, 4, 3, euler=euler)
    assert sum(len(r) for r in co.coefficient_rows(pop)) > 6
    _compare(_optimiser(ff, lib), pop, data)


def test_sr_dopri5():
    """SR with Dopri5 + PID at the sizes of test_gpu_sr_grad_dopri5_bitexact's smallest case."""
    lib, ff, data, pop = _sr(24, 8, 23, dopri5=True)
    ref_fit, ref_pop = _compare(_optimiser(ff, lib), pop, data)
    assert not bits_equal(ref_pop, pop)  # some candidate's best epoch came after an Adam step


def test_dynamic_acrobot_register_path():
    """Dynamic Acrobot, B 5, R 3, 16 steps: state_size 2, the register kernel with the dual JIT."""
    env, lib, ff, data, pop = dynamic_setup(P=5, R=3, n_steps=16, depth=4, N=24, seed=5)
    opt = _optimiser(ff, lib)
    _compare(opt, pop, data)
    assert opt.use_jit and opt.last_jit_info is not None


def test_static_harmonic_oscillator_with_observation_noise():
    env, lib, ff, data, pop = static_setup(P=5, R=3, n_steps=16, seed=5, env="harmonic", obs_noise=0.1)
    _compare(_optimiser(ff, lib), pop, data)


def test_dynamic_state_size_4_interpreted():
    """state_size 4, B 4, R 3: the interpreted LDS-column kernel (no dual-number code)."""
    env, lib, ff, data, pop = dynamic_setup(P=4, R=3, n_steps=16, depth=4, N=24, seed=5, state_size=4)
    opt = _optimiser(ff, lib)
    _compare(opt, pop, data)
    assert opt.last_jit_info is None


def test_several_chunks_reparameterise_every_epoch():
    """More coefficients than one launch holds (cap forced to 3, as test_gpu_sr_grad_chunks): the
    other chunks' coefficients are literals, so the device loop re-parameterises per epoch."""
    lib, ff, data, pop = _sr(16, 4, 7)
    opt = _optimiser(ff, lib)
    opt.param_cap = lambda n_data: 3
    counts = [len(r) for r in co.coefficient_rows(pop)]
    assert max(counts) > 6 and len(co.chunk_windows(counts, 3)) >= 3
    ref_fit, ref_pop = _compare(opt, pop, data)
    assert not bits_equal(ref_pop, pop)


def test_candidate_without_coefficients_and_blown_up_candidate():
    """A batch with a candidate that has no coefficient rows and one whose solve diverges (loss =
    max_fitness, zero gradient): both come back unchanged."""
    lib, ff, data, pop = _sr(4, 4, 11)
    N = pop.shape[2]
    plain = np.stack([tree_from_expr(("+", "x0", "x1"), lib, N), tree_from_expr(("-", "x0", "x1"), lib, N)])
    blown = np.stack([tree_from_expr(("*", 1e30, ("*", "x0", "x0")), lib, N),
                      tree_from_expr(("*", 1e30, ("*", "x1", "x1")), lib, N)])
    batch = np.concatenate([pop[:2], plain[None], pop[2:], blown[None]]).astype(np.float32)
    rows = co.coefficient_rows(batch)
    assert len(rows[2]) == 0 and len(rows[5]) == 2
    ref_fit, ref_pop = _compare(_optimiser(ff, lib), batch, data)
    assert ref_fit[5] == np.float32(ff.max_fitness)
    assert bits_equal(ref_pop[2], batch[2]) and bits_equal(ref_pop[5], batch[5])


class _WrappedAdam:
    """an optax-style object that is not the built-in optimiser: takes the host loop"""

    def __init__(self):
        self.inner = co.adam(0.01)

    def init(self, params):
        return self.inner.init(params)

    def update(self, g, state, params=None):
        return self.inner.update(g, state, params)


def test_custom_optimiser_on_cuda_input_takes_the_host_loop():
    import torch
    lib, ff, data, pop = _sr(6, 4, 3)
    opt = _optimiser(ff, lib)
    ref_fit, ref_pop = opt.optimise(pop, data, N_EPOCH, _WrappedAdam())

    def no_device_loop(*a, **k):
        raise AssertionError("a custom optimiser entered the device loop")

    opt._optimise_device = no_device_loop
    fit, out = opt.optimise(torch.from_numpy(pop).cuda(), data, N_EPOCH, _WrappedAdam())
    assert fit.is_cuda and out.is_cuda
    assert bits_equal(fit.cpu().numpy(), ref_fit) and bits_equal(out.cpu().numpy(), ref_pop)
    # ... and the built-in optimiser with the same hyperparameters on the device gives the same
    del opt._optimise_device
    fit2, out2 = opt.optimise(torch.from_numpy(pop).cuda(), data, N_EPOCH, co.adam(0.01))
    assert bits_equal(fit2.cpu().numpy(), ref_fit) and bits_equal(out2.cpu().numpy(), ref_pop)


def test_whole_optimising_generation(monkeypatch):
    """GeneticProgramming at generation 14 with gradient_steps 5: a CUDA-tensor population gives
    the numpy-input run's fitness, population, best_fitnesses and best_solutions bit for bit, with
    the device loop (default) and with MTGP_OPT_DEVICE=0."""
    import torch
    lib, ff, data, pop = _sr(60, 4, 9)

    def run(population):
        s = mt.GeneticProgramming(20, 60, ff, SR_OPS, [["x0", "x1"]], [2], max_nodes=20, size_parsinomy=0.01,
                                  coefficient_optimisation=True, gradient_steps=5, verbose=False)
        s.current_generation = 14
        fit, newpop = s.evaluate_population(population, data)
        return fit, newpop, s.best_fitnesses[14], s.best_solutions[14]

    ref = run(pop[None])
    assert not bits_equal(ref[1][0], pop)  # the optimisation changed some candidate
    for knob in (None, "0"):
        if knob is None:
            monkeypatch.delenv("MTGP_OPT_DEVICE", raising=False)
        else:
            monkeypatch.setenv("MTGP_OPT_DEVICE", knob)
        fit, newpop, bf, bs = run(torch.from_numpy(pop[None]).cuda())
        assert fit.is_cuda and newpop.is_cuda
        assert bits_equal(fit.cpu().numpy(), ref[0]), (knob, mismatch_report(fit.cpu().numpy(), ref[0], "fitness"))
        assert bits_equal(newpop.cpu().numpy(), ref[1]), knob
        assert bits_equal(bf, ref[2]) and bits_equal(bs, ref[3]), knob
