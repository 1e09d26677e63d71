"""Device evolve on the GPU (csrc/mtgp_evolve.hip, multitreegp_amd.device_evolve) against the host
library (HostEvolver), under the parity contract: columns f, a, b of every row bit-identical;
values bit-identical except where the device's f64 log rounds differently inside a normal draw --
no value off by more than 1 float32 ulp, and at most 0.1 % of the non-empty rows off at all.  Then
the strategy's device path: value semantics, evaluate_population on a CUDA tensor, a whole loop."""
import numpy as np
import pytest
import torch

import multitreegp_amd as mt
from helpers import CONTROL_OPS, SR_OPS, sr_setup
from test_device_evolve_host import VARS, _lib, evolvers

pytestmark = pytest.mark.gpu


def _ordered(x):
    """float32 bits as integers ordered like the floats (adjacent floats differ by 1)."""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def assert_parity(got, ref, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == ref.shape, what
    for col, name in enumerate("fab"):
        assert np.array_equal(got[..., col].view(np.uint32), ref[..., col].view(np.uint32)), f"{what}: column {name}"
    ulps = np.abs(_ordered(got[..., 3]) - _ordered(ref[..., 3]))
    off = int(np.count_nonzero(ulps))
    rows = int(np.count_nonzero(ref[..., 0]))
    print(f"{what}: {off} of {rows} non-empty rows with a value 1 ulp off")
    assert ulps.max(initial=0) <= 1, f"{what}: a value differs by {ulps.max()} ulp"
    assert off <= 0.001 * rows, f"{what}: {off} of {rows} values differ"
    return off


@pytest.mark.parametrize("rtp", [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.9, 0.1, 0.0)],
                         ids=["crossover", "mutation", "resample", "mixed"])
def test_one_generation(rtp):
    host, dev = evolvers(_lib(), E=40, rtp=rtp)
    parents = host.sample_population(2048, seed=3)
    fit = np.random.default_rng(4).random((1, 2048)).astype(np.float32)
    ref = host.evolve(parents, fit, seed=11, current_generation=0)
    assert_parity(dev.evolve(parents, fit, seed=11, current_generation=0), ref, "generation")


def test_twenty_chained_generations():
    host, dev = evolvers(_lib(), N=20, depth=4, E=4, rtp=(0.5, 0.4, 0.1), num_pop=2, migration_size=4, period=3)
    pops = host.sample_population(128, seed=3)
    rng = np.random.default_rng(0)
    for gen in range(20):
        fit = rng.random((2, 128)).astype(np.float32)
        ref = host.evolve(pops, fit, seed=100 + gen, current_generation=gen)
        assert_parity(dev.evolve(pops, fit, seed=100 + gen, current_generation=gen), ref, f"generation {gen}")
        pops = ref.copy()


@pytest.mark.parametrize("E", [64, 0])
def test_migration_with_tied_fitness(E):
    host, dev = evolvers(_lib(), E=E, num_pop=3, migration_size=6, period=1)
    pops = host.sample_population(64, seed=7)
    fit = (np.random.default_rng(8).integers(0, 4, (3, 64)) * 0.25).astype(np.float32)
    ref = host.evolve(pops, fit, seed=1, current_generation=0)
    assert_parity(dev.evolve(pops, fit, seed=1, current_generation=0), ref, f"E {E}")


@pytest.mark.parametrize("N,depth,T", [(64, 10, 3), (128, 16, 2), (7, 3, 3)], ids=["N64", "N128", "N7"])
def test_row_chunk_edges(N, depth, T):
    host, dev = evolvers(_lib(T), N=N, depth=depth, E=8, rtp=(0.5, 0.4, 0.1))
    pops = host.sample_population(128, seed=5)
    fit = np.random.default_rng(6).random((1, 128)).astype(np.float32)
    for gen in range(2):
        ref = host.evolve(pops, fit, seed=21 + gen, current_generation=gen)
        assert_parity(dev.evolve(pops, fit, seed=21 + gen, current_generation=gen), ref, f"N {N} generation {gen}")
        pops = ref.copy()


@pytest.mark.parametrize("S,N,depth", [(3000, 40, 5), (64, 128, 16)])
def test_sample_population(S, N, depth):
    host, dev = evolvers(_lib(), N=N, depth=depth)
    got = dev.sample_population(S, seed=1)
    assert got.is_cuda and got.dtype == torch.float32
    assert_parity(got, host.sample_population(S, seed=1), f"sample N {N}")


def _overlap(a, b):
    lo_a, lo_b = a.data_ptr(), b.data_ptr()
    return lo_a < lo_b + b.numel() * 4 and lo_b < lo_a + a.numel() * 4


def test_value_semantics():
    """Returned generations the caller keeps are never written again, and an output never shares
    memory with its input."""
    _, dev = evolvers(_lib(), E=4, rtp=(0.5, 0.4, 0.1))
    cur = dev.sample_population(64, seed=2)
    fit = torch.rand((1, 64), device=cur.device, generator=torch.Generator(cur.device).manual_seed(1))
    kept, snaps = [], []
    for g in range(8):
        nxt = dev.evolve(cur, fit, seed=50 + g, current_generation=g)
        assert not _overlap(nxt, cur) and not _overlap(nxt, fit)
        assert all(not _overlap(nxt, k) for k in kept)
        if g < 3:
            kept.append(nxt)
            snaps.append(nxt.cpu().numpy().copy())
        cur = nxt
    torch.cuda.synchronize()
    for k, s in zip(kept, snaps):
        assert np.array_equal(k.cpu().numpy().view(np.uint32), s.view(np.uint32))


def _acrobot_gp(parsimony, backend="device", generations=8):
    env = mt.Acrobot(0.0, 0.0)
    ff = mt.DynamicEvaluator(env, 2, 0.05, solver=mt.RK4())
    gp = mt.GeneticProgramming(generations, 32, ff, CONTROL_OPS, VARS[:2], [2, 1], num_populations=2, max_nodes=30,
                               max_init_depth=5, size_parsinomy=parsimony, migration_period=2,
                               migration_percentage=0.125, elite_percentage=0.125, verbose=False,
                               evolve_backend=backend)
    return gp, mt.control_data(env, 8, 0.05, None, seed=1, n_steps=40)


@pytest.mark.parametrize("parsimony", [0.0, 0.25])
def test_evaluate_population_follows_its_input(parsimony):
    """A CUDA-tensor population gives CUDA tensors with the fitness, best_solutions and
    best_fitnesses of the same population as numpy, bit for bit."""
    gp_d, data = _acrobot_gp(parsimony)
    gp_n, _ = _acrobot_gp(parsimony, backend="native")
    pops = gp_d.initialize_population(5)
    assert pops.is_cuda and tuple(pops.shape) == (2, 32, 3, 30, 4)
    fit_d, back_d = gp_d.evaluate_population(pops, data)
    fit_n, back_n = gp_n.evaluate_population(pops.cpu().numpy(), data)
    assert fit_d.is_cuda and back_d.is_cuda and isinstance(fit_n, np.ndarray) and isinstance(back_n, np.ndarray)
    assert tuple(fit_d.shape) == (2, 32) and back_d.shape == pops.shape
    assert np.array_equal(fit_d.cpu().numpy().view(np.uint32), fit_n.view(np.uint32))
    assert np.array_equal(back_d.cpu().numpy().view(np.uint32), back_n.view(np.uint32))
    assert np.array_equal(gp_d.best_fitnesses.view(np.uint32), gp_n.best_fitnesses.view(np.uint32))
    assert np.array_equal(gp_d.best_solutions.view(np.uint32), gp_n.best_solutions.view(np.uint32))


def test_five_generation_device_loop():
    """initialize_population -> evaluate -> evolve on the device with a real evaluator; at each
    generation the device children equal HostEvolver.evolve of the downloaded device parents and
    device fitness (one-step parity along the device trajectory)."""
    from multitreegp_amd.host import HostEvolver
    gp, data = _acrobot_gp(0.0)
    host = HostEvolver.for_strategy(gp)
    pops = gp.initialize_population(9)
    for g in range(5):
        assert gp.current_generation == g
        fit, pops = gp.evaluate_population(pops, data)
        children = gp.evolve(pops, fit, 40 + g)
        assert children.is_cuda and tuple(children.shape) == (2, 32, 3, 30, 4) and tuple(fit.shape) == (2, 32)
        ref = host.evolve(pops.cpu().numpy(), fit.cpu().numpy(), 40 + g, g)
        assert_parity(children, ref, f"loop generation {g}")
        pops = children
    assert gp.current_generation == 5


def test_optimising_generation_on_a_device_population():
    """coefficient_optimisation at a generation that optimises (g = 14): a CUDA-tensor population
    gives the numpy-input result bit for bit."""
    env, lib, ff, data, pop = sr_setup(P=64, R=4, n_save=9, save_every=2, h=0.05, depth=4, N=20, seed=9)

    def run(as_tensor):
        gp = mt.GeneticProgramming(20, 64, ff, SR_OPS, [["x0", "x1"]], [2], max_nodes=20, size_parsinomy=0.01,
                                   migration_percentage=0.125, elite_percentage=0.125,
                                   coefficient_optimisation=True, gradient_steps=1, verbose=False,
                                   evolve_backend="device" if as_tensor else "native")
        gp.current_generation = 14
        p = torch.from_numpy(pop[None]).cuda() if as_tensor else pop[None]
        fit, back = gp.evaluate_population(p, data)
        if as_tensor:
            assert fit.is_cuda and back.is_cuda
            fit, back = fit.cpu().numpy(), back.cpu().numpy()
        return fit, back, gp.best_fitnesses.copy(), gp.best_solutions.copy()

    for a, b in zip(run(True), run(False)):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
