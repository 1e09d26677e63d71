"""The evolution step's one C++ implementation (csrc/mtgp_evolve_core.h) on the CPU, through both
of its drivers: the host library (HostEvolver, csrc/mtgp_evolve.cpp, threads) and the host twins of
libmtgp_hip.so (mtgp_evolve_device_host / mtgp_sample_population_device_host, serial).  Both must
reproduce, bit for bit over whole arrays, the digests recorded from the separate host library this
header replaced (tests/golden/evolve_parity.json) -- same seed, same draws, glibc's log, so no
allowance.  Plus memory safety on malformed populations (guard regions and sanitized stand-alone
programs), the argument domain without a GPU, and the strategy's backend switch."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd.device_evolve import DeviceEvolver
from multitreegp_amd.host import HostEvolver

from helpers import CONTROL_OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARS = [["y1", "y2", "y3", "y4", "a1", "a2", "u"], ["a1", "a2"], ["y1", "y2"]]
TP = [0.6 * 0.4 ** i for i in range(7)]


def _lib(T=3):
    return mt.NodeLibrary(CONTROL_OPS, VARS[:T], [1] * T)


def evolvers(lib, N=40, depth=5, E=0, rtp=(0.9, 0.1, 0.0), num_pop=1, migration_size=0, period=10, rp=1.0):
    """(HostEvolver, DeviceEvolver) of one strategy."""
    args = (lib, N, depth, 1.0, period, migration_size, 7, E, np.tile(TP, (num_pop, 1)),
            np.tile(rtp, (num_pop, 1)), np.full(num_pop, rp), num_pop)
    return HostEvolver(*args), DeviceEvolver(*args)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------- parity
# Each case yields, in order, every array its comparison covers.  `host` samples the parents;
# `side` is what is under test: the HostEvolver itself or the Twin of the DeviceEvolver.
GOLDEN = os.path.join(ROOT, "tests", "golden", "evolve_parity.json")


class Twin:
    def __init__(self, dev):
        self.evolve, self.sample_population = dev.evolve_host, dev.sample_population_host


def _one_generation(host, side):
    parents = host.sample_population(2048, seed=3)
    fit = np.random.default_rng(4).random((1, 2048)).astype(np.float32)
    yield side.evolve(parents, fit, seed=11, current_generation=0)


def _twenty_chained(host, side):
    pops = host.sample_population(128, seed=3)
    rng = np.random.default_rng(0)
    for gen in range(20):
        fit = rng.random((2, 128)).astype(np.float32)
        pops = side.evolve(pops, fit, seed=100 + gen, current_generation=gen).copy()
        yield pops


def _tied_migration(host, side):
    pops = host.sample_population(64, seed=7)
    fit = (np.random.default_rng(8).integers(0, 4, (3, 64)) * 0.25).astype(np.float32)
    yield side.evolve(pops, fit, seed=1, current_generation=0)


def _two_generations(host, side):
    pops = host.sample_population(128, seed=5)
    fit = np.random.default_rng(6).random((1, 128)).astype(np.float32)
    for gen in range(2):
        pops = side.evolve(pops, fit, seed=21 + gen, current_generation=gen).copy()
        yield pops


def _sampled(S):
    def run(host, side):
        yield side.sample_population(S, seed=1)
    return run


RTPS = {"crossover": (1.0, 0.0, 0.0), "mutation": (0.0, 1.0, 0.0), "resample": (0.0, 0.0, 1.0),
        "mixed": (0.9, 0.1, 0.0)}
CHUNKS = {"N64": (64, 10, 3), "N128": (128, 16, 2), "N7": (7, 3, 3)}
SAMPLES = {"3000-40-5": (3000, 40, 5), "64-128-16": (64, 128, 16)}
# case id -> (trees, evolvers() keywords, the arrays it yields)
PARITY_CASES = {
    **{f"one_generation[{k}]": (3, dict(E=40, rtp=rtp), _one_generation) for k, rtp in RTPS.items()},
    "twenty_chained": (3, dict(N=20, depth=4, E=4, rtp=(0.5, 0.4, 0.1), num_pop=2, migration_size=4, period=3),
                       _twenty_chained),
    **{f"tied_migration[{E}]": (3, dict(E=E, num_pop=3, migration_size=6, period=1), _tied_migration)
       for E in (64, 0)},
    **{f"row_chunk_edges[{k}]": (T, dict(N=N, depth=depth, E=8, rtp=(0.5, 0.4, 0.1)), _two_generations)
       for k, (N, depth, T) in CHUNKS.items()},
    **{f"sample_population[{k}]": (3, dict(N=N, depth=depth), _sampled(S)) for k, (S, N, depth) in SAMPLES.items()},
}


def parity_digests(case):
    """{"host": [...], "twin": [...]}: the sha256 of every array of the case, from each side."""
    T, kw, run = PARITY_CASES[case]
    host, dev = evolvers(_lib(T), **kw)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()  # noqa: E731
    return {"host": [sha(a) for a in run(host, host)], "twin": [sha(a) for a in run(host, Twin(dev))]}


def assert_recorded(case):
    """The host library and the twin are one implementation now, so each is held against what the
    two-implementation parent produced: digests of whole arrays recorded from its libmtgp_host.so
    (scripts/record_evolve_parity.py; its twin hashed to the same values)."""
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][case]
    got = parity_digests(case)
    for side in ("host", "twin"):
        assert len(got[side]) == len(want)
        for k, (g, w) in enumerate(zip(got[side], want)):
            assert g == w, f"{side}, array {k}"


@pytest.mark.parametrize("rtp", list(RTPS))
def test_one_generation_equals_host_library(rtp):
    """S 2048, E 40, T 3, N 40, depth 5: about 1,000 pairs per operator mix (the all-mutation case
    runs every one of the seven mutations and both arities of the operator-changing ones)."""
    assert_recorded(f"one_generation[{rtp}]")


def test_twenty_chained_generations_equal():
    """N 20, depth 4 (size limits and retry loops hit constantly), 2 populations, migration size 4
    every 3rd generation, fresh random fitness: equal at every generation."""
    assert_recorded("twenty_chained")


@pytest.mark.parametrize("E", [64, 0])
def test_migration_with_tied_fitness(E):
    """3 populations of 64, migration 6 every generation, fitness quantised to 4 values: the
    stable descending order (receiver) is not the reverse of the stable ascending one (sender,
    elitism), and selection uses the pre-migration fitness."""
    assert_recorded(f"tied_migration[{E}]")


@pytest.mark.parametrize("N,depth,T", list(CHUNKS.values()), ids=list(CHUNKS))
def test_row_chunk_edges(N, depth, T):
    """One 64-row chunk exactly; two chunks with I = 2N - 1 in sample_tree; smaller than a chunk
    (empty < 8 always).  S 128, mixed operators, two generations."""
    assert_recorded(next(f"row_chunk_edges[{k}]" for k, v in CHUNKS.items() if v == (N, depth, T)))


@pytest.mark.parametrize("S,N,depth", list(SAMPLES.values()))
def test_sample_population_equals_host_library(S, N, depth):
    assert_recorded(f"sample_population[{S}-{N}-{depth}]")


# ------------------------------------------------------------------ malformed input
GUARD = 4096  # bytes around every buffer


def _guarded(nbytes, fill):
    """A 16-B aligned uint8 view of nbytes inside a block with GUARD bytes of 0xA5 on both sides."""
    block = np.full(nbytes + 2 * GUARD + 16, 0xA5, np.uint8)
    off = GUARD + (-(block.ctypes.data + GUARD)) % 16
    view = block[off:off + nbytes]
    view[:] = fill
    return block, view, off


def _guards_intact(block, off, nbytes):
    return bool(np.all(block[:off] == 0xA5) and np.all(block[off + nbytes:] == 0xA5))


@pytest.mark.parametrize("kind", ["random_bits", "wild_indices"])
def test_malformed_population_stays_inside_its_buffers(kind):
    """Populations that violate the layout (random bits with NaN, huge and negative f / a / b):
    the result is unspecified, but the call returns and nothing outside the buffers is touched."""
    P, S, T, N = 3, 48, 3, 40
    _, dev = evolvers(_lib(), N=N, depth=5, E=6, rtp=(0.4, 0.5, 0.1), num_pop=P, migration_size=5, period=1)
    rng = np.random.default_rng(17)
    n = P * S * T * N * 4
    if kind == "random_bits":
        bits = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        bits[::7] = 0x7FC00000  # NaN
        pop_bytes = bits.view(np.uint8)
    else:  # plausible magnitudes, wrong structure
        rows = np.empty((P * S * T * N, 4), np.float32)
        rows[:, 0] = rng.integers(-3, len(dev._slots) + 3, len(rows))
        rows[:, 1] = rng.integers(-5, N + 5, len(rows))
        rows[:, 2] = rng.choice(np.array([-1e30, -7, -1, 0, 3, N - 1, N, 2**31, 1e30, np.nan], np.float32), len(rows))
        rows[:, 3] = rng.standard_normal(len(rows))
        pop_bytes = rows.view(np.uint8).reshape(-1)
    fit_bits = rng.integers(0, 2**32, P * S, dtype=np.uint64).astype(np.uint32)
    fit_bits[::5] = 0x7FC00000
    pb, pv, po = _guarded(n * 4, pop_bytes)
    fb, fv, fo = _guarded(P * S * 4, fit_bits.view(np.uint8))
    ob, ov, oo = _guarded(n * 4, 0)
    before = pv.copy()
    dev.cfg.current_generation = 0
    rc = dev.hip.mtgp_evolve_device_host(pv.ctypes.data, fv.ctypes.data, P, S, T, N, ctypes.addressof(dev.cfg),
                                         5, ov.ctypes.data)
    assert rc == S
    assert _guards_intact(pb, po, n * 4) and _guards_intact(fb, fo, P * S * 4) and _guards_intact(ob, oo, n * 4)
    assert np.array_equal(pv, before)  # inputs are read only


_SAN_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mtgp_host.h"
static uint64_t state = 0x1234567ull;
static uint32_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 32); }
// S 32, T 2: too few tree rows for a second thread (the driver's serial path); S 352, T 64: 174
// pairs of 1536 rows and 1056 sampled candidates, four threads' worth for both entries
static int run(int S, int T) {
  const int P = 3, N = 24, n_funcs = 8, n_ops = 3, n_vars = 3;
  int32_t slots[n_funcs] = {0, 0, 2, 2, 1, 0, 0, 0}, op_index[n_ops] = {2, 3, 4};
  double op_prob[n_ops] = {0.5, 0.3, 0.2}, tp[P * 4], rtp[P * 3] = {0.4, 0.5, 0.1, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0},
         rp[P] = {1.0, 0.7, 0.5};
  std::vector<float> var_mask((size_t)T * n_vars, 1.0f);
  for (int t = 1; t < T; t += 2) var_mask[(size_t)t * n_vars] = 0.0f;
  for (int i = 0; i < P * 4; ++i) tp[i] = 0.25;
  MtgpEvolveConfig c = {n_funcs, slots, n_ops, op_index, op_prob, 5, n_vars, var_mask.data(), 4, 1.0f, 0, 1, 5, 4, 4,
                        tp, rtp, rp};
  const size_t n = (size_t)P * S * T * N * 4;
  for (int round = 0; round < 3; ++round) {
    // heap blocks of the exact size (no slack for the sanitizer to miss)
    std::vector<float> pops(n), out(n), fit((size_t)P * S);
    for (size_t i = 0; i < n; ++i) {
      uint32_t b = rnd();
      if (round == 1) {  // small integers in and around the valid ranges
        const float v = (float)((int)(b % 40) - 8);
        pops[i] = v;
        continue;
      }
      if (b % 9 == 0) b = 0x7fc00000u;
      memcpy(&pops[i], &b, 4);
    }
    if (round == 2) {  // valid parents, hostile fitness only
      if (mtgp_sample_population(P, S, T, N, &c, 9, pops.data()) != 0) return 2;
    }
    for (size_t i = 0; i < fit.size(); ++i) {
      uint32_t b = rnd();
      if (b % 4 == 0) b = 0x7fc00000u;
      memcpy(&fit[i], &b, 4);
    }
    for (int gen = 0; gen < 2; ++gen) {
      c.current_generation = gen;
      if (mtgp_evolve_populations(pops.data(), fit.data(), P, S, T, N, &c, 77 + gen, out.data()) != S) return 3;
      if (round == 2) pops = out;
    }
  }
  return 0;
}
int main() {
  if (int rc = run(32, 2)) return rc;
  if (int rc = run(352, 64)) return rc;
  puts("evolve core: clean");
  return 0;
}
"""


def _sanitized_run(tmp_path, san):
    """The host library's translation unit (the core header behind its threaded driver) in a
    stand-alone program of its own, compiled with `san` and run as a child process with 4 threads
    on malformed populations and fitness."""
    cxx = os.environ.get("CXX", "g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <thread>\nint main() { std::thread t([] {}); t.join(); return 0; }\n")
    if subprocess.run([cxx, *san, "-pthread", str(probe), "-o", str(tmp_path / "probe")],
                      capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no program sanitized this way can be linked and run here")
    src = tmp_path / "evo_san.cpp"
    src.write_text(_SAN_MAIN)
    exe = tmp_path / "evo_san"
    csrc = os.path.join(ROOT, "multitreegp_amd", "csrc")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-pthread", *san, "-I",
                    os.path.join(ROOT, "include"), "-I", csrc, str(src), os.path.join(csrc, "mtgp_evolve.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env={**os.environ, "MTGP_HOST_THREADS": "4"})
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout + r.stderr


def test_malformed_population_under_sanitizers(tmp_path):
    """g++ -fsanitize=address,undefined: no access outside the buffers, no undefined arithmetic."""
    _sanitized_run(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_threaded_driver_under_thread_sanitizer(tmp_path):
    """g++ -fsanitize=thread: the workers share only what they read."""
    _sanitized_run(tmp_path, ["-fsanitize=thread"])


# --------------------------------------------------------------------- arguments
def test_argument_errors_without_a_gpu():
    """Null pointers, N > 256, elite > population, tournament_size over the kernel's bound and a
    misaligned base pointer are MTGP_ERR_ARG before any device call."""
    host, dev = evolvers(_lib(), E=4)
    lib, cfg = dev.hip, dev.cfg
    P, S, T, N = 1, 16, 3, 40
    pops = host.sample_population(S, seed=0)
    fit = np.zeros((P, S), np.float32)
    out = np.empty_like(pops)
    blob = np.zeros(len(dev._blob_host) + 16, np.uint8)
    blob = blob[(-blob.ctypes.data) % 16:][:len(dev._blob_host)]
    ws = np.zeros(lib.mtgp_evolve_workspace_bytes(P, S) // 4, np.int32)
    assert len(ws) == 2 * P * S

    def device(p=pops.ctypes.data, f=fit.ctypes.data, s=S, n=N, c=ctypes.addressof(cfg), b=blob.ctypes.data,
               w=ws.ctypes.data, o=out.ctypes.data):
        return lib.mtgp_evolve_device(p, f, P, s, T, n, c, b, 1, w, o, None)

    def twin(p=pops.ctypes.data, f=fit.ctypes.data, s=S, n=N, c=ctypes.addressof(cfg), o=out.ctypes.data):
        return lib.mtgp_evolve_device_host(p, f, P, s, T, n, c, 1, o)

    for call in (device, twin):
        assert call(p=None) == nat.ERR_ARG and call(f=None) == nat.ERR_ARG and call(o=None) == nat.ERR_ARG
        assert call(c=None) == nat.ERR_ARG
        assert call(n=257) == nat.ERR_ARG
        assert call(s=2) == nat.ERR_ARG  # elite_size 4 > pop_size 2
        assert call(p=pops.ctypes.data + 4) == nat.ERR_ARG and call(o=out.ctypes.data + 8) == nat.ERR_ARG
    assert device(b=None) == nat.ERR_ARG and device(w=None) == nat.ERR_ARG
    assert twin() == S  # the same arguments are accepted when valid
    _, wide = evolvers(_lib())
    wide.cfg.tournament_size = nat.EVOLVE_MAX_TOURNAMENT + 1
    tp = np.ones(nat.EVOLVE_MAX_TOURNAMENT + 1)
    wide.cfg.tournament_prob = tp.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert device(c=ctypes.addressof(wide.cfg)) == nat.ERR_ARG and twin(c=ctypes.addressof(wide.cfg)) == nat.ERR_ARG
    assert lib.mtgp_evolve_config_pack(ctypes.addressof(wide.cfg), 1, 3, None, 0) == nat.ERR_ARG
    assert lib.mtgp_sample_population_device(P, S, T, 257, ctypes.addressof(cfg), blob.ctypes.data, 1,
                                             out.ctypes.data, None) == nat.ERR_ARG
    assert lib.mtgp_sample_population_device(P, S, T, N, ctypes.addressof(cfg), None, 1, out.ctypes.data,
                                             None) == nat.ERR_ARG
    assert lib.mtgp_sample_population_device_host(P, S, T, N, ctypes.addressof(cfg), 1, None) == nat.ERR_ARG
    assert lib.mtgp_evolve_workspace_bytes(0, 8) == nat.ERR_ARG
    with pytest.raises(ValueError):
        dev.evolve_host(pops[:, :, :2], fit, 0, 0)


@pytest.mark.parametrize("what", ["N257", "tournament65", "reproduction_prob0"])
def test_host_library_rejects_what_the_device_rejects(what):
    """The host entries take the core's argument domain (include/mtgp_host.h): trees over 256
    nodes, tournaments over 64 and a reproduction probability of 0 (tree_mask would redraw for
    ever) are ValueErrors from HostEvolver.evolve and sample_population alike."""
    N, ts, rp = {"N257": (257, 7, 1.0), "tournament65": (40, 65, 1.0), "reproduction_prob0": (40, 7, 0.0)}[what]
    ev = HostEvolver(_lib(), N, 5, 1.0, 10, 0, ts, 0, np.ones((1, ts)), np.array([[0.9, 0.1, 0.0]]), np.array([rp]), 1)
    pops = np.zeros((1, 8, 3, N, 4), np.float32)
    pops[..., N - 1, 0] = 1.0  # every tree one coefficient: a valid population
    pops[..., 1:3] = -1.0
    with pytest.raises(ValueError):
        ev.evolve(pops, np.zeros((1, 8), np.float32), seed=1, current_generation=0)
    with pytest.raises(ValueError):
        ev.sample_population(8, seed=1)
    ok = HostEvolver(_lib(), 256, 5, 1.0, 10, 0, 64, 0, np.ones((1, 64)), np.array([[0.9, 0.1, 0.0]]),
                     np.array([1e-3]), 1)  # the bounds themselves are inside the domain
    assert ok.evolve(ok.sample_population(8, seed=1), np.zeros((1, 8), np.float32), 1, 0).shape == (1, 8, 3, 256, 4)


def test_host_library_takes_any_float_aligned_array():
    """The 16-byte rule is the device entry's and the twins' (test_argument_errors_without_a_gpu);
    mtgp_evolve_populations and mtgp_sample_population copy rows with memcpy: arrays 4 bytes off a
    16-byte boundary give the bits of aligned ones."""
    host, _ = evolvers(_lib(), E=4, rtp=(0.5, 0.4, 0.1), num_pop=2, migration_size=3, period=1)
    S = 48

    def off4(shape):
        raw = np.zeros(int(np.prod(shape)) + 8, np.float32)
        a = raw[(-raw.ctypes.data // 4) % 4 + 1:][:int(np.prod(shape))].reshape(shape)
        assert a.ctypes.data % 16 == 4
        return a

    pops = host.sample_population(S, seed=2)
    fit = np.random.default_rng(1).random((2, S)).astype(np.float32)
    ref = host.evolve(pops, fit, seed=9, current_generation=0)
    assert pops.ctypes.data % 16 == 0 and ref.ctypes.data % 16 == 0
    p4, o4, s4 = off4(pops.shape), off4(ref.shape), off4(pops.shape)
    p4[:] = pops
    assert same_bits(host.evolve(p4, fit, seed=9, current_generation=0), ref)  # the input alone
    f32p = ctypes.POINTER(ctypes.c_float)
    rc = host.lib.mtgp_evolve_populations(p4.ctypes.data_as(f32p), fit.ctypes.data_as(f32p), 2, S, 3, host.N,
                                          ctypes.byref(host.cfg), 9, o4.ctypes.data_as(f32p))
    assert rc == S and same_bits(o4, ref)  # input and output
    assert host.lib.mtgp_sample_population(2, S, 3, host.N, ctypes.byref(host.cfg), 2, s4.ctypes.data_as(f32p)) == 0
    assert same_bits(s4, pops)


def test_strategy_accepts_the_device_backend():
    env = mt.Acrobot(0.0, 0.0)
    ff = mt.DynamicEvaluator(env, 2, 0.05, solver=mt.RK4())
    kw = dict(max_nodes=30, migration_percentage=0.125, elite_percentage=0.125, verbose=False)
    gp = mt.GeneticProgramming(2, 32, ff, CONTROL_OPS, VARS[:2], [2, 1], evolve_backend="device", **kw)
    assert gp.evolve_backend == "device"
    with pytest.raises(ValueError):
        mt.GeneticProgramming(2, 32, ff, CONTROL_OPS, VARS[:2], [2, 1], evolve_backend="jax", **kw)
