"""Device optimise, CPU side: the host twins (mtgp_coef_*_host) run the kernels' core code
(csrc/mtgp_optim_core.h) on the CPU and must equal multitreegp_amd.coefficients -- coefficient_rows,
parameterise, Adam.update + add, the argmin over the epochs -- bit for bit (NaNs as a class where
arithmetic makes them).  Plus memory safety on hostile populations and chunk windows (guard regions
and a sanitized stand-alone program) and argument errors without a GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import multitreegp_amd as mt
from multitreegp_amd import _native as nat
from multitreegp_amd import coefficients as co
from multitreegp_amd.sampling import sample_population

from helpers import CONTROL_OPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARS = [["y1", "y2", "y3", "y4", "a1", "a2", "u"], ["a1", "a2"], ["y1", "y2"]]
B0, T0, N0 = 7, 3, 15


def _lib():
    return mt.NodeLibrary(CONTROL_OPS, VARS, [1, 1, 1])


def aligned(shape, dtype, fill=0):
    """A 16-B aligned array (the entry points refuse a misaligned population)."""
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    raw = np.zeros(n + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    a = raw[off:off + n].view(dtype).reshape(shape)
    a[...] = fill
    return a


def acopy(x):
    a = aligned(x.shape, x.dtype)
    a.view(np.uint8).reshape(-1)[:] = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    return a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_bits_nan_class(a, b):
    """float32 arrays equal bit for bit, except that any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def twin_index(cands):
    lib = nat.load()
    B, T, N, _ = cands.shape
    c = acopy(cands)
    rowidx = np.full((B, T * N), -7, np.int32)
    count = np.full(B, -7, np.int32)
    assert lib.mtgp_coef_index_host(c.ctypes.data, B, T, N, rowidx.ctypes.data, count.ctypes.data) == nat.OK
    return rowidx, count


def twin_parameterise(cands, library, n_data, lo, cap):
    """The device loop's steps on the CPU: index, K from the counts, parameterise."""
    lib = nat.load()
    B, T, N, _ = cands.shape
    c = acopy(cands)
    rowidx, count = twin_index(cands)
    K = max([1] + [min(lo + cap, int(n)) - lo for n in count])
    pop = aligned(cands.shape, np.float32, np.nan)
    theta = np.full((B, K), np.nan, np.float32)
    nparam = np.full(B, -7, np.int32)
    base = library.native()
    rc = lib.mtgp_coef_parameterise_host(c.ctypes.data, B, T, N, ctypes.byref(base), n_data, lo, K, pop.ctypes.data,
                                         theta.ctypes.data, nparam.ctypes.data)
    assert rc == nat.OK
    assert same_bits(c, cands)  # the input is read only
    return pop, theta, nparam, K, rowidx, count


def check_against_parameterise(cands, library, n_data, lo, cap):
    rows = co.coefficient_rows(cands)
    want_pop, want_theta, want_n, want_K, _ = co.parameterise(cands, rows, library, n_data, lo, lo + cap)
    pop, theta, nparam, K, rowidx, count = twin_parameterise(cands, library, n_data, lo, cap)
    N = cands.shape[2]
    for b, r in enumerate(rows):
        assert count[b] == len(r)
        assert np.array_equal(rowidx[b, :len(r)], r[:, 0] * N + r[:, 1]) and np.all(rowidx[b, len(r):] == -1)
    assert K == want_K
    assert same_bits(pop, want_pop), np.argwhere(pop.view(np.uint32) != want_pop.view(np.uint32))[:5]
    assert same_bits(theta, want_theta)
    assert np.array_equal(nparam, want_n)


def sampled(seed=0):
    return sample_population(seed, _lib(), B0, 1, max_init_depth=4, max_nodes=N0)[0]


def hostile(library, n_data, seed=1):
    """[B0, T0, N0, 4] whose f column draws from the values the host rule treats specially."""
    rng = np.random.default_rng(seed)
    top, vs = library.n_funcs - 1, library.var_start
    pool = np.array([np.nan, np.inf, -np.inf, top + 1, top + 5, 1e10, 2.0 ** 31, -2.0 ** 31, -3e9, -3.0, -1.0, -0.0, 0.0,
                     1.0, 1.0, 1.0, 1.0000001, 0.99999994, 3.7, 2.0, vs, vs + n_data - 1, vs + n_data, top - 1, top,
                     vs + 0.5, top + 0.5], np.float32)
    c = rng.standard_normal((B0, T0, N0, 4)).astype(np.float32)
    c[..., 0] = rng.choice(pool, size=(B0, T0, N0))
    c[..., 3][rng.random((B0, T0, N0)) < 0.1] = np.float32(np.nan)
    c[1][..., 0] = np.float32(2.0)  # a candidate with no coefficient rows
    c[2][..., 0] = np.float32(1.0)  # every row a coefficient: T * N = 45 exceeds every cap used here
    return c


WINDOWS = [(0, 4), (4, 4), (64, 4), (0, 40), (40, 40), (0, 57)]  # (lo, cap): first, second, past every count


@pytest.mark.parametrize("n_data", [7, 5])
@pytest.mark.parametrize("lo,cap", WINDOWS)
def test_parameterise_twin_equals_host_rule(lo, cap, n_data):
    """Sampled populations, hostile f columns, a candidate without coefficients and one made of
    them, over the windows (0, cap), (cap, 2 cap) and a lo beyond every count."""
    library = _lib()
    assert library.var_start + n_data + cap <= nat.MAX_FUNCS
    pop = sampled()
    pop[3][..., 0][pop[3][..., 0] == 1.0] = 2.0  # sampled, no coefficient rows
    assert max(len(r) for r in co.coefficient_rows(pop)) > 4
    check_against_parameterise(pop, library, n_data, lo, cap)
    check_against_parameterise(hostile(library, n_data), library, n_data, lo, cap)


# ------------------------------------------------------------------------- Adam
SPECIAL = np.array([0.0, np.inf, -np.inf, np.nan, 1e-21, 1e20, -1e-21, -0.0], np.float32)


def adam_case(seed=2):
    """3 candidates (T 2, N 12) with 12, 5 and 0 coefficient rows, and their index."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((3, 2, 12, 4)).astype(np.float32)
    c[..., 0] = 2.0
    c[0, :, ::2, 0] = 1.0
    c[1, 1, 3:8, 0] = 1.0
    return c


class Twin:
    """The state of one device loop on the CPU (mtgp_coef_adam_step_host, mtgp_coef_scatter_host)."""

    def __init__(self, cands, windows=None):
        self.lib = nat.load()
        self.inp = acopy(cands)
        self.work = acopy(cands)
        self.B, self.T, self.N, _ = cands.shape
        self.rowidx, self.count = twin_index(cands)
        self.M = max(1, int(self.count.max()))
        self.windows = windows or [(0, self.M)]
        shape = (self.B, self.M)
        self.mu, self.nu, self.best_vals = (np.full(shape, np.nan, np.float32) for _ in range(3))
        self.best_loss = np.full(self.B, np.nan, np.float32)
        self.theta = [np.zeros((self.B, K), np.float32) for _, K in self.windows]
        self.t = 0

    def step(self, grads, loss, opt):
        """grads [B, M] over all coefficients of a candidate; every window of the epoch."""
        self.t += 1
        s = opt.scalars(self.t)
        loss = np.ascontiguousarray(loss, np.float32)
        for i, (lo, K) in enumerate(self.windows):
            g = np.zeros((self.B, K), np.float32)
            part = grads[:, lo:lo + K]
            g[:, :part.shape[1]] = part
            rc = self.lib.mtgp_coef_adam_step_host(
                self.work.ctypes.data, self.B, self.T, self.N, self.rowidx.ctypes.data, self.count.ctypes.data, lo, K,
                self.M, g.ctypes.data, loss.ctypes.data, ctypes.byref(s), int(self.t == 1),
                int(i == len(self.windows) - 1), self.mu.ctypes.data, self.nu.ctypes.data, self.best_vals.ctypes.data,
                self.best_loss.ctypes.data, self.theta[i].ctypes.data)
            assert rc == nat.OK

    def scatter(self):
        out = aligned(self.inp.shape, np.float32, np.nan)
        rc = self.lib.mtgp_coef_scatter_host(self.inp.ctypes.data, self.B, self.T, self.N, self.M,
                                             self.best_vals.ctypes.data, out.ctypes.data)
        assert rc == nat.OK
        return out


def values_of(cands, rows):
    return [c[r[:, 0], r[:, 1], 3].copy() for c, r in zip(cands, rows)]


@pytest.mark.parametrize("hyper", [dict(), dict(learning_rate=0.75, b1=0.0, b2=0.97, eps=1e-3, eps_root=1e-6)],
                         ids=["default", "b1_0_eps_root"])
def test_adam_twin_chained_12_steps(hyper):
    """12 chained steps against Adam.update + add: values, moments and theta bit for bit (NaNs as a
    class), with gradients 0, +-inf, NaN, 1e-21 (nu subnormal) and 1e20 (g * g overflows)."""
    cands = adam_case()
    rows = co.coefficient_rows(cands)
    opt = co.Adam(**hyper)
    tw = Twin(cands)
    ref = cands.copy()
    states = [opt.init(v) for v in values_of(ref, rows)]
    rng = np.random.default_rng(5)
    for t in range(12):
        grads = (rng.standard_normal((3, tw.M)) * 10.0 ** rng.integers(-3, 3, (3, tw.M))).astype(np.float32)
        grads[0, :len(SPECIAL)] = np.roll(SPECIAL, t)  # every special value visits every slot's history
        grads[0, 8:11] = [1e-21, 1e20, 0.0]             # ... and slots that see one of them only
        if t == 5:
            grads[1, :len(SPECIAL)] = SPECIAL
        tw.step(grads, np.zeros(3, np.float32), opt)
        for b, r in enumerate(rows):
            v = ref[b][r[:, 0], r[:, 1], 3]
            upd, states[b] = opt.update(grads[b, :len(r)], states[b], v)
            ref[b][r[:, 0], r[:, 1], 3] = (v + upd).astype(np.float32)
            n = len(r)
            assert same_bits_nan_class(tw.mu[b, :n], states[b].mu), (t, b)
            assert same_bits_nan_class(tw.nu[b, :n], states[b].nu), (t, b)
            assert same_bits_nan_class(tw.theta[0][b, :n], ref[b][r[:, 0], r[:, 1], 3]), (t, b)
        assert same_bits_nan_class(tw.work, ref), t
    assert np.isfinite(tw.work[1][..., 3]).any() and np.isnan(tw.work[0][..., 3]).any()
    assert 0 < states[0].nu[8] < np.finfo(np.float32).tiny and np.isinf(states[0].nu[9])  # subnormal, overflowed


LOSSES = np.array([[3.0, 1.0, 5.0, 2.0, 7.0],
                   [1.0, 2.0, 4.0, np.nan, 7.0],
                   [2.0, 3.0, 3.0, 1.0, np.nan],
                   [1.0, 4.0, 2.0, np.nan, 7.0],
                   [5.0, 5.0, 1.0, 0.0, 7.0]], np.float32)  # [epoch, candidate]: tie, rising, last, NaN, NaN at 2


@pytest.mark.parametrize("windows", [None, [(0, 2), (2, 2), (4, 2)]], ids=["one_window", "three_windows"])
def test_best_epoch_tracking_and_scatter(windows):
    """The tracked best equals np.argmin / min over the loss table (a tie at two epochs, a rising
    sequence, the minimum at the last epoch, NaN losses) and the scatter gives hist_c[best]; with
    several windows the best loss is committed by the last one only."""
    rng = np.random.default_rng(8)
    c = rng.standard_normal((5, 1, 8, 4)).astype(np.float32)
    c[..., 0] = 2.0
    for b, n in enumerate([6, 5, 3, 1, 0]):
        c[b, 0, :n, 0] = 1.0
    rows = co.coefficient_rows(c)
    opt = co.Adam(0.1)
    tw = Twin(c, windows)
    hist = []
    for e in range(LOSSES.shape[0]):
        hist.append(np.array(tw.work, copy=True))
        tw.step(rng.standard_normal((5, tw.M)).astype(np.float32), LOSSES[e], opt)
    best = np.argmin(LOSSES, axis=0)
    assert list(best) == [1, 0, 4, 1, 2]
    want = np.stack([hist[e][b] for b, e in enumerate(best)])
    assert same_bits(tw.scatter(), want)
    assert same_bits_nan_class(tw.best_loss, LOSSES.min(axis=0))
    assert not same_bits(hist[1][0], hist[2][0]) and len(rows[4]) == 0  # the values did move


# ------------------------------------------------------------------ memory safety
GUARD = 4096


def guarded(shape, dtype, fill):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    block = np.full(n + 2 * GUARD + 16, 0xA5, np.uint8)
    off = GUARD + (-(block.ctypes.data + GUARD)) % 16
    view = block[off:off + n].view(dtype).reshape(shape)
    view[...] = fill
    return block, view, (off, n)


def intact(block, where):
    off, n = where
    return bool(np.all(block[:off] == 0xA5) and np.all(block[off + n:] == 0xA5))


@pytest.mark.parametrize("kind", ["random_bits", "special_f", "all_coefficients"])
@pytest.mark.parametrize("lo,K", [(0, 4), (4, 4), (1000, 3), (0, 50), (2 ** 31 - 1, 1)])
def test_hostile_populations_stay_inside_their_buffers(kind, lo, K):
    """Random bits, special f values and all-coefficient candidates through every twin, with
    windows inside, across and beyond the counts and an index array of wild values: guard bytes
    around every output stay untouched and inputs are read only."""
    lib = nat.load()
    library = _lib()
    B, T, N = B0, T0, N0
    rng = np.random.default_rng(3)
    if kind == "random_bits":
        bits = rng.integers(0, 2 ** 32, B * T * N * 4, dtype=np.uint64).astype(np.uint32)
        bits[::7] = 0x7FC00000
        bits[::5] = 0x3F800000  # 1.0f
        src = bits.view(np.float32).reshape(B, T, N, 4)
    elif kind == "special_f":
        src = hostile(library, 5)
    else:
        src = np.ones((B, T, N, 4), np.float32)
    cands = acopy(src)
    blocks = {}

    def out(name, shape, dtype, fill):
        blocks[name] = guarded(shape, dtype, fill)
        return blocks[name][1]

    rowidx, count = out("rowidx", (B, T * N), np.int32, 0), out("count", (B,), np.int32, 0)
    assert lib.mtgp_coef_index_host(cands.ctypes.data, B, T, N, rowidx.ctypes.data, count.ctypes.data) == nat.OK
    pop, theta, nparam = out("pop", src.shape, np.float32, 0), out("theta", (B, K), np.float32, 0), out("nparam", (B,), np.int32, 0)
    base = library.native()
    assert lib.mtgp_coef_parameterise_host(cands.ctypes.data, B, T, N, ctypes.byref(base), 5, lo, K, pop.ctypes.data,
                                           theta.ctypes.data, nparam.ctypes.data) == nat.OK
    assert np.all((nparam >= 0) & (nparam <= K))
    M = max(1, int(count.max()))
    work = out("work", src.shape, np.float32, 0)
    work[...] = cands
    mu, nu, bv = (out(n, (B, M), np.float32, 0) for n in ("mu", "nu", "best_vals"))
    bl, th2 = out("best_loss", (B,), np.float32, 0), out("theta2", (B, K), np.float32, 0)
    grad = rng.standard_normal((B, K)).astype(np.float32)
    loss = rng.standard_normal(B).astype(np.float32)
    s = co.Adam().scalars(1)
    for wild in (False, True):
        idx, cnt = rowidx.copy(), count.copy()
        if wild:  # an index array that is not mtgp_coef_index's: still nothing outside the buffers
            idx[...] = rng.choice(np.array([-2 ** 31, -1, 0, T * N - 1, T * N, 2 ** 31 - 1], np.int64), idx.shape)
            cnt[...] = rng.choice(np.array([-5, 0, M, M + 1, 2 ** 31 - 1], np.int64), cnt.shape)
        for first in (1, 0):
            rc = lib.mtgp_coef_adam_step_host(work.ctypes.data, B, T, N, idx.ctypes.data, cnt.ctypes.data, lo, K, M,
                                              grad.ctypes.data, loss.ctypes.data, ctypes.byref(s), first, 1,
                                              mu.ctypes.data, nu.ctypes.data, bv.ctypes.data, bl.ctypes.data,
                                              th2.ctypes.data)
            assert rc == nat.OK
    res = out("out", src.shape, np.float32, 0)
    assert lib.mtgp_coef_scatter_host(cands.ctypes.data, B, T, N, M, bv.ctypes.data, res.ctypes.data) == nat.OK
    for name, (block, _, where) in blocks.items():
        assert intact(block, where), name
    assert same_bits(cands, src)
    assert same_bits(res[..., :3], src[..., :3]) and same_bits(work[..., :3], src[..., :3])  # only values move


_SAN_MAIN = r"""
#include <stdio.h>
#include <string.h>
#include <vector>
#include "mtgp_optim_core.h"
using namespace mtgp_opt;
static uint64_t state = 0x9876543ull;
static uint32_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 32); }
int main() {
  const int B = 5, T = 3, N = 21, TN = T * N;
  const float special[] = {1.0f, 1.0f, 2.0f, -0.0f, 1e10f, -3e9f, 127.0f, 128.0f, 9.0f, 14.5f, 0.99999994f};
  ParamCfg P;
  P.n_funcs = 14, P.var_start = 7, P.n_data = 5;
  for (int i = 0; i < kMaxFuncs; ++i) P.fn[i] = (int8_t)(i >= 7 && i < 14 ? kFnVar : 2);
  const int los[] = {0, 3, 60, 63, 1000, INT32_MAX}, Ks[] = {1, 3, 59};
  for (int round = 0; round < 3; ++round) {
    // heap blocks of the exact size (no slack for the sanitizer to miss)
    std::vector<float> cands((size_t)B * TN * 4), pop(cands.size()), out(cands.size());
    for (size_t i = 0; i < cands.size(); ++i) {
      uint32_t b = rnd();
      if (round == 1) { cands[i] = special[b % 11]; continue; }
      if (round == 2) { cands[i] = 1.0f; continue; }
      if (b % 9 == 0) b = 0x7fc00000u;
      if (b % 5 == 0) b = 0x3f800000u;
      memcpy(&cands[i], &b, 4);
    }
    std::vector<int32_t> rowidx((size_t)B * TN), count(B), nparam(B);
    host_index(cands.data(), B, T, N, rowidx.data(), count.data());
    int M = 1;
    for (int b = 0; b < B; ++b) M = count[b] > M ? count[b] : M;
    for (int lo : los) for (int K : Ks) {
      P.lo = lo, P.K = K;
      if (!param_ok(P)) return 2;
      std::vector<float> theta((size_t)B * K), grad((size_t)B * K), loss(B), mu((size_t)B * M), nu(mu.size()),
          bv(mu.size()), bl(B);
      host_parameterise(cands.data(), B, T, N, P, pop.data(), theta.data(), nparam.data());
      for (int b = 0; b < B; ++b) if (nparam[b] < 0 || nparam[b] > K) return 3;
      for (auto& g : grad) { uint32_t b = rnd(); memcpy(&g, &b, 4); }
      for (auto& l : loss) { uint32_t b = rnd(); if (b % 3 == 0) b = 0x7fc00000u; memcpy(&l, &b, 4); }
      const AdamScalars s = {0.1f, 0.9f, 0.001f, 0.999f, 0.1f, 0.001f, 0.0f, 1e-8f, -0.001f};
      std::vector<float> work = cands;
      for (int e = 0; e < 3; ++e)
        host_adam_step(work.data(), B, T, N, rowidx.data(), count.data(), lo, K, M, grad.data(), loss.data(), s, e == 0,
                       true, mu.data(), nu.data(), bv.data(), bl.data(), e == 1 ? nullptr : theta.data());
      // an index array with wild entries and counts
      std::vector<int32_t> wild(rowidx.size()), wcount(B);
      for (auto& w : wild) w = (int32_t)rnd();
      for (auto& w : wcount) w = (int32_t)rnd();
      host_adam_step(work.data(), B, T, N, wild.data(), wcount.data(), lo, K, M, grad.data(), loss.data(), s, false, true,
                     mu.data(), nu.data(), bv.data(), bl.data(), theta.data());
      host_scatter(cands.data(), B, T, N, M, bv.data(), out.data());
    }
  }
  puts("optim core: clean");
  return 0;
}
"""


def test_hostile_population_under_sanitizers(tmp_path):
    """The core header in a stand-alone program of its own (g++ -fsanitize=address,undefined), run
    as a child process on hostile populations, chunk windows and index arrays."""
    cxx = os.environ.get("CXX", "g++")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 \
            or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitized program can be linked and run here")
    src = tmp_path / "optim_asan.cpp"
    src.write_text(_SAN_MAIN)
    exe = tmp_path / "optim_asan"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", *san, "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "multitreegp_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout, r.stdout + r.stderr


# --------------------------------------------------------------------- arguments
def test_argument_errors_without_a_gpu():
    """Null pointers, limits and misalignment are MTGP_ERR_ARG before any device call, for the
    device entry points (given host memory here: they must return before touching it) and twins."""
    lib = nat.load()
    library = _lib()
    base = library.native()
    vs = library.var_start
    B, T, N, K, M = 2, 2, 8, 3, 4
    c = aligned((B, T, N, 4), np.float32, 1.0)
    pop, res = aligned(c.shape, np.float32), aligned(c.shape, np.float32)
    rowidx, count, nparam = np.zeros((B, T * N), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    theta, grad = np.zeros((B, 64), np.float32), np.zeros((B, 64), np.float32)
    loss, bl = np.zeros(B, np.float32), np.zeros(B, np.float32)
    mu, nu, bv = (np.zeros((B, T * N), np.float32) for _ in range(3))
    s = co.Adam().scalars(1)
    p = lambda a: a.ctypes.data  # noqa: E731
    E = nat.ERR_ARG
    for dev in (True, False):
        tail = (None,) if dev else ()
        index = lib.mtgp_coef_index if dev else lib.mtgp_coef_index_host
        par = lib.mtgp_coef_parameterise if dev else lib.mtgp_coef_parameterise_host
        adam = lib.mtgp_coef_adam_step if dev else lib.mtgp_coef_adam_step_host
        scat = lib.mtgp_coef_scatter if dev else lib.mtgp_coef_scatter_host

        def index_(cp=p(c), n=N, b=B, r=p(rowidx), k=p(count)):
            return index(cp, b, T, n, r, k, *tail)

        assert index_(cp=None) == E and index_(r=None) == E and index_(k=None) == E
        assert index_(n=nat.MAX_NODES + 1) == E and index_(n=0) == E and index_(b=0) == E
        assert index_(cp=p(c) + 4) == E and index_(r=p(rowidx) + 2) == E

        def par_(cp=p(c), n=N, lb=ctypes.byref(base), nd=7, lo=0, k=K, po=p(pop), th=p(theta), npm=p(nparam)):
            return par(cp, B, T, n, lb, nd, lo, k, po, th, npm, *tail)

        assert par_(cp=None) == E and par_(lb=None) == E and par_(po=None) == E and par_(th=None) == E and par_(npm=None) == E
        assert par_(k=0) == E and par_(lo=-1) == E and par_(n=nat.MAX_NODES + 1) == E
        assert par_(nd=7, k=nat.MAX_DATA - 7 + 1) == E and vs + nat.MAX_DATA + 1 <= nat.MAX_FUNCS  # n_data + K > MTGP_MAX_DATA
        big = nat.MtgpNodeLibrary()
        big.n_funcs, big.var_start = nat.MAX_FUNCS, nat.MAX_FUNCS - 8
        assert par_(lb=ctypes.byref(big), nd=7, k=2) == E               # var_start + n_data + K > MTGP_MAX_FUNCS
        big.n_funcs = nat.MAX_FUNCS + 1
        assert par_(lb=ctypes.byref(big)) == E
        assert par_(cp=p(c) + 8) == E and par_(po=p(pop) + 4) == E and par_(po=p(c)) == E

        def adam_(cp=p(c), n=N, r=p(rowidx), cn=p(count), lo=0, k=K, m=M, g=p(grad), l=p(loss), sc=ctypes.byref(s),
                  a=p(mu), b=p(nu), v=p(bv), bl_=p(bl), th=p(theta)):
            return adam(cp, B, T, n, r, cn, lo, k, m, g, l, sc, 1, 1, a, b, v, bl_, th, *tail)

        for name in ("cp", "r", "cn", "g", "l", "sc", "a", "b", "v", "bl_"):
            assert adam_(**{name: None}) == E, name
        assert adam_(k=0) == E and adam_(lo=-1) == E and adam_(m=0) == E and adam_(m=T * N + 1) == E
        assert adam_(n=nat.MAX_NODES + 1) == E and adam_(cp=p(c) + 4) == E and adam_(g=p(grad) + 1) == E

        def scat_(cp=p(c), n=N, m=M, v=p(bv), o=p(res)):
            return scat(cp, B, T, n, m, v, o, *tail)

        assert scat_(cp=None) == E and scat_(v=None) == E and scat_(o=None) == E and scat_(o=p(c)) == E
        assert scat_(m=0) == E and scat_(n=nat.MAX_NODES + 1) == E and scat_(o=p(res) + 8) == E
        if not dev:  # the same arguments are accepted when valid (theta may be NULL)
            assert index_() == nat.OK and par_() == nat.OK and adam_() == nat.OK and adam_(th=None) == nat.OK
            assert scat_() == nat.OK


def test_chunk_windows_and_adam_scalars():
    """chunk_windows restates loss_and_grad's chunking; Adam.scalars are Adam.update's float32 expressions."""
    assert co.chunk_windows([0, 0], 5) == [(0, 1)]
    assert co.chunk_windows([3, 12, 0], 5) == [(0, 5), (5, 5), (10, 2)]
    assert co.chunk_windows([5], 5) == [(0, 5)]
    s = co.Adam(0.001, 0.9, 0.999).scalars(3)
    f = np.float32
    assert f(s.c1) == f(1) - f(0.9) ** f(3) and f(s.neg_lr) == f(-0.001) and f(s.a) == f(1 - 0.9)
