"""Truth tables of the variant dispatcher (multitreegp_amd/csrc/mtgp_variants.h), on the CPU.

The launch layer picks a kernel instantiation from run-time flags through these wrappers, so this is
the one place that pins template position to flag name: a swapped NOISE would launch a noise kernel
without a key pointer, and a swapped JIT cannot be seen in any result (JIT and interpreter are
bit-identical by design).  A stand-alone program that includes only the header runs every input
combination of every wrapper under AddressSanitizer and UBSan."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include "mtgp_variants.h"
#include <cstdio>
#include <cstdlib>

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); ++g_fail; } \
  } while (0)

// a constant must be usable as a template argument, as a kernel launch uses it
template <bool B> struct Flag { static constexpr bool value = B; };
template <int I> struct Int { static constexpr int value = I; };

template <bool kTrajOnly>
static void ctl_table() {
  for (int m = 0; m < 8; ++m) {
    const bool traj = m & 1, noise = m & 2, jit = m & 4;
    int calls = 0;
    mtgp::ctl_variant<kTrajOnly>(traj, noise, jit, [&](auto T, auto N, auto J) {
      ++calls;
      CHECK(Flag<T()>::value == traj);
      CHECK(Flag<N()>::value == noise);
      CHECK(Flag<J()>::value == jit);
      if (kTrajOnly) CHECK(Flag<T()>::value);
    });
    CHECK(calls == (kTrajOnly && !traj ? 0 : 1));
  }
  for (int m = 0; m < 4; ++m) {
    const bool traj = m & 1, noise = m & 2;
    int calls = 0;
    mtgp::ctl_interp_variant<kTrajOnly>(traj, noise, [&](auto T, auto N) {
      ++calls;
      CHECK(Flag<T()>::value == traj);
      CHECK(Flag<N()>::value == noise);
      if (kTrajOnly) CHECK(Flag<T()>::value);
    });
    CHECK(calls == (kTrajOnly && !traj ? 0 : 1));
  }
}

int main() {
  ctl_table<false>();
  ctl_table<true>();
  for (int m = 0; m < 4; ++m) {  // the SR kernels' (traj, jit)
    const bool traj = m & 1, jit = m & 2;
    int calls = 0;
    mtgp::sr_variant(traj, jit, [&](auto T, auto J) {
      ++calls;
      CHECK(Flag<T()>::value == traj);
      CHECK(Flag<J()>::value == jit);
    });
    CHECK(calls == 1);
  }
  for (int b = 0; b < 2; ++b) {  // one flag (ERK, Dopri5), and the value the functor returns
    int calls = 0;
    const int r = mtgp::with_flag(b != 0, [&](auto F) { ++calls; return Flag<F()>::value ? 7 : 3; });
    CHECK(calls == 1 && r == (b ? 7 : 3));
  }
  for (int m = 0; m < 16; ++m) {  // the pack: every position carries its own flag
    const bool a = m & 1, b = m & 2, c = m & 4, d = m & 8;
    int calls = 0;
    mtgp::with_flags([&](auto A, auto B, auto C, auto D) {
      ++calls;
      CHECK(Flag<A()>::value == a && Flag<B()>::value == b && Flag<C()>::value == c && Flag<D()>::value == d);
    }, a, b, c, d);
    CHECK(calls == 1);
  }
  // the integer sets of the launch layer: k_ctl_grad's na (switch 0, 1, 2, default 3), the SR
  // kernels' n_var 1 .. 4 and the environment 0, 1, else 2 -- out of range goes to the last value
  for (int v = -3; v <= 20; ++v) {
    int calls = 0, got = -1;
    mtgp::int_variant<0, 1, 2, 3>(v, [&](auto NA) { ++calls; got = Int<NA()>::value; });
    CHECK(calls == 1 && got == (v == 0 ? 0 : v == 1 ? 1 : v == 2 ? 2 : 3));
    calls = 0;
    mtgp::int_variant<1, 2, 3, 4>(v, [&](auto NV) { ++calls; got = Int<NV()>::value; });
    CHECK(calls == 1 && got == (v == 1 ? 1 : v == 2 ? 2 : v == 3 ? 3 : 4));
    calls = 0;
    const int r = mtgp::int_variant<0, 1, 2>(v, [&](auto E) { ++calls; return 10 * Int<E()>::value; });
    CHECK(calls == 1 && r == (v == 0 ? 0 : v == 1 ? 10 : 20));
  }
  if (g_fail) return 1;
  std::puts("variants ok");
  return 0;
}
"""


def test_truth_tables_under_sanitizers(tmp_path):
    """Every wrapper, every input combination: the functor is called exactly once (never for a
    trajectory-only kernel without `traj`), each constant equals the run-time flag of its name, and
    the integer wrapper sends out-of-range values where the replaced switches' `default:` did."""
    cxx = os.environ.get("CXX", "g++")
    src = tmp_path / "variants_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "variants_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "multitreegp_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "variants ok" in r.stdout, r.stdout + r.stderr
