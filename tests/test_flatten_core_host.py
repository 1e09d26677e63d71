"""The wave flattener's per-row core (multitreegp_amd/csrc/mtgp_flatten_uniform.h) on the CPU.

k_flatten_wave resolves the rows with u_resolve_op, links every non-leaf row to its parent
(u_claim), sums each row's path to the root (u_walk) and writes its word (u_emit_node); a tree with a
row reached twice is walked by one lane (u_serial_walk).  A stand-alone program runs exactly these
functions over plain arrays, one row after the other, and compares the program, its length and its
error with the serial flatten_tree, word for word: seeded random trees, arbitrary arrays (forward
references, rows with two parents, bad opcodes) and the shapes where the closed form could go wrong
(chains, combs, full trees, folded constants, zero-masked slots).  Built with AddressSanitizer and
UBSan, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_MAIN = r"""
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "mtgp_flatten_uniform.h"

using namespace mtgp;

static constexpr int NMAX = 128;
struct Tab {
  uint32_t w[NMAX], len[NMAX];
  float cv[NMAX], val[NMAX];
  int32_t pos[NMAX];
  uint32_t flag[NMAX];
};

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
                    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
  float unit() { return (float)(next() >> 40) / 16777216.0f; }
};

// node library: 0 empty, 1 coefficient, 2.. operators, then n_var variables
static const int kOps[] = {MTGP_FN_ADD, MTGP_FN_SUB, MTGP_FN_MUL, MTGP_FN_DIV, MTGP_FN_SIN, MTGP_FN_COS,
                           MTGP_FN_EXP, MTGP_FN_ABS};
static const int kNOps = 8, kNVar = 5;
static MtgpNodeLibrary make_lib() {
  MtgpNodeLibrary lib;
  std::memset(&lib, 0, sizeof lib);
  lib.fn[0] = MTGP_FN_ZERO; lib.fn[1] = MTGP_FN_ZERO;
  for (int k = 0; k < kNOps; ++k) lib.fn[2 + k] = (int8_t)kOps[k];
  lib.var_start = 2 + kNOps;
  for (int k = 0; k < kNVar; ++k) lib.fn[lib.var_start + k] = MTGP_FN_VAR;
  lib.n_funcs = lib.var_start + kNVar;
  return lib;
}

// the wave flattener, its lanes one after the other; returns n as the kernel stores it
static int wave_flatten(const float* tree, int N, const MtgpNodeLibrary& lib, int n_data, uint64_t zmask, int gap_at,
                        int gap, int L, MtgpInstr* out, bool* was_shared) {
  static Tab S;
  int fnr[NMAX], ja[NMAX], jb[NMAX];
  const int cap = L - 1;
  for (int i = 0; i < NMAX; ++i) { S.val[i] = i < N ? tree[4 * i + 3] : 0.0f; S.flag[i] = 0; S.pos[i] = 0; }
  for (int i = 0; i < N; ++i) {  // round 0
    fnr[i] = -1; ja[i] = jb[i] = -1;
    uint32_t kind = K_CONST, slot = 0, isc = 1;
    float cv = 0.0f;
    bool done = true;
    const float fx = tree[4 * i];
    if (fx == 1.0f) cv = tree[4 * i + 3];
    else {
      int32_t f = f2i_sat(fx);
      f = f < 0 ? 0 : (f > lib.n_funcs - 1 ? lib.n_funcs - 1 : f);
      const int fn = lib.fn[f];
      if (fn == MTGP_FN_VAR) {
        int sl = f - lib.var_start;
        if (sl > n_data - 1) sl = n_data - 1;
        slot = (uint32_t)(sl >= gap_at ? sl + gap : sl);
        if (!((zmask >> sl) & 1ull)) { kind = K_VAR; isc = 0; }
      } else if (fn_arity(fn) > 0) {
        fnr[i] = fn;
        ja[i] = norm_index(tree[4 * i + 1], N);
        if (fn_arity(fn) == 2) jb[i] = norm_index(tree[4 * i + 2], N);
        done = false;
      }
    }
    if (done) { S.w[i] = u_pack(kind, MTGP_FN_ZERO, slot, isc, 1, 0); S.len[i] = 1u | 1u << 16; S.cv[i] = cv; }
  }
  for (int i = 0; i < N; ++i)  // the rounds: a row after its operand rows
    if (fnr[i] >= 0) u_resolve_op(S, i, fnr[i], ja[i], jb[i]);
  const uint32_t wr = S.w[N - 1], lr = S.len[N - 1];
  int n;
  if ((int)u_need(wr) > MTGP_STACK_MAX) n = -MTGP_ERR_STACK;
  else if ((int)(lr & 0xffffu) > cap) n = -MTGP_ERR_PROG_TOO_LONG;
  else n = (int)(lr >> 16);
  auto emit = [&](int at, const MtgpInstr& v) {
    if (at < 0 || at >= L) { std::printf("emit out of range: %d of %d\n", at, L); std::exit(2); }
    out[at] = v;
  };
  *was_shared = false;
  if (n > 0 && u_leaf(wr)) {
    ULeaf x; x.isc = u_isc(wr); x.v = S.cv[N - 1]; x.slot = u_slot(wr);
    out[0] = u_load(x, false);
  } else if (n > 0) {
    for (int i = 0; i < NMAX; ++i) { S.flag[i] = 0; S.pos[i] = (int32_t)kULinkNone; }
    for (int i = 0; i < N; ++i)
      if (fnr[i] >= 0 && !u_isc(S.w[i])) u_claim(S, i, ja[i], jb[i], [&](int c) { ++S.flag[c]; });
    bool shared = false;
    for (int i = 0; i < NMAX; ++i) shared = shared || S.flag[i] > 1u;
    *was_shared = shared;
    if (!shared) {
      for (int i = 0; i < N; ++i) {
        if (!(fnr[i] >= 0 && !u_isc(S.w[i]))) continue;
        const int pp = u_walk(S, i, N - 1);
        if (pp >= 0) u_emit_node(S, i, ja[i], jb[i], pp & 0xffff, (pp >> 16) != 0, emit, [](int, int, bool) {});
      }
    } else {
      const bool ok = u_serial_walk(S, N - 1, cap, N, emit, [&](int i, int& ca, int& cb) {
        ca = norm_index(tree[4 * i + 1], N);
        cb = norm_index(tree[4 * i + 2], N);
      });
      if (!ok) n = -MTGP_ERR_PROG_TOO_LONG;
    }
  }
  MtgpInstr e; e.op = (uint32_t)MTGP_OP_END << MTGP_OP_SHIFT; e.imm = 0.0f;
  out[n > 0 ? n : 0] = e;
  return n;
}

static int g_fail = 0, g_cases = 0, g_shared = 0, g_err = 0;

static void check(const char* what, const std::vector<float>& tree, int N, const MtgpNodeLibrary& lib, int n_data,
                  uint64_t zmask, int gap_at, int gap, int L) {
  std::vector<MtgpInstr> a(L), b(L);
  std::vector<RowInfo> info(MTGP_MAX_NODES);
  const int nr = flatten_tree(tree.data(), N, &lib, n_data, zmask, a.data(), L, info.data(), nullptr, gap_at, gap);
  bool shared = false;
  const int nw = wave_flatten(tree.data(), N, lib, n_data, zmask, gap_at, gap, L, b.data(), &shared);
  ++g_cases; g_shared += shared; g_err += nr <= 0;
  bool same = nr == nw;
  for (int k = 0; same && k <= (nr > 0 ? nr : 0); ++k) same = std::memcmp(&a[k], &b[k], sizeof(MtgpInstr)) == 0;
  if (!same) {
    if (++g_fail <= 10) std::printf("%s: N %d zmask %llx L %d: serial %d, wave %d (shared %d)\n", what, N,
                                    (unsigned long long)zmask, L, nr, nw, (int)shared);
  }
}

struct Build {  // a tree written from the top row down, as the reference lays it out
  std::vector<float> t;
  int N, next;
  explicit Build(int n) : t(4 * n, 0.0f), N(n), next(n - 1) {}
  int row() { return next--; }
  void leaf(int i, Rng& r, int var_only = -1) {
    if (var_only >= 0 || r.below(2)) t[4 * i] = (float)(2 + kNOps + (var_only >= 0 ? var_only : r.below(kNVar)));
    else { t[4 * i] = 1.0f; t[4 * i + 3] = r.unit() * 4 - 2; }
  }
  void op(int i, int k, int a, int b) { t[4 * i] = (float)(2 + k); t[4 * i + 1] = (float)a; t[4 * i + 2] = (float)b; }
};

// random tree of at most `budget` rows below row i
static void grow(Build& b, int i, int depth, Rng& r, int p_leaf) {
  if (depth == 0 || b.next < 2 || r.below(100) < p_leaf) { b.leaf(i, r); return; }
  const int k = r.below(kNOps);
  const int ar = fn_arity(kOps[k]);
  const int a = b.row(), c = ar == 2 ? b.row() : 0;
  b.op(i, k, a, c);
  grow(b, a, depth - 1, r, p_leaf);
  if (ar == 2) grow(b, c, depth - 1, r, p_leaf);
}

int main() {
  const MtgpNodeLibrary lib = make_lib();
  Rng r{12345};
  const uint64_t masks[] = {0ull, 0x3ull, 0x15ull, 0x1full};
  auto all_masks = [&](const char* what, const Build& b, int L) {
    for (uint64_t m : masks) check(what, b.t, b.N, lib, kNVar, m, 3, 2, L);
  };
  for (int N : {1, 2, 7, 33, 64, 128}) {
    const int L = (2 * N + 8 + 3) / 4 * 4;
    { Build b(N); all_masks("empty", b, L); }
    { Build b(N); b.leaf(b.row(), r); all_masks("leaf", b, L); }
    { Build b(N); b.leaf(b.row(), r, 1); all_masks("var leaf", b, L); }
    for (int k : {4, 6}) {  // unary chain over every row (sin fuses with its leaf, exp does not)
      Build b(N);
      for (int i = N - 1; i > 0; --i) b.op(i, k, i - 1, 0);
      b.leaf(0, r, 2);
      all_masks("chain", b, L);
    }
    for (int side = 0; side < 2; ++side) {  // left and right combs
      Build b(N);
      int i = b.row();
      while (b.next >= 2) {
        const int lf = b.row(), nx = b.row();
        b.op(i, 1 + side, side ? lf : nx, side ? nx : lf);
        b.leaf(lf, r);
        i = nx;
      }
      b.leaf(i, r, 0);
      all_masks("comb", b, L);
    }
    for (int d = 1; d <= 7; ++d) {  // full binary trees (stack need grows with the depth: errors at 8+)
      if ((1 << d) - 1 > N) break;
      Build b(N);
      grow(b, b.row(), d - 1, r, 0);
      all_masks("full", b, L);
    }
  }
  for (int it = 0; it < 4000; ++it) {  // random trees, some with constant subtrees
    const int N = 1 + r.below(it % 4 == 0 ? 128 : 64);
    Build b(N);
    grow(b, b.row(), 1 + r.below(10), r, 10 + r.below(40));
    check("random", b.t, N, lib, kNVar, masks[r.below(4)], r.below(kNVar + 1), r.below(3), (2 * N + 8 + 3) / 4 * 4);
  }
  for (int it = 0; it < 4000; ++it) {  // arbitrary arrays: forward references, shared rows, bad opcodes
    const int N = 1 + r.below(40);
    std::vector<float> t(4 * N);
    for (int i = 0; i < N; ++i) {
      t[4 * i] = (float)(r.below(lib.n_funcs + 5) - 2) + (r.below(10) == 0 ? 0.5f : 0.0f);
      t[4 * i + 1] = (float)(r.below(2 * N + 6) - N - 3);
      t[4 * i + 2] = (float)(r.below(2 * N + 6) - N - 3);
      t[4 * i + 3] = r.unit() * 6 - 3;
    }
    const int L = it % 3 == 0 ? 16 : (it % 3 == 1 ? (2 * N + 8 + 3) / 4 * 4 : 400);
    check("arbitrary", t, N, lib, kNVar, masks[r.below(4)], 0, 0, L);
  }
  for (int it = 0; it < 2000; ++it) {  // DAGs of operators only: many shared rows, long expansions
    const int N = 2 + r.below(24);
    std::vector<float> t(4 * N);
    for (int i = 0; i < N; ++i) {
      if (i < 2) { t[4 * i] = (float)(2 + kNOps + r.below(kNVar)); continue; }
      t[4 * i] = (float)(2 + r.below(kNOps));
      const int near = it % 4 == 0 ? i : (i < 3 ? i : 3);  // operands among the last rows: deep expansions
      t[4 * i + 1] = (float)(i - 1 - r.below(near));
      t[4 * i + 2] = (float)(i - 1 - r.below(near));
    }
    check("dag", t, N, lib, kNVar, 0ull, 0, 0, it % 3 == 0 ? 64 : (it % 3 == 1 ? 600 : 4000));
  }
  std::printf("%d cases, %d with a shared row, %d errors, %d differ\n", g_cases, g_shared, g_err, g_fail);
  if (g_fail || g_shared < 100 || g_err < 10) return 1;
  std::puts("flatten core ok");
  return 0;
}
"""


def test_wave_core_matches_serial_flattener_under_sanitizers(tmp_path):
    """Closed-form positions, path sums and the one-lane walk for shared rows give flatten_tree's
    program, length and error for every tree; the run must see shared rows and errors at all."""
    cxx = os.environ.get("CXX", "g++")
    src = tmp_path / "flatten_core_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "flatten_core_main"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "multitreegp_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "flatten core ok" in r.stdout, r.stdout + r.stderr
