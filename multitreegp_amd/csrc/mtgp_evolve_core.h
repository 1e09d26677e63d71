// mtgp_evolve_core.h -- the evolution step (the reference's genetic_operators/, gp.py:475-525):
// the one C++ implementation, allocation-free with bounded buffers, compiled for the host and the
// device (MTGP_HD).  The host library (csrc/mtgp_evolve.cpp, libmtgp_host.so) and the k_evo_*
// kernels (csrc/mtgp_evolve.hip) are drivers around it, so a generation is the same draw for draw
// wherever it runs.  Same operators, probabilities and array contract as the numpy restatement
// (multitreegp_amd/genetic_operators.py, the tested spec): a tree is float32 [N, 4] rows
// [f, a, b, value], empty rows packed low, root at row N-1, descending rows in preorder,
// a = k-1, b = k-1-|subtree(a)|.  Edits are done on the preorder node list and written back.
// tests/test_host_evolve.py and tests/golden/evolve_parity.json pin the output bit for bit.
//
// Random numbers: xoshiro256** streams, one per (population, pair) or sampled candidate, derived
// from the seed.  Runs are distributed like the reference's (JAX threefry keys split per
// operation), not draw for draw.
//
// References: initialization.py:9-164 (sample_tree), mutation.py:9-579, crossover.py:8-218,
// reproduction.py:8-176, genetic_programming.py:475-525.
//
// Execution model.  A "group" of lanes (one wave on the device, one lane on the host) handles one
// (population, pair) or one sampled candidate.  Every lane runs the pair's xoshiro256** stream and
// every decision redundantly, so control flow is uniform over the group and needs no cross-lane
// traffic; the per-group workspace (Ws: LDS on the device) is written with the same values by all
// lanes.  Only the row loops (tree loads, copies, splice_rows, from_preorder's row writes) are
// split over the lanes, 16 B per lane.
//
// Floating point: compiled with -ffp-contract=off; f64 divide and sqrt are IEEE on both sides;
// pow(0.7, d) comes from a table the host fills (Cfg::pow07, read through Ctx::pw); log() inside Rng::normal is the one
// libm call left, so a coefficient may differ by 1 float32 ulp between host and device.
//
// Safety: every index derived from tree contents (a/b columns, f values, scanned sizes) is clamped
// before use and every loop over contents is bounded by N, so a population that violates the
// layout gives an unspecified result but never an access outside the buffers.
#ifndef MTGP_EVOLVE_CORE_H
#define MTGP_EVOLVE_CORE_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

#include "mtgp_f32math.h"
#include "mtgp_host.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define MTGP_EVO_SYNC() __syncthreads()
#else
#define MTGP_EVO_SYNC() ((void)0)
#endif

namespace mtgp_evo {

constexpr int kMaxNodes = 256;      // MTGP_MAX_NODES
constexpr int kMaxTournament = 64;  // tournament_size bound (Ws::tour)
constexpr int kMaxRetries = 1000;
constexpr int kMaxDepth = 30;
constexpr int kStack = 40;  // sample_tree's traversal stack (depth of a heap index < 2^31)
constexpr int kPre = 8;     // nodes a mutation puts in front of / around an old subtree
constexpr int kMaxFuncs = 128;  // MTGP_MAX_FUNCS (the evaluator's bound on the node library)

MTGP_HD inline int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
// (int)f as x86's cvttss2si gives it (out of range and NaN: INT32_MIN), without the undefined cast
MTGP_HD inline int f2i(float f) { return (f >= -2147483648.0f && f < 2147483648.0f) ? (int)f : INT32_MIN; }

// ---------------------------------------------------------------- random numbers
struct Rng {
  uint64_t s[4];
  MTGP_HD static uint64_t splitmix(uint64_t& x) {
    uint64_t z = (x += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
  MTGP_HD Rng(uint64_t seed, uint64_t a, uint64_t b) {
    uint64_t x = seed ^ (a * 0xd1342543de82ef95ull) ^ (b * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull);
    for (int i = 0; i < 4; ++i) s[i] = splitmix(x);
  }
  MTGP_HD static uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
  MTGP_HD uint64_t next() {
    const uint64_t r = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl(s[3], 45);
    return r;
  }
  MTGP_HD double uniform() { return (double)(next() >> 11) * 0x1.0p-53; }
  MTGP_HD int integer(int n) { return (int)((next() >> 32) * (uint64_t)n >> 32); }  // [0, n)
  // Marsaglia polar in two halves: the draws (all the stream sees), and the value -- log, divide
  // and sqrt -- which the callers form only where the coefficient is kept
  struct NormalDraw {
    double u, q;
  };
  MTGP_HD NormalDraw normal_draw() {
    for (;;) {
      const double u = 2.0 * uniform() - 1.0, v = 2.0 * uniform() - 1.0, q = u * u + v * v;
      if (q > 0.0 && q < 1.0) {
        NormalDraw d;
        d.u = u, d.q = q;
        return d;
      }
    }
  }
  MTGP_HD static double normal_value(NormalDraw d) { return d.u * ::sqrt(-2.0 * ::log(d.q) / d.q); }
  MTGP_HD double normal() { return normal_value(normal_draw()); }
  // index drawn with weights w[0..n) (not all zero); W is double or float (widened exactly)
  template <class W>
  MTGP_HD int choice(const W* w, int n) {
    double tot = 0.0;
    for (int i = 0; i < n; ++i) tot += (double)w[i];
    double u = uniform() * tot;
    int last = 0;
    for (int i = 0; i < n; ++i) {
      const double wi = (double)w[i];
      if (wi <= 0.0) continue;
      last = i;
      if (u < wi) return i;
      u -= wi;
    }
    return last;
  }
};

struct Node {
  int32_t f;
  float v;
};

// ------------------------------------------------------------------ configuration
// The small tables live in one blob (host memory for the twin, device memory for the kernels);
// Cfg holds views into it plus the per-generation scalars and travels by value.
struct Cfg {
  const double* op_prob;   // [n_ops]
  const double* tp;        // [num_pop, tournament_size]
  const double* rtp;       // [num_pop, 3]
  const double* rp;        // [num_pop]
  const int32_t* op_index; // [n_ops]
  const float* var_mask;   // [T, n_vars]
  const uint8_t* kind;     // [n_funcs]: operand count (bits 0-1) | 4 when the index is an operator
  const int32_t* var_cnt;  // [T]: allowed variables of a tree whose mask is all 0 / 1, else -1
  const int32_t* var_list; // [T, n_vars]: their indices (into the mask), ascending
  int32_t n_funcs, n_ops, var_start, n_vars, depth, tournament_size, elite_size, migration_size, migrate;
  int32_t num_pop, pop_size, T, N;
  float sd;
  uint64_t seed;
  double pow07[kMaxDepth + 1];  // std::pow(0.7, d), filled by the host

  MTGP_HD int arity(int f) const { return (f >= 0 && f < n_funcs) ? (kind[f] & 3) : 0; }
  MTGP_HD bool is_op(float f) const {
    if (!(f >= 0.0f && f < (float)n_funcs)) return false;
    const int k = (int)f;
    return (float)k == f && (kind[k] & 4);
  }
  MTGP_HD bool is_var(float f) const { return f >= (float)var_start && f < (float)(var_start + n_vars); }
  MTGP_HD bool is_leaf(float f) const { return f == 1.0f || is_var(f); }
};

struct BlobLayout {
  size_t op_prob, tp, rtp, rp, op_index, var_mask, var_cnt, var_list, kind, bytes;
};
inline BlobLayout blob_layout(int n_funcs, int n_ops, int n_vars, int T, int num_pop, int tournament_size) {
  BlobLayout b;
  size_t o = 0;
  b.op_prob = o, o += sizeof(double) * (size_t)n_ops;
  b.tp = o, o += sizeof(double) * (size_t)num_pop * tournament_size;
  b.rtp = o, o += sizeof(double) * (size_t)num_pop * 3;
  b.rp = o, o += sizeof(double) * (size_t)num_pop;
  b.op_index = o, o += sizeof(int32_t) * (size_t)n_ops;
  b.var_mask = o, o += sizeof(float) * (size_t)T * n_vars;
  b.var_cnt = o, o += sizeof(int32_t) * (size_t)T;
  b.var_list = o, o += sizeof(int32_t) * (size_t)T * n_vars;
  b.kind = o, o += (size_t)n_funcs;
  b.bytes = (o + 15) & ~(size_t)15;
  return b;
}
inline void bind_blob(Cfg& c, const BlobLayout& b, const void* base) {
  const char* p = (const char*)base;
  c.op_prob = (const double*)(p + b.op_prob);
  c.tp = (const double*)(p + b.tp);
  c.rtp = (const double*)(p + b.rtp);
  c.rp = (const double*)(p + b.rp);
  c.op_index = (const int32_t*)(p + b.op_index);
  c.var_mask = (const float*)(p + b.var_mask);
  c.var_cnt = (const int32_t*)(p + b.var_cnt);
  c.var_list = (const int32_t*)(p + b.var_list);
  c.kind = (const uint8_t*)(p + b.kind);
}

// ---------------------------------------------------------------------- workspace
struct Lanes {
  int lane, n;
};

struct Ws {  // per group; carved from one 16-B aligned block of ws_bytes(N)
  float* t1;     // [4N] rows of the first parent's tree (16-B aligned)
  float* t2;     // [4N]
  int32_t* c1;   // [N + 1] crossover weight prefix sums
  int32_t* c2;
  int32_t* z1;   // [N] subtree sizes (crossover: of t1's rows; lists: of the preorder nodes)
  int32_t* z2;   // [N] (crossover: of t2's rows; lists: the size stack)
  Node* n;       // [N] preorder list of a tree
  Node* m;       // [N] the edited list
  int32_t* sf;   // [2N - 1] sample_tree: heap-ordered f
  float* sc;     // [2N - 1] and coefficient
  int32_t* tour; // [kMaxTournament]
  int32_t* stk;  // [kStack]
  Node* pre;     // [kPre]
  uint8_t* kind; // [kMaxFuncs] the device's copy of Cfg::kind (the serial loops look it up per row)
};
MTGP_HD inline size_t ws_bytes(int N) {
  const size_t n = (size_t)N;
  return 32 * n + 8 * (n + 1) + 8 * n + 16 * n + 8 * (2 * n - 1) + 4 * (size_t)kMaxTournament + 4 * (size_t)kStack +
         8 * (size_t)kPre + (size_t)kMaxFuncs + 16;
}
MTGP_HD inline Ws ws_carve(void* base, int N) {
  char* p = (char*)base;
  Ws w;
  w.t1 = (float*)p, p += 16 * (size_t)N;
  w.t2 = (float*)p, p += 16 * (size_t)N;
  w.n = (Node*)p, p += 8 * (size_t)N;
  w.m = (Node*)p, p += 8 * (size_t)N;
  w.pre = (Node*)p, p += 8 * (size_t)kPre;
  w.c1 = (int32_t*)p, p += 4 * (size_t)(N + 1);
  w.c2 = (int32_t*)p, p += 4 * (size_t)(N + 1);
  w.z1 = (int32_t*)p, p += 4 * (size_t)N;
  w.z2 = (int32_t*)p, p += 4 * (size_t)N;
  w.sf = (int32_t*)p, p += 4 * (size_t)(2 * N - 1);
  w.sc = (float*)p, p += 4 * (size_t)(2 * N - 1);
  w.tour = (int32_t*)p, p += 4 * (size_t)kMaxTournament;
  w.stk = (int32_t*)p, p += 4 * (size_t)kStack;
  w.kind = (uint8_t*)p;
  return w;
}

struct Ctx {
  const Cfg& C;
  Ws W;
  Lanes L;
  const double* pw;  // Cfg::pow07 of the call's own configuration (not of a copy)
};

// ------------------------------------------------------------------------ row I/O
MTGP_HD inline void put_row(float* o, int k, float f, float a, float b, float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<float4*>(o + 4 * (size_t)k) = make_float4(f, a, b, v);
#else
  const float r[4] = {f, a, b, v};
  memcpy(o + 4 * (size_t)k, r, sizeof r);
#endif
}
MTGP_HD inline void copy_row(float* dst, const float* src, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<float4*>(dst + 4 * (size_t)k) = *reinterpret_cast<const float4*>(src + 4 * (size_t)k);
#else
  memcpy(dst + 4 * (size_t)k, src + 4 * (size_t)k, 4 * sizeof(float));
#endif
}
// rows [0, rows) split over the lanes; the barrier orders the copy against the group's later use
MTGP_HD inline void copy_rows(float* dst, const float* src, int rows, Lanes L) {
  for (int k = L.lane; k < rows; k += L.n) copy_row(dst, src, k);
  MTGP_EVO_SYNC();
}

// ---------------------------------------------------------------- fitness ordering
// Total order for any bits: NaN last, +-0 tie, the index breaks ties.  For NaN-free input the
// ranks are those of a stable sort by F[a] < F[b] (and by -F[a] < -F[b] for the descending order),
// the reference's argsort.  The kernel counts ranks (order_ranks); the host driver sorts.
MTGP_HD inline bool fit_less(float a, float b) { return a < b || (a == a && b != b); }
MTGP_HD inline bool fit_greater(float a, float b) { return a > b || (a == a && b != b); }
MTGP_HD inline bool fit_same(float a, float b) { return a == b || (a != a && b != b); }
// rank = #smaller + #equal with lower index; asc[rank_asc] = i, desc[rank_desc] = i
MTGP_HD inline void order_ranks(const float* F, int S, int i, int* rank_asc, int* rank_desc) {
  const float x = F[i];
  int ra = 0, rd = 0;
  for (int j = 0; j < S; ++j) {
    const float y = F[j];
    const int tie = fit_same(y, x) && j < i;
    ra += fit_less(y, x) || tie;
    rd += fit_greater(y, x) || tie;
  }
  *rank_asc = ra;
  *rank_desc = rd;
}

// -------------------------------------------------------------- layout helpers
MTGP_HD inline int find_end_idx(const float* t, int idx) {  // mutation.py:9-26
  int open = 1, k = idx;
  while (open > 0 && k >= 0) {
    open -= 1;
    open += (t[4 * k + 1] >= 0.0f) + (t[4 * k + 2] >= 0.0f);
    --k;
  }
  return k;
}

MTGP_HD inline int to_preorder(const float* t, int N, Node* out) {
  int n = 0;
  for (int k = N - 1; k >= 0; --k) {
    const int f = f2i(t[4 * k]);
    if (f == 0) break;
    out[n].f = f;
    out[n].v = t[4 * k + 3];
    ++n;
  }
  return n;
}

// sz[i] of a preorder list (st: the size stack, as long as the list)
MTGP_HD inline void subtree_sizes(const Cfg& C, const Node* n, int cnt, int32_t* sz, int32_t* st) {
  int sp = 0;
  for (int i = cnt - 1; i >= 0; --i) {
    int s = 1;
    const int ar = C.arity(n[i].f);
    for (int a = 0; a < ar && sp > 0; ++a) s += st[--sp];
    s = s > C.N ? C.N : s;
    sz[i] = s;
    st[sp++] = s;
  }
}

// preorder -> [N, 4] rows; false when the tree does not fit (nothing is written)
MTGP_HD inline bool from_preorder(const Ctx& X, const Node* m, int cnt, float* out) {
  const int N = X.C.N;
  if (cnt > N || cnt <= 0) return false;
  subtree_sizes(X.C, m, cnt, X.W.z1, X.W.z2);
  for (int k = X.L.lane; k < N; k += X.L.n) {
    const int i = N - 1 - k;
    if (i < cnt) {
      const int f = m[i].f, ar = X.C.arity(f);
      const int bs = X.W.z1[clampi(i + 1, 0, cnt - 1)];
      put_row(out, k, (float)f, ar >= 1 ? (float)(k - 1) : -1.0f, ar == 2 ? (float)(k - 1 - bs) : -1.0f,
              f == 1 ? m[i].v : 0.0f);
    } else {
      put_row(out, k, 0.0f, -1.0f, -1.0f, 0.0f);
    }
  }
  MTGP_EVO_SYNC();
  return true;
}

// ---------------------------------------------------------------- sampling
// Rng::choice over tree tr's variable mask.  For a 0 / 1 mask the weights sum to their count and
// the running subtraction steps by exactly 1.0, so the draw stops at the floor(u)-th allowed
// variable (the last one, should u round up to the count): the same index without the two passes.
MTGP_HD inline int choose_var(const Cfg& C, Rng& g, int tr) {
  const int cnt = C.var_cnt[tr];
  if (cnt > 0) {
    const int j = (int)(g.uniform() * (double)cnt);
    return C.var_list[(size_t)tr * C.n_vars + (j > cnt - 1 ? cnt - 1 : j)];
  }
  return g.choice(C.var_mask + (size_t)tr * C.n_vars, C.n_vars);
}

// initialization.py:9-124 for one tree: breadth-first draws, operators only while
// open_slots < N - i - 1 and depth + 1 < depth_limit, leaf = coefficient w.p. 0.5 else an allowed
// variable.  The preorder list (descending depth-first rows) goes to out[0, cap), the node count
// is returned (counted past cap, never written past it)
MTGP_HD inline int sample_tree(const Ctx& X, Rng& g, int depth_limit, int tr, Node* out, int cap) {
  const Cfg& C = X.C;
  const int N = C.N, tree_size = (int)((1u << C.depth) - 1u), I = tree_size < 2 * N - 1 ? tree_size : 2 * N - 1;
  int32_t* f = X.W.sf;
  float* coef = X.W.sc;
  int open = 1, cnt = 0;
  for (int i = 0; i < I && open > 0; ++i) {
    const int d = 31 - __builtin_clz((unsigned)(i + 1));
    const Rng::NormalDraw nd = g.normal_draw();
    const int leaf = g.uniform() < 0.5 ? 1 : C.var_start + choose_var(C, g, tr);
    int index = leaf;
    if (open < N - i - 1 && d + 1 < depth_limit && g.uniform() < X.pw[d])
      index = C.op_index[g.choice(C.op_prob, C.n_ops)];
    if (i > 0) {
      const int pf = f[(i + (i % 2) - 2) / 2];
      if (!(C.arity(pf) + i % 2 > 1)) index = 0;
    }
    f[i] = index;
    coef[i] = index == 1 ? (float)(Rng::normal_value(nd) * C.sd) : 0.0f;
    if (index != 0) {
      open = open + C.arity(index) - 1;
      open = open < 0 ? 0 : open;
    }
    cnt = i + 1;
  }
  int n = 0, sp = 0;
  int32_t* stk = X.W.stk;
  stk[sp++] = 0;
  while (sp > 0) {  // preorder = first operand first
    const int i = stk[--sp];
    if (i >= cnt || f[i] == 0) continue;
    if (n < cap) {
      out[n].f = f[i];
      out[n].v = coef[i];
    }
    ++n;
    const int ar = C.arity(f[i]);
    if (ar >= 2 && sp < kStack) stk[sp++] = 2 * i + 2;
    if (ar >= 1 && sp < kStack) stk[sp++] = 2 * i + 1;
  }
  return n;
}

MTGP_HD inline Node new_leaf(const Ctx& X, Rng& g, int tr) {  // mutation.py:60, 188
  const Rng::NormalDraw nd = g.normal_draw();
  Node r;
  if (g.uniform() < 0.5) {
    r.f = 1, r.v = (float)(Rng::normal_value(nd) * X.C.sd);
    return r;
  }
  r.f = X.C.var_start + choose_var(X.C, g, tr), r.v = 0.0f;
  return r;
}
MTGP_HD inline int new_operator(const Ctx& X, Rng& g) { return X.C.op_index[g.choice(X.C.op_prob, X.C.n_ops)]; }

// The empty-row count (f == 0) and the lowest row of the preorder (one above the highest row whose
// f truncates to 0, where to_preorder stops) -- the one pass over all N rows, done by the lanes
// together.  In a valid tree rows [0, lo) are exactly the empty rows, so
// the serial loops below start at lo: empty rows weigh nothing in any choice.
struct RowInfo {
  int e, lo;
};
MTGP_HD inline RowInfo rows_info(const float* t, int N, Lanes L) {
  RowInfo r;
  r.e = 0, r.lo = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  for (int base = 0; base < N; base += 64) {  // one wave (Lanes{lane, 64}); the ballots are wave-uniform
    const int k = base + L.lane;
    const float f = k < N ? t[4 * k] : 1.0f;
    const unsigned long long bz = __ballot(f == 0.0f), bi = __ballot(f2i(f) == 0);
    r.e += __popcll(bz);
    if (bi) r.lo = base + 64 - __clzll(bi);
  }
#else
  (void)L;
  for (int k = 0; k < N; ++k) {
    r.e += t[4 * k] == 0.0f;
    r.lo = f2i(t[4 * k]) == 0 ? k + 1 : r.lo;
  }
#endif
  return r;
}

// ------------------------------------------------------------------ mutation
enum RowKind { kLeafRows = 0, kOpRows = 1, kOpRowsNoRoot = 2 };
MTGP_HD inline bool row_weight(const Cfg& C, const float* t, int k, int kind) {
  if (kind == kLeafRows) return C.is_leaf(t[4 * k]);
  if (kind == kOpRowsNoRoot && k == C.N - 1) return false;
  return C.is_op(t[4 * k]);
}
MTGP_HD inline int count_rows(const Cfg& C, const float* t, int kind, int lo) {
  int n = 0;
  for (int k = lo; k < C.N; ++k) n += row_weight(C, t, k, kind);
  return n;
}
// Rng::choice over the 0/1 row weights: tot is their count, u steps down by exactly 1.0
MTGP_HD inline int choose_row(const Cfg& C, Rng& g, const float* t, int kind, int count, int lo) {
  double u = g.uniform() * (double)count;
  int last = 0;
  for (int k = lo; k < C.N; ++k) {
    if (!row_weight(C, t, k, kind)) continue;
    last = k;
    if (u < 1.0) return k;
    u -= 1.0;
  }
  return last;
}

// The tree with the subtree at `row` (whole: the whole tree) replaced by pre[0, npre) with the old
// subtree inserted before pre[old_at] (old_at < 0: dropped, old_at == npre: appended); false when
// the result does not fit (nothing is written)
MTGP_HD inline bool rebuild(const Ctx& X, const float* t, int row, int npre, int old_at, bool whole, float* out) {
  const int N = X.C.N;
  Node* n = X.W.n;
  Node* m = X.W.m;
  const Node* pre = X.W.pre;
  const int len0 = to_preorder(t, N, n);
  if (len0 == 0) return false;
  int p = 0, size = len0;
  if (!whole) {
    p = clampi(N - 1 - row, 0, len0 - 1);
    subtree_sizes(X.C, n, len0, X.W.z1, X.W.z2);
    size = clampi(X.W.z1[p], 1, len0 - p);
  }
  int len = 0;
  for (int j = 0; j < p; ++j, ++len)
    if (len < N) m[len] = n[j];
  for (int j = 0; j <= npre; ++j) {
    if (j == old_at)
      for (int q = 0; q < size; ++q, ++len)
        if (len < N) m[len] = n[p + q];
    if (j < npre) {
      if (len < N) m[len] = pre[j];
      ++len;
    }
  }
  for (int j = p + size; j < len0; ++j, ++len)
    if (len < N) m[len] = n[j];
  return from_preorder(X, m, len, out);
}

// t with row `row` given a new f (and, set_v, value)
MTGP_HD inline void copy_patched(const Ctx& X, const float* t, float* out, int row, float f, bool set_v, float v) {
  for (int k = X.L.lane; k < X.C.N; k += X.L.n) {
    if (k == row) put_row(out, k, f, t[4 * k + 1], t[4 * k + 2], set_v ? v : t[4 * k + 3]);
    else copy_row(out, t, k);
  }
  MTGP_EVO_SYNC();
}

MTGP_HD inline int op_and_subtree(const Ctx& X, Rng& g, int tr, bool* second) {
  // draws of prepend_operator / insert_operator: operator, a depth-2 subtree, the side
  Node* pre = X.W.pre;
  const int op = new_operator(X, g);
  pre[0].f = op, pre[0].v = 0.0f;
  const int ns = clampi(sample_tree(X, g, 2, tr, pre + 1, kPre - 1), 0, kPre - 1);
  *second = g.uniform() < 0.5;
  return ns;
}

// the seven mutations (mutation.py:127-503); t is the parent's tree in the workspace (W.t1)
MTGP_HD inline bool mutate_tree_op(const Ctx& X, int which, const float* t, RowInfo ri, Rng& g, int tr,
                                   float* out) {
  const Cfg& C = X.C;
  const int N = C.N;
  Node* pre = X.W.pre;
  switch (which) {
    case 0: {  // add_subtree
      const int cnt = count_rows(C, t, kLeafRows, ri.lo);
      if (cnt == 0) return false;
      const int row = choose_row(C, g, t, kLeafRows, cnt, ri.lo);
      const int ns = clampi(sample_tree(X, g, 2, tr, pre, kPre), 0, kPre);
      return rebuild(X, t, row, ns, -1, false, out);
    }
    case 1: {  // mutate_leaf
      const int cnt = count_rows(C, t, kLeafRows, ri.lo);
      if (cnt == 0) return false;
      for (int it = 0; it < kMaxRetries; ++it) {
        const int row = choose_row(C, g, t, kLeafRows, cnt, ri.lo);
        const Node nl = new_leaf(X, g, tr);
        if (!(t[4 * row] == (float)nl.f && nl.f != 1)) {
          copy_patched(X, t, out, row, (float)nl.f, true, nl.f == 1 ? nl.v : 0.0f);
          return true;
        }
      }
      return false;
    }
    case 2: {  // mutate_operator
      const int cnt = count_rows(C, t, kOpRows, ri.lo);
      if (cnt == 0) return false;
      const int empty = ri.e;
      int row = -1, op = 0;
      for (int it = 0; it < kMaxRetries; ++it) {
        const int r = choose_row(C, g, t, kOpRows, cnt, ri.lo);
        const int o = new_operator(X, g);
        const int size = r - find_end_idx(t, r);
        const int need = C.arity(o) == 2 ? 7 : 8;
        if (!(t[4 * r] == (float)o || empty + size < need)) {
          row = r;
          op = o;
          break;
        }
      }
      if (row < 0) return false;
      const int cur = C.arity(f2i(t[4 * row])), nw = C.arity(op);
      if (cur == nw) {
        copy_patched(X, t, out, row, (float)op, false, 0.0f);
        return true;
      }
      pre[0].f = op, pre[0].v = 0.0f;
      int ns = 1;
      if (nw == 1) {
        ns += clampi(sample_tree(X, g, 2, tr, pre + ns, kPre - ns), 0, kPre - ns);
      } else {
        ns += clampi(sample_tree(X, g, 1, tr, pre + ns, kPre - ns), 0, kPre - ns);
        ns += clampi(sample_tree(X, g, 1, tr, pre + ns, kPre - ns), 0, kPre - ns);
      }
      return rebuild(X, t, row, ns, -1, false, out);
    }
    case 3: {  // delete_operator
      const int cnt = count_rows(C, t, kOpRowsNoRoot, ri.lo);
      if (cnt == 0) return false;
      const int row = choose_row(C, g, t, kOpRowsNoRoot, cnt, ri.lo);
      pre[0] = new_leaf(X, g, tr);
      return rebuild(X, t, row, 1, -1, false, out);
    }
    case 4: {  // prepend_operator
      bool second;
      const int ns = op_and_subtree(X, g, tr, &second);
      if (C.arity(pre[0].f) == 2) return rebuild(X, t, N - 1, 1 + ns, second ? 1 + ns : 1, true, out);
      return rebuild(X, t, N - 1, 1, 1, true, out);
    }
    case 5: {  // insert_operator
      const int cnt = count_rows(C, t, kOpRowsNoRoot, ri.lo);
      if (cnt == 0) return false;
      const int row = choose_row(C, g, t, kOpRowsNoRoot, cnt, ri.lo);
      bool second;
      const int ns = op_and_subtree(X, g, tr, &second);
      if (C.arity(pre[0].f) == 2) return rebuild(X, t, row, 1 + ns, second ? 1 + ns : 1, false, out);
      return rebuild(X, t, row, 1, 1, false, out);
    }
    default: {  // replace_tree
      const int cnt = sample_tree(X, g, C.depth, tr, X.W.m, N);
      return from_preorder(X, X.W.m, cnt, out);
    }
  }
}

// get_mutations (mutation.py:523-539); t in the workspace
MTGP_HD inline void mutate_tree(const Ctx& X, const float* t, Rng& g, int tr, float* out) {
  const int N = X.C.N;
  const RowInfo ri = rows_info(t, N, X.L);
  const int empty = ri.e, used = N - empty;
  double p[7] = {1, 1, 1, 1, 1, 1, 1};
  if (empty < 8) p[0] = 0, p[1] = 1, p[2] = 1, p[3] = 1, p[4] = 0, p[5] = 0, p[6] = 1;
  if (used <= 3) p[0] = 1, p[1] = 1, p[2] = 1, p[3] = 0, p[4] = 1, p[5] = 0, p[6] = 1;
  if (used == 1) p[0] = 1, p[1] = 1, p[2] = 0, p[3] = 0, p[4] = 1, p[5] = 0, p[6] = 1;
  // Rng::choice over the 0/1 table: the same draw, stepping down by exactly 1.0
  double tot = 0.0;
  for (int i = 0; i < 7; ++i) tot += p[i];
  double u = g.uniform() * tot;
  int which = 0;
  for (int i = 0; i < 7; ++i) {
    if (p[i] <= 0.0) continue;
    which = i;
    if (u < p[i]) break;
    u -= p[i];
  }
  if (!mutate_tree_op(X, which, t, ri, g, tr, out)) copy_rows(out, t, N, X.L);
}

// ------------------------------------------------------------------ crossover
// The crossover's pass over a tree's rows, low to high: the row weights (crossover.py: 0 empty,
// 2 operator, 1 leaf) as prefix sums c -- small integers, so Rng::choice's running subtraction and
// choose_prefix's binary search pick the same row for every draw -- and every row's subtree size sz
// from the arities (the operands of row k are the subtrees rooted at k-1 and just below it).  Rows
// [0, ri.lo) -- the empty rows of a valid tree: weight 0, size 1 -- are filled by the lanes
// together; the recurrence runs over the tree's own rows only.
MTGP_HD inline void scan(const Cfg& C, const float* t, RowInfo ri, int32_t* c, int32_t* sz, Lanes L) {
  const int N = C.N, nf = C.n_funcs;
  for (int k = L.lane; k < ri.lo; k += L.n) c[k + 1] = 0, sz[k] = 1;
  MTGP_EVO_SYNC();
  int acc = 0, prev = ri.lo > 0 ? 1 : 0;
  c[0] = 0;
  for (int k = ri.lo; k < N; ++k) {
    const float f = t[4 * k];
    const int fi = f2i(f);
    const bool in = fi >= 0 && fi < nf;
    const int kd = in ? C.kind[fi] : 0;  // Cfg::is_op and Cfg::arity with one range test and one lookup
    const bool isop = f >= 0.0f && (float)fi == f && (kd & 4);
    const int ar = kd & 3;
    acc += f == 0.0f ? 0 : (isop ? 2 : 1);
    c[k + 1] = acc;
    int s = 1;
    if (ar >= 1 && k >= 1) {
      const int sa = prev, kb = k - 1 - sa;  // prev == sz[k - 1], kept in a register
      s += sa;
      if (ar >= 2 && kb >= 0) s += sz[kb];
    }
    prev = sz[k] = s > N ? N : s;
  }
}

MTGP_HD inline int choose_prefix(Rng& g, const int32_t* c, int N) {
  const double u = g.uniform() * (double)c[N];
  int lo = 0, hi = N - 1;  // first i with c[i + 1] > u
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((double)c[mid + 1] > u) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

MTGP_HD inline bool cx_invalid_e(const float* t1, const float* t2, int N, int i1, int i2, int e1, int e2) {
  const int s1 = i1 - find_end_idx(t1, i1), s2 = i2 - find_end_idx(t2, i2);
  bool equal = false;
  if (s1 == s2 && (N - e1 > 1 || N - e2 > 1)) {
    equal = true;
    for (int k = 0; k < s1; ++k) {
      const float* a = t1 + 4 * (i1 - k);
      const float* b = t2 + 4 * (i2 - k);
      const bool same_leaf = a[3] == b[3] && a[0] == 1.0f;
      if (!((a[0] == b[0] && a[0] > 1.0f) || same_leaf)) {
        equal = false;
        break;
      }
    }
  }
  return e1 < s2 - s1 || e2 < s1 - s2 || equal;
}

// One crossover offspring written straight from the parents' rows (the same result as splicing the
// preorder lists through rebuild, without them): `a`'s rows above ia, then `b`'s subtree at ib (sb
// rows), then `a`'s rows below its subtree at ia (sa rows), each row
// [f, k-1 | -1, k-1-|subtree(k-1)| | -1, value if coefficient] as from_preorder writes it.  The
// subtree sizes of `a`'s rows above ia are a's own plus (sb - sa) for the ancestors of ia.  `a`
// and `b` may be the same tree (both tournaments picked one candidate).  The output rows are split
// over the lanes: every row's source and operand size follow from the two scans alone
MTGP_HD inline void splice_rows(const Ctx& X, const float* a, const int32_t* za, int lo_a, int ia, int sa,
                                const float* b, const int32_t* zb, int ib, int sb, float* o) {
  const Cfg& C = X.C;
  const int N = C.N, d = sb - sa, n = N - lo_a + d, kb = ia - sb, lo = N - n;
  auto ZA = [&](int i) { return za[clampi(i, 0, N - 1)]; };
  auto ZB = [&](int i) { return zb[clampi(i, 0, N - 1)]; };
  auto size_at = [&](int k) {  // subtree size of output row k (any segment)
    if (k > ia) {
      const int s = ZA(k);
      return k - s + 1 <= ia ? s + d : s;  // an ancestor of the splice point
    }
    if (k > kb) return ZB(ib - (ia - k));
    return ZA(k + d);
  };
  for (int k = X.L.lane; k < N; k += X.L.n) {
    const float* src;
    int bs;  // |subtree(k - 1)| in the offspring
    if (k > ia) {
      src = a + 4 * k;
      bs = size_at(k - 1);
    } else if (k > kb) {
      const int r = ib - (ia - k);
      src = b + 4 * clampi(r, 0, N - 1);
      bs = k - 1 > kb ? ZB(r - 1) : size_at(k - 1);
    } else if (k >= lo) {
      src = a + 4 * clampi(k + d, 0, N - 1);
      bs = k >= 1 ? ZA(k - 1 + d) : 0;
    } else {
      put_row(o, k, 0.0f, -1.0f, -1.0f, 0.0f);
      continue;
    }
    const int f = f2i(src[0]), ar = C.arity(f);
    put_row(o, k, (float)f, ar >= 1 ? (float)(k - 1) : -1.0f, ar == 2 ? (float)(k - 1 - bs) : -1.0f,
            f == 1 ? src[3] : 0.0f);
  }
}

// crossover of one tree pair (crossover.py:60-192); t1, t2 in the workspace
MTGP_HD inline void crossover(const Ctx& X, const float* t1, const float* t2, Rng& g, float* o1, float* o2) {
  const int N = X.C.N;
  const Ws& W = X.W;
  const RowInfo x1 = rows_info(t1, N, X.L), x2 = rows_info(t2, N, X.L);
  scan(X.C, t1, x1, W.c1, W.z1, X.L);
  scan(X.C, t2, x2, W.c2, W.z2, X.L);
  bool done = false;
  if (W.c1[N] != 0 && W.c2[N] != 0) {
    for (int it = 0; it < kMaxRetries; ++it) {
      const int i1 = choose_prefix(g, W.c1, N), i2 = choose_prefix(g, W.c2, N);
      if (cx_invalid_e(t1, t2, N, i1, i2, x1.e, x2.e)) continue;
      const int n1 = N - x1.lo, n2 = N - x2.lo, s1 = W.z1[i1], s2 = W.z2[i2];
      if (n1 - s1 + s2 <= N && n2 - s2 + s1 <= N && n1 - s1 + s2 > 0 && n2 - s2 + s1 > 0) {
        splice_rows(X, t1, W.z1, x1.lo, i1, s1, t2, W.z2, i2, s2, o1);
        splice_rows(X, t2, W.z2, x2.lo, i2, s2, t1, W.z1, i1, s1, o2);
        MTGP_EVO_SYNC();
        done = true;
      }
      break;
    }
  }
  if (!done) {
    copy_rows(o1, t1, N, X.L);
    copy_rows(o2, t2, N, X.L);
  }
}

// ------------------------------------------------------------- one generation
struct Gen {
  const float* pops;     // [num_pop, pop_size, T, N, 4]
  const float* fitness;  // [num_pop, pop_size]
  const int32_t* asc;    // [num_pop, pop_size] stable ascending order
  const int32_t* desc;   // [num_pop, pop_size] stable descending order
  float* out;            // [num_pop, E + 2 * pairs, T, N, 4]
};

// Candidate j of population i after the ring migration (reproduction.py:110-131), read through the
// source map instead of a migrated copy: the first migration_size come from the sender's best,
// the rest are the receiver's own in descending order
MTGP_HD inline const float* candidate(const Cfg& C, const Gen& G, int i, int j) {
  const int S = C.pop_size;
  j = clampi(j, 0, S - 1);
  int p = i, idx = j;
  if (C.migrate) {
    if (j < C.migration_size) {
      p = (i + C.num_pop - 1) % C.num_pop;
      idx = G.asc[(size_t)p * S + j];
    } else {
      idx = G.desc[(size_t)i * S + j];
    }
  }
  idx = clampi(idx, 0, S - 1);
  return G.pops + ((size_t)p * S + idx) * ((size_t)C.T * C.N * 4);
}

MTGP_HD inline int tournament(const Cfg& C, Rng& g, const float* F, const double* tp, int32_t* idx) {
  const int ts = C.tournament_size;  // reproduction.py:29-49
  for (int j = 0; j < ts; ++j) idx[j] = g.integer(C.pop_size);
  for (int j = 1; j < ts; ++j) {  // stable insertion sort by F
    const int x = idx[j];
    const float fx = F[x];
    int m = j;
    while (m > 0 && fx < F[idx[m - 1]]) {
      idx[m] = idx[m - 1];
      --m;
    }
    idx[m] = x;
  }
  return idx[g.choice(tp, ts)];
}

// tree_mask (mutation.py:28-41): advances g past the accepted round of T draws and returns the
// stream at that round's start, which replays the bits tree by tree
MTGP_HD inline Rng mask_round(Rng& g, int T, double p) {
  for (;;) {
    const Rng start = g;
    bool anyone = false;
    for (int t = 0; t < T; ++t) anyone |= g.uniform() < p;
    if (anyone) return start;
  }
}

MTGP_HD inline void elite_rows(const Cfg& C, const Gen& G, int i, int e, Lanes L) {
  const size_t csz = (size_t)C.T * C.N * 4;
  const int E = C.elite_size, out_size = E + 2 * ((C.pop_size - E) / 2);
  const float* src = candidate(C, G, i, G.asc[(size_t)i * C.pop_size + e]);
  float* dst = G.out + ((size_t)i * out_size + e) * csz;
  for (size_t k = L.lane; k < csz / 4; k += L.n) copy_row(dst, src, (int)k);
}

// pair k of population i: two tournaments, then crossover / mutation / resampling
MTGP_HD inline void reproduce_pair(const Ctx& X, const Gen& G, int i, int k) {
  const Cfg& C = X.C;
  const Ws& W = X.W;
  const int S = C.pop_size, T = C.T, N = C.N, E = C.elite_size, n_pairs = (S - E) / 2, out_size = E + 2 * n_pairs;
  const size_t tsz = (size_t)4 * N, csz = tsz * T;
  Rng g(C.seed, (uint64_t)i + 1, (uint64_t)k + 1);
  const float* F = G.fitness + (size_t)i * S;
  const double* tp = C.tp + (size_t)i * C.tournament_size;
  const double repro = C.rp[i];
  const float* p1 = candidate(C, G, i, tournament(C, g, F, tp, W.tour));
  const float* p2 = candidate(C, G, i, tournament(C, g, F, tp, W.tour));
  float* O = G.out + (size_t)i * csz * out_size;
  float* c1 = O + (size_t)(E + k) * csz;
  float* c2 = O + (size_t)(E + n_pairs + k) * csz;
  const int type = g.choice(C.rtp + (size_t)i * 3, 3);
  if (type == 0) {  // crossover_trees (crossover.py:194-218)
    Rng mg = mask_round(g, T, repro);
    for (int t = 0; t < T; ++t) {
      if (mg.uniform() < repro) {
        copy_rows(W.t1, p1 + t * tsz, N, X.L);
        copy_rows(W.t2, p2 + t * tsz, N, X.L);
        crossover(X, W.t1, W.t2, g, c1 + t * tsz, c2 + t * tsz);
      } else {
        copy_rows(c1 + t * tsz, p1 + t * tsz, N, X.L);
        copy_rows(c2 + t * tsz, p2 + t * tsz, N, X.L);
      }
    }
  } else if (type == 1) {  // mutate_pair (gp.py:499-511, mutation.py:555-577)
    for (int side = 0; side < 2; ++side) {
      const float* par = side ? p2 : p1;
      float* ch = side ? c2 : c1;
      Rng mg = mask_round(g, T, repro);
      for (int t = 0; t < T; ++t) {
        if (mg.uniform() < repro) {
          copy_rows(W.t1, par + t * tsz, N, X.L);
          mutate_tree(X, W.t1, g, t, ch + t * tsz);
        } else {
          copy_rows(ch + t * tsz, par + t * tsz, N, X.L);
        }
      }
    }
  } else {  // sample_pair (gp.py:513-525): two fresh candidates
    for (int side = 0; side < 2; ++side) {
      float* ch = side ? c2 : c1;
      for (int t = 0; t < T; ++t) {
        const int cnt = sample_tree(X, g, C.depth, t, W.m, N);
        from_preorder(X, W.m, cnt, ch + t * tsz);
      }
    }
  }
}

// candidate b of initialize_population (gp.py:298-308)
MTGP_HD inline void sample_candidate(const Ctx& X, long b, float* out) {
  const Cfg& C = X.C;
  Rng g(C.seed, 0x5a4d5045ull, (uint64_t)b + 1);
  for (int t = 0; t < C.T; ++t) {
    const int cnt = sample_tree(X, g, C.depth, t, X.W.m, C.N);
    from_preorder(X, X.W.m, cnt, out + ((size_t)b * C.T + t) * 4 * C.N);
  }
}

// ------------------------------------------------------------------ host side
// Argument checks, the configuration blob and the CPU drivers (the same core code, looping where
// the device uses a grid): the host library runs them on its threads, the "host twins" in
// libmtgp_hip.so serially.
// the configuration alone (what the blob is packed from)
inline bool config_ok(int32_t num_pop, int32_t T, const MtgpEvolveConfig* c) {
  if (!c || num_pop < 1 || num_pop > 65535 || T < 1 || T > 65535) return false;
  if (c->n_ops < 1 || c->n_vars < 1 || c->n_funcs < 2 || c->n_funcs > kMaxFuncs || c->max_init_depth < 1 ||
      c->max_init_depth > kMaxDepth || c->tournament_size < 1 || c->tournament_size > kMaxTournament ||
      c->elite_size < 0)
    return false;
  if (!c->slots || !c->op_index || !c->op_prob || !c->var_mask || !c->tournament_prob ||
      !c->reproduction_type_prob || !c->reproduction_prob)
    return false;
  if (c->var_start < 0 || c->var_start > c->n_funcs - c->n_vars) return false;
  for (int i = 0; i < c->n_funcs; ++i)
    if (c->slots[i] < 0 || c->slots[i] > 2) return false;
  for (int i = 0; i < c->n_ops; ++i)
    if (c->op_index[i] < 0 || c->op_index[i] >= c->n_funcs) return false;
  for (int i = 0; i < num_pop; ++i)
    if (!(c->reproduction_prob[i] > 0.0)) return false;  // tree_mask redraws until one tree is chosen
  return true;
}
inline bool args_ok(int32_t num_pop, int32_t pop_size, int32_t T, int32_t N, const MtgpEvolveConfig* c) {
  if (pop_size < 1 || N < 1 || N > kMaxNodes || !config_ok(num_pop, T, c)) return false;
  return (int64_t)num_pop * pop_size <= (1 << 27) && c->elite_size <= pop_size;
}

inline size_t blob_bytes(const MtgpEvolveConfig* c, int num_pop, int T) {
  return blob_layout(c->n_funcs, c->n_ops, c->n_vars, T, num_pop, c->tournament_size).bytes;
}
inline void pack_blob(const MtgpEvolveConfig* c, int num_pop, int T, void* out) {
  const BlobLayout b = blob_layout(c->n_funcs, c->n_ops, c->n_vars, T, num_pop, c->tournament_size);
  char* p = (char*)out;
  memset(p, 0, b.bytes);
  memcpy(p + b.op_prob, c->op_prob, sizeof(double) * (size_t)c->n_ops);
  memcpy(p + b.tp, c->tournament_prob, sizeof(double) * (size_t)num_pop * c->tournament_size);
  memcpy(p + b.rtp, c->reproduction_type_prob, sizeof(double) * (size_t)num_pop * 3);
  memcpy(p + b.rp, c->reproduction_prob, sizeof(double) * (size_t)num_pop);
  memcpy(p + b.op_index, c->op_index, sizeof(int32_t) * (size_t)c->n_ops);
  memcpy(p + b.var_mask, c->var_mask, sizeof(float) * (size_t)T * c->n_vars);
  for (int t = 0; t < T; ++t) {
    int32_t* cnt = (int32_t*)(p + b.var_cnt) + t;
    int32_t* list = (int32_t*)(p + b.var_list) + (size_t)t * c->n_vars;
    *cnt = 0;
    for (int i = 0; i < c->n_vars; ++i) {
      const float w = c->var_mask[(size_t)t * c->n_vars + i];
      if (w == 1.0f && *cnt >= 0) list[(*cnt)++] = i;
      else if (w != 0.0f) *cnt = -1;
    }
  }
  for (int i = 0; i < c->n_funcs; ++i) p[b.kind + (size_t)i] = (char)c->slots[i];
  for (int i = 0; i < c->n_ops; ++i) p[b.kind + (size_t)c->op_index[i]] |= 4;
}

// scalars of a call + views into `blob` (packed from the same configuration)
inline Cfg make_cfg(const MtgpEvolveConfig* c, int num_pop, int pop_size, int T, int N, uint64_t seed,
                    const void* blob) {
  Cfg C;
  bind_blob(C, blob_layout(c->n_funcs, c->n_ops, c->n_vars, T, num_pop, c->tournament_size), blob);
  C.n_funcs = c->n_funcs, C.n_ops = c->n_ops, C.var_start = c->var_start, C.n_vars = c->n_vars;
  C.depth = c->max_init_depth, C.tournament_size = c->tournament_size, C.elite_size = c->elite_size;
  C.migration_size = c->migration_size;
  C.migrate = num_pop > 1 && c->migration_period > 0 && (c->current_generation + 1) % c->migration_period == 0;
  C.num_pop = num_pop, C.pop_size = pop_size, C.T = T, C.N = N;
  C.sd = c->coefficient_sd;
  C.seed = seed;
  for (int d = 0; d <= kMaxDepth; ++d) C.pow07[d] = pow(0.7, (double)d);
  return C;
}

// The CPU drivers.  `run(n, grain, body)` is the caller's executor: it calls body(lo, hi) on
// disjoint ranges that cover [0, n), on at most n / grain threads.  Every range carves a workspace
// of its own and every pair / candidate owns its random stream and its output rows, so the result
// does not depend on how the ranges are cut.  Serial is the executor of a caller without threads.
struct Serial {
  template <class F>
  void operator()(long n, long, F body) const {
    body(0L, n);
  }
};

struct HostWs {  // one worker's workspace
  std::vector<char> mem;
  Ws W;
  explicit HostWs(int N)
      : mem(ws_bytes(N) + 16), W(ws_carve((void*)(((uintptr_t)mem.data() + 15) & ~(uintptr_t)15), N)) {}
};

// mtgp_evolve_populations; returns the output population size, -1 on bad arguments or no memory
template <class Exec = Serial>
inline int host_evolve(const float* pops, const float* fitness, int32_t num_pop, int32_t pop_size, int32_t T,
                       int32_t N, const MtgpEvolveConfig* c, uint64_t seed, float* out, Exec run = Exec()) try {
  if (!pops || !fitness || !out || !args_ok(num_pop, pop_size, T, N, c)) return -1;
  std::vector<char> blob(blob_bytes(c, num_pop, T));
  pack_blob(c, num_pop, T, blob.data());
  const Cfg C = make_cfg(c, num_pop, pop_size, T, N, seed, blob.data());
  // the orders k_evo_order counts (order_ranks), sorted: fit_less / fit_greater are strict weak
  // orders for any bits and the stable sort breaks their ties by index, as the ranks do
  std::vector<int32_t> ord(2 * (size_t)num_pop * pop_size);
  int32_t* asc = ord.data();
  int32_t* desc = asc + (size_t)num_pop * pop_size;
  for (int i = 0; i < num_pop; ++i) {
    const float* F = fitness + (size_t)i * pop_size;
    int32_t* a = asc + (size_t)i * pop_size;
    int32_t* d = desc + (size_t)i * pop_size;
    std::iota(a, a + pop_size, 0);
    std::iota(d, d + pop_size, 0);
    std::stable_sort(a, a + pop_size, [F](int32_t x, int32_t y) { return fit_less(F[x], F[y]); });
    std::stable_sort(d, d + pop_size, [F](int32_t x, int32_t y) { return fit_greater(F[x], F[y]); });
  }
  Gen G;
  G.pops = pops, G.fitness = fitness, G.asc = asc, G.desc = desc, G.out = out;
  const int E = c->elite_size, n_pairs = (pop_size - E) / 2;
  const long grain = 65536L / ((long)T * N);  // a thread per >= 64K tree rows of offspring
  for (int i = 0; i < num_pop; ++i) {
    for (int e = 0; e < E; ++e) elite_rows(C, G, i, e, Lanes{0, 1});
    run((long)n_pairs, grain < 1 ? 1L : grain, [&C, &G, i, N](long lo, long hi) {
      const HostWs ws(N);
      const Ctx X{C, ws.W, Lanes{0, 1}, C.pow07};
      for (long k = lo; k < hi; ++k) reproduce_pair(X, G, i, (int)k);
    });
  }
  return E + 2 * n_pairs;
} catch (const std::bad_alloc&) {
  return -1;
}

// mtgp_sample_population; returns 0, -1 on bad arguments or no memory
template <class Exec = Serial>
inline int host_sample(int32_t num_pop, int32_t pop_size, int32_t T, int32_t N, const MtgpEvolveConfig* c,
                       uint64_t seed, float* out, Exec run = Exec()) try {
  if (!out || !args_ok(num_pop, pop_size, T, N, c)) return -1;
  std::vector<char> blob(blob_bytes(c, num_pop, T));
  pack_blob(c, num_pop, T, blob.data());
  const Cfg C = make_cfg(c, num_pop, pop_size, T, N, seed, blob.data());
  run((long)num_pop * pop_size, 256L, [&C, N, out](long lo, long hi) {
    const HostWs ws(N);
    const Ctx X{C, ws.W, Lanes{0, 1}, C.pow07};
    for (long b = lo; b < hi; ++b) sample_candidate(X, b, out);
  });
  return 0;
} catch (const std::bad_alloc&) {
  return -1;
}

}  // namespace mtgp_evo

#endif  // MTGP_EVOLVE_CORE_H
