// mtgp_optim_core.h -- the host side of coefficient optimisation (multitreegp_amd/coefficients.py:
// coefficient_rows, parameterise, Adam.update, the best-epoch choice of optimise) restated
// allocation-free for the host and the device (MTGP_HD), so the optimising generation can stay on
// the GPU.  Those Python functions stay the first implementation (the numpy-input loop, pinned to
// the oracle); this header is the second one the parity tests hold against them bit for bit
// (tests/test_device_optimise_host.py,
// tests/test_gpu_device_optimise.py).
//
// Everything here is per row or per (candidate, coefficient): the kernels (csrc/mtgp_optim.hip)
// supply a coefficient row's ordinal by ballot + prefix popcount, the host twins by a running
// count.  Rows are [f, a, b, value]; a coefficient row is one with f == 1.0f exactly.
//
// Floating point: compiled with -ffp-contract=off and no fast-math, so every multiply, add,
// divide and square root below is one correctly rounded float32 operation on both sides, the
// operations numpy performs in Adam.update.
//
// Safety: no index is derived from row contents except the node-function lookup, whose index is
// clamped to the library first; ordinals are bounded by T * N and windows by K.
#ifndef MTGP_OPTIM_CORE_H
#define MTGP_OPTIM_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "mtgp_f32math.h"

namespace mtgp_opt {

constexpr int kMaxFuncs = 128;  // MTGP_MAX_FUNCS
constexpr int kMaxNodes = 256;  // MTGP_MAX_NODES
constexpr int kMaxData = 64;    // MTGP_MAX_DATA
constexpr int kFnVar = 1;       // MTGP_FN_VAR

struct Row {
  float f, a, b, v;
};

// what parameterise needs of the node library and the chunk window, passed by value
struct ParamCfg {
  int32_t n_funcs, var_start;  // the evaluator's library (before the K parameter slots)
  int32_t n_data, lo, K;       // data-vector length, first coefficient ordinal and size of the window
  int8_t fn[kMaxFuncs];
};

// the nine float32 scalars of one Adam.update, computed by the host with numpy's expressions
struct AdamScalars {
  float a, b;    // 1 - b1, b1
  float c, d;    // 1 - b2, b2
  float c1, c2;  // 1 - b1^t, 1 - b2^t
  float eps_root, eps, neg_lr;
};

MTGP_HD inline bool is_coef(float f) { return f == 1.0f; }

// coefficients._f2i_sat: truncation towards zero, saturating, NaN -> 0 (only compared with small
// library indices afterwards, so int32 saturation equals the int64 of the numpy code)
MTGP_HD inline int32_t f2i_sat(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return INT32_MAX;
  if (f <= -2147483648.0f) return INT32_MIN;
  return (int32_t)f;
}

// The f column of one row under parameterise.  ord: the row's ordinal among its candidate's
// coefficient rows (used only when it is one).  *slot: k - lo when the row becomes parameter
// k - lo of the window (its value goes to theta), else -1.
MTGP_HD inline float param_f(const ParamCfg& P, float f, int32_t ord, int32_t* slot) {
  *slot = -1;
  if (is_coef(f)) {
    const int64_t k = (int64_t)ord - P.lo;
    if (k < 0 || k >= P.K) return f;  // outside the window: stays a coefficient row
    *slot = (int32_t)k;
    return (float)(P.var_start + P.n_data + (int32_t)k);
  }
  const int32_t top = P.n_funcs - 1;
  int32_t fi = f2i_sat(f);
  if (fi > top) {  // lax.switch clamps the operator index
    f = (float)top;
    fi = top;
  }
  if (fi >= P.var_start && fi <= top) {
    const int32_t c = fi < 0 ? 0 : fi;
    if (P.fn[c] == kFnVar && fi - P.var_start > P.n_data - 1) f = (float)(P.var_start + P.n_data - 1);
  }
  return f;
}

// np.argmin over the epochs, one epoch at a time: true when this epoch's loss replaces the best
// so far (first epoch; strictly smaller; or the first NaN, which np.argmin returns)
MTGP_HD inline bool better(bool first, float loss, float best) {
  if (first) return true;
  if (best != best) return false;
  return loss != loss || loss < best;
}

// Adam.update followed by values + update, operation for operation
MTGP_HD inline float adam_value(const AdamScalars& s, float g, float v, float* mu_io, float* nu_io) {
  const float m1 = s.a * g, m2 = s.b * *mu_io;
  const float mu = m1 + m2;
  const float gg = g * g;
  const float n1 = s.c * gg, n2 = s.d * *nu_io;
  const float nu = n1 + n2;
  const float mu_hat = mu / s.c1;
  const float nu_hat = nu / s.c2;
  const float r = mtgp_sqrtf(nu_hat + s.eps_root);
  const float u = mu_hat / (r + s.eps);
  const float upd = s.neg_lr * u;
  *mu_io = mu;
  *nu_io = nu;
  return v + upd;
}

// ------------------------------------------------------------------ argument rules
MTGP_HD inline bool shape_ok(int64_t B, int64_t T, int64_t N) {
  return B >= 1 && T >= 1 && N >= 1 && N <= kMaxNodes && B * T * N <= ((int64_t)1 << 27);
}

inline bool param_ok(const ParamCfg& P) {
  return P.n_funcs >= 1 && P.n_funcs <= kMaxFuncs && P.var_start >= 0 && P.n_data >= 1 && P.K >= 1 && P.lo >= 0 &&
         (int64_t)P.n_data + P.K <= kMaxData && (int64_t)P.var_start + P.n_data + P.K <= kMaxFuncs;
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

// ------------------------------------------------------------------ the host twins
// rowidx [B, T*N]: flat (tree * N + row) index of the j-th coefficient row (-1 beyond the count)
inline void host_index(const float* cands, int B, int T, int N, int32_t* rowidx, int32_t* count) {
  const int TN = T * N;
  for (int b = 0; b < B; ++b) {
    const Row* rows = (const Row*)cands + (size_t)b * TN;
    int n = 0;
    for (int r = 0; r < TN; ++r)
      if (is_coef(rows[r].f)) rowidx[(size_t)b * TN + n++] = r;
    count[b] = n;
    for (int r = n; r < TN; ++r) rowidx[(size_t)b * TN + r] = -1;
  }
}

inline void host_parameterise(const float* cands, int B, int T, int N, const ParamCfg& P, float* pop, float* theta,
                              int32_t* nparam) {
  const int TN = T * N;
  for (int b = 0; b < B; ++b) {
    const Row* in = (const Row*)cands + (size_t)b * TN;
    Row* out = (Row*)pop + (size_t)b * TN;
    for (int k = 0; k < P.K; ++k) theta[(size_t)b * P.K + k] = 0.0f;
    int ord = 0, used = 0;
    for (int r = 0; r < TN; ++r) {
      Row w = in[r];
      int32_t slot;
      w.f = param_f(P, w.f, ord, &slot);
      if (is_coef(in[r].f)) ++ord;
      if (slot >= 0) {
        theta[(size_t)b * P.K + slot] = w.v;
        ++used;
      }
      out[r] = w;
    }
    nparam[b] = used;
  }
}

// One epoch for the window [lo, lo + K) of every candidate's coefficients.  State arrays mu, nu,
// best_vals are [B, M] over all of a candidate's coefficients (M >= every count); grad and theta
// are the window's [B, K].  commit: this is the epoch's last window, best_loss takes the loss.
inline void host_adam_step(float* cands, int B, int T, int N, const int32_t* rowidx, const int32_t* count, int lo,
                           int K, int M, const float* grad, const float* loss, const AdamScalars& s, bool first,
                           bool commit, float* mu, float* nu, float* best_vals, float* best_loss, float* theta) {
  const int TN = T * N;
  for (int b = 0; b < B; ++b) {
    Row* rows = (Row*)cands + (size_t)b * TN;
    const bool take = better(first, loss[b], first ? 0.0f : best_loss[b]);
    const int n = count[b] < M ? count[b] : M;
    for (int k = 0; k < K && (int64_t)lo + k < n; ++k) {  // (so j < n <= M)
      const int j = lo + k, r = rowidx[(size_t)b * TN + j];
      if (r < 0 || r >= TN) continue;
      const size_t sj = (size_t)b * M + j;
      const float v = rows[r].v;
      if (take) best_vals[sj] = v;
      float m = first ? 0.0f : mu[sj], u = first ? 0.0f : nu[sj];  // the first epoch starts from Adam.init
      const float nv = adam_value(s, grad[(size_t)b * K + k], v, &m, &u);
      mu[sj] = m;
      nu[sj] = u;
      rows[r].v = nv;
      if (theta) theta[(size_t)b * K + k] = nv;
    }
    if (commit && take) best_loss[b] = loss[b];
  }
}

inline void host_scatter(const float* cands, int B, int T, int N, int M, const float* best_vals, float* out) {
  const int TN = T * N;
  for (int b = 0; b < B; ++b) {
    const Row* in = (const Row*)cands + (size_t)b * TN;
    Row* o = (Row*)out + (size_t)b * TN;
    int ord = 0;
    for (int r = 0; r < TN; ++r) {
      Row w = in[r];
      if (is_coef(w.f)) {
        if (ord < M) w.v = best_vals[(size_t)b * M + ord];
        ++ord;
      }
      o[r] = w;
    }
  }
}

}  // namespace mtgp_opt
#endif  // MTGP_OPTIM_CORE_H
