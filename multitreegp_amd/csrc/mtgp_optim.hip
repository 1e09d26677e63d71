// mtgp_optim.hip -- coefficient optimisation's host work on the device (ABI v23): the candidates
// of an optimising generation stay on the GPU.  The rules are csrc/mtgp_optim_core.h
// (coefficients.py restated); this file is the launch geometry and the C entry points.
//
// Every kernel is one wave per candidate on the caller's stream, no host synchronisation, no
// device-to-host copy.  At the 50 candidates of an optimising generation they are latency-bound:
// what they buy is the host loop they replace, so they are kept plain.
//   k_coef_index   rows of 64 at a time: ballot of f == 1, prefix popcount = the row's ordinal
//   k_coef_param   the same scan; 16-B row loads and stores, f rewritten by mtgp_opt::param_f
//   k_coef_adam    best-epoch tracking, then Adam, per (candidate, coefficient of the window)
//   k_coef_scatter the scan again: a copy of the candidates with best_vals in the value column
#include <hip/hip_runtime.h>

#include <string.h>

#include "mtgp.h"
#include "mtgp_optim_core.h"

using namespace mtgp_opt;

static_assert(sizeof(MtgpAdamScalars) == sizeof(AdamScalars), "MtgpAdamScalars layout");
static_assert(sizeof(Row) == 16, "row layout");

namespace {

constexpr int kWave = 64;

// ordinal of this lane's row among the candidate's coefficient rows seen so far; `running` is
// wave-uniform and advances by the rows of this pass
__device__ inline int scan_ordinal(bool coef, int& running) {
  const uint64_t mask = __builtin_amdgcn_ballot_w64(coef);
  const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  const int ord = running + before;
  running += __builtin_popcountll(mask);
  return ord;
}

__global__ __launch_bounds__(kWave) void k_coef_index(const float4* __restrict__ cands, int TN,
                                                      int32_t* __restrict__ rowidx, int32_t* __restrict__ count) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float4* in = cands + (size_t)b * TN;
  int32_t* idx = rowidx + (size_t)b * TN;
  int running = 0;
  for (int base = 0; base < TN; base += kWave) {
    const int r = base + lane;
    const bool coef = r < TN && is_coef(in[r < TN ? r : 0].x);
    const int ord = scan_ordinal(coef, running);
    if (coef) idx[ord] = r;  // ord < number of rows scanned so far <= TN
  }
  for (int r = running + lane; r < TN; r += kWave) idx[r] = -1;
  if (lane == 0) count[b] = running;
}

__global__ __launch_bounds__(kWave) void k_coef_param(const float4* __restrict__ cands, int TN, ParamCfg P,
                                                      float4* __restrict__ pop, float* __restrict__ theta,
                                                      int32_t* __restrict__ nparam) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float4* in = cands + (size_t)b * TN;
  float4* out = pop + (size_t)b * TN;
  float* th = theta + (size_t)b * P.K;
  int running = 0;
  for (int base = 0; base < TN; base += kWave) {
    const int r = base + lane;
    const bool live = r < TN;
    float4 w = in[live ? r : 0];
    const bool coef = live && is_coef(w.x);
    const int ord = scan_ordinal(coef, running);
    if (live) {
      int32_t slot;
      w.x = param_f(P, w.x, ord, &slot);
      if (slot >= 0) th[slot] = w.w;  // slot < K
      out[r] = w;
    }
  }
  // parameters in use: the coefficient rows of the window; the rest of theta is zero
  int used = running - P.lo;
  used = used < 0 ? 0 : (used > P.K ? P.K : used);
  for (int k = used + lane; k < P.K; k += kWave) th[k] = 0.0f;
  if (lane == 0) nparam[b] = used;
}

struct AdamArgs {
  float* cands;
  const int32_t* rowidx;
  const int32_t* count;
  const float* grad;
  const float* loss;
  float *mu, *nu, *best_vals, *best_loss, *theta;
  int TN, lo, K, M, first, commit;
};

__global__ __launch_bounds__(kWave) void k_coef_adam(AdamArgs A, AdamScalars s) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float loss = A.loss[b];
  // (every lane reads best_loss[b] here, in the one wave that also writes it below)
  const bool take = better(A.first != 0, loss, A.first ? 0.0f : A.best_loss[b]);
  const int cnt = A.count[b];
  const int n = cnt < A.M ? cnt : A.M;
  float4* rows = (float4*)A.cands + (size_t)b * A.TN;
  const int32_t* idx = A.rowidx + (size_t)b * A.TN;
  for (int k = lane; k < A.K && (int64_t)A.lo + k < n; k += kWave) {  // (so j < n <= M)
    const int j = A.lo + k, r = idx[j];
    if (r < 0 || r >= A.TN) continue;
    const size_t sj = (size_t)b * A.M + j;
    const float v = rows[r].w;
    if (take) A.best_vals[sj] = v;
    float mu = A.first ? 0.0f : A.mu[sj], nu = A.first ? 0.0f : A.nu[sj];
    const float nv = adam_value(s, A.grad[(size_t)b * A.K + k], v, &mu, &nu);
    A.mu[sj] = mu;
    A.nu[sj] = nu;
    rows[r].w = nv;
    if (A.theta) A.theta[(size_t)b * A.K + k] = nv;
  }
  __syncthreads();
  if (lane == 0 && A.commit && take) A.best_loss[b] = loss;
}

__global__ __launch_bounds__(kWave) void k_coef_scatter(const float4* __restrict__ cands, int TN, int M,
                                                        const float* __restrict__ best_vals,
                                                        float4* __restrict__ out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float4* in = cands + (size_t)b * TN;
  float4* o = out + (size_t)b * TN;
  const float* bv = best_vals + (size_t)b * M;
  int running = 0;
  for (int base = 0; base < TN; base += kWave) {
    const int r = base + lane;
    const bool live = r < TN;
    float4 w = in[live ? r : 0];
    const bool coef = live && is_coef(w.x);
    const int ord = scan_ordinal(coef, running);
    if (coef && ord < M) w.w = bv[ord];
    if (live) o[r] = w;
  }
}

bool make_param(const MtgpNodeLibrary* lib, int32_t n_data, int32_t lo, int32_t K, ParamCfg* P) {
  if (!lib || lib->n_funcs < 1 || lib->n_funcs > kMaxFuncs) return false;
  P->n_funcs = lib->n_funcs, P->var_start = lib->var_start, P->n_data = n_data, P->lo = lo, P->K = K;
  memcpy(P->fn, lib->fn, kMaxFuncs);
  return param_ok(*P);
}

bool index_args(const float* cands, int32_t B, int32_t T, int32_t N, const int32_t* rowidx, const int32_t* count) {
  return cands && rowidx && count && shape_ok(B, T, N) && aligned(cands, 16) && aligned(rowidx, 4) &&
         aligned(count, 4);
}

bool param_args(const float* cands, int32_t B, int32_t T, int32_t N, const float* pop, const float* theta,
                const int32_t* nparam) {
  return cands && pop && theta && nparam && pop != cands && shape_ok(B, T, N) && aligned(cands, 16) &&
         aligned(pop, 16) && aligned(theta, 4) && aligned(nparam, 4);
}

bool adam_args(const float* cands, int32_t B, int32_t T, int32_t N, const int32_t* rowidx, const int32_t* count,
               int32_t lo, int32_t K, int32_t M, const float* grad, const float* loss, const MtgpAdamScalars* s,
               const float* mu, const float* nu, const float* best_vals, const float* best_loss, const float* theta) {
  if (!cands || !rowidx || !count || !grad || !loss || !s || !mu || !nu || !best_vals || !best_loss) return false;
  if (!shape_ok(B, T, N) || K < 1 || lo < 0 || M < 1 || (int64_t)M > (int64_t)T * N) return false;
  return aligned(cands, 16) && aligned(rowidx, 4) && aligned(count, 4) && aligned(grad, 4) && aligned(loss, 4) &&
         aligned(mu, 4) && aligned(nu, 4) && aligned(best_vals, 4) && aligned(best_loss, 4) && aligned(theta, 4);
}

bool scatter_args(const float* cands, int32_t B, int32_t T, int32_t N, int32_t M, const float* best_vals,
                  const float* out) {
  return cands && best_vals && out && out != cands && shape_ok(B, T, N) && M >= 1 && (int64_t)M <= (int64_t)T * N &&
         aligned(cands, 16) && aligned(out, 16) && aligned(best_vals, 4);
}

AdamScalars scalars(const MtgpAdamScalars* s) {
  AdamScalars a;
  memcpy(&a, s, sizeof(a));
  return a;
}

}  // namespace

extern "C" int mtgp_coef_index(const float* cands, int32_t B, int32_t T, int32_t N, int32_t* rowidx, int32_t* count,
                               void* stream) {
  if (!index_args(cands, B, T, N, rowidx, count)) return MTGP_ERR_ARG;
  hipLaunchKernelGGL(k_coef_index, dim3((unsigned)B), dim3(kWave), 0, (hipStream_t)stream, (const float4*)cands,
                     T * N, rowidx, count);
  return hipGetLastError() == hipSuccess ? MTGP_OK : MTGP_ERR_LAUNCH;
}

extern "C" int mtgp_coef_parameterise(const float* cands, int32_t B, int32_t T, int32_t N, const MtgpNodeLibrary* lib,
                                      int32_t n_data, int32_t lo, int32_t K, float* pop, float* theta,
                                      int32_t* nparam, void* stream) {
  ParamCfg P;
  if (!param_args(cands, B, T, N, pop, theta, nparam) || !make_param(lib, n_data, lo, K, &P)) return MTGP_ERR_ARG;
  hipLaunchKernelGGL(k_coef_param, dim3((unsigned)B), dim3(kWave), 0, (hipStream_t)stream, (const float4*)cands,
                     T * N, P, (float4*)pop, theta, nparam);
  return hipGetLastError() == hipSuccess ? MTGP_OK : MTGP_ERR_LAUNCH;
}

extern "C" int mtgp_coef_adam_step(float* cands, int32_t B, int32_t T, int32_t N, const int32_t* rowidx,
                                   const int32_t* count, int32_t lo, int32_t K, int32_t M, const float* grad,
                                   const float* loss, const MtgpAdamScalars* s, int32_t first, int32_t commit,
                                   float* mu, float* nu, float* best_vals, float* best_loss, float* theta,
                                   void* stream) {
  if (!adam_args(cands, B, T, N, rowidx, count, lo, K, M, grad, loss, s, mu, nu, best_vals, best_loss, theta))
    return MTGP_ERR_ARG;
  const AdamArgs A{cands, rowidx, count, grad, loss, mu, nu, best_vals, best_loss, theta, T * N, lo, K, M,
                   first != 0, commit != 0};
  hipLaunchKernelGGL(k_coef_adam, dim3((unsigned)B), dim3(kWave), 0, (hipStream_t)stream, A, scalars(s));
  return hipGetLastError() == hipSuccess ? MTGP_OK : MTGP_ERR_LAUNCH;
}

extern "C" int mtgp_coef_scatter(const float* cands, int32_t B, int32_t T, int32_t N, int32_t M,
                                 const float* best_vals, float* out, void* stream) {
  if (!scatter_args(cands, B, T, N, M, best_vals, out)) return MTGP_ERR_ARG;
  hipLaunchKernelGGL(k_coef_scatter, dim3((unsigned)B), dim3(kWave), 0, (hipStream_t)stream, (const float4*)cands,
                     T * N, M, best_vals, (float4*)out);
  return hipGetLastError() == hipSuccess ? MTGP_OK : MTGP_ERR_LAUNCH;
}

// the same core on host memory, no GPU needed
extern "C" int mtgp_coef_index_host(const float* cands, int32_t B, int32_t T, int32_t N, int32_t* rowidx,
                                    int32_t* count) {
  if (!index_args(cands, B, T, N, rowidx, count)) return MTGP_ERR_ARG;
  host_index(cands, B, T, N, rowidx, count);
  return MTGP_OK;
}

extern "C" int mtgp_coef_parameterise_host(const float* cands, int32_t B, int32_t T, int32_t N,
                                           const MtgpNodeLibrary* lib, int32_t n_data, int32_t lo, int32_t K,
                                           float* pop, float* theta, int32_t* nparam) {
  ParamCfg P;
  if (!param_args(cands, B, T, N, pop, theta, nparam) || !make_param(lib, n_data, lo, K, &P)) return MTGP_ERR_ARG;
  host_parameterise(cands, B, T, N, P, pop, theta, nparam);
  return MTGP_OK;
}

extern "C" int mtgp_coef_adam_step_host(float* cands, int32_t B, int32_t T, int32_t N, const int32_t* rowidx,
                                        const int32_t* count, int32_t lo, int32_t K, int32_t M, const float* grad,
                                        const float* loss, const MtgpAdamScalars* s, int32_t first, int32_t commit,
                                        float* mu, float* nu, float* best_vals, float* best_loss, float* theta) {
  if (!adam_args(cands, B, T, N, rowidx, count, lo, K, M, grad, loss, s, mu, nu, best_vals, best_loss, theta))
    return MTGP_ERR_ARG;
  host_adam_step(cands, B, T, N, rowidx, count, lo, K, M, grad, loss, scalars(s), first != 0, commit != 0, mu, nu,
                 best_vals, best_loss, theta);
  return MTGP_OK;
}

extern "C" int mtgp_coef_scatter_host(const float* cands, int32_t B, int32_t T, int32_t N, int32_t M,
                                      const float* best_vals, float* out) {
  if (!scatter_args(cands, B, T, N, M, best_vals, out)) return MTGP_ERR_ARG;
  host_scatter(cands, B, T, N, M, best_vals, out);
  return MTGP_OK;
}
