// mtgp_evolve.hip -- the evolution step on the device (ABI v22): the population stays on the GPU
// between generations.  The algorithm is csrc/mtgp_evolve_core.h (the one implementation, which
// the host library runs too); this file is the launch geometry and the C entry points.  The host
// twins at the end run the core's CPU drivers serially (mtgp_evo::Serial): test instruments.
//
// A generation is three launches on the caller's stream, no host synchronisation, no D2H copy:
//   k_evo_order   one thread per candidate: its stable ascending and descending fitness ranks (counted)
//                 (elitism / migration sender, migration receiver), scattered into order arrays
//   k_evo_elite   one block per elite candidate: coalesced 16-B row copies
//   k_evo_repro   one wave per (population, pair): the pair's xoshiro stream runs redundantly in
//                 every lane (wave-uniform decisions), scans and node lists in LDS, rows 16 B per lane
// The migrated population is never materialised: parents are read through the source map the two
// order arrays define (mtgp_evo::candidate).
#include <hip/hip_runtime.h>

#include "mtgp.h"
#include "mtgp_evolve_core.h"

using namespace mtgp_evo;

namespace {

constexpr int kWave = 64;
constexpr int kOrderBlock = 256;
constexpr int kOrderTile = 2048;  // fitness values staged in LDS per pass of k_evo_order
constexpr int kEliteBlock = 256;

__global__ __launch_bounds__(kOrderBlock) void k_evo_order(const float* __restrict__ fitness, int S,
                                                           int32_t* __restrict__ asc, int32_t* __restrict__ desc) {
  // mtgp_evo::order_ranks with the fitness vector staged through LDS a tile at a time (every
  // thread reads all S values: broadcast LDS reads instead of S dependent global loads)
  __shared__ float tile[kOrderTile];
  const int p = blockIdx.y, i = blockIdx.x * kOrderBlock + threadIdx.x;
  const float* F = fitness + (size_t)p * S;
  const bool live = i < S;
  const float x = live ? F[i] : 0.0f;
  int ra = 0, rd = 0;
  for (int base = 0; base < S; base += kOrderTile) {
    const int n = S - base < kOrderTile ? S - base : kOrderTile;
    for (int j = threadIdx.x; j < n; j += kOrderBlock) tile[j] = F[base + j];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const float y = tile[j];
      const int tie = fit_same(y, x) && base + j < i;
      ra += fit_less(y, x) || tie;
      rd += fit_greater(y, x) || tie;
    }
    __syncthreads();
  }
  if (live) {
    asc[(size_t)p * S + ra] = i;  // ranks of a total order: a permutation of [0, S)
    desc[(size_t)p * S + rd] = i;
  }
}

__global__ __launch_bounds__(kEliteBlock) void k_evo_elite(Cfg C, Gen G) {
  Lanes L;
  L.lane = threadIdx.x, L.n = kEliteBlock;
  elite_rows(C, G, blockIdx.y, blockIdx.x, L);
}

__global__ __launch_bounds__(kWave) void k_evo_repro(Cfg C, Gen G) {
  extern __shared__ __align__(16) char evo_lds[];
  const Ws W = ws_carve(evo_lds, C.N);
  for (int i = threadIdx.x; i < C.n_funcs; i += kWave) W.kind[i] = C.kind[i];
  __syncthreads();
  Cfg L = C;  // scalars and blob pointers; the pow table stays in the argument (Ctx::pw)
  L.kind = W.kind;
  const Ctx X{L, W, Lanes{(int)threadIdx.x, kWave}, C.pow07};
  reproduce_pair(X, G, blockIdx.y, blockIdx.x);
}

__global__ __launch_bounds__(kWave) void k_evo_sample(Cfg C, float* out) {
  extern __shared__ __align__(16) char evo_lds[];
  const Ws W = ws_carve(evo_lds, C.N);
  for (int i = threadIdx.x; i < C.n_funcs; i += kWave) W.kind[i] = C.kind[i];
  __syncthreads();
  Cfg L = C;  // scalars and blob pointers; the pow table stays in the argument (Ctx::pw)
  L.kind = W.kind;
  const Ctx X{L, W, Lanes{(int)threadIdx.x, kWave}, C.pow07};
  sample_candidate(X, (long)blockIdx.x, out);
}

}  // namespace

extern "C" int mtgp_evolve_config_pack(const MtgpEvolveConfig* cfg, int32_t num_pop, int32_t num_trees, void* blob,
                                       int32_t capacity) {
  if (!config_ok(num_pop, num_trees, cfg)) return MTGP_ERR_ARG;
  const size_t bytes = blob_bytes(cfg, num_pop, num_trees);
  if (bytes > (size_t)INT32_MAX) return MTGP_ERR_ARG;
  if (blob) {
    if ((size_t)capacity < bytes) return MTGP_ERR_ARG;
    pack_blob(cfg, num_pop, num_trees, blob);
  }
  return (int)bytes;
}

extern "C" int mtgp_evolve_workspace_bytes(int32_t num_pop, int32_t pop_size) {
  if (num_pop < 1 || pop_size < 1 || (int64_t)num_pop * pop_size > (1 << 27)) return MTGP_ERR_ARG;
  return (int)(2 * sizeof(int32_t) * (size_t)num_pop * pop_size);
}

extern "C" int mtgp_evolve_device(const float* populations, const float* fitness, int32_t num_pop, int32_t pop_size,
                                  int32_t num_trees, int32_t N, const MtgpEvolveConfig* cfg, const void* blob,
                                  uint64_t seed, void* workspace, float* out, void* stream) {
  if (!populations || !fitness || !blob || !workspace || !out) return MTGP_ERR_ARG;
  if (!args_ok(num_pop, pop_size, num_trees, N, cfg)) return MTGP_ERR_ARG;
  if ((((uintptr_t)populations) | ((uintptr_t)out) | ((uintptr_t)blob)) & 15u) return MTGP_ERR_ARG;
  if (((uintptr_t)workspace | (uintptr_t)fitness) & 3u) return MTGP_ERR_ARG;
  const Cfg C = make_cfg(cfg, num_pop, pop_size, num_trees, N, seed, blob);
  Gen G;
  G.pops = populations, G.fitness = fitness, G.out = out;
  int32_t* asc = (int32_t*)workspace;
  int32_t* desc = asc + (size_t)num_pop * pop_size;
  G.asc = asc, G.desc = desc;
  hipStream_t s = (hipStream_t)stream;
  const int E = cfg->elite_size, n_pairs = (pop_size - E) / 2;
  hipLaunchKernelGGL(k_evo_order, dim3((unsigned)((pop_size + kOrderBlock - 1) / kOrderBlock), (unsigned)num_pop),
                     dim3(kOrderBlock), 0, s, fitness, pop_size, asc, desc);
  if (hipGetLastError() != hipSuccess) return MTGP_ERR_LAUNCH;
  if (E > 0) {
    hipLaunchKernelGGL(k_evo_elite, dim3((unsigned)E, (unsigned)num_pop), dim3(kEliteBlock), 0, s, C, G);
    if (hipGetLastError() != hipSuccess) return MTGP_ERR_LAUNCH;
  }
  if (n_pairs > 0) {
    hipLaunchKernelGGL(k_evo_repro, dim3((unsigned)n_pairs, (unsigned)num_pop), dim3(kWave), ws_bytes(N), s, C, G);
    if (hipGetLastError() != hipSuccess) return MTGP_ERR_LAUNCH;
  }
  return E + 2 * n_pairs;
}

extern "C" int mtgp_sample_population_device(int32_t num_pop, int32_t pop_size, int32_t num_trees, int32_t N,
                                             const MtgpEvolveConfig* cfg, const void* blob, uint64_t seed, float* out,
                                             void* stream) {
  if (!blob || !out || !args_ok(num_pop, pop_size, num_trees, N, cfg)) return MTGP_ERR_ARG;
  if ((((uintptr_t)out) | ((uintptr_t)blob)) & 15u) return MTGP_ERR_ARG;
  const Cfg C = make_cfg(cfg, num_pop, pop_size, num_trees, N, seed, blob);
  hipLaunchKernelGGL(k_evo_sample, dim3((unsigned)((long)num_pop * pop_size)), dim3(kWave), ws_bytes(N),
                     (hipStream_t)stream, C, out);
  if (hipGetLastError() != hipSuccess) return MTGP_ERR_LAUNCH;
  return MTGP_OK;
}

extern "C" int mtgp_evolve_device_host(const float* populations, const float* fitness, int32_t num_pop,
                                       int32_t pop_size, int32_t num_trees, int32_t N, const MtgpEvolveConfig* cfg,
                                       uint64_t seed, float* out) {
  // the device entry's 16-B rule (the kernels move rows as float4), kept so both reject alike
  if ((((uintptr_t)populations) | ((uintptr_t)out)) & 15u) return MTGP_ERR_ARG;
  const int rc = host_evolve(populations, fitness, num_pop, pop_size, num_trees, N, cfg, seed, out);
  return rc < 0 ? MTGP_ERR_ARG : rc;
}

extern "C" int mtgp_sample_population_device_host(int32_t num_pop, int32_t pop_size, int32_t num_trees, int32_t N,
                                                  const MtgpEvolveConfig* cfg, uint64_t seed, float* out) {
  if ((uintptr_t)out & 15u) return MTGP_ERR_ARG;
  return host_sample(num_pop, pop_size, num_trees, N, cfg, seed, out) < 0 ? MTGP_ERR_ARG : MTGP_OK;
}
