// mtgp_evolve.cpp -- the native host library (include/mtgp_host.h, libmtgp_host.so): the evolution
// step of csrc/mtgp_evolve_core.h on the CPU, so a whole generation at BASELINE scale costs
// milliseconds next to the GPU evaluation.  This file is the threads and the C entry points; the
// operators, the argument checks and the drivers (host_evolve, host_sample) are the core header's.
//
// The pairs of a population are independent (one random stream and two output candidates each), so
// they run on plain std::threads (contiguous blocks, no OpenMP runtime to spin beside torch's) with
// a result that does not depend on the thread count.
#include <sched.h>

#include <algorithm>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mtgp_evolve_core.h"

namespace {

// Threads: MTGP_HOST_THREADS, else OMP_NUM_THREADS (the CPU share a GPU pool grants the job), else
// the process's CPU affinity, at most 64.
long host_threads() {
  if (const char* e = std::getenv("MTGP_HOST_THREADS")) return std::max(1L, std::atol(e));
  if (const char* e = std::getenv("OMP_NUM_THREADS")) return std::max(1L, std::min(64L, std::atol(e)));
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof(set), &set) == 0) return std::max(1L, std::min(64L, (long)CPU_COUNT(&set)));
  return 8;
}

// body(lo, hi) over contiguous blocks of [0, n) on host_threads() threads; a thread only for every
// `grain` items (the core's executor)
struct ParallelFor {
  template <class F>
  void operator()(long n, long grain, F body) const {
    const long hw = std::max(1L, (long)std::thread::hardware_concurrency());
    const long nt = std::max(1L, std::min({host_threads(), hw, n / std::max(1L, grain)}));
    if (nt == 1) return body(0L, n);
    std::vector<std::thread> th;
    for (long t = 0; t < nt; ++t) th.emplace_back([=, &body]() { body(n * t / nt, n * (t + 1) / nt); });
    for (auto& x : th) x.join();
  }
};

}  // namespace

extern "C" int mtgp_host_abi_version(void) { return MTGP_HOST_ABI_VERSION; }

extern "C" int mtgp_evolve_populations(const float* pops, const float* fitness, int32_t num_pop, int32_t pop_size,
                                       int32_t T, int32_t N, const MtgpEvolveConfig* cfg, uint64_t seed, float* out) {
  return mtgp_evo::host_evolve(pops, fitness, num_pop, pop_size, T, N, cfg, seed, out, ParallelFor());
}

extern "C" int mtgp_sample_population(int32_t num_pop, int32_t pop_size, int32_t T, int32_t N,
                                      const MtgpEvolveConfig* cfg, uint64_t seed, float* out) {
  return mtgp_evo::host_sample(num_pop, pop_size, T, N, cfg, seed, out, ParallelFor());
}
