// Microbenchmark and check: the minimum over lanes 0..15 of a wave (FairShare::step's reduction) by
// four LDS shuffles (__shfl_xor 1, 2, 4, 8) against four DPP row operations (quad_perm for xor 1 and
// xor 2, row_ror:4 and row_ror:8 for the rest: min is symmetric, so a rotate serves).  Checks that
// lane 0 holds the same integer for random and edge inputs in all 64 lanes, then prints the cycles
// per reduction of both forms inside a dependent chain.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

__device__ __forceinline__ int min16_shfl(int m) {
#pragma unroll
  for (int w = 1; w < 16; w <<= 1) {
    const int o = __shfl_xor(m, w, 64);
    m = o < m ? o : m;
  }
  return m;
}

template <int CTRL>
__device__ __forceinline__ int dpp_min(int m) {
  const int o = __builtin_amdgcn_update_dpp(0x7fffffff, m, CTRL, 0xf, 0xf, false);
  return o < m ? o : m;
}
__device__ __forceinline__ int min16_dpp(int m) {
  m = dpp_min<0xB1>(m);   // quad_perm:[1,0,3,2]
  m = dpp_min<0x4E>(m);   // quad_perm:[2,3,0,1]
  m = dpp_min<0x124>(m);  // row_ror:4
  return dpp_min<0x128>(m);  // row_ror:8
}

// out[2 * wave + {0, 1}] = readfirstlane of the shuffle / DPP minimum of lanes 0..15 of that wave
__global__ void k_check(const int* in, int* out, int n_waves) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (wave >= n_waves) return;
  const int m = in[wave * 64 + (threadIdx.x & 63)];
  const int a = __builtin_amdgcn_readfirstlane(min16_shfl(m));
  const int b = __builtin_amdgcn_readfirstlane(min16_dpp(m));
  if ((threadIdx.x & 63) == 0) {
    out[2 * wave] = a;
    out[2 * wave + 1] = b;
  }
}

template <int MODE>
__global__ void k_time(const int* in, int* out, long long* cyc, int iters) {
  int m = in[threadIdx.x & 63];
  int acc = 0;
  const long long t0 = clock64();
#pragma unroll 4
  for (int it = 0; it < iters; ++it) {
    const int r = __builtin_amdgcn_readfirstlane(MODE == 0 ? min16_shfl(m) : min16_dpp(m));
    acc += r;
    m = (m ^ r) + it;  // the next reduction depends on this one
  }
  const long long t1 = clock64();
  out[blockIdx.x * blockDim.x + threadIdx.x] = acc + m;
  if ((threadIdx.x & 63) == 0) cyc[blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}

#define CHECK(x) do { if ((x) != hipSuccess) { printf("HIP error at line %d\n", __LINE__); return 2; } } while (0)

int main() {
  const int n_waves = 4096;
  std::vector<int> h(n_waves * 64);
  srand(7);
  const int edges[] = {0, 1, -1, 0x7fffffff, (int)0x80000000u, 0x7ffffffe, 200, 201};
  for (int w = 0; w < n_waves; ++w)
    for (int l = 0; l < 64; ++l) {
      int v = (int)(((unsigned)rand() << 16) ^ (unsigned)rand());
      if (w % 4 == 1) v = edges[rand() % 8];                     // edge values everywhere
      if (w % 4 == 2) v = l < 16 ? 0x7fffffff : rand() % 100;    // every post invalid, small values outside the row
      if (w % 4 == 3) v = (l == w % 16) ? rand() % 1000 : 0x7fffffff;  // one valid post
      h[w * 64 + l] = v;
    }
  int *in, *out;
  long long* cyc;
  CHECK(hipMalloc(&in, h.size() * sizeof(int)));
  CHECK(hipMalloc(&out, 1 << 22));
  CHECK(hipMalloc(&cyc, 1 << 16));
  CHECK(hipMemcpy(in, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_check, dim3(n_waves / 4), dim3(256), 0, 0, in, out, n_waves);
  std::vector<int> res(2 * n_waves);
  CHECK(hipMemcpy(res.data(), out, res.size() * sizeof(int), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int w = 0; w < n_waves; ++w) {
    int want = 0x7fffffff;
    for (int l = 0; l < 16; ++l) want = h[w * 64 + l] < want ? h[w * 64 + l] : want;
    if (res[2 * w] != want || res[2 * w + 1] != want) {
      if (bad < 5) printf("wave %d: host %d shuffle %d dpp %d\n", w, want, res[2 * w], res[2 * w + 1]);
      ++bad;
    }
  }
  printf("check: %d waves, %d mismatches\n", n_waves, bad);
  const int iters = 4096;
  for (int blocks : {1, 1024}) {
    for (int mode = 0; mode < 2; ++mode) {
      auto kern = mode == 0 ? k_time<0> : k_time<1>;
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, in, out, cyc, iters);
      hipEvent_t a, b;
      CHECK(hipEventCreate(&a));
      CHECK(hipEventCreate(&b));
      CHECK(hipEventRecord(a));
      hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, 0, in, out, cyc, iters);
      CHECK(hipEventRecord(b));
      CHECK(hipEventSynchronize(b));
      float ms;
      CHECK(hipEventElapsedTime(&ms, a, b));
      long long c;
      CHECK(hipMemcpy(&c, cyc, 8, hipMemcpyDeviceToHost));
      printf("%s blocks %d x 256: %.1f cyc per reduction (wave 0), kernel %.3f ms\n", mode == 0 ? "shuffle" : "dpp    ",
             blocks, (double)c / iters, ms);
    }
  }
  return bad ? 1 : 0;
}
