// Lab: how many queries per lane should the nearest-neighbour loop hold, how far should it be unrolled, and should the
// reference set come through the scalar unit or through LDS?  (not part of the product)
//   scalar<QPL, UNROLL>  the library's nn_query_kernel: a wave-uniform const __restrict__ read of R, loaded through the scalar unit
//   lds<QPL>             the same loop with R staged NN_BLOCK points at a time through LDS by the workgroup, read back by every lane
//                        from one address (a broadcast read)
// 1e6 queries against 1e5 reference points, both uniform in [-1, 1]^3; R is cut into the fewest pieces that give the launch at
// least NN_TARGET_WG workgroups (the library's rule without its floor); HIP events, best of 5 after 2 warm-up launches; every
// variant's combined result must be bit-identical to the first one's.  One JSON line per variant.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/lab/nn_variants tools/lab/nn_variants.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../deepsdf_amd/csrc/pointset.hpp"

using namespace dsdf;

#define CK(x)                                                                                    \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); }   \
  } while (0)

template <int QPL>
__global__ __launch_bounds__(NN_BLOCK) void lds_query_kernel(const float* __restrict__ R, int nr, int chunk,
                                                             const float* __restrict__ Q, int nq, float* __restrict__ d2_out,
                                                             int32_t* __restrict__ idx_out) {
  __shared__ float tile[NN_BLOCK * 3];
  const int64_t q0 = (int64_t)blockIdx.x * (NN_BLOCK * QPL) + threadIdx.x;
  float px[QPL], py[QPL], pz[QPL], best[QPL];
  int bi[QPL];
  const int j0 = blockIdx.y * chunk;
  const int j1 = min(nr, j0 + chunk);
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int64_t q = q0 + k * NN_BLOCK;
    const int64_t qc = q < nq ? q : nq - 1;
    px[k] = Q[qc * 3];
    py[k] = Q[qc * 3 + 1];
    pz[k] = Q[qc * 3 + 2];
    best[k] = __builtin_inff();
    bi[k] = j0;
  }
  for (int b = j0; b < j1; b += NN_BLOCK) {
    const int cnt = min(NN_BLOCK, j1 - b);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * 3; i += NN_BLOCK) tile[i] = R[(int64_t)b * 3 + i];
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < cnt; ++t) {
      const float rx = tile[t * 3], ry = tile[t * 3 + 1], rz = tile[t * 3 + 2];
#pragma unroll
      for (int k = 0; k < QPL; ++k) {
        const float dx = px[k] - rx, dy = py[k] - ry, dz = pz[k] - rz;
        const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const bool better = d2 < best[k];
        best[k] = better ? d2 : best[k];
        bi[k] = better ? b + t : bi[k];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int64_t q = q0 + k * NN_BLOCK;
    if (q >= nq) continue;
    const int64_t o = (int64_t)blockIdx.y * nq + q;
    d2_out[o] = best[k];
    idx_out[o] = bi[k];
  }
}

typedef void (*Kernel)(const float*, int, int, const float*, int, float*, int32_t*);

struct Variant {
  const char* name;
  int qpl, unroll;
  Kernel k;
};

int main() {
  const int nq = 1000000, nr = 100000, reps = 5;
  std::mt19937 gen(1);
  std::uniform_real_distribution<float> U(-1.f, 1.f);
  std::vector<float> hq((size_t)nq * 3), hr((size_t)nr * 3);
  for (auto& v : hq) v = U(gen);
  for (auto& v : hr) v = U(gen);
  const int max_splits = NN_MAX_SPLITS;
  float *Q, *R, *pd2, *d2, *d2_first;
  int32_t *pidx, *idx, *idx_first;
  CK(hipMalloc(&Q, hq.size() * 4));
  CK(hipMalloc(&R, hr.size() * 4));
  CK(hipMalloc(&pd2, (size_t)max_splits * nq * 4));
  CK(hipMalloc(&pidx, (size_t)max_splits * nq * 4));
  CK(hipMalloc(&d2, (size_t)nq * 4));
  CK(hipMalloc(&idx, (size_t)nq * 4));
  CK(hipMalloc(&d2_first, (size_t)nq * 4));
  CK(hipMalloc(&idx_first, (size_t)nq * 4));
  CK(hipMemcpy(Q, hq.data(), hq.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(R, hr.data(), hr.size() * 4, hipMemcpyHostToDevice));
  const Variant variants[] = {
      {"scalar", 1, 1, nn_query_kernel<1, 1>}, {"scalar", 1, 4, nn_query_kernel<1, 4>}, {"scalar", 2, 1, nn_query_kernel<2, 1>},
      {"scalar", 2, 4, nn_query_kernel<2, 4>}, {"scalar", 4, 1, nn_query_kernel<4, 1>}, {"scalar", 4, 4, nn_query_kernel<4, 4>},
      {"scalar", 4, 8, nn_query_kernel<4, 8>}, {"scalar", 8, 1, nn_query_kernel<8, 1>}, {"scalar", 8, 4, nn_query_kernel<8, 4>},
      {"lds", 1, 4, lds_query_kernel<1>},      {"lds", 4, 4, lds_query_kernel<4>},      {"lds", 8, 4, lds_query_kernel<8>},
  };
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> ha(nq), hb(nq);
  std::vector<int32_t> ia(nq), ib(nq);
  bool first = true;
  for (const Variant& v : variants) {
    const int tiles = (nq + NN_BLOCK * v.qpl - 1) / (NN_BLOCK * v.qpl);
    const int ns = std::min(max_splits, std::max(1, (NN_TARGET_WG + tiles - 1) / tiles));
    const int chunk = (nr + ns - 1) / ns;
    const dim3 grid(tiles, ns);
    float best = 1e30f;
    for (int r = 0; r < reps + 2; ++r) {
      CK(hipEventRecord(e0, 0));
      hipLaunchKernelGGL(v.k, grid, dim3(NN_BLOCK), 0, 0, (const float*)R, nr, chunk, (const float*)Q, nq, pd2, pidx);
      CK(hipGetLastError());
      CK(hipEventRecord(e1, 0));
      CK(hipEventSynchronize(e1));
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (r >= 2) best = std::min(best, ms);
    }
    hipLaunchKernelGGL(nn_combine_kernel, dim3((nq + NN_BLOCK - 1) / NN_BLOCK), dim3(NN_BLOCK), 0, 0, (const float*)pd2,
                       (const int32_t*)pidx, nq, ns, first ? d2_first : d2, first ? idx_first : idx);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    bool same = true;
    if (!first) {
      CK(hipMemcpy(ha.data(), d2_first, (size_t)nq * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(hb.data(), d2, (size_t)nq * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(ia.data(), idx_first, (size_t)nq * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(ib.data(), idx, (size_t)nq * 4, hipMemcpyDeviceToHost));
      same = memcmp(ha.data(), hb.data(), (size_t)nq * 4) == 0 && memcmp(ia.data(), ib.data(), (size_t)nq * 4) == 0;
    }
    first = false;
    printf("{\"variant\": \"%s\", \"queries_per_lane\": %d, \"unroll\": %d, \"queries\": %d, \"refs\": %d, \"splits\": %d, "
           "\"ms\": %.3f, \"gpairs_s\": %.1f, \"equals_first\": %s}\n",
           v.name, v.qpl, v.unroll, nq, nr, ns, best, (double)nq * nr / best / 1e6, same ? "true" : "false");
    fflush(stdout);
    if (!same) return 2;
  }
  return 0;
}
