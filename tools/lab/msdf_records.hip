// Lab: how should the mesh-SDF query loop read its face records?  (not part of the product)
//   scalar  the library's msdf_query_kernel: a wave-uniform const __restrict__ read, loaded through the scalar unit
//   lds     the same loop with the records staged MSDF_BLOCK at a time through LDS by the workgroup, then read from there
// 1e5 queries in [-1, 1]^3 against random triangles (the pair test is branch-free, so its cost does not depend on the
// geometry), face splits by the library's rule; HIP events, best of 5 after 2 warm-up launches; the two variants' partials
// must be bit-identical.  One JSON line per (faces, mode, variant).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/lab/msdf_records tools/lab/msdf_records.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../../deepsdf_amd/csrc/meshsdf.hpp"

using namespace dsdf;

#define CK(x)                                                                                    \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); }   \
  } while (0)

template <bool DIST, bool WIND>
__global__ __launch_bounds__(MSDF_BLOCK) void lds_query_kernel(const MsdfTri* __restrict__ tri, int nf, int chunk,
                                                               const float* __restrict__ P, int nq, MsdfPartial part) {
  __shared__ MsdfTri tile[MSDF_BLOCK];
  const int q = blockIdx.x * MSDF_BLOCK + threadIdx.x;
  const int qc = q < nq ? q : nq - 1;
  const float3 p = make_float3(P[(int64_t)qc * 3], P[(int64_t)qc * 3 + 1], P[(int64_t)qc * 3 + 2]);
  const int f0 = blockIdx.y * chunk;
  const int f1 = min(nf, f0 + chunk);
  float best = __builtin_inff();
  int bestf = f0;
  float wsum = 0.f, wcomp = 0.f;
  for (int base = f0; base < f1; base += MSDF_BLOCK) {
    const int n = min(MSDF_BLOCK, f1 - base);
    __syncthreads();
    if ((int)threadIdx.x < n) tile[threadIdx.x] = tri[base + threadIdx.x];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const MsdfTri t = tile[j];
      const float3 ap = make_float3(p.x - t.a.x, p.y - t.a.y, p.z - t.a.z);
      if (DIST) {
        float3 rel;
        const float d2 = msdf_face_d2(t, ap, rel);
        const bool better = d2 < best;
        best = better ? d2 : best;
        bestf = better ? base + j : bestf;
      }
      if (WIND) {
        const float y = msdf_half_solid_angle(t, ap) - wcomp;
        const float s = wsum + y;
        wcomp = (s - wsum) - y;
        wsum = s;
      }
    }
  }
  if (q >= nq) return;
  const int64_t o = (int64_t)blockIdx.y * nq + q;
  if (DIST) {
    part.d2[o] = best;
    part.face[o] = bestf;
  }
  if (WIND) part.wind[o] = wsum;
}

static int n_splits(int nf, int nq) {      // the library's rule (dsdf_api.hip msdf_plan)
  const int qb = (nq + MSDF_BLOCK - 1) / MSDF_BLOCK;
  if (qb >= MSDF_TARGET_WG) return 1;
  int ns = (MSDF_TARGET_WG + qb - 1) / qb;
  ns = std::min(ns, std::min(nf / MSDF_MIN_SPLIT_FACES, MSDF_MAX_SPLITS));
  return std::max(ns, 1);
}

template <bool DIST, bool WIND>
static float run(bool lds, const MsdfTri* tri, int nf, const float* P, int nq, MsdfPartial part) {
  const int ns = n_splits(nf, nq), chunk = (nf + ns - 1) / ns;
  const dim3 grid((nq + MSDF_BLOCK - 1) / MSDF_BLOCK, ns);
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float best = 1e30f;
  for (int it = 0; it < 7; ++it) {
    CK(hipEventRecord(e0));
    if (lds) hipLaunchKernelGGL((lds_query_kernel<DIST, WIND>), grid, dim3(MSDF_BLOCK), 0, 0, tri, nf, chunk, P, nq, part);
    else hipLaunchKernelGGL((msdf_query_kernel<DIST, WIND>), grid, dim3(MSDF_BLOCK), 0, 0, tri, nf, chunk, P, nq, part);
    CK(hipGetLastError());
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    if (it >= 2 && ms < best) best = ms;
  }
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  return best;
}

int main() {
  const int nq = 100000, nv = 4096;
  std::mt19937 g(1);
  std::uniform_real_distribution<float> u(-1.f, 1.f);
  std::vector<float> hp(nq * 3), hv(nv * 3);
  for (auto& x : hp) x = u(g);
  for (auto& x : hv) x = u(g);
  float *P, *V;
  CK(hipMalloc(&P, hp.size() * 4));
  CK(hipMalloc(&V, hv.size() * 4));
  CK(hipMemcpy(P, hp.data(), hp.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(V, hv.data(), hv.size() * 4, hipMemcpyHostToDevice));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  for (int nf : {20480, 81920}) {
    std::vector<int32_t> hf(nf * 3);
    for (auto& i : hf) i = (int32_t)(g() % nv);      // random triangles over [-1, 1]^3, all indices in range
    int32_t* F;
    MsdfTri* tri;
    CK(hipMalloc(&F, hf.size() * 4));
    CK(hipMalloc(&tri, (size_t)nf * sizeof(MsdfTri)));
    CK(hipMemcpy(F, hf.data(), hf.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(msdf_prepare_kernel, dim3((nf + MSDF_PREP_BLOCK - 1) / MSDF_PREP_BLOCK), dim3(MSDF_PREP_BLOCK), 0, 0, V,
                       nv, F, nf, tri);
    CK(hipGetLastError());
    const int ns = n_splits(nf, nq);
    const size_t slab = (size_t)ns * nq;
    MsdfPartial part[2];
    char* ws[2];
    std::vector<char> host[2];
    for (int k = 0; k < 2; ++k) {
      CK(hipMalloc(&ws[k], slab * 12));
      CK(hipMemset(ws[k], 0, slab * 12));
      part[k].d2 = (float*)ws[k];
      part[k].face = (int32_t*)(ws[k] + slab * 4);
      part[k].wind = (float*)(ws[k] + slab * 8);
    }
    for (int mode = 0; mode < 2; ++mode) {
      float ms[2];
      for (int k = 0; k < 2; ++k) {
        ms[k] = mode == 0 ? run<true, true>(k == 1, tri, nf, P, nq, part[k]) : run<true, false>(k == 1, tri, nf, P, nq, part[k]);
        host[k].resize(slab * 12);
        CK(hipMemcpy(host[k].data(), ws[k], slab * 12, hipMemcpyDeviceToHost));
      }
      const bool same = memcmp(host[0].data(), host[1].data(), mode == 0 ? slab * 12 : slab * 8) == 0;
      for (int k = 0; k < 2; ++k)
        printf("{\"lab\": \"msdf_records\", \"faces\": %d, \"queries\": %d, \"splits\": %d, \"mode\": \"%s\", \"records\": \"%s\", "
               "\"ms\": %.4f, \"gpairs_s\": %.2f, \"bit_identical\": %s, \"device\": \"%s\"}\n",
               nf, nq, ns, mode == 0 ? "sdf" : "distance", k ? "lds" : "scalar", ms[k], (double)nq * nf / ms[k] / 1e6,
               same ? "true" : "false", prop.name);
      fflush(stdout);
    }
    for (int k = 0; k < 2; ++k) CK(hipFree(ws[k]));
    CK(hipFree(F));
    CK(hipFree(tri));
  }
  CK(hipFree(P));
  CK(hipFree(V));
  return 0;
}
