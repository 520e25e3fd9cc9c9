// blockops.hpp -- the workgroup primitives of the geometry headers (mcubes, tetmesh, sparsegrid, meshtopo, pointset), defined once.
// Device only.  Every helper takes its workgroup size as a template argument and its LDS from the caller; all of it is integer
// arithmetic or fp64 in a fixed order, so a result is a pure function of the input: two runs give identical bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsdf {

constexpr int MC_SCAN_THREADS = 1024;    // offset_scan_kernel: lanes of its one workgroup ...
constexpr int MC_SCAN_PER_THREAD = 8;    // ... and counts per lane and pass (the names are marching cubes', its first user)

// Inclusive scan of one value per lane over the N lanes of a workgroup (Hillis-Steele in sh[N]); returns the lane's prefix and
// leaves every prefix in sh.  A caller that reuses sh puts a barrier in between.
template <typename T, int N>
__device__ __forceinline__ T block_scan_incl(T x, T* sh) {
  const int t = threadIdx.x;
  sh[t] = x;
  __syncthreads();
  for (int d = 1; d < N; d <<= 1) {
    const T y = t >= d ? sh[t - d] : T(0);
    __syncthreads();
    sh[t] += y;
    __syncthreads();
  }
  return sh[t];
}

// Sum of one value per lane over the N lanes of a workgroup in a fixed halving tree (sh[N]), returned to every lane.  A caller that
// reuses sh puts a barrier in between.
template <typename T, int N>
__device__ __forceinline__ T block_tree_sum(T v, T* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int w = N / 2; w > 0; w >>= 1) {
    if (t < w) sh[t] += sh[t + w];
    __syncthreads();
  }
  return sh[0];
}

// Grid point p of a grid [nx][ny][nz] (z fastest) -> (i, j, k).
__device__ __forceinline__ void grid_ijk(int64_t p, int ny, int nz, int& i, int& j, int& k) {
  const int64_t syz = (int64_t)ny * nz;
  i = (int)(p / syz);
  const int r = (int)(p - (int64_t)i * syz);
  j = r / nz;
  k = r - j * nz;
}

// An index read from memory, clamped into [0, n) before it is used as an address.
__device__ __forceinline__ int64_t clamp_index(int64_t i, int64_t n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// NS streams of per-workgroup counts -> their exclusive 64-bit offsets; stream s's grand total goes to off[s][nb] and totals[s].
template <int NS>
struct OffsetScan {
  const int32_t* cnt[NS];      // [nb]
  int64_t* off[NS];            // [nb + 1]
  int64_t nb;
  int64_t* totals;             // [NS]
};

// One workgroup.  A pass takes MC_SCAN_THREADS * MC_SCAN_PER_THREAD counts of every stream: a lane sums its MC_SCAN_PER_THREAD
// counts, the lane sums go through block_scan_incl's steps -- all NS streams in the same step, so a pass costs one stream's
// barriers whatever NS is -- and a running carry joins the passes.  (One stream after the other in one LDS array was measured too and
// costs the two-stream user 2-3 % of this kernel: DESIGN 4.17.1.)
template <int NS>
__global__ __launch_bounds__(MC_SCAN_THREADS) void offset_scan_kernel(OffsetScan<NS> a) {
  __shared__ int64_t sh[NS][MC_SCAN_THREADS];
  const int t = threadIdx.x;
  int64_t carry[NS] = {};
  for (int64_t base = 0; base < a.nb; base += (int64_t)MC_SCAN_THREADS * MC_SCAN_PER_THREAD) {
    const int64_t b0 = base + (int64_t)t * MC_SCAN_PER_THREAD;
    int64_t x[NS] = {};
    for (int q = 0; q < MC_SCAN_PER_THREAD; ++q) {
      if (b0 + q < a.nb) {
#pragma unroll
        for (int s = 0; s < NS; ++s) x[s] += a.cnt[s][b0 + q];
      }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) sh[s][t] = x[s];
    __syncthreads();
    for (int d = 1; d < MC_SCAN_THREADS; d <<= 1) {
      int64_t y[NS];
#pragma unroll
      for (int s = 0; s < NS; ++s) y[s] = t >= d ? sh[s][t - d] : 0;
      __syncthreads();
#pragma unroll
      for (int s = 0; s < NS; ++s) sh[s][t] += y[s];
      __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      int64_t e = carry[s] + sh[s][t] - x[s];                      // exclusive offset of element b0
      for (int q = 0; q < MC_SCAN_PER_THREAD; ++q) {
        if (b0 + q < a.nb) {
          a.off[s][b0 + q] = e;
          e += a.cnt[s][b0 + q];
        }
      }
      carry[s] += sh[s][MC_SCAN_THREADS - 1];
    }
    __syncthreads();     // every lane has read the last entries before the next pass overwrites them
  }
  if (t == 0) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      a.off[s][a.nb] = carry[s];
      a.totals[s] = carry[s];
    }
  }
}

}  // namespace dsdf
