// pointset.hpp -- point-set kernels behind the reconstruction metrics (gfx950): brute-force nearest neighbour between two point
// sets, a deterministic fp64 mean, and area-weighted sampling of a triangle mesh's surface.
//
// Spec: include/dsdf.h (dsdf_nn_*, dsdf_mean_f64, dsdf_surf_*), restated in fp64 / numpy by tests/pointset_numpy.py.
//
// Nearest neighbour -- the layout of meshsdf.hpp's query pass with a 9-instruction pair test:
//   query:   NN_QPL queries per lane (q = tile * NN_TILE + k * NN_BLOCK + lane: every load and store is coalesced), NN_BLOCK lanes
//            per workgroup; blockIdx.y takes one contiguous range of R (split).  The loop over R is wave-uniform: every lane reads
//            the same point, which the compiler loads through the scalar unit (const __restrict__, uniform index); one scalar
//            load feeds NN_QPL * 64 pair tests.  With one split the kernel writes the outputs itself.
//   combine: one thread per query walks the splits in order with strict <, so the lowest index wins ties across splits as it
//            does inside one.
// Mean -- contiguous slices per workgroup, fp64 lane sums in a fixed stride order, a fixed LDS tree, a one-workgroup final pass.
// Surface sampling -- prepare: per-face fp32 area, a three-pass fp64 inclusive scan (tile sums, scan of the tile sums by one
//   workgroup, tile scan plus offset); sample: one thread per sample, Philox4x32-10 keyed by the seed with the sample's index
//   as counter, a binary search of the CDF, barycentric point.
// No atomics anywhere; two identical calls give identical bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blockops.hpp"
#include "common.hpp"

namespace dsdf {

constexpr int NN_BLOCK = 256;
constexpr int NN_QPL = 4;                     // queries per lane   } what the library instantiates; tools/lab/nn_variants.hip
constexpr int NN_UNROLL = 4;                  // points per wait    } measures the alternatives
constexpr int NN_TILE = NN_BLOCK * NN_QPL;    // queries per workgroup
constexpr int NN_TARGET_WG = 2048;            // workgroups a query launch aims for (8 per CU) before it stops splitting R
constexpr int NN_MIN_SPLIT_REFS = 1024;       // no split gets fewer reference points than this
constexpr int NN_MAX_SPLITS = 64;

// Split s = blockIdx.y covers R[s * chunk, min(nr, (s + 1) * chunk)) and writes row s of d2 / idx ([n_splits][nq]; either may be
// NULL).  A lane whose split holds no comparable point (every d2 NaN or +inf) reports (+inf, first index of the split).
template <int QPL, int UNROLL>
__global__ __launch_bounds__(NN_BLOCK) void nn_query_kernel(const float* __restrict__ R, int nr, int chunk,
                                                            const float* __restrict__ Q, int nq, float* __restrict__ d2_out,
                                                            int32_t* __restrict__ idx_out) {
  const int64_t q0 = (int64_t)blockIdx.x * (NN_BLOCK * QPL) + threadIdx.x;
  float px[QPL], py[QPL], pz[QPL], best[QPL];
  int bi[QPL];
  const int j0 = blockIdx.y * chunk;
  const int j1 = min(nr, j0 + chunk);
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int64_t q = q0 + k * NN_BLOCK;
    const int64_t qc = q < nq ? q : nq - 1;             // tail lanes compute a duplicate and write nothing
    px[k] = Q[qc * 3];
    py[k] = Q[qc * 3 + 1];
    pz[k] = Q[qc * 3 + 2];
    best[k] = __builtin_inff();
    bi[k] = j0;
  }
#pragma unroll UNROLL                                   // UNROLL points' scalar loads in flight per wait
  for (int j = j0; j < j1; ++j) {
    const float rx = R[(int64_t)j * 3], ry = R[(int64_t)j * 3 + 1], rz = R[(int64_t)j * 3 + 2];
#pragma unroll
    for (int k = 0; k < QPL; ++k) {
      const float dx = px[k] - rx, dy = py[k] - ry, dz = pz[k] - rz;
      const float d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
      const bool better = d2 < best[k];                 // false for NaN: such a pair is never chosen
      best[k] = better ? d2 : best[k];
      bi[k] = better ? j : bi[k];
    }
  }
#pragma unroll
  for (int k = 0; k < QPL; ++k) {
    const int64_t q = q0 + k * NN_BLOCK;
    if (q >= nq) continue;
    const int64_t o = (int64_t)blockIdx.y * nq + q;
    if (d2_out) d2_out[o] = best[k];
    if (idx_out) idx_out[o] = bi[k];
  }
}

__global__ __launch_bounds__(NN_BLOCK) void nn_combine_kernel(const float* __restrict__ pd2, const int32_t* __restrict__ pidx,
                                                              int nq, int n_splits, float* __restrict__ d2_out,
                                                              int32_t* __restrict__ idx_out) {
  const int64_t q = (int64_t)blockIdx.x * NN_BLOCK + threadIdx.x;
  if (q >= nq) return;
  float best = pd2[q];
  int bi = pidx[q];
  for (int s = 1; s < n_splits; ++s) {
    const int64_t o = (int64_t)s * nq + q;
    const float d2 = pd2[o];
    if (d2 < best) {
      best = d2;
      bi = pidx[o];
    }
  }
  if (d2_out) d2_out[q] = best;
  if (idx_out) idx_out[q] = bi;
}

// ---- mean ------------------------------------------------------------------------------------------------------------------
constexpr int MEAN_BLOCK = 256;
constexpr int MEAN_MAX_BLOCKS = 1024;          // partial sums: the fixed workspace of dsdf_mean_f64 (DSDF_MEAN_WS_BYTES)
constexpr int MEAN_MIN_SLICE = 4096;           // values per workgroup before a second workgroup is started

// Workgroup b sums x[b * slice, min(n, (b + 1) * slice)): lane t takes elements t, t + 256, ... of the slice in order.
__global__ __launch_bounds__(MEAN_BLOCK) void mean_partial_kernel(const float* __restrict__ x, int64_t n, int64_t slice,
                                                                  double* __restrict__ part) {
  __shared__ double sh[MEAN_BLOCK];
  const int64_t i0 = (int64_t)blockIdx.x * slice;
  const int64_t i1 = i0 + slice < n ? i0 + slice : n;
  double s = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += MEAN_BLOCK) s += (double)x[i];
  const double tot = block_tree_sum<double, MEAN_BLOCK>(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(MEAN_BLOCK) void mean_final_kernel(const double* __restrict__ part, int n_part, int64_t n,
                                                                double* __restrict__ mean) {
  __shared__ double sh[MEAN_BLOCK];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += MEAN_BLOCK) s += part[i];
  const double tot = block_tree_sum<double, MEAN_BLOCK>(s, sh);
  if (threadIdx.x == 0) mean[0] = tot / (double)n;
}

// ---- surface sampling ------------------------------------------------------------------------------------------------------
constexpr int SURF_BLOCK = 256;
constexpr int SURF_PER_LANE = 4;
constexpr int SURF_TILE = SURF_BLOCK * SURF_PER_LANE;       // faces per workgroup of the scan

struct SurfBuf {          // carved from the caller's `surf` buffer (dsdf_surf_plan)
  double* cdf;            // [nf] inclusive prefix sums of area; cdf[nf - 1] is the total
  double* tile;           // [n_tiles] tile sums, then their exclusive prefix sums
  float* area;            // [nf]
};

__device__ __forceinline__ void surf_face(const float* __restrict__ V, int nv, const int32_t* __restrict__ F, int64_t f,
                                          float3& a, float3& ab, float3& ac) {
  float3 v[3];
  for (int r = 0; r < 3; ++r) {
    int i = F[f * 3 + r];
    i = i < 0 ? 0 : (i >= nv ? nv - 1 : i);             // the host range-checks; this only keeps reads inside V
    v[r] = make_float3(V[(int64_t)i * 3], V[(int64_t)i * 3 + 1], V[(int64_t)i * 3 + 2]);
  }
  a = v[0];
  ab = make_float3(v[1].x - v[0].x, v[1].y - v[0].y, v[1].z - v[0].z);
  ac = make_float3(v[2].x - v[0].x, v[2].y - v[0].y, v[2].z - v[0].z);
}

// area = 0.5 * sqrt(n.n), n = ab x ac; every product, difference and sum rounded on its own -- the rn_* helpers of common.hpp keep
// the compiler from contracting them -- and sqrtf is the correctly rounded root (__fsqrt_rn is not), so the host can restate the
// areas bit for bit (tests/pointset_numpy.py face_areas_f32).  Once per mesh: the root's refinement costs nothing that matters.
__global__ __launch_bounds__(SURF_BLOCK) void surf_area_kernel(const float* __restrict__ V, int nv, const int32_t* __restrict__ F,
                                                               int nf, float* __restrict__ area) {
  const int64_t f = (int64_t)blockIdx.x * SURF_BLOCK + threadIdx.x;
  if (f >= nf) return;
  float3 a, ab, ac;
  surf_face(V, nv, F, f, a, ab, ac);
  const float nx = rn_sub(rn_mul(ab.y, ac.z), rn_mul(ab.z, ac.y));
  const float ny = rn_sub(rn_mul(ab.z, ac.x), rn_mul(ab.x, ac.z));
  const float nz = rn_sub(rn_mul(ab.x, ac.y), rn_mul(ab.y, ac.x));
  const float nn = rn_add(rn_add(rn_mul(nx, nx), rn_mul(ny, ny)), rn_mul(nz, nz));
  area[f] = 0.5f * sqrtf(nn);
}

// pass 1 (WRITE = false): tile[b] = sum of the tile's areas.  pass 3 (WRITE = true): cdf = tile scan + tile[b] (now the exclusive
// prefix of the tile sums).  Both form the same sums in the same order: lane t owns faces [4 t, 4 t + 4) of the tile.
template <bool WRITE>
__global__ __launch_bounds__(SURF_BLOCK) void surf_scan_tile_kernel(SurfBuf s, int nf) {
  __shared__ double sh[SURF_BLOCK];
  const int64_t f0 = (int64_t)blockIdx.x * SURF_TILE + (int64_t)threadIdx.x * SURF_PER_LANE;
  double v[SURF_PER_LANE], run = 0.0;
#pragma unroll
  for (int k = 0; k < SURF_PER_LANE; ++k) {
    run += f0 + k < nf ? (double)s.area[f0 + k] : 0.0;
    v[k] = run;
  }
  const double incl = block_scan_incl<double, SURF_BLOCK>(run, sh);
  if (!WRITE) {
    if (threadIdx.x == SURF_BLOCK - 1) s.tile[blockIdx.x] = incl;
    return;
  }
  // the lane's exclusive prefix is the neighbour's inclusive one (incl - run would round once more)
  const double off = s.tile[blockIdx.x] + (threadIdx.x ? sh[threadIdx.x - 1] : 0.0);
#pragma unroll
  for (int k = 0; k < SURF_PER_LANE; ++k)
    if (f0 + k < nf) s.cdf[f0 + k] = off + v[k];
}

// pass 2: one workgroup turns tile[0 .. n_tiles) into its exclusive prefix sums, 256 at a time with a running carry.
__global__ __launch_bounds__(SURF_BLOCK) void surf_scan_tiles_kernel(double* __restrict__ tile, int n_tiles) {
  __shared__ double sh[SURF_BLOCK];
  double carry = 0.0;
  for (int i0 = 0; i0 < n_tiles; i0 += SURF_BLOCK) {
    const int i = i0 + threadIdx.x;
    block_scan_incl<double, SURF_BLOCK>(i < n_tiles ? tile[i] : 0.0, sh);
    const double excl = threadIdx.x ? sh[threadIdx.x - 1] : 0.0;
    const double last = sh[SURF_BLOCK - 1];
    __syncthreads();                                     // sh is rewritten by the next round
    if (i < n_tiles) tile[i] = carry + excl;
    carry += last;
  }
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t w[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

struct SurfOut {
  float* points;     // [n][3]
  int32_t* face;     // [n], may be NULL
  float* bary;       // [n][2], may be NULL
};

// Sample i = offset + thread.  Counter (lo32(i), 0, hi32(i), 0) places the point, (lo32(i), 1, hi32(i), 0) draws its noise.
__global__ __launch_bounds__(SURF_BLOCK) void surf_sample_kernel(const float* __restrict__ V, int nv,
                                                                 const int32_t* __restrict__ F, int nf,
                                                                 const double* __restrict__ cdf, int64_t n, uint64_t offset,
                                                                 uint64_t seed, float stddev, SurfOut out) {
  const int64_t t = (int64_t)blockIdx.x * SURF_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint64_t i = offset + (uint64_t)t;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), ilo = (uint32_t)i, ihi = (uint32_t)(i >> 32);
  uint32_t w[4];
  philox4x32_10(ilo, 0u, ihi, 0u, k0, k1, w);
  const double total = cdf[nf - 1];
  const double r = __ull2double_rn(((uint64_t)w[0] << 32) | w[3]) * 5.421010862427522170037e-20;      // 2^-64
  const double x = __dmul_rn(r, total);                  // a lone product that is only compared: nothing to contract it with
  // first f with cdf[f] > x; x >= total (r rounds to 1): first f with cdf[f] >= total, the last face that added area
  const bool clamp = !(x < total);
  int lo = 0, hi = nf - 1;                               // the answer lies in [lo, hi]: cdf[nf - 1] = total satisfies both tests
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const double c = cdf[mid];
    const bool ok = clamp ? c >= total : c > x;
    hi = ok ? mid : hi;
    lo = ok ? lo : mid + 1;
  }
  float u = (float)(w[1] >> 8) * 5.9604644775390625e-8f, v = (float)(w[2] >> 8) * 5.9604644775390625e-8f;      // 2^-24
  if (__fadd_rn(u, v) > 1.f) {                           // u, v: 24-bit integers times 2^-24, exact; fusing either into the sum changes nothing
    u = 1.f - u;
    v = 1.f - v;
  }
  float3 a, ab, ac;
  surf_face(V, nv, F, lo, a, ab, ac);
  float px = fmaf(ac.x, v, fmaf(ab.x, u, a.x)), py = fmaf(ac.y, v, fmaf(ab.y, u, a.y)), pz = fmaf(ac.z, v, fmaf(ab.z, u, a.z));
  if (stddev != 0.f) {
    // Box-Muller: (g0, g1) from words 0, 1 and g2 from words 2, 3; the radius argument lies in (0, 1], so the log is finite
    uint32_t g[4];
    philox4x32_10(ilo, 1u, ihi, 0u, k0, k1, g);
    const float ua = (float)((g[0] >> 8) + 1u) * 5.9604644775390625e-8f, ub = (float)(g[1] >> 8) * 5.9604644775390625e-8f;
    const float uc = (float)((g[2] >> 8) + 1u) * 5.9604644775390625e-8f, ud = (float)(g[3] >> 8) * 5.9604644775390625e-8f;
    const float ra = sqrtf(-2.f * logf(ua)), rc = sqrtf(-2.f * logf(uc));
    const float ta = 6.283185307179586f * ub, tc = 6.283185307179586f * ud;
    px = fmaf(stddev, ra * cosf(ta), px);
    py = fmaf(stddev, ra * sinf(ta), py);
    pz = fmaf(stddev, rc * cosf(tc), pz);
  }
  out.points[t * 3] = px;
  out.points[t * 3 + 1] = py;
  out.points[t * 3 + 2] = pz;
  if (out.face) out.face[t] = lo;
  if (out.bary) {
    out.bary[t * 2] = u;
    out.bary[t * 2 + 1] = v;
  }
}

}  // namespace dsdf
