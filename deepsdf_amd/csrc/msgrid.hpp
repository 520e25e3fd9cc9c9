// msgrid.hpp -- the two ends of microstructure meshing (the reference's deep_sdf/mesh.py create_mesh_microstructure :226-295 and
// analysis/geometry.py sdf_struct) on the device (gfx950): the decoder's input rows in front of the decode, the caps behind it.
//
//   ms_rows_kernel   rows [n][L + 3] = [spline latent at xo | folded xyz] for points [start, start + n) of the padded grid (linear
//                    index, z fastest) or for an explicit point list.
//                    xo      = (fp32 index * voxel_size) + voxel_origin: one rounded multiply, one rounded add, never an FMA
//                    folded  = (2/p) * |((xo - t%2) mod 2p) - p| - 1, mod = fmodf + the sign fix of a floored remainder, every
//                              operation rounded on its own in the reference's order; the constants come rounded from double
//                    inside  = -1 <= xo <= 1 on the three axes; outside rows carry exact zeros in the latent columns
//                    latent  = tensor-product B-spline (degree 1..3 per axis, clamped non-decreasing knots, control points
//                              [ncp][L], first parametric axis fastest), basis by Cox-de Boor in fp32
//                    A workgroup takes MS_TILE consecutive points.  Phase 1 (one lane per point): coordinates, span, the
//                    (px+1)(py+1)(pz+1) weights and the first control-point index, left in LDS.  Phase 2 (all lanes): the tile's
//                    rows are ONE contiguous run of MS_TILE * (L + 3) floats; lane e writes element e, so stores are
//                    coalesced for every L, and for L >= 64 a wave reads 64 consecutive floats of one control point per term.
//                    A lane steps from element to element without a division; with degree 1 on every axis (the reference's
//                    default) the eight control-point loads of an element are issued together (template LIN).
//                    The span search reads the knots with a wave-uniform index (scalar loads).
//   ms_caps_kernel   in place on the SDF of grid points [start, start + n): the ordered cap records (max or min against a plane
//                    at m * (1 - measure)), then the six planes of the unit cube with max.  xo is recomputed from the index.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"

namespace dsdf {

constexpr int MS_BLOCK = 256;
constexpr int MS_TILE = 64;          // points per workgroup: one lane of the first wave each in phase 1
constexpr int MS_MAX_DEG = 3;
constexpr int MS_WEIGHTS = (MS_MAX_DEG + 1) * (MS_MAX_DEG + 1) * (MS_MAX_DEG + 1);
constexpr int MS_WSTRIDE = MS_WEIGHTS + 1;   // odd stride: lanes of one wave that sit on different points hit different banks
constexpr int MS_MAX_CAPS = 6;

struct MsGrid {
  int n[3];                          // padded grid
  float vs[3], org[3];               // voxel size and origin
  float sub[3], mod[3], p[3], scale[3];   // fold: t % 2, 2p, p, 2/p
};

struct MsSpline {
  int deg[3], ncp[3], koff[3];       // knots of axis a start at knots[koff[a]], ncp[a] + deg[a] + 1 of them
  const float* knots;
  const float* cp;                   // [ncp0 * ncp1 * ncp2][L]
  int L;
};

struct MsCapRec { int dim, cap; float m, c; };     // c = m * (1 - measure)
struct MsCaps { int n; MsCapRec r[MS_MAX_CAPS]; };

// The coordinate arithmetic goes through the single rounded operations of common.hpp (rn_mul, rn_add, rn_sub): never an FMA.
__device__ __forceinline__ float ms_xo(int i, float vs, float org) { return rn_add(rn_mul((float)i, vs), org); }

__device__ __forceinline__ float ms_fold(float x, float sub, float mod, float p, float scale) {
  float r = fmodf(rn_sub(x, sub), mod);
  if (r != 0.f && r < 0.f) r = rn_add(r, mod);          // floored remainder, mod > 0
  return rn_sub(rn_mul(scale, fabsf(rn_sub(r, p))), 1.f);
}

__device__ __forceinline__ void ms_index(int64_t idx, const MsGrid& g, int& i, int& j, int& k) {
  const int64_t syz = (int64_t)g.n[1] * g.n[2];
  i = (int)(idx / syz);
  const int r = (int)(idx - (int64_t)i * syz);
  j = r / g.n[2];
  k = r - j * g.n[2];
}

// Span and basis of one axis.  u is clamped to the knot range; the span is the last non-empty one whose left knot is <= u, so the
// right end of the range evaluates to the end value.  N[0..p] are the basis functions of control points span - p .. span.
__device__ __forceinline__ int ms_basis(const float* __restrict__ U, int p, int ncp, float u, float* N) {
  u = fminf(fmaxf(u, U[p]), U[ncp]);
  int span = p;
  for (int s = p + 1; s < ncp; ++s)                          // s is wave-uniform: the knots come through the scalar cache
    if (U[s] <= u && U[s] < U[s + 1]) span = s;
  float left[MS_MAX_DEG + 1], right[MS_MAX_DEG + 1];
  N[0] = 1.f;
#pragma unroll
  for (int j = 1; j <= MS_MAX_DEG; ++j) {
    if (j <= p) {
      left[j] = u - U[span + 1 - j];
      right[j] = U[span + j] - u;
      float saved = 0.f;
#pragma unroll
      for (int r = 0; r < j; ++r) {
        const float t = N[r] / (right[r + 1] + left[j - r]);
        N[r] = saved + right[r + 1] * t;
        saved = left[j - r] * t;
      }
      N[j] = saved;
    }
  }
  return span;
}

// AT (dsdf_ms_rows_at): the tile's points are the padded-grid indices at[t0 ..], in any order -- the coordinate arithmetic is that of
// grid mode -- and phase 1's weights (w_out [n][MS_WEIGHTS], slot (k * 4 + j) * 4 + i, unused slots zero) and first control-point
// index (base_out [n], -1: outside) are written too.  An index outside [0, npts) gives a zero row, zero weights and base -1.
template <bool LIN, bool AT = false>
__global__ __launch_bounds__(MS_BLOCK) void ms_rows_kernel(MsGrid g, MsSpline s, int64_t start, int64_t n,
                                                           const float* __restrict__ pts, int inside_test, int with_xyz,
                                                           float* __restrict__ rows, const int64_t* __restrict__ at = nullptr,
                                                           int64_t npts = 0, float* __restrict__ w_out = nullptr,
                                                           int32_t* __restrict__ base_out = nullptr) {
  __shared__ float w_s[MS_TILE * MS_WSTRIDE];
  __shared__ float xyz_s[MS_TILE][3];
  __shared__ int base_s[MS_TILE];                            // first control point of the row, -1: outside (zeros)
  const int tid = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * MS_TILE;
  const int npt = (int)((n - t0) < (int64_t)MS_TILE ? (n - t0) : (int64_t)MS_TILE);
  if (tid < npt) {
    float xo[3];
    bool valid = true;
    if (AT) {
      int64_t gi = at[t0 + tid];
      valid = gi >= 0 && gi < npts;
      if (!valid) gi = 0;
      int ijk[3];
      ms_index(gi, g, ijk[0], ijk[1], ijk[2]);
      for (int a = 0; a < 3; ++a) xo[a] = ms_xo(ijk[a], g.vs[a], g.org[a]);
    } else if (pts) {
      for (int a = 0; a < 3; ++a) xo[a] = pts[(t0 + tid) * 3 + a];
    } else {
      int ijk[3];
      ms_index(start + t0 + tid, g, ijk[0], ijk[1], ijk[2]);
      for (int a = 0; a < 3; ++a) xo[a] = ms_xo(ijk[a], g.vs[a], g.org[a]);
    }
    bool inside = valid;
    for (int a = 0; a < 3; ++a) {
      xyz_s[tid][a] = valid ? ms_fold(xo[a], g.sub[a], g.mod[a], g.p[a], g.scale[a]) : 0.f;
      inside = inside && xo[a] >= -1.f && xo[a] <= 1.f;
    }
    int base = -1;
    if (inside || !inside_test) {
      float N[3][MS_MAX_DEG + 1];
      int first[3];
      for (int a = 0; a < 3; ++a) first[a] = ms_basis(s.knots + s.koff[a], s.deg[a], s.ncp[a], xo[a], N[a]) - s.deg[a];
      base = first[0] + s.ncp[0] * (first[1] + s.ncp[1] * first[2]);
      float* w = w_s + tid * MS_WSTRIDE;
#pragma unroll
      for (int k = 0; k <= MS_MAX_DEG; ++k)
#pragma unroll
        for (int j = 0; j <= MS_MAX_DEG; ++j)
#pragma unroll
          for (int i = 0; i <= MS_MAX_DEG; ++i)              // unrolled with guards: N stays in registers
            if (k <= s.deg[2] && j <= s.deg[1] && i <= s.deg[0]) w[(k * 4 + j) * 4 + i] = (N[0][i] * N[1][j]) * N[2][k];
    }
    base_s[tid] = base;
  }
  __syncthreads();
  if (AT) {
    if (base_out && tid < npt) base_out[t0 + tid] = base_s[tid];
    if (w_out) {
      for (int e = tid; e < npt * MS_WEIGHTS; e += MS_BLOCK) {   // coalesced: the tile's weights are one contiguous run
        const int pt = e / MS_WEIGHTS, sl = e % MS_WEIGHTS;
        const bool used = base_s[pt] >= 0 && (sl & 3) <= s.deg[0] && ((sl >> 2) & 3) <= s.deg[1] && (sl >> 4) <= s.deg[2];
        w_out[t0 * MS_WEIGHTS + e] = used ? w_s[pt * MS_WSTRIDE + sl] : 0.f;
      }
    }
  }
  const int L = s.L, W = L + (with_xyz ? 3 : 0);
  const int total = npt * W;
  float* __restrict__ out = rows + t0 * W;
  const int sj = s.ncp[0] * L, sk = s.ncp[0] * s.ncp[1] * L;
  // element e = pt * W + c; the next one of this lane is MS_BLOCK further: (pt, c) advance by a quotient and a remainder that are
  // the same for every lane, so the loop has no division
  const int dq = MS_BLOCK / W, dr = MS_BLOCK - dq * W;
  int pt = tid / W, c = tid - pt * W;
  for (int e = tid; e < total; e += MS_BLOCK) {
    float v = 0.f;
    if (c >= L) {
      v = xyz_s[pt][c - L];
    } else {
      const int b = base_s[pt];
      if (b >= 0) {
        const float* __restrict__ cp = s.cp + (int64_t)b * L + c;
        const float* w = w_s + pt * MS_WSTRIDE;
        if (LIN) {                                           // degree 1 on every axis: eight independent loads in flight
          float q[8];
#pragma unroll
          for (int t = 0; t < 8; ++t) q[t] = cp[(t >> 2) * sk + ((t >> 1) & 1) * sj + (t & 1) * L];
#pragma unroll
          for (int t = 0; t < 8; ++t) v = fmaf(w[((t >> 2) * 4 + ((t >> 1) & 1)) * 4 + (t & 1)], q[t], v);
        } else {
          for (int k = 0; k <= s.deg[2]; ++k)
            for (int j = 0; j <= s.deg[1]; ++j)
              for (int i = 0; i <= s.deg[0]; ++i) v = fmaf(w[(k * 4 + j) * 4 + i], cp[k * sk + j * sj + i * L], v);
        }
      }
    }
    out[e] = v;
    pt += dq;
    c += dr;
    if (c >= W) { c -= W; ++pt; }
  }
}

__global__ __launch_bounds__(MS_BLOCK) void ms_caps_kernel(MsGrid g, MsCaps caps, int64_t start, int64_t n, float* __restrict__ sdf) {
  const int64_t q = (int64_t)blockIdx.x * MS_BLOCK + threadIdx.x;
  if (q >= n) return;
  int ijk[3];
  ms_index(start + q, g, ijk[0], ijk[1], ijk[2]);
  float xo[3];
  for (int a = 0; a < 3; ++a) xo[a] = ms_xo(ijk[a], g.vs[a], g.org[a]);
  float v = sdf[q];
  for (int r = 0; r < caps.n; ++r) {
    const MsCapRec R = caps.r[r];
    const float x = R.dim == 0 ? xo[0] : (R.dim == 1 ? xo[1] : xo[2]);
    const float border = rn_mul(rn_sub(x, R.c), -R.m);
    if (R.cap < 0) { const float nb = -border; v = nb > v ? nb : v; }     // a NaN sdf stays, as with numpy's maximum
    else v = border < v ? border : v;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float lo = -rn_mul(rn_sub(xo[a], -1.f), 1.f);
    v = lo > v ? lo : v;
    const float hi = -rn_mul(rn_sub(xo[a], 1.f), -1.f);
    v = hi > v ? hi : v;
  }
  sdf[q] = v;
}

}  // namespace dsdf
