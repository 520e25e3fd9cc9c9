// meshtopo.hpp -- the surface stage of the reference's analysis/geometry.py DeepSDFMesh (trimesh on the CPU: face adjacency,
// connected components, watertightness, degenerate faces, vertex normals; the volume constraint and the normal-projected shape
// derivative of optimization/) on the device (gfx950).  Sorting stays with the caller: every kernel here takes sorted arrays.
//
//   mt_edge_keys_kernel    half-edge h = 3 f + k runs F[f][k] -> F[f][(k + 1) % 3]; key = (min << 32) | max, -1 when both ends are equal
//   mt_adjacency_kernel    a stencil over positions i - 2 .. i + 2 of the sorted keys: a key >= 0 that occurs exactly twice pairs its two
//                          half-edges (trimesh's face_adjacency rule: an edge of 1 or of more than 2 faces joins nothing); six integer
//                          counts per workgroup, summed by mt_stats_sum_kernel in workgroup order
//   mt_cc_*                connected components of the faces under the mate relation: the init and hook kernels of components.hpp's
//                          scheme (min-hooking with shortcutting; its int32 atomicMin / atomicAdd are the ONLY atomics this file uses)
//   mt_degenerate_kernel   the zero-area rule of meshsdf.hpp's prepare pass (|ab x ac|^2 <= 1e-14 (longest edge)^4, fp64 on the fp32
//                          vertices), restated: sharing the function would change that kernel's code object
//   mt_vertex_kernel       one lane per vertex gathers its corners (sorted by vertex: a fixed order, no atomics), fp64 throughout:
//                          the angle-weighted normal (current trimesh's vertex_normals) and d volume / d vertex = (1/6) sum b x c
//   mt_volume_*            (1/6) sum_f a . (b x c) in fp64: per-workgroup sums over contiguous slices, then one workgroup (dsdf_mean_f64's shape)
//   mt_project_kernel      out[v][d][r] = ((jac[v][r] * stretch[a]) clipped * n[a]) * n[d]: a streaming writer of three times the
//                          Jacobian's bytes; a lane reads VEC columns once and stores them to the three planes, coalesced
// Every index read from a caller's array is clamped before it is used as an address (as msdf_prepare_kernel does): a badly sorted
// or out-of-range array gives an unspecified result and no access outside the arrays.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blockops.hpp"
#include "components.hpp"

namespace dsdf {

constexpr int MT_BLOCK = 256;            // lanes per workgroup of every kernel of this file
constexpr int MT_VOL_MAX_BLOCKS = 1024;  // partial sums of the volume
constexpr int MT_VOL_MIN_SLICE = 4096;   // faces per workgroup before a second workgroup is started
constexpr int MT_STATS = 6;              // distinct, boundary, non-manifold, paired, paired same-direction, key -1
constexpr int MT_STAT_BITS = 10;         // of a workgroup's count of one of them
static_assert(MT_BLOCK < (1 << MT_STAT_BITS) && MT_STATS * MT_STAT_BITS < 64, "six counts share one summed int64");

__device__ __forceinline__ int mt_clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__global__ __launch_bounds__(MT_BLOCK) void mt_edge_keys_kernel(const int32_t* __restrict__ F, int64_t n_half, int nv,
                                                                int64_t* __restrict__ keys) {
  const int64_t h = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (h >= n_half) return;
  const int64_t f = h / 3;
  const int k = (int)(h - f * 3);
  const int a = mt_clampi(F[f * 3 + k], nv), b = mt_clampi(F[f * 3 + (k + 1) % 3], nv);
  keys[h] = a == b ? (int64_t)-1 : (((int64_t)(a < b ? a : b) << 32) | (int64_t)(a < b ? b : a));
}

// 1 if half-edge h runs from its lower to its higher vertex index
__device__ __forceinline__ int mt_ascending(const int32_t* __restrict__ F, int64_t h) {
  const int64_t f = h / 3;
  const int k = (int)(h - f * 3);
  return F[f * 3 + k] < F[f * 3 + (k + 1) % 3];
}

__global__ __launch_bounds__(MT_BLOCK) void mt_adjacency_kernel(const int32_t* __restrict__ F, int64_t n_half,
                                                                const int64_t* __restrict__ keys, const int64_t* __restrict__ order,
                                                                int32_t* __restrict__ mate, int64_t* __restrict__ part) {
  __shared__ int64_t sh[MT_BLOCK];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * MT_BLOCK + t;
  int c[MT_STATS] = {0, 0, 0, 0, 0, 0};
  if (i < n_half) {
    const int64_t k = keys[i];
    const bool p1 = i >= 1 && keys[i - 1] == k, p2 = i >= 2 && keys[i - 2] == k;
    const bool n1 = i + 1 < n_half && keys[i + 1] == k, n2 = i + 2 < n_half && keys[i + 2] == k;
    const int64_t h = clamp_index(order[i], n_half);
    int64_t other = -1;
    if (k >= 0) {
      if (p1 && !p2 && !n1) other = i - 1;                    // the second of a run of exactly two
      else if (n1 && !p1 && !n2) other = i + 1;               // the first of one
    }
    const int64_t ho = other >= 0 ? clamp_index(order[other], n_half) : -1;
    mate[h] = (int32_t)ho;
    if (k < 0) c[5] = 1;
    else if (!p1) {                                           // the first position of its run counts the edge
      c[0] = 1;
      if (!n1) c[1] = 1;
      else if (n2) c[2] = 1;
      else {
        c[3] = 1;
        c[4] = mt_ascending(F, h) == mt_ascending(F, ho);
      }
    }
  }
  // the six counts, each at most MT_BLOCK, ride in one sum: MT_STAT_BITS bits apiece
  int64_t packed = 0;
  for (int s = 0; s < MT_STATS; ++s) packed |= (int64_t)c[s] << (MT_STAT_BITS * s);
  const int64_t tot = block_tree_sum<int64_t, MT_BLOCK>(packed, sh);
  if (t < MT_STATS) part[(int64_t)blockIdx.x * MT_STATS + t] = (tot >> (MT_STAT_BITS * t)) & ((1 << MT_STAT_BITS) - 1);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_stats_sum_kernel(const int64_t* __restrict__ part, int64_t n_part,
                                                                int64_t* __restrict__ stats) {
  __shared__ int64_t sh[MT_BLOCK];
  const int t = threadIdx.x;
  for (int s = 0; s < MT_STATS; ++s) {
    int64_t a = 0;
    for (int64_t b = t; b < n_part; b += MT_BLOCK) a += part[b * MT_STATS + s];
    const int64_t tot = block_tree_sum<int64_t, MT_BLOCK>(a, sh);
    if (t == 0) stats[s] = tot;
    __syncthreads();
  }
}

// ---- components ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT_BLOCK) void mt_cc_init_kernel(int32_t* __restrict__ f, int nf) {
  const int64_t u = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (u < nf) f[u] = (int32_t)u;
}

// *flag != 0 afterwards: some f went down.
__global__ __launch_bounds__(MT_BLOCK) void mt_cc_hook_kernel(const int32_t* __restrict__ mate, int nf, int32_t* f,
                                                              const int32_t* __restrict__ gf, int32_t* __restrict__ flag) {
  const int64_t u = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (u >= nf) return;
  bool changed = false;
  const int fu = mt_clampi(f[u], nf);
  int best = gf[u];                                            // the shortcut f[u] <- min(f[u], gf[u]) rides along
  for (int k = 0; k < 3; ++k) {
    const int m = mate[u * 3 + k];
    if (m < 0) continue;
    const int g = gf[mt_clampi(m / 3, nf)];
    changed |= cc_lower(f, fu, g);
    best = g < best ? g : best;
  }
  changed |= cc_lower(f, u, best);
  if (changed) *flag = 1;
}

// ---- geometry -----------------------------------------------------------------------------------------------------------------
struct MtTri { double a[3], b[3], c[3]; };

// the face's vertices starting at corner k, in cyclic order
__device__ __forceinline__ MtTri mt_face(const float* __restrict__ V, int nv, const int32_t* __restrict__ F, int64_t f, int k) {
  MtTri t;
  const int ia = mt_clampi(F[f * 3 + k], nv), ib = mt_clampi(F[f * 3 + (k + 1) % 3], nv), ic = mt_clampi(F[f * 3 + (k + 2) % 3], nv);
  for (int x = 0; x < 3; ++x) {
    t.a[x] = (double)V[(int64_t)ia * 3 + x];
    t.b[x] = (double)V[(int64_t)ib * 3 + x];
    t.c[x] = (double)V[(int64_t)ic * 3 + x];
  }
  return t;
}

__device__ __forceinline__ void mt_cross(const double* p, const double* q, double* n) {
  n[0] = p[1] * q[2] - p[2] * q[1];
  n[1] = p[2] * q[0] - p[0] * q[2];
  n[2] = p[0] * q[1] - p[1] * q[0];
}

__device__ __forceinline__ double mt_dot(const double* p, const double* q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; }

// e1 = b - a, e2 = c - a, n = e1 x e2, nn = n . n; true for a zero-area face
__device__ __forceinline__ bool mt_zero_area(const MtTri& t, double* e1, double* e2, double* n, double* nn) {
  double g[3];
  for (int x = 0; x < 3; ++x) { e1[x] = t.b[x] - t.a[x]; e2[x] = t.c[x] - t.a[x]; g[x] = t.c[x] - t.b[x]; }
  mt_cross(e1, e2, n);
  *nn = mt_dot(n, n);
  const double lmax = fmax(mt_dot(e1, e1), fmax(mt_dot(e2, e2), mt_dot(g, g)));
  return *nn <= 1e-14 * lmax * lmax;
}

__global__ __launch_bounds__(MT_BLOCK) void mt_degenerate_kernel(const float* __restrict__ V, int nv, const int32_t* __restrict__ F,
                                                                 int nf, uint8_t* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (f >= nf) return;
  const int i0 = F[f * 3], i1 = F[f * 3 + 1], i2 = F[f * 3 + 2];
  double e1[3], e2[3], n[3], nn;
  const bool zero = mt_zero_area(mt_face(V, nv, F, f, 0), e1, e2, n, &nn);
  out[f] = (uint8_t)(i0 == i1 || i1 == i2 || i2 == i0 || zero);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_vertex_kernel(const float* __restrict__ V, int nv, const int32_t* __restrict__ F,
                                                             int64_t n_half, const int64_t* __restrict__ corner_order,
                                                             const int64_t* __restrict__ vstart, float* __restrict__ normals,
                                                             float* __restrict__ vol_grad) {
  const int64_t v = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (v >= nv) return;
  int64_t lo = vstart[v], hi = vstart[v + 1];
  lo = lo < 0 ? 0 : (lo > n_half ? n_half : lo);
  hi = hi < lo ? lo : (hi > n_half ? n_half : hi);
  double s[3] = {0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t c = clamp_index(corner_order[i], n_half);
    const int64_t f = c / 3;
    const MtTri t = mt_face(V, nv, F, f, (int)(c - f * 3));
    double bc[3];
    mt_cross(t.b, t.c, bc);
    for (int x = 0; x < 3; ++x) g[x] += bc[x];
    double e1[3], e2[3], n[3], nn;
    if (mt_zero_area(t, e1, e2, n, &nn)) continue;
    const double ln = sqrt(nn);
    const double w = atan2(ln, mt_dot(e1, e2)) / ln;
    for (int x = 0; x < 3; ++x) s[x] += w * n[x];
  }
  if (normals) {
    const double ls = sqrt(mt_dot(s, s));
    for (int x = 0; x < 3; ++x) normals[v * 3 + x] = ls > 0.0 ? (float)(s[x] / ls) : 0.f;
  }
  if (vol_grad)
    for (int x = 0; x < 3; ++x) vol_grad[v * 3 + x] = (float)(g[x] / 6.0);
}

__global__ __launch_bounds__(MT_BLOCK) void mt_volume_part_kernel(const float* __restrict__ V, int nv, const int32_t* __restrict__ F,
                                                                  int64_t nf, int64_t slice, double* __restrict__ part) {
  __shared__ double sh[MT_BLOCK];
  const int64_t f0 = (int64_t)blockIdx.x * slice;
  const int64_t f1 = f0 + slice < nf ? f0 + slice : nf;
  double s = 0.0;
  for (int64_t f = f0 + threadIdx.x; f < f1; f += MT_BLOCK) {
    const MtTri t = mt_face(V, nv, F, f, 0);
    double bc[3];
    mt_cross(t.b, t.c, bc);
    s += mt_dot(t.a, bc);
  }
  const double tot = block_tree_sum<double, MT_BLOCK>(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(MT_BLOCK) void mt_volume_final_kernel(const double* __restrict__ part, int n_part, double* __restrict__ volume) {
  __shared__ double sh[MT_BLOCK];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += MT_BLOCK) s += part[i];
  const double tot = block_tree_sum<double, MT_BLOCK>(s, sh);
  if (threadIdx.x == 0) volume[0] = tot / 6.0;
}

// ---- projection ---------------------------------------------------------------------------------------------------------------
struct MtStretch { float s[3]; };

// Lane t takes columns [q * VEC, q * VEC + VEC) of vertex v = t / Rq: one read of the Jacobian, one store per plane.  Consecutive
// lanes take consecutive columns, so each of the three stores of a wave covers contiguous bytes of one plane (of a few vertices when
// R is short).  Products only, each rounded on its own: nothing here can be contracted.
template <int VEC>
__global__ __launch_bounds__(MT_BLOCK) void mt_project_kernel(const float* __restrict__ jac, const int32_t* __restrict__ axis,
                                                              const float* __restrict__ normals, int64_t total, int64_t Rq,
                                                              MtStretch st, float clip, float* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * MT_BLOCK + threadIdx.x;
  if (t >= total) return;
  const int64_t v = t / Rq, q = t - v * Rq, R = Rq * VEC;
  const int a = mt_clampi(axis[v], 3);
  const float n[3] = {normals[v * 3], normals[v * 3 + 1], normals[v * 3 + 2]};
  float j[VEC];
  if constexpr (VEC == 4) {
    const float4 x = *reinterpret_cast<const float4*>(jac + v * R + q * 4);
    j[0] = x.x; j[1] = x.y; j[2] = x.z; j[3] = x.w;
  } else {
    j[0] = jac[v * R + q];
  }
  for (int x = 0; x < VEC; ++x) {
    j[x] = __fmul_rn(j[x], st.s[a]);
    if (clip > 0.f && fabsf(j[x]) > clip) j[x] = 0.f;
    j[x] = __fmul_rn(j[x], n[a]);
  }
  for (int d = 0; d < 3; ++d) {
    float* __restrict__ o = out + (v * 3 + d) * R + q * VEC;
    if constexpr (VEC == 4)
      *reinterpret_cast<float4*>(o) = make_float4(__fmul_rn(j[0], n[d]), __fmul_rn(j[1], n[d]), __fmul_rn(j[2], n[d]), __fmul_rn(j[3], n[d]));
    else
      o[0] = __fmul_rn(j[0], n[d]);
  }
}

}  // namespace dsdf
