// voldiff.hpp -- d(volume mesh vertices) / d(spline control points): msdiff.hpp's derivative carried from the marching-cubes
// vertices (edge classes 1, 2, 4) to every vertex of tetmesh.hpp's mesh, the face and body diagonals (classes 3, 5, 6, 7) included
// (gfx950).  The reference differentiates its tetgen mesh only through the surface (analysis/geometry.py get_dTheta :176-197).
//
// Vertex v = vert_index[i] of the compacted list of moving vertices is (p, c) = (vert_point[v], vert_class[v]) of dsdf_tet_emit:
// direction d = (c & 1, (c >> 1) & 1, (c >> 2) & 1), q = p + sum_b d[b] * stride[b], capped values s0 = grid[p], s1 = grid[q].
//   t = (level - s0) / (s1 - s0) in tet_vertex_kernel's sequence; with t_clamp = tau > 0 the vertex moves iff tau <= t <= 1 - tau
//   (1 - tau rounded to fp32): otherwise the clamp holds it and its derivative is exactly zero.  tau = 0 zeroes nothing.
//   dt/ds0, dt/ds1: msd_dt, the surface's.  Every coordinate b with d[b] = 1 moves by the same t:
//   d verts[v, b] / d cp[k, l] = d[b] * scale[b] * sum_e dt/ds_e * m_e * G_e[l] * B_k(xo_e),   scale = voxel_size / 2
// The band (MsdBand) is the volume mesh's own: an endpoint of a crossing diagonal need not lie on a crossing axis edge.
//
// This file holds what the volume mesh decides for itself: vd_vertex's rule for which list entries move (list entry, class, point,
// the far endpoint per axis against the grid's size, the clamp) and the scalar in front of each endpoint.  Everything behind that --
// the endpoint record, msd_ends, the index walk, the control-point split, the first stage of the adjoint -- is msdiff.hpp's, once.
//
//   vd_jvp_kernel       one wave per moving vertex (msd_jvp_kernel's form): msd_end_dot over the lanes, the fixed xor-shuffle tree,
//                       then per flagged coordinate b  fma(scale[b] * dt1, dot1, fma(scale[b] * dt0, dot0, 0)): a class-1/2/4
//                       vertex has msd_jvp_kernel's bits.  The entry zeroes d_verts first; rows off the list stay zero.
//   vd_vjp_part_kernel  msd_vjp_part over the list (workgroup (part, tile), MSD_VJP_VERTS list entries in order, LDS tile of
//                       MSD_VJP_TILE floats, a barrier per endpoint, no atomics) with the volume's factor: the scalar of a vertex is
//                       gs = sum over flagged b, increasing, of scale[b] * grad[v, b] (each product and sum rounded on its own);
//                       endpoint e adds fma(gs * dt_e, w * G[l], acc).  msd_vjp_sum_kernel adds the parts in part order.
//   vd_dtheta_kernel    the dense normal-projected derivative of the moving vertices (include/dsdf.h states the sequence).
// A list entry, class, point, far endpoint, band row or base out of range contributes nothing; nothing is read out of bounds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.hpp"
#include "msdiff.hpp"

namespace dsdf {

constexpr int VD_DENSE_VERTS = 64;     // list entries one workgroup of the dense kernel takes at most
constexpr int VD_DENSE_COLS = 2048;    // columns it aims at when a vertex's row is shorter: eight per lane

struct VdMesh {
  const float* grid;                   // capped sdf [npts]
  const int64_t* vert_point;           // [V]
  const int32_t* vert_class;           // [V]
  const int32_t* vert_index;           // [Vm] ids of the moving vertices
  const int32_t* band_of;              // [npts]
  int64_t npts, stride[3], V, Vm;
  int dims[3];
  float scale[3];
  float level, t_clamp;
};

// Vertex id (-1: list entry out of range), class (0: the vertex does not move) and the two endpoints, coef = dt/ds_k, of list
// entry i: the same for every lane of a workgroup / wave that shares i.
__device__ __forceinline__ int vd_vertex(const VdMesh& M, const MsdBand& B, int64_t i, MsdEnd e[2], int64_t* vid) {
  msd_no_ends(e);
  const int64_t v = M.vert_index[i];
  *vid = v >= 0 && v < M.V ? v : -1;
  if (*vid < 0) return 0;
  const int c = M.vert_class[v];
  const int64_t p = M.vert_point[v];
  if (c < 1 || c > 7 || p < 0 || p >= M.npts) return 0;
  const uint32_t pu = (uint32_t)p, syz = (uint32_t)M.stride[0], sz = (uint32_t)M.stride[1];      // npts <= 2^30
  const uint32_t ix = pu / syz, rem = pu - ix * syz, iy = rem / sz, iz = rem - iy * sz;
  const int idx[3] = {(int)ix, (int)iy, (int)iz};
  int64_t q = p;
  for (int b = 0; b < 3; ++b) {
    if (!((c >> b) & 1)) continue;
    if (idx[b] + 1 >= M.dims[b]) return 0;                   // the far endpoint lies past the grid
    q += M.stride[b];
  }
  const float s0 = M.grid[p], s1 = M.grid[q];
  if (M.t_clamp > 0.f) {
    const float t = rn_div(rn_sub(M.level, s0), rn_sub(s1, s0));
    if (!(t >= M.t_clamp && t <= rn_sub(1.f, M.t_clamp))) return 0;      // held by the clamp
  }
  float dt[2];
  msd_dt(M.level, s0, s1, dt);
  const int64_t g[2] = {p, q};
  msd_ends(B, M.band_of, g, dt, e);
  return c;
}

__global__ __launch_bounds__(MSD_BLOCK) void vd_jvp_kernel(VdMesh M, MsdBand B, const float* __restrict__ d_cp,
                                                           float* __restrict__ d_verts) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (MSD_BLOCK / 64) + (threadIdx.x >> 6);
  if (i >= M.Vm) return;                                     // (no barrier below)
  MsdEnd e[2];
  int64_t v;
  const int c = vd_vertex(M, B, i, e, &v);
  if (v < 0) return;
  float dot[2] = {0.f, 0.f};
  for (int k = 0; k < 2; ++k) {
    if (e[k].row < 0) continue;                              // wave-uniform
    float acc = msd_end_dot(B, e[k], d_cp, lane, 64);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    dot[k] = acc;
  }
  if (lane < 3) {
    float tot = 0.f;
    for (int k = 0; k < 2; ++k)
      if (e[k].row >= 0) tot = fmaf(rn_mul(M.scale[lane], e[k].coef), dot[k], tot);
    d_verts[v * 3 + lane] = ((c >> lane) & 1) ? tot : 0.f;
  }
}

// The volume's part of msd_vjp_part: its list is the moving vertices, and endpoint k of entry i adds f = rn(gs * dt/ds_k) times
// the walk's products, gs = sum over flagged b, increasing, of rn(scale[b] * grad_verts[v, b]).  An entry that does not move has
// class 0 and no endpoint: nothing of grad_verts is read for it.
__device__ __forceinline__ int64_t msd_vjp_count(const VdMesh& M) { return M.Vm; }

__device__ __forceinline__ void msd_vjp_ends(const VdMesh& M, const MsdBand& B, int64_t i, const float* __restrict__ grad_verts,
                                             MsdEnd e[2]) {
  int64_t v;
  const int c = vd_vertex(M, B, i, e, &v);
  float gs = 0.f;
  for (int b = 0; b < 3; ++b)
    if ((c >> b) & 1) gs = rn_add(gs, rn_mul(M.scale[b], grad_verts[v * 3 + b]));
  for (int k = 0; k < 2; ++k) e[k].coef = rn_mul(gs, e[k].coef);
}

__global__ __launch_bounds__(MSD_BLOCK) void vd_vjp_part_kernel(VdMesh M, MsdBand B, const float* __restrict__ grad_verts,
                                                                float* __restrict__ part) {
  msd_vjp_part(M, B, grad_verts, part);
}

struct VdProject { float stretch[3]; float clip; };

// vpw list entries per workgroup (host: 1 unless a row of R columns is short).  Phase 1, one lane per entry: class, endpoints and
// normal, left in LDS.  Phase 2: lane t takes column t % R of entry t / R and writes its three planes; consecutive lanes write
// consecutive columns of one plane.
__global__ __launch_bounds__(MSD_BLOCK) void vd_dtheta_kernel(VdMesh M, MsdBand B, const float* __restrict__ normals, VdProject P,
                                                              float* __restrict__ out, int vpw) {
  __shared__ MsdEnd end_s[VD_DENSE_VERTS][2];
  __shared__ int class_s[VD_DENSE_VERTS];
  __shared__ float n_s[VD_DENSE_VERTS][4];                   // the normal and n . n (0: the row is zero)
  const int tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * vpw;
  const int nv = (int)((M.Vm - i0) < (int64_t)vpw ? (M.Vm - i0) : (int64_t)vpw);
  if (tid < nv) {
    MsdEnd e[2];
    int64_t v;
    const int c = vd_vertex(M, B, i0 + tid, e, &v);
    end_s[tid][0] = e[0];
    end_s[tid][1] = e[1];
    class_s[tid] = c;
    float n[3] = {0.f, 0.f, 0.f};
    if (v >= 0) for (int b = 0; b < 3; ++b) n[b] = normals[v * 3 + b];
    n_s[tid][0] = n[0]; n_s[tid][1] = n[1]; n_s[tid][2] = n[2];
    n_s[tid][3] = rn_add(rn_add(rn_mul(n[0], n[0]), rn_mul(n[1], n[1])), rn_mul(n[2], n[2]));
  }
  __syncthreads();
  const uint32_t R = (uint32_t)B.ncp_total * (uint32_t)B.L, L = (uint32_t)B.L;
  const uint32_t total = (uint32_t)nv * R;                   // vpw * R <= max(R, VD_DENSE_COLS)
  for (uint32_t t = tid; t < total; t += MSD_BLOCK) {
    const uint32_t vl = t / R, r = t - vl * R;
    const uint32_t cpi = r / L, l = r - cpi * L;
    int ci[3];
    msd_split(B, cpi, ci);
    const int c = class_s[vl];
    float T = 0.f;
    for (int k = 0; k < 2; ++k) {
      const MsdEnd& e = end_s[vl][k];
      if (e.row < 0) continue;
      const int s = msd_slot(B, e, ci);
      if (s < 0) continue;
      T = rn_add(T, rn_mul(rn_mul(e.coef, B.w[e.row * MS_WEIGHTS + s]), B.G[e.row * B.ldg + l]));
    }
    const float nn = n_s[vl][3];
    float nj = 0.f;
    for (int b = 0; b < 3; ++b) {
      float j = ((c >> b) & 1) ? rn_mul(rn_mul(P.stretch[b], M.scale[b]), T) : 0.f;
      if (P.clip > 0.f && fabsf(j) > P.clip) j = 0.f;
      nj = rn_add(nj, rn_mul(n_s[vl][b], j));
    }
    const bool zero = nn == 0.f || c == 0;                   // a zero normal, a vertex that does not move: +0
    const float s = zero ? 0.f : rn_div(nj, nn);
    float* __restrict__ o = out + ((i0 + vl) * 3) * (int64_t)R + r;
    for (int b = 0; b < 3; ++b) o[(int64_t)b * R] = zero ? 0.f : rn_mul(n_s[vl][b], s);
  }
}

}  // namespace dsdf
