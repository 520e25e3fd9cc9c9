// msdiff.hpp -- d(mesh vertices) / d(spline control points) of a microstructure mesh (the reference's deep_sdf/mesh.py
// create_mesh_microstructure_diff :346-454, which runs latent_dim x n_control_points double-backward passes over the whole grid) on
// the device (gfx950), assembled in closed form from marching cubes' own interpolation.
//
// Vertex v sits on grid edge (p, a) between p and q = p + e_a with capped values s0, s1; only its coordinate a moves:
//   t = (level - s0) / (s1 - s0),  dt/ds0 = (level - s1) / (s1 - s0)^2,  dt/ds1 = -(level - s0) / (s1 - s0)^2     (fp32)
//   ds_g / dcp[c, l] = m_g * G_g[l] * B_c(xo_g)     G = d sdf / d latent of the row the forward decoded, B the basis weight the row
//                                                   kernel holds (msgrid.hpp), m = inside and the caps left the decoder's value
//   J[v, c, l] = scale[a] * sum_k dt/ds_k * m_k * G_k[l] * B_c(xo_k),   scale = voxel_size / 2
// The band is the set of grid points that carry an endpoint; band_of maps a grid index to its band row (G, weights, base, m).
//
//   msd_dense_kernel     a workgroup streams the [ncp][L] blocks of its vertices (zeros outside the two supports): one vertex when the
//                        block is long, up to MSD_DENSE_VERTS when it is short, so that a workgroup has MSD_DENSE_STORES stores
//                        to make; a lane's store is VEC consecutive latent columns of one control point, stores are coalesced.
//                        `full`: the reference's [V][3][ncp][L] with the two zero planes written.
//   msd_jvp_kernel       one wave per vertex: the (slot, l) products of each endpoint over the lanes, a fixed xor-shuffle tree.
//   msd_vjp_part_kernel  first stage of the adjoint: workgroup (part, tile) walks MSD_VJP_VERTS vertices in order and adds each
//                        endpoint's (slot, l) products into its LDS tile of grad_cp -- the slots of one endpoint name distinct
//                        control points, so the adds of one step never collide, and a barrier separates the steps (a vertex with
//                        no valid endpoint is skipped by the whole workgroup): no atomics, a fixed order.  msd_vjp_sum_kernel adds
//                        the parts in part order.
// A vertex whose edge, band row or base index is out of range contributes nothing (nothing is read or written out of bounds).  An
// edge (p, a) is in range iff 0 <= a <= 2, 0 <= p < npts and p's index along a is below dims[a] - 1 -- the volume's rule
// (vd_vertex): an edge at the last index of axis 1 or 2, whose p + stride[a] is the first point of the next row, is refused like
// one that leaves the grid.  An endpoint is in range iff its band_of row lies in 0 .. nb - 1, its mask is set, 0 <= base < ncp and
// first[x] + deg[x] < n_cp[x] on every axis.
//
// Shared with the volume mesh's derivative (voldiff.hpp), defined here once: the endpoint record MsdEnd, msd_dt (the dt pair),
// msd_ends (band row, mask, base, support check -> the two records; the caller has found p and q valid by its own rule and supplies
// the coefficients), msd_walk (t -> (slot, l) -> weight * G and the control net's float), msd_split / msd_slot (control point ->
// weight slot of an endpoint's support), msd_end_dot, msd_vjp_part (the first stage's body; the mesh type supplies msd_vjp_count and
// msd_vjp_ends, its list and its per-vertex factor) and msd_vjp_sum_kernel.  Shared arithmetic uses common.hpp's rn_* helpers: the
// same bits in every kernel it is inlined into.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msgrid.hpp"

namespace dsdf {

constexpr int MSD_BLOCK = 256;
constexpr int MSD_DENSE_VERTS = 64;    // vertices one workgroup of the dense kernel takes at most
constexpr int MSD_DENSE_STORES = 2048; // stores it aims at when a vertex's block is shorter: eight per lane
constexpr int MSD_VJP_VERTS = 512;     // vertices per first-stage partial of the adjoint
constexpr int MSD_VJP_TILE = 8192;     // floats of grad_cp one workgroup accumulates in LDS (32 KiB)

struct MsdMesh {
  const float* grid;                   // capped sdf [npts]
  const int64_t* edge_point;           // [V]
  const int32_t* edge_axis;            // [V]
  const int32_t* band_of;              // [npts] grid index -> band row, < 0: not in the band
  int64_t npts, stride[3], V;
  uint32_t magic[2];                   // floor(p / stride[o]) = (p * magic[o]) >> shift[o] for every 0 <= p < 2^30, o = 0, 1 (msd_magic)
  int shift[2];
  float scale[3];                      // voxel_size / 2
  float level;
};

// The multiplier and shift of an exact division of a 30-bit number by d, 2 <= d <= 2^30 [host]: with l = ceil(log2 d), k = 30 + l and
// m = ceil(2^k / d) one has 2^k <= m d < 2^k + 2^l = 2^k + 2^(k - 30), so floor(p m / 2^k) = floor(p / d) for 0 <= p < 2^30
// (Granlund and Montgomery 1994, theorem 4.2); m <= 2^31, and p m < 2^61 fits 64 bits.
inline void msd_magic(int64_t d, uint32_t* magic, int* shift) {
  int l = 0;
  while (((int64_t)1 << l) < d) ++l;
  *shift = 30 + l;
  *magic = (uint32_t)((((uint64_t)1 << *shift) + (uint64_t)d - 1) / (uint64_t)d);
}

struct MsdBand {
  const float* G;                      // [nb][ldg]: the first L columns are d sdf / d latent
  const float* w;                      // [nb][MS_WEIGHTS], slot (k * 4 + j) * 4 + i
  const int32_t* base;                 // [nb] first control point, -1: outside
  const uint8_t* m;                    // [nb] 1: the decoder's value survived the caps
  int64_t nb, ldg;
  int deg[3], ncp[3];
  int L, ncp_total;
};

struct MsdEnd { float coef; int64_t row; int first[3]; };   // coef: the caller's factor of the endpoint; row < 0: it contributes nothing

__device__ __forceinline__ void msd_no_ends(MsdEnd e[2]) {
  e[0].row = e[1].row = -1;
  e[0].coef = e[1].coef = 0.f;
}

// dt/ds0, dt/ds1 of t = (level - s0) / (s1 - s0)
__device__ __forceinline__ void msd_dt(float level, float s0, float s1, float dt[2]) {
  const float d = rn_sub(s1, s0), dd = rn_mul(d, d);
  dt[0] = rn_div(rn_sub(level, s1), dd);
  dt[1] = -rn_div(rn_sub(level, s0), dd);
}

// The endpoints at grid points g of a vertex whose mesh found them valid: band row, mask, base control point, the first control
// point per axis and the support check.  An endpoint that passes gets its row and the caller's coef[k]; the other stays as it was.
__device__ __forceinline__ void msd_ends(const MsdBand& B, const int32_t* __restrict__ band_of, const int64_t g[2], const float coef[2],
                                         MsdEnd e[2]) {
  for (int k = 0; k < 2; ++k) {
    const int64_t r = band_of[g[k]];
    if (r < 0 || r >= B.nb || !B.m[r]) continue;
    int b = B.base[r];
    if (b < 0 || b >= B.ncp_total) continue;
    bool ok = true;
    for (int x = 0; x < 3; ++x) {
      const int n = B.ncp[x];
      e[k].first[x] = x < 2 ? b % n : b;
      b /= n;
      ok = ok && e[k].first[x] + B.deg[x] < n;
    }
    if (!ok) continue;
    e[k].row = r;
    e[k].coef = coef[k];
  }
}

// Axis and the two endpoints, coef = scale[a] * dt/ds_k, of vertex v (the same for every lane of a workgroup / wave that shares v).
__device__ __forceinline__ int msd_vertex(const MsdMesh& M, const MsdBand& B, int64_t v, MsdEnd e[2]) {
  msd_no_ends(e);
  const int a = M.edge_axis[v];
  const int64_t p = M.edge_point[v];
  if (a < 0 || a > 2 || p < 0 || p >= M.npts) return a < 0 || a > 2 ? 0 : a;
  // The volume's rule (vd_vertex): the far endpoint lies past the grid along a iff p's index along a is the last one, that is iff
  // p's offset within one step of the next slower axis (the whole grid for a = 0) plus stride[a] leaves that step.  The offset
  // p mod stride[a - 1] comes from the host's multiplier (MsdMesh::magic): a division per vertex on this path, the head of the chain
  // of dependent reads that sets the adjoint's time per vertex, cost the surface adjoint 3 %.
  const int o = a > 0 ? a - 1 : 0;
  const uint32_t pu = (uint32_t)p, d = (uint32_t)M.stride[o];                                      // npts <= 2^30
  const uint32_t outer = a > 0 ? d : (uint32_t)M.npts;
  const uint32_t off = a > 0 ? pu - (uint32_t)(((uint64_t)pu * M.magic[o]) >> M.shift[o]) * d : pu;
  if (off + (uint32_t)M.stride[a] >= outer) return a;
  const int64_t q = p + M.stride[a];
  float dt[2];
  msd_dt(M.level, M.grid[p], M.grid[q], dt);
  const int64_t g[2] = {p, q};
  const float coef[2] = {rn_mul(M.scale[a], dt[0]), rn_mul(M.scale[a], dt[1])};
  msd_ends(B, M.band_of, g, coef, e);
  return a;
}

// Control point c of the net -> its index on each axis.
__device__ __forceinline__ void msd_split(const MsdBand& B, uint32_t c, int ci[3]) {
  const int cr = (int)(c / (uint32_t)B.ncp[0]);
  ci[0] = (int)(c % (uint32_t)B.ncp[0]);
  ci[1] = cr % B.ncp[1];
  ci[2] = cr / B.ncp[1];
}

// The weight slot of control point ci in endpoint e's support, -1: outside it.
__device__ __forceinline__ int msd_slot(const MsdBand& B, const MsdEnd& e, const int ci[3]) {
  const int i = ci[0] - e.first[0], j = ci[1] - e.first[1], kk = ci[2] - e.first[2];
  if (i < 0 || i > B.deg[0] || j < 0 || j > B.deg[1] || kk < 0 || kk > B.deg[2]) return -1;
  return (kk * 4 + j) * 4 + i;
}

// The walk over an endpoint's (slot, l) products, t = slot * L + l below msd_walk_total: -> rn(w[slot] * G[l]), *at the float of the
// control net [ncp][L] the product belongs to.  w, G: the endpoint's rows (msd_row_w, msd_row_G), taken once before the loop.
__device__ __forceinline__ int msd_walk_total(const MsdBand& B) { return (B.deg[0] + 1) * (B.deg[1] + 1) * (B.deg[2] + 1) * B.L; }

__device__ __forceinline__ const float* msd_row_w(const MsdBand& B, const MsdEnd& e) { return B.w + e.row * MS_WEIGHTS; }
__device__ __forceinline__ const float* msd_row_G(const MsdBand& B, const MsdEnd& e) { return B.G + e.row * B.ldg; }

__device__ __forceinline__ float msd_walk(const MsdBand& B, const MsdEnd& e, const float* __restrict__ w, const float* __restrict__ G, int t,
                                          int64_t* at) {
  const int d0 = B.deg[0] + 1, d1 = B.deg[1] + 1, L = B.L;
  const int s = t / L, l = t - s * L;
  const int i = s % d0, sr = s / d0;
  const int j = sr % d1, kk = sr / d1;
  const int c = (e.first[0] + i) + B.ncp[0] * ((e.first[1] + j) + B.ncp[1] * (e.first[2] + kk));
  *at = (int64_t)c * L + l;
  return rn_mul(w[(kk * 4 + j) * 4 + i], G[l]);
}

// The VEC values of store q (control point q / (L / VEC), latent columns (q % (L / VEC)) * VEC ..) of a vertex with endpoints e.
template <int VEC>
__device__ __forceinline__ void msd_dense_store(const MsdBand& B, const MsdEnd* e, uint32_t q, uint32_t Lq, float* __restrict__ out) {
  const uint32_t c = q / Lq, l = (q - c * Lq) * VEC;
  int ci[3];
  msd_split(B, c, ci);
  float val[VEC];
  for (int x = 0; x < VEC; ++x) val[x] = 0.f;
  for (int k = 0; k < 2; ++k) {
    if (e[k].row < 0) continue;
    const int s = msd_slot(B, e[k], ci);
    if (s < 0) continue;
    const float f = rn_mul(e[k].coef, B.w[e[k].row * MS_WEIGHTS + s]);
    const float* __restrict__ G = B.G + e[k].row * B.ldg + l;
    for (int x = 0; x < VEC; ++x) val[x] = fmaf(f, G[x], val[x]);
  }
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(out) = make_float4(val[0], val[1], val[2], val[3]);
  else out[0] = val[0];
}

// vpw vertices per workgroup (host: 1 unless a vertex's block is short; then as many as make MSD_DENSE_STORES stores, at most
// MSD_DENSE_VERTS).  Phase 1, one lane per vertex: axis and endpoints, left in LDS.  Phase 2: the workgroup's vertices are one
// contiguous run of the output, lane t writes store t.
template <int VEC>
__global__ __launch_bounds__(MSD_BLOCK) void msd_dense_kernel(MsdMesh M, MsdBand B, float* __restrict__ jac,
                                                              int32_t* __restrict__ axis_out, int full, int vpw) {
  __shared__ MsdEnd end_s[MSD_DENSE_VERTS][2];
  __shared__ int axis_s[MSD_DENSE_VERTS];
  const int tid = threadIdx.x;
  const int64_t v0 = (int64_t)blockIdx.x * vpw;
  const int nv = (int)((M.V - v0) < (int64_t)vpw ? (M.V - v0) : (int64_t)vpw);
  if (tid < nv) {
    MsdEnd e[2];
    const int a = msd_vertex(M, B, v0 + tid, e);
    end_s[tid][0] = e[0];
    end_s[tid][1] = e[1];
    axis_s[tid] = a;
    if (axis_out) axis_out[v0 + tid] = a;
  }
  __syncthreads();
  const uint32_t Lq = (uint32_t)(B.L / VEC), nq = (uint32_t)B.ncp_total * Lq;          // stores per plane
  const int64_t per = (int64_t)B.ncp_total * B.L;
  if (vpw == 1) {                                           // a long block: plane by plane, no division by the block length
    const int a = axis_s[0];
    for (int b = full ? 0 : a; b < (full ? 3 : a + 1); ++b) {
      float* __restrict__ out = jac + (full ? (v0 * 3 + b) * per : v0 * per);
      for (uint32_t q = tid; q < nq; q += MSD_BLOCK) {
        if (b == a) msd_dense_store<VEC>(B, end_s[0], q, Lq, out + (int64_t)q * VEC);
        else for (int x = 0; x < VEC; ++x) out[(int64_t)q * VEC + x] = 0.f;
      }
    }
    return;
  }
  const uint32_t planes = full ? 3u : 1u, pv = planes * nq;                              // stores per vertex: at most MSD_DENSE_STORES
  float* __restrict__ out0 = jac + v0 * (int64_t)planes * per;
  const uint32_t total = (uint32_t)nv * pv;
  for (uint32_t t = tid; t < total; t += MSD_BLOCK) {
    const uint32_t vl = t / pv, r = t - vl * pv;
    const uint32_t b = full ? r / nq : 0u, q = r - b * nq;
    float* __restrict__ out = out0 + (int64_t)t * VEC;
    if (!full || (int)b == axis_s[vl]) msd_dense_store<VEC>(B, end_s[vl], q, Lq, out);
    else for (int x = 0; x < VEC; ++x) out[x] = 0.f;
  }
}

// sum over the (slot, l) products of one endpoint: sum_s sum_l w[s] * G[l] * x[c(s)][l], this lane's share
__device__ __forceinline__ float msd_end_dot(const MsdBand& B, const MsdEnd& e, const float* __restrict__ x, int lane, int step) {
  const int total = msd_walk_total(B);
  const float* __restrict__ w = msd_row_w(B, e);
  const float* __restrict__ G = msd_row_G(B, e);
  float acc = 0.f;
  for (int t = lane; t < total; t += step) {
    int64_t at;
    const float wg = msd_walk(B, e, w, G, t, &at);
    acc = fmaf(wg, x[at], acc);
  }
  return acc;
}

__global__ __launch_bounds__(MSD_BLOCK) void msd_jvp_kernel(MsdMesh M, MsdBand B, const float* __restrict__ d_cp,
                                                            float* __restrict__ d_verts) {
  const int lane = threadIdx.x & 63;
  const int64_t v = (int64_t)blockIdx.x * (MSD_BLOCK / 64) + (threadIdx.x >> 6);
  if (v >= M.V) return;                                      // (no barrier below)
  MsdEnd e[2];
  const int a = msd_vertex(M, B, v, e);
  float tot = 0.f;
  for (int k = 0; k < 2; ++k) {
    if (e[k].row < 0) continue;                              // wave-uniform
    float acc = msd_end_dot(B, e[k], d_cp, lane, 64);
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    tot = fmaf(e[k].coef, acc, tot);
  }
  if (lane < 3) d_verts[v * 3 + lane] = lane == a ? tot : 0.f;
}

// The surface's part of the adjoint's first stage: its list is every vertex, and endpoint k of vertex v adds
// f = g * (scale[a] * dt/ds_k) times the walk's products, g = grad_verts[v, a]: f is left in e[k].coef.
__device__ __forceinline__ int64_t msd_vjp_count(const MsdMesh& M) { return M.V; }

__device__ __forceinline__ void msd_vjp_ends(const MsdMesh& M, const MsdBand& B, int64_t v, const float* __restrict__ grad_verts,
                                             MsdEnd e[2]) {
  const float g = grad_verts[v * 3 + msd_vertex(M, B, v, e)];
  for (int k = 0; k < 2; ++k) e[k].coef = rn_mul(g, e[k].coef);
}

// First stage of the adjoint of a mesh type with msd_vjp_count and msd_vjp_ends (the surface above, the volume in voldiff.hpp).
template <class Mesh>
__device__ __forceinline__ void msd_vjp_part(const Mesh& M, const MsdBand& B, const float* __restrict__ grad_verts,
                                             float* __restrict__ part) {
  __shared__ float acc[MSD_VJP_TILE];
  const int tid = threadIdx.x;
  const int64_t per = (int64_t)B.ncp_total * B.L;
  const int64_t tile0 = (int64_t)blockIdx.y * MSD_VJP_TILE;
  const int tn = (int)((per - tile0) < (int64_t)MSD_VJP_TILE ? (per - tile0) : (int64_t)MSD_VJP_TILE);
  for (int t = tid; t < tn; t += MSD_BLOCK) acc[t] = 0.f;
  __syncthreads();
  const int64_t n = msd_vjp_count(M), i0 = (int64_t)blockIdx.x * MSD_VJP_VERTS;
  const int64_t i1 = i0 + MSD_VJP_VERTS < n ? i0 + MSD_VJP_VERTS : n;
  const int total = msd_walk_total(B);
  for (int64_t i = i0; i < i1; ++i) {                        // every bound and branch around the barriers is workgroup-uniform
    MsdEnd e[2];
    msd_vjp_ends(M, B, i, grad_verts, e);
    if (e[0].row < 0 && e[1].row < 0) continue;              // uniform: nothing to add, no barrier needed
    for (int k = 0; k < 2; ++k) {
      if (e[k].row >= 0) {
        const float* __restrict__ w = msd_row_w(B, e[k]);
        const float* __restrict__ G = msd_row_G(B, e[k]);
        for (int t = tid; t < total; t += MSD_BLOCK) {
          int64_t at;
          const float wg = msd_walk(B, e[k], w, G, t, &at);
          at -= tile0;
          if (at >= 0 && at < tn) acc[at] = fmaf(e[k].coef, wg, acc[at]);
        }
      }
      __syncthreads();
    }
  }
  float* __restrict__ out = part + (int64_t)blockIdx.x * per + tile0;
  for (int t = tid; t < tn; t += MSD_BLOCK) out[t] = acc[t];
}

__global__ __launch_bounds__(MSD_BLOCK) void msd_vjp_part_kernel(MsdMesh M, MsdBand B, const float* __restrict__ grad_verts,
                                                                 float* __restrict__ part) {
  msd_vjp_part(M, B, grad_verts, part);
}

__global__ __launch_bounds__(MSD_BLOCK) void msd_vjp_sum_kernel(const float* __restrict__ part, int n_parts, int64_t per,
                                                                float* __restrict__ grad_cp) {
  const int64_t t = (int64_t)blockIdx.x * MSD_BLOCK + threadIdx.x;
  if (t >= per) return;
  float s = 0.f;
  for (int p = 0; p < n_parts; ++p) s += part[(int64_t)p * per + t];
  grad_cp[t] = s;
}

}  // namespace dsdf
