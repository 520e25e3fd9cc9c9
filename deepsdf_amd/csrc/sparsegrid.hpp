// sparsegrid.hpp -- surface following on blocks of the dense grid sdf[nx][ny][nz] (z fastest): the index and streaming kernels that
// let the meshing paths decode only the blocks the surface passes through.  The decode itself and marching cubes are
// the existing ones; nothing here computes an SDF value.
//
// Block edge b >= 2 cells.  Coarse coordinates of axis a: {0, b, 2b, ... < n_a - 1} + {n_a - 1}, that is min(m * b, n_a - 1) for
// m = 0 .. nb_a, nb_a = ceil((n_a - 1) / b) blocks (the last one may be short).  Block (I, J, K), linear (I * nb_y + J) * nb_z + K, owns
// the closed point box between consecutive coarse coordinates: neighbours share their face points, every cell lies in one block.
// A grid point is inside iff v < level (strictly): marching cubes' rule.
//
// State of a block (one byte): 0 inactive, 1 new (active, its points not all valued yet), 2 valued.  have[p] (one byte per grid
// point): the point holds a decoded value.  Passes, one thread per block or per point, SG_BLOCK threads per workgroup, integer
// work and plain stores, no atomics; every count is a per-workgroup total (LDS scan) summed or scanned by one workgroup, so the
// emitted order is the ascending linear index and two runs give identical bytes:
//   coarse   the coarse lattice's linear indices, ascending; have = 1 there (have is cleared first, by a memset on the stream)
//   seed     state = 1 where the 8 corners are not all inside or all outside, or min |v - level| <= thr (fp32); else 0
//   grow     gather form: an inactive block whose face-neighbour is in state 1 (its values were written this round) and whose
//            shared face has mixed inside flags is marked in `pend` (mark kernel: reads state, writes pend); then 1 -> 2 and
//            marked -> 1 (apply kernel: every thread touches its own block only).  A neighbour valued in an earlier round was
//            examined in that round and the face's values have not changed since, so looking at state 1 alone loses nothing.
//   points   count, then emit, the points without a value that lie in a block of state 1; emit sets have
//   coords   xyz of a list of indices: fp32 index * voxel_size, then + origin, each rounded on its own (never an FMA)
//   scatter  grid[idx[q]] = values[q]
//   caps_at  the microstructure caps (msgrid.hpp ms_caps_kernel, restated) in place on the values of a list of indices
//   fill     a point without a value takes the value at the low corner of the lowest-index block that contains it
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blockops.hpp"
#include "common.hpp"

namespace dsdf {

constexpr int SG_BLOCK = 256;
constexpr int SG_MAX_CAPS = 6;

struct SgGrid {
  int n[3], nb[3], nc[3];      // points, blocks, coarse coordinates (nb + 1) per axis
  int b;
  int64_t npts, nblk, ncoarse;
};

struct SgWs {                  // carved from the caller's workspace (sg_plan in dsdf_api.hip)
  uint8_t* state;              // [nblk]
  uint8_t* pend;               // [nblk]
  uint8_t* have;               // [npts]
  int32_t* part;               // [nparts] per-workgroup totals
  int64_t* offs;               // [nparts + 1] exclusive offsets
  int64_t nparts;              // workgroups of a per-point pass (>= those of a per-block pass)
};

struct SgCapRec { int dim, cap; float m, c; };
struct SgCaps {
  int n[3];
  float vs[3], org[3];
  int ncaps;
  SgCapRec r[SG_MAX_CAPS];
};

__device__ __forceinline__ int sg_cc(const SgGrid& g, int a, int m) {
  const int x = m * g.b;
  return x < g.n[a] - 1 ? x : g.n[a] - 1;
}

// The blocks of axis a whose closed range holds coordinate x: lo, and lo + 1 as well when cnt == 2 (x is a shared coarse coordinate).
__device__ __forceinline__ void sg_blocks_of(const SgGrid& g, int a, int x, int& lo, int& cnt) {
  int I = x / g.b;
  if (I > g.nb[a] - 1) I = g.nb[a] - 1;
  const int lower = (I > 0 && x == I * g.b) ? 1 : 0;
  lo = I - lower;
  cnt = 1 + lower;
}

__device__ __forceinline__ bool sg_in_new_block(const SgGrid& g, const uint8_t* __restrict__ state, const int* ijk) {
  int lo[3], cnt[3];
  for (int a = 0; a < 3; ++a) sg_blocks_of(g, a, ijk[a], lo[a], cnt[a]);
  bool hit = false;
  for (int di = 0; di < cnt[0]; ++di)
    for (int dj = 0; dj < cnt[1]; ++dj)
      for (int dk = 0; dk < cnt[2]; ++dk)
        hit |= state[((int64_t)(lo[0] + di) * g.nb[1] + (lo[1] + dj)) * g.nb[2] + (lo[2] + dk)] == 1;
  return hit;
}

__global__ __launch_bounds__(SG_BLOCK) void sg_coarse_kernel(SgGrid g, int64_t* __restrict__ indices, uint8_t* __restrict__ have) {
  const int64_t q = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  if (q >= g.ncoarse) return;
  const int64_t cyz = (int64_t)g.nc[1] * g.nc[2];
  const int I = (int)(q / cyz);
  const int r = (int)(q - (int64_t)I * cyz);
  const int J = r / g.nc[2], K = r - J * g.nc[2];
  const int64_t p = ((int64_t)sg_cc(g, 0, I) * g.n[1] + sg_cc(g, 1, J)) * g.n[2] + sg_cc(g, 2, K);
  indices[q] = p;
  have[p] = 1;
}

__device__ __forceinline__ void sg_block_ijk(int64_t blk, const SgGrid& g, int* B) {
  const int64_t byz = (int64_t)g.nb[1] * g.nb[2];
  B[0] = (int)(blk / byz);
  const int r = (int)(blk - (int64_t)B[0] * byz);
  B[1] = r / g.nb[2];
  B[2] = r - B[1] * g.nb[2];
}

__global__ __launch_bounds__(SG_BLOCK) void sg_seed_kernel(SgGrid g, const float* __restrict__ sdf, float level, float thr,
                                                           uint8_t* __restrict__ state, int32_t* __restrict__ part) {
  __shared__ int s[SG_BLOCK];
  const int64_t blk = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  int act = 0;
  if (blk < g.nblk) {
    int B[3];
    sg_block_ijk(blk, g, B);
    int n_in = 0;
    bool close = false;
    for (int c = 0; c < 8; ++c) {
      const int x = sg_cc(g, 0, B[0] + ((c >> 2) & 1)), y = sg_cc(g, 1, B[1] + ((c >> 1) & 1)), z = sg_cc(g, 2, B[2] + (c & 1));
      const float v = sdf[((int64_t)x * g.n[1] + y) * g.n[2] + z];
      n_in += v < level ? 1 : 0;
      close |= fabsf(rn_sub(v, level)) <= thr;                       // false for a NaN
    }
    act = ((n_in != 0 && n_in != 8) || close) ? 1 : 0;
    state[blk] = (uint8_t)act;
  }
  const int tot = block_scan_incl<int, SG_BLOCK>(act, s);
  if (threadIdx.x == SG_BLOCK - 1) part[blockIdx.x] = tot;
}

// Mixed inside flags over the face of block B in the plane of coarse coordinate B[a] + side of axis a.
__device__ __forceinline__ bool sg_face_mixed(const SgGrid& g, const float* __restrict__ sdf, float level, const int* B, int a, int side) {
  const int u = (a + 1) % 3, w = (a + 2) % 3;
  const int64_t stride[3] = {(int64_t)g.n[1] * g.n[2], (int64_t)g.n[2], 1};
  const int xa = sg_cc(g, a, B[a] + side);
  const int u0 = sg_cc(g, u, B[u]), u1 = sg_cc(g, u, B[u] + 1), w0 = sg_cc(g, w, B[w]), w1 = sg_cc(g, w, B[w] + 1);
  bool any_in = false, any_out = false;
  for (int iu = u0; iu <= u1; ++iu) {
    const float* row = sdf + xa * stride[a] + iu * stride[u];
    for (int iw = w0; iw <= w1; ++iw) {
      const bool in = row[iw * stride[w]] < level;
      any_in |= in;
      any_out |= !in;
    }
  }
  return any_in && any_out;
}

__global__ __launch_bounds__(SG_BLOCK) void sg_grow_mark_kernel(SgGrid g, const float* __restrict__ sdf, float level,
                                                                const uint8_t* __restrict__ state, uint8_t* __restrict__ pend) {
  const int64_t blk = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  if (blk >= g.nblk) return;
  uint8_t mark = 0;
  if (state[blk] == 0) {
    int B[3];
    sg_block_ijk(blk, g, B);
    const int64_t bstride[3] = {(int64_t)g.nb[1] * g.nb[2], (int64_t)g.nb[2], 1};
    for (int a = 0; a < 3 && !mark; ++a) {
      if (B[a] > 0 && state[blk - bstride[a]] == 1 && sg_face_mixed(g, sdf, level, B, a, 0)) mark = 1;
      if (!mark && B[a] + 1 < g.nb[a] && state[blk + bstride[a]] == 1 && sg_face_mixed(g, sdf, level, B, a, 1)) mark = 1;
    }
  }
  pend[blk] = mark;
}

__global__ __launch_bounds__(SG_BLOCK) void sg_grow_apply_kernel(int64_t nblk, uint8_t* __restrict__ state, const uint8_t* __restrict__ pend,
                                                                 int32_t* __restrict__ part) {
  __shared__ int s[SG_BLOCK];
  const int64_t blk = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  int act = 0;
  if (blk < nblk) {
    const uint8_t st = state[blk];
    if (st == 1) state[blk] = 2;
    else if (st == 0 && pend[blk]) { state[blk] = 1; act = 1; }
  }
  const int tot = block_scan_incl<int, SG_BLOCK>(act, s);
  if (threadIdx.x == SG_BLOCK - 1) part[blockIdx.x] = tot;
}

// One workgroup: *out = the sum of part[0 .. n) in 64 bits, a fixed order.
__global__ __launch_bounds__(SG_BLOCK) void sg_sum_kernel(const int32_t* __restrict__ part, int64_t n, int64_t* __restrict__ out) {
  __shared__ int64_t s[SG_BLOCK];
  int64_t x = 0;
  for (int64_t q = threadIdx.x; q < n; q += SG_BLOCK) x += part[q];
  const int64_t tot = block_tree_sum<int64_t, SG_BLOCK>(x, s);
  if (threadIdx.x == 0) *out = tot;
}

__global__ __launch_bounds__(SG_BLOCK) void sg_points_count_kernel(SgGrid g, const uint8_t* __restrict__ state,
                                                                   const uint8_t* __restrict__ have, int32_t* __restrict__ part) {
  __shared__ int s[SG_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  int f = 0;
  if (p < g.npts && !have[p]) {
    int ijk[3];
    grid_ijk(p, g.n[1], g.n[2], ijk[0], ijk[1], ijk[2]);
    f = sg_in_new_block(g, state, ijk) ? 1 : 0;
  }
  const int tot = block_scan_incl<int, SG_BLOCK>(f, s);
  if (threadIdx.x == SG_BLOCK - 1) part[blockIdx.x] = tot;
}

// The count pass's flags again (state and have are unchanged in between), placed by scan + offset; nothing is written at or past n.
__global__ __launch_bounds__(SG_BLOCK) void sg_points_emit_kernel(SgGrid g, const uint8_t* __restrict__ state, uint8_t* __restrict__ have,
                                                                  const int64_t* __restrict__ offs, int64_t n, int64_t* __restrict__ indices) {
  __shared__ int s[SG_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  int f = 0;
  if (p < g.npts && !have[p]) {
    int ijk[3];
    grid_ijk(p, g.n[1], g.n[2], ijk[0], ijk[1], ijk[2]);
    f = sg_in_new_block(g, state, ijk) ? 1 : 0;
  }
  const int inc = block_scan_incl<int, SG_BLOCK>(f, s);
  if (!f) return;
  const int64_t at = offs[blockIdx.x] + inc - 1;
  if (at < n) {
    indices[at] = p;
    have[p] = 1;
  }
}

struct SgAxes { int n[3]; float vs[3], org[3]; };

__global__ __launch_bounds__(SG_BLOCK) void sg_coords_kernel(SgAxes g, const int64_t* __restrict__ indices, int64_t n, float* __restrict__ xyz) {
  const int64_t q = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  if (q >= n) return;
  int ijk[3];
  grid_ijk(indices[q], g.n[1], g.n[2], ijk[0], ijk[1], ijk[2]);
  for (int a = 0; a < 3; ++a) xyz[q * 3 + a] = rn_add(rn_mul((float)ijk[a], g.vs[a]), g.org[a]);
}

// An index outside [0, npts) writes nothing.
__global__ __launch_bounds__(SG_BLOCK) void sg_scatter_kernel(const int64_t* __restrict__ indices, int64_t n, const float* __restrict__ values,
                                                              float* __restrict__ sdf, int64_t npts) {
  const int64_t q = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  if (q >= n) return;
  const int64_t p = indices[q];
  if (p >= 0 && p < npts) sdf[p] = values[q];
}

// ms_caps_kernel's arithmetic (msgrid.hpp) at listed points: xo = fp32 index * voxel size + origin, each rounded on its own; the
// records in order (a min and a max do not commute), then the six faces of [-1, 1]^3.
__global__ __launch_bounds__(SG_BLOCK) void sg_caps_kernel(SgCaps c, const int64_t* __restrict__ indices, int64_t n, float* __restrict__ sdf) {
  const int64_t q = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  if (q >= n) return;
  int ijk[3];
  grid_ijk(indices[q], c.n[1], c.n[2], ijk[0], ijk[1], ijk[2]);
  float xo[3];
  for (int a = 0; a < 3; ++a) xo[a] = rn_add(rn_mul((float)ijk[a], c.vs[a]), c.org[a]);
  float v = sdf[q];
  for (int r = 0; r < c.ncaps; ++r) {
    const SgCapRec R = c.r[r];
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

// A corner of the coarse lattice always has a value, so no thread reads what another one writes.
__global__ __launch_bounds__(SG_BLOCK) void sg_fill_kernel(SgGrid g, const uint8_t* __restrict__ have, float* __restrict__ sdf) {
  const int64_t p = (int64_t)blockIdx.x * SG_BLOCK + threadIdx.x;
  if (p >= g.npts || have[p]) return;
  int ijk[3], lo[3], cnt;
  grid_ijk(p, g.n[1], g.n[2], ijk[0], ijk[1], ijk[2]);
  for (int a = 0; a < 3; ++a) sg_blocks_of(g, a, ijk[a], lo[a], cnt);
  sdf[p] = sdf[((int64_t)(lo[0] * g.b) * g.n[1] + lo[1] * g.b) * g.n[2] + lo[2] * g.b];
}

}  // namespace dsdf
