// mcubes.hpp -- marching cubes over a dense fp32 grid sdf[nx][ny][nz] (z fastest) on the device (gfx950).
//
// A grid point is inside iff v < level (strictly).  One vertex per grid edge whose endpoints lie on different sides; edge
// (p, a) runs from grid point p to p + e_a.  Output order is fixed by prefix sums, no atomics: vertices by grid-point linear
// index, then axis x, y, z; faces by cell linear index (a cell is named by its lower corner), then table order.
//
// Passes (one thread per grid point, MC_BLOCK points per workgroup, linear order):
//   1. classify:  mask[p] = 3-bit crossing mask of p's edges, cas[p] = 8-bit case of the cell at p (0 off the cell range);
//                 per workgroup, its vertex and triangle totals
//   2. scan:      one workgroup turns the per-workgroup totals into 64-bit exclusive offsets (+ the two grand totals):
//                 blockops.hpp's offset_scan_kernel<2>
//   3. vertices:  workgroup scan of popcount(mask) + offset -> vbase[p] (id of p's first vertex) and the interpolated positions
//   4. faces:     workgroup scan of the triangle counts + offset; edge (corner c of cell p, axis a) has vertex id
//                 vbase[q] + popcount(mask[q] & ((1 << a) - 1)), q = p + offset(c): no edge-id map
//   edges (on request, dsdf_mc_edges): pass 3's scan again, writing (p, a) of every vertex id instead of its position; it reads
//                 only what passes 1 and 2 left (mask, offsets)
// The case table is generated (deepsdf_amd/mc_table.py -> mc_table.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blockops.hpp"
#include "common.hpp"
#include "mc_table.hpp"

namespace dsdf {

constexpr int MC_BLOCK = 256;
constexpr int MC_MAX_DIM = 1024;

__constant__ int8_t mc_tri_d[256][MC_TABLE_W] = DSDF_MC_TRI_INIT;
__constant__ uint8_t mc_ntri_d[256] = DSDF_MC_NTRI_INIT;
__constant__ uint8_t mc_edge_d[12][2] = DSDF_MC_EDGES_INIT;
static const int8_t mc_tri_h[256][MC_TABLE_W] = DSDF_MC_TRI_INIT;   // what dsdf_mc_case_table returns

struct McGrid {
  const float* sdf;
  int nx, ny, nz;
  float level;
  int64_t npts;
};

struct McWs {             // carved from the caller's workspace (mc_plan in dsdf_api.hip)
  uint8_t* mask;          // [npts]
  uint8_t* cas;           // [npts]
  int32_t* vbase;         // [npts]
  int32_t* bv;            // [nblocks] vertices per workgroup
  int32_t* bf;            // [nblocks] triangles per workgroup
  int64_t* ov;            // [nblocks + 1] exclusive offsets
  int64_t* of;            // [nblocks + 1]
  int64_t nblocks;
};

struct McOut {
  float spacing[3], origin[3];
  float* verts;           // [nv][3]
  int32_t* faces;         // [nf][3]
  int64_t nv, nf;         // sizes of the caller's buffers: nothing is written past them
};

__global__ __launch_bounds__(MC_BLOCK) void mc_classify_kernel(McGrid g, McWs w) {
  __shared__ int s[MC_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  int nv = 0, nt = 0;
  if (p < g.npts) {
    int i, j, k;
    grid_ijk(p, g.ny, g.nz, i, j, k);
    const int64_t syz = (int64_t)g.ny * g.nz;
    const float* v = g.sdf + p;
    const bool in0 = v[0] < g.level;
    const bool hx = i + 1 < g.nx, hy = j + 1 < g.ny, hz = k + 1 < g.nz;
    uint32_t m = 0;
    if (hx && (v[syz] < g.level) != in0) m |= 1u;
    if (hy && (v[g.nz] < g.level) != in0) m |= 2u;
    if (hz && (v[1] < g.level) != in0) m |= 4u;
    uint32_t cs = 0;
    if (hx && hy && hz) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int64_t off = (c & 1) * syz + ((c >> 1) & 1) * (int64_t)g.nz + ((c >> 2) & 1);
        cs |= (uint32_t)(v[off] < g.level) << c;
      }
    }
    w.mask[p] = (uint8_t)m;
    w.cas[p] = (uint8_t)cs;
    nv = __popc(m);
    nt = mc_ntri_d[cs];
  }
  // both counts in one scan: a workgroup has at most 3 * 256 vertices and 5 * 256 triangles (< 2^16 each)
  const int tot = block_scan_incl<int, MC_BLOCK>(nv | (nt << 16), s);
  if (threadIdx.x == MC_BLOCK - 1) {
    w.bv[blockIdx.x] = tot & 0xFFFF;
    w.bf[blockIdx.x] = tot >> 16;
  }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_vertex_kernel(McGrid g, McWs w, McOut o) {
  __shared__ int s[MC_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const uint32_t m = p < g.npts ? w.mask[p] : 0u;
  const int n = __popc(m);
  const int inc = block_scan_incl<int, MC_BLOCK>(n, s);
  if (p >= g.npts) return;
  int64_t id = w.ov[blockIdx.x] + inc - n;
  w.vbase[p] = (int32_t)id;          // the host refuses totals above INT32_MAX before this launch
  if (!m) return;
  int i, j, k;
  grid_ijk(p, g.ny, g.nz, i, j, k);
  const int64_t stride[3] = {(int64_t)g.ny * g.nz, (int64_t)g.nz, 1};
  const int idx[3] = {i, j, k};
  const float v0 = g.sdf[p];
  for (int a = 0; a < 3; ++a) {
    if (!((m >> a) & 1u)) continue;
    const float v1 = g.sdf[p + stride[a]];
    // v0 and v1 lie on different sides of the level, so v1 != v0.  Every operation rounds on its own: the rn_* helpers of
    // common.hpp keep the compiler from contracting origin + x * spacing (or any other pair) into an FMA.
    const float t = rn_div(rn_sub(g.level, v0), rn_sub(v1, v0));
    if (id < o.nv) {
      float* out = o.verts + id * 3;
      for (int b = 0; b < 3; ++b) {
        const float x = b == a ? rn_add((float)idx[b], t) : (float)idx[b];
        out[b] = rn_add(o.origin[b], rn_mul(x, o.spacing[b]));
      }
    }
    ++id;
  }
}

// The grid edge of every vertex id, in the vertex kernel's order: the same scan of popcount(mask) + offset, so it needs only what
// the count pass left (mask, ov) and neither the grid nor vbase.  Nothing is written at or past nv.
__global__ __launch_bounds__(MC_BLOCK) void mc_edge_kernel(int64_t npts, McWs w, int64_t nv, int64_t* __restrict__ edge_point,
                                                           int32_t* __restrict__ edge_axis) {
  __shared__ int s[MC_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const uint32_t m = p < npts ? w.mask[p] : 0u;
  const int n = __popc(m);
  const int inc = block_scan_incl<int, MC_BLOCK>(n, s);
  if (!m) return;
  int64_t id = w.ov[blockIdx.x] + inc - n;
  for (int a = 0; a < 3; ++a) {
    if (!((m >> a) & 1u)) continue;
    if (id < nv) {
      edge_point[id] = p;
      edge_axis[id] = a;
    }
    ++id;
  }
}

__global__ __launch_bounds__(MC_BLOCK) void mc_face_kernel(McGrid g, McWs w, McOut o) {
  __shared__ int s[MC_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * MC_BLOCK + threadIdx.x;
  const uint32_t cs = p < g.npts ? w.cas[p] : 0u;
  const int n = mc_ntri_d[cs];
  const int inc = block_scan_incl<int, MC_BLOCK>(n, s);
  if (p >= g.npts || n == 0) return;
  const int64_t first = w.of[blockIdx.x] + inc - n;
  const int64_t syz = (int64_t)g.ny * g.nz;
  for (int tr = 0; tr < n; ++tr) {
    if (first + tr >= o.nf) break;
    int32_t* out = o.faces + (first + tr) * 3;
    for (int r = 0; r < 3; ++r) {
      const int e = mc_tri_d[cs][3 * tr + r];
      const int c = mc_edge_d[e][0], a = mc_edge_d[e][1];
      const int64_t q = p + (c & 1) * syz + ((c >> 1) & 1) * (int64_t)g.nz + ((c >> 2) & 1);
      out[r] = w.vbase[q] + __popc(w.mask[q] & ((1u << a) - 1u));
    }
  }
}

}  // namespace dsdf
