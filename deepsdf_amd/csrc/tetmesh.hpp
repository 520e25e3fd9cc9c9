// tetmesh.hpp -- a conforming tetrahedral mesh of the solid {sdf < level} of a dense fp32 grid sdf[nx][ny][nz] (z fastest) on the
// device (gfx950), with its boundary triangles, and the solid's connected components.  The specification is in include/dsdf.h
// (dsdf_tet_*); tests/tet_numpy.py restates it in numpy.
//
// Every cell is cut into the six Kuhn tetrahedra around its diagonal (0,0,0)-(1,1,1): permutation pi of the axes gives the corners
// q0 = cell origin, q1 = q0 + e_pi0, q2 = q1 + e_pi1, q3 = q2 + e_pi2, with det(q1 - q0, q2 - q0, q3 - q0) = sign(pi).  Every
// orientation below follows from that sign and from integer relabellings: there is no floating-point orientation test.  A
// tetrahedron edge is (p, c): its lower grid point and a class c in 1..7 with direction (c & 1, (c >> 1) & 1, (c >> 2) & 1).
//
// Passes (one thread per grid point, TET_BLOCK points per workgroup, linear order; the shape of mcubes.hpp):
//   1. classify:  rec[p] = bit 0 inside, bits 1..7 crossing classes of p's edges; ne[p] / nb[p] = elements / boundary triangles of
//                 the cell at p (0 off the cell range); per workgroup its three totals
//   2. scan:      one workgroup turns the per-workgroup totals into 64-bit exclusive offsets (+ the three grand totals):
//                 blockops.hpp's offset_scan_kernel<3>
//   3. vertices:  workgroup scan of popcount(rec) + offset -> vbase[p]; positions (and on request the (point, class) of every id)
//   4. elements:  workgroup scan of ne | nb << 16 + offsets; the id of the grid vertex q is vbase[q], of edge vertex (q, c)
//                 vbase[q] + popcount(rec[q] & ((1 << c) - 1)): no edge-id map, no atomics
//   components:   components.hpp's min-label hooking with shortcutting over the 14-neighbour graph of the Kuhn edges: its int32
//                 atomicMin / atomicAdd are the only atomics this file uses and change the road, not the result
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blockops.hpp"
#include "common.hpp"
#include "components.hpp"
#include "mcubes.hpp"

namespace dsdf {

constexpr int TET_BLOCK = 256;
constexpr int TET_MAX_ELEMS = 18;        // elements of a cell (3 per Kuhn tetrahedron)
constexpr int TET_MAX_BFACES = 36;       // boundary triangles of a cell (2 cut + 2 x 2 plane per Kuhn tetrahedron)
static_assert(TET_BLOCK * TET_MAX_BFACES < (1 << 16) && TET_BLOCK * TET_MAX_ELEMS < (1 << 16), "two counts share one scanned int");

struct TetWs {            // carved from the caller's workspace (tet_plan in dsdf_api.hip)
  uint8_t* rec;           // [npts]
  uint8_t* ne;            // [npts]
  uint8_t* nb;            // [npts]
  int32_t* vbase;         // [npts]
  int32_t* bcount[3];     // [nblocks] vertices, elements, boundary triangles per workgroup
  int64_t* boff[3];       // [nblocks + 1] exclusive offsets
  int64_t nblocks;
};

struct TetOut {
  float spacing[3], origin[3];
  float t_clamp;
  float* verts;           // [nv][3]
  int32_t* tets;          // [nt][4]
  int32_t* bfaces;        // [nb][3]
  int8_t* bface_kind;     // [nb]
  int64_t* vert_point;    // [nv] or NULL
  int32_t* vert_class;    // [nv] or NULL
  int64_t nv, nt, nb;     // sizes of the caller's buffers: nothing is written past them
};

// axis pi_r of Kuhn tetrahedron pi (itertools.permutations(range(3)) order) and the permutation's sign
__device__ __forceinline__ constexpr int tet_axis(int pi, int r) {
  constexpr int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  return P[pi][r];
}
__device__ __forceinline__ constexpr int tet_sign(int pi) {
  constexpr int S[6] = {1, -1, -1, 1, 1, -1};
  return S[pi];
}
// corner r of Kuhn tetrahedron pi as a mask of unit steps (bit a: one step along axis a)
__device__ __forceinline__ constexpr int tet_corner(int pi, int r) {
  return r == 0 ? 0 : r == 1 ? (1 << tet_axis(pi, 0)) : r == 2 ? ((1 << tet_axis(pi, 0)) | (1 << tet_axis(pi, 1))) : 7;
}
// elements / cut triangles of a Kuhn tetrahedron and triangles of the inside part of a face, by the number of inside corners
__device__ __forceinline__ int tet_n_elems(int n) { return (0x13310 >> (4 * n)) & 0xF; }
__device__ __forceinline__ int tet_n_cut(int n) { return (0x01210 >> (4 * n)) & 0xF; }
__device__ __forceinline__ int tet_n_plane(int n) { return (0x1210 >> (4 * n)) & 0xF; }

__device__ __forceinline__ int64_t tet_offset(int m, int64_t syz, int nz) {
  return (m & 1) * syz + ((m >> 1) & 1) * (int64_t)nz + ((m >> 2) & 1);
}

__global__ __launch_bounds__(TET_BLOCK) void tet_classify_kernel(McGrid g, TetWs w) {
  __shared__ int s[TET_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * TET_BLOCK + threadIdx.x;
  int nv = 0, ne = 0, nb = 0;
  if (p < g.npts) {
    int idx[3];
    grid_ijk(p, g.ny, g.nz, idx[0], idx[1], idx[2]);
    const int dims[3] = {g.nx, g.ny, g.nz};
    const int64_t syz = (int64_t)g.ny * g.nz;
    const bool h[3] = {idx[0] + 1 < g.nx, idx[1] + 1 < g.ny, idx[2] + 1 < g.nz};
    uint32_t cs = 0;                       // inside bits of the (up to) eight points p + d(m) that lie in the grid
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const bool ok = (!(m & 1) || h[0]) && (!(m & 2) || h[1]) && (!(m & 4) || h[2]);
      if (ok) cs |= (uint32_t)(g.sdf[p + tet_offset(m, syz, g.nz)] < g.level) << m;
    }
    uint32_t rec = cs & 1u;
#pragma unroll
    for (int c = 1; c < 8; ++c) {
      const bool ok = (!(c & 1) || h[0]) && (!(c & 2) || h[1]) && (!(c & 4) || h[2]);
      if (ok && ((cs >> c) & 1u) != (cs & 1u)) rec |= 1u << c;
    }
    if (h[0] && h[1] && h[2] && cs) {
#pragma unroll
      for (int pi = 0; pi < 6; ++pi) {
        int in[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) in[r] = (cs >> tet_corner(pi, r)) & 1;
        const int n = in[0] + in[1] + in[2] + in[3];
        ne += tet_n_elems(n);
        nb += tet_n_cut(n);
        if (idx[tet_axis(pi, 2)] == 0) nb += tet_n_plane(in[0] + in[1] + in[2]);
        if (idx[tet_axis(pi, 0)] == dims[tet_axis(pi, 0)] - 2) nb += tet_n_plane(in[1] + in[2] + in[3]);
      }
    }
    w.rec[p] = (uint8_t)rec;
    w.ne[p] = (uint8_t)ne;
    w.nb[p] = (uint8_t)nb;
    nv = __popc(rec);
  }
  const int tv = block_scan_incl<int, TET_BLOCK>(nv, s);
  __syncthreads();
  const int tf = block_scan_incl<int, TET_BLOCK>(ne | (nb << 16), s);
  if (threadIdx.x == TET_BLOCK - 1) {
    w.bcount[0][blockIdx.x] = tv;
    w.bcount[1][blockIdx.x] = tf & 0xFFFF;
    w.bcount[2][blockIdx.x] = tf >> 16;
  }
}

__global__ __launch_bounds__(TET_BLOCK) void tet_vertex_kernel(McGrid g, TetWs w, TetOut o) {
  __shared__ int s[TET_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * TET_BLOCK + threadIdx.x;
  const uint32_t rec = p < g.npts ? w.rec[p] : 0u;
  const int n = __popc(rec);
  const int inc = block_scan_incl<int, TET_BLOCK>(n, s);
  if (p >= g.npts) return;
  int64_t id = w.boff[0][blockIdx.x] + inc - n;
  w.vbase[p] = (int32_t)id;            // the host refuses totals above INT32_MAX before this launch
  if (!rec) return;
  int idx[3];
  grid_ijk(p, g.ny, g.nz, idx[0], idx[1], idx[2]);
  const int64_t syz = (int64_t)g.ny * g.nz;
  const float v0 = g.sdf[p];
  for (int c = 0; c < 8; ++c) {
    if (!((rec >> c) & 1u)) continue;
    float t = 0.f;
    if (c) {
      const float v1 = g.sdf[p + tet_offset(c, syz, g.nz)];
      // v0 and v1 lie on different sides of the level, so v1 != v0.  Every operation rounds on its own (the rn_* helpers of
      // common.hpp), in mc_vertex_kernel's sequence: a class-1/2/4 vertex has that kernel's bits.
      t = rn_div(rn_sub(g.level, v0), rn_sub(v1, v0));
      // The clamp is compare-and-select, not fminf(fmaxf()): those return the other operand for a NaN, and a NaN t (a NaN grid
      // value, an edge from -inf to +inf) has to stay NaN under every t_clamp, as in ms_caps_kernel.  For every other t the two
      // forms give the same bits.
      if (o.t_clamp > 0.f) {
        const float hi = rn_sub(1.f, o.t_clamp);
        t = t < o.t_clamp ? o.t_clamp : t;
        t = t > hi ? hi : t;
      }
    }
    if (id < o.nv) {
      float* out = o.verts + id * 3;
      for (int b = 0; b < 3; ++b) {
        const float x = ((c >> b) & 1) ? rn_add((float)idx[b], t) : (float)idx[b];
        out[b] = rn_add(o.origin[b], rn_mul(x, o.spacing[b]));
      }
      if (o.vert_point) o.vert_point[id] = p;
      if (o.vert_class) o.vert_class[id] = c;
    }
    ++id;
  }
}

// ---- elements -------------------------------------------------------------------------------------------------------------------
struct TetEmit {
  int32_t* tets;
  int32_t* bfaces;
  int8_t* kind;
  int64_t nt, nb;     // buffer sizes
  int64_t te, be;     // next element / boundary triangle
};

// (v0, v1, v2, v3) of orientation sgn, stored positive
__device__ __forceinline__ void tet_put(TetEmit& E, int v0, int v1, int v2, int v3, int sgn) {
  if (E.te < E.nt) *reinterpret_cast<int4*>(E.tets + E.te * 4) = sgn > 0 ? make_int4(v0, v1, v2, v3) : make_int4(v0, v1, v3, v2);
  ++E.te;
}

__device__ __forceinline__ void tet_put_tri(TetEmit& E, int a, int b, int c, int kind) {
  if (E.be < E.nb) {
    int32_t* out = E.bfaces + E.be * 3;
    out[0] = a; out[1] = b; out[2] = c;
    E.kind[E.be] = (int8_t)kind;
  }
  ++E.be;
}

// The prism (a0, a1, a2 | b0, b1, b2), vertical edges ai-bi, whose tetrahedron (a0, a1, a2, b0) has orientation sgn: relabelled so
// that a0 is its lowest id (exchanging the triangles flips sgn, rotating them does not), then every quadrilateral's diagonal
// leaves from its lowest id.  Ids are distinct.
__device__ __forceinline__ void tet_put_prism(TetEmit& E, int a0, int a1, int a2, int b0, int b1, int b2, int sgn) {
  const int ma = min(a0, min(a1, a2)), mb = min(b0, min(b1, b2));
  if (mb < ma) {
    int t;
    t = a0; a0 = b0; b0 = t;
    t = a1; a1 = b1; b1 = t;
    t = a2; a2 = b2; b2 = t;
    sgn = -sgn;
  }
  const int m = min(ma, mb);
  if (a1 == m) {
    int t;
    t = a0; a0 = a1; a1 = a2; a2 = t;
    t = b0; b0 = b1; b1 = b2; b2 = t;
  } else if (a2 == m) {
    int t;
    t = a2; a2 = a1; a1 = a0; a0 = t;
    t = b2; b2 = b1; b1 = b0; b0 = t;
  }
  tet_put(E, a0, b0, b1, b2, sgn);
  const int q = min(min(a1, a2), min(b1, b2));
  if (q == a1 || q == b2) {
    tet_put(E, a0, a1, a2, b2, sgn);
    tet_put(E, a0, a1, b2, b1, sgn);
  } else {
    tet_put(E, a0, a1, a2, b1, sgn);
    tet_put(E, a0, a2, b2, b1, sgn);
  }
}

// An oriented polygon of n = 3 or 4 ids: a quadrilateral is rotated to its lowest id, its diagonal leaves from there.
__device__ __forceinline__ void tet_put_poly(TetEmit& E, int u0, int u1, int u2, int u3, int n, int kind) {
  if (n == 3) {
    tet_put_tri(E, u0, u1, u2, kind);
    return;
  }
  const int m = min(min(u0, u1), min(u2, u3));
  int t;
  if (u1 == m) { t = u0; u0 = u1; u1 = u2; u2 = u3; u3 = t; }
  else if (u2 == m) { t = u0; u0 = u2; u2 = t; t = u1; u1 = u3; u3 = t; }
  else if (u3 == m) { t = u3; u3 = u2; u2 = u1; u1 = u0; u0 = t; }
  tet_put_tri(E, u0, u1, u2, kind);
  tet_put_tri(E, u0, u2, u3, kind);
}

// sign of the arrangement (a, b, c, d) of {0, 1, 2, 3}
__device__ __forceinline__ int tet_parity(int a, int b, int c, int d) {
  const int inv = (a > b) + (a > c) + (a > d) + (b > c) + (b > d) + (c > d);
  return (inv & 1) ? -1 : 1;
}

// The inside part of face (X, Y, Z) (corner numbers, outward order) of a Kuhn tetrahedron: walk round it, keep inside corners and
// crossing-edge vertices.
__device__ __forceinline__ void tet_put_face(TetEmit& E, const int* gid, const int (*eid)[4], const int* in, int X, int Y, int Z, int kind) {
  const int f[3] = {X, Y, Z};
  int u[6], n = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int a = f[r], b = f[(r + 1) % 3];
    if (in[a]) u[n++] = gid[a];
    if (in[a] != in[b]) u[n++] = eid[a][b];
  }
  if (n) tet_put_poly(E, u[0], u[1], u[2], n == 4 ? u[3] : 0, n, kind);
}

__global__ __launch_bounds__(TET_BLOCK) void tet_element_kernel(McGrid g, TetWs w, TetOut o) {
  __shared__ int s[TET_BLOCK];
  const int64_t p = (int64_t)blockIdx.x * TET_BLOCK + threadIdx.x;
  const int ne = p < g.npts ? w.ne[p] : 0, nb = p < g.npts ? w.nb[p] : 0;
  const int inc = block_scan_incl<int, TET_BLOCK>(ne | (nb << 16), s);
  if (p >= g.npts || (ne == 0 && nb == 0)) return;    // ne + nb > 0 only at the lower corner of a cell: p + d(7) is in the grid
  TetEmit E;
  E.tets = o.tets; E.bfaces = o.bfaces; E.kind = o.bface_kind; E.nt = o.nt; E.nb = o.nb;
  E.te = w.boff[1][blockIdx.x] + (inc & 0xFFFF) - ne;
  E.be = w.boff[2][blockIdx.x] + (inc >> 16) - nb;
  int idx[3];
  grid_ijk(p, g.ny, g.nz, idx[0], idx[1], idx[2]);
  const int dims[3] = {g.nx, g.ny, g.nz};
  const int64_t syz = (int64_t)g.ny * g.nz;
  int vb[8];
  uint32_t rc[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int64_t q = p + tet_offset(m, syz, g.nz);
    vb[m] = w.vbase[q];
    rc[m] = w.rec[q];
  }
#pragma unroll
  for (int pi = 0; pi < 6; ++pi) {
    const int sg = tet_sign(pi);
    int in[4], gid[4], eid[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      in[r] = rc[tet_corner(pi, r)] & 1u;
      gid[r] = vb[tet_corner(pi, r)];
    }
    const int n = in[0] + in[1] + in[2] + in[3];
    if (n == 0) continue;
    // the id of edge vertex (lower corner r0, class c); meaningful only where the edge crosses, read only there
#pragma unroll
    for (int r0 = 0; r0 < 4; ++r0) {
      eid[r0][r0] = 0;
#pragma unroll
      for (int r1 = r0 + 1; r1 < 4; ++r1) {
        const int c = tet_corner(pi, r1) ^ tet_corner(pi, r0);
        eid[r0][r1] = eid[r1][r0] = vb[tet_corner(pi, r0)] + __popc(rc[tet_corner(pi, r0)] & ((1u << c) - 1u));
      }
    }
    if (n == 4) {
      tet_put(E, gid[0], gid[1], gid[2], gid[3], sg);
    } else {
      int I[4], O[4], ni = 0, no = 0;        // inside / outside corners in increasing order
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (in[r]) I[ni++] = r;
        else O[no++] = r;
      }
      if (n == 1) {
        const int A = I[0], B = O[0], C = O[1], D = O[2];
        const int sgn = sg * tet_parity(A, B, C, D);
        const int x = eid[A][B], y = sgn > 0 ? eid[A][C] : eid[A][D], z = sgn > 0 ? eid[A][D] : eid[A][C];
        tet_put(E, gid[A], x, y, z, 1);
        tet_put_tri(E, x, y, z, 0);
      } else if (n == 3) {
        const int A = I[0], B = I[1], C = I[2], D = O[0];
        const int sgn = sg * tet_parity(A, B, C, D);
        const int b0 = eid[A][D], b1 = eid[B][D], b2 = eid[C][D];
        tet_put_prism(E, gid[A], gid[B], gid[C], b0, b1, b2, sgn);
        tet_put_tri(E, b0, sgn > 0 ? b1 : b2, sgn > 0 ? b2 : b1, 0);
      } else {
        const int A = I[0], B = I[1], C = O[0], D = O[1];
        const int sgn = sg * tet_parity(A, C, D, B);
        const int a1 = eid[A][C], a2 = eid[A][D], b1 = eid[B][C], b2 = eid[B][D];
        tet_put_prism(E, gid[A], a1, a2, gid[B], b1, b2, sgn);
        if (sgn > 0) tet_put_poly(E, a1, a2, b2, b1, 4, 0);
        else tet_put_poly(E, a1, b1, b2, a2, 4, 0);
      }
    }
    // the two faces that can lie in an outer plane of the grid: (q0, q1, q2) in the low plane of axis pi2 (normal sign(pi) e_pi2),
    // (q1, q2, q3) in the high plane of axis pi0 (normal sign(pi) e_pi0)
    if (idx[tet_axis(pi, 2)] == 0) {
      if (sg < 0) tet_put_face(E, gid, eid, in, 0, 1, 2, 1 + 2 * tet_axis(pi, 2));
      else tet_put_face(E, gid, eid, in, 0, 2, 1, 1 + 2 * tet_axis(pi, 2));
    }
    if (idx[tet_axis(pi, 0)] == dims[tet_axis(pi, 0)] - 2) {
      if (sg > 0) tet_put_face(E, gid, eid, in, 1, 2, 3, 2 + 2 * tet_axis(pi, 0));
      else tet_put_face(E, gid, eid, in, 1, 3, 2, 2 + 2 * tet_axis(pi, 0));
    }
  }
}

// ---- components -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TET_BLOCK) void tet_cc_init_kernel(McGrid g, int32_t* __restrict__ f) {
  const int64_t u = (int64_t)blockIdx.x * TET_BLOCK + threadIdx.x;
  if (u < g.npts) f[u] = g.sdf[u] < g.level ? (int32_t)u : -1;
}

// mt_cc_hook_kernel over the grid: u's neighbours are u +- d(c), c = 1..7, inside the grid and inside the solid (gf >= 0).
__global__ __launch_bounds__(TET_BLOCK) void tet_cc_hook_kernel(McGrid g, int32_t* f, const int32_t* __restrict__ gf,
                                                                int32_t* __restrict__ flag) {
  const int64_t u = (int64_t)blockIdx.x * TET_BLOCK + threadIdx.x;
  if (u >= g.npts) return;
  int best = gf[u];
  if (best < 0) return;
  const int64_t fu = clamp_index(f[u], g.npts);
  int idx[3];
  grid_ijk(u, g.ny, g.nz, idx[0], idx[1], idx[2]);
  const int64_t syz = (int64_t)g.ny * g.nz;
  bool changed = false;
  for (int c = 1; c < 8; ++c) {
    const int d[3] = {c & 1, (c >> 1) & 1, (c >> 2) & 1};
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      const int i = idx[0] + sgn * d[0], j = idx[1] + sgn * d[1], k = idx[2] + sgn * d[2];
      if (i < 0 || j < 0 || k < 0 || i >= g.nx || j >= g.ny || k >= g.nz) continue;
      const int gv = gf[u + sgn * tet_offset(c, syz, g.nz)];
      if (gv < 0) continue;
      changed |= cc_lower(f, fu, gv);
      best = gv < best ? gv : best;
    }
  }
  changed |= cc_lower(f, u, best);
  if (changed) *flag = 1;
}

}  // namespace dsdf
