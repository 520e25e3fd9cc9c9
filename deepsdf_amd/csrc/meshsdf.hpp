// meshsdf.hpp -- signed distance from points to a triangle mesh on the device (gfx950): brute force over every face.
//
// Per query p (spec: include/dsdf.h, restated in fp64 by tests/meshsdf_numpy.py):
//   d2     min over faces of |p - c_f|^2, c_f the closest point of the closed triangle (Ericson, Real-Time Collision
//          Detection 5.1.5), the difference vector formed explicitly; ties go to the lowest face index
//   w      sum over faces of the Van Oosterom-Strackee solid angle / 4 pi
//   sdf    inside (floor(|w| + 0.5) odd) ? -sqrt(d2) : sqrt(d2), negated when flip_sign
//
// Passes:
//   1. prepare: one thread per face turns (V, F) into a 64-byte MsdfTri record (vertex a, edges ab / ac, their dot products);
//               face indices are clamped into [0, nv); a zero-area face becomes its longest edge and adds no winding
//   2. query:   one query per lane, MSDF_BLOCK lanes per workgroup; blockIdx.y takes one contiguous face range (split).
//               The face loop is wave-uniform: every lane reads the same record, which the compiler loads through the
//               scalar unit (const __restrict__, uniform index).  The pair test is branch-free (Voronoi regions by selects).
//               Per split and query: the best d2, its face and the split's winding sum go to the workspace.
//   3. combine: one thread per query walks the splits in order (strict < keeps the lowest face on ties, winding summed in
//               split order), recomputes the closest point of the winning face and writes the requested outputs.
// No atomics anywhere: d2, face and closest point do not depend on the split; two calls give identical bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsdf {

constexpr int MSDF_BLOCK = 256;
constexpr int MSDF_PREP_BLOCK = 256;
constexpr int MSDF_TARGET_WG = 2048;          // workgroups a query launch aims for (8 per CU) before it stops splitting faces
constexpr int MSDF_MIN_SPLIT_FACES = 1024;    // no split gets fewer faces than this
constexpr int MSDF_MAX_SPLITS = 64;

struct __align__(16) MsdfTri {
  float4 a;      // vertex a, w = ab.ab
  float4 ab;     // b - a, w = ab.ac
  float4 ac;     // c - a, w = ac.ac
  float4 aux;    // x = 1 (counts in the winding number) or 0 (zero-area face); y, z, w unused
};

struct MsdfPartial {     // carved from the caller's workspace: [n_splits][nq] each
  float* d2;
  int32_t* face;
  float* wind;
};

__device__ __forceinline__ float3 f3sub(float3 x, float3 y) { return make_float3(x.x - y.x, x.y - y.y, x.z - y.z); }
__device__ __forceinline__ float f3dot(float3 x, float3 y) { return x.x * y.x + x.y * y.y + x.z * y.z; }
__device__ __forceinline__ float3 f3cross(float3 x, float3 y) {
  return make_float3(x.y * y.z - x.z * y.y, x.z * y.x - x.x * y.z, x.x * y.y - x.y * y.x);
}

__global__ __launch_bounds__(MSDF_PREP_BLOCK) void msdf_prepare_kernel(const float* __restrict__ V, int nv,
                                                                       const int32_t* __restrict__ F, int nf,
                                                                       MsdfTri* __restrict__ tri) {
  const int f = blockIdx.x * MSDF_PREP_BLOCK + threadIdx.x;
  if (f >= nf) return;
  float3 v[3];
  for (int r = 0; r < 3; ++r) {
    int i = F[(int64_t)f * 3 + r];
    i = i < 0 ? 0 : (i >= nv ? nv - 1 : i);            // the host range-checks; this only keeps reads inside V
    v[r] = make_float3(V[(int64_t)i * 3], V[(int64_t)i * 3 + 1], V[(int64_t)i * 3 + 2]);
  }
  float3 a = v[0], ab = f3sub(v[1], v[0]), ac = f3sub(v[2], v[0]);
  const float3 bc = f3sub(v[2], v[1]);
  const float lab = f3dot(ab, ab), lac = f3dot(ac, ac), lbc = f3dot(bc, bc);
  const float3 n = f3cross(ab, ac);
  const float lmax = fmaxf(lab, fmaxf(lac, lbc));
  // zero area (to fp32 resolution: height below ~1e-7 of the longest edge): the face is its longest edge, stored as the
  // triangle (p, q, p) -- Ericson's regions then reduce to the segment's, and the face adds no winding
  const bool degen = f3dot(n, n) <= 1e-14f * lmax * lmax;
  float wt = 1.f;
  if (degen) {
    wt = 0.f;
    if (lbc >= lab && lbc >= lac) { a = v[1]; ab = bc; }
    else if (lac >= lab) { ab = ac; }
    ac = make_float3(0.f, 0.f, 0.f);
  }
  MsdfTri t;
  t.a = make_float4(a.x, a.y, a.z, f3dot(ab, ab));
  t.ab = make_float4(ab.x, ab.y, ab.z, f3dot(ab, ac));
  t.ac = make_float4(ac.x, ac.y, ac.z, f3dot(ac, ac));
  t.aux = make_float4(wt, 0.f, 0.f, 0.f);
  tri[f] = t;
}

// Barycentric (v, w) of the closest point a + v ab + w ac of the closed triangle to p (ap = p - a).  Ericson's region tests in
// his order -- A, B, AB, C, AC, BC, interior, first match wins -- evaluated for all regions and resolved by selects, so lanes in
// different regions run the same instructions.  One reciprocal serves whichever region needs a quotient.
__device__ __forceinline__ void msdf_closest_bary(const MsdfTri& t, float3 ap, float& v, float& w) {
  const float3 ab = make_float3(t.ab.x, t.ab.y, t.ab.z), ac = make_float3(t.ac.x, t.ac.y, t.ac.z);
  const float d1 = f3dot(ab, ap), d2 = f3dot(ac, ap);
  const float d3 = d1 - t.a.w, d4 = d2 - t.ab.w;         // ab.bp, ac.bp  (bp = ap - ab)
  const float d5 = d1 - t.ab.w, d6 = d2 - t.ac.w;        // ab.cp, ac.cp  (cp = ap - ac)
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  const bool rA = d1 <= 0.f && d2 <= 0.f;
  const bool rB = d3 >= 0.f && d4 <= d3;
  const bool rAB = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
  const bool rC = d6 >= 0.f && d5 <= d6;
  const bool rAC = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
  const bool rBC = va <= 0.f && e43 >= 0.f && e56 >= 0.f;
  // quotient of the edge regions (num / den), or 1 / (va + vb + vc) inside; later selects take precedence
  float num = 1.f, den = va + vb + vc;
  num = rBC ? e43 : num;  den = rBC ? e43 + e56 : den;
  num = rAC ? d2 : num;   den = rAC ? d2 - d6 : den;
  num = rAB ? d1 : num;   den = rAB ? d1 - d3 : den;
  const float q = num * __builtin_amdgcn_rcpf(den);
  float vv = vb * q, ww = vc * q;                         // interior (num = 1)
  vv = rBC ? 1.f - q : vv;  ww = rBC ? q : ww;
  vv = rAC ? 0.f : vv;      ww = rAC ? q : ww;
  vv = rC ? 0.f : vv;       ww = rC ? 1.f : ww;
  vv = rAB ? q : vv;        ww = rAB ? 0.f : ww;
  vv = rB ? 1.f : vv;       ww = rB ? 0.f : ww;
  vv = rA ? 0.f : vv;       ww = rA ? 0.f : ww;
  // a region test that rounding left unmatched with a vanishing denominator: fall back to vertex a rather than NaN
  const bool bad = !(__builtin_isfinite(vv) && __builtin_isfinite(ww));
  v = bad ? 0.f : vv;
  w = bad ? 0.f : ww;
}

__device__ __forceinline__ float3 msdf_point(const MsdfTri& t, float v, float w) {
  return make_float3(fmaf(t.ac.x, w, fmaf(t.ab.x, v, t.a.x)), fmaf(t.ac.y, w, fmaf(t.ab.y, v, t.a.y)),
                     fmaf(t.ac.z, w, fmaf(t.ab.z, v, t.a.z)));
}

// Signed solid angle of the face seen from p (Van Oosterom & Strackee 1983), halved: atan2(a.(b x c), |a||b||c| + (a.b)|c| +
// (b.c)|a| + (c.a)|b|) with a, b, c the vertices minus p.
__device__ __forceinline__ float msdf_half_solid_angle(const MsdfTri& t, float3 ap) {
  const float3 a = make_float3(-ap.x, -ap.y, -ap.z);
  const float3 b = make_float3(a.x + t.ab.x, a.y + t.ab.y, a.z + t.ab.z);
  const float3 c = make_float3(a.x + t.ac.x, a.y + t.ac.y, a.z + t.ac.z);
  const float la = __builtin_sqrtf(f3dot(a, a)), lb = __builtin_sqrtf(f3dot(b, b)), lc = __builtin_sqrtf(f3dot(c, c));
  const float det = f3dot(a, f3cross(b, c));
  const float den = la * lb * lc + f3dot(a, b) * lc + f3dot(b, c) * la + f3dot(c, a) * lb;
  return t.aux.x * atan2f(det, den);
}

// Query pass.  DIST: track the closest face; WIND: sum the solid angles.  Split s = blockIdx.y covers faces
// [s * chunk, min(nf, (s + 1) * chunk)).
template <bool DIST, bool WIND>
__global__ __launch_bounds__(MSDF_BLOCK) void msdf_query_kernel(const MsdfTri* __restrict__ tri, int nf, int chunk,
                                                                const float* __restrict__ P, int nq, MsdfPartial part) {
  const int q = blockIdx.x * MSDF_BLOCK + threadIdx.x;
  const int qc = q < nq ? q : nq - 1;                   // tail lanes compute a duplicate and write nothing
  const float3 p = make_float3(P[(int64_t)qc * 3], P[(int64_t)qc * 3 + 1], P[(int64_t)qc * 3 + 2]);
  const int f0 = blockIdx.y * chunk;
  const int f1 = min(nf, f0 + chunk);
  float best = __builtin_inff();
  int bestf = f0;
  float wsum = 0.f, wcomp = 0.f;                        // compensated (Kahan) sum: the split changes w by ~1 ulp, not ~sqrt(nf)
  for (int f = f0; f < f1; ++f) {
    const MsdfTri t = tri[f];
    const float3 ap = make_float3(p.x - t.a.x, p.y - t.a.y, p.z - t.a.z);
    if (DIST) {
      float v, w;
      msdf_closest_bary(t, ap, v, w);
      const float3 c = msdf_point(t, v, w);
      const float3 d = f3sub(p, c);
      const float d2 = f3dot(d, d);
      const bool better = d2 < best;
      best = better ? d2 : best;
      bestf = better ? f : bestf;
    }
    if (WIND) {
      const float y = msdf_half_solid_angle(t, ap) - wcomp;
      const float s = wsum + y;
      wcomp = (s - wsum) - y;
      wsum = s;
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

struct MsdfOut {
  float* sdf;        // [nq]
  float* d2;         // [nq]
  int32_t* face;     // [nq]
  float* closest;    // [nq][3]
  float* winding;    // [nq]
  int flip;
};

__global__ __launch_bounds__(MSDF_BLOCK) void msdf_combine_kernel(const MsdfTri* __restrict__ tri, const float* __restrict__ P,
                                                                  int nq, int n_splits, int dist, int wind, MsdfPartial part,
                                                                  MsdfOut out) {
  const int q = blockIdx.x * MSDF_BLOCK + threadIdx.x;
  if (q >= nq) return;
  float best = __builtin_inff(), hw = 0.f;
  int bestf = 0;
  for (int s = 0; s < n_splits; ++s) {
    const int64_t o = (int64_t)s * nq + q;
    if (dist) {
      const float d2 = part.d2[o];
      if (d2 < best || s == 0) {
        best = d2;
        bestf = part.face[o];
      }
    }
    if (wind) hw += part.wind[o];
  }
  // sum of half solid angles / 2 pi = sum of solid angles / 4 pi
  const float w = hw * 0.15915494309189535f;
  if (out.d2) out.d2[q] = best;
  if (out.face) out.face[q] = bestf;
  if (out.winding) out.winding[q] = w;
  if (out.closest) {
    const float3 p = make_float3(P[(int64_t)q * 3], P[(int64_t)q * 3 + 1], P[(int64_t)q * 3 + 2]);
    const MsdfTri t = tri[bestf];
    float v, ww;
    msdf_closest_bary(t, make_float3(p.x - t.a.x, p.y - t.a.y, p.z - t.a.z), v, ww);
    const float3 c = msdf_point(t, v, ww);
    out.closest[(int64_t)q * 3] = c.x;
    out.closest[(int64_t)q * 3 + 1] = c.y;
    out.closest[(int64_t)q * 3 + 2] = c.z;
  }
  if (out.sdf) {
    const bool inside = ((int64_t)floorf(fabsf(w) + 0.5f)) & 1;
    float d = __builtin_sqrtf(best);
    d = inside ? -d : d;
    out.sdf[q] = out.flip ? -d : d;
  }
}

}  // namespace dsdf
