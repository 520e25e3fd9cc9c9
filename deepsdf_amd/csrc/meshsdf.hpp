// meshsdf.hpp -- signed distance from points to a triangle mesh on the device (gfx950): brute force over every face.
//
// Per query p (spec: include/dsdf.h, restated in fp64 by tests/meshsdf_numpy.py):
//   d2     min over faces of |p - c_f|^2, c_f the closest point of the closed triangle, the difference vector formed explicitly;
//          ties go to the lowest face index
//   w      sum over faces of the Van Oosterom-Strackee solid angle / 4 pi
//   sdf    inside (floor(|w| + 0.5) odd) ? -sqrt(d2) : sqrt(d2), negated when flip_sign
//
// Passes:
//   1. prepare: one thread per face turns (V, F) into a 64-byte MsdfTri record (vertex a, edges ab / ac, the reciprocal squared
//               edge lengths, the unit normal and its length -- the normal in fp64); face indices are clamped into [0, nv); a
//               zero-area face becomes its longest edge and adds no winding
//   2. query:   one query per lane, MSDF_BLOCK lanes per workgroup; blockIdx.y takes one contiguous face range (split).
//               The face loop is wave-uniform: every lane reads the same record, which the compiler loads through the
//               scalar unit (const __restrict__, uniform index).  The pair test is branch-free (Voronoi regions by selects
//               between the three clamped edges and the plane foot), accurate to ~1e-7 of |p - a| whatever the face's
//               shape (msdf_face_d2).
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
  float4 a;      // vertex a, w = 1 / |ab|^2
  float4 ab;     // b - a, w = 1 / |ac|^2
  float4 ac;     // c - a, w = 1 / |bc|^2 (bc = ac - ab as the query pass forms it); the reciprocal of a zero length is stored as 0
  float4 aux;    // x = |ab x ac|, or 0 for a zero-area face (adds no winding); y, z, w = the unit normal (ab x ac) / x; from fp64
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
  // once per face, so in fp64: the normal of a sliver is a difference of nearly equal products (its fp32 value is noise once the
  // height falls below ~1e-4 of the longest edge), and the zero-area test reads the same quantity
  const double ex[3] = {(double)v[1].x - v[0].x, (double)v[1].y - v[0].y, (double)v[1].z - v[0].z};
  const double fx[3] = {(double)v[2].x - v[0].x, (double)v[2].y - v[0].y, (double)v[2].z - v[0].z};
  const double gx[3] = {(double)v[2].x - v[1].x, (double)v[2].y - v[1].y, (double)v[2].z - v[1].z};
  const double lab = ex[0] * ex[0] + ex[1] * ex[1] + ex[2] * ex[2], lac = fx[0] * fx[0] + fx[1] * fx[1] + fx[2] * fx[2];
  const double lbc = gx[0] * gx[0] + gx[1] * gx[1] + gx[2] * gx[2];
  const double n[3] = {ex[1] * fx[2] - ex[2] * fx[1], ex[2] * fx[0] - ex[0] * fx[2], ex[0] * fx[1] - ex[1] * fx[0]};
  const double nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  const double lmax = fmax(lab, fmax(lac, lbc));
  // zero area (height below ~1e-7 of the longest edge): the face is its longest edge, stored as the triangle (p, q, p) -- its
  // three edges are then that segment twice and the point p --, and the face has no normal and adds no winding
  const bool degen = nn <= 1e-14 * lmax * lmax;
  float ln = 0.f;
  float3 nh = make_float3(0.f, 0.f, 0.f);
  if (degen) {
    if (lbc >= lab && lbc >= lac) { a = v[1]; ab = f3sub(v[2], v[1]); }
    else if (lac >= lab) { ab = ac; }
    ac = make_float3(0.f, 0.f, 0.f);
  } else {
    const double rn = 1.0 / sqrt(nn);
    ln = (float)sqrt(nn);
    nh = make_float3((float)(n[0] * rn), (float)(n[1] * rn), (float)(n[2] * rn));
  }
  // reciprocal squared lengths of the edges as the query pass sees them (fp32 vectors; bc by the same fp32 subtraction)
  const float3 bc = f3sub(ac, ab);
  const double l2[3] = {(double)ab.x * ab.x + (double)ab.y * ab.y + (double)ab.z * ab.z,
                        (double)ac.x * ac.x + (double)ac.y * ac.y + (double)ac.z * ac.z,
                        (double)bc.x * bc.x + (double)bc.y * bc.y + (double)bc.z * bc.z};
  MsdfTri t;
  t.a = make_float4(a.x, a.y, a.z, l2[0] > 0.0 ? (float)(1.0 / l2[0]) : 0.f);
  t.ab = make_float4(ab.x, ab.y, ab.z, l2[1] > 0.0 ? (float)(1.0 / l2[1]) : 0.f);
  t.ac = make_float4(ac.x, ac.y, ac.z, l2[2] > 0.0 ? (float)(1.0 / l2[2]) : 0.f);
  t.aux = make_float4(ln, nh.x, nh.y, nh.z);
  tri[f] = t;
}

// Squared distance from p to the closed triangle (ap = p - a) and the closest point minus a, in `rel`.  Ericson's seven regions
// (Real-Time Collision Detection 5.1.5) in his order -- A, B, AB, C, AC, BC, interior, first match wins --, from quantities that
// keep their meaning on a sliver: the unclamped parameters u = (p - s).e / |e|^2 of the three edges, and the side of each edge
// the foot of the perpendicular falls on, s = n^.(e x (p - s)) with the unit normal of the prepare pass.  Ericson's own va, vb,
// vc are |n|^2 times a barycentric coordinate computed from products of O(1) dot products, noise once |n|^2 nears 1e-7 (a height of
// 1e-3 of the longest edge gives 1e-6); here every deciding quantity is a length or a signed area with an error of ~1e-7 of |ap|
// whatever the shape, neighbouring regions return neighbouring points, so a test that rounding gets wrong moves the answer by
// that error and no more.  The vertex tests come first: a needle's side tests alone pass up to error / sin(apex / 2) beyond its
// tip.  A vertex or edge region yields the clamped point of one edge (A, B, AB: ab; C, AC: ac; BC: bc) and the distance from
// the residual (p - s) - t e; the interior the plane foot ap - (ap.n^) n^ and (ap.n^)^2.  A zero-area face is the segment ab.
// Branch-free, no reciprocal: the regions are resolved by selects.
__device__ __forceinline__ float msdf_face_d2(const MsdfTri& t, float3 ap, float3& rel) {
  const float3 ab = make_float3(t.ab.x, t.ab.y, t.ab.z), ac = make_float3(t.ac.x, t.ac.y, t.ac.z);
  const float3 nh = make_float3(t.aux.y, t.aux.z, t.aux.w);
  const float3 bc = f3sub(ac, ab), bp = f3sub(ap, ab);
  const float uab = f3dot(ap, ab) * t.a.w, uac = f3dot(ap, ac) * t.ab.w, ubc = f3dot(bp, bc) * t.ac.w;
  const float sab = f3dot(nh, f3cross(ab, ap)), sac = f3dot(nh, f3cross(ap, ac)), sbc = f3dot(nh, f3cross(bc, bp));
  const bool rA = uab <= 0.f && uac <= 0.f, rB = uab >= 1.f && ubc <= 0.f, rC = uac >= 1.f && ubc >= 1.f;
  const bool rAB = sab <= 0.f && uab >= 0.f && uab <= 1.f, rAC = sac <= 0.f && uac >= 0.f && uac <= 1.f;
  const bool rBC = sbc <= 0.f && ubc >= 0.f && ubc <= 1.f;
  const bool on_ab = rA || rB || rAB || !(t.aux.x > 0.f);
  const bool on_ac = !on_ab && (rC || rAC);
  const bool on_bc = !on_ab && !on_ac && rBC;
  const bool inside = !on_ab && !on_ac && !on_bc;
  // the edge: its start relative to a (0 or ab), the query relative to that start, its direction and the clamped parameter
  const float3 s0 = on_bc ? ab : make_float3(0.f, 0.f, 0.f), sp = on_bc ? bp : ap;
  const float3 e = on_ab ? ab : (on_ac ? ac : bc);
  const float u = on_ab ? uab : (on_ac ? uac : ubc);
  const float tc = fminf(fmaxf(u, 0.f), 1.f);
  const float3 r = make_float3(fmaf(-tc, e.x, sp.x), fmaf(-tc, e.y, sp.y), fmaf(-tc, e.z, sp.z));
  const float h = f3dot(ap, nh);
  rel = inside ? make_float3(fmaf(-h, nh.x, ap.x), fmaf(-h, nh.y, ap.y), fmaf(-h, nh.z, ap.z))
               : make_float3(fmaf(tc, e.x, s0.x), fmaf(tc, e.y, s0.y), fmaf(tc, e.z, s0.z));
  return inside ? h * h : f3dot(r, r);
}

// sqrt of x >= 0 to fp64 accuracy without the fp64 square-root sequence: the fp32 root, then one Newton step in fp64 (the
// reciprocal it needs only has to be good to fp32).  x = 0 (a query on a vertex) gives 0.
__device__ __forceinline__ double msdf_sqrt(double x) {
  const float sf = __builtin_sqrtf((float)x);
  const double s = (double)sf;
  const double y = fma(fma(-s, s, x), (double)(0.5f * __builtin_amdgcn_rcpf(sf)), s);
  return sf > 0.f ? y : 0.0;
}

// Signed solid angle of the face seen from p (Van Oosterom & Strackee 1983), halved: atan2(a.(b x c), |a||b||c| + (a.b)|c| +
// (b.c)|a| + (c.a)|b|) with a, b, c the vertices minus p.  Both arguments cancel when p is close to the face's plane compared
// with the face's size -- always, next to a sliver -- and the angle is their ratio, so neither is formed from fp32 products:
//   the numerator a.(b x c) equals a.(ab x ac), which is -|n| (ap . n^) with the prepare pass's normal (relative error ~1e-7);
//   the denominator is summed in fp64 from the fp32 vectors (its terms cancel to ~(height / size)^2 of their size).
// Zero-area faces (|n| stored as 0) add nothing, and neither does a face seen from one of its own vertices.
__device__ __forceinline__ float msdf_half_solid_angle(const MsdfTri& t, float3 ap) {
  const float det = -t.aux.x * (ap.x * t.aux.y + ap.y * t.aux.z + ap.z * t.aux.w);
  const double ax = -(double)ap.x, ay = -(double)ap.y, az = -(double)ap.z;
  const double bx = ax + (double)t.ab.x, by = ay + (double)t.ab.y, bz = az + (double)t.ab.z;
  const double cx = ax + (double)t.ac.x, cy = ay + (double)t.ac.y, cz = az + (double)t.ac.z;
  const double la = msdf_sqrt(ax * ax + ay * ay + az * az), lb = msdf_sqrt(bx * bx + by * by + bz * bz);
  const double lc = msdf_sqrt(cx * cx + cy * cy + cz * cz);
  const double ab = ax * bx + ay * by + az * bz, bc = bx * cx + by * cy + bz * cz, ca = cx * ax + cy * ay + cz * az;
  const double den = la * lb * lc + ab * lc + bc * la + ca * lb;
  // a zero-area face, or p on a vertex (where the angle is undefined and the numerator is +-0): atan2(+-0, 1) = +-0, never the
  // +-pi that a denominator of rounding's sign would give; selected, so that the loop stays branch-free
  const bool live = t.aux.x > 0.f && la > 0.0 && lb > 0.0 && lc > 0.0;
  return atan2f(live ? det : 0.f, live ? (float)den : 1.f);
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
      float3 rel;
      const float d2 = msdf_face_d2(t, ap, rel);
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
    float3 rel;
    msdf_face_d2(t, make_float3(p.x - t.a.x, p.y - t.a.y, p.z - t.a.z), rel);
    out.closest[(int64_t)q * 3] = t.a.x + rel.x;
    out.closest[(int64_t)q * 3 + 1] = t.a.y + rel.y;
    out.closest[(int64_t)q * 3 + 2] = t.a.z + rel.z;
  }
  if (out.sdf) {
    const bool inside = ((int64_t)floorf(fabsf(w) + 0.5f)) & 1;
    float d = __builtin_sqrtf(best);
    d = inside ? -d : d;
    out.sdf[q] = out.flip ? -d : d;
  }
}

}  // namespace dsdf
