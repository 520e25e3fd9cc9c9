// fem.hpp -- P1 linear elasticity on a tetrahedral mesh (gfx950), matrix-free and fp64 throughout: the element geometry, the operator
// A = P K P + (I - P), its 3x3 block-Jacobi preconditioner, the boundary load, the kernels of a preconditioned CG whose scalars never
// leave the device, the strain energy density and the boundary (Hadamard) gradients.  The specification is in include/dsdf.h
// (dsdf_fem_*) and DESIGN 4.21; tests/fem_numpy.py restates it in numpy / scipy.
//
// One thread per element or per vertex, FEM_BLOCK per workgroup.  Nothing is scattered: a per-element pass writes what the element
// contributes, a per-vertex pass gathers it over the vertex's corners c = 4 e + a in the order of a stable sort of the corners by
// vertex.  There is no floating-point atomic; every sum over the mesh is block_tree_sum per workgroup and one fixed-order pass over
// the per-workgroup partials, so two runs give identical bytes.
//
// The element geometry (FEM_GEOM doubles: the gradients of the barycentric functions 1..3 and the volume) is computed ONCE with every
// operation rounded on its own (no contraction), in the order the numpy restatement uses: the stored values are the oracle's bits, so
// the rounding of the gradients cancels out of every comparison with it.  Everything downstream may contract.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "blockops.hpp"

namespace dsdf {

constexpr int FEM_BLOCK = 256;
constexpr int FEM_GEOM = 10;       // doubles per element, stored [FEM_GEOM][n_tets]: g1 (3), g2 (3), g3 (3), V
constexpr int FEM_NODAL_MEAN = 1, FEM_NODAL_LAST = 2;

struct FemMesh {                   // device view of an operator (DsdfFemOp)
  const int32_t* tets;             // [nt][4]
  const int64_t* corder;           // [4 nt] corners sorted by vertex (stable)
  const int64_t* vstart;           // [nv + 1]
  const double* geom;              // [FEM_GEOM][nt]
  const uint8_t* mask;             // [nv] 1: fixed or held (P zeroes it)
  int64_t nt, nv;
  double lam, mu;
};

struct FemScal {                   // the CG's scalars, device resident
  double rho, rho0, alpha, beta, pap, tol2;
  int32_t it, done, converged, pad;
};

__device__ __forceinline__ void fem_cross_rn(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The gradients of element e's four barycentric functions and its volume from the stored geometry; g0 = -((g1 + g2) + g3).
__device__ __forceinline__ double fem_grads(const double* __restrict__ geom, int64_t nt, int64_t e, double (*g)[3]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) g[1 + k / 3][k % 3] = geom[(int64_t)k * nt + e];
#pragma unroll
  for (int i = 0; i < 3; ++i) g[0][i] = -((g[1][i] + g[2][i]) + g[3][i]);
  return geom[(int64_t)9 * nt + e];
}

// Gradient a (0..3) of element e alone.
__device__ __forceinline__ void fem_grad_of(const double* __restrict__ geom, int64_t nt, int64_t e, int a, double* g) {
  if (a > 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = geom[(int64_t)(3 * (a - 1) + i) * nt + e];
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] = -((geom[(int64_t)i * nt + e] + geom[(int64_t)(3 + i) * nt + e]) + geom[(int64_t)(6 + i) * nt + e]);
  }
}

__device__ __forceinline__ void fem_corner_range(const int64_t* __restrict__ vstart, int64_t v, int64_t n, int64_t& lo, int64_t& hi) {
  lo = vstart[v]; hi = vstart[v + 1];
  lo = lo < 0 ? 0 : (lo > n ? n : lo);
  hi = hi < lo ? lo : (hi > n ? n : hi);
}

// ---- set-up -------------------------------------------------------------------------------------------------------------------
// Element e: e_k = x_k - x_0, c1 = e2 x e3, c2 = e3 x e1, c3 = e1 x e2, det = (e1.x c1.x + e1.y c1.y) + e1.z c1.z, V = det / 6,
// g_k = c_k / det.  V <= 0 (or not a number) or a non-finite gradient: the element is skipped -- stored as zeros, so that it adds an
// exact zero everywhere -- and counted.
__global__ __launch_bounds__(FEM_BLOCK) void fem_geom_kernel(const double* __restrict__ X, int64_t nv, const int32_t* __restrict__ tets,
                                                             int64_t nt, double* __restrict__ geom, int32_t* __restrict__ cnt_part) {
#pragma clang fp contract(off)
  __shared__ int sh[FEM_BLOCK];
  const int64_t e = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  int skipped = 0;
  if (e < nt) {
    const int4 id = *reinterpret_cast<const int4*>(tets + e * 4);
    const int64_t v[4] = {clamp_index(id.x, nv), clamp_index(id.y, nv), clamp_index(id.z, nv), clamp_index(id.w, nv)};
    double x[4][3], ed[3][3], c[3][3];
    for (int k = 0; k < 4; ++k)
      for (int i = 0; i < 3; ++i) x[k][i] = X[v[k] * 3 + i];
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < 3; ++i) ed[k][i] = x[k + 1][i] - x[0][i];
    fem_cross_rn(ed[1], ed[2], c[0]);
    fem_cross_rn(ed[2], ed[0], c[1]);
    fem_cross_rn(ed[0], ed[1], c[2]);
    const double det = (ed[0][0] * c[0][0] + ed[0][1] * c[0][1]) + ed[0][2] * c[0][2];
    const double V = det / 6.0;
    bool ok = V > 0.0;
    double g[9];
    for (int k = 0; k < 9; ++k) {
      g[k] = c[k / 3][k % 3] / det;
      ok = ok && isfinite(g[k]);
    }
    skipped = ok ? 0 : 1;
    for (int k = 0; k < 9; ++k) geom[(int64_t)k * nt + e] = ok ? g[k] : 0.0;
    geom[(int64_t)9 * nt + e] = ok ? V : 0.0;
  }
  const int tot = block_tree_sum<int, FEM_BLOCK>(skipped, sh);
  if (threadIdx.x == 0) cnt_part[blockIdx.x] = tot;
}

// Vertex v: D = sum over its corners of K_aa = V ((lam + mu) g g^T + mu (g.g) I), six values (xx, yy, zz, xy, xz, yz), and its inverse
// by the adjugate.  A vertex with no element that counts is held (counted); held and fixed vertices get mask 1 and the identity.
__global__ __launch_bounds__(FEM_BLOCK) void fem_diag_kernel(FemMesh m, const uint8_t* __restrict__ fixed, double* __restrict__ diag,
                                                             double* __restrict__ dinv, uint8_t* __restrict__ mask,
                                                             int32_t* __restrict__ cnt_part) {
  __shared__ int sh[FEM_BLOCK];
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  int held = 0;
  if (v < m.nv) {
    int64_t lo, hi;
    fem_corner_range(m.vstart, v, 4 * m.nt, lo, hi);
    double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n = 0;
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t c = clamp_index(m.corder[i], 4 * m.nt);
      const int64_t e = c >> 2;
      const double V = m.geom[(int64_t)9 * m.nt + e];
      if (!(V > 0.0)) continue;
      ++n;
      double g[3];
      fem_grad_of(m.geom, m.nt, e, (int)(c & 3), g);
      const double a = V * (m.lam + m.mu), b = V * m.mu * (g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
      d[0] += a * g[0] * g[0] + b; d[1] += a * g[1] * g[1] + b; d[2] += a * g[2] * g[2] + b;
      d[3] += a * g[0] * g[1]; d[4] += a * g[0] * g[2]; d[5] += a * g[1] * g[2];
    }
    held = n == 0;
    const bool fx = held || (fixed && fixed[v]);
    mask[v] = (uint8_t)fx;
    double inv[6] = {1.0, 1.0, 1.0, 0.0, 0.0, 0.0};
    if (fx) {
      d[0] = d[1] = d[2] = 1.0;
      d[3] = d[4] = d[5] = 0.0;
    } else {
      const double c0 = d[1] * d[2] - d[5] * d[5], c1 = d[4] * d[5] - d[3] * d[2], c2 = d[3] * d[5] - d[4] * d[1];
      const double det = d[0] * c0 + d[3] * c1 + d[4] * c2;
      inv[0] = c0 / det; inv[3] = c1 / det; inv[4] = c2 / det;
      inv[1] = (d[0] * d[2] - d[4] * d[4]) / det;
      inv[5] = (d[3] * d[4] - d[0] * d[5]) / det;
      inv[2] = (d[0] * d[1] - d[3] * d[3]) / det;
    }
    for (int k = 0; k < 6; ++k) { diag[v * 6 + k] = d[k]; dinv[v * 6 + k] = inv[k]; }
  }
  const int tot = block_tree_sum<int, FEM_BLOCK>(held, sh);
  if (threadIdx.x == 0) cnt_part[blockIdx.x] = tot;
}

__global__ __launch_bounds__(FEM_BLOCK) void fem_count_final_kernel(const int32_t* __restrict__ part, int64_t n, int64_t* __restrict__ out) {
  __shared__ int64_t sh[FEM_BLOCK];
  int64_t s = 0;
  for (int64_t i = threadIdx.x; i < n; i += FEM_BLOCK) s += part[i];
  const int64_t tot = block_tree_sum<int64_t, FEM_BLOCK>(s, sh);
  if (threadIdx.x == 0) out[0] = tot;
}

// One workgroup: the per-workgroup partials in a fixed order (a lane's strided share, then the tree).
__device__ __forceinline__ double fem_final_sum(const double* __restrict__ part, int64_t n, double* sh) {
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += FEM_BLOCK) s += part[i];
  return block_tree_sum<double, FEM_BLOCK>(s, sh);
}

__global__ __launch_bounds__(FEM_BLOCK) void fem_sum_final_kernel(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
  __shared__ double sh[FEM_BLOCK];
  const double tot = fem_final_sum(part, n, sh);
  if (threadIdx.x == 0) out[0] = tot;
}

// ---- the operator ---------------------------------------------------------------------------------------------------------------
// H = grad x = sum_b (P x)_b g_b^T of element e (H[i][j] = d x_i / d X_j).
__device__ __forceinline__ void fem_grad_field(const FemMesh& m, int64_t e, const double* __restrict__ x, bool masked, double (*g)[3],
                                               double (*H)[3]) {
  const int4 id = *reinterpret_cast<const int4*>(m.tets + e * 4);
  const int64_t v[4] = {clamp_index(id.x, m.nv), clamp_index(id.y, m.nv), clamp_index(id.z, m.nv), clamp_index(id.w, m.nv)};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) H[i][j] = 0.0;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    if (masked && m.mask[v[b]]) continue;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double p = x[v[b] * 3 + i];
#pragma unroll
      for (int j = 0; j < 3; ++j) H[i][j] += p * g[b][j];
    }
  }
}

// Pass 1, per element: sig[.][e] = V sigma(P x), sigma = lam tr(H) I + mu (H + H^T), six values (xx, yy, zz, xy, xz, yz).
__global__ __launch_bounds__(FEM_BLOCK) void fem_stress_kernel(FemMesh m, const double* __restrict__ x, double* __restrict__ sig,
                                                               const FemScal* __restrict__ scal) {
  if (scal && scal->done) return;
  const int64_t e = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  if (e >= m.nt) return;
  double g[4][3], H[3][3];
  const double V = fem_grads(m.geom, m.nt, e, g);
  fem_grad_field(m, e, x, true, g, H);
  const double lt = m.lam * ((H[0][0] + H[1][1]) + H[2][2]);
  sig[e] = V * (lt + m.mu * (H[0][0] + H[0][0]));
  sig[m.nt + e] = V * (lt + m.mu * (H[1][1] + H[1][1]));
  sig[2 * m.nt + e] = V * (lt + m.mu * (H[2][2] + H[2][2]));
  sig[3 * m.nt + e] = V * (m.mu * (H[0][1] + H[1][0]));
  sig[4 * m.nt + e] = V * (m.mu * (H[0][2] + H[2][0]));
  sig[5 * m.nt + e] = V * (m.mu * (H[1][2] + H[2][1]));
}

// Pass 2, per vertex: y_v = sum over its corners (e, a) of (V sigma)_e g_a, or x_v at a masked vertex; on request the workgroup's
// share of x . y.
__global__ __launch_bounds__(FEM_BLOCK) void fem_gather_kernel(FemMesh m, const double* __restrict__ sig, const double* __restrict__ x,
                                                               double* __restrict__ y, double* __restrict__ part,
                                                               const FemScal* __restrict__ scal) {
  __shared__ double sh[FEM_BLOCK];
  if (scal && scal->done) return;
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  double dot = 0.0;
  if (v < m.nv) {
    double a[3] = {0.0, 0.0, 0.0};
    const double xv[3] = {x[v * 3], x[v * 3 + 1], x[v * 3 + 2]};
    if (m.mask[v]) {
      a[0] = xv[0]; a[1] = xv[1]; a[2] = xv[2];
    } else {
      int64_t lo, hi;
      fem_corner_range(m.vstart, v, 4 * m.nt, lo, hi);
      for (int64_t i = lo; i < hi; ++i) {
        const int64_t c = clamp_index(m.corder[i], 4 * m.nt);
        const int64_t e = c >> 2;
        double g[3], s[6];
        fem_grad_of(m.geom, m.nt, e, (int)(c & 3), g);
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] = sig[(int64_t)k * m.nt + e];
        a[0] += (s[0] * g[0] + s[3] * g[1]) + s[4] * g[2];
        a[1] += (s[3] * g[0] + s[1] * g[1]) + s[5] * g[2];
        a[2] += (s[4] * g[0] + s[5] * g[1]) + s[2] * g[2];
      }
    }
    y[v * 3] = a[0]; y[v * 3 + 1] = a[1]; y[v * 3 + 2] = a[2];
    dot = (xv[0] * a[0] + xv[1] * a[1]) + xv[2] * a[2];
  }
  if (part) {
    const double tot = block_tree_sum<double, FEM_BLOCK>(dot, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
  }
}

// ---- preconditioned CG: every kernel returns at once when `done` is set, so the state is frozen from that launch on ------------------
__device__ __forceinline__ void fem_precond(const double* __restrict__ dinv, int64_t v, const double* r, double* z) {
  const double* d = dinv + v * 6;
  z[0] = (d[0] * r[0] + d[3] * r[1]) + d[4] * r[2];
  z[1] = (d[3] * r[0] + d[1] * r[1]) + d[5] * r[2];
  z[2] = (d[4] * r[0] + d[5] * r[1]) + d[2] * r[2];
}

// x = 0, r = P f, z = D^-1 r, p = z; the workgroup's share of z . r
__global__ __launch_bounds__(FEM_BLOCK) void fem_cg_start_kernel(int64_t nv, const uint8_t* __restrict__ mask, const double* __restrict__ dinv,
                                                                 const double* __restrict__ f, double* __restrict__ x, double* __restrict__ r,
                                                                 double* __restrict__ z, double* __restrict__ p, double* __restrict__ part) {
  __shared__ double sh[FEM_BLOCK];
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  double dot = 0.0;
  if (v < nv) {
    double rv[3], zv[3];
    for (int i = 0; i < 3; ++i) rv[i] = mask[v] ? 0.0 : f[v * 3 + i];
    fem_precond(dinv, v, rv, zv);
    for (int i = 0; i < 3; ++i) { x[v * 3 + i] = 0.0; r[v * 3 + i] = rv[i]; z[v * 3 + i] = zv[i]; p[v * 3 + i] = zv[i]; }
    dot = (zv[0] * rv[0] + zv[1] * rv[1]) + zv[2] * rv[2];
  }
  const double tot = block_tree_sum<double, FEM_BLOCK>(dot, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// rho0 = <z0, r0>.  A zero right-hand side is solved by x = 0; a rho0 that is not a positive number ends the solve unconverged.
__global__ __launch_bounds__(FEM_BLOCK) void fem_cg_init_kernel(const double* __restrict__ part, int64_t n, FemScal* s, double tol2) {
  __shared__ double sh[FEM_BLOCK];
  const double rho = fem_final_sum(part, n, sh);
  if (threadIdx.x == 0) {
    s->rho = s->rho0 = rho;
    s->alpha = s->beta = s->pap = 0.0;
    s->tol2 = tol2;
    s->it = 0;
    s->converged = rho == 0.0;
    s->done = !(rho > 0.0);
    s->pad = 0;
  }
}

// pap = <p, A p>; alpha = rho / pap, or done (not converged) when pap <= 0
__global__ __launch_bounds__(FEM_BLOCK) void fem_cg_alpha_kernel(const double* __restrict__ part, int64_t n, FemScal* s) {
  __shared__ double sh[FEM_BLOCK];
  if (s->done) return;
  const double pap = fem_final_sum(part, n, sh);
  if (threadIdx.x == 0) {
    s->pap = pap;
    if (pap > 0.0) s->alpha = s->rho / pap;
    else s->done = 1;
  }
}

// x += alpha p, r -= alpha A p, z = D^-1 r; the workgroup's share of z . r
__global__ __launch_bounds__(FEM_BLOCK) void fem_cg_update_kernel(int64_t nv, const double* __restrict__ dinv, const FemScal* __restrict__ s,
                                                                  const double* __restrict__ p, const double* __restrict__ ap,
                                                                  double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                                  double* __restrict__ part) {
  __shared__ double sh[FEM_BLOCK];
  if (s->done) return;
  const double alpha = s->alpha;
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  double dot = 0.0;
  if (v < nv) {
    double rv[3], zv[3];
    for (int i = 0; i < 3; ++i) {
      x[v * 3 + i] += alpha * p[v * 3 + i];
      rv[i] = r[v * 3 + i] - alpha * ap[v * 3 + i];
      r[v * 3 + i] = rv[i];
    }
    fem_precond(dinv, v, rv, zv);
    for (int i = 0; i < 3; ++i) z[v * 3 + i] = zv[i];
    dot = (zv[0] * rv[0] + zv[1] * rv[1]) + zv[2] * rv[2];
  }
  const double tot = block_tree_sum<double, FEM_BLOCK>(dot, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// rho' = <z, r>: one more iteration is complete; converged when rho' <= tol2 rho0 (MFEM's CGSolver), done unconverged when rho' is
// negative or not a number; beta = rho' / rho
__global__ __launch_bounds__(FEM_BLOCK) void fem_cg_beta_kernel(const double* __restrict__ part, int64_t n, FemScal* s) {
  __shared__ double sh[FEM_BLOCK];
  if (s->done) return;
  const double rn = fem_final_sum(part, n, sh);
  if (threadIdx.x == 0) {
    s->it += 1;
    s->beta = rn / s->rho;
    s->rho = rn;
    if (rn <= s->tol2 * s->rho0) { s->done = 1; s->converged = rn >= 0.0; }
    else if (!(rn > 0.0)) s->done = 1;
  }
}

// p = z + beta p
__global__ __launch_bounds__(FEM_BLOCK) void fem_cg_dir_kernel(int64_t n3, const FemScal* __restrict__ s, const double* __restrict__ z,
                                                               double* __restrict__ p) {
  if (s->done) return;
  const double beta = s->beta;
  const int64_t i = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  if (i < n3) p[i] = z[i] + beta * p[i];
}

// ---- after the solve --------------------------------------------------------------------------------------------------------------
// Element e: w = lam tr(H)^2 + mu sum_ij H_ij (H_ij + H_ji), H = grad u (no mask: u is what the caller hands in); 0 for a skipped
// element.  The workgroup's shares of sum V w and sum V.
__global__ __launch_bounds__(FEM_BLOCK) void fem_energy_elem_kernel(FemMesh m, const double* __restrict__ u, double* __restrict__ we,
                                                                    double* __restrict__ part_c, double* __restrict__ part_v) {
  __shared__ double sh[FEM_BLOCK];
  const int64_t e = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  double vw = 0.0, vol = 0.0;
  if (e < m.nt) {
    double g[4][3], H[3][3];
    vol = fem_grads(m.geom, m.nt, e, g);
    double w = 0.0;
    if (vol > 0.0) {
      fem_grad_field(m, e, u, false, g, H);
      const double tr = (H[0][0] + H[1][1]) + H[2][2];
      double q = 0.0;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) q += H[i][j] * (H[i][j] + H[j][i]);
      w = m.lam * tr * tr + m.mu * q;
    }
    we[e] = w;
    vw = vol * w;
  }
  const double tc = block_tree_sum<double, FEM_BLOCK>(vw, sh);
  __syncthreads();
  const double tv = block_tree_sum<double, FEM_BLOCK>(vol, sh);
  if (threadIdx.x == 0) { part_c[blockIdx.x] = tc; part_v[blockIdx.x] = tv; }
}

// Vertex v: mean: sum V w / sum V over its elements that count; last: w of the one with the highest index (the last such corner of
// the sorted list); 0 without one.
__global__ __launch_bounds__(FEM_BLOCK) void fem_energy_vertex_kernel(FemMesh m, const double* __restrict__ we, int mode, double* __restrict__ wv) {
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  if (v >= m.nv) return;
  int64_t lo, hi;
  fem_corner_range(m.vstart, v, 4 * m.nt, lo, hi);
  double sw = 0.0, sv = 0.0, last = 0.0;
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t e = clamp_index(m.corder[i], 4 * m.nt) >> 2;
    const double V = m.geom[(int64_t)9 * m.nt + e];
    if (!(V > 0.0)) continue;
    last = we[e];
    sw += V * last;
    sv += V;
  }
  wv[v] = mode == FEM_NODAL_LAST ? last : (sv > 0.0 ? sw / sv : 0.0);
}

// ---- boundary: the load and the Hadamard gradients ------------------------------------------------------------------------------
// Face (a, b, c) in its stored order: n = (b - a) x (c - a) = 2 A n_f, every operation rounded on its own (the oracle's bits).
// Vertex v sums over its boundary corners, in the order of the stable sort of the face corners by vertex:
//   LOAD:  sqrt((n.x^2 + n.y^2) + n.z^2) * 0.5 / 3 * t over the selected faces, 0 at a masked vertex
//   else:  (0.5 n) / 3 over all faces, times weight[v] when given
template <bool LOAD>
__global__ __launch_bounds__(FEM_BLOCK) void fem_boundary_kernel(const double* __restrict__ X, int64_t nv, const int32_t* __restrict__ F,
                                                                 int64_t nb, const int64_t* __restrict__ border,
                                                                 const int64_t* __restrict__ bvstart, const uint8_t* __restrict__ sel,
                                                                 double t0, double t1, double t2, const uint8_t* __restrict__ mask,
                                                                 const double* __restrict__ weight, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  if (v >= nv) return;
  int64_t lo, hi;
  fem_corner_range(bvstart, v, 3 * nb, lo, hi);
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t f = clamp_index(border[i], 3 * nb) / 3;
    if (LOAD && sel && !sel[f]) continue;
    const int64_t ia = clamp_index(F[f * 3], nv), ib = clamp_index(F[f * 3 + 1], nv), ic = clamp_index(F[f * 3 + 2], nv);
    double e1[3], e2[3], n[3];
    for (int k = 0; k < 3; ++k) { e1[k] = X[ib * 3 + k] - X[ia * 3 + k]; e2[k] = X[ic * 3 + k] - X[ia * 3 + k]; }
    fem_cross_rn(e1, e2, n);
    if (LOAD) {
      const double a3 = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) * 0.5 / 3.0;
      s[0] += a3 * t0; s[1] += a3 * t1; s[2] += a3 * t2;
    } else {
      for (int k = 0; k < 3; ++k) s[k] += n[k] * 0.5 / 3.0;
    }
  }
  if (LOAD) {
    if (mask && mask[v]) s[0] = s[1] = s[2] = 0.0;
  } else if (weight) {
    const double w = weight[v];
    for (int k = 0; k < 3; ++k) s[k] *= w;
  }
  for (int k = 0; k < 3; ++k) out[v * 3 + k] = s[k];
}

// ---- the exact discrete gradient of the compliance with respect to the vertices ------------------------------------
// Pi(X, u) = 2 f(X) . u - u^T K(X) u is the compliance at the solution and stationary in the free components of u, so
// d compliance / dX = dPi/dX at fixed u = gK + 2 sum over the tractions of gL.  Two passes shaped like the operator's, one boundary pass.
//
// Pass 1, per element: E = V (w I - 2 H^T S), H = grad u (no mask: u is what the caller hands in), S = lam tr(H) I + mu (H + H^T),
// w as in fem_energy_elem_kernel, (H^T S)_kj = sum_i H_ik S_ij; emt[3 k + j][e] (geom's layout).  d(V w)/dx_b = E g_b, from
// dV/dx_b = V g_b and d g_a,j / d x_b,k = -g_b,j g_a,k.  E is not symmetric.  A skipped element stores nine exact zeros.
__global__ __launch_bounds__(FEM_BLOCK) void fem_emt_kernel(FemMesh m, const double* __restrict__ u, double* __restrict__ emt) {
  const int64_t e = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  if (e >= m.nt) return;
  double g[4][3], H[3][3], E[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const double V = fem_grads(m.geom, m.nt, e, g);
  if (V > 0.0) {
    fem_grad_field(m, e, u, false, g, H);
    const double tr = (H[0][0] + H[1][1]) + H[2][2];
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) q += H[i][j] * (H[i][j] + H[j][i]);
    const double w = m.lam * tr * tr + m.mu * q, lt = m.lam * tr;
    double S[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) S[i][j] = (i == j ? lt : 0.0) + m.mu * (H[i][j] + H[j][i]);
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double hs = (H[0][k] * S[0][j] + H[1][k] * S[1][j]) + H[2][k] * S[2][j];
        E[3 * k + j] = V * ((k == j ? w : 0.0) - 2.0 * hs);
      }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) emt[(int64_t)k * m.nt + e] = E[k];
}

// Pass 2, per vertex: gK_v = -sum over its corners (e, a) of E_e g_a, in corner_order's order; masked vertices included (a clamped
// vertex moves with the mesh like any other).
__global__ __launch_bounds__(FEM_BLOCK) void fem_emt_gather_kernel(FemMesh m, const double* __restrict__ emt, double* __restrict__ grad) {
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  if (v >= m.nv) return;
  int64_t lo, hi;
  fem_corner_range(m.vstart, v, 4 * m.nt, lo, hi);
  double a[3] = {0.0, 0.0, 0.0};
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t c = clamp_index(m.corder[i], 4 * m.nt);
    const int64_t e = c >> 2;
    double g[3], E[9];
    fem_grad_of(m.geom, m.nt, e, (int)(c & 3), g);
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = emt[(int64_t)k * m.nt + e];
    a[0] += (E[0] * g[0] + E[1] * g[1]) + E[2] * g[2];
    a[1] += (E[3] * g[0] + E[4] * g[1]) + E[5] * g[2];
    a[2] += (E[6] * g[0] + E[7] * g[1]) + E[8] * g[2];
  }
  grad[v * 3] = -a[0]; grad[v * 3 + 1] = -a[1]; grad[v * 3 + 2] = -a[2];
}

// Boundary pass, per vertex: gL_v = sum over its boundary corners on selected faces (a, b, c), in bcorner_order's order, of
// c_f dA_f/dx_v: N = (b - a) x (c - a) as in fem_boundary_kernel, |N| = sqrt((N.x^2 + N.y^2) + N.z^2), n^ = N / |N|,
// c_f = ((u~_a + u~_b) + u~_c) . t / 3 with u~ = u zeroed at masked vertices, dA/dx_a = n^ x (x_c - x_b) / 2,
// dA/dx_b = n^ x (x_a - x_c) / 2, dA/dx_c = n^ x (x_b - x_a) / 2.  Every operation rounded on its own.  A face with |N| == 0 or a
// non-finite n^ adds exact zeros: the area is not differentiable there (the boundary's counterpart of a skipped element).
__global__ __launch_bounds__(FEM_BLOCK) void fem_load_gradient_kernel(const double* __restrict__ X, int64_t nv, const int32_t* __restrict__ F,
                                                                      int64_t nb, const int64_t* __restrict__ border,
                                                                      const int64_t* __restrict__ bvstart, const uint8_t* __restrict__ sel,
                                                                      double t0, double t1, double t2, const uint8_t* __restrict__ mask,
                                                                      const double* __restrict__ u, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * FEM_BLOCK + threadIdx.x;
  if (v >= nv) return;
  int64_t lo, hi;
  fem_corner_range(bvstart, v, 3 * nb, lo, hi);
  double s[3] = {0.0, 0.0, 0.0};
  for (int64_t i = lo; i < hi; ++i) {
    const int64_t bc = clamp_index(border[i], 3 * nb);
    const int64_t f = bc / 3;
    const int k = (int)(bc - 3 * f);
    if (sel && !sel[f]) continue;
    const int64_t id[3] = {clamp_index(F[f * 3], nv), clamp_index(F[f * 3 + 1], nv), clamp_index(F[f * 3 + 2], nv)};
    double x[3][3], e1[3], e2[3], n[3];
    for (int c = 0; c < 3; ++c)
      for (int j = 0; j < 3; ++j) x[c][j] = X[id[c] * 3 + j];
    for (int j = 0; j < 3; ++j) { e1[j] = x[1][j] - x[0][j]; e2[j] = x[2][j] - x[0][j]; }
    fem_cross_rn(e1, e2, n);
    const double len = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    const double nh[3] = {n[0] / len, n[1] / len, n[2] / len};
    if (!(len != 0.0) || !isfinite(nh[0]) || !isfinite(nh[1]) || !isfinite(nh[2])) continue;
    double us[3][3];
    for (int c = 0; c < 3; ++c) {
      const bool held = mask && mask[id[c]];
      for (int j = 0; j < 3; ++j) us[c][j] = held ? 0.0 : u[id[c] * 3 + j];
    }
    const double s0 = (us[0][0] + us[1][0]) + us[2][0], s1 = (us[0][1] + us[1][1]) + us[2][1], s2 = (us[0][2] + us[1][2]) + us[2][2];
    const double cf = ((s0 * t0 + s1 * t1) + s2 * t2) / 3.0;
    const int p = k == 0 ? 2 : (k == 1 ? 0 : 1), q = k == 0 ? 1 : (k == 1 ? 2 : 0);      // corner k: n^ x (x_p - x_q) / 2
    double d[3], dA[3];
    for (int j = 0; j < 3; ++j) d[j] = x[p][j] - x[q][j];
    fem_cross_rn(nh, d, dA);
    for (int j = 0; j < 3; ++j) s[j] += cf * (dA[j] * 0.5);
  }
  for (int j = 0; j < 3; ++j) out[v * 3 + j] = s[j];
}

}  // namespace dsdf
