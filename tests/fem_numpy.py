"""The fp64 oracle of the P1 linear-elasticity solver (include/dsdf.h dsdf_fem_*), in numpy and scipy: the element
geometry with every operation rounded on its own (the kernels store the same bits), K assembled as a scipy.sparse CSR from
K_ab[i][j] = V (lam g_a,i g_b,j + mu g_b,i g_a,j + mu (g_a . g_b) delta_ij), the masked operator, spsolve, a numpy restatement of the
same preconditioned CG with the same preconditioner and stopping rule, every post-processing quantity, the term-wise absolute values
the rounding bounds are stated against, the wrong variants the discrimination tests evaluate, and the same CG with its whole path kept,
in four correct restatements and four wrong ones, on the solves the CG tests share (cg_problem).  Degrees of freedom are interleaved:
dof 3 v + i is component i of vertex v."""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

U = 2.0 ** -53


# ---- element geometry -----------------------------------------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def geometry(verts, tets):
    """(geom [10, T]: g_1, g_2, g_3 and V, zeros for a skipped element; skipped [T] bool)."""
    x = np.asarray(verts, dtype=np.float64)[np.asarray(tets, dtype=np.int64)]
    e1, e2, e3 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0], x[:, 3] - x[:, 0]
    c = [_cross(e2, e3), _cross(e3, e1), _cross(e1, e2)]
    det = (e1[:, 0] * c[0][:, 0] + e1[:, 1] * c[0][:, 1]) + e1[:, 2] * c[0][:, 2]
    V = det / 6.0
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.concatenate([ck / det[:, None] for ck in c], 1)            # [T, 9]
    ok = (V > 0.0) & np.isfinite(g).all(1)
    geom = np.where(ok[None, :], np.concatenate([g.T, V[None, :]], 0), 0.0)
    return geom, ~ok


def gradients(geom):
    """(g [T, 4, 3], V [T]); g_0 = -((g_1 + g_2) + g_3)."""
    g123 = geom[:9].T.reshape(-1, 3, 3)
    g0 = -((g123[:, 0] + g123[:, 1]) + g123[:, 2])
    return np.concatenate([g0[:, None], g123], 1), geom[9]


def corner_counts(ids, n_verts):
    return np.bincount(np.asarray(ids, dtype=np.int64).reshape(-1), minlength=n_verts)


def held_vertices(tets, skipped, n_verts):
    """[V] bool: no element that counts."""
    t = np.asarray(tets, dtype=np.int64)[~skipped]
    return corner_counts(t, n_verts) == 0


# ---- K --------------------------------------------------------------------------------------------------------------------------
def element_matrices(g, V, lam, mu, variant=None, absolute=False):
    """[T, 4, 3, 4, 3]: K_e[a, i, b, j].  variant: 'swap' (lam and mu exchanged), 'no_transpose' (the g_b g_a^T term dropped).
    absolute: the sum of the absolute values of the terms instead (what a counted rounding bound is stated against)."""
    if variant == "swap":
        lam, mu = mu, lam
    if absolute:
        g, lam = np.abs(g), abs(lam)
    t1 = lam * np.einsum("eai,ebj->eaibj", g, g)
    t2 = mu * np.einsum("ebi,eaj->eaibj", g, g)
    t3 = mu * np.einsum("eak,ebk->eab", g, g)[:, :, None, :, None] * np.eye(3)[None, None, :, None, :]
    if variant == "no_transpose":
        t2 = 0.0
    return V[:, None, None, None, None] * (t1 + t2 + t3)


def assemble(verts, tets, lam, mu, variant=None, absolute=False):
    """K [3V, 3V] CSR (duplicates summed)."""
    nv = len(verts)
    tets = np.asarray(tets, dtype=np.int64)
    g, V = gradients(geometry(verts, tets)[0])
    Ke = element_matrices(g, V, lam, mu, variant, absolute)
    dof = 3 * tets[:, :, None] + np.arange(3)[None, None, :]                 # [T, 4, 3]
    rows = np.broadcast_to(dof[:, :, :, None, None], Ke.shape).reshape(-1)
    cols = np.broadcast_to(dof[:, None, None, :, :], Ke.shape).reshape(-1)
    return sp.coo_matrix((Ke.reshape(-1), (rows, cols)), shape=(3 * nv, 3 * nv)).tocsr()


def masked(K, mask):
    """A = P K P + (I - P) for mask [V] bool (True: the vertex's three components are zeroed)."""
    keep = np.repeat(~np.asarray(mask, dtype=bool), 3).astype(np.float64)
    P = sp.diags(keep)
    return (P @ K @ P + sp.diags(1.0 - keep)).tocsr()


def diag_blocks(A):
    """[V, 6]: (xx, yy, zz, xy, xz, yz) of every vertex's 3 x 3 diagonal block."""
    nv = A.shape[0] // 3
    out = np.zeros((nv, 6))
    idx = 3 * np.arange(nv)
    for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        out[:, k] = np.asarray(A[idx + i, idx + j]).reshape(-1)
    return out


def sym3(d):
    """[V, 6] -> [V, 3, 3]."""
    m = np.empty((len(d), 3, 3))
    for k, (i, j) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        m[:, i, j] = m[:, j, i] = d[:, k]
    return m


def block_inverse(d):
    """[V, 6] -> [V, 3, 3] inverses."""
    return np.linalg.inv(sym3(d))


# ---- the operator without a matrix (the large grid, where assembling would take longer than a test may) ---------------------------
def apply_free(verts, tets, lam, mu, mask, x, absolute=False):
    """A x [V, 3] element by element; absolute: sum of the absolute values of the terms (|A| |x| term-wise)."""
    tets = np.asarray(tets, dtype=np.int64)
    g, V = gradients(geometry(verts, tets)[0])
    keep = ~np.asarray(mask, dtype=bool)
    xm = np.where(keep[:, None], x, 0.0)
    if absolute:
        g, xm, lam = np.abs(g), np.abs(xm), abs(lam)
    H = np.einsum("ebi,ebj->eij", xm[tets], g)
    sig = lam * np.trace(H, axis1=1, axis2=2)[:, None, None] * np.eye(3)[None] + mu * (H + H.transpose(0, 2, 1))
    F = V[:, None, None] * np.einsum("eij,eaj->eai", sig, g)
    y = np.zeros((len(verts), 3))
    np.add.at(y, tets.reshape(-1), F.reshape(-1, 3))
    return np.where(keep[:, None], y, np.abs(x) if absolute else x)


def apply_bound_c(n_corners, n_row=None):
    """Roundings between a term V * coefficient * g * g * x of row i and the value compared: the kernels 14 + n_corners,
    the CSR oracle 9 + n_corners + n_row (n_row: entries of the longest row; at most 3 (3 n_corners + 1))."""
    if n_row is None:
        n_row = 3 * (3 * n_corners + 1)
    return 23 + 2 * n_corners + n_row


def sum_roundings(n):
    """Roundings on the way of one term through the kernels' sum of n values (one per lane, an 8-level tree, ceil(n / 65536) strided
    additions and another 8-level tree) plus numpy's pairwise sum (at most 19 + log2 n)."""
    return 35 + math.ceil(n / 65536) + math.ceil(math.log2(max(n, 2)))


# ---- load -----------------------------------------------------------------------------------------------------------------------
def face_normals(verts, bfaces, flip=False):
    """n = (b - a) x (c - a) = 2 A n_f per face, every operation rounded on its own; flip: the wrong (inward) sign."""
    x = np.asarray(verts, dtype=np.float64)[np.asarray(bfaces, dtype=np.int64)]
    n = _cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
    return -n if flip else n


def load(verts, bfaces, sel, t, mask=None):
    """f [V, 3] = sum over the selected faces of area / 3 * t at each of their vertices, zero at masked vertices."""
    n = face_normals(verts, bfaces)
    a3 = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) * 0.5 / 3.0
    a3 = np.where(np.asarray(sel, dtype=bool), a3, 0.0)
    f = np.zeros((len(verts), 3))
    np.add.at(f, np.asarray(bfaces, dtype=np.int64).reshape(-1), np.repeat(a3[:, None] * np.asarray(t, dtype=np.float64)[None, :], 3, 0))
    if mask is not None:
        f[np.asarray(mask, dtype=bool)] = 0.0
    return f


# ---- solve ----------------------------------------------------------------------------------------------------------------------
def spsolve(A, b):
    return spla.spsolve(A.tocsc(), b.reshape(-1)).reshape(-1, 3)


def pcg(A, Dinv, b, rel_tol=1e-10, max_iter=10000):
    """The kernels' preconditioned CG restated: (u [V, 3], iterations, converged, <z, r> / <z0, r0>).  Dinv [V, 3, 3]."""
    def prec(r):
        return np.einsum("vij,vj->vi", Dinv, r.reshape(-1, 3)).reshape(-1)
    b = b.reshape(-1)
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    rho0 = rho = float(z @ r)
    if not rho0 > 0.0:
        return x.reshape(-1, 3), 0, rho0 == 0.0, 0.0
    it, conv = 0, False
    while it < max_iter:
        ap = A @ p
        pap = float(p @ ap)
        if not pap > 0.0:
            break
        alpha = rho / pap
        x += alpha * p
        r -= alpha * ap
        z = prec(r)
        rn = float(z @ r)
        it += 1
        beta, rho = rn / rho, rn
        if rn <= rel_tol * rel_tol * rho0:
            conv = rn >= 0.0
            break
        if not rn > 0.0:
            break
        p = z + beta * p
    return x.reshape(-1, 3), it, conv, rho / rho0


# ---- the same CG, followed step by step (tests/test_gpu_fem_cg.py) ----------------------------------------------------
CG_WRONG = ("stale_rho", "steepest", "rho0", "dir_from_r")


def block_inverse_adjugate(d):
    """[V, 6] -> [V, 3, 3] inverses by cofactors over the determinant: the kernels' route, another rounding than numpy's LU."""
    xx, yy, zz, xy, xz, yz = (d[:, k] for k in range(6))
    c = np.stack([yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy, xz * yz - xy * zz, xy * yz - xz * yy, xy * xz - xx * yz], 1)
    det = (xx * c[:, 0] + xy * c[:, 3]) + xz * c[:, 4]
    return sym3(c / det[:, None])


def free_operator(verts, tets, lam, mu, mask):
    """x [3V] -> A x [3V] without the assembled matrix: every element's 12 x 12 block times its own twelve values, then the elements'
    forces summed per vertex -- the kernels' grouping (within the element first), where the CSR adds a row's entries one by one."""
    tets = np.asarray(tets, dtype=np.int64)
    Ke = element_matrices(*gradients(geometry(verts, tets)[0]), lam, mu).reshape(len(tets), 12, 12)
    keep = ~np.asarray(mask, dtype=bool)
    nv, flat = len(verts), tets.reshape(-1)

    def op(x):
        x = x.reshape(-1, 3)
        F = np.matmul(Ke, np.where(keep[:, None], x, 0.0)[tets].reshape(-1, 12, 1)).reshape(-1, 3)
        y = np.stack([np.bincount(flat, weights=F[:, i], minlength=nv) for i in range(3)], 1)
        return np.where(keep[:, None], y, x).reshape(-1)
    return op


def _dot(order):
    if order == "blas":
        return lambda a, b: float(a @ b)
    if order == "reversed":                      # the products summed pairwise from the far end: another grouping than the BLAS kernel's
        return lambda a, b: float(np.add.reduce((a * b)[::-1].copy()))
    raise ValueError(order)


def pcg_trace(A, Dinv, b, rel_tol=1e-10, max_iter=10000, dot="blas", wrong=None):
    """pcg, keeping the path.  A: a matrix or a callable x [3V] -> A x; dot: 'blas' or 'reversed'; wrong: None or one of CG_WRONG --
    'stale_rho' (beta = rho' / the rho of the iteration before), 'steepest' (beta = 0), 'rho0' (beta = rho' / rho0), 'dir_from_r'
    (p = r + beta p).  With a matrix, 'blas' and wrong=None every operation is pcg's: identical bytes.
    Returns a dict: x [V, 3], it, conv, ratio as pcg; xs [it + 1, V, 3], xs[k] iterate k; ratios [it + 1], rho_k / rho0 (the recursive
    one); scal [(rho', alpha, beta, pap)] per completed iteration; paps, ps: every p . A p computed and its p, the one that ended the
    solve included; rho0."""
    op = A if callable(A) else (lambda v: A @ v)
    dt = _dot(dot)

    def prec(r):
        return np.einsum("vij,vj->vi", Dinv, r.reshape(-1, 3)).reshape(-1)
    b = b.reshape(-1)
    x = np.zeros_like(b)
    r = b.copy()
    z = prec(r)
    p = z.copy()
    with np.errstate(all="ignore"):
        rho0 = rho = dt(z, r)
    out = dict(xs=[x.reshape(-1, 3).copy()], ratios=[1.0], scal=[], paps=[], ps=[], rho0=rho0)

    def done(it, conv, ratio):
        out.update(x=x.reshape(-1, 3), it=it, conv=conv, ratio=ratio, xs=np.stack(out["xs"]), ratios=np.array(out["ratios"]))
        return out
    if not rho0 > 0.0:
        out["ratios"] = [0.0]
        return done(0, rho0 == 0.0, 0.0)
    it, conv, rho_before = 0, False, rho0
    with np.errstate(all="ignore"):
        while it < max_iter:
            ap = op(p)
            pap = dt(p, ap)
            out["paps"].append(pap)
            out["ps"].append(p.copy())
            if not pap > 0.0:
                break
            alpha = rho / pap
            x += alpha * p
            r -= alpha * ap
            z = prec(r)
            rn = dt(z, r)
            it += 1
            beta = {None: rn / rho, "dir_from_r": rn / rho, "stale_rho": rn / rho_before, "steepest": 0.0, "rho0": rn / rho0}[wrong]
            rho_before, rho = rho, rn
            out["xs"].append(x.reshape(-1, 3).copy())
            out["ratios"].append(rho / rho0)
            out["scal"].append((rn, alpha, beta, pap))
            if rn <= rel_tol * rel_tol * rho0:
                conv = rn >= 0.0
                break
            if not rn > 0.0:
                break
            p = (r if wrong == "dir_from_r" else z) + beta * p
        return done(it, conv, rho / rho0)


def iterate(tr, k):
    """Iterate k of a trace; the last one from its end on (what solve(max_iter=k) returns)."""
    return tr["xs"][min(k, tr["it"])]


def cg_variants(verts, tets, lam, mu, mask, f, **kw):
    """Four correct restatements of one solve, differing pairwise in what the kernels differ from any of them in: the operator's sum
    order (assembled CSR / element by element), the dot products' order, and the route to the block inverses (LU / adjugate).
    (A, Dinv by LU, {name: trace}); the first, 'csr', is pcg itself."""
    A = masked(assemble(verts, tets, lam, mu), mask)
    d = diag_blocks(A)
    inv, adj = block_inverse(d), block_inverse_adjugate(d)
    free = free_operator(verts, tets, lam, mu, mask)
    runs = {"csr": (A, inv, "blas"), "csr reversed adjugate": (A, adj, "reversed"), "free adjugate": (free, adj, "blas"),
            "free reversed": (free, inv, "reversed")}
    return A, inv, {k: pcg_trace(op, Di, f, dot=dt, **kw) for k, (op, Di, dt) in runs.items()}


def energy_norm(A, d):
    d = d.reshape(-1)
    return math.sqrt(max(float(d @ (A @ d)), 0.0))


def cg_spread(A, traces, ref, k_max):
    """s [k_max + 1]: s[k] the largest pairwise ||x_j^a - x_j^b||_A / ||ref||_A over the traces and j <= k."""
    tr = list(traces.values())
    nref = energy_norm(A, ref)
    s = np.zeros(k_max + 1)
    for k in range(k_max + 1):
        xs = [iterate(t, k) for t in tr]
        s[k] = max(energy_norm(A, xs[a] - xs[b]) for a in range(len(tr)) for b in range(a)) / nref
    return np.maximum.accumulate(s)


def cg_ratio_spread(traces, k_max):
    """q [k_max + 1]: the same for the scalar rho_j / rho0, relative to the first trace's."""
    tr = list(traces.values())
    q = np.zeros(k_max + 1)
    for k in range(k_max + 1):
        rs = [t["ratios"][min(k, t["it"])] for t in tr]
        q[k] = (max(rs) - min(rs)) / abs(rs[0]) if rs[0] != 0.0 else 0.0
    return np.maximum.accumulate(q)


def cg_iterate_bound(s):
    """What tests/test_gpu_fem_cg.py holds the kernels' iterate k to, in relative energy norm: 16 times the restatements' own spread --
    the kernels differ from a restatement in one more respect (contraction) than the restatements among themselves -- floored at 16 U."""
    return 16.0 * np.maximum(s, U)


def cg_ratio_bound(q):
    """The same for the returned ratio, relative: 16 times the restatements' spread in rho_k / rho0, floored at 64 U."""
    return np.maximum(16.0 * q, 64.0 * U)


def true_residual(A, Dinv, b, u):
    """<D^-1 (b - A u), b - A u> / <D^-1 b, b>."""
    b = b.reshape(-1)
    r = b - A @ u.reshape(-1)
    pr = np.einsum("vij,vj->vi", Dinv, r.reshape(-1, 3)).reshape(-1)
    pb = np.einsum("vij,vj->vi", Dinv, b.reshape(-1, 3)).reshape(-1)
    return float(pr @ r) / float(pb @ b)


def energy_distance(A, u, ref):
    """||u - ref||_A / ||ref||_A."""
    d = (u - ref).reshape(-1)
    return math.sqrt(float(d @ (A @ d)) / float(ref.reshape(-1) @ (A @ ref.reshape(-1))))


# ---- after the solve ------------------------------------------------------------------------------------------------------------
def energy_density(verts, tets, lam, mu, u, absolute=False):
    """(w [T]: lam tr(H)^2 + mu sum H_ij (H_ij + H_ji), 0 for a skipped element; V [T]).  absolute: the term-wise absolute sum."""
    tets = np.asarray(tets, dtype=np.int64)
    g, V = gradients(geometry(verts, tets)[0])
    if absolute:
        g, u, lam = np.abs(g), np.abs(u), abs(lam)
    H = np.einsum("ebi,ebj->eij", np.asarray(u, dtype=np.float64)[tets], g)
    tr = (H[:, 0, 0] + H[:, 1, 1]) + H[:, 2, 2]
    w = lam * tr * tr + mu * np.einsum("eij,eij->e", H, H + H.transpose(0, 2, 1))
    return np.where(V > 0.0, w, 0.0), V


def nodal_density(tets, w, V, n_verts, mode="mean"):
    """[V]: 'mean' sum V w / sum V over the vertex's elements that count, 'last' w of the one with the highest index; 0 without one."""
    tets = np.asarray(tets, dtype=np.int64)
    ok = V > 0.0
    out = np.zeros(n_verts)
    if mode == "mean":
        num, den = np.zeros(n_verts), np.zeros(n_verts)
        np.add.at(num, tets[ok].reshape(-1), np.repeat(V[ok] * w[ok], 4))
        np.add.at(den, tets[ok].reshape(-1), np.repeat(V[ok], 4))
        np.divide(num, den, out=out, where=den > 0.0)
    else:
        out[tets[ok].reshape(-1)] = np.repeat(w[ok], 4)        # increasing element index; of repeated indices the last assignment stays
    return out


def boundary_gradient(verts, bfaces, weight=None, flip=False, absolute=False):
    """[V, 3]: sum over the vertex's boundary triangles of (0.5 n) / 3, times weight[v]."""
    n = face_normals(verts, bfaces, flip) * 0.5 / 3.0
    if absolute:
        n = np.abs(n)
    g = np.zeros((len(verts), 3))
    np.add.at(g, np.asarray(bfaces, dtype=np.int64).reshape(-1), np.repeat(n, 3, 0))
    return g if weight is None else g * np.asarray(weight)[:, None]


# ---- meshes the CPU and the GPU tests share ----------------------------------------------------------------------------------------
ONE_TET = (np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.2], [0.2, 1.1, 0.4], [0.3, 0.2, 0.9]]), np.array([[0, 1, 2, 3]], dtype=np.int32),
           np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32), np.zeros(4, dtype=np.int8))


def random_grid():
    """The 9 x 8 x 7 grid of test_gpu_tetmesh.py."""
    return np.random.default_rng(7).uniform(-1, 1, (9, 8, 7)).astype(np.float32)


def degenerate_grid():
    """The same grid with a few values equal to the level: with t_clamp = 0 the elements around them have zero volume."""
    g = random_grid()
    for p in ((2, 3, 3), (5, 4, 2), (6, 2, 5), (3, 5, 4)):
        g[p] = 0.0
    return g


def inside_grid(n):
    return -np.ones((n, n, n), dtype=np.float32)


def arrays(m):
    return m.verts, m.tets, m.bfaces, m.bface_kind


def cpu_meshes():
    """{name: (verts, tets, bfaces, bface_kind)} from tests/tet_numpy.py: the smallest mesh at which each mechanism can fail."""
    from tests import tet_numpy
    return {"one tet": ONE_TET, "2x2x2": arrays(tet_numpy.tetrahedralize(inside_grid(2))), "3x3x3": arrays(tet_numpy.tetrahedralize(inside_grid(3))),
            "cut": arrays(tet_numpy.tetrahedralize(random_grid(), t_clamp=0.05)), "degenerate": arrays(tet_numpy.tetrahedralize(degenerate_grid()))}


def reference_attributes(verts, bfaces, tolerance=3e-2):
    """The reference's 1 / 2 / 3 rule (TetMesh.boundary_attributes) in numpy."""
    c = np.asarray(verts)[np.asarray(bfaces, dtype=np.int64)]
    x_max, z_max = c[:, :, 0].max(1), c[:, :, 2].max(1)
    return np.where(x_max < tolerance, 1, np.where(z_max > np.asarray(verts)[:, 2].max() - tolerance, 2, 3)).astype(np.int32)


def clamped_faces(verts, bfaces):
    """[M] bool: the faces the tests clamp -- attribute 1 where a face carries it, else the first face alone (the single tetrahedron)."""
    sel = reference_attributes(verts, bfaces) == 1
    return sel if sel.any() else np.arange(len(bfaces)) == 0


def attributes(verts, bfaces):
    """The reference's attributes, with the first face made 1 where no face carries it (so that every test mesh can be clamped)."""
    a = reference_attributes(verts, bfaces)
    if not (a == 1).any():
        a[0] = 1
    return a


def kappa(A, d):
    """Condition number of D^-1 A for the block diagonal d [V, 6]: dense up to 400 unknowns, Lanczos above."""
    D = sp.block_diag(list(sym3(d)), format="csc")
    if A.shape[0] <= 400:
        import scipy.linalg as sl
        ev = sl.eigh(A.toarray(), D.toarray(), eigvals_only=True)
        return float(ev[-1] / ev[0])
    hi = spla.eigsh(A.tocsc(), k=1, M=D, which="LM", return_eigenvectors=False)[0]
    lo = spla.eigsh(A.tocsc(), k=1, M=D, sigma=0.0, which="LM", return_eigenvectors=False)[0]
    return float(hi / lo)


def fixed_vertices(bfaces, sel, n_verts):
    out = np.zeros(n_verts, dtype=bool)
    out[np.asarray(bfaces, dtype=np.int64)[np.asarray(sel, dtype=bool)].reshape(-1)] = True
    return out


def largest_component(m):
    """The elements, boundary faces and vertices of the mesh's largest vertex-connected component, renumbered: (verts, tets, bfaces, kind)."""
    import scipy.sparse.csgraph as csg
    t = np.asarray(m.tets, dtype=np.int64)
    nv = len(m.verts)
    adj = sp.coo_matrix((np.ones(3 * len(t)), (np.repeat(t[:, 0], 3), t[:, 1:].reshape(-1))), shape=(nv, nv))
    _, lab = csg.connected_components(adj, directed=False)
    used = np.zeros(nv, dtype=bool)
    used[t.reshape(-1)] = True
    best = np.bincount(lab[used]).argmax()
    keep = used & (lab == best)
    new = np.cumsum(keep) - 1
    te = t[keep[t[:, 0]]]
    bf = np.asarray(m.bfaces, dtype=np.int64)
    kb = keep[bf[:, 0]]
    return m.verts[keep], new[te].astype(np.int32), new[bf[kb]].astype(np.int32), np.asarray(m.bface_kind)[kb]


# ---- the solves the CG tests follow (tests/test_fem_cpu.py proves them, tests/test_gpu_fem_cg.py runs them on the kernels) -----------
CG_LAM, CG_MU, CG_TRACTION = 0.7, 1.3, (0.0, 0.0, -0.01)
CG_TRAJECTORY = ("2x2x2", "3x3x3", "cut")
OVERFLOW_SCALE, OVERFLOW_DIRECTION = 1e160, (0.3, -0.2, 0.5)
# name: (mesh, lam, mu, load, iterations before the ending)
CG_ENDINGS = {"zero load": ("2x2x2", CG_LAM, CG_MU, "zero", 0), "nan load": ("2x2x2", CG_LAM, CG_MU, "nan", 0),
              "pap after 0": ("2x2x2", -1.9, 1.0, "random", 0), "pap after 1": ("2x2x2", -1.2, 1.0, "random", 1),
              "pap after 3": ("3x3x3", -1.0, 1.0, "random", 3), "overflow": ("2x2x2", CG_LAM, CG_MU, "overflow", 1),
              "one free vertex 0.7": ("one tet", CG_LAM, CG_MU, "vertex", 1), "one free vertex -1.0": ("one tet", -1.0, 1.0, "vertex", 1),
              "one free vertex -1.2": ("one tet", -1.2, 1.0, "vertex", 1), "one free vertex -1.9": ("one tet", -1.9, 1.0, "vertex", 1)}
_cg_cache = {}


def cg_load(kind, verts, bfaces, mask):
    """The loads of CG_ENDINGS and of the trajectories ('traction'), [V, 3], zero at the masked vertices."""
    nv = len(verts)
    first_free = int(np.flatnonzero(~mask)[0])
    if kind in ("traction", "nan"):
        f = load(verts, bfaces, attributes(verts, bfaces) == 2, CG_TRACTION, mask)
        if kind == "nan":
            f[first_free, 1] = np.nan
        return f
    if kind == "random":
        f = np.random.default_rng(5).standard_normal((nv, 3))
        f[mask] = 0.0
        return f
    f = np.zeros((nv, 3))
    if kind == "vertex":
        f[first_free] = OVERFLOW_DIRECTION
    elif kind == "overflow":            # one vertex: every product of <z, r> and <p, A p> is zero or of one sign, whatever the order
        f[first_free] = OVERFLOW_SCALE * np.asarray(OVERFLOW_DIRECTION)
    elif kind != "zero":
        raise ValueError(kind)
    return f


def cg_problem(name):
    """The solve `name` (of CG_TRAJECTORY or CG_ENDINGS) on the CPU meshes, with its four restatements: computed once, never changed.
    dict: mesh (the four arrays), lam, mu, mask, f, A, Dinv, traces, q (cg_ratio_spread); for a trajectory also ref (spsolve), s
    (cg_spread) and it_max, all up to k_max = the longest restatement + 2."""
    if name in _cg_cache:
        return _cg_cache[name]
    if "meshes" not in _cg_cache:
        _cg_cache["meshes"] = cpu_meshes()
    mesh, lam, mu, kind, _ = CG_ENDINGS[name] if name in CG_ENDINGS else (name, CG_LAM, CG_MU, "traction", None)
    v, t, bf, bk = _cg_cache["meshes"][mesh]
    nv = len(v)
    mask = held_vertices(t, geometry(v, t)[1], nv) | fixed_vertices(bf, clamped_faces(v, bf), nv)
    f = cg_load(kind, v, bf, mask)
    A, Dinv, traces = cg_variants(v, t, lam, mu, mask, f)
    k_max = max(tr["it"] for tr in traces.values()) + 2
    out = dict(name=name, mesh=(v, t, bf, bk), lam=lam, mu=mu, mask=mask, f=f, A=A, Dinv=Dinv, traces=traces, k_max=k_max,
               q=cg_ratio_spread(traces, k_max))
    if name in CG_TRAJECTORY:
        out["ref"] = spsolve(A, f)
        out["s"] = cg_spread(A, traces, out["ref"], k_max)
    _cg_cache[name] = out
    return out
