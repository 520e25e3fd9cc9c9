"""The fp64 oracle of the exact discrete compliance gradient (include/dsdf.h dsdf_fem_stiffness_gradient / dsdf_fem_load_gradient,
DESIGN 4.21.6), in numpy on top of tests/fem_numpy.py, which it imports and does not change.

Pi(X, u) = 2 f(X) . u - u^T K(X) u equals the compliance at the solution and is stationary in the free components of u, so
dJ/dX = dPi/dX at fixed u = gK + 2 sum over the tractions of gL:

    gK_v = -sum over the corners (e, a) of v of E_e g_a,   E = V (w I - 2 H^T S)        (emt, stiffness_gradient)
    gL_v = sum over the loaded faces of v of c_f dA_f/dx_v                              (load_gradient)

Each of the three takes absolute=True: the sum of the absolute values of the terms that are added (|lam|, |g|, |u|, |t| and the
absolute values of the face's edge and unit normal in place of the values), what a counted rounding bound is stated against.
pi(X) evaluates Pi by spsolve; variant= switches on the wrong forms the discrimination test evaluates."""
import numpy as np

from tests import fem_numpy as F

U = F.U
WRONG = ("no_load", "load_once", "energy_only", "transposed", "half", "boundary")


# ---- stiffness term ---------------------------------------------------------------------------------------------------------------
def emt(verts, tets, lam, mu, u, variant=None, absolute=False):
    """E [9, T], row-major 3 k + j (geom's layout): V (w I - 2 H^T S), (H^T S)_kj = sum_i H_ik S_ij; nine exact zeros for a skipped
    element.  variant: 'energy_only' (E = V w I), 'transposed' (H S for H^T S)."""
    tets = np.asarray(tets, dtype=np.int64)
    g, V = F.gradients(F.geometry(verts, tets)[0])
    u = np.asarray(u, dtype=np.float64)
    if absolute:
        g, u, lam = np.abs(g), np.abs(u), abs(lam)
    H = np.einsum("eai,eaj->eij", u[tets], g)
    tr = (H[:, 0, 0] + H[:, 1, 1]) + H[:, 2, 2]
    S = lam * tr[:, None, None] * np.eye(3)[None] + mu * (H + H.transpose(0, 2, 1))
    w = lam * tr * tr + mu * np.einsum("eij,eij->e", H, H + H.transpose(0, 2, 1))
    HS = np.einsum("eki,eij->ekj", H, S) if variant == "transposed" else np.einsum("eik,eij->ekj", H, S)
    if variant == "energy_only":
        HS = np.zeros_like(HS)
    sign = 1.0 if absolute else -1.0
    E = V[:, None, None] * (w[:, None, None] * np.eye(3)[None] + sign * 2.0 * HS)
    E = np.where((V > 0.0)[:, None, None], E, 0.0)
    return E.reshape(len(tets), 9).T.copy()


def stiffness_gradient(verts, tets, lam, mu, u, variant=None, absolute=False):
    """gK [V, 3] = -sum over the vertex's corners of E g_a (absolute: + sum |E|_terms |g_a|)."""
    tets = np.asarray(tets, dtype=np.int64)
    g = F.gradients(F.geometry(verts, tets)[0])[0]
    E = emt(verts, tets, lam, mu, u, variant, absolute).T.reshape(-1, 3, 3)
    if absolute:
        g = np.abs(g)
    c = np.einsum("ekj,eaj->eak", E, g)
    out = np.zeros((len(verts), 3))
    np.add.at(out, tets.reshape(-1), c.reshape(-1, 3))
    return out if absolute else -out


# ---- load term --------------------------------------------------------------------------------------------------------------------
def _cross(a, b, absolute):
    if absolute:
        a, b = np.abs(a), np.abs(b)
        return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], 1)
    return F._cross(a, b)


def load_gradient(verts, bfaces, sel, t, mask, u, absolute=False):
    """gL [V, 3] for one traction t on the faces sel: sum over the vertex's selected faces (a, b, c) of c_f dA_f/dx_v with
    c_f = ((u~_a + u~_b) + u~_c) . t / 3 (u~: u zeroed at masked vertices), dA/dx_a = n^ x (x_c - x_b) / 2, dA/dx_b = n^ x (x_a - x_c) / 2,
    dA/dx_c = n^ x (x_b - x_a) / 2, n^ = N / |N|, N = (b - a) x (c - a).  A face with |N| == 0 or a non-finite n^ adds exact zeros."""
    bf = np.asarray(bfaces, dtype=np.int64)
    X = np.asarray(verts, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    N = F.face_normals(X, bf)
    norm = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        nh = N / norm[:, None]
    ok = (norm != 0.0) & np.isfinite(nh).all(1) & np.asarray(sel, dtype=bool)
    nh = np.where(ok[:, None], nh, 0.0)
    um = np.where(np.asarray(mask, dtype=bool)[:, None], 0.0, np.asarray(u, dtype=np.float64))
    if absolute:
        um, t = np.abs(um), np.abs(t)
    s = (um[bf[:, 0]] + um[bf[:, 1]]) + um[bf[:, 2]]
    cf = ((s[:, 0] * t[0] + s[:, 1] * t[1]) + s[:, 2] * t[2]) / 3.0
    x = X[bf]
    out = np.zeros((len(X), 3))
    for k, (p, q) in enumerate(((2, 1), (0, 2), (1, 0))):                  # corner k: n^ x (x_p - x_q) / 2
        d = _cross(nh, x[:, p] - x[:, q], absolute) * 0.5
        np.add.at(out, bf[:, k], np.where(ok[:, None], cf[:, None] * d, 0.0))
    return out


# ---- today's boundary formula (the reference's), for comparison -----------------------------------------------------------------------
def boundary_formula(verts, tets, bfaces, lam, mu, u):
    w, V = F.energy_density(verts, tets, lam, mu, u)
    return F.boundary_gradient(verts, bfaces, weight=-F.nodal_density(tets, w, V, len(verts), "mean"))


def compliance_gradient(verts, tets, bfaces, lam, mu, mask, u, tractions, variant=None):
    """gC [V, 3] = gK + 2 sum gL over tractions [(sel, t)].  variant: None or one of WRONG -- 'no_load' (gK alone), 'load_once'
    (gK + gL), 'energy_only', 'transposed' (emt's), 'half' (the whole gradient halved), 'boundary' (-w_v sum A_f n_f / 3)."""
    if variant == "boundary":
        return boundary_formula(verts, tets, bfaces, lam, mu, u)
    gK = stiffness_gradient(verts, tets, lam, mu, u, variant if variant in ("energy_only", "transposed") else None)
    gL = sum(load_gradient(verts, bfaces, sel, t, mask, u) for sel, t in tractions)
    if variant == "no_load":
        return gK
    if variant == "load_once":
        return gK + gL
    return 0.5 * (gK + 2.0 * gL) if variant == "half" else gK + 2.0 * gL


# ---- the problem the tests differentiate --------------------------------------------------------------------------------------------
TRACTION = (0.0, 0.0, -0.01)


class Problem:
    """One of fem_numpy.cpu_meshes() with attribute 1 clamped and TRACTION on attribute 2 (attribute 3 where no face carries 2).
    The attributes, the mask and the selection come from the unperturbed mesh and stay."""

    def __init__(self, mesh, lam, mu):
        v, t, bf, _ = mesh
        self.X = np.asarray(v, dtype=np.float64)
        self.t, self.bf = np.asarray(t, dtype=np.int64), np.asarray(bf, dtype=np.int64)
        self.lam, self.mu = float(lam), float(mu)
        self.attr = F.attributes(self.X, self.bf)
        self.loaded = 2 if (self.attr == 2).any() else 3
        self.sel = self.attr == self.loaded
        nv = len(self.X)
        self.skipped = F.geometry(self.X, self.t)[1]
        self.mask = F.held_vertices(self.t, self.skipped, nv) | F.fixed_vertices(self.bf, self.attr == 1, nv)
        self.tractions = [(self.sel, TRACTION)]

    def solve(self, X=None):
        """(u, f) by spsolve on the vertices X (default: the mesh's)."""
        X = self.X if X is None else X
        A = F.masked(F.assemble(X, self.t, self.lam, self.mu), self.mask)
        f = F.load(X, self.bf, self.sel, TRACTION, self.mask)
        return F.spsolve(A, f), f

    def pi(self, X=None):
        """Pi = 2 f . u - u^T K u at the solution u of the vertices X: f . A^-1 f, the compliance."""
        u, f = self.solve(X)
        return float((f * u).sum())

    def gradient(self, variant=None, u=None):
        u = self.solve()[0] if u is None else u
        return compliance_gradient(self.X, self.t, self.bf, self.lam, self.mu, self.mask, u, self.tractions, variant)


def theta(n_verts, seed):
    return np.random.default_rng(seed).standard_normal((n_verts, 3))


def central_difference(fun, X, th, h):
    return (fun(X + h * th) - fun(X - h * th)) / (2.0 * h)


def fd_error(fd, g, g_exact, th):
    """|fd - g . theta| / sum |g_exact . theta| (term-wise)."""
    return abs(fd - float((g * th).sum())) / float(np.abs(g_exact * th).sum())
