"""CPU: the oracle of the exact discrete compliance gradient (tests/femgrad_numpy.py) against a central difference of
the compliance itself, the discrimination of every wrong form, the degenerate mesh, and the argument checks of the two C entries
without a device."""
import ctypes as C

import numpy as np
import pytest

from tests import fem_numpy as F
from tests import femgrad_numpy as G

MESHES = ("one tet", "2x2x2", "3x3x3", "cut")
LAME = ((0.7, 1.3), (0.0, 105.0))
SEEDS = (0, 1, 2, 3)
H1, H2 = 1e-4, 1e-5
RIGHT_AT_H1 = 1e-6           # measured worst 4.96e-7 (cut); the margin of 2 is for other BLAS builds
ORDER_GAIN = 30.0            # second order gives 100 from h = 1e-4 to 1e-5; 100 was measured
MISS = 1000.0                # a wrong form misses by more than this many times what the right one leaves


@pytest.fixture(scope="module")
def meshes():
    return F.cpu_meshes()


@pytest.fixture(scope="module")
def differences(meshes):
    """{(mesh, lam, mu): (problem, u, g, {(seed, h): central difference})}: every solve once."""
    out = {}
    for name in MESHES:
        for lam, mu in LAME:
            p = G.Problem(meshes[name], lam, mu)
            u = p.solve()[0]
            fd = {(s, h): G.central_difference(p.pi, p.X, G.theta(len(p.X), s), h) for s in SEEDS for h in (H1, H2)}
            out[name, lam, mu] = (p, u, p.gradient(u=u), fd)
    return out


@pytest.mark.parametrize("lam,mu", LAME)
@pytest.mark.parametrize("name", MESHES)
def test_the_gradient_is_the_derivative_of_the_compliance(differences, name, lam, mu):
    p, u, g, fd = differences[name, lam, mu]
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    err = {h: max(G.fd_error(fd[s, h], g, g, G.theta(len(p.X), s)) for s in SEEDS) for h in (H1, H2)}
    print(f"{name} lam {lam} mu {mu}: worst error h={H1:g} {err[H1]:.3e}, h={H2:g} {err[H2]:.3e}, gain {err[H1] / err[H2]:.1f}")
    assert err[H1] <= RIGHT_AT_H1
    assert err[H1] >= ORDER_GAIN * err[H2]
    # the two terms are of one size: neither may be left out
    gK = G.stiffness_gradient(p.X, p.t, lam, mu, u)
    gL = G.load_gradient(p.X, p.bf, p.sel, G.TRACTION, p.mask, u)
    assert 0.1 < np.abs(gL).max() / np.abs(gK).max() < 10.0
    assert np.array_equal(g, gK + 2.0 * gL)


@pytest.mark.parametrize("variant", G.WRONG)
@pytest.mark.parametrize("lam,mu", LAME)
@pytest.mark.parametrize("name", MESHES)
def test_every_wrong_form_misses_the_same_difference(differences, name, lam, mu, variant):
    p, u, g, fd = differences[name, lam, mu]
    gw = p.gradient(variant, u=u)
    right = max(G.fd_error(fd[s, H1], g, g, G.theta(len(p.X), s)) for s in SEEDS)
    miss = min(G.fd_error(fd[s, H1], gw, g, G.theta(len(p.X), s)) for s in SEEDS)
    print(f"{name} lam {lam} mu {mu} {variant}: smallest miss {miss:.3e}, the right form's worst {right:.3e}, ratio {miss / right:.1f}")
    assert miss > MISS * right


def test_boundary_formula_has_the_wrong_sign_along_the_normals(meshes):
    """Perturbations along the boundary normals, what the optimiser moves: on the single tetrahedron the reference's formula and
    the central difference disagree in sign; the exact gradient agrees to 6 digits."""
    p = G.Problem(meshes["one tet"], 0.0, 105.0)
    th = F.boundary_gradient(p.X, p.bf)
    th = th / np.linalg.norm(th, axis=1, keepdims=True)
    fd = G.central_difference(p.pi, p.X, th, H1)
    exact, boundary = float((p.gradient() * th).sum()), float((p.gradient("boundary") * th).sum())
    assert abs(fd - exact) <= 1e-6 * abs(fd) and fd * boundary < 0


def test_degenerate_mesh_is_finite_and_exactly_zero_where_nothing_is_differentiable(meshes):
    p = G.Problem(meshes["degenerate"], 0.7, 1.3)
    N = F.face_normals(p.X, p.bf)
    flat = (N == 0).all(1)
    assert p.skipped.sum() == 53 and flat.sum() == 44 and (flat & p.sel).sum() == 1
    for u in (p.solve()[0], np.random.default_rng(11).standard_normal(p.X.shape)):
        E = G.emt(p.X, p.t, p.lam, p.mu, u)
        assert np.isfinite(E).all() and not E[:, p.skipped].any() and E[:, ~p.skipped].any()
        g = p.gradient(u=u)
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        # the skipped elements: the same gradient from the mesh without them
        assert np.array_equal(G.stiffness_gradient(p.X, p.t, p.lam, p.mu, u), G.stiffness_gradient(p.X, p.t[~p.skipped], p.lam, p.mu, u))
        # the zero-area faces: nothing from them alone, and the same gradient without them
        assert not G.load_gradient(p.X, p.bf, flat, G.TRACTION, p.mask, u).any()
        assert np.array_equal(G.load_gradient(p.X, p.bf, p.sel, G.TRACTION, p.mask, u),
                              G.load_gradient(p.X, p.bf, p.sel & ~flat, G.TRACTION, p.mask, u))
        a = G.load_gradient(p.X, p.bf, p.sel, G.TRACTION, p.mask, u, absolute=True)
        assert np.isfinite(a).all() and (a >= np.abs(G.load_gradient(p.X, p.bf, p.sel, G.TRACTION, p.mask, u))).all()


def test_gradient_entries_are_exported_and_refuse_bad_arguments_before_any_launch():
    from deepsdf_amd import _lib
    lib = _lib.lib()
    bad, short = -1, -2
    p = 0x1000                                                        # never dereferenced: every call below fails before a launch
    P, Q, R, N = C.c_void_p(p), C.c_void_p(0x2000), C.c_void_p(0x3000), C.c_void_p(0)
    b = C.c_size_t()
    assert lib.dsdf_fem_plan(100, 300, 50, C.byref(b)) == 0
    big = 1 << 24

    def op(**kw):
        d = dict(tets=p, corner_order=p, vstart=p, geom=p, dinv=p, mask=p, n_verts=100, n_tets=300, lam=0.0, mu=105.0)
        d.update(kw)
        return C.byref(_lib.DsdfFemOp(**d))
    sg = lib.dsdf_fem_stiffness_gradient
    assert sg(None, P, Q, R, P, big, N) == bad
    for k in ("tets", "corner_order", "vstart", "geom", "dinv", "mask"):
        assert sg(op(**{k: 0}), P, Q, R, P, big, N) == bad, k
    assert sg(op(tets=0x1004), P, Q, R, P, big, N) == bad and b"aligned" in lib.dsdf_last_error()
    assert sg(op(n_verts=0), P, Q, R, P, big, N) == bad and sg(op(mu=0.0), P, Q, R, P, big, N) == bad
    assert sg(op(), P, Q, R, N, big, N) == bad and sg(op(), P, Q, R, C.c_void_p(0x1010), big, N) == bad
    assert sg(op(), P, Q, R, P, b.value - 1, N) == short
    assert sg(op(), N, Q, R, P, big, N) == bad and sg(op(), P, N, R, P, big, N) == bad and sg(op(), P, Q, N, P, big, N) == bad
    assert sg(op(), P, Q, P, P, big, N) == bad and b"u == grad" in lib.dsdf_last_error()
    assert sg(op(), P, P, R, P, big, N) == bad and sg(op(), P, Q, Q, P, big, N) == bad
    lg = lib.dsdf_fem_load_gradient
    t3 = (C.c_double * 3)(0.0, 0.0, -0.01)
    ok = dict(verts=P, nv=100, bf=P, nb=50, border=P, bvstart=P, sel=N, t=t3, mask=N, u=Q, grad=R)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lg(a["verts"], a["nv"], a["bf"], a["nb"], a["border"], a["bvstart"], a["sel"], a["t"], a["mask"], a["u"], a["grad"], N)
    for k in ("verts", "bf", "border", "bvstart", "u", "grad"):
        assert call(**{k: N}) == bad, k
    assert call(t=None) == bad and call(nv=0) == bad and call(nb=-1) == bad
    assert call(u=R) == bad and b"u == grad" in lib.dsdf_last_error()
    for v in (float("inf"), float("-inf"), float("nan")):
        for i in range(3):
            t = [0.0, 0.0, -0.01]
            t[i] = v
            assert call(t=(C.c_double * 3)(*t)) == bad and b"traction" in lib.dsdf_last_error()
    # dsdf_fem_plan is what it was: the gradient entries add no region (fem_sigma holds 6 doubles per element; emt is the caller's)
    assert lib.dsdf_fem_plan(100, 300, 50, C.byref(b)) == 0
    rows, total = _lib.ws_regions()
    assert [r[0] for r in rows] == ["fem_sigma", "fem_r", "fem_z", "fem_p", "fem_ap", "fem_part0", "fem_part1", "fem_cnt", "fem_scal"]
    assert total == b.value and dict((r[0], r[2]) for r in rows)["fem_sigma"] == 300 * 6 * 8
