"""-m gpu: the mesh SDF (csrc/meshsdf.hpp through deepsdf_amd.meshsdf.TriangleMesh) where whole well-shaped unit meshes do not
look: one face at a time in every Voronoi region, slivers down to a height of 1e-6 of the longest edge (alone, and inside a
closed plate and an open ribbon), exact arithmetic and the tie rule on a dyadic cube, powers-of-two scalings, a translated mesh,
and the values at every branch of the planner's split rule.  The reference is the fp64 oracle of tests/meshsdf_numpy.py on the
fp32-rounded inputs; TOL, W_TOL and the sign band are tests/test_gpu_meshsdf.py's.  Every test prints its measured maxima."""
import functools

import numpy as np
import pytest

from tests import meshsdf_numpy as mn
from tests.test_gpu_meshsdf import TOL, W_TOL, _check_against_oracle, _mesh, _near_surface
from tests.test_gpu_workspace import MSDF_CASES

pytestmark = pytest.mark.gpu
AWAY = 1e-3          # winding numbers and signs are compared where the oracle's distance exceeds this


def _fmt(err):
    return {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in err.items() if k != "_ref"}


def _run(V, F, P):
    m = _mesh(V, F)
    d2, face, C = m.squared_distance(P)
    return dict(sdf=m.sdf(P), d2=d2, face=face, C=C, w=m.winding_number(P))


def _compare(V, F, P, o, sel=None):
    """Maxima of the outputs `o` of _run against the oracle; sel: the queries to compare (indices), default all of them."""
    if sel is not None:
        P, o = P[sel], {k: v[sel] for k, v in o.items()}
    P = np.asarray(P, np.float32).astype(np.float64)
    rd2, _, rC, rw = mn.mesh_query(V, F, P)
    rd = np.sqrt(rd2)
    C = o["C"].astype(np.float64)
    assert all(np.all(np.isfinite(v)) for v in o.values())
    err = dict(dist=np.abs(np.sqrt(o["d2"].astype(np.float64)) - rd).max(),                    # every query, no mask
               face=np.abs(mn.face_distance(V, F, P, o["face"]) - rd).max(),                   # the face attains the minimum
               closest=np.abs(np.linalg.norm(P - C, axis=1) - rd).max(),                       # the point is a closest point
               on_face=mn.face_distance(V, F, C, o["face"]).max())                             # ... and lies on that face
    away = rd > AWAY
    # the parity rule jumps at half-integer winding numbers (far from the surface of an open mesh): the sign is compared where
    # the oracle's winding number is further from the jump than the tolerance of w itself
    steady = away & (np.abs(np.abs(rw) % 1.0 - 0.5) > W_TOL)
    rsdf = np.where(mn.inside(rw), -rd, rd)
    err.update(w=float(np.abs(o["w"] - rw)[away].max()) if away.any() else 0.0,
               sdf_abs=np.abs(np.abs(o["sdf"].astype(np.float64)) - rd).max(),
               sdf=float(np.abs(o["sdf"] - rsdf)[steady].max()) if steady.any() else 0.0,
               near=float(1.0 - away.mean()), unsteady=int((away & ~steady).sum()), n=len(P))
    err["_ref"] = (rd, rC, rw)
    return err


def _assert_bounds(err, tol, w_tol=W_TOL):
    shown = _fmt(err)
    for k in ("dist", "face", "closest", "sdf_abs", "sdf"):
        assert err[k] <= tol, (k, shown)
    assert err["on_face"] <= 1e-5, shown
    assert err["w"] <= w_tol, shown
    assert err["unsteady"] <= 0.02 * err["n"], shown             # the sign comparison leaves out next to nothing


def _worst(acc, err):
    for k, v in err.items():
        if k != "_ref":
            acc[k] = max(acc.get(k, 0), v)


# ---- 1. one well-shaped triangle, all seven regions -----------------------------------------------------------------------------
def _well_shaped_triangle(g):
    while True:
        T = g.uniform(-1, 1, (3, 3))
        e = [T[(k + 1) % 3] - T[k] for k in range(3)]
        cos = [-(e[k] @ e[k - 1]) / np.linalg.norm(e[k]) / np.linalg.norm(e[k - 1]) for k in range(3)]
        if max(cos) <= np.cos(np.radians(35)) and min(np.linalg.norm(x) for x in e) >= 0.5:
            return T


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_triangle_in_every_region(seed):
    g = np.random.default_rng([1, seed])
    T = _well_shaped_triangle(g)
    n = np.cross(T[1] - T[0], T[2] - T[0])
    n /= np.linalg.norm(n)
    uv = g.uniform(-1.2, 2.2, (2400, 2))           # barycentric coordinates well beyond the face on every side
    z = np.where(np.arange(2400) % 3 == 0, 0.0, g.normal(0, 0.2, 2400))
    Q = T[0] + uv[:, :1] * (T[1] - T[0]) + uv[:, 1:] * (T[2] - T[0]) + z[:, None] * n
    R, off = mn.random_rotation(g), g.uniform(-0.5, 0.5, 3)
    V, P = mn._f32(T @ R.T + off), mn._f32(Q @ R.T + off)
    worst = {}
    for order in mn.VERTEX_ORDERS:
        F = np.array([order], dtype=np.int64)
        count = np.bincount(mn.regions(P, *(V[i] for i in order)), minlength=7)
        assert count.min() >= 50, dict(zip(mn.REGIONS, count))
        o = _run(V, F, P)
        err = _compare(V, F, P, o)
        err["point"] = np.abs(o["C"] - err["_ref"][1]).max()
        assert np.all(o["face"] == 0)
        _assert_bounds(err, TOL)
        assert err["point"] <= TOL, _fmt(err)
        _worst(worst, err)
    print("regions", seed, dict(zip(mn.REGIONS, count)), _fmt(worst))


# ---- 2. the sliver sweep on one triangle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", mn.SLIVER_HEIGHTS)
def test_sliver_sweep(h):
    """Height h against a unit longest edge, two families, six vertex orders, three poses, 1050 queries each.  Bounds: TOL down to
    h = 1e-5; TOL + h at 1e-6, which the three edge segments alone attain."""
    tol = TOL + h if h < 5e-6 else TOL
    worst = {}
    for family, V, F, P in mn.sliver_cases(h):
        assert not mn.is_zero_area(V, F).any()                   # a decade above the zero-area threshold: the oracle's side ...
        o = _run(V, F, P)
        assert np.any(o["w"] != 0)                               # ... and the kernel's (a zero-area face adds no winding at all)
        err = _compare(V, F, P, o)
        assert np.all(o["face"] == 0)
        _worst(worst, err)
    print("sliver", h, _fmt(worst))
    _assert_bounds(worst, tol)


# ---- 3. slivers inside meshes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1e-1, 1e-2, 1e-3, 1e-4])
def test_closed_plate(t):
    g = np.random.default_rng([3, int(round(-np.log10(t)))])
    V, F = mn.plate(t, g)
    P = mn.plate_queries(V, F, t, g)
    err = _check_against_oracle(V, F, P)
    print("plate", t, _fmt(err))


@pytest.mark.parametrize("aspect", [1e-2, 1e-3, 1e-4])
def test_open_ribbon_of_needles(aspect):
    g = np.random.default_rng([4, int(round(-np.log10(aspect)))])
    V, F = mn.ribbon(aspect, g)
    assert not mn.is_zero_area(V, F).any()
    P = mn.plate_queries(V, F, aspect, g)
    err = _compare(V, F, P, _run(V, F, P))
    print("ribbon", aspect, _fmt(err))
    for k in ("dist", "face", "closest", "sdf_abs", "sdf"):
        assert err[k] <= TOL, (k, _fmt(err))
    assert err["on_face"] <= 1e-5 and err["unsteady"] <= 0.02 * err["n"], _fmt(err)


# ---- 4. exact arithmetic on the dyadic cube ---------------------------------------------------------------------------------------
def _lattice():
    ax = np.arange(-2, 2.25, 0.25)
    return np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)


def _assert_bit_exact(V, F, P):
    """d2, face and closest equal the fp64 oracle bit for bit (every intermediate on either side is a small dyadic rational, so
    both are exact); the sign is exact and w within 1e-5 of the oracle's integer off the surface.  Returns (outputs, oracle)."""
    o = _run(V, F, P)
    rd2, rface, rC, rw = mn.mesh_query(V, F, P)
    assert np.array_equal(rd2, rd2.astype(np.float32)) and np.array_equal(rC, rC.astype(np.float32))
    assert np.array_equal(o["d2"], rd2.astype(np.float32))
    assert np.array_equal(o["face"], rface)                      # the LOWEST face index on ties
    assert np.array_equal(o["C"], rC.astype(np.float32))
    off = rd2 > 0
    assert np.sqrt(rd2[off]).min() >= 0.25
    rsdf = np.where(mn.inside(rw), -1.0, 1.0) * np.sqrt(rd2)
    assert np.array_equal(o["sdf"][off], rsdf[off].astype(np.float32))
    assert np.array_equal(np.abs(o["sdf"]), np.sqrt(rd2).astype(np.float32))
    werr = np.abs(o["w"] - np.round(rw))[off].max()
    assert np.abs(rw - np.round(rw))[off].max() <= 1e-12 and werr <= 1e-5, werr
    return o, (rd2, rface, rC, rw), werr


def test_dyadic_cube_is_bit_exact_and_ties_take_the_lowest_face():
    V, F = mn.cube()
    P = _lattice()
    o, (rd2, rface, _, _), werr = _assert_bit_exact(V, F, P)
    a, b, c = (V[F[:, k]] for k in range(3))
    per_face = ((P[:, None] - mn.closest_points(P[:, None], a[None], b[None], c[None])) ** 2).sum(-1)
    tied = ((per_face == rd2[:, None]).sum(1) >= 2).mean()
    assert tied >= 0.5, tied                                     # most lattice points have several faces at the exact minimum
    box = mn.box_sdf(P)
    assert np.array_equal(o["sdf"][box != 0], box[box != 0].astype(np.float32))
    assert np.array_equal(np.abs(o["sdf"]), np.abs(box).astype(np.float32))
    print(f"dyadic cube: {len(P)} lattice points, {tied:.0%} tied, w err {werr:.1e}")


def test_dyadic_zero_area_faces_at_the_lowest_indices():
    V, F = mn.cube()
    nv = len(V)
    extra = np.array([[-1.5, 0.5, 1.25], [-0.5, 0.5, 1.25], [0.5, 0.5, 1.25],          # collinear, edges 1, 1, 2
                      [0.25, 1.5, -0.75], [0.25, 2.0, -0.75],                          # a repeated vertex, edge 0.5
                      [-0.5, -1.75, 0.25]])                                            # a point
    Fz = np.array([[nv, nv + 1, nv + 2], [nv + 2, nv, nv + 1], [nv + 3, nv + 3, nv + 4], [nv + 5, nv + 5, nv + 5]])
    Vd, Fd = np.concatenate([V, extra]), np.concatenate([Fz, F])
    assert mn.is_zero_area(Vd, Fd).tolist() == [True] * 4 + [False] * 12
    o, (rd2, rface, _, _), werr = _assert_bit_exact(Vd, Fd, _lattice())
    hits = np.bincount(rface, minlength=16)[:4]
    assert hits[0] > 0 and hits[2] > 0 and hits[3] > 0 and hits[1] == 0, hits       # face 1 is face 0 again: it never wins a tie
    print(f"dyadic zero-area faces: wins per prepended face {hits.tolist()}, w err {werr:.1e}")


def test_dyadic_ties_across_face_ranges():
    """The cube's 12 faces 171 times over: 2052 faces in two ranges, every minimum attained in both, so the combine pass decides
    which face is reported (a 12-face mesh has one range and never asks it)."""
    V, F = mn.cube()
    Fr = np.tile(F, (171, 1))
    ax = np.arange(-2, 2.5, 0.5)
    P = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    m = _mesh(V, Fr)
    assert m.plan(len(P))[1] == 2
    d2, face, C = m.squared_distance(P)
    rd2, rface, rC, _ = mn.mesh_query(V, Fr, P)
    assert rface.max() < 12
    assert np.array_equal(d2, rd2.astype(np.float32)) and np.array_equal(face, rface) and np.array_equal(C, rC.astype(np.float32))
    print(f"dyadic ties across ranges: {len(P)} lattice points, {len(Fr)} faces, 2 ranges")


# ---- 5. scale and translation -----------------------------------------------------------------------------------------------------
def _scale_mesh(name):
    V, F = mn.icosphere(2) if name == "icosphere" else mn.torus()
    g = np.random.default_rng(51)
    P = np.concatenate([g.uniform(-1.2, 1.2, (1500, 3)), _near_surface(V, F, 500, 52)])
    return mn._f32(V), F, mn._f32(P)


@pytest.mark.parametrize("name", ["icosphere", "torus"])
def test_scaling_by_a_power_of_two_commutes(name):
    V, F, P = _scale_mesh(name)
    base = _run(V, F, P)
    err = _compare(V, F, P, base)
    _assert_bounds(err, TOL)
    for k in (-10, 10):
        s = np.float32(2.0 ** k)
        o = _run(V * 2.0 ** k, F, P * 2.0 ** k)
        werr = np.abs(o["w"] - base["w"]).max()
        print(f"scale 2^{k} {name}: w differs by {werr:.1e}; unit scale {_fmt({x: err[x] for x in ('dist', 'closest', 'w')})}")
        assert np.array_equal(o["face"], base["face"])
        assert np.array_equal(o["d2"], base["d2"] * s * s)
        assert np.array_equal(o["C"], base["C"] * s)
        assert np.array_equal(o["sdf"], base["sdf"] * s)          # the inside decision with it: the sign of sdf
        assert np.array_equal(o["sdf"] < 0, base["sdf"] < 0)
        assert werr <= 1e-6


@pytest.mark.parametrize("name", ["icosphere", "torus"])
def test_translated_mesh(name):
    """Mesh and queries moved by (64, -32, 128) and rounded to fp32: the kernel differences first, so its errors stay at the
    local scale.  The returned point is an fp32 number near 128: half an ulp per coordinate is up to (3.8, 1.9, 7.6)e-6, 8.7e-6
    in length, which the 1e-5 of the closest-point checks still covers."""
    V, F, P = _scale_mesh(name)
    t = np.array([64.0, -32.0, 128.0])
    err = _check_against_oracle(mn._f32(V + t), F, mn._f32(P + t))
    print("translated", name, _fmt(err))


# ---- 6. values at the split rule's branches ---------------------------------------------------------------------------------------
FULL_PAIRS = 2 * 10 ** 7        # above this many (face, query) pairs the oracle sees a fixed subset of the queries


@functools.lru_cache(maxsize=None)
def _icosphere6():
    V, F = mn.icosphere(6)
    return mn._f32(V), F


@functools.lru_cache(maxsize=None)
def _split_mesh(nf):
    V, F = _icosphere6()
    return V, F[:nf], _mesh(V, F[:nf])


@pytest.mark.parametrize("nf,nq", MSDF_CASES)
def test_values_at_the_split_branches(nf, nq):
    V, F, m = _split_mesh(nf)
    assert len(F) == nf
    P = mn._f32(np.random.default_rng([6, nf, nq]).uniform(-1.2, 1.2, (nq, 3)))
    d2, face, C = m.squared_distance(P)                          # the GPU always computes every query
    o = dict(sdf=m.sdf(P), d2=d2, face=face, C=C, w=m.winding_number(P))
    sel = None
    if nf * nq > FULL_PAIRS:
        sel = np.unique(np.concatenate([np.arange(256), np.arange(nq - 600, nq), np.arange(0, nq, 997)]))
    err = _compare(V, F, P, o, sel)
    print(f"split {nf} x {nq}: {m.plan(nq)[1]} ranges", _fmt(err))
    assert err["near"] <= 0.02, _fmt(err)
    _assert_bounds(err, TOL)


def test_the_split_sweep_visits_one_two_five_and_the_cap():
    seen = {_split_mesh(nf)[2].plan(nq)[1] for nf, nq in MSDF_CASES}
    assert {1, 2, 5, 64} <= seen, seen
