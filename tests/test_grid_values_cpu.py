"""No GPU: the inputs of tests/test_gpu_grid_values.py (tests/grid_values.py) carry what they promise, the oracle's
mesh of every finite one is a conforming mesh, and the inputs have power: each WRONG variant of the tie rules (tet_numpy.VARIANTS,
voldiff_numpy.TIE_VARIANTS) changes an output on the grid built for it and changes nothing on the continuous random grid that every
earlier kernel-level test used."""
import numpy as np
import pytest

from tests import grid_values as gv, tet_numpy, voldiff_numpy as vd

FIELDS, SPACING, ORIGIN, GRIDS = gv.FIELDS, gv.SPACING, gv.ORIGIN, gv.GRIDS
FINITE = [("quantised", 0.0), ("quantised", 0.25), ("quantised", -0.5), ("signed_zero", 0.0), ("signed_zero", -0.0),
          ("clamp_edges_0.05", 0.0), ("clamp_edges_0.25", 0.0), ("magnitudes", 0.0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Every array of two oracle meshes has the same shape and bytes."""
    return all(getattr(a, f).shape == getattr(b, f).shape and getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in FIELDS)


_MESH = {}


def mesh(name, level=0.0, tau=0.0, variant=None):
    key = (name, repr(float(level)), tau, variant)
    if key not in _MESH:
        g = gv.uniform() if name == "uniform" else GRIDS[name]()
        _MESH[key] = tet_numpy.tetrahedralize(g, level, SPACING, ORIGIN, t_clamp=tau, variant=variant)
    return _MESH[key]


# ---- the inputs carry what they promise -------------------------------------------------------------------------------------------
def test_the_shared_constants_are_the_tet_mesher_tests_own():
    """gv.uniform() is the 9 x 8 x 7 grid of tests/test_gpu_tetmesh.py, and spacing, origin and the arrays' names are its too."""
    from tests import test_gpu_tetmesh as tm
    assert gv.uniform().tobytes() == tm.GRIDS["9x8x7"]().tobytes() and gv.uniform().shape == tm.GRIDS["9x8x7"]().shape == gv.SHAPE
    assert (gv.FIELDS, gv.SPACING, gv.ORIGIN) == (tm.FIELDS, tm.SPACING, tm.ORIGIN)
    assert len(gv.CONTENTS) == 7 and sum(n == "signed_zero" for n, _, _ in gv.CONTENTS) == 2


@pytest.mark.parametrize("name,level,want", gv.CONTENTS, ids=[f"{n}-{lv!r}" for n, lv, _ in gv.CONTENTS])
def test_every_grid_contains_what_it_states(name, level, want):
    g = GRIDS[name]()
    assert g.shape == gv.SHAPE and g.dtype == np.float32
    have = gv.measure(g, level)
    want = dict(want)
    zero_volume = want.pop("zero_volume", None)
    print(f"{name} at level {level!r}: {have}")
    for k, n in want.items():
        assert have[k] >= n, (name, level, k, have[k], n)
    assert have["classes"] == [1, 2, 3, 4, 5, 6, 7]
    if zero_volume is not None:
        m = mesh(name, level)
        vol = tet_numpy.volumes(m.verts, m.tets)
        print(f"{name} at level {level!r}: {int((vol == 0).sum())} zero-volume elements of {len(vol)}")
        assert (vol == 0).sum() >= zero_volume and not (vol < 0).any()


def test_the_uniform_grid_contains_none_of_it():
    have = gv.measure(gv.uniform())
    assert all(have[k] == 0 for k in have if k != "classes"), have


def test_signed_zero_is_what_the_caps_leave():
    g, u = gv.signed_zero(), gv.uniform()
    assert (bits(g[0][u[0] < 0]) == 0x80000000).all() and (u[0] < 0).sum() >= 20          # a whole outer plane
    assert not tet_numpy.is_inside(g[0]).any()                                            # equal to the level: outside
    interior = np.zeros(gv.SHAPE, dtype=bool)
    interior[1:-1, 1:-1, 1:-1] = True
    assert (bits(g)[interior] == 0x80000000).sum() == 24 and (bits(g) == 0).sum() == 8


@pytest.mark.parametrize("tau", gv.TAUS)
def test_clamp_edges_plants_all_six_per_class(tau):
    """Each planted t has the stated bits in the mesher's own sequence, and the oracle's fp32 rule says by name which of them moves:
    t == tau and t == 1 - tau move, one ulp outside is held."""
    g, plants = gv.clamp_edges(tau)
    f = g.reshape(-1)
    targets = gv.clamp_targets(tau)
    assert targets[0] < targets[1] < targets[2] < targets[3] < targets[4] < targets[5]
    assert bits(targets[1]) == bits(np.float32(tau)) and bits(targets[4]) == bits(np.float32(1) - np.float32(tau))
    _, _, vp, vc = tet_numpy.vertices(g)
    mv = vd.moves(g, vp, vc, tau)
    seen = set()
    for pl in plants:
        assert (f[pl["p"]] < 0) != (f[pl["q"]] < 0)
        assert bits(tet_numpy.edge_t(f[pl["p"]], f[pl["q"]], 0.0)) == bits(pl["t"])
        v = np.nonzero((vp == pl["p"]) & (vc == pl["cls"]))[0]
        assert len(v) == 1, pl
        assert bool(mv[v[0]]) == pl["moves"], (pl["cls"], pl["kind"])
        seen.add((pl["cls"], pl["kind"], bool(f[pl["p"]] < 0)))
    assert {s[:2] for s in seen} == {(c, k) for c in range(1, 8) for k, _ in gv.KINDS}
    assert {s[2] for s in seen} == {True, False}                                          # the inside end is p on some, q on others


def test_magnitudes_in_ieee_arithmetic():
    g, plants = gv.magnitudes()
    f = g.reshape(-1)
    tiny = np.finfo(np.float32).tiny
    for pl in plants:
        t = tet_numpy.edge_t(f[pl["p"]], f[pl["q"]], 0.0)
        if pl["what"] == "subnormal difference":
            assert 0 < abs(float(f[pl["q"]]) - float(f[pl["p"]])) < tiny and t == 0.5
        elif pl["what"] == "overflowing difference":
            with np.errstate(over="ignore"):
                assert np.isinf(f[pl["q"]] - f[pl["p"]]) and t == 0 and np.isfinite(f[[pl["p"], pl["q"]]]).all()
        else:
            assert min(abs(f[pl["p"]]), abs(f[pl["q"]])) < tiny and (t == 1 or 0 < t < tiny)
    assert len(plants) == 7 * len(gv.MAGNITUDE_PAIRS)
    assert np.isfinite(mesh("magnitudes").verts).all()


# ---- the oracle's meshes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", (0.0,) + gv.TAUS)
@pytest.mark.parametrize("name,level", FINITE, ids=lambda v: repr(v))
def test_every_finite_grid_gives_a_conforming_mesh(name, level, tau):
    m = mesh(name, level, tau)
    assert len(m.tets) > 0 and len(m.bfaces) > 0
    vol, surf, bound = tet_numpy.check_invariants(m, positive=tau > 0)
    assert abs(vol - surf) <= bound
    m0 = mesh(name, level, 0.0)                                  # the clamp moves vertices and nothing else
    assert all(getattr(m, f).tobytes() == getattr(m0, f).tobytes() for f in FIELDS[1:])
    assert (len(m.verts), len(m.tets), len(m.bfaces)) == tet_numpy.counts(GRIDS[name](), level)


def test_level_minus_zero_is_level_zero():
    for name in ("signed_zero", "quantised"):
        for tau in (0.0, 0.05):
            assert same(mesh(name, -0.0, tau), mesh(name, 0.0, tau)), (name, tau)
        g = GRIDS[name]()
        for a, b in zip(tet_numpy.components(g, -0.0), tet_numpy.components(g, 0.0)):
            assert np.array_equal(a, b)


def test_non_finite_values_follow_the_comparison():
    """v < level decides: NaN and +inf are outside, -inf is inside.  The topology is the twin's; the coordinates differ from the
    twin's only on the planted points' own edges; a NaN t stays NaN under every t_clamp."""
    v = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    assert tet_numpy.is_inside(v).tolist() == [False, False, True, False, False]
    assert tet_numpy.is_inside(v, -0.0).tolist() == [False, False, True, False, False]
    g, twin, planted = gv.non_finite()
    assert np.array_equal(tet_numpy.is_inside(g), tet_numpy.is_inside(twin))
    for tau in (0.0,) + gv.TAUS:
        m = tet_numpy.tetrahedralize(g, 0.0, SPACING, ORIGIN, t_clamp=tau)
        t = tet_numpy.tetrahedralize(twin, 0.0, SPACING, ORIGIN, t_clamp=tau)
        assert all(getattr(m, f).tobytes() == getattr(t, f).tobytes() for f in FIELDS[1:])
        q, _ = vd.far_point(g.shape, m.vert_point, m.vert_class)
        touched = planted[m.vert_point] | planted[q]
        differs = (bits(m.verts) != bits(t.verts)).any(1)
        assert not differs[~touched].any() and differs.any()
        nan = np.isnan(m.verts).any(1)
        print(f"non_finite, t_clamp {tau}: {int(np.isnan(m.verts).sum())} NaN coordinates on {int(nan.sum())} vertices, "
              f"{int(differs.sum())} vertices differ from the twin's")
        assert nan.sum() >= 30 and not (nan & ~touched).any() and not np.isinf(m.verts).any()
        assert np.array_equal(bits(vd.vertices_from_edges(g, m.vert_point, m.vert_class, tau, 0.0, SPACING, ORIGIN)), bits(m.verts))
        held = ~vd.moves(g, m.vert_point, m.vert_class, tau)
        if tau > 0:
            assert held[nan].all()                                # in the derivative a NaN t is held


# ---- the inputs have power -----------------------------------------------------------------------------------------------------------
def test_a_tie_counted_inside_shows_on_quantised_and_signed_zero_only():
    for name, level in (("quantised", 0.0), ("quantised", 0.25), ("signed_zero", 0.0), ("signed_zero", -0.0)):
        right, wrong = mesh(name, level), mesh(name, level, variant="le_inside")
        assert right.tets.shape != wrong.tets.shape or not np.array_equal(right.tets, wrong.tets), (name, level)
        g = GRIDS[name]()
        assert tet_numpy.counts(g, level) != (len(wrong.verts), len(wrong.tets), len(wrong.bfaces))
        assert not np.array_equal(tet_numpy.components(g, level)[0], tet_numpy.components(g, level, variant="le_inside")[0])
    for level in (0.0, 0.25):
        assert same(mesh("uniform", level), mesh("uniform", level, variant="le_inside"))
    u = gv.uniform()
    assert np.array_equal(tet_numpy.components(u)[0], tet_numpy.components(u, variant="le_inside")[0])


@pytest.mark.parametrize("tau", gv.TAUS)
def test_a_strict_clamp_rule_shows_on_clamp_edges_only(tau):
    g, plants = gv.clamp_edges(tau)
    _, _, vp, vc = tet_numpy.vertices(g)
    right, wrong = vd.moves(g, vp, vc, tau), vd.moves(g, vp, vc, tau, variant="strict_clamp")
    on_boundary = {(pl["p"], pl["cls"]) for pl in plants if pl["kind"] in ("tau", "hi")}
    assert {(int(vp[v]), int(vc[v])) for v in np.nonzero(right != wrong)[0]} == on_boundary and len(on_boundary) == 14
    u = gv.uniform()
    _, _, up, uc = tet_numpy.vertices(u)
    for t in gv.TAUS:
        assert np.array_equal(vd.moves(u, up, uc, t), vd.moves(u, up, uc, t, variant="strict_clamp"))
        assert 0 < vd.moves(u, up, uc, t).sum() < (uc > 0).sum()                          # the rule holds some and moves some there


@pytest.mark.parametrize("tau", gv.TAUS)
def test_an_fmin_fmax_clamp_shows_on_non_finite_only(tau):
    right, wrong = mesh("non_finite", 0.0, tau), mesh("non_finite", 0.0, tau, variant="fminmax_clamp")
    assert np.isnan(right.verts).sum() >= 30 and np.isfinite(wrong.verts).all()
    for name, level in FINITE + [("uniform", 0.0), ("uniform", 0.25)]:
        assert same(mesh(name, level, tau), mesh(name, level, tau, variant="fminmax_clamp")), (name, level)


def test_the_sign_of_a_zero_t_cannot_reach_a_coordinate():
    """t = -0.0 is common (p tied with the level, q inside: +0 / negative) and |t| changes its bits; but a coordinate is
    origin + (idx + t) * spacing with idx >= +0, and (+0) + (-0) = +0 in round-to-nearest: in the stated sequence no output depends on
    the sign of a zero t.  So the variant "abs_t" changes t on these grids and no coordinate on any finite grid -- the property the
    GPU test then pins bit for bit at idx = 0 on the low planes.  On non_finite it changes only which NaN a coordinate is."""
    for name, level in (("signed_zero", 0.0), ("quantised", 0.0), ("quantised", 0.25)):
        have = gv.measure(GRIDS[name](), level)
        assert have["t_neg_zero"] >= 40
        m = mesh(name, level)
        on_low_plane = (m.vert_class > 0) & (np.stack(np.unravel_index(m.vert_point, gv.SHAPE), 1) == 0).any(1)
        assert on_low_plane.sum() >= 10
    for name, level in FINITE + [("uniform", 0.0)]:
        for tau in (0.0, 0.05):
            assert same(mesh(name, level, tau), mesh(name, level, tau, variant="abs_t")), (name, level, tau)
    right, wrong = mesh("non_finite"), mesh("non_finite", variant="abs_t")
    assert np.array_equal(np.isnan(right.verts), np.isnan(wrong.verts))
    fin = ~np.isnan(right.verts)
    assert np.array_equal(bits(right.verts)[fin], bits(wrong.verts)[fin])
