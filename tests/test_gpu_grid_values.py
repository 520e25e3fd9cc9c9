"""-m gpu: the grid-to-mesh chain -- marching cubes, the tetrahedral mesher, the solid's components, the two mesh derivatives -- on the
grid values the package really meshes (tests/grid_values.py): ties with the level, plateaus, zeros of both signs, t on
the clamp's boundaries, subnormal and overflowing differences, NaN and infinities.  The mesher, marching cubes and dsdf_vd_dtheta are
compared bit for bit with their numpy restatements, the contractions with the fp64 oracle at the bounds counted in
tests/voldiff_numpy.py and tests/msdiff_numpy.py, unchanged.  Every case is one or two launches on 504 points; every oracle mesh is
built once per module.  tests/test_grid_values_cpu.py shows on the CPU that these inputs tell the wrong tie rules from the right ones
and that the continuous random grid of the earlier tests does not.

Which NaN: IEEE 754 leaves the sign and payload of a NaN that an operation generates to the implementation (x86 sets the sign bit,
gfx950 does not), so where the specification's coordinate is a NaN the device's must be a NaN, and every other coordinate must have
the specification's bits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import grid_values as gv, mc_numpy, msdiff_numpy as mn, tet_numpy, voldiff_numpy as vd
from tests.test_gpu_tetmesh import _gpu, _host, _same_as_oracle

pytestmark = pytest.mark.gpu

FIELDS, SPACING, ORIGIN, GRIDS = gv.FIELDS, gv.SPACING, gv.ORIGIN, gv.GRIDS
LEVELS = [(n, lv) for n in GRIDS for lv in (0.0, 0.25)] + [("signed_zero", -0.0)]
TAUS = (0.0,) + gv.TAUS
DERIVATIVE_GRIDS = ("quantised", "signed_zero", "clamp_edges_0.05", "clamp_edges_0.25")
DEGREES, N_CP, L = mn.CASES["deg131_L2"]


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(what, got, want):
    """NaN where the specification has a NaN (any NaN: see the module's note), the specification's bits everywhere else."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, int(np.isnan(got).sum()), int(nan.sum()))
    d = int((bits(got)[~nan] != bits(want)[~nan]).sum())
    if d:
        print(f"{what}: {d} of {int((~nan).sum())} coordinates differ from the single-rounded specification, by at most "
              f"{mc_numpy.ulp_distance(got[~nan], want[~nan])} ulp")
    assert d == 0, (what, d)


_GRID, _ORACLE, _MC = {}, {}, {}


def grid(name):
    if name not in _GRID:
        _GRID[name] = GRIDS[name]()
    return _GRID[name]


def oracle(name, level, tau):
    key = (name, repr(float(level)), tau)
    if key not in _ORACLE:
        _ORACLE[key] = tet_numpy.tetrahedralize(grid(name), level, SPACING, ORIGIN, t_clamp=tau)
    return _ORACLE[key]


def mc_oracle(name, level):
    key = (name, repr(float(level)))
    if key not in _MC:
        with np.errstate(all="ignore"):
            _MC[key] = mc_numpy.marching_cubes(grid(name), level, SPACING, ORIGIN)
    return _MC[key]


def is_finite(name):
    return not name.startswith("non_finite") or name.endswith("twin")


# ---- the tetrahedral mesher ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name,level", LEVELS, ids=lambda v: repr(v))
def test_mesher_bit_for_bit_against_the_oracle(name, level, tau):
    g, r = grid(name), oracle(name, level, tau)
    m = _gpu(g, level, SPACING, ORIGIN, t_clamp=tau)
    assert (m.n_verts, m.n_tets, m.n_bfaces) == tet_numpy.counts(g, level)                # dsdf_tet_count's totals
    what = f"{name} level {level!r} t_clamp {tau}"
    if is_finite(name):
        h = _same_as_oracle(what, m, r)
        vol, surf, bound = tet_numpy.check_invariants(SimpleNamespace(**h), positive=tau > 0)
        assert abs(vol - surf) <= bound
    else:
        h = _host(m)
        for f in FIELDS[1:]:
            assert h[f].shape == getattr(r, f).shape and np.array_equal(h[f], getattr(r, f)), (what, f)
        same_floats(what, h["verts"], r.verts)
        assert np.isnan(r.verts).sum() >= 30                                              # a NaN t stays NaN under every t_clamp
    assert len(h["tets"]) > 0 and len(h["bfaces"]) > 0


def test_level_minus_zero_is_level_zero_on_the_device():
    for tau in (0.0, 0.05):
        a, b = _host(_gpu(grid("signed_zero"), -0.0, SPACING, ORIGIN, t_clamp=tau)), _host(_gpu(grid("signed_zero"), 0.0, SPACING, ORIGIN, t_clamp=tau))
        assert all(a[f].tobytes() == b[f].tobytes() for f in FIELDS)


@pytest.mark.parametrize("tau", TAUS)
def test_non_finite_values_change_only_their_own_edges(tau):
    """tets, bfaces and the (point, class) of every vertex are functions of the inside pattern alone: the twin's.  The coordinates
    differ from the twin's -- both from the device, NaN compared by bits -- only at vertices whose edge touches a planted point."""
    g, twin, planted = gv.non_finite()
    a, b = _host(_gpu(g, 0.0, SPACING, ORIGIN, t_clamp=tau)), _host(_gpu(twin, 0.0, SPACING, ORIGIN, t_clamp=tau))
    for f in FIELDS[1:]:
        assert a[f].tobytes() == b[f].tobytes(), f
    q, _ = vd.far_point(g.shape, a["vert_point"], a["vert_class"])
    touched = planted[a["vert_point"]] | planted[q]
    differs = (bits(a["verts"]) != bits(b["verts"])).any(1)
    print(f"non_finite, t_clamp {tau}: {int(differs.sum())} vertices differ from the twin's, {int(touched.sum())} touch a planted point, "
          f"{int(np.isnan(a['verts']).sum())} NaN coordinates")
    assert not differs[~touched].any() and differs.sum() >= 30 and np.isfinite(b["verts"]).all()


@pytest.mark.parametrize("name,level", [("quantised", 0.0), ("quantised", 0.25), ("signed_zero", 0.0), ("signed_zero", -0.0)], ids=lambda v: repr(v))
def test_components_against_the_union_find_on_tied_grids(name, level):
    """A value equal to the level is outside: a plane of ties separates solids."""
    from deepsdf_amd.mesh import solid_components
    g = grid(name)
    label, size, rounds = solid_components(torch.from_numpy(g.copy()).cuda(), level)
    rl, rs = tet_numpy.components(g, level)
    wl, _ = tet_numpy.components(g, level, variant="le_inside")
    assert not np.array_equal(rl, wl)                                                     # the input tells v <= level from v < level
    assert np.array_equal(label.cpu().numpy().reshape(-1), rl) and np.array_equal(size.cpu().numpy().reshape(-1), rs)
    print(f"components {name} level {level!r}: {int((rs > 0).sum())} components, {rounds} rounds")
    assert 1 <= rounds <= tet_numpy.component_depth(g, level) + 1


def two_solid_tied_grid():
    """The quantised grid with the whole plane x = 4 set to the level: ties, so outside, and nothing joins the solid on its two
    sides."""
    g = gv.quantised()
    g[4] = 0.0
    return g


def test_keep_largest_on_a_two_solid_tied_grid():
    g = two_solid_tied_grid()
    label, size = tet_numpy.components(g)
    roots = np.nonzero(size > 0)[0]
    assert len(roots) >= 2
    root = int(np.argmax(size))                                                           # the first maximum: the lowest label among the largest
    sides = np.unravel_index(np.nonzero(label >= 0)[0], g.shape)[0]
    assert (sides < 4).any() and (sides > 4).any() and not (sides == 4).any()
    alone = np.where(((label >= 0) & (label != root)).reshape(g.shape), np.float32(1.0), g)       # the other solids removed by hand
    for tau in (0.0, 0.05):
        kept = _gpu(g, 0.0, SPACING, ORIGIN, t_clamp=tau, keep_largest=True)
        h = _same_as_oracle(f"large solid alone, t_clamp {tau}", kept, tet_numpy.tetrahedralize(alone, 0.0, SPACING, ORIGIN, t_clamp=tau))
        ha = _host(_gpu(alone, 0.0, SPACING, ORIGIN, t_clamp=tau))
        assert all(h[f].tobytes() == ha[f].tobytes() for f in FIELDS)
        whole = _gpu(g, 0.0, SPACING, ORIGIN, t_clamp=tau)
        assert whole.n_tets > kept.n_tets > 0


# ---- marching cubes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", LEVELS, ids=lambda v: repr(v))
def test_marching_cubes_bit_for_bit_and_the_mesher_s_axis_vertices(name, level):
    from deepsdf_amd.mesh import marching_cubes
    g = grid(name)
    v, f = marching_cubes(torch.from_numpy(g.copy()).cuda(), level, SPACING, ORIGIN)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    vr, fr = mc_oracle(name, level)
    assert f.dtype == np.int32 and f.shape == fr.shape and np.array_equal(f, fr) and len(f) > 0
    same_floats(f"marching cubes, {name} level {level!r}", v, vr)
    assert is_finite(name) == bool(np.isfinite(vr).all())
    h = _host(_gpu(g, level, SPACING, ORIGIN))
    axis = h["verts"][np.isin(h["vert_class"], [1, 2, 4])]
    assert axis.shape == v.shape and np.array_equal(bits(axis), bits(v))                 # both from the device: NaN by bits too


# ---- the derivatives -----------------------------------------------------------------------------------------------------------------------
def make_valid(sb, rows, degrees, n_cp):
    """The synthetic band with the given rows kept (mask 1) and inside the domain (a base, non-zero weights): an endpoint there
    contributes, so a vertex on it has a zero row only if the clamp holds it."""
    for r in sorted(set(int(x) for x in rows)):
        sb["mask"][r] = 1
        if sb["base"][r] >= 0:
            continue
        sb["base"][r] = 0
        for k in range(degrees[2] + 1):
            for j in range(degrees[1] + 1):
                for i in range(degrees[0] + 1):
                    w = np.float32(0.25 + ((r + i + 2 * j + 3 * k) % 7) / 8)
                    c = i + n_cp[0] * (j + n_cp[1] * k)
                    sb["weights"][r, (k * 4 + j) * 4 + i], sb["B"][r, c], sb["support"][r, c] = w, w, True


def volume_band(name, tau):
    from tests.test_gpu_voldiff import Band
    return Band(grid(name), DEGREES, N_CP, L, tau)


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name", DERIVATIVE_GRIDS)
def test_volume_derivative_against_the_oracles(name, tau):
    """dsdf_vd_jvp / dsdf_vd_vjp against the fp64 contraction at jvp_bound / vjp_bound where a term is non-zero and exact zeros where
    none is; dsdf_vd_dtheta against its stated fp32 sequence bit for bit, with and without the clip."""
    from tests.test_gpu_voldiff import _check_contractions
    B = volume_band(name, tau).upload()
    mv = vd.moves(B.grid, B.vp, B.vc, tau)
    assert set(B.vc[mv].tolist()) == set(range(1, 8))
    rj, rv = _check_contractions(B, f"{name}, tau {tau}")
    assert rj <= 1 and rv <= 1
    normals = np.random.default_rng(5).standard_normal((len(B.vp), 3)).astype(np.float32)
    stretch, scale = (2.0, 1.0, 1.0), B.scale
    for clip in (1.0, 0.0):
        want = vd.dtheta_fp32(B.grid, B.vp, B.vc, B.index, tau, B.sb, scale, normals, stretch, clip, DEGREES, N_CP)
        got = B.dtheta(torch.from_numpy(normals).cuda(), stretch, clip)
        assert np.isfinite(want).all() and np.array_equal(bits(got), bits(want)), (name, tau, clip)
    held = ~mv[B.index]
    assert not bits(want[held]).any() and (tau == 0) == (not held.any())


@pytest.mark.parametrize("tau", gv.TAUS)
def test_every_planted_vertex_moves_or_is_held_by_name(tau):
    """On clamp_edges every planted vertex's row of dsdf_vd_jvp and of dsdf_vd_dtheta is all-zero bits exactly when the oracle's fp32
    rule says the clamp holds it: t == tau and t == 1 - tau move, one ulp outside is held -- all 7 x 6 plants, by name."""
    g, plants = gv.clamp_edges(tau)
    B = volume_band(f"clamp_edges_{tau}", tau)
    assert np.array_equal(B.grid, g)
    _, r0, r1 = vd.band(g.shape, B.vp, B.vc)
    ids = [int(np.nonzero((B.vp == pl["p"]) & (B.vc == pl["cls"]))[0][0]) for pl in plants]
    make_valid(B.sb, np.concatenate([r0[ids], r1[ids]]), DEGREES, N_CP)
    B.upload()
    mv = vd.moves(g, B.vp, B.vc, tau)
    dcp = torch.from_numpy(np.random.default_rng(3).standard_normal((B.ncp, L)).astype(np.float32)).cuda()
    jv = bits(B.jvp(dcp))
    normals = np.random.default_rng(5).standard_normal((len(B.vp), 3)).astype(np.float32)
    dt = bits(B.dtheta(torch.from_numpy(normals).cuda(), (2.0, 1.0, 1.0), 0.0))
    want = vd.dtheta_fp32(g, B.vp, B.vc, B.index, tau, B.sb, B.scale, normals, (2.0, 1.0, 1.0), 0.0, DEGREES, N_CP)
    assert np.array_equal(dt, bits(want))
    at = {int(v): i for i, v in enumerate(B.index)}
    for pl, v in zip(plants, ids):
        name = (tau, pl["cls"], pl["kind"])
        assert bool(mv[v]) == pl["moves"], name
        assert bool(jv[v].any()) == pl["moves"], name
        assert bool(dt[at[v]].any()) == pl["moves"], name
    assert sum(pl["moves"] for pl in plants) == 7 * 4


def fp32_dt(g, vp, vc):
    """dt/ds0, dt/ds1 [V, 2] in msd_dt's own fp32 sequence (level 0), and the fp64 values."""
    F = np.float32
    f = np.ascontiguousarray(g, dtype=F).reshape(-1)
    q, _ = vd.far_point(g.shape, vp, vc)
    s0, s1 = f[vp], f[q]
    with np.errstate(all="ignore"):
        d = s1 - s0
        dd = d * d
        dt32 = np.stack([(F(0) - s1) / dd, -((F(0) - s0) / dd)], 1)
        return dt32, np.stack(mn.dt_factors(s0, s1), 1)


def kind(x):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 3, np.where(np.isposinf(x), 1, np.where(np.isneginf(x), 2, 0)))


def classify(g, vp, vc, mv):
    """(dt32 [V, 2], nonfinite [V], lost [V]) of the moving vertices: dt inf or NaN in msd_dt's fp32 sequence (a subnormal difference
    squares to 0: x / 0); dt lost to an infinite difference (x / inf = 0 where fp64 has a number)."""
    dt32, dt64 = fp32_dt(g, vp, vc)
    nonfinite = mv & ~np.isfinite(dt32).all(1)
    return dt32, nonfinite, mv & ~nonfinite & ((dt32 == 0) & (dt64 != 0)).any(1)


def adjoint_with_infinite_factors(s, dt32, ok, rows, Bm, G, support, which):
    """[ncp, L] fp64: sum over the vertices `which` and their valid endpoints of s[v] * dt32[v, e] * weight * G on the endpoint's
    support -- the adjoint's terms with the fp32 sequence's infinite factors: +-inf, NaN where both signs meet, 0 where none lands."""
    out = np.zeros((Bm.shape[1], G.shape[1]))
    with np.errstate(all="ignore"):
        for e in range(2):
            v = np.nonzero(which & ok[:, e])[0]
            r = rows[v, e]
            f = (np.asarray(s, dtype=np.float64)[v] * dt32[v, e].astype(np.float64))[:, None, None]
            term = np.where(support[r][:, :, None], f * Bm[r][:, :, None] * G[r].astype(np.float64)[:, None, :], 0.0)
            out = out + term.sum(0)
    return out


def check_adjoint_with_abnormal_vertices(tag, got, expect, want, bound):
    """The entries an infinite term lands on have the kind the fp32 sequence gives; every other entry is the normal vertices' sum at
    the counted bound.  (On `magnitudes` the band's supports are seeded per row and the abnormal vertices' supports cover the whole
    control net: every entry is of the first sort, and the bound is held by the run that lists the normal vertices alone.)"""
    hit = kind(expect) != 0
    assert hit.any(), tag
    assert np.array_equal(kind(got)[hit], kind(expect)[hit]), tag
    assert np.isfinite(got[~hit]).all(), tag
    r = mn.ratio(np.where(hit, 0.0, got), np.where(hit, 0.0, want), np.where(hit, 0.0, bound))
    print(f"{tag}: every vertex listed, {int(hit.sum())} of {hit.size} adjoint entries non-finite, the others' worst error / bound {r:.3f}")
    assert r <= 1, tag


@pytest.mark.parametrize("tau", (0.0, 0.05))
def test_volume_derivative_on_magnitudes(tau):
    """The counted bounds are relative-error bounds: they hold while dt, in msd_dt's fp32 sequence, is a finite number that did not
    lose everything.  The other vertices are listed on their own (vert_index takes any subset) and held to the unchanged bounds; with
    every vertex listed their rows keep their bits, a row whose dt is inf or NaN has the same non-finite kind as the fp32 sequence
    gives, a row whose dt is lost is exactly zero, the adjoint's entries are non-finite of that kind exactly where such a vertex's
    support lands and within the bound elsewhere, and dsdf_vd_dtheta is its stated sequence (NaN for NaN, bits else)."""
    from tests.test_gpu_voldiff import _check_contractions
    g, plants = gv.magnitudes()
    B = volume_band("magnitudes", tau)
    _, r0, r1 = vd.band(g.shape, B.vp, B.vc)
    ids = np.array([int(np.nonzero((B.vp == pl["p"]) & (B.vc == pl["cls"]))[0][0]) for pl in plants])
    make_valid(B.sb, np.concatenate([r0[ids], r1[ids]]), DEGREES, N_CP)
    mv = vd.moves(g, B.vp, B.vc, tau)
    dt32, nonfinite, lost = classify(g, B.vp, B.vc, mv)
    normal = ~(nonfinite | lost)
    what = np.array([pl["what"] for pl in plants])
    assert nonfinite[ids[what == "subnormal difference"]].all() and nonfinite.sum() >= 14
    assert (lost | ~mv)[ids[what == "overflowing difference"]].all() and (tau > 0 or lost.sum() >= 14)
    assert normal[ids[what == "subnormal endpoint"]].all()
    listed = np.nonzero(B.vc > 0)[0].astype(np.int32)
    # 1. the normal vertices alone, at the unchanged bounds
    B.index = listed[normal[listed]]
    B.upload()
    _check_contractions(B, f"magnitudes, tau {tau}, {int(nonfinite.sum())} vertices with a non-finite dt and {int(lost.sum())} with a lost dt "
                           f"not listed", keep=normal)
    rng = np.random.default_rng(3)                               # _check_contractions' own inputs
    w = rng.standard_normal((len(B.vp), 3)).astype(np.float32)
    dcp = rng.standard_normal((B.ncp, L)).astype(np.float32)
    jv_normal = B.jvp(torch.from_numpy(dcp).cuda()).cpu().numpy()
    # 2. every vertex listed
    B.index = listed
    B.upload()
    T, ds, n_terms, (ok0, ok1, _, _), Tabs = B.oracle()
    jv = B.jvp(torch.from_numpy(dcp).cuda()).cpu().numpy()
    assert np.array_equal(bits(jv[normal]), bits(jv_normal[normal]))
    assert not jv[lost].any()
    dot = ((B.sb["B"] @ dcp.astype(np.float64)) * B.sb["G"].astype(np.float64)).sum(1)          # per band row
    dot_abs = ((B.sb["B"] @ np.abs(dcp).astype(np.float64)) * np.abs(B.sb["G"]).astype(np.float64)).sum(1)
    v = np.nonzero(nonfinite)[0]
    assert (ok0[v] & ok1[v]).all() and (np.abs(dot[r0[v]]) > 1e-3 * dot_abs[r0[v]]).all() and (np.abs(dot[r1[v]]) > 1e-3 * dot_abs[r1[v]]).all()
    with np.errstate(all="ignore"):
        expect = dt32[v, 0].astype(np.float64) * dot[r0[v]] + dt32[v, 1].astype(np.float64) * dot[r1[v]]
    flagged = vd.directions(B.vc[v])[1] == 1
    assert (kind(expect) != 0).all() and len(set(kind(expect).tolist())) >= 2
    assert np.array_equal(kind(jv[v])[flagged], np.broadcast_to(kind(expect)[:, None], flagged.shape)[flagged])
    assert not bits(jv[v])[~flagged].any()
    gs = (ds * w.astype(np.float64)).sum(1)                      # the vertex's scalar; its sign is safe from cancellation:
    assert (np.abs(gs[v]) > 1e-3 * np.abs(ds * w)[v].sum(1)).all()
    T[~normal], Tabs[~normal] = 0, 0
    expect = adjoint_with_infinite_factors(gs, dt32, np.stack([ok0, ok1], 1), np.stack([r0, r1], 1), B.sb["B"], B.sb["G"], B.sb["support"],
                                           nonfinite)
    got = B.vjp(torch.from_numpy(w).cuda()).cpu().numpy()
    check_adjoint_with_abnormal_vertices(f"vd_vjp on magnitudes, tau {tau}", got, expect, (gs[:, None, None] * T).sum(0),
                                         vd.vjp_bound(n_terms, B.parts()[1], (np.abs(ds * w).sum(1)[:, None, None] * Tabs).sum(0)))
    normals = np.random.default_rng(5).standard_normal((len(B.vp), 3)).astype(np.float32)
    for clip in (1.0, 0.0):
        with np.errstate(all="ignore"):
            want = vd.dtheta_fp32(g, B.vp, B.vc, B.index, tau, B.sb, B.scale, normals, (2.0, 1.0, 1.0), clip, DEGREES, N_CP)
        got = B.dtheta(torch.from_numpy(normals).cuda(), (2.0, 1.0, 1.0), clip).cpu().numpy()
        same_floats(f"dtheta on magnitudes, tau {tau}, clip {clip}", got, want)
    assert not np.isfinite(want).all()


def test_surface_derivative_on_magnitudes():
    """dsdf_msd_jacobian, dsdf_msd_jvp and dsdf_msd_vjp on `magnitudes`, by the scheme above.  The normal vertices as an edge list of
    their own: tests/test_gpu_msdiff_kernels.py's checks at dense_bound, jvp_bound and vjp_bound, unchanged.  Every vertex listed: the
    normal rows keep their bits; a row whose dt is lost is exactly zero; an entry of a row with a non-finite dt has the kind that
    dt * weight * G gives on its endpoints' supports and is +0 off them; the adjoint as in the volume's test."""
    from tests.test_gpu_msdiff_kernels import SCALE, Surface, check_contractions
    g, plants = gv.magnitudes()
    ep, ea = mn.edges(g)
    sb = mn.surface_band(g.shape, ep, ea, DEGREES, N_CP, L)
    rows = sb["band_of"][np.unique([pl[k] for pl in plants for k in ("p", "q")])]
    make_valid(sb, rows[rows >= 0], DEGREES, N_CP)
    S = Surface(g, "deg131_L2", edges=(ep, ea), sb=sb)
    spec = S.spec()
    dt32, nonfinite, lost = classify(g, ep, 1 << ea, np.ones(len(ep), dtype=bool))
    normal = ~(nonfinite | lost)
    print(f"magnitudes: {S.V} surface vertices, {int(nonfinite.sum())} with a non-finite dt, {int(lost.sum())} with a lost dt")
    assert nonfinite.sum() >= 6 and lost.sum() >= 6 and spec["end"][nonfinite].all()
    # 1. the normal vertices alone
    Sn = Surface(g, "deg131_L2", edges=(ep[normal], ea[normal]), sb=sb)
    spec_n = Sn.spec()
    jac_n = Sn.jacobian(0)[0].cpu().numpy()
    # dense_bound is relative to the entry's own terms and assumes that no rounding on the way underflows.  Next to a subnormal grid
    # value dt is 4e-40, or a normal 2e-38 whose products with scale and weight are subnormal: such an entry is a subnormal number,
    # and each of the four roundings on its way (dt, scale * dt, * weight, the fma with G) can lose up to 2^-150, half the smallest
    # subnormal, absolutely -- the standard model fl(x) = x (1 + delta) + eta, |eta| <= 2^-150.  Carried to the entry with scale <= 1
    # and weight <= 1 that is at most 2^-150 (3 |G| + 1) per endpoint.  It is added to the entries below 2^-100 only: with |G| < 8 an
    # entry above that has no intermediate below 2^-103, far from fp32's 2^-126, and keeps dense_bound as it stands.
    small = (spec_n["Jabs"] > 0) & (spec_n["Jabs"] < 2.0 ** -100)
    assert small.sum() >= 100 and SCALE.max() <= 1 and sb["weights"].max() <= 1 and np.abs(sb["G"]).max() < 8
    absG = np.abs(sb["G"]).astype(np.float64)
    eta = 2.0 ** -150 * ((3 * absG[spec_n["row"][:, 0]] + 1) + (3 * absG[spec_n["row"][:, 1]] + 1))             # [V, L]
    rd = mn.ratio(jac_n, spec_n["J"], mn.dense_bound(spec_n["Jabs"]) + np.where(small, eta[:, None, :], 0.0))
    print(f"magnitudes, normal vertices: {int(small.sum())} entries below 2^-100 of {int((spec_n['Jabs'] > 0).sum())}")
    rj, rv, _ = check_contractions(Sn, spec_n, "magnitudes, normal vertices")
    print(f"magnitudes, normal vertices: dense Jacobian worst error / bound {rd:.3f}")
    assert rd <= 1 and rj <= 1 and rv <= 1
    # 2. every vertex listed
    w, dcp = mn.contraction_inputs(S.V, S.ncp, S.L)
    x = torch.from_numpy(dcp).cuda()
    jac, axis = S.jacobian(0)
    jac = jac.cpu().numpy()
    assert np.array_equal(axis.cpu().numpy(), ea) and np.array_equal(bits(jac[normal]), bits(jac_n)) and not jac[lost].any()
    Bm, support = mn.scatter_weights(sb["weights"], sb["base"], mn.base_in_range(sb["base"], DEGREES, N_CP), DEGREES, N_CP)
    G = sb["G"].astype(np.float64)
    v = np.nonzero(nonfinite)[0]
    expect = np.zeros((len(v), S.ncp, S.L))
    with np.errstate(all="ignore"):
        for e in range(2):
            r = spec["row"][v, e]
            expect = expect + np.where(support[r][:, :, None], dt32[v, e].astype(np.float64)[:, None, None] * Bm[r][:, :, None] * G[r][:, None, :], 0.0)
    on = (support[spec["row"][v, 0]] | support[spec["row"][v, 1]])[:, :, None] & np.ones(S.L, dtype=bool)
    assert (kind(expect)[on] != 0).all() and np.array_equal(kind(jac[v]), kind(expect)) and not bits(jac[v])[~on].any()
    jv, jv_n = S.jvp(x).cpu().numpy(), Sn.jvp(x).cpu().numpy()
    assert np.array_equal(bits(jv[normal]), bits(jv_n)) and not jv[lost].any()
    dot = ((Bm @ dcp.astype(np.float64)) * G).sum(1)
    dot_abs = ((Bm @ np.abs(dcp).astype(np.float64)) * np.abs(G)).sum(1)
    r0, r1 = spec["row"][v, 0], spec["row"][v, 1]
    assert (np.abs(dot[r0]) > 1e-3 * dot_abs[r0]).all() and (np.abs(dot[r1]) > 1e-3 * dot_abs[r1]).all()
    with np.errstate(all="ignore"):
        expect = dt32[v, 0].astype(np.float64) * dot[r0] + dt32[v, 1].astype(np.float64) * dot[r1]
    on_axis = np.arange(3)[None, :] == ea[v][:, None]
    assert (kind(expect) != 0).all() and np.array_equal(kind(jv[v])[on_axis], kind(expect)) and not bits(jv[v])[~on_axis].any()
    s = SCALE.astype(np.float64)[ea] * w.astype(np.float64)[np.arange(S.V), ea]
    expect = adjoint_with_infinite_factors(s, dt32, spec["end"], spec["row"], Bm, sb["G"], support, nonfinite)
    kept = dict(spec, J=np.where(normal[:, None, None], spec["J"], 0.0), Jabs=np.where(normal[:, None, None], spec["Jabs"], 0.0))
    c = mn.contractions(kept, w, dcp)
    got = S.vjp(torch.from_numpy(w).cuda()).cpu().numpy()
    check_adjoint_with_abnormal_vertices("msd_vjp on magnitudes", got, expect, c["vjp"][0], mn.vjp_bound(c["n_terms"], S.parts()[1], c["vjp"][1]))


@pytest.mark.parametrize("name", DERIVATIVE_GRIDS)
def test_surface_derivative_against_the_fp64_oracle(name):
    """dsdf_msd_jacobian entry by entry, dsdf_msd_jvp and dsdf_msd_vjp at their counted bounds, exact zeros where no term is non-zero."""
    from tests.test_gpu_msdiff_kernels import Surface, check_contractions
    S = Surface(grid(name), "deg131_L2")
    spec = S.spec()
    mn.check_edges_reproduce(grid(name))
    jac, axis = S.jacobian(0)
    assert np.array_equal(axis.cpu().numpy(), S.ea)
    bound = mn.dense_bound(spec["Jabs"])
    assert not bits(jac)[bound == 0].any()
    rd = mn.ratio(jac.cpu().numpy(), spec["J"], bound)
    rj, rv, _ = check_contractions(S, spec, name)
    print(f"{name}: dense Jacobian worst error / bound {rd:.3f}")
    assert rj <= 1 and rv <= 1
    assert rd <= 1 and (bound > 0).sum() > 1000


@pytest.mark.parametrize("case", list(mn.CASES))
def test_jvp_has_the_bits_of_the_volume_kernel_on_axis_edges_of_quantised(case):
    from tests.test_gpu_msdiff_kernels import Surface
    S = Surface(grid("quantised"), case)
    spec = S.spec()
    _, dcp = mn.contraction_inputs(S.V, S.ncp, S.L)
    x = torch.from_numpy(dcp).cuda()
    sj, vj = S.jvp(x), S.volume_jvp(x)
    assert np.array_equal(bits(sj), bits(vj)) and bits(sj).any()
    f = grid("quantised").reshape(-1)
    stride = np.array([gv.SHAPE[1] * gv.SHAPE[2], gv.SHAPE[2], 1])
    assert ((f[S.ep] == 0) | (f[S.ep + stride[S.ea]] == 0)).sum() >= 40                  # edges with an end on the level
    # a vertex whose only valid endpoint is tied with the level has a zero factor there (dt/ds = -(level - s) / d^2): a zero row too
    nonzero_term = (spec["Jabs"] > 0).any((1, 2))
    assert (bits(sj).any(1) <= spec["end"].any(1)).all() and (bits(sj).any(1) >= nonzero_term).all()


def test_surface_jvp_has_the_volume_kernel_s_bits_on_magnitudes():
    """The same endpoint code in both kernels: where dt is inf or NaN too (NaN for NaN, bits elsewhere)."""
    from tests.test_gpu_msdiff_kernels import Surface
    S = Surface(grid("magnitudes"), "deg131_L2")
    _, dcp = mn.contraction_inputs(S.V, S.ncp, S.L)
    x = torch.from_numpy(dcp).cuda()
    sj, vj = S.jvp(x).cpu().numpy(), S.volume_jvp(x).cpu().numpy()
    same_floats("msd_jvp against vd_jvp on magnitudes", sj, vj)
    assert not np.isfinite(sj).all() and np.isfinite(sj).any(1).sum() > 500


# ---- the real thing ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remove_orphans", [True, False])
def test_the_capped_structure_holds_these_values_and_meshes_as_the_oracle(tmp_path, remove_orphans):
    from analysis.geometry import STRETCH, DeepSDFMesh
    from deepsdf_amd.mesh import default_cap_border_dict
    from tests.test_gpu_microstructure import _tiny_experiment
    exp = _tiny_experiment(str(tmp_path))
    options = dict(experiment_directory=exp, checkpoint="latest", degrees=[1, 1, 1], refinement=1, cap_border_dict=default_cap_border_dict(),
                   N_base_reconstruction=6, tiling=[2, 1, 1], remove_orphans=remove_orphans)
    dm = DeepSDFMesh(options)
    dm.generate_surface_mesh(np.tile(dm.latent[0], (27, 1)))
    g = dm.diff.grid.cpu().numpy()
    assert g.dtype == np.float32 and np.isfinite(g).all()
    # the premise of this file: the caps leave -0.0f, and values equal to the level off the border
    n_neg_zero, n_tied_inner = int((bits(g) == 0x80000000).sum()), int((g[1:-1, 1:-1, 1:-1] == 0).sum())
    print(f"remove_orphans={remove_orphans}: grid {g.shape}, {n_neg_zero} values -0.0f, {int((g == 0).sum())} equal to the level, "
          f"{n_tied_inner} of them off the border")
    assert n_neg_zero >= 1 and n_tied_inner >= 1
    if remove_orphans:                                           # keep_largest, restated: every other solid's points set to the level
        label, size = tet_numpy.components(g)
        root = int(np.argmax(size))
        g = np.where(((label >= 0) & (label != root)).reshape(g.shape), np.float32(0.0), g)
    vs = dm.diff.voxel_size
    for tau in (0.0, 0.05):
        vm = dm.generate_volume_mesh(t_clamp=tau)
        r = tet_numpy.tetrahedralize(g, 0.0, vs, (0, 0, 0), t_clamp=tau)
        assert np.array_equal(vm.tets.cpu().numpy(), r.tets) and np.array_equal(vm.bfaces.cpu().numpy(), r.bfaces)
        assert np.array_equal(vm.bface_kind.cpu().numpy(), r.bface_kind)
        assert np.array_equal(vm.vert_point.cpu().numpy(), r.vert_point) and np.array_equal(vm.vert_class.cpu().numpy(), r.vert_class)
        want = (r.verts.astype(np.float64) - np.asarray(vs, dtype=np.float64)) / 2 * np.asarray(STRETCH, dtype=np.float64)
        got = vm.verts.cpu().numpy()
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
        assert len(r.tets) > 0
