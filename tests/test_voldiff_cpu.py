"""CPU (no GPU needed): the fp64 oracle of the volume mesh derivative (tests/voldiff_numpy.py) against central differences of
tests/tet_numpy.py's mesher, the boundary form of the volume's gradient against central differences of the elements' total volume,
and the four wrong variants of the oracle against the bounds the GPU tests hold the kernels to."""
import math

import numpy as np
import pytest

from tests import tet_numpy, voldiff_numpy as vd

GRID = np.random.default_rng(1).uniform(-1, 1, (6, 5, 4)).astype(np.float32)
SPACING = (0.5, 0.25, 0.75)
COUNTS = [58, 51, 44, 35, 48, 38, 31, 34]


def _mesh(tau, dtype=np.float32):
    return tet_numpy.vertices(GRID, 0.0, SPACING, (0, 0, 0), tau, dtype)


def test_the_grid_has_every_class_moving_and_clamped():
    _, _, vp, vc = _mesh(0.0)
    assert len(vp) == 339 and np.bincount(vc, minlength=8).tolist() == COUNTS
    moving = vc > 0
    assert int(moving.sum()) == 281 and int(np.isin(vc, (3, 5, 6, 7)).sum()) == 138
    for tau, share, least_clamped, least_kept in ((0.25, 29.5, 9, 20), (0.1, 10.7, 1, 0)):
        mv = vd.moves(GRID, vp, vc, tau)
        clamped = moving & ~mv
        print(f"tau {tau}: {int(clamped.sum())} of {int(moving.sum())} moving vertices clamped ({100 * clamped.sum() / moving.sum():.1f} %), "
              f"per class clamped {np.bincount(vc[clamped], minlength=8)[1:].tolist()} kept {np.bincount(vc[mv], minlength=8)[1:].tolist()}")
        assert round(100 * clamped.sum() / moving.sum(), 1) == share
        assert np.bincount(vc[clamped], minlength=8)[1:].min() >= least_clamped
        assert np.bincount(vc[mv], minlength=8)[1:].min() >= least_kept
    assert vd.moves(GRID, vp, vc, 0.0).sum() == 281                                  # tau = 0 zeroes nothing


@pytest.mark.parametrize("tau", [0.0, 0.25])
def test_vertex_derivative_equals_central_differences(tau):
    """d verts / d grid value, fp64, step h = 1e-6 |s1 - s0| per vertex: truncation about 1e-12 and rounding about 2e-10 of the
    derivative, against a bound of 1e-8 of the vertex's largest entry."""
    g64 = GRID.astype(np.float64)
    _, _, vp, vc = _mesh(tau, np.float64)
    D0, D1, q, mv = vd.dvert_dgrid(g64, vp, vc, tau, SPACING)
    flat = g64.reshape(-1)
    moving = np.nonzero(vc > 0)[0]
    worst, skipped = 0.0, 0
    for v in moving:
        s0, s1 = flat[vp[v]], flat[q[v]]
        h = 1e-6 * abs(s1 - s0)
        t = -s0 / (s1 - s0)
        # dt/ds is at most 1 / |s1 - s0|: a step of h moves t by at most 1e-6
        if tau > 0 and min(abs(t - tau), abs(t - (1 - tau))) <= 2e-6:
            skipped += 1
            continue
        for at, want in ((vp[v], D0[v]), (q[v], D1[v])):
            hi, lo = g64.copy(), g64.copy()
            hi.reshape(-1)[at] += h
            lo.reshape(-1)[at] -= h
            cd = (tet_numpy.vertices(hi, 0.0, SPACING, (0, 0, 0), tau, np.float64)[0][v] -
                  tet_numpy.vertices(lo, 0.0, SPACING, (0, 0, 0), tau, np.float64)[0][v]) / (2 * h)
            top = max(np.abs(D0[v]).max(), np.abs(D1[v]).max())
            if not mv[v]:
                assert not cd.any() and not want.any(), v                             # held by the clamp: exactly zero
            else:
                assert top > 0
                worst = max(worst, float(np.abs(cd - want).max() / top))
    print(f"tau {tau}: worst |central difference - oracle| / largest entry {worst:.3e} (bound 1e-8), {skipped} vertices at a clamp edge left out")
    assert skipped <= 0.02 * len(moving)
    assert worst <= 1e-8
    assert not D0[vc == 0].any() and not D1[vc == 0].any()


def _total_volume(g, tau):
    m = tet_numpy.tetrahedralize(g, 0.0, SPACING, (0, 0, 0), tau, np.float64)
    return math.fsum(tet_numpy.volumes(m.verts, m.tets).tolist()), m


@pytest.mark.parametrize("tau", [0.0, 0.25])
def test_boundary_gradient_is_the_derivative_of_the_total_volume(tau):
    """gV = (1 / 3) sum A_f n_f is the exact derivative of a closed mesh's volume with respect to a vertex, so for a band point g:
    d (sum of element volumes) / d s_g = sum_v gV_v . d vert_v / d s_g.  Fourth-order central differences
    (V(-2h) - 8 V(-h) + 8 V(h) - V(2h)) / 12 h with h = f d, f = 1e-3 and d the smallest |s1 - s0| among the point's crossing edges.
    Truncation: t is a rational function of s_g with pole distance d, so the relative error is about f^4 = 1e-12.  Rounding: about
    a thousand element volumes of at most 0.1, each from three products of fp64 coordinate differences, leave about 3e-16 in the
    compensated sum; over 12 h / 18 with d >= 0.01 and terms of 0.05 or more that is about 1e-9 at worst, 1e-11 typically.  (The
    second-order difference cannot reach the bound on this grid: its best step leaves 1e-8 of both kinds.)
    Bound: 1e-8 sum |terms|."""
    g64 = GRID.astype(np.float64)
    _, m = _total_volume(g64, tau)
    vp, vc = m.vert_point, m.vert_class
    D0, D1, q, mv = vd.dvert_dgrid(g64, vp, vc, tau, SPACING)
    gV = vd.boundary_volume_gradient(m.verts, m.bfaces)
    flat = g64.reshape(-1)
    band, _, _ = vd.band(GRID.shape, vp, vc)
    on = vc > 0
    t = np.where(on, -flat[vp] / np.where(on, flat[q] - flat[vp], 1.0), 0.5)
    edge = on & (tau > 0) & (np.minimum(np.abs(t - tau), np.abs(t - (1 - tau))) <= 4e-3)
    done, worst = 0, 0.0
    for g in band:
        mine = on & ((vp == g) | (q == g))
        if edge[mine].any():
            continue
        h = 1e-3 * np.abs(flat[q] - flat[vp])[mine].min()
        if abs(flat[g]) <= 4 * h:                                                     # the perturbation must change no sign
            continue
        terms = np.concatenate([(gV * D0)[on & (vp == g)].reshape(-1), (gV * D1)[on & (q == g)].reshape(-1)])
        vol = {}
        for k in (-2, -1, 1, 2):
            moved = g64.copy()
            moved.reshape(-1)[g] += k * h
            vol[k] = _total_volume(moved, tau)[0]
        cd = (vol[-2] - 8 * vol[-1] + 8 * vol[1] - vol[2]) / (12 * h)
        mag = float(np.abs(terms).sum())
        if mag == 0:              # every vertex around it is held by the clamp, or moves where gV has no component: rounding alone
            assert abs(cd) <= 1e-10
            continue
        worst = max(worst, abs(cd - float(terms.sum())) / mag)
        done += 1
        if done == 20:
            break
    print(f"tau {tau}: {done} band points, worst |central difference - sum gV . dvert| / sum |terms| {worst:.3e} (bound 1e-8)")
    assert done == 20
    assert worst <= 1e-8


def _contractions(sb, vp, vc, tau, degrees, L, variant=None):
    T, dm, (ok0, ok1, r0, r1), Tabs = vd.tangent(GRID, vp, vc, tau, sb["band"], sb["G"], sb["B"], sb["mask"], variant=variant)
    scale = np.array(SPACING) / 2
    rng = np.random.default_rng(3)
    w, dcp = rng.standard_normal((len(vp), 3)), rng.standard_normal(T.shape[1:])
    jvp = ((dm * scale)[:, :, None] * (T * dcp[None]).reshape(len(vp), 1, -1)).sum(2)
    jmag = ((dm * scale)[:, :, None] * (Tabs * np.abs(dcp)[None]).reshape(len(vp), 1, -1)).sum(2)
    gs = (dm * scale * w).sum(1)
    vt = gs[:, None, None] * T
    n_terms = (ok0[:, None] & sb["support"][r0]).sum(0) + (ok1[:, None] & sb["support"][r1]).sum(0)
    return jvp, jmag, vt.sum(0), (np.abs(dm * scale * w).sum(1)[:, None, None] * Tabs).sum(0), n_terms


def test_wrong_variants_miss_the_gpu_bounds():
    """Each wrong variant of the oracle differs from the specification, on the GPU test's grid and synthetic band at tau = 0.25, by
    at least 1e3 times the bound the kernels are held to (tests/test_gpu_voldiff.py uses the same bounds)."""
    tau, degrees, n_cp, L = 0.25, (1, 3, 1), (3, 5, 2), 2
    _, _, vp, vc = _mesh(tau)
    sb = vd.synthetic_band(GRID.shape, vp, vc, degrees, n_cp, L, 7)
    jvp, jmag, vjp, vmag, n_terms = _contractions(sb, vp, vc, tau, degrees, L)
    jb, vb = vd.jvp_bound(degrees, L, jmag), vd.vjp_bound(n_terms, 1, vmag)
    assert (jb[jmag > 0] > 0).all() and (vb[vmag > 0] > 0).all() and (jmag > 0).sum() > 200
    for variant in vd.VARIANTS:
        j2, _, v2, _, _ = _contractions(sb, vp, vc, tau, degrees, L, variant)
        # where the specification's terms are all zero the kernels must give an exact zero: any difference there misses by infinity
        with np.errstate(divide="ignore", invalid="ignore"):
            fj = float(np.nanmax(np.abs(j2 - jvp) / jb))
            fv = float(np.nanmax(np.abs(v2 - vjp) / vb))
        print(f"variant {variant}: misses the jvp bound by a factor {fj:.3g}, the vjp bound by {fv:.3g}")
        assert fj >= 1e3 and fv >= 1e3, variant
