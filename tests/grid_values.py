"""The grid values the package really meshes, as inputs for the grid-to-mesh chain; host only, numpy only.

Every kernel-level test of marching cubes, the tetrahedral mesher and the two mesh derivatives used a continuous random grid: no value
equals the level, no two neighbours are equal, nothing is a zero of either sign, no t lands on a clamp boundary.  The caps
(ms_caps_kernel), their plateaus and keep_largest write exactly such values.  Each grid here is the 9 x 8 x 7 uniform grid of
tests/test_gpu_tetmesh.py (504 points: two workgroups of TET_BLOCK, no axis equal to another) with one family of values imposed, and
comes with the minimum counts of what it must contain (CONTENTS; `measure` counts them on the oracle, tests/test_grid_values_cpu.py
asserts them).  Nothing is thinned or skipped at run time: a builder that cannot plant what it promises raises."""
import numpy as np

from tests import tet_numpy

F = np.float32
SHAPE = (9, 8, 7)
NPTS = int(np.prod(SHAPE))
STRIDE = np.array([SHAPE[1] * SHAPE[2], SHAPE[2], 1], dtype=np.int64)
TAUS = (0.05, 0.25)
# the six planted values of t around a clamp's two boundaries and whether vd_vertex's rule tau <= t <= hi lets the vertex move
KINDS = (("below tau", False), ("tau", True), ("above tau", True), ("below hi", True), ("hi", True), ("above hi", False))


def uniform():
    """The continuous random grid every earlier kernel-level test used: on it no wrong variant of the tie rules shows."""
    return np.random.default_rng(7).uniform(-1, 1, SHAPE).astype(F)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _step(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)


def _free_edges(used, seed):
    """take(class) -> (p, q = p + d(class)): the next edge, in a seeded order of the grid's points, that lies in the grid and whose two
    points no earlier plant uses."""
    order = np.random.default_rng(seed).permutation(NPTS)
    idx = np.stack(np.unravel_index(np.arange(NPTS), SHAPE), 1)

    def take(c):
        d = _step(c)
        for p in order:
            q = p + d @ STRIDE
            if used[p] or ((idx[p] + d) >= np.asarray(SHAPE)).any() or used[q]:
                continue
            used[p] = used[q] = True
            return int(p), int(q)
        raise AssertionError(f"no free edge of class {c} left")
    return take


# ---- quantised ------------------------------------------------------------------------------------------------------------------
def quantised():
    """round(g * 4) / 4: ties with the levels 0, 0.25 and -0.5, plateaus of equal neighbours, t exactly 0 and exactly 1 (and zeros of
    both signs: numpy rounds -0.1 to -0.0)."""
    return (np.round(uniform() * 4) / 4).astype(F)


# ---- signed zeros ---------------------------------------------------------------------------------------------------------------
def signed_zero():
    """What ms_caps_kernel's last line (lo > v ? lo : v with lo = -0.0 on a border plane) leaves: every inside value of the outer plane
    x = 0 and of 24 interior points becomes -0.0f -- equal to the level, sign bit set, so now outside -- and 8 more points +0.0f."""
    g = uniform()
    g[0][g[0] < 0] = F(-0.0)
    rng = np.random.default_rng(11)
    interior = np.zeros(SHAPE, dtype=bool)
    interior[1:-1, 1:-1, 1:-1] = True
    neg = np.nonzero((interior & (g < 0)).reshape(-1))[0]
    pick = rng.choice(neg, 24, replace=False)
    g.reshape(-1)[pick] = F(-0.0)
    rest = np.setdiff1d(np.nonzero(interior.reshape(-1))[0], pick)
    g.reshape(-1)[rng.choice(rest, 8, replace=False)] = F(0.0)
    return g


# ---- t on the clamp's boundaries --------------------------------------------------------------------------------------------------
def clamp_targets(tau):
    """The six fp32 values of t, in KINDS' order: tau, hi = 1 - tau as the kernels form it, and their neighbouring floats."""
    t, hi = F(tau), F(1) - F(tau)
    inf = F(np.inf)
    return [np.nextafter(t, -inf), t, np.nextafter(t, inf), np.nextafter(hi, -inf), hi, np.nextafter(hi, inf)]


def _pair_with_t(a, target, p_inside):
    """(v0, v1) on different sides of level 0 whose t, in the mesher's own fp32 sequence (0 - v0) / (v1 - v0), has exactly `target`'s
    bits: the inside value is -a (or a neighbouring float), the outside value is searched among the floats next to the real solution."""
    a0 = float(a)
    for j in range(256):                                        # a over one binade: every alignment of a against v1 - v0 occurs
        a = F(a0 * 2.0 ** (-j / 256))
        b0 = F(float(a) * (1 - float(target)) / float(target)) if p_inside else F(float(a) * float(target) / (1 - float(target)))
        cand = (_bits(b0).astype(np.int64) + np.arange(-512, 513)).astype(np.uint32).view(F)
        v0, v1 = (np.full_like(cand, -a), cand) if p_inside else (cand, np.full_like(cand, -a))
        hit = np.nonzero(_bits(tet_numpy.edge_t(v0, v1, 0.0)) == _bits(target))[0]
        if len(hit):
            return F(v0[hit[0]]), F(v1[hit[0]])
    raise AssertionError(f"no fp32 pair gives t = {target!r}")


def clamp_edges(tau):
    """(grid, plants): for each of the seven edge classes six planted pairs across level 0 whose t is exactly tau, one ulp below, one
    ulp above, and the same three around fp32(1 - tau); the inside end alternates between p and q.  plants: dicts of tau, cls, kind,
    moves (KINDS), p, q, t."""
    assert tau in TAUS
    g = uniform()
    f = g.reshape(-1)
    take = _free_edges(np.zeros(NPTS, dtype=bool), 100 + int(round(tau * 100)))
    plants = []
    for c in range(1, 8):
        for k, ((kind, mv), target) in enumerate(zip(KINDS, clamp_targets(tau))):
            p, q = take(c)
            p_inside = (c + k) % 2 == 0
            v0, v1 = _pair_with_t(0.25 + 0.5 * abs(float(f[p])), target, p_inside)
            f[p], f[q] = v0, v1
            plants.append(dict(tau=tau, cls=c, kind=kind, moves=mv, p=p, q=q, t=target))
    for pl in plants:                                           # planted values are not overwritten by a later plant
        assert _bits(tet_numpy.edge_t(f[pl["p"]], f[pl["q"]], 0.0)) == _bits(pl["t"]), pl
    assert len(plants) == 7 * 6 and all(sum(pl["cls"] == c for pl in plants) == 6 for c in range(1, 8))
    return g, plants


# ---- magnitudes -------------------------------------------------------------------------------------------------------------------
MAGNITUDE_PAIRS = (("subnormal difference", -1e-40, 1e-40, 0.5), ("subnormal difference", 1e-40, -1e-40, 0.5),
                   ("overflowing difference", -3e38, 3e38, 0.0), ("overflowing difference", 3e38, -3e38, 0.0),
                   ("subnormal endpoint", -1e-40, 0.5, None), ("subnormal endpoint", -0.5, 1e-40, 1.0),
                   ("subnormal endpoint", 1e-40, -0.5, None), ("subnormal endpoint", 0.5, -1e-40, 1.0))


def magnitudes():
    """(grid, plants): on every edge class, crossing pairs whose difference is subnormal (t = 0.5 in IEEE arithmetic), whose
    difference overflows (t = 0: finite / inf) and with one subnormal endpoint (t subnormal, or exactly 1).  plants: dicts of what,
    cls, p, q, t (the IEEE fp32 value)."""
    g = uniform()
    f = g.reshape(-1)
    take = _free_edges(np.zeros(NPTS, dtype=bool), 200)
    plants = []
    for c in range(1, 8):
        for what, v0, v1, t in MAGNITUDE_PAIRS:
            p, q = take(c)
            f[p], f[q] = F(v0), F(v1)
            got = tet_numpy.edge_t(f[p], f[q], 0.0)
            assert t is None or got == F(t), (what, v0, v1, got)
            plants.append(dict(what=what, cls=c, p=p, q=q, t=F(got)))
    return g, plants


# ---- non-finite values ------------------------------------------------------------------------------------------------------------
NON_FINITE_POINTS = (((2, 2, 2), np.nan), ((4, 5, 3), np.inf), ((6, 2, 4), -np.inf),
                     ((3, 4, 2), -np.inf), ((4, 4, 2), np.inf),          # a class-1 edge from -inf to +inf
                     ((6, 5, 2), -np.inf), ((7, 6, 3), np.inf))          # a class-7 edge from -inf to +inf


def non_finite():
    """(grid, twin, planted [npts] bool): a NaN point, a +inf point, a -inf point and two edges from -inf to +inf (an axis edge and a
    body diagonal), all interior, so that all 14 Kuhn neighbours of each exist; twin: the same grid with each replaced by +1 or -1
    of the same side of the level (NaN and +inf are outside, -inf is inside)."""
    g = uniform()
    twin = g.copy()
    planted = np.zeros(SHAPE, dtype=bool)
    for at, v in NON_FINITE_POINTS:
        assert all(1 <= at[a] <= SHAPE[a] - 2 for a in range(3))
        g[at], twin[at], planted[at] = F(v), F(-1.0 if v == -np.inf else 1.0), True
    return g, twin, planted.reshape(-1)


# ---- what each grid must contain ------------------------------------------------------------------------------------------------------
def measure(grid, level=0.0):
    """Counts on the oracle: points tied with the level, zeros by sign bit, crossing edges by their unclamped fp32 t."""
    g = np.ascontiguousarray(grid, dtype=F)
    _, _, vp, vc = tet_numpy.vertices(g, level)
    f = g.reshape(-1)
    e = vc > 0
    p = vp[e]
    q = p + np.stack([vc[e] & 1, (vc[e] >> 1) & 1, (vc[e] >> 2) & 1], 1) @ STRIDE
    t = tet_numpy.edge_t(f[p], f[q], level)
    with np.errstate(invalid="ignore", over="ignore"):
        d = f[q] - f[p]
        tiny = np.finfo(F).tiny
        return dict(ties=int((g == F(level)).sum()), neg_zero=int((_bits(g) == 0x80000000).sum()), pos_zero=int((_bits(g) == 0).sum()),
                    equal_neighbours=int(sum((np.diff(g, axis=a) == 0).sum() for a in range(3))),
                    t0=int((t == 0).sum()), t_neg_zero=int((_bits(t) == 0x80000000).sum()), t1=int((t == 1).sum()),
                    t_nan=int(np.isnan(t).sum()), t_subnormal=int(((t != 0) & (np.abs(t) < tiny)).sum()),
                    subnormal_difference=int(((d != 0) & (np.abs(d) < tiny)).sum()), infinite_difference=int(np.isinf(d).sum()),
                    classes=sorted(set(vc[e].tolist())))


# minimum counts, asserted by tests/test_grid_values_cpu.py on `measure` (and, for zero_volume, on the oracle mesh).  A list, not a
# dict keyed by (grid, level): 0.0 == -0.0 and they hash alike, so the two signed_zero entries would be one.
CONTENTS = [
    ("quantised", 0.0, dict(ties=64, t0=147, t1=140, equal_neighbours=100, zero_volume=430)),
    ("quantised", 0.25, dict(ties=70, t0=100, t1=100)),
    ("quantised", -0.5, dict(ties=57, t0=40, t1=40)),
    ("signed_zero", 0.0, dict(neg_zero=40, pos_zero=8, ties=48, t_neg_zero=40, t1=40)),
    ("signed_zero", -0.0, dict(neg_zero=40, pos_zero=8, ties=48, t0=40, t_neg_zero=40, t1=40)),
    ("magnitudes", 0.0, dict(subnormal_difference=14, infinite_difference=14, t_subnormal=14, t0=14, t1=14)),
    ("non_finite", 0.0, dict(t_nan=30, infinite_difference=40)),
]

# what the two test files share: the output arrays of a mesh, a spacing and an origin that are not dyadic on any axis (those of
# tests/test_gpu_tetmesh.py), and the grids by name
FIELDS = ("verts", "tets", "bfaces", "bface_kind", "vert_point", "vert_class")
SPACING, ORIGIN = (0.3, 0.7, 1.1), (-0.9, 0.1, 0.35)
GRIDS = {"quantised": quantised, "signed_zero": signed_zero, "clamp_edges_0.05": lambda: clamp_edges(0.05)[0],
         "clamp_edges_0.25": lambda: clamp_edges(0.25)[0], "magnitudes": lambda: magnitudes()[0],
         "non_finite": lambda: non_finite()[0], "non_finite_twin": lambda: non_finite()[1]}
