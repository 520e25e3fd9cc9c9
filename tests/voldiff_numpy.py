"""Numpy fp64 reference for the derivative of a volume mesh's vertices (tests/tet_numpy.py's mesh) with respect to the grid values
and the spline's control points, written from the specification in include/dsdf.h (dsdf_vd_*) and DESIGN 4.22.

Vertex (p, c): d = (c & 1, (c >> 1) & 1, (c >> 2) & 1), q = p + d . stride, t = (level - s0) / (s1 - s0); class 0 does not move; with
t_clamp = tau > 0 the vertex moves iff tau <= t <= 1 - tau in the mesher's own arithmetic.  Every flagged coordinate moves by t:

    d verts[v, b] / d cp[k, l] = d[b] * scale[b] * T[v, k, l],   T = sum_e dt/ds_e * m_e * G_e[l] * B_k(xo_e).

Four WRONG variants (`variant=`) exist so that the tests can show their inputs tell them apart from the specification:
    "lowest_coord"   only the lowest flagged coordinate moves
    "q_lowest_axis"  q taken along the lowest flagged axis only
    "no_clamp"       the clamp ignored
    "reversed_bits"  class bits mapped to axes in reverse (bit 0 -> z)
and a fifth for tests/test_grid_values_cpu.py, which no continuous random grid shows:
    "strict_clamp"   the vertex moves iff tau < t < 1 - tau: a t exactly on a clamp boundary held
Also: the seeded synthetic band of the kernel-level tests, the bounds counted from the kernels, and the fp32 restatement of
dsdf_vd_dtheta's stated sequence."""
import numpy as np

from tests import msdiff_numpy, tet_numpy

VARIANTS = ("lowest_coord", "q_lowest_axis", "no_clamp", "reversed_bits")
TIE_VARIANTS = ("strict_clamp",)
U = 2.0 ** -24


def directions(vert_class, variant=None):
    """(dq [V, 3]: the steps to the far endpoint, dm [V, 3]: the coordinates that move), 0 / 1."""
    c = np.asarray(vert_class, dtype=np.int64)
    d = np.stack([c & 1, (c >> 1) & 1, (c >> 2) & 1], 1)
    if variant == "reversed_bits":
        d = d[:, ::-1].copy()
    lowest = np.zeros_like(d)
    has = d.any(1)
    lowest[np.nonzero(has)[0], np.argmax(d[has], 1)] = 1
    dq = lowest if variant == "q_lowest_axis" else d
    dm = lowest if variant == "lowest_coord" else d
    return dq, dm


def strides(dims):
    return np.array([dims[1] * dims[2], dims[2], 1], dtype=np.int64)


def far_point(grid_shape, vert_point, vert_class, variant=None):
    """(q [V], ok [V]): the far endpoint; a wrong variant's q can leave the grid: then q = p and ok is False."""
    p = np.asarray(vert_point, dtype=np.int64)
    q = p + directions(vert_class, variant)[0] @ strides(grid_shape)
    ok = q < int(np.prod(grid_shape))
    return np.where(ok, q, p), ok


def moves(grid, vert_point, vert_class, t_clamp, level=0.0, variant=None, dtype=np.float32):
    """[V] bool: class >= 1 and the clamp leaves t unchanged (t in the mesher's sequence in `dtype`): tau <= t <= 1 - tau, both ends
    included; a NaN t fails the comparisons and is held."""
    g = np.ascontiguousarray(grid, dtype=dtype).reshape(-1)
    c = np.asarray(vert_class)
    p = np.asarray(vert_point, dtype=np.int64)
    q, ok = far_point(np.shape(grid), p, c, variant)
    mv = (c > 0) & ok
    if t_clamp > 0 and variant != "no_clamp":
        tau = dtype(t_clamp)
        t = tet_numpy.edge_t(g[p], g[q], level, 0.0, dtype)
        with np.errstate(invalid="ignore"):
            mv = mv & ((t > tau) & (t < dtype(1) - tau) if variant == "strict_clamp" else (t >= tau) & (t <= dtype(1) - tau))
    return mv


def grid_factors(grid, vert_point, vert_class, t_clamp, level=0.0, variant=None, dtype=np.float32):
    """(q [V], dm [V, 3], dt0 [V], dt1 [V] fp64, zero where the vertex does not move, mv [V])."""
    g64 = np.asarray(grid, dtype=np.float64).reshape(-1)
    p = np.asarray(vert_point, dtype=np.int64)
    _, dm = directions(vert_class, variant)
    q, _ = far_point(np.shape(grid), p, vert_class, variant)
    mv = moves(grid, vert_point, vert_class, t_clamp, level, variant, dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        d0, d1 = msdiff_numpy.dt_factors(g64[p], g64[q], level)
    return q, dm * mv[:, None], np.where(mv, d0, 0.0), np.where(mv, d1, 0.0), mv


def band(grid_shape, vert_point, vert_class):
    """(band [nb] sorted unique endpoints of the class >= 1 vertices, row0 [V], row1 [V]; rows of class-0 vertices: their point's
    searchsorted position, not to be used)."""
    p = np.asarray(vert_point, dtype=np.int64)
    c = np.asarray(vert_class)
    q = p + directions(c)[0] @ strides(grid_shape)
    on = c > 0
    b = np.unique(np.concatenate([p[on], q[on]]))
    return b, np.minimum(np.searchsorted(b, p), len(b) - 1), np.minimum(np.searchsorted(b, q), len(b) - 1)


def tangent(grid, vert_point, vert_class, t_clamp, band_idx, G_band, B_band, m_band, level=0.0, variant=None, swap_dt=False):
    """(T [V, ncp, L] fp64, dm [V, 3], ends: (valid0 [V], valid1 [V], row0, row1), Tabs: the sum of the two endpoints' magnitudes,
    for the bounds).  An endpoint outside band_idx contributes nothing (a wrong variant's q can leave the band).  swap_dt: WRONG on
    purpose, each endpoint takes the other's dt factor (tests/msdiff_numpy.py's "swapped_dt")."""
    q, dm, d0, d1, mv = grid_factors(grid, vert_point, vert_class, t_clamp, level, variant)
    if swap_dt:
        d0, d1 = d1, d0
    p = np.asarray(vert_point, dtype=np.int64)
    G, B, m = (np.asarray(x, dtype=np.float64) for x in (G_band, B_band, m_band))
    T = np.zeros((len(p), B.shape[1], G.shape[1]))
    Tabs = np.zeros_like(T)
    ends = []
    for pts, dt in ((p, d0), (q, d1)):
        r = np.minimum(np.searchsorted(band_idx, pts), len(band_idx) - 1)
        ok = mv & (band_idx[r] == pts) & (m[r] != 0)
        term = (np.where(ok, dt, 0.0))[:, None, None] * B[r][:, :, None] * G[r][:, None, :]
        T += term
        Tabs += np.abs(term)
        ends.append((ok, r))
    return T, dm, (ends[0][0], ends[1][0], ends[0][1], ends[1][1]), Tabs


def dvert_dgrid(grid, vert_point, vert_class, t_clamp, spacing=(1, 1, 1), level=0.0, variant=None, dtype=np.float64):
    """(D0 [V, 3], D1 [V, 3], q, mv): d verts[v] / d grid[p], d verts[v] / d grid[q] of tet_numpy.vertices."""
    q, dm, d0, d1, mv = grid_factors(grid, vert_point, vert_class, t_clamp, level, variant, dtype)
    sp = np.asarray(spacing, dtype=np.float64)
    return dm * sp * d0[:, None], dm * sp * d1[:, None], q, mv


def boundary_volume_gradient(verts, bfaces):
    """gV [V, 3] = (1 / 3) sum A_f n_f over the vertex's boundary triangles: d (enclosed volume) / d vertex of a closed mesh."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(bfaces, dtype=np.int64)
    an = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]) / 6.0
    g = np.zeros_like(v)
    for k in range(3):
        np.add.at(g, f[:, k], an)
    return g


# ---- the kernel-level tests' band ----------------------------------------------------------------------------------------------
def synthetic_band(grid_shape, vert_point, vert_class, degrees, n_cp, L, seed):
    """A seeded random band on the endpoints of the class >= 1 vertices: dict of band [nb] int64, band_of [npts] int32, G [nb, L]
    fp32, weights [nb, 64] fp32 (slot (k * 4 + j) * 4 + i), base [nb] int32 (-1 on about one row in nine), mask [nb] uint8 (0 on
    about one row in seven), and for the oracle B [nb, ncp] fp64 (the weights scattered) and support [nb, ncp] bool."""
    rng = np.random.default_rng(seed)
    b, _, _ = band(grid_shape, vert_point, vert_class)
    nb, ncp = len(b), int(np.prod(n_cp))
    G = rng.standard_normal((nb, L)).astype(np.float32)
    first = np.stack([rng.integers(0, n_cp[a] - degrees[a], nb) for a in range(3)], 1)
    base = (first[:, 0] + n_cp[0] * (first[:, 1] + n_cp[1] * first[:, 2])).astype(np.int32)
    base[rng.random(nb) < 1 / 9] = -1
    mask = (rng.random(nb) >= 1 / 7).astype(np.uint8)
    weights = np.zeros((nb, 64), dtype=np.float32)
    B = np.zeros((nb, ncp))
    support = np.zeros((nb, ncp), dtype=bool)
    rows = np.nonzero(base >= 0)[0]
    for k in range(degrees[2] + 1):
        for j in range(degrees[1] + 1):
            for i in range(degrees[0] + 1):
                w = rng.uniform(0.1, 1.0, nb).astype(np.float32) * (base >= 0)
                weights[:, (k * 4 + j) * 4 + i] = w
                c = base[rows] + i + n_cp[0] * (j + n_cp[1] * k)
                B[rows, c] = w[rows]
                support[rows, c] = True
    band_of = np.full(int(np.prod(grid_shape)), -1, dtype=np.int32)
    band_of[b] = np.arange(nb, dtype=np.int32)
    return dict(band=b, band_of=band_of, G=G, weights=weights, base=base, mask=mask, B=B, support=support)


# ---- bounds counted from the kernels (csrc/voldiff.hpp) --------------------------------------------------------------------------
# A term is one product scale * dt * weight * G * x.  Its fp32 factors: dt carries 5 roundings (s1 - s0, its square, the numerator,
# the quotient: 1 + 2 + 1 + 1), scale * dt one, weight * G one; one more covers the second-order terms.
def jvp_bound(degrees, L, mag):
    """vd_jvp_kernel: a lane's fma chain over ceil(n / 64) of the endpoint's n = prod(deg + 1) * L products, six levels of the
    xor-shuffle tree, two fmas that join the endpoints; the factors' 8 roundings."""
    n = int(np.prod([d + 1 for d in degrees])) * L
    return (-(-n // 64) + 6 + 2 + 8) * U * mag


def vjp_bound(n_terms, parts, mag):
    """vd_vjp_part_kernel + msd_vjp_sum_kernel: entry (k, l) receives n_terms[k] fmas, one per (vertex, endpoint) whose support
    holds k, in list order, and `parts` additions of the second stage.  The factors: the 8 above, and the scalar
    gs = sum_b scale[b] * grad[b] (a product and at most two further additions per coordinate: 3) -- gs * dt takes the place of
    scale * dt: 11."""
    return (np.asarray(n_terms, dtype=np.float64)[:, None] + parts + 11) * U * mag


# ---- dsdf_vd_dtheta's stated sequence, in fp32 --------------------------------------------------------------------------------
def dtheta_fp32(grid, vert_point, vert_class, vert_index, t_clamp, sb, scale, normals, stretch, clip, degrees, n_cp, level=0.0):
    """out [len(vert_index), 3, ncp * L] fp32, every operation rounded once, in the order include/dsdf.h states.  Takes in-range
    list entries, classes and points only (the robustness cases are compared against zero rows)."""
    F = np.float32
    g = np.ascontiguousarray(grid, dtype=F).reshape(-1)
    idx = np.asarray(vert_index, dtype=np.int64)
    p, c = np.asarray(vert_point, dtype=np.int64)[idx], np.asarray(vert_class)[idx]
    dq, _ = directions(c)
    q = p + dq @ strides(np.shape(grid))
    s0, s1 = g[p], g[q]
    mv = moves(grid, p, c, t_clamp, level)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = s1 - s0
        dd = d * d
        dts = ((F(level) - s1) / dd, -(F(level) - s0) / dd)
    ncp, L = int(np.prod(n_cp)), sb["G"].shape[1]
    W = np.zeros((len(sb["band"]), ncp), dtype=F)                 # the weight of control point k at a band row, 0 off its support
    W[sb["support"]] = sb["B"][sb["support"]].astype(F)
    T = np.zeros((len(idx), ncp, L), dtype=F)
    for pts, dt in ((p, dts[0]), (q, dts[1])):
        r = sb["band_of"][pts]
        ok = mv & (r >= 0) & (sb["mask"][r] != 0) & (sb["base"][r] >= 0)
        f = (dt[:, None] * W[r]).astype(F)                                        # dt * weight
        term = (f[:, :, None] * sb["G"][r][:, None, :]).astype(F)                 # * G
        on = (ok[:, None] & sb["support"][r])[:, :, None]
        T = np.where(on, (T + term).astype(F), T)
    T = T.reshape(len(idx), ncp * L)
    n = np.asarray(normals, dtype=F)[idx]
    ss = (np.asarray(stretch, dtype=F) * np.asarray(scale, dtype=F)).astype(F)
    nj = np.zeros_like(T)
    for b in range(3):
        j = np.where((dq[:, b] == 1)[:, None], (ss[b] * T).astype(F), F(0))
        if clip > 0:
            j = np.where(np.abs(j) > F(clip), F(0), j)
        nj = (nj + (n[:, b:b + 1] * j).astype(F)).astype(F)
    nn = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]).astype(F) + n[:, 2] * n[:, 2]).astype(F)
    zero = (nn == 0) | ~mv
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (nj / nn[:, None]).astype(F)
    out = np.stack([(n[:, b:b + 1] * s).astype(F) for b in range(3)], 1)
    out[zero] = 0
    return out


def vertices_from_edges(grid, vert_point, vert_class, t_clamp, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """The mesher's vertices from (vert_point, vert_class) alone, fp32, every operation rounded on its own (tet_numpy.vertices'
    sequence): [V, 3]."""
    F = np.float32
    g = np.ascontiguousarray(grid, dtype=F)
    p, c = np.asarray(vert_point, dtype=np.int64), np.asarray(vert_class, dtype=np.int64)
    d, _ = directions(c)
    f = g.reshape(-1)
    t = tet_numpy.edge_t(f[p], f[p + d @ strides(g.shape)], level, t_clamp, F)         # the select-form clamp: a NaN t stays NaN
    t = np.where(c == 0, F(0), t).astype(F)
    idx = np.stack(np.unravel_index(p, g.shape), 1).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        pos = np.where(d == 1, idx + t[:, None], idx).astype(F)
        return (np.asarray(origin, F) + (pos * np.asarray(spacing, F)).astype(F)).astype(F)
