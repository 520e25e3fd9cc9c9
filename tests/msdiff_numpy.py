"""Numpy fp64 reference for the derivative of a microstructure mesh with respect to the spline's control points, written from the
specification in include/dsdf.h (dsdf_msd_*) and DESIGN 4.12: the grid edges of marching cubes' vertices, the band of grid points
that carry one, the dense tensor-product basis, and the Jacobian

    J[v, c, l] = (voxel_size[a] / 2) * sum_k dt/ds_k * m_k * G_k[l] * B_c(xo_k).

The tests compare the HIP kernels (csrc/msdiff.hpp) against it and pin the formula itself against end-to-end autograd.  For the
kernel-level tests (tests/test_gpu_msdiff_kernels.py): the entry rule, the specification on a synthetic band with entries out of
range (surface_spec), five wrong variants, and the bounds counted from the kernels."""
import numpy as np
import torch

from oracle import deepsdf_oracle as orc
from tests import mc_numpy, ms_numpy


def edges(sdf, level=0.0):
    """(edge_point [V] int64, edge_axis [V] int64) of every vertex of mc_numpy.marching_cubes(sdf, level), in its order."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    nx, ny, nz = sdf.shape
    inside = sdf < np.float32(level)
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    sel = np.nonzero(cross.reshape(-1))[0]
    return sel // 3, sel % 3


def vertices_from_edges(sdf, edge_point, edge_axis, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """origin + (p + t e_a) * spacing in fp32 with every operation rounded on its own: marching cubes' vertices from their edges."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    F = np.float32
    stride = np.array([sdf.shape[1] * sdf.shape[2], sdf.shape[2], 1], dtype=np.int64)
    f = sdf.reshape(-1)
    p, a = np.asarray(edge_point, dtype=np.int64), np.asarray(edge_axis, dtype=np.int64)
    v0, v1 = f[p], f[p + stride[a]]
    t = (F(level) - v0) / (v1 - v0)
    pos = np.stack(np.unravel_index(p, sdf.shape), 1).astype(F)
    pos[np.arange(len(p)), a] += t
    return (np.asarray(origin, F) + pos * np.asarray(spacing, F)).astype(F)


def band(edge_point, edge_axis, dims):
    """(band [nb] sorted unique grid indices of {p, p + e_a}, row0 [V], row1 [V]: the band rows of the two endpoints)."""
    stride = np.array([dims[1] * dims[2], dims[2], 1], dtype=np.int64)
    p = np.asarray(edge_point, dtype=np.int64)
    q = p + stride[np.asarray(edge_axis, dtype=np.int64)]
    b = np.unique(np.concatenate([p, q]))
    return b, np.searchsorted(b, p), np.searchsorted(b, q)


def dense_basis(degrees, knots, pts):
    """B [n, ncp] fp64: the tensor-product basis weight of every control point (first parametric axis fastest) at pts [n, 3]."""
    Bs = [ms_numpy.basis_matrix(int(degrees[a]), knots[a], np.asarray(pts)[:, a]) for a in range(3)]
    return np.einsum("pk,pj,pi->pkji", Bs[2], Bs[1], Bs[0]).reshape(len(pts), -1)


def dt_factors(s0, s1, level=0.0):
    """(dt/ds0, dt/ds1) of t = (level - s0) / (s1 - s0), fp64."""
    s0, s1 = np.asarray(s0, dtype=np.float64), np.asarray(s1, dtype=np.float64)
    d2 = (s1 - s0) ** 2
    return (level - s1) / d2, -(level - s0) / d2


def jacobian(capped, edge_point, edge_axis, voxel_size, G_band, B_band, m_band, level=0.0):
    """(J [V, ncp, L] fp64, axis [V]).  capped: the grid [nx, ny, nz] whose edges carry the vertices; G_band [nb, L], B_band
    [nb, ncp] and m_band [nb] at the rows of band(edge_point, edge_axis, capped.shape)."""
    capped = np.asarray(capped, dtype=np.float64)
    _, r0, r1 = band(edge_point, edge_axis, capped.shape)
    stride = np.array([capped.shape[1] * capped.shape[2], capped.shape[2], 1], dtype=np.int64)
    a = np.asarray(edge_axis, dtype=np.int64)
    p = np.asarray(edge_point, dtype=np.int64)
    f = capped.reshape(-1)
    d0, d1 = dt_factors(f[p], f[p + stride[a]], level)
    G, B, m = (np.asarray(x, dtype=np.float64) for x in (G_band, B_band, m_band))
    scale = np.asarray(voxel_size, dtype=np.float64)[a] / 2
    J = ((scale * d0 * m[r0])[:, None, None] * B[r0][:, :, None] * G[r0][:, None, :] +
         (scale * d1 * m[r1])[:, None, None] * B[r1][:, :, None] * G[r1][:, None, :])
    return J, a


# ---- kernel level: the entry rule, the specification on a synthetic band, wrong variants, bounds (tests/test_gpu_msdiff_kernels.py) ----
# Five WRONG variants (`variant=`) exist so that the tests can show their inputs tell them apart from the specification:
#     "swapped_dt"              each endpoint takes the other's dt factor
#     "slot_transposed"         weight slot (k * 4 + j) * 4 + i read as (i * 4 + j) * 4 + k
#     "mask_ignored"            a masked endpoint contributes
#     "base_minus_one_as_zero"  a row outside the domain (base = -1) read as if its support began at control point 0
#     "wrapped_edge_counts"     an edge is refused only when p + stride[a] leaves the grid: one at the last index of axis 1 or 2
#                               wraps into the next row and contributes
VARIANTS = ("swapped_dt", "slot_transposed", "mask_ignored", "base_minus_one_as_zero", "wrapped_edge_counts")
U = 2.0 ** -24
SPACING = (0.5, 0.25, 0.75)                       # scale = SPACING / 2, exact in fp32
# (degrees, n_cp, L), one per form of msd_dense_kernel: dword stores with several vertices per workgroup; float4 stores at the cap
# MSD_DENSE_VERTS; dword stores, an odd L, one vertex per workgroup; float4 stores, one vertex per workgroup, two adjoint tiles
CASES = {"deg131_L2": ((1, 3, 1), (3, 5, 2), 2), "deg111_L4": ((1, 1, 1), (2, 2, 2), 4),
         "deg313_L27": ((3, 1, 3), (4, 4, 5), 27), "deg313_L128": ((3, 1, 3), (4, 4, 5), 128)}


def seeded_grid(shape=(6, 5, 4)):
    return np.random.default_rng(1).uniform(-1, 1, shape).astype(np.float32)


def base_in_range(base, degrees, n_cp):
    """[nb] bool: 0 <= base < ncp and first[x] + deg[x] < n_cp[x] on every axis."""
    b = np.asarray(base, dtype=np.int64)
    ok = (b >= 0) & (b < int(np.prod(n_cp)))
    first = np.stack([b % n_cp[0], (b // n_cp[0]) % n_cp[1], b // (n_cp[0] * n_cp[1])], 1)
    return ok & (first + np.asarray(degrees) < np.asarray(n_cp)).all(1)


def entry_rule(dims, edge_point, edge_axis, band_of, mask, base, degrees, n_cp, variant=None):
    """Which vertices and which of their endpoints contribute (include/dsdf.h, dsdf_msd_*):
    vertex (p, a): 0 <= a <= 2, 0 <= p, and the index of p along a is below dims[a] - 1 (the volume's rule);
    endpoint g in {p, p + stride[a]}: band_of[g] in 0 .. nb - 1, mask != 0, 0 <= base < ncp, first[x] + deg[x] < n_cp[x] on every axis.
    -> (vertex [V] bool, end [V, 2] bool, row [V, 2] int64: the band rows, 0 where there is none)."""
    dims = tuple(int(d) for d in dims)
    npts, nb = int(np.prod(dims)), len(mask)
    stride = np.array([dims[1] * dims[2], dims[2], 1], dtype=np.int64)
    p, a = np.asarray(edge_point, dtype=np.int64), np.asarray(edge_axis, dtype=np.int64)
    vert = (a >= 0) & (a <= 2) & (p >= 0) & (p < npts)
    ps, as_ = np.where(vert, p, 0), np.where(vert, a, 0)
    q = ps + stride[as_]
    if variant == "wrapped_edge_counts":
        vert &= q < npts
    else:
        idx = np.stack(np.unravel_index(ps, dims), 1)[np.arange(len(p)), as_]
        vert &= idx < np.asarray(dims)[as_] - 1
    q = np.where(vert, q, 0)
    m = np.ones(nb, dtype=bool) if variant == "mask_ignored" else np.asarray(mask) != 0
    b = np.asarray(base, dtype=np.int64)
    row_ok = m & base_in_range(np.where(b == -1, 0, b) if variant == "base_minus_one_as_zero" else b, degrees, n_cp)
    r = np.asarray(band_of, dtype=np.int64)[np.stack([ps, q], 1)]
    in_band = (r >= 0) & (r < nb)
    r = np.where(in_band, r, 0)
    return vert, vert[:, None] & in_band & row_ok[r], r


def scatter_weights(weights, base, rows_ok, degrees, n_cp, transposed=False):
    """(B [nb, ncp] fp64: the weight of every control point at the rows with rows_ok, 0 elsewhere; support [nb, ncp] bool)."""
    nb, ncp = len(base), int(np.prod(n_cp))
    B, support = np.zeros((nb, ncp)), np.zeros((nb, ncp), dtype=bool)
    rows = np.nonzero(rows_ok)[0]
    for k in range(degrees[2] + 1):
        for j in range(degrees[1] + 1):
            for i in range(degrees[0] + 1):
                c = np.asarray(base, dtype=np.int64)[rows] + i + n_cp[0] * (j + n_cp[1] * k)
                B[rows, c] = weights[rows, (i * 4 + j) * 4 + k if transposed else (k * 4 + j) * 4 + i]
                support[rows, c] = True
    return B, support


def surface_band(grid_shape, edge_point, edge_axis, degrees, n_cp, L, seed=7):
    """voldiff_numpy.synthetic_band on the edges' endpoints (classes 1 << axis).  The rows outside the domain (base = -1), whose
    weights it leaves zero, get seeded weights as large as the others': a kernel that read them would show."""
    from tests import voldiff_numpy as vd
    sb = vd.synthetic_band(grid_shape, edge_point, 1 << np.asarray(edge_axis, dtype=np.int64), degrees, n_cp, L, seed)
    out = np.nonzero(sb["base"] < 0)[0]
    fill = np.random.default_rng(seed + 1000).uniform(0.1, 1.0, (len(out), 64)).astype(np.float32)
    for s in range(64):
        if (s & 3) <= degrees[0] and ((s >> 2) & 3) <= degrees[1] and (s >> 4) <= degrees[2]:
            sb["weights"][out, s] = fill[:, s]
    return sb


def surface_spec(grid, edge_point, edge_axis, sb, degrees, n_cp, scale, level=0.0, variant=None):
    """The specification of dsdf_msd_* on a band of surface_band's form, entries out of range included, in fp64 of the fp32 inputs:
    dict of J [V, ncp, L], Jabs (sum of the two endpoints' magnitudes, for the bounds), axis [V] (what the kernels report), vert [V],
    end [V, 2], row [V, 2], support [nb, ncp], n_terms [ncp] (the adjoint's additions per control point).
    The entry rule turns the input into a healthy one (a refused vertex: class 0; a refused endpoint: its row masked -- every
    endpoint condition is a property of the grid point), and voldiff_numpy.tangent assembles it: J = scale[a] * T."""
    from tests import voldiff_numpy as vd
    band, band_of, nb = sb["band"], np.asarray(sb["band_of"], dtype=np.int64), len(sb["band"])
    vert, end, row = entry_rule(grid.shape, edge_point, edge_axis, band_of, sb["mask"], sb["base"], degrees, n_cp, variant)
    at = band_of[band]
    off = np.delete(band_of, band)
    assert (((at < 0) | (at >= nb)) | (at == np.arange(nb))).all() and ((off < 0) | (off >= nb)).all()   # a row or none, never another
    base = np.asarray(sb["base"], dtype=np.int64)
    if variant == "base_minus_one_as_zero":
        base = np.where(base == -1, 0, base)
    fits = base_in_range(base, degrees, n_cp)
    m = np.ones(nb, dtype=bool) if variant == "mask_ignored" else np.asarray(sb["mask"]) != 0
    B, support = scatter_weights(sb["weights"], base, fits, degrees, n_cp, transposed=variant == "slot_transposed")
    a = np.asarray(edge_axis, dtype=np.int64)
    axis = np.where((a >= 0) & (a <= 2), a, 0)
    p = np.where(vert, np.asarray(edge_point, dtype=np.int64), 0)
    T, _, (ok0, ok1, r0, r1), Tabs = vd.tangent(grid, p, np.where(vert, 1 << axis, 0), 0.0, band, sb["G"], B, m & fits & (at == np.arange(nb)),
                                                level, swap_dt=variant == "swapped_dt")
    assert np.array_equal(np.stack([ok0, ok1], 1), end)                       # the rule above and the assembly name the same endpoints
    assert np.array_equal(np.stack([r0, r1], 1)[end], row[end])
    s = np.asarray(scale, dtype=np.float32).astype(np.float64)[axis][:, None, None]
    T *= s
    Tabs *= np.abs(s)
    n_terms = (ok0[:, None] & support[r0]).sum(0) + (ok1[:, None] & support[r1]).sum(0)
    return dict(J=T, Jabs=Tabs, axis=axis, vert=vert, end=end, row=row, support=support, n_terms=n_terms)


# Bounds counted from csrc/msdiff.hpp, in units U = 2^-24 of sum |terms|; a term is one product scale * dt * weight * G (* x).  dt
# carries 5 roundings (msd_dt: s1 - s0 one, its square two -- the difference enters twice -- the numerator one, the quotient one).
DENSE_ROUNDINGS = 10


def dense_bound(mag):
    """msd_dense_store: dt 5, coef = rn(scale * dt) 1, f = rn(coef * w) 1, val = fma(f, G, val) once per endpoint -- the first
    endpoint's term passes through both: 2 -- and one for the second-order terms: 10."""
    return DENSE_ROUNDINGS * U * mag


def jvp_bound(degrees, L, mag):
    """msd_jvp_kernel has vd_jvp_kernel's shape: a lane's fma chain over ceil(n / 64) of the endpoint's n = prod(deg + 1) * L
    products rn(w * G), six levels of the xor-shuffle tree, tot = fma(coef, acc, tot) once per endpoint (2), and the factors' 8
    roundings (dt 5, scale * dt 1, w * G 1, second order 1): voldiff_numpy.jvp_bound as it stands."""
    from tests import voldiff_numpy as vd
    return vd.jvp_bound(degrees, L, mag)


def vjp_bound(n_terms, parts, mag):
    """msd_vjp_part + msd_vjp_sum_kernel: entry (k, l) receives n_terms[k] fmas acc = fma(f, rn(w * G), acc), one per (vertex,
    endpoint) whose support holds k, and `parts` additions of the second stage.  The factors: dt 5, scale * dt 1, f = rn(g * coef) 1,
    w * G 1, second order 1: 9."""
    return (np.asarray(n_terms, dtype=np.float64)[:, None] + parts + 9) * U * mag


def contraction_inputs(V, ncp, L, seed=3):
    """(w [V, 3], dcp [ncp, L]) fp32, seeded: the cotangent and the tangent the tests contract with."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((V, 3)).astype(np.float32), rng.standard_normal((ncp, L)).astype(np.float32)


def contractions(spec, w, dcp, first=None):
    """The fp64 contractions of the first `first` vertices (all by default): dict of jvp (want [V, 3], mag [V, 3]) -- zero off the
    reported axis -- vjp (want [ncp, L], mag) and n_terms [ncp] of those vertices."""
    n = len(spec["axis"]) if first is None else first
    J, Jabs, a = spec["J"][:n], spec["Jabs"][:n], spec["axis"][:n]
    x = dcp.astype(np.float64)
    want_j, mag_j = np.zeros((n, 3)), np.zeros((n, 3))
    want_j[np.arange(n), a] = np.einsum("vkl,kl->v", J, x)
    mag_j[np.arange(n), a] = np.einsum("vkl,kl->v", Jabs, np.abs(x))
    g = w.astype(np.float64)[np.arange(n), a]
    end, row, support = spec["end"][:n], spec["row"][:n], spec["support"]
    n_terms = sum((end[:, e, None] & support[row[:, e]]).sum(0) for e in range(2))
    return dict(jvp=(want_j, mag_j), vjp=(np.einsum("v,vkl->kl", g, J), np.einsum("v,vkl->kl", np.abs(g), Jabs)), n_terms=n_terms)


def ratio(got, want, bound):
    """Worst |got - want| / bound over the entries with a bound; where the bound is zero `got` must be zero (asserted)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == bound.shape
    assert not got[bound == 0].any()
    on = bound > 0
    return float((np.abs(got - want)[on] / bound[on]).max()) if on.any() else 0.0


def invalid_entries(grid, edge_point, edge_axis, sb, degrees, n_cp):
    """The healthy input with entries out of range written over it: (edge_point, edge_axis, sb, touched [V] bool, zero [V] bool).
    Vertex level (each vertex must get exact zeros: `zero`): edge_axis -1 and 3; edge_point -1 and npts + 5; an edge at the last
    index of axis 0 (its far endpoint leaves the grid), of axis 1 and of axis 2 (it wraps into the next row), the last two between
    two band rows that are kept, inside the domain and unchanged below, so that the wrapped edge would contribute if it counted.
    Band level: band_of -1, nb, nb + 7; base -2, ncp; a base whose support overruns axis 0.  touched: the vertices written over
    and those with an endpoint at a changed band row; every other vertex must keep its bits."""
    dims = grid.shape
    npts, nb, ncp = grid.size, len(sb["band"]), int(np.prod(n_cp))
    stride = np.array([dims[1] * dims[2], dims[2], 1], dtype=np.int64)
    ep, ea = np.array(edge_point, dtype=np.int64), np.array(edge_axis, dtype=np.int64)
    sb = {k: np.array(v) for k, v in sb.items()}
    good = (sb["mask"] != 0) & base_in_range(sb["base"], degrees, n_cp)
    good_pt = np.zeros(npts, dtype=bool)
    good_pt[sb["band"][good]] = True
    idx = np.stack(np.unravel_index(np.arange(npts), dims), 1)
    V = len(ep)
    ids = [int(i) for i in np.linspace(2, V - 3, 7)]                          # seven vertices across the list: more than one workgroup
    ea[ids[0]], ea[ids[1]] = -1, 3
    ep[ids[2]], ep[ids[3]] = -1, npts + 5
    wrapped = []
    for a, v in zip(range(3), ids[4:7]):
        last = np.nonzero((idx[:, a] == dims[a] - 1) & good_pt & (np.arange(npts) + stride[a] < npts if a else True))[0]
        if a:
            last = last[good_pt[last + stride[a]]]
            wrapped += [int(last[0]), int(last[0] + stride[a])]
        ep[v], ea[v] = last[0], a
    zero = np.zeros(V, dtype=bool)
    zero[ids[:7]] = True
    free = np.nonzero(good & ~np.isin(sb["band"], wrapped))[0]                # rows to damage: healthy ones the wrapped edges do not use
    rows = free[np.linspace(1, len(free) - 2, 6).astype(int)]
    assert len(set(rows.tolist())) == 6
    for r, val in zip(rows[:3], (-1, nb, nb + 7)):
        sb["band_of"][sb["band"][r]] = val
    sb["base"][rows[3]], sb["base"][rows[4]] = -2, ncp
    sb["base"][rows[5]] = n_cp[0] - degrees[0]                                # first = (n_cp[0] - deg[0], 0, 0): one too far on axis 0
    hit = np.zeros(npts, dtype=bool)
    hit[sb["band"][rows]] = True
    p0, a0 = np.asarray(edge_point, dtype=np.int64), np.asarray(edge_axis, dtype=np.int64)
    touched = zero | hit[p0] | hit[p0 + stride[a0]]
    return ep, ea, sb, touched, zero


def check_edges_reproduce(sdf, level=0.0):
    """The edge list is mc_numpy.marching_cubes' own: its vertices recomputed from the edges, bit for bit."""
    p, a = edges(sdf, level)
    v, _ = mc_numpy.marching_cubes(sdf, level)
    assert np.array_equal(vertices_from_edges(sdf, p, a, level).view(np.uint32), v.view(np.uint32))
    return p, a


def clamped(p, inner):
    return [-1.0] * (p + 1) + list(inner) + [1.0] * (p + 1)


# non-uniform, a repeated interior knot each, every value exact in fp32 (the knot vectors of tests/test_gpu_microstructure.py)
KNOTS = {1: clamped(1, [-0.5, 0.25, 0.25, 0.625]), 2: clamped(2, [-0.375, 0.125, 0.125]), 3: clamped(3, [-0.25, 0.25, 0.25, 0.75])}
LINEAR_KNOTS = [[-1.0, -1.0, 1.0, 1.0]] * 3


class Fp64Structure:
    """An fp64 torch restatement of create_mesh_microstructure's forward up to the capped grid, differentiable in the control points:
    cp -> ms_numpy.basis_matrix -> oracle decoder_forward -> caps (torch.maximum / minimum in dict order, then the six planes).
    The coordinates are ms_numpy.grid_axes' fp32 values promoted to double.  The output bias is shifted once so that the given
    quantile (the median by default) of the decoder's values inside the domain is zero: the level set crosses the structure, and a
    small quantile leaves a small surface (few band points: the way to a seed whose every ReLU margin is large in a wide net); `params` are fp32 values held in double."""

    def __init__(self, L, net_kw, seed, degrees, knots, tiling, N, caps, cp_amp, quantile=0.5):
        self.L, self.degrees, self.knots, self.tiling, self.N, self.caps = L, tuple(degrees), knots, list(tiling), list(N), caps
        self.net = orc.make_net(L, **net_kw)
        self.params = {k: v.double() for k, v in orc.init_params(self.net, 100 + seed).items()}
        self.ncp = int(np.prod([len(U) - p - 1 for p, U in zip(degrees, knots)]))
        self.cp = np.random.default_rng(seed).uniform(-cp_amp, cp_amp, size=(self.ncp, L)).astype(np.float32)
        axes = ms_numpy.grid_axes(N, tiling)
        self.dims = [len(a[0]) for a in axes]
        self.xo = ms_numpy.grid_points(axes, 0).astype(np.float64)
        self.folded = torch.from_numpy(ms_numpy.grid_points(axes, 1).astype(np.float64))
        self.inside = ms_numpy.grid_inside(axes)
        self.B = dense_basis(degrees, knots, self.xo) * self.inside[:, None]         # outside rows: a constant zero latent
        self._Bt = torch.from_numpy(self.B)
        self._xs = [torch.from_numpy(a[0].astype(np.float64)).reshape(s) for a, s in zip(axes, [(-1, 1, 1), (1, -1, 1), (1, 1, -1)])]
        self.vs = [2.0 / (n + 2 - 1 - 2) for n in N]
        with torch.no_grad():
            raw = self.decode(self.rows(torch.from_numpy(self.cp).double()))[0].reshape(-1)
            last = f"lin{self.net.n_lin - 1}.bias"
            shifted = self.params[last] - torch.atanh(raw[torch.from_numpy(self.inside)].quantile(quantile))
            self.params[last] = shifted.float().double()                             # every parameter stays an fp32 value

    def rows(self, cp_t):
        return torch.cat([self._Bt @ cp_t, self.folded], 1)

    def decode(self, rows):
        """(raw [dims], Saved with min_abs_pre) of decoder input rows [n, L + 3]."""
        y, sv = orc.decoder_forward(self.net, self.params, rows, training=False, track_margin=True)
        return y.reshape(self.dims), sv

    def cap(self, raw):
        """(capped, [every plane value a cap compares against, each [dims]])."""
        v, planes = raw, []
        for loc, d in self.caps.items():
            dim, m = ms_numpy.LOCATION[loc]
            border = (self._xs[dim] - m * (1 - d["measure"])) * -m
            planes.append((-border if d["cap"] == -1 else border).expand(self.dims))
            v = torch.maximum(v, -border) if d["cap"] == -1 else torch.minimum(v, border)
        for dim in range(3):
            for m in (-1, 1):
                plane = -((self._xs[dim] - m) * -m)
                planes.append(plane.expand(self.dims))
                v = torch.maximum(v, plane)
        return v, planes

    def conditions(self, raw, sv, planes, band_idx):
        """(smallest |raw - cap plane value|, smallest ReLU margin) over the band: the function is smooth where both are positive."""
        r = raw.detach().reshape(-1)[band_idx]
        gap = min(float((r - p.reshape(-1)[band_idx]).abs().min()) for p in planes)
        return gap, float(sv.min_abs_pre.detach()[band_idx].min())
