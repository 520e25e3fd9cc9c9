"""Reference tetrahedral mesher in numpy, written from the specification in include/dsdf.h (dsdf_tet_*): the solid {sdf < level}
of a regular grid cut into the six Kuhn tetrahedra of every cell, each clipped against the level set.  The tests compare the HIP
kernels (csrc/tetmesh.hpp) against it array for array and check mesh properties on it.  fp32 with every operation rounded on its
own (dtype=np.float64 gives the same mesh in fp64, for the volume identities).  Also: a union-find `components`, a vectorised
`counts`, and the mesh invariants the CPU and the GPU tests share."""
import itertools
from types import SimpleNamespace

import numpy as np

PERMS = list(itertools.permutations(range(3)))


def perm_sign(p):
    return -1 if sum(p[a] > p[b] for a in range(len(p)) for b in range(a + 1, len(p))) % 2 else 1


SIGNS = [perm_sign(p) for p in PERMS]
# corner k of Kuhn tetrahedron pi as a bit mask of unit steps (bit a: one step along axis a)
CORNERS = [(0, 1 << p[0], (1 << p[0]) | (1 << p[1]), 7) for p in PERMS]
N_ELEMS = (0, 1, 3, 3, 1)          # elements of a Kuhn tetrahedron by its number of inside corners
N_CUT = (0, 1, 2, 1, 0)            # cut-face triangles
N_PLANE = (0, 1, 2, 1)             # triangles of the inside part of a face by its number of inside corners


def _dir(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.int64)


# WRONG variants (`variant=`), for tests/test_grid_values_cpu.py: each is a mistake a kernel could make that no continuous random grid
# shows, and exists so that a test can prove that its inputs tell it from the specification.
#     "le_inside"     inside = sdf <= level: a value equal to the level counted inside
#     "fminmax_clamp" the clamp as fmin(fmax(t, tau), 1 - tau): a NaN t becomes tau
#     "abs_t"         t taken as |t|: the sign of a zero t (and of a NaN) lost
VARIANTS = ("le_inside", "fminmax_clamp", "abs_t")


def is_inside(sdf, level=0.0, variant=None):
    """The specification's comparison v < level in the grid's own type: a value equal to the level (of either sign of zero), NaN and
    +inf are outside, -inf is inside."""
    sdf = np.asarray(sdf)
    with np.errstate(invalid="ignore"):
        return sdf <= sdf.dtype.type(level) if variant == "le_inside" else sdf < sdf.dtype.type(level)


def clamp_t(t, t_clamp, dtype=np.float32, variant=None):
    """The specification's clamp, compare-and-select: t < tau ? tau : t, then t > hi ? hi : t, hi = 1 - tau in `dtype`.  A NaN t
    fails both comparisons and stays NaN under every tau; tau = 0 does not touch t."""
    if not t_clamp > 0:
        return t
    tau = dtype(t_clamp)
    hi = dtype(1) - tau
    with np.errstate(invalid="ignore"):
        if variant == "fminmax_clamp":
            return np.fmin(np.fmax(t, tau), hi)
        t = np.where(t < tau, tau, t)
        return np.where(t > hi, hi, t)


def edge_t(v0, v1, level, t_clamp=0.0, dtype=np.float32, variant=None):
    """t of an edge from value v0 to value v1 in the mesher's sequence: (level - v0) / (v1 - v0), every operation rounded on its own
    in `dtype`, then the clamp."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        t = (dtype(level) - v0) / (v1 - v0)
    if variant == "abs_t":
        t = np.abs(t)
    return clamp_t(t, t_clamp, dtype, variant)


def records(sdf, level=0.0, variant=None):
    """(inside [nx, ny, nz] bool, rec [npts, 8] bool: slot 0 = inside, slot c = edge (p, class c) crosses)."""
    sdf = np.asarray(sdf)
    inside = is_inside(sdf, level, variant)
    nx, ny, nz = sdf.shape
    rec = np.zeros((nx, ny, nz, 8), dtype=bool)
    rec[..., 0] = inside
    for c in range(1, 8):
        dx, dy, dz = _dir(c)
        rec[:nx - dx, :ny - dy, :nz - dz, c] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
    return inside, rec.reshape(-1, 8)


def vertices(sdf, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0), t_clamp=0.0, dtype=np.float32, contracted=False, variant=None):
    """(verts [V, 3], vbase [npts] id of the first vertex of every grid point, vert_point [V] int64, vert_class [V] int32).

    contracted=True replaces the last step by fma(x, spacing, origin) (formed in fp64 from the fp32 operands, rounded once): NOT the
    specification; it exists so that a test can prove that its inputs tell the two apart."""
    sdf = np.ascontiguousarray(sdf, dtype=dtype)
    nx, ny, nz = sdf.shape
    _, rec = records(sdf, level, variant)
    flat = rec.reshape(-1)
    sel = np.nonzero(flat)[0]
    p, c = sel // 8, sel % 8
    vbase = (np.cumsum(rec.sum(1)) - rec.sum(1)).astype(np.int64)
    stride = np.array([ny * nz, nz, 1], dtype=np.int64)
    d = np.stack([c & 1, (c >> 1) & 1, (c >> 2) & 1], 1)
    f = sdf.reshape(-1)
    t = edge_t(f[p], f[p + d @ stride], level, t_clamp, dtype, variant)      # every operation rounded on its own
    t = np.where(c == 0, dtype(0), t).astype(dtype)
    idx = np.stack(np.unravel_index(p, (nx, ny, nz)), 1).astype(dtype)
    sp, org = np.asarray(spacing, dtype), np.asarray(origin, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        pos = np.where(d == 1, idx + t[:, None], idx).astype(dtype)
        if contracted:
            verts = (org.astype(np.float64) + pos.astype(np.float64) * sp.astype(np.float64)).astype(dtype)
        else:
            verts = (org + (pos * sp).astype(dtype)).astype(dtype)
    return verts.reshape(-1, 3), vbase, p.astype(np.int64), c.astype(np.int32)


def _orient(t, sgn):
    return t if sgn > 0 else (t[0], t[1], t[3], t[2])


def _parity(order):
    return perm_sign(order)


def _split_prism(a, b, sgn, stats=None):
    """Three tetrahedra of the prism (a0, a1, a2 | b0, b1, b2), vertical edges ai-bi, whose tetrahedron (a0, a1, a2, b0) has
    orientation sgn: every quadrilateral's diagonal leaves from its lowest id."""
    ids = list(a) + list(b)
    k = int(np.argmin(ids))
    if k >= 3:
        a, b, sgn, k = b, a, -sgn, k - 3
    a = (a[k], a[(k + 1) % 3], a[(k + 2) % 3])
    b = (b[k], b[(k + 1) % 3], b[(k + 2) % 3])
    m = min(a[1], a[2], b[2], b[1])
    first = m == a[1] or m == b[2]
    if stats is not None:
        stats["diagonal"].add(bool(first))
    if first:
        out = [(a[0], b[0], b[1], b[2]), (a[0], a[1], a[2], b[2]), (a[0], a[1], b[2], b[1])]
    else:
        out = [(a[0], b[0], b[1], b[2]), (a[0], a[1], a[2], b[1]), (a[0], a[2], b[2], b[1])]
    return [_orient(t, sgn) for t in out]


def _split_poly(u):
    """Triangles of an oriented polygon of 3 or 4 vertex ids: a quadrilateral's diagonal leaves from its lowest id."""
    if len(u) == 3:
        return [tuple(u)]
    k = int(np.argmin(u))
    u = [u[(k + r) % 4] for r in range(4)]
    return [(u[0], u[1], u[2]), (u[0], u[2], u[3])]


def tetrahedralize(sdf, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0), t_clamp=0.0, dtype=np.float32, stats=None, variant=None):
    """The mesh of the specification: a namespace of verts [V, 3], tets [T, 4] int32, bfaces [M, 3] int32, bface_kind [M] int8,
    vert_point [V] int64, vert_class [V] int32.  stats (a dict) receives the (permutation, inside mask) pairs met and the outcomes
    of the pyramid's diagonal."""
    sdf = np.ascontiguousarray(sdf, dtype=dtype)
    nx, ny, nz = sdf.shape
    dims = (nx, ny, nz)
    inside, rec = records(sdf, level, variant)
    verts, vbase, vert_point, vert_class = vertices(sdf, level, spacing, origin, t_clamp, dtype, variant=variant)
    ins = inside.reshape(-1)
    bits = (rec * (1 << np.arange(8))).sum(1).astype(np.int64)          # the point byte
    stride = (ny * nz, nz, 1)
    if stats is not None:
        stats.setdefault("cases", set())
        stats.setdefault("diagonal", set())
    tets, bfaces, kinds = [], [], []
    any_in = np.zeros((nx - 1, ny - 1, nz - 1), dtype=bool)
    for c in range(8):
        dx, dy, dz = _dir(c)
        any_in |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz]
    for i, j, k in zip(*np.nonzero(any_in)):                           # cells in linear order
        cell = (int(i), int(j), int(k))
        p = (cell[0] * ny + cell[1]) * nz + cell[2]
        for pi, perm in enumerate(PERMS):
            s = SIGNS[pi]
            q = [p + sum(((m >> a) & 1) * stride[a] for a in range(3)) for m in CORNERS[pi]]
            inn = [bool(ins[x]) for x in q]
            if stats is not None:
                stats["cases"].add((pi, sum(inn[r] << r for r in range(4))))
            n_in = sum(inn)
            if n_in == 0:
                continue

            def g(r):
                return int(vbase[q[r]])

            def e(r0, r1):
                lo, hi = min(r0, r1), max(r0, r1)
                c = CORNERS[pi][hi] ^ CORNERS[pi][lo]
                return int(vbase[q[lo]]) + bin(int(bits[q[lo]]) & ((1 << c) - 1)).count("1")

            I = [r for r in range(4) if inn[r]]
            O = [r for r in range(4) if not inn[r]]
            if n_in == 4:
                tets.append(_orient((g(0), g(1), g(2), g(3)), s))
            elif n_in == 1:
                A, (B, Cc, D) = I[0], O
                t = _orient((g(A), e(A, B), e(A, Cc), e(A, D)), s * _parity((A, B, Cc, D)))
                tets.append(t)
                bfaces.append(t[1:])
                kinds.append(0)
            elif n_in == 3:
                (A, B, Cc), D = I, O[0]
                sgn = s * _parity((A, B, Cc, D))
                a, b = (g(A), g(B), g(Cc)), (e(A, D), e(B, D), e(Cc, D))
                tets += _split_prism(a, b, sgn, stats)
                bfaces.append(b if sgn > 0 else (b[0], b[2], b[1]))
                kinds.append(0)
            else:
                (A, B), (Cc, D) = I, O
                sgn = s * _parity((A, Cc, D, B))
                a, b = (g(A), e(A, Cc), e(A, D)), (g(B), e(B, Cc), e(B, D))
                tets += _split_prism(a, b, sgn, stats)
                quad = [a[1], a[2], b[2], b[1]] if sgn > 0 else [a[1], b[1], b[2], a[2]]
                tr = _split_poly(quad)
                bfaces += tr
                kinds += [0] * len(tr)
            # the inside part of the two faces that can lie in an outer plane of the grid: (q0, q1, q2) in the low plane of
            # axis perm[2], (q1, q2, q3) in the high plane of axis perm[0]
            for face, on, kind in (((0, 1, 2) if s < 0 else (0, 2, 1), cell[perm[2]] == 0, 1 + 2 * perm[2]),
                                   ((1, 2, 3) if s > 0 else (1, 3, 2), cell[perm[0]] == dims[perm[0]] - 2, 2 + 2 * perm[0])):
                if not on:
                    continue
                poly = []
                for r in range(3):
                    X, Y = face[r], face[(r + 1) % 3]
                    if inn[X]:
                        poly.append(g(X))
                    if inn[X] != inn[Y]:
                        poly.append(e(X, Y))
                if poly:
                    tr = _split_poly(poly)
                    bfaces += tr
                    kinds += [kind] * len(tr)
    return SimpleNamespace(verts=verts, tets=np.array(tets, dtype=np.int32).reshape(-1, 4),
                           bfaces=np.array(bfaces, dtype=np.int32).reshape(-1, 3), bface_kind=np.array(kinds, dtype=np.int8),
                           vert_point=vert_point, vert_class=vert_class)


def counts(sdf, level=0.0):
    """(V, T, M) of the specification, vectorised: no mesh is built."""
    sdf = np.asarray(sdf)
    nx, ny, nz = sdf.shape
    inside, rec = records(sdf, level)
    V = int(rec.sum())
    cube = [inside[(m & 1):nx - 1 + (m & 1), ((m >> 1) & 1):ny - 1 + ((m >> 1) & 1), ((m >> 2) & 1):nz - 1 + ((m >> 2) & 1)].astype(np.int64)
            for m in range(8)]
    n_elems, n_cut, n_plane = np.array(N_ELEMS), np.array(N_CUT), np.array(N_PLANE)
    T = M = 0
    for pi, perm in enumerate(PERMS):
        c = [cube[m] for m in CORNERS[pi]]
        n_in = c[0] + c[1] + c[2] + c[3]
        T += int(n_elems[n_in].sum())
        M += int(n_cut[n_in].sum())
        lo = [slice(None)] * 3
        lo[perm[2]] = 0
        M += int(n_plane[(c[0] + c[1] + c[2])[tuple(lo)]].sum())
        hi = [slice(None)] * 3
        hi[perm[0]] = -1
        M += int(n_plane[(c[1] + c[2] + c[3])[tuple(hi)]].sum())
    return V, T, M


def components(sdf, level=0.0, variant=None):
    """(label [npts] int32: the lowest linear index of the point's solid component, -1 outside; size [npts] int32: the component's
    inside-point count at its root, 0 elsewhere).  Union-find over the 14-neighbour graph of the Kuhn edges."""
    sdf = np.asarray(sdf)
    nx, ny, nz = sdf.shape
    ins = is_inside(sdf, level, variant).reshape(-1)
    parent = np.arange(ins.size)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    idx = np.arange(ins.size).reshape(nx, ny, nz)
    for c in range(1, 8):
        dx, dy, dz = _dir(c)
        a, b = idx[:nx - dx, :ny - dy, :nz - dz].reshape(-1), idx[dx:, dy:, dz:].reshape(-1)
        for u, v in zip(a[ins[a] & ins[b]], b[ins[a] & ins[b]]):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    label = np.full(ins.size, -1, dtype=np.int32)
    size = np.zeros(ins.size, dtype=np.int32)
    for u in np.nonzero(ins)[0]:
        label[u] = find(u)
        size[label[u]] += 1
    return label, size


def component_depth(sdf, level=0.0):
    """The largest number of Kuhn edges on a shortest path from a component's root (its lowest index) to one of its points, over
    all components: breadth-first search on the 14-neighbour graph.  Min-label hooking carries a root's label at least one edge
    further per round (a point takes the lowest label its neighbours held when the round began), so it needs at most this many
    rounds to converge and one more to see that nothing changes."""
    sdf = np.asarray(sdf)
    ins = is_inside(sdf, level)
    label, _ = components(sdf, level)
    dist = np.full(sdf.shape, -1, dtype=np.int64)
    roots = np.unique(label[label >= 0])
    dist.reshape(-1)[roots] = 0
    dirs = [s * _dir(c) for c in range(1, 8) for s in (1, -1)]
    frontier = [tuple(int(x) for x in np.unravel_index(r, sdf.shape)) for r in roots]
    depth = 0
    while frontier:
        nxt = []
        for q in frontier:
            for d in dirs:
                r = (q[0] + int(d[0]), q[1] + int(d[1]), q[2] + int(d[2]))
                if all(0 <= r[a] < sdf.shape[a] for a in range(3)) and ins[r] and dist[r] < 0:
                    dist[r] = dist[q] + 1
                    nxt.append(r)
        if nxt:
            depth += 1
        frontier = nxt
    assert (dist[ins] >= 0).all()
    return depth


# ---- invariants -------------------------------------------------------------------------------------------------------------
def volumes(verts, tets):
    """fp64 signed volume of every element."""
    v = np.asarray(verts, dtype=np.float64)
    t = np.asarray(tets, dtype=np.int64)
    a = v[t[:, 0]]
    return np.einsum("ij,ij->i", v[t[:, 1]] - a, np.cross(v[t[:, 2]] - a, v[t[:, 3]] - a)) / 6.0


def surface_volume_terms(verts, faces):
    """The terms a . (b x c) / 6 of the divergence-theorem volume of an oriented triangle soup."""
    v = np.asarray(verts, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    return np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])) / 6.0


def element_faces(tets):
    """[4T, 3] outward faces of positively oriented elements (v0, v1, v2, v3): (v1, v2, v3), (v0, v3, v2), (v0, v1, v3), (v0, v2, v1)."""
    t = np.asarray(tets, dtype=np.int64)
    return np.concatenate([t[:, [1, 2, 3]], t[:, [0, 3, 2]], t[:, [0, 1, 3]], t[:, [0, 2, 1]]])


def _canon(f):
    """Every triangle rotated so that its lowest id comes first (orientation kept)."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    k = np.argmin(f, 1)
    r = np.arange(len(f))
    return np.stack([f[r, k], f[r, (k + 1) % 3], f[r, (k + 2) % 3]], 1)


def check_invariants(m, positive=True):
    """The conformity properties of the specification on a mesh; returns (sum of element volumes, boundary volume, bound)."""
    vol = volumes(m.verts, m.tets)
    if positive:
        assert (vol > 0).all(), f"{int((vol <= 0).sum())} of {len(vol)} elements are not positive (min {vol.min()})"
    ef = element_faces(m.tets)
    key = np.sort(ef, 1)
    uniq, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    assert cnt.max() <= 2, "a triangle lies in more than two elements"
    once = _canon(ef[cnt[inv.reshape(-1)] == 1])
    emitted = _canon(m.bfaces)
    a = {tuple(r) for r in once.tolist()}
    b = {tuple(r) for r in emitted.tolist()}
    assert len(b) == len(emitted), "a boundary triangle is emitted twice"
    assert a == b, f"boundary triangles: {len(a - b)} missing, {len(b - a)} surplus"
    f = np.asarray(m.bfaces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    fwd = {tuple(r) for r in d.tolist()}
    assert len(fwd) == len(d) and all((y, x) in fwd for x, y in fwd), "the boundary is not closed"
    terms = surface_volume_terms(m.verts, m.bfaces)
    return float(vol.sum()), float(terms.sum()), volume_bound(m.verts, m.tets, m.bfaces)


def _abs_products(a, b, c):
    """Sum of the magnitudes of the six products of the determinant |a b c|, per row."""
    a, b, c = np.abs(a), np.abs(b), np.abs(c)
    return sum(a[:, x] * b[:, y] * c[:, z] for x, y, z in itertools.permutations(range(3)))


def volume_bound(verts, tets, bfaces):
    """count * 2^-52 * sum |terms| for the two fp64 volume sums: a term is one product of three coordinates (differences for the
    elements; exact in fp64 from fp32 vertices), six to a determinant, each met by a bounded number of roundings of 2^-53."""
    v = np.asarray(verts, dtype=np.float64)
    t, f = np.asarray(tets, dtype=np.int64), np.asarray(bfaces, dtype=np.int64)
    a = v[t[:, 0]]
    mag = _abs_products(v[t[:, 1]] - a, v[t[:, 2]] - a, v[t[:, 3]] - a).sum() + _abs_products(v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]).sum()
    return float(6 * (len(t) + len(f)) * 2.0 ** -52 * mag / 6.0)
