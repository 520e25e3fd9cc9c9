"""fp64 numpy oracle of the mesh SDF (include/dsdf.h dsdf_msdf_*, csrc/meshsdf.hpp) and the test meshes.  No torch.

Oracle, restated from the spec: closest point of the closed triangle by Ericson's region tests (Real-Time Collision Detection
5.1.5; va, vb, vc from triple products with the normal) -- a zero-area face by its three edges instead --, squared distance
from the explicit difference vector, lowest face index on ties; winding number = sum of Van Oosterom-Strackee solid angles / 4 pi; inside iff floor(|w| + 0.5) is odd.  The
inputs are rounded to fp32 first (what the kernel sees), then everything runs in fp64, queries in chunks.
"""
import numpy as np


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _segment(p, a, b):
    """Closest points on segments a-b (broadcast) to p."""
    ab = b - a
    den = np.einsum("...i,...i->...", ab, ab)
    t = np.where(den > 0, np.einsum("...i,...i->...", p - a, ab) / np.where(den > 0, den, 1.0), 0.0)
    return a + np.clip(t, 0.0, 1.0)[..., None] * ab


def _dot(x, y):
    return np.einsum("...i,...i->...", x, y)


def _ericson(p, a, b, c):
    """(d1 .. d6, va, vb, vc, ab, ac) of Ericson's test for points p against triangles (a, b, c), broadcast, fp64.
    d3 .. d6 follow from d1, d2 and the edges' dot products (bp = ap - ab, cp = ap - ac).  va, vb, vc are |n|^2 times the
    barycentric coordinates.  Ericson takes them from the dot products (vc = d1 d4 - d3 d2, ...), whose rounding is absolute,
    ~1e-16 of |ab|^2 |ap|^2: on a sliver of height 1e-6 (|n|^2 = 1e-12) that leaves the interior quotient four digits.  By
    Lagrange's identity they are triple products with the normal, vc = n . (ab x ap) = ap . (n x ab) and so on, whose rounding
    is relative to |n|; the vectors n x ab, ac x n, n x bc belong to the face alone."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bb, bc, cc = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
    d3, d4, d5, d6 = d1 - bb, d2 - bc, d1 - bc, d2 - cc
    n = np.cross(ab, ac)
    vc, vb = _dot(ap, np.cross(n, ab)), _dot(ap, np.cross(ac, n))
    va = _dot(ap, np.cross(n, ac - ab)) + _dot(n, n)             # bp . (n x bc), with ab . (n x bc) = -|n|^2
    return (d1, d2, d3, d4, d5, d6), (va, vb, vc), ab, ac


def _region_tests(d, v):
    """Ericson's six tests in his order: A, B, AB, C, AC, BC (interior: none of them)."""
    (d1, d2, d3, d4, d5, d6), (va, vb, vc) = d, v
    return [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
            (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]


def closest_points(p, a, b, c):
    """Closest points of triangles (a, b, c) to points p (all [..., 3], broadcast), fp64.  Ericson's regions; degenerate
    triangles (zero area) take the closest of their three edges."""
    d, vs, ab, ac = _ericson(p, a, b, c)
    (d1, d2, d3, d4, d5, d6), (va, vb, vc) = d, vs
    nn = _dot(np.cross(ab, ac), np.cross(ab, ac))
    lmax = np.maximum(np.maximum(_dot(ab, ab), _dot(ac, ac)), _dot(c - b, c - b))
    degen = nn <= 1e-14 * lmax * lmax
    with np.errstate(divide="ignore", invalid="ignore"):
        den = va + vb + vc
        v, w = vb / den, vc / den                                  # interior; NaN only on degenerate faces, replaced below
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
    one, zero = np.ones_like(v), np.zeros_like(v)
    tests = _region_tests(d, vs)
    for m, vv, ww in reversed(list(zip(tests, (zero, one, t_ab, zero, zero, 1 - t_bc), (zero, zero, zero, one, t_ac, t_bc)))):
        v, w = np.where(m, vv, v), np.where(m, ww, w)              # the first match in Ericson's order is assigned last
    out = a + v[..., None] * ab + w[..., None] * ac
    if np.any(degen):
        s = [_segment(p, a, b), _segment(p, b, c), _segment(p, c, a)]
        dd = np.stack([((p - x) ** 2).sum(-1) for x in s], -1)
        k = np.argmin(dd, -1)
        seg = np.choose(k[..., None], s)
        out = np.where(degen[..., None], seg, out)
    return out


def solid_angles(p, a, b, c):
    """Signed solid angles of triangles (a, b, c) seen from p (Van Oosterom-Strackee), fp64.  The numerator A . (B x C) equals
    A . ((b - a) x (c - a)): one dot product with the face's normal."""
    A, B, Cc = a - p, b - p, c - p
    la, lb, lc = (np.sqrt(_dot(x, x)) for x in (A, B, Cc))
    det = _dot(A, np.cross(b - a, c - a))
    den = la * lb * lc + _dot(A, B) * lc + _dot(B, Cc) * la + _dot(Cc, A) * lb
    return 2.0 * np.arctan2(det, den)


def mesh_query(V, F, P, chunk_pairs=4_000_000):
    """(d2, face, closest, w) of every query: fp64 on fp32-rounded inputs."""
    V, P = _f32(V), _f32(P)
    F = np.asarray(F, dtype=np.int64)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    n = (np.cross(b - a, c - a) ** 2).sum(-1)
    lmax = np.max(np.stack([((b - a) ** 2).sum(-1), ((c - a) ** 2).sum(-1), ((c - b) ** 2).sum(-1)]), 0)
    wt = (n > 1e-14 * lmax * lmax).astype(np.float64)        # zero-area faces add no winding
    nq, nf = len(P), len(F)
    d2, face, cl, w = np.empty(nq), np.empty(nq, np.int64), np.empty((nq, 3)), np.empty(nq)
    step = max(1, chunk_pairs // max(nf, 1))
    for s in range(0, nq, step):
        p = P[s:s + step, None, :]
        cp = closest_points(p, a[None], b[None], c[None])
        dd = ((p - cp) ** 2).sum(-1)
        k = np.argmin(dd, 1)                                   # first minimum: the lowest face index
        r = np.arange(len(k))
        d2[s:s + step], face[s:s + step], cl[s:s + step] = dd[r, k], k, cp[r, k]
        w[s:s + step] = (solid_angles(p, a[None], b[None], c[None]) * wt).sum(1) / (4 * np.pi)
    return d2, face, cl, w


def face_distance(V, F, P, face):
    """sqrt of the squared distance from each query to the face given for it (fp64)."""
    V, P = _f32(V), _f32(P)
    F = np.asarray(F, dtype=np.int64)[face]
    cp = closest_points(P, V[F[:, 0]], V[F[:, 1]], V[F[:, 2]])
    return np.sqrt(((P - cp) ** 2).sum(-1))


def inside(w):
    return (np.floor(np.abs(w) + 0.5).astype(np.int64) % 2) == 1


def mesh_sdf(V, F, P):
    d2, _, _, w = mesh_query(V, F, P)
    d = np.sqrt(d2)
    return np.where(inside(w), -d, d)


# ---- meshes (outward-facing, counter-clockwise seen from outside) ---------------------------------------------------------
def cube(h=1.0):
    """Axis-aligned cube [-h, h]^3, 12 triangles."""
    V = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], dtype=np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    F = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int64)
    return V, F


def box_sdf(P, h=1.0):
    q = np.abs(P) - h
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)


def icosphere(subdiv=2, r=1.0, center=(0, 0, 0)):
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    V = [np.array(v, float) / np.linalg.norm(v) for v in V]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            k = (min(i, j), max(i, j))
            if k not in mid:
                v = V[i] + V[j]
                V.append(v / np.linalg.norm(v))
                mid[k] = len(V) - 1
            return mid[k]
        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = nf
    return np.array(V) * r + np.asarray(center, float), np.array(F, dtype=np.int64)


def torus(R=0.6, r=0.25, n=32, m=16):
    u, v = np.meshgrid(np.arange(n) * 2 * np.pi / n, np.arange(m) * 2 * np.pi / m, indexing="ij")
    V = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    F = []
    for i in range(n):
        for j in range(m):
            a, b, c, d = i * m + j, ((i + 1) % n) * m + j, ((i + 1) % n) * m + (j + 1) % m, i * m + (j + 1) % m
            F += [(a, b, c), (a, c, d)]
    return V, np.array(F, dtype=np.int64)


def concat(*meshes):
    Vs, Fs, off = [], [], 0
    for V, F in meshes:
        Vs.append(V)
        Fs.append(F + off)
        off += len(V)
    return np.concatenate(Vs), np.concatenate(Fs)


def nested_shells(subdiv=2):
    """A sphere of radius 0.9 with a spherical cavity of radius 0.4 (both outward-facing: the parity rule, not the
    orientation, makes the cavity outside)."""
    return concat(icosphere(subdiv, 0.9), icosphere(subdiv, 0.4))


def two_parts(subdiv=2):
    return concat(icosphere(subdiv, 0.4, (-0.5, 0, 0)), icosphere(subdiv, 0.3, (0.5, 0.1, 0)))


def hemisphere(subdiv=2):
    """The z >= 0 half of an icosphere: an open surface (fractional winding numbers)."""
    V, F = icosphere(subdiv)
    keep = (V[F][:, :, 2] >= -1e-9).all(1)
    return V, F[keep]


# ---- a second fp64 formulation, region names, and the inputs of tests/test_gpu_meshsdf_faces.py -----------------------------
def closest_points_edges_plane(p, a, b, c):
    """Closest points of non-degenerate triangles by another route than closest_points: the nearest of the three clamped edge
    segments, or the foot of the perpendicular on the plane when it lies on the inner side of all three edges (signed areas
    against the normal).  fp64, broadcast like closest_points."""
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    n = np.cross(b - a, c - a)
    s = [_segment(p, a, b), _segment(p, b, c), _segment(p, c, a)]
    d = np.stack([((p - x) ** 2).sum(-1) for x in s], -1)
    out = np.choose(np.argmin(d, -1)[..., None], s)
    side = [(np.cross(y - x, p - x) * n).sum(-1) for x, y in ((a, b), (b, c), (c, a))]
    foot = p - ((p - a) * n).sum(-1, keepdims=True) / (n * n).sum(-1, keepdims=True) * n
    return np.where(((side[0] >= 0) & (side[1] >= 0) & (side[2] >= 0))[..., None], foot, out)


REGIONS = ("A", "B", "AB", "C", "AC", "BC", "IN")


def regions(p, a, b, c):
    """Index into REGIONS of Ericson's region of each query, first match in his order (what closest_points resolves)."""
    d, v, _, _ = _ericson(p, a, b, c)
    tests = _region_tests(d, v)
    out = np.full(tests[0].shape, 6)
    for k in range(5, -1, -1):
        out = np.where(tests[k], k, out)
    return out


def is_zero_area(V, F):
    """The spec's zero-area rule per face, fp64 on the fp32-rounded vertices."""
    V = _f32(V)
    a, b, c = (V[np.asarray(F)[:, k]] for k in range(3))
    n = (np.cross(b - a, c - a) ** 2).sum(-1)
    lmax = np.max(np.stack([((b - a) ** 2).sum(-1), ((c - a) ** 2).sum(-1), ((c - b) ** 2).sum(-1)]), 0)
    return n <= 1e-14 * lmax * lmax


def random_rotation(g):
    """A proper rotation drawn from generator g (QR of a Gaussian matrix)."""
    q, r = np.linalg.qr(g.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


VERTEX_ORDERS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))
SLIVER_HEIGHTS = (1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)
SLIVER_QUERY_HEIGHTS = (0.0, 1e-3, -1e-3, 0.05, -0.05, 0.3, -0.3)


def sliver(family, h, g):
    """One triangle with unit longest edge and height h, in its own frame (long axis x, lateral y, normal z): 'needle' has its
    apex over the middle third of the base, 'short_base' a base of length h."""
    if family == "needle":
        return np.array([[0, 0, 0], [1, 0, 0], [g.uniform(1 / 3, 2 / 3), h, 0]], dtype=np.float64)
    return np.array([[0, 0, 0], [1, -h / 2, 0], [1, h / 2, 0]], dtype=np.float64)


def sliver_queries(h, g, per_height=150):
    """Queries over and beside a sliver of sliver(): along the long axis in [-0.2, 1.2], laterally N(0, 3h), at the heights of
    SLIVER_QUERY_HEIGHTS."""
    return np.concatenate([np.stack([g.uniform(-0.2, 1.2, per_height), g.normal(0, 3 * h, per_height),
                                     np.full(per_height, z)], 1) for z in SLIVER_QUERY_HEIGHTS])


def sliver_cases(h, seed=0, poses=3, per_height=150):
    """The sliver sweep at height h: (family, V [3, 3], F [1, 3], P) for both families, every vertex order and `poses` seeded
    rotations and offsets in [-0.5, 0.5]^3.  V and P are rounded to fp32 (what the kernel sees)."""
    g = np.random.default_rng([seed, int(round(-np.log10(h)))])
    for family in ("needle", "short_base"):
        for _ in range(poses):
            T, R, off = sliver(family, h, g), random_rotation(g), g.uniform(-0.5, 0.5, 3)
            P = _f32(sliver_queries(h, g, per_height) @ R.T + off)
            V = _f32(T @ R.T + off)
            for order in VERTEX_ORDERS:
                yield family, V, np.array([order], dtype=np.int64), P


def plate(t, g):
    """cube() scaled by (1, 1, t) and rotated: a closed mesh whose four side walls are slivers of aspect t."""
    V, F = cube()
    return (V * [1, 1, t]) @ random_rotation(g).T, F


def plate_queries(V, F, t, g, n=1500):
    """Queries around the rim and near the faces of plate(): random surface points plus offsets at the plate's own scale (t) and
    at 0.05, half each, and a few far ones."""
    f = g.integers(0, len(F), n)
    u, v = g.random(n), g.random(n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    a, b, c = V[F[f, 0]], V[F[f, 1]], V[F[f, 2]]
    s = np.where(np.arange(n) % 2 == 0, 2 * t, 0.05)[:, None]
    return np.concatenate([a + u[:, None] * (b - a) + v[:, None] * (c - a) + g.normal(0, 1, (n, 3)) * s,
                           g.uniform(-1.5, 1.5, (n // 5, 3))])


def ribbon(aspect, g, n=40):
    """An open strip of n needle triangles: unit length, width `aspect`, cut across n / 2 times, so every triangle has height
    ~aspect against a longest edge of 1; randomly rotated."""
    k = n // 2
    y = np.linspace(0, aspect, k + 1)
    V = np.concatenate([np.stack([np.zeros(k + 1), y, np.zeros(k + 1)], 1), np.stack([np.ones(k + 1), y, np.zeros(k + 1)], 1)])
    F = np.array([t for i in range(k) for t in ((i, k + 1 + i, k + 2 + i), (i, k + 2 + i, i + 1))], dtype=np.int64)
    return V @ random_rotation(g).T, F
