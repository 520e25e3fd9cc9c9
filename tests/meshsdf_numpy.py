"""fp64 numpy oracle of the mesh SDF (include/dsdf.h dsdf_msdf_*, csrc/meshsdf.hpp) and the test meshes.  No torch.

Oracle, restated from the spec: closest point of the closed triangle by Ericson's region tests (Real-Time Collision Detection
5.1.5) -- a zero-area face by its three edges instead --, squared distance from the explicit difference vector, lowest face
index on ties; winding number = sum of Van Oosterom-Strackee solid angles / 4 pi; inside iff floor(|w| + 0.5) is odd.  The
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


def closest_points(p, a, b, c):
    """Closest points of triangles (a, b, c) to points p (all [..., 3], broadcast), fp64.  Ericson's regions; degenerate
    triangles (zero area) take the closest of their three edges."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    bp = p - b
    d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
    cp = p - c
    d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    n = np.cross(ab, ac)
    nn = (n * n).sum(-1)
    lmax = np.maximum(np.maximum((ab * ab).sum(-1), (ac * ac).sum(-1)), ((c - b) ** 2).sum(-1))
    degen = nn <= 1e-14 * lmax * lmax
    with np.errstate(divide="ignore", invalid="ignore"):
        den = va + vb + vc
        v_in, w_in = vb / den, vc / den
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        out = a + v_in[..., None] * ab + w_in[..., None] * ac        # NaN only on degenerate faces, replaced below
    regions = [  # Ericson's order reversed: later assignments win
        ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), lambda: b + t_bc[..., None] * (c - b)),
        ((vb <= 0) & (d2 >= 0) & (d6 <= 0), lambda: a + t_ac[..., None] * ac),
        ((d6 >= 0) & (d5 <= d6), lambda: np.broadcast_to(c, out.shape)),
        ((vc <= 0) & (d1 >= 0) & (d3 <= 0), lambda: a + t_ab[..., None] * ab),
        ((d3 >= 0) & (d4 <= d3), lambda: np.broadcast_to(b, out.shape)),
        ((d1 <= 0) & (d2 <= 0), lambda: np.broadcast_to(a, out.shape)),
    ]
    for m, f in regions:
        out = np.where(m[..., None], f(), out)
    if np.any(degen):
        s = [_segment(p, a, b), _segment(p, b, c), _segment(p, c, a)]
        d = np.stack([((p - x) ** 2).sum(-1) for x in s], -1)
        k = np.argmin(d, -1)
        seg = np.choose(k[..., None], s)
        out = np.where(degen[..., None], seg, out)
    return out


def solid_angles(p, a, b, c):
    """Signed solid angles of triangles (a, b, c) seen from p (Van Oosterom-Strackee), fp64."""
    A, B, Cc = a - p, b - p, c - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (A, B, Cc))
    det = (A * np.cross(B, Cc)).sum(-1)
    den = la * lb * lc + (A * B).sum(-1) * lc + (B * Cc).sum(-1) * la + (Cc * A).sum(-1) * lb
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
