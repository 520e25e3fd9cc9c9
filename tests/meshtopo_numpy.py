"""Pure-numpy fp64 oracle of csrc/meshtopo.hpp (include/dsdf.h dsdf_mt_*): half-edge mates by sorting, component labels by
union-find, the edge statistics, angle-weighted vertex normals, the enclosed volume and its vertex gradient, and the projection in
fp32 numpy with the device's operation order.  Also the hand-made meshes the tests share."""
import numpy as np

STATS = ("edges", "boundary", "nonmanifold", "paired", "same_direction", "degenerate_halfedges")


# ---- topology -----------------------------------------------------------------------------------------------------------------
def edge_keys(faces):
    """keys [3F] int64 of half-edges h = 3 f + k (faces[f][k] -> faces[f][(k + 1) % 3]): (min << 32) | max, -1 for equal ends."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    return np.where(a == b, -1, (np.minimum(a, b) << 32) | np.maximum(a, b))


def adjacency(faces):
    """(mate [3F] int32, stats dict): a half-edge whose key >= 0 occurs exactly twice gets the other one, every other -1."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    keys = edge_keys(f)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    mate = np.full(len(keys), -1, dtype=np.int32)
    uniq, first, count = np.unique(sk, return_index=True, return_counts=True)
    ok = uniq >= 0
    two = ok & (count == 2)
    h0, h1 = order[first[two]], order[first[two] + 1]
    mate[h0], mate[h1] = h1, h0
    a, b = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
    asc = a < b
    stats = dict(edges=int(ok.sum()), boundary=int((ok & (count == 1)).sum()), nonmanifold=int((ok & (count > 2)).sum()),
                 paired=int(two.sum()), same_direction=int((asc[h0] == asc[h1]).sum()), degenerate_halfedges=int((keys < 0).sum()))
    return mate, stats


def stats_list(stats):
    return [stats[k] for k in STATS]


def components(mate, n_faces):
    """(label [F] int32 = the lowest face index of the face's component, size [F] int32: the count at that face, 0 elsewhere)."""
    parent = np.arange(n_faces, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for h in np.nonzero(np.asarray(mate) >= 0)[0]:
        ru, rv = find(h // 3), find(int(mate[h]) // 3)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)                  # the root is always the lowest index of its tree
    label = np.array([find(x) for x in range(n_faces)], dtype=np.int32)
    size = np.bincount(label, minlength=n_faces).astype(np.int32) if n_faces else np.zeros(0, np.int32)
    return label, size


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def _tri(verts, faces):
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return v, f


def face_degenerate(verts, faces):
    v, f = _tri(verts, faces)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    lmax = np.maximum(((b - a) ** 2).sum(1), np.maximum(((c - a) ** 2).sum(1), ((c - b) ** 2).sum(1)))
    zero = (n * n).sum(1) <= 1e-14 * lmax * lmax
    return zero | (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])


def vertex_geometry(verts, faces):
    """(normals [V, 3] fp64 unit or exactly 0, |s| [V], sum of corner angles [V], vol_grad [V, 3] fp64, sum |b x c| / 6 [V])."""
    v, f = _tri(verts, faces)
    V = len(v)
    s, wsum, g, gabs = np.zeros((V, 3)), np.zeros(V), np.zeros((V, 3)), np.zeros(V)
    zero = face_degenerate(verts, faces) if len(f) else np.zeros(0, bool)
    for k in range(3):
        ia, ib, ic = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        a, b, c = v[ia], v[ib], v[ic]
        bc = np.cross(b, c)
        np.add.at(g, ia, bc)
        np.add.at(gabs, ia, np.abs(bc).max(1))
        e1, e2 = b - a, c - a
        n = np.cross(e1, e2)
        ln = np.sqrt((n * n).sum(1))
        live = ~zero
        ang = np.arctan2(ln[live], (e1[live] * e2[live]).sum(1))
        np.add.at(s, ia[live], (ang / ln[live])[:, None] * n[live])
        np.add.at(wsum, ia[live], ang)
    ls = np.sqrt((s * s).sum(1))
    normals = np.where(ls[:, None] > 0, s / np.where(ls > 0, ls, 1.0)[:, None], 0.0)
    return normals, ls, wsum, g / 6.0, gabs / 6.0


def volume(verts, faces):
    """((1 / 6) sum a . (b x c), (1 / 6) sum of the nine |products| per face: the scale of the sum's rounding)."""
    v, f = _tri(verts, faces)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    terms = (a * np.cross(b, c)).sum(1)
    mag = (np.abs(a) * (np.abs(b[:, [1, 2, 0]] * c[:, [2, 0, 1]]) + np.abs(b[:, [2, 0, 1]] * c[:, [1, 2, 0]]))).sum()
    return float(terms.sum() / 6.0), float(mag / 6.0)


def project(jac, axis, normals, stretch, clip):
    """dsdf_mt_project in fp32 numpy, the same products in the same order: out [V, 3, R]."""
    jac, n = np.asarray(jac, dtype=np.float32), np.asarray(normals, dtype=np.float32)
    a = np.asarray(axis, dtype=np.int64)
    j = jac * np.asarray(stretch, dtype=np.float32)[a][:, None]
    if clip > 0:
        j = np.where(np.abs(j) > np.float32(clip), np.float32(0), j)
    ja = j * n[np.arange(len(a)), a][:, None]
    out = ja[:, None, :] * n[:, :, None]
    assert out.dtype == np.float32
    return out


# ---- meshes -------------------------------------------------------------------------------------------------------------------
TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)            # outward


def hand_made():
    """{name: (verts, faces)}: the small meshes of the adjacency test."""
    two_v = np.concatenate([TET_V, TET_V + 2.0])
    out = {"tetrahedron": (TET_V, TET_F), "minus_one_face": (TET_V, TET_F[:3])}
    flipped = TET_F.copy()
    flipped[2] = flipped[2][::-1]
    out["one_face_flipped"] = (TET_V, flipped)
    share_v = TET_F + 3                                         # vertices 3 .. 6: vertex 3 is the first one's apex
    out["share_a_vertex"] = (np.concatenate([TET_V, TET_V[1:] + np.float32(1.5)]), np.concatenate([TET_F, share_v]))
    m = np.array([0, 1, 4, 5])                                  # the second tetrahedron reuses vertices 0 and 1: edge (0, 1) has 4 faces
    out["share_an_edge"] = (np.concatenate([TET_V, -TET_V[2:]]), np.concatenate([TET_F, m[TET_F]]))
    out["duplicated_face"] = (TET_V, np.concatenate([TET_F, TET_F[1:2]]))
    out["repeated_index"] = (TET_V, np.concatenate([TET_F, np.array([[3, 3, 1]], np.int32)]))
    # runs of equal keys at both ends of the sorted array: the lowest edge (0, 1) and the highest (5, 6) in three faces each, and
    # three half-edges of key -1 in front of everything
    ends = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4], [5, 6, 2], [6, 5, 3], [5, 6, 4], [2, 2, 2]], np.int32)
    out["runs_at_both_ends"] = (two_v[:7], ends)
    return out


def quad_strip(n_faces):
    """An open strip of n_faces triangles (a row of quads cut in two), vertices on two lines."""
    k = np.arange(n_faces)
    lo, hi = k // 2, k // 2 + (n_faces + 3) // 2
    even = np.stack([lo, lo + 1, hi], 1)
    odd = np.stack([lo + 1, hi + 1, hi], 1)
    faces = np.where((k % 2 == 0)[:, None], even, odd).astype(np.int32)
    m = (n_faces + 3) // 2
    x = np.arange(m, dtype=np.float32)
    verts = np.concatenate([np.stack([x, 0 * x, 0 * x], 1), np.stack([x, 0 * x + 1, 0 * x], 1)]).astype(np.float32)
    return verts, faces


def index_torus(nu, nv, offset=0):
    """Faces [2 nu nv, 3] of a closed nu x nv torus of vertex ids offset .. offset + nu nv - 1 (connectivity only)."""
    i, j = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    p = lambda a, b: offset + (a % nu) * nv + (b % nv)
    t1 = np.stack([p(i, j), p(i + 1, j), p(i + 1, j + 1)], -1).reshape(-1, 3)
    t2 = np.stack([p(i, j), p(i + 1, j + 1), p(i, j + 1)], -1).reshape(-1, 3)
    return np.concatenate([t1, t2]).astype(np.int32)


def torus_pair(nu, nv):
    return np.concatenate([index_torus(nu, nv), index_torus(nu, nv, nu * nv)])


def two_spheres(N=16):
    """The union of two separate spheres (radii 0.4 and 0.25) on an N^3 grid over [-1, 1]^3: (sdf float32, spacing)."""
    x = np.linspace(-1, 1, N, dtype=np.float64)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    sdf = np.minimum(np.sqrt((X + 0.55) ** 2 + Y * Y + Z * Z) - 0.4, np.sqrt((X - 0.55) ** 2 + Y * Y + Z * Z) - 0.25)
    return sdf.astype(np.float32), 2.0 / (N - 1)


_FIELD_MESHES = {}


def field_meshes():
    """{name: (verts float32, faces int32)} of the four marching-cubes meshes the tests share (tests/mc_numpy.py), built once."""
    if not _FIELD_MESHES:
        from tests import mc_numpy
        for name, (sdf, h) in (("sphere12", mc_numpy.sphere(12)), ("torus20", mc_numpy.torus(20)), ("two_spheres16", two_spheres(16)),
                               ("smooth_9_10_11", (mc_numpy.smooth_field((9, 10, 11), 3), 0.125))):
            v, f = mc_numpy.marching_cubes(sdf, 0.0, (h, h, h), (-1.0, -1.0, -1.0))
            v.setflags(write=False)
            f.setflags(write=False)
            _FIELD_MESHES[name] = (v, f)
    return _FIELD_MESHES


def relabel(label, perm):
    """Labels and sizes of the mesh faces[perm] from the labels of faces: face i of the permuted mesh is face perm[i]."""
    comp = np.asarray(label)[perm]                              # the component of every permuted face, named by its old label
    lowest = np.full(len(label), len(label), dtype=np.int64)
    np.minimum.at(lowest, comp, np.arange(len(perm)))
    new = lowest[comp].astype(np.int32)
    return new, np.bincount(new, minlength=len(perm)).astype(np.int32)
