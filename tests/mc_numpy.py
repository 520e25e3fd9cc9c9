"""Reference marching cubes in numpy, written from the specification in include/dsdf.h (dsdf_mc_*) with the generated case
table (deepsdf_amd/mc_table.py): the tests compare the HIP kernels against it array for array, and check mesh properties on it.
Also: a minimal binary-PLY reader and closed-manifold checks."""
import numpy as np

from deepsdf_amd import mc_table

OFFS = np.array([mc_table.corner_pos(c) for c in range(8)], dtype=np.int64)
EDGES = np.array(mc_table.EDGES, dtype=np.int64)
TABLE = np.array(mc_table.table_rows(), dtype=np.int64)
NTRI = np.array([len(t) for t in mc_table.TABLE], dtype=np.int64)


def _crossings(sdf, level):
    """(inside [nx, ny, nz], flat crossing flags [(grid point, axis)], grid point p and axis a of every crossing edge)."""
    inside = sdf < np.float32(level)
    nx, ny, nz = sdf.shape
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)                       # (grid point, axis), grid point linear order
    sel = np.nonzero(flat)[0]
    return inside, flat, sel // 3, sel % 3


def vertices(sdf, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0), contracted=False):
    """verts [V, 3] float32 in the library's order: origin + (p + t e_a) * spacing, fp32, every operation rounded on its own.

    contracted=True replaces the last step by fma(x, spacing, origin) -- what a compiler makes of it when it may contract -- formed
    in fp64 from the fp32 operands (the product is exact there) and rounded to fp32 once.  It is NOT the specification: it exists
    so that a test can prove that its inputs tell the two apart."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    nx, ny, nz = sdf.shape
    lvl = np.float32(level)
    _, _, p, a = _crossings(sdf, level)
    stride = np.array([ny * nz, nz, 1], dtype=np.int64)
    f = sdf.reshape(-1)
    v0, v1 = f[p], f[p + stride[a]]
    t = (lvl - v0) / (v1 - v0)                     # float32 throughout, every operation rounded on its own
    pos = np.stack(np.unravel_index(p, (nx, ny, nz)), 1).astype(np.float32)
    pos[np.arange(len(p)), a] += t
    if contracted:
        return (np.asarray(origin, np.float32).astype(np.float64) +
                pos.astype(np.float64) * np.asarray(spacing, np.float32).astype(np.float64)).astype(np.float32)
    return (np.asarray(origin, np.float32) + pos * np.asarray(spacing, np.float32)).astype(np.float32)


def marching_cubes(sdf, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0), contracted=False):
    """(verts [V, 3] float32, faces [F, 3] int32) in the library's order; the vertex arithmetic is that of vertices()."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    nx, ny, nz = sdf.shape
    inside, flat, _, _ = _crossings(sdf, level)
    vid = np.cumsum(flat) - 1
    stride = np.array([ny * nz, nz, 1], dtype=np.int64)
    verts = vertices(sdf, level, spacing, origin, contracted)

    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = OFFS[c]
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ci, cj, ck = np.nonzero(NTRI[case] > 0)        # cells in linear order
    cs = case[ci, cj, ck]
    cell_p = (ci * ny + cj) * nz + ck
    rows = TABLE[cs][:, :3 * mc_table.MAX_TRIS].reshape(len(cs), mc_table.MAX_TRIS, 3)
    valid = rows[:, :, 0] >= 0
    e = rows[valid]                                # [F, 3] edge ids, cell order then table order
    cp = np.broadcast_to(cell_p[:, None], valid.shape)[valid]
    corner, axis = EDGES[e, 0], EDGES[e, 1]
    q = cp[:, None] + OFFS[corner] @ stride
    faces = vid[q * 3 + axis].astype(np.int32)
    return verts, faces.reshape(-1, 3)


def closed_manifold_stats(verts, faces):
    """(every edge in exactly two faces with opposite directions, Euler characteristic, signed volume)."""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    nv = max(len(verts), 1)
    key = d[:, 0] * nv + d[:, 1]
    rkey = d[:, 1] * nv + d[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    ok = bool((cnt == 1).all()) and bool(np.isin(rkey, uniq).all()) and not bool((d[:, 0] == d[:, 1]).any())
    n_edges = len(uniq) // 2
    euler = len(verts) - n_edges + len(f)
    v = np.asarray(verts, dtype=np.float64)
    vol = float(np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]])).sum() / 6.0)
    return ok, euler, vol


def read_ply(path):
    """Parse a binary little-endian PLY with float x, y, z vertices and `list uchar int` faces -> (header, verts, faces)."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii")
    nv = nf = None
    for line in header.splitlines():
        w = line.split()
        if w[:2] == ["element", "vertex"]:
            nv = int(w[2])
        elif w[:2] == ["element", "face"]:
            nf = int(w[2])
    verts = np.frombuffer(raw, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    rec = np.frombuffer(raw, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=end + 12 * nv)
    assert (rec["n"] == 3).all()
    assert len(raw) == end + 12 * nv + 13 * nf
    return header, verts, rec["idx"].copy()


def sphere(N, r=0.5):
    x = np.linspace(-1, 1, N, dtype=np.float64)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (np.sqrt(X * X + Y * Y + Z * Z) - r).astype(np.float32), 2.0 / (N - 1)


def torus(N, R=0.5, r=0.2):
    x = np.linspace(-1, 1, N, dtype=np.float64)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return (np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z) - r).astype(np.float32), 2.0 / (N - 1)


def smooth_field(shape, seed):
    """A seeded sum of six products of sines on a grid of any shape, float32: a smooth field with many level crossings."""
    g = np.random.default_rng(seed)
    axes = np.meshgrid(*[np.linspace(0, 1, n) for n in shape], indexing="ij")
    out = np.zeros(shape)
    for _ in range(6):
        k, ph, a = g.uniform(1, 6, 3), g.uniform(0, 2 * np.pi, 3), g.uniform(0.2, 1.0)
        out += a * np.sin(k[0] * axes[0] + ph[0]) * np.sin(k[1] * axes[1] + ph[1]) * np.sin(k[2] * axes[2] + ph[2])
    return out.astype(np.float32)


# a non-cubic grid whose spacing and origin are not dyadic on any axis: x * spacing is inexact, so a fused origin + x * spacing shows
NON_DYADIC = dict(shape=(33, 40, 47), seed=5, level=0.1, spacing=(0.3, 0.7, 1.1), origin=(3.1, -1.3, 0.55))


def differing(a, b):
    """(entries whose bits differ, entries) of two float32 arrays of one shape."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    return int((a.view(np.uint32) != b.view(np.uint32)).sum()), a.size


def ulp_distance(a, b):
    """Largest distance of two float32 arrays in units in the last place (adjacent floats are 1 apart, +0 and -0 are 0 apart)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    return int(d.max()) if d.size else 0
