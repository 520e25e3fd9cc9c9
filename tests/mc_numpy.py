"""Reference marching cubes in numpy, written from the specification in include/dsdf.h (dsdf_mc_*) with the generated case
table (deepsdf_amd/mc_table.py): the tests compare the HIP kernels against it array for array, and check mesh properties on it.
Also: a minimal binary-PLY reader and closed-manifold checks."""
import numpy as np

from deepsdf_amd import mc_table

OFFS = np.array([mc_table.corner_pos(c) for c in range(8)], dtype=np.int64)
EDGES = np.array(mc_table.EDGES, dtype=np.int64)
TABLE = np.array(mc_table.table_rows(), dtype=np.int64)
NTRI = np.array([len(t) for t in mc_table.TABLE], dtype=np.int64)


def marching_cubes(sdf, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """(verts [V, 3] float32, faces [F, 3] int32) in the library's order."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    nx, ny, nz = sdf.shape
    lvl = np.float32(level)
    inside = sdf < lvl
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    flat = cross.reshape(-1)                       # (grid point, axis), grid point linear order
    vid = np.cumsum(flat) - 1
    sel = np.nonzero(flat)[0]
    p, a = sel // 3, sel % 3
    stride = np.array([ny * nz, nz, 1], dtype=np.int64)
    f = sdf.reshape(-1)
    v0, v1 = f[p], f[p + stride[a]]
    t = (lvl - v0) / (v1 - v0)                     # float32 throughout, every operation rounded on its own
    pos = np.stack(np.unravel_index(p, (nx, ny, nz)), 1).astype(np.float32)
    pos[np.arange(len(p)), a] += t
    verts = np.asarray(origin, np.float32) + pos * np.asarray(spacing, np.float32)

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
    return verts.astype(np.float32), faces.reshape(-1, 3)


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
