"""Tetrahedral volume meshes of the solid {sdf < level} of a dense device grid (csrc/tetmesh.hpp, dsdf_tet_*).

    mesh    tetrahedralize    count / scan / emit on the device, one host sync to read the three totals: vertices, positively
                              oriented elements, outward boundary triangles with the outer plane each lies in
    solid   solid_components  connected components of the inside grid points under the Kuhn edges (= the mesh's components)
    TetMesh                   volumes, the boundary as a SurfaceMesh on the same vertex ids, the reference's boundary attributes,
                              and the MFEM mesh v1.0 writer

The reference builds this stage with tetgenpy and gustaf from the surface (analysis/geometry.py tetrahedralize_surface /
export_volume_mesh); here the elements come straight from the grid the surface came from.  There is no CPU path for the mesher;
a TetMesh built from arrays (an oracle's, a file's) can still be measured and written on the host."""
import ctypes as C

import numpy as np
import torch

from . import _lib      # and nothing from mesh.py, which re-exports this module: either can be imported first

INT32_MAX = 2 ** 31 - 1


def _check_grid(sdf_grid, what):
    g = sdf_grid
    if not torch.is_tensor(g) or g.dim() != 3:
        raise ValueError(f"{what} expects a 3-D tensor [nx, ny, nz]")
    if g.device.type != "cuda":
        raise _lib.DsdfError(f"{what} needs a grid on a HIP device (no CPU fallback)")
    return g.to(torch.float32).contiguous()


def _workspace(g):
    b = C.c_size_t()
    _lib.check(_lib.lib().dsdf_tet_workspace_bytes(*g.shape, C.byref(b)))
    return torch.empty(b.value, dtype=torch.uint8, device=g.device)


def solid_components(sdf_grid, level=0.0):
    """(label [nx, ny, nz] int32: the lowest linear index of the point's component of the solid {sdf < level}, -1 outside;
    size [nx, ny, nz] int32: the component's inside-point count at its root, 0 elsewhere; rounds: hooking rounds run).  Two inside
    points are connected when a Kuhn edge joins them (14 neighbours): exactly the components of tetrahedralize's mesh."""
    g = _check_grid(sdf_grid, "solid_components")
    nx, ny, nz = g.shape
    with torch.cuda.device(g.device):
        ws = _workspace(g)
        label = torch.empty(g.shape, dtype=torch.int32, device=g.device)
        size = torch.empty(g.shape, dtype=torch.int32, device=g.device)
        rounds = C.c_int32()
        _lib.check(_lib.lib().dsdf_tet_components(_lib.ptr(g), nx, ny, nz, float(level), _lib.ptr(label), _lib.ptr(size), C.byref(rounds),
                                                  _lib.ptr(ws), ws.numel(), _lib.stream()))
    return label, size, rounds.value


def largest_component_only(sdf_grid, level=0.0):
    """The grid with every inside point outside the largest component (most inside points; ties: the lowest label) set to a value
    that is not inside.  No edge joins a kept point to a dropped one, so the kept component meshes bit for bit as before."""
    g = _check_grid(sdf_grid, "largest_component_only")
    label, size, _ = solid_components(g, level)
    flat = size.reshape(-1)
    if int(flat.max()) == 0:
        return g
    root = int(torch.argmax(flat))                    # the first maximum: the lowest label among the largest
    fill = torch.full((), float(level), dtype=torch.float32, device=g.device)
    return torch.where((label >= 0) & (label != root), fill, g)


def tetrahedralize(sdf_grid, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), *, t_clamp=0.0, keep_largest=False,
                   return_edges=False):
    """Tetrahedral mesh of {sdf < level} on a dense device grid sdf_grid [nx, ny, nz] (z fastest; 2 <= n <= 1024 per axis;
    spacing > 0): a TetMesh on the grid's device.  Geometry, order and orientation: include/dsdf.h (dsdf_tet_*).

    t_clamp in [0, 0.5): every edge parameter is clamped to [t_clamp, 1 - t_clamp], which bounds how thin a cut element can get
    (0: untouched; a grid value equal to level then gives zero-volume elements, see TetMesh.volumes).  keep_largest: mesh only the
    largest solid component.  return_edges: also vert_point [V] int64 / vert_class [V] int32, the grid point and the edge class
    (0: the grid point itself) of every vertex."""
    t_clamp = float(t_clamp)
    if not 0.0 <= t_clamp < 0.5:
        raise ValueError(f"t_clamp must lie in [0, 0.5), got {t_clamp}")
    g = _check_grid(sdf_grid, "tetrahedralize")
    if keep_largest:
        g = largest_component_only(g, level)
    nx, ny, nz = g.shape
    lib = _lib.lib()
    sp, org = (C.c_float * 3)(*_lib.triple(spacing, "spacing")), (C.c_float * 3)(*_lib.triple(origin, "origin"))
    dev = g.device
    with torch.cuda.device(dev):
        ws = _workspace(g)
        totals = torch.empty(3, dtype=torch.int64, device=dev)
        _lib.check(lib.dsdf_tet_count(_lib.ptr(g), nx, ny, nz, float(level), _lib.ptr(totals), _lib.ptr(ws), ws.numel(), _lib.stream()))
        nv, nt, nb = totals.tolist()                        # the one host sync of a mesh
        if max(nv, nt, nb) > INT32_MAX:                     # the library refuses before writing anything: raise its error
            _lib.check(lib.dsdf_tet_emit(_lib.ptr(g), nx, ny, nz, float(level), sp, org, t_clamp, nv, nt, nb, None, None, None, None,
                                         None, None, _lib.ptr(ws), ws.numel(), _lib.stream()))
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        tets = torch.empty(nt, 4, dtype=torch.int32, device=dev)
        bfaces = torch.empty(nb, 3, dtype=torch.int32, device=dev)
        kind = torch.empty(nb, dtype=torch.int8, device=dev)
        vp = torch.empty(nv, dtype=torch.int64, device=dev) if return_edges else None
        vc = torch.empty(nv, dtype=torch.int32, device=dev) if return_edges else None
        _lib.check(lib.dsdf_tet_emit(_lib.ptr(g), nx, ny, nz, float(level), sp, org, t_clamp, nv, nt, nb, _lib.ptr(verts), _lib.ptr(tets),
                                     _lib.ptr(bfaces), _lib.ptr(kind), _lib.ptr(vp), _lib.ptr(vc), _lib.ptr(ws), ws.numel(), _lib.stream()))
    m = TetMesh(verts, tets, bfaces, kind, vp, vc)
    m._indices_checked = True                               # the kernels' own ids: boundary_surface need not range-check them
    return m


class TetMesh:
    """verts [V, 3], tets [T, 4] int32 (positively oriented), bfaces [M, 3] int32 (outward), bface_kind [M] int8 (0: a cut face,
    1..6: the outer grid plane -x, +x, -y, +y, -z, +z), optionally vert_point [V] int64 / vert_class [V] int32.  Tensors on any
    device, or arrays (moved to host tensors)."""

    def __init__(self, verts, tets, bfaces, bface_kind, vert_point=None, vert_class=None):
        def t(x, dtype=None):
            if x is None:
                return None
            x = x.detach() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            return x if dtype is None else x.to(dtype)
        self.verts = t(verts)
        self.tets, self.bfaces, self.bface_kind = t(tets, torch.int32), t(bfaces, torch.int32), t(bface_kind, torch.int8)
        self.vert_point, self.vert_class = t(vert_point, torch.int64), t(vert_class, torch.int32)
        if self.verts.dim() != 2 or self.verts.shape[1] != 3 or self.tets.dim() != 2 or self.tets.shape[1] != 4 or \
                self.bfaces.dim() != 2 or self.bfaces.shape[1] != 3 or self.bface_kind.shape != self.bfaces.shape[:1]:
            raise ValueError("TetMesh needs verts [V, 3], tets [T, 4], bfaces [M, 3] and bface_kind [M]")
        self._indices_checked = False                          # arrays of any origin: SurfaceMesh checks their range

    @property
    def device(self):
        return self.verts.device

    @property
    def n_verts(self):
        return int(self.verts.shape[0])

    @property
    def n_tets(self):
        return int(self.tets.shape[0])

    @property
    def n_bfaces(self):
        return int(self.bfaces.shape[0])

    def volumes(self):
        """[T] fp64: the signed volume of every element from the stored vertices.  Positive by construction; with t_clamp = 0 it
        is exactly zero where a grid value equal to the level put an edge vertex on a grid point, and an element thinner than the
        fp32 rounding of its vertices (t within rounding of 0 or 1) can come out at that scale with either sign.  t_clamp > 0
        keeps every element clear of both."""
        v = self.verts.to(torch.float64)
        t = self.tets.long()
        a = v[t[:, 0]]
        return torch.einsum("ij,ij->i", v[t[:, 1]] - a, torch.linalg.cross(v[t[:, 2]] - a, v[t[:, 3]] - a)) / 6.0

    def volume(self):
        return float(self.volumes().sum())

    def boundary_surface(self):
        """The boundary triangles as a SurfaceMesh on the same vertex ids (components, watertightness, normals, volume)."""
        from .surface import SurfaceMesh
        return SurfaceMesh(self.verts, self.bfaces, self.device, _checked=self._indices_checked)

    def to(self, device):
        """The same mesh with every array on `device`."""
        m = TetMesh(*[None if t is None else t.to(device)
                      for t in (self.verts, self.tets, self.bfaces, self.bface_kind, self.vert_point, self.vert_class)])
        m._indices_checked = self._indices_checked
        return m

    def transformed(self, scale=1.0, shift=0.0):
        """A TetMesh with vertices verts * scale + shift (three values each, or one), in the vertices' dtype; scale > 0."""
        s = torch.tensor(_lib.triple(scale, "scale"), dtype=self.verts.dtype, device=self.device)
        d = torch.tensor(_lib.triple(shift, "shift"), dtype=self.verts.dtype, device=self.device)
        if not bool((s > 0).all()):
            raise ValueError("scale must be positive on every axis (a negative factor would turn the elements inside out)")
        m = TetMesh(self.verts * s + d, self.tets, self.bfaces, self.bface_kind, self.vert_point, self.vert_class)
        m._indices_checked = self._indices_checked
        return m

    def boundary_attributes(self, tolerance=3e-2):
        """[M] int32, the reference's rule (analysis/geometry.py:153-167) on this mesh's coordinates: 1 if the triangle's largest x
        lies below the tolerance, else 2 if its largest z lies above max(z) - tolerance, else 3."""
        if self.n_bfaces == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        corners = self.verts[self.bfaces.long()]                      # [M, 3 corners, 3]
        x_max, z_max = corners[:, :, 0].amax(1), corners[:, :, 2].amax(1)
        top = self.verts[:, 2].max() - tolerance
        three = torch.full_like(x_max, 3, dtype=torch.int32)
        return torch.where(x_max < tolerance, torch.ones_like(three), torch.where(z_max > top, 2 * torch.ones_like(three), three))

    @classmethod
    def read_mfem(cls, path):
        """(TetMesh on the host with fp64 vertices, attributes [M] int32) of an MFEM mesh v1.0 text file as write_mfem writes it:
        tetrahedra (geometry 4) and boundary triangles (geometry 2) only; anything else is a ValueError that names it.  bface_kind
        is not in the file and comes back 0."""
        with open(path) as fh:
            body = [ln.strip() for ln in fh.read().splitlines()]
        if not body or body[0] != "MFEM mesh v1.0":
            raise ValueError(f"{path}: not an 'MFEM mesh v1.0' file")
        body = [ln for ln in body[1:] if ln and not ln.startswith("#")]
        try:
            at = {name: body.index(name) for name in ("dimension", "elements", "boundary", "vertices")}
        except ValueError:
            raise ValueError(f"{path}: needs the sections dimension, elements, boundary and vertices") from None
        if body[at["dimension"] + 1] != "3":
            raise ValueError(f"{path}: dimension {body[at['dimension'] + 1]}, only 3 is read")

        def block(name, skip, cols, dtype, what):
            n = int(body[at[name] + 1])
            rows = body[at[name] + 1 + skip:at[name] + 1 + skip + n]
            arr = np.array([r.split() for r in rows] if n else np.empty((0, cols)), dtype=object)
            if len(rows) != n or arr.ndim != 2 or arr.shape[1] != cols:
                raise ValueError(f"{path}: the {name} section holds something else than {n} {what}")
            return arr.astype(dtype)
        el = block("elements", 1, 6, np.int64, "tetrahedra `attribute 4 v0 v1 v2 v3`")
        bd = block("boundary", 1, 5, np.int64, "triangles `attribute 2 v0 v1 v2`")
        if len(el) and not (el[:, 1] == 4).all():
            raise ValueError(f"{path}: element geometry {sorted(set(el[:, 1].tolist()) - {4})}, only tetrahedra (4) are read")
        if len(bd) and not (bd[:, 1] == 2).all():
            raise ValueError(f"{path}: boundary geometry {sorted(set(bd[:, 1].tolist()) - {2})}, only triangles (2) are read")
        if body[at["vertices"] + 2] != "3":
            raise ValueError(f"{path}: vertices of dimension {body[at['vertices'] + 2]} (a nodes grid function is not read), only 3 is")
        vx = block("vertices", 2, 3, np.float64, "vertices of 3 coordinates")
        m = cls(vx, el[:, 2:].astype(np.int32), bd[:, 2:].astype(np.int32), np.zeros(len(bd), dtype=np.int8))
        return m, torch.from_numpy(bd[:, 0].astype(np.int32))

    def write_mfem(self, path, attributes=None):
        """MFEM mesh v1.0 text: elements `1 4 v0 v1 v2 v3` (attribute 1, geometry 4 = tetrahedron), boundary `attr 2 v0 v1 v2`
        (geometry 2 = triangle; attributes [M], default boundary_attributes()), vertices with the shortest digits that read back as
        the stored fp32 values (fp64 vertices are written with fp64 digits).  Needs no device."""
        attr = self.boundary_attributes() if attributes is None else attributes
        attr = (attr.detach().cpu().numpy() if torch.is_tensor(attr) else np.asarray(attr)).astype(np.int64).reshape(-1)
        if attr.shape[0] != self.n_bfaces:
            raise ValueError(f"attributes must have {self.n_bfaces} entries, got {attr.shape[0]}")
        v = self.verts.detach().cpu().numpy()
        t = self.tets.detach().cpu().numpy().astype(np.int64)
        f = self.bfaces.detach().cpu().numpy().astype(np.int64)

        def rows(cols):                                               # one line per row, columns joined by blanks: no Python loop
            out = cols[0]
            for c in cols[1:]:
                out = np.char.add(np.char.add(out, " "), c)
            return "\n".join(out.tolist())

        el = rows([np.full(len(t), "1 4")] + [t[:, k].astype(np.str_) for k in range(4)]) if len(t) else ""
        bd = rows([attr.astype(np.str_), np.full(len(f), "2")] + [f[:, k].astype(np.str_) for k in range(3)]) if len(f) else ""
        vx = rows([v[:, k].astype(np.str_) for k in range(3)]) if len(v) else ""     # numpy's str of a float scalar: repr digits
        with open(path, "w") as fh:
            fh.write("MFEM mesh v1.0\n\ndimension\n3\n\n")
            fh.write(f"elements\n{len(t)}\n{el}\n\n" if len(t) else "elements\n0\n\n")
            fh.write(f"boundary\n{len(f)}\n{bd}\n\n" if len(f) else "boundary\n0\n\n")
            fh.write(f"vertices\n{len(v)}\n3\n{vx}\n" if len(v) else "vertices\n0\n3\n")
