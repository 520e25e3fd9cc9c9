"""The surface stage of the reference's ``analysis/geometry.py: DeepSDFMesh`` on the GPU.

The reference hands the mesh of ``create_mesh_microstructure_diff`` to trimesh on the CPU: face adjacency, the largest connected
component ("remove orphans"), the watertightness test, degenerate faces, vertex normals, and from those the normal-projected shape
derivative.  Here all of it comes from the kernels of csrc/meshtopo.hpp (include/dsdf.h ``dsdf_mt_*``); the sorts they consume are
``torch.sort(stable=True)`` / ``torch.searchsorted`` on the device.

    SurfaceMesh(verts, faces)        a device-resident triangle mesh; every derived quantity is computed once and cached
    SurfaceMesh.from_diff(d, stretch)  wraps a MicrostructureMeshDiff: vertex ids stay those of its Jacobian

``keep_largest_component`` and ``drop_degenerate_faces`` return a new SurfaceMesh with the SAME vertex array and a subset of the faces
in their original order, so a vertex id means the same thing before and after; vertices no face refers to get a zero normal and a
zero gradient.  There is no CPU path."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import mesh as _mesh

INT32_MAX = 2 ** 31 - 1
MAX_FACES = INT32_MAX // 3
STATS = ("edges", "boundary", "nonmanifold", "paired", "same_direction", "degenerate_halfedges")


class SurfaceMesh:
    def __init__(self, verts, faces, device=None, _checked=False):
        if device is None:
            device = next((t.device for t in (verts, faces) if torch.is_tensor(t) and t.device.type == "cuda"), "cuda")
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DsdfError("SurfaceMesh needs a HIP device (no CPU fallback)")
        V = verts.detach() if torch.is_tensor(verts) else torch.from_numpy(np.asarray(verts, dtype=np.float64))
        F = faces.detach() if torch.is_tensor(faces) else torch.from_numpy(np.array(faces))          # a copy: the array may be read-only
        if V.dim() != 2 or V.shape[1] != 3 or V.shape[0] < 1:
            raise ValueError(f"verts must have shape [n >= 1, 3], got {tuple(V.shape)}")
        if F.dim() != 2 or F.shape[1] != 3:
            raise ValueError(f"faces must have shape [m, 3], got {tuple(F.shape)}")
        if F.is_floating_point() or F.is_complex() or F.dtype == torch.bool:
            raise ValueError(f"faces must hold integers, got {F.dtype}")
        if V.shape[0] > INT32_MAX or F.shape[0] > MAX_FACES:
            raise ValueError(f"at most {INT32_MAX} vertices and {MAX_FACES} faces")
        self.device = device
        self.V = V.to(device=device, dtype=torch.float32).contiguous()
        Fd = F.to(device=device)
        if not _checked and F.shape[0] > 0:
            lo, hi = torch.aminmax(Fd.reshape(-1).to(torch.int64))
            lo, hi, fin = torch.stack([lo, hi, torch.isfinite(self.V).all().to(torch.int64)]).tolist()
            if not fin:
                raise ValueError("verts must be finite (after conversion to fp32)")
            if lo < 0 or hi >= V.shape[0]:
                raise ValueError(f"face indices must lie in [0, {V.shape[0]}), found [{lo}, {hi}]")
        self.F = Fd.to(torch.int32).contiguous()
        self.n_verts, self.n_faces = int(V.shape[0]), int(F.shape[0])
        self.diff, self.stretch = None, (1.0, 1.0, 1.0)
        self.component_rounds = None       # rounds the last component pass took (diagnostics)
        self._cache = {}

    @classmethod
    def from_diff(cls, d, stretch=(1, 1, 1)):
        """The mesh of a MicrostructureMeshDiff with vertex coordinate a multiplied by stretch[a] (the reference stretches x by 2);
        volume_gradient, shape_derivative and dtheta then carry the same factor into the derivative."""
        stretch = tuple(float(s) for s in stretch)
        if len(stretch) != 3 or not all(np.isfinite(stretch)):
            raise ValueError(f"stretch must be three finite factors, got {stretch}")
        verts = d.verts * torch.tensor(stretch, dtype=d.verts.dtype, device=d.verts.device)
        m = cls(verts, d.faces, d.device)
        m.diff, m.stretch = d, stretch
        return m

    @property
    def vertices(self):
        return self.V

    @property
    def faces(self):
        return self.F

    def _subset(self, keep):
        m = SurfaceMesh(self.V, self.F[keep], self.device, _checked=True)
        m.diff, m.stretch = self.diff, self.stretch
        return m

    def _ws(self):
        nb = C.c_size_t()
        _lib.check(_lib.lib().dsdf_mt_plan(self.n_verts, self.n_faces, C.byref(nb)))
        return torch.empty(max(nb.value, 256), dtype=torch.uint8, device=self.device)

    # ---- topology -------------------------------------------------------------------------------------------------------------
    def _adjacency(self):
        """(mate [3F] int32, stats [6] int64 on the host)."""
        if "adj" not in self._cache:
            nf = self.n_faces
            with torch.cuda.device(self.device):
                mate = torch.empty(3 * nf, dtype=torch.int32, device=self.device)
                stats = torch.zeros(len(STATS), dtype=torch.int64, device=self.device)
                if nf:
                    lib = _lib.lib()
                    keys = torch.empty(3 * nf, dtype=torch.int64, device=self.device)
                    _lib.check(lib.dsdf_mt_edge_keys(_lib.ptr(self.F), nf, self.n_verts, _lib.ptr(keys), _lib.stream()))
                    skeys, order = torch.sort(keys, stable=True)
                    ws = self._ws()
                    _lib.check(lib.dsdf_mt_adjacency(_lib.ptr(self.F), nf, _lib.ptr(skeys), _lib.ptr(order), _lib.ptr(mate), _lib.ptr(stats), _lib.ptr(ws),
                                                     ws.numel(), _lib.stream()))
            self._cache["adj"] = (mate, stats.tolist())
        return self._cache["adj"]

    def half_edge_mates(self):
        """mate [3F] int32: the other half-edge of every edge shared by exactly two faces, -1 elsewhere (half-edge 3 f + k runs
        faces[f][k] -> faces[f][(k + 1) % 3])."""
        return self._adjacency()[0]

    def edge_stats(self):
        """{edges, boundary, nonmanifold, paired, same_direction, degenerate_halfedges}: counts of distinct edges, edges of one
        face, edges of more than two, edges of exactly two, those of the latter whose half-edges run the same way, and half-edges
        whose two ends are one vertex."""
        return dict(zip(STATS, self._adjacency()[1]))

    @property
    def is_watertight(self):
        s = self.edge_stats()
        return self.n_faces > 0 and s["boundary"] == 0 and s["nonmanifold"] == 0 and s["degenerate_halfedges"] == 0

    @property
    def is_winding_consistent(self):
        return self.is_watertight and self.edge_stats()["same_direction"] == 0

    def _components(self):
        if "cc" not in self._cache:
            nf = self.n_faces
            with torch.cuda.device(self.device):
                label = torch.empty(nf, dtype=torch.int32, device=self.device)
                size = torch.empty(nf, dtype=torch.int32, device=self.device)
                rounds = C.c_int32(0)
                if nf:
                    mate = self.half_edge_mates()
                    ws = self._ws()
                    _lib.check(_lib.lib().dsdf_mt_components(_lib.ptr(mate), nf, _lib.ptr(label), _lib.ptr(size), C.byref(rounds), _lib.ptr(ws), ws.numel(),
                                                             _lib.stream()))
            self.component_rounds = rounds.value
            self._cache["cc"] = (label, size)
        return self._cache["cc"]

    def face_labels(self):
        """label [F] int32: the lowest face index of the face's component (faces joined across edges of exactly two faces)."""
        return self._components()[0]

    def component_sizes(self):
        """size [F] int32: at the lowest face of every component its face count, 0 elsewhere."""
        return self._components()[1]

    @property
    def n_components(self):
        if "ncc" not in self._cache:
            self._cache["ncc"] = int((self.component_sizes() > 0).sum()) if self.n_faces else 0
        return self._cache["ncc"]

    def keep_largest_component(self):
        """The faces of the component with the most faces (ties: the lowest label), as a new SurfaceMesh on the same vertices."""
        if self.n_faces == 0:
            return self
        label, size = self._components()
        root = int((size == size.max()).nonzero()[0])          # nonzero() lists indices in ascending order
        return self._subset(label == root)

    def degenerate_faces(self):
        """mask [F] bool: faces with a repeated index or of zero area (the mesh SDF's rule)."""
        if "deg" not in self._cache:
            with torch.cuda.device(self.device):
                out = torch.zeros(self.n_faces, dtype=torch.uint8, device=self.device)
                if self.n_faces:
                    _lib.check(_lib.lib().dsdf_mt_face_degenerate(_lib.ptr(self.V), self.n_verts, _lib.ptr(self.F), self.n_faces, _lib.ptr(out), _lib.stream()))
            self._cache["deg"] = out.bool()
        return self._cache["deg"]

    def drop_degenerate_faces(self):
        return self._subset(~self.degenerate_faces())

    # ---- geometry -------------------------------------------------------------------------------------------------------------
    def _vertex_geometry(self):
        if "vg" not in self._cache:
            with torch.cuda.device(self.device):
                corners, order = torch.sort(self.F.reshape(-1).to(torch.int64), stable=True)
                vstart = torch.searchsorted(corners, torch.arange(self.n_verts + 1, dtype=torch.int64, device=self.device))
                normals = torch.empty(self.n_verts, 3, dtype=torch.float32, device=self.device)
                grad = torch.empty(self.n_verts, 3, dtype=torch.float32, device=self.device)
                _lib.check(_lib.lib().dsdf_mt_vertex_geometry(_lib.ptr(self.V), self.n_verts, _lib.ptr(self.F), self.n_faces, _lib.ptr(order), _lib.ptr(vstart),
                                                              _lib.ptr(normals), _lib.ptr(grad), _lib.stream()))
            self._cache["vg"] = (normals, grad)
        return self._cache["vg"]

    def vertex_normals(self):
        """[V, 3] fp32: the angle-weighted mean of the face normals around every vertex (current trimesh's vertex_normals), unit
        length, or exactly zero for a vertex without a face of non-zero area."""
        return self._vertex_geometry()[0]

    def volume_vertex_gradient(self):
        """[V, 3] fp32: d volume / d vertex = (1 / 6) sum over the vertex's corners (a, b, c) of b x c."""
        return self._vertex_geometry()[1]

    def volume(self):
        """The enclosed volume (1 / 6) sum a . (b x c) (divergence theorem; meaningful for a closed, consistently wound mesh),
        summed in fp64 on the device."""
        if "vol" not in self._cache:
            vol = torch.zeros(1, dtype=torch.float64, device=self.device)
            if self.n_faces:
                with torch.cuda.device(self.device):
                    ws = self._ws()
                    _lib.check(_lib.lib().dsdf_mt_volume(_lib.ptr(self.V), self.n_verts, _lib.ptr(self.F), self.n_faces, _lib.ptr(vol), _lib.ptr(ws), ws.numel(),
                                                         _lib.stream()))
            self._cache["vol"] = float(vol)
        return self._cache["vol"]

    # ---- derivatives with respect to the control points (a MicrostructureMeshDiff attached) --------------------------------------------
    def _need_diff(self):
        if self.diff is None:
            raise ValueError("this SurfaceMesh carries no derivative: build it with SurfaceMesh.from_diff")
        return self.diff

    def _stretch_t(self):
        return torch.tensor(self.stretch, dtype=torch.float32, device=self.device)

    def volume_gradient(self):
        """d volume / d control points [ncp, L]: the adjoint of the mesh derivative applied to stretch * volume_vertex_gradient; the
        dense Jacobian is never built."""
        return self._need_diff().vjp(self.volume_vertex_gradient() * self._stretch_t())

    def shape_derivative(self, grad_verts):
        """grad_verts [V, 3] -> [ncp, L]: the adjoint of dtheta(clip=0), i.e. the vjp of stretch * n (n . g).  This path has NO
        outlier clipping: the reference's rule zeroes single entries of the dense Jacobian, which the adjoint never forms."""
        d = self._need_diff()
        g = torch.as_tensor(grad_verts).to(self.device, torch.float32)
        if g.shape != (self.n_verts, 3):
            raise ValueError(f"grad_verts must be [{self.n_verts}, 3], got {tuple(g.shape)}")
        n = self.vertex_normals()
        return d.vjp(n * (n * g).sum(1, keepdim=True) * self._stretch_t())

    def dtheta(self, clip=1.0):
        """The reference's get_dTheta on the surface: [V, 3, ncp * L] fp32, every column of the (stretched, clipped) Jacobian
        projected onto the vertex normal.  clip > 0 zeroes entries with |entry| > clip after the stretch (the reference's outlier
        rule); clip = 0 keeps everything.  Raises MemoryError, stating the size, when the array would not fit the device."""
        d = self._need_diff()
        V, R = self.n_verts, d.n_control_points * d.latent_size
        need = 4 * V * 3 * R
        free = _mesh._free_device_memory(self.device)
        if need + 4 * V * R > free:
            raise MemoryError(f"dtheta [{V}, 3, {R}] fp32 takes {need} bytes ({need / 2 ** 30:.2f} GiB) besides the Jacobian's "
                              f"{4 * V * R}, the device has {free} bytes free: use shape_derivative / volume_gradient, or a coarser grid")
        jac, axis = d.jacobian()
        with torch.cuda.device(self.device):
            out = torch.empty(V, 3, R, dtype=torch.float32, device=self.device)
            st = (C.c_float * 3)(*self.stretch)
            _lib.check(_lib.lib().dsdf_mt_project(_lib.ptr(jac), _lib.ptr(axis), _lib.ptr(self.vertex_normals()), V, R, st, float(clip), _lib.ptr(out), _lib.stream()))
        return out
