"""Signed distance from points to a triangle mesh on the GPU, and the mesh readers that feed it.

The reference's ``SDFfromMesh`` (sdf_sampler/sdf_sampler.py:201-242) takes its distance from ``igl.point_mesh_squared_distance``
and its sign from an embree ray test (``contains_points``: inside is negative).  Here both come from one HIP kernel
(csrc/meshsdf.hpp, include/dsdf.h ``dsdf_msdf_*``): the exact distance to the closest triangle, brute force over every face,
and the generalized winding number, whose parity (``floor(|w| + 0.5)`` odd) is the inside test.

    read_mesh                     PLY (ascii, binary either endianness) and OBJ -> (V float64 [n, 3], F int64 [m, 3])
    read_points                   the vertices of a PLY / OBJ file, faces or none (SurfaceSamples files) -> float64 [n, 3]
    TriangleMesh                  validates and uploads a mesh once, then answers .sdf / .squared_distance / .winding_number,
                                  and draws area-weighted surface samples (.sample_surface, .area; csrc/pointset.hpp)
    point_mesh_squared_distance   igl's argument order and return shapes (sqrD [n], I [n], C [n, 3])
    winding_number                igl's argument order (V, F, O) -> w [n]

numpy in gives numpy out (fp32 values, int32 face ids); a torch tensor gives tensors on the mesh's device.  There is no CPU path.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib

INT32_MAX = 2 ** 31 - 1


# ---- readers ----------------------------------------------------------------------------------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _fan(polys):
    """Fan triangulation of index lists: (p0, p[j], p[j + 1]) for j = 1 .. len - 2."""
    tris = [(p[0], p[j], p[j + 1]) for p in polys for j in range(1, len(p) - 1)]
    return np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def _ply_header(fh):
    if fh.readline().strip() != b"ply":
        raise ValueError("not a PLY file (first line is not 'ply')")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("PLY header has no end_header")
        tok = line.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "end_header":
            break
        if tok[0] == "format":
            if len(tok) < 2 or tok[1] not in ("ascii", "binary_little_endian", "binary_big_endian"):
                raise ValueError(f"unsupported PLY format line: {line!r}")
            fmt = tok[1]
        elif tok[0] == "element":
            if len(tok) != 3 or not tok[2].isdigit():
                raise ValueError(f"bad PLY element line: {line!r}")
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == "property":
            if not elements:
                raise ValueError("PLY property before any element")
            if len(tok) == 5 and tok[1] == "list" and tok[2] in _PLY_TYPES and tok[3] in _PLY_TYPES:
                elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
            elif len(tok) == 3 and tok[1] in _PLY_TYPES:
                elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
            else:
                raise ValueError(f"bad PLY property line: {line!r}")
        else:
            raise ValueError(f"unexpected PLY header line: {line!r}")
    if fmt is None:
        raise ValueError("PLY header has no format line")
    return fmt, elements


def _ply_binary_element(buf, pos, count, props, endian):
    """Rows of one binary element -> ({name: array or list of index arrays}, new position)."""
    if all(p[2] is None for p in props):               # fixed layout: one structured read
        dt = np.dtype([(n, endian + t) for n, t, _ in props])
        if pos + dt.itemsize * count > len(buf):
            raise ValueError("PLY data is truncated")
        rows = np.frombuffer(buf, dt, count, pos)
        return {n: rows[n] for n, _, _ in props}, pos + dt.itemsize * count
    # every list of the first row has the length of all rows (triangles): try that layout first, then fall back to row by row
    try:
        fields, p = [], pos
        for n, t, it in props:
            if it is None:
                fields.append((n, endian + t))
                p += np.dtype(t).itemsize
            else:
                k = int(np.frombuffer(buf, endian + t, 1, p)[0])
                fields.append((n + "#n", endian + t))
                fields.append((n, endian + it, (k,)))
                p += np.dtype(t).itemsize + k * np.dtype(it).itemsize
        dt = np.dtype(fields)
        if count and pos + dt.itemsize * count <= len(buf):
            rows = np.frombuffer(buf, dt, count, pos)
            if all(np.all(rows[n + "#n"] == dt[n].shape[0]) for n, _, it in props if it is not None):
                out = {n: rows[n] for n, _, _ in props}
                return out, pos + dt.itemsize * count
    except (IndexError, ValueError):
        pass
    out = {n: [] for n, _, _ in props}
    for _ in range(count):
        for n, t, it in props:
            ts = np.dtype(t).itemsize
            if pos + ts > len(buf):
                raise ValueError("PLY data is truncated")
            v = np.frombuffer(buf, endian + t, 1, pos)[0]
            pos += ts
            if it is not None:
                k = int(v)
                if k < 0 or pos + k * np.dtype(it).itemsize > len(buf):
                    raise ValueError("PLY data is truncated")
                v = np.frombuffer(buf, endian + it, k, pos)
                pos += k * np.dtype(it).itemsize
            out[n].append(v)
    return out, pos


def _read_ply(path):
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh)
        body = fh.read()
    data = {}
    if fmt == "ascii":
        lines = iter(body.decode("ascii", "replace").splitlines())
        for name, count, props in elements:
            out = {n: [] for n, _, _ in props}
            for _ in range(count):
                tok = next((ln.split() for ln in lines if ln.strip()), None)
                if tok is None:
                    raise ValueError(f"PLY data is truncated in element {name!r}")
                i = 0
                try:
                    for n, t, it in props:
                        if it is None:
                            out[n].append(float(tok[i]))
                            i += 1
                        else:
                            k = int(tok[i])
                            out[n].append([int(x) for x in tok[i + 1:i + 1 + k]])
                            if len(out[n][-1]) != k:
                                raise ValueError
                            i += 1 + k
                except (IndexError, ValueError):
                    raise ValueError(f"malformed PLY row in element {name!r}: {' '.join(tok)!r}") from None
            data[name] = out
    else:
        endian = "<" if fmt == "binary_little_endian" else ">"
        pos = 0
        for name, count, props in elements:
            data[name], pos = _ply_binary_element(body, pos, count, props, endian)
    if "vertex" not in data or not all(a in data["vertex"] for a in "xyz"):
        raise ValueError("PLY file has no vertex element with x, y, z")
    V = np.stack([np.asarray(data["vertex"][a], dtype=np.float64) for a in "xyz"], axis=1).reshape(-1, 3)
    F = np.zeros((0, 3), np.int64)
    face = data.get("face")
    if face is not None:
        key = "vertex_indices" if "vertex_indices" in face else ("vertex_index" if "vertex_index" in face else None)
        if key is None:
            raise ValueError("PLY face element has no vertex_indices / vertex_index list")
        lists = face[key]
        if isinstance(lists, np.ndarray) and lists.ndim == 2 and lists.shape[1] == 3:
            F = lists.astype(np.int64)
        else:
            F = _fan([list(map(int, p)) for p in lists])
    return V, F


def _read_obj(path):
    verts, polys = [], []
    with open(path, "r", errors="replace") as fh:
        for ln, line in enumerate(fh, 1):
            tok = line.split()
            if not tok:
                continue
            try:
                if tok[0] == "v":
                    verts.append([float(x) for x in tok[1:4]])
                    if len(verts[-1]) != 3:
                        raise ValueError
                elif tok[0] == "f":
                    idx = []
                    for t in tok[1:]:
                        i = int(t.split("/")[0])
                        if i == 0:
                            raise ValueError
                        idx.append(i - 1 if i > 0 else len(verts) + i)
                    if len(idx) < 3:
                        raise ValueError
                    polys.append(idx)
            except ValueError:
                raise ValueError(f"{path}:{ln}: malformed OBJ line {line.strip()!r}") from None
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), _fan(polys)


def read_mesh(path):
    """(V float64 [n, 3], F int64 [m, 3]) of a .ply or .obj file; polygons are fan-triangulated.  ValueError on malformed input
    or face indices outside [0, n)."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".ply":
        V, F = _read_ply(path)
    elif ext == ".obj":
        V, F = _read_obj(path)
    else:
        raise ValueError(f"read_mesh: unsupported mesh file {path!r} (.ply or .obj)")
    if F.size and (F.min() < 0 or F.max() >= len(V)):
        raise ValueError(f"{path}: face index outside [0, {len(V)})")
    return V, F


def read_points(path):
    """Vertices float64 [n, 3] of a .ply or .obj file; a face element is read and ignored, a vertex-only PLY is fine."""
    return read_mesh(path)[0]


# ---- device API -------------------------------------------------------------------------------------------------------------
def _as_host_or_device(x, what, device, cols=3, dtype=torch.float32):
    """(tensor on `device`, returns_numpy, return device)."""
    if torch.is_tensor(x):
        t, numpy_out, out_dev = x.detach(), False, x.device
    else:
        t, numpy_out, out_dev = torch.from_numpy(np.ascontiguousarray(np.asarray(x))), True, None
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{what} must have shape [n, {cols}], got {tuple(t.shape)}")
    return t.to(device=device, dtype=dtype).contiguous(), numpy_out, out_dev


class TriangleMesh:
    """A triangle mesh resident on a HIP device, prepared once (dsdf_msdf_prepare) for any number of queries."""

    def __init__(self, vertices, faces, device=None):
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise _lib.DsdfError("TriangleMesh needs a HIP device (no CPU fallback)")
        V = vertices.detach() if torch.is_tensor(vertices) else torch.from_numpy(np.asarray(vertices, dtype=np.float64))
        F = faces.detach() if torch.is_tensor(faces) else torch.from_numpy(np.asarray(faces))
        if V.dim() != 2 or V.shape[1] != 3 or V.shape[0] < 1:
            raise ValueError(f"vertices must have shape [n >= 1, 3], got {tuple(V.shape)}")
        if F.dim() != 2 or F.shape[1] != 3 or F.shape[0] < 1:
            raise ValueError(f"faces must have shape [m >= 1, 3], got {tuple(F.shape)}")
        if F.is_floating_point() or F.is_complex() or F.dtype == torch.bool:
            raise ValueError(f"faces must hold integers, got {F.dtype}")
        if V.shape[0] > INT32_MAX or F.shape[0] > INT32_MAX:
            raise ValueError("meshes beyond 2^31 - 1 vertices or faces are not supported")
        self.device = device
        self.V = V.to(device=device, dtype=torch.float32).contiguous()
        Fd = F.to(device=device)
        # one reduction (one host sync) checks finiteness and the index range together
        lo, hi = torch.aminmax(Fd.reshape(-1).to(torch.int64))
        fin = torch.isfinite(self.V).all()
        lo, hi, fin = torch.stack([lo, hi, fin.to(torch.int64)]).tolist()
        if not fin:
            raise ValueError("vertices must be finite (after conversion to fp32)")
        if lo < 0 or hi >= V.shape[0]:
            raise ValueError(f"face indices must lie in [0, {V.shape[0]}), found [{lo}, {hi}]")
        self.F = Fd.to(torch.int32).contiguous()
        self.n_faces = int(F.shape[0])
        lib = _lib.lib()
        tb = C.c_size_t()
        _lib.check(lib.dsdf_msdf_plan(self.n_faces, 0, C.byref(tb), None, None))
        with torch.cuda.device(device):
            self.tri = torch.empty(tb.value, dtype=torch.uint8, device=device)
            _lib.check(lib.dsdf_msdf_prepare(_lib.ptr(self.V), self.V.shape[0], _lib.ptr(self.F), self.n_faces, _lib.ptr(self.tri),
                                             self.tri.numel(), _lib.stream()))
        self._surf = None              # (buffer, total area, area offset): dsdf_surf_prepare, on first use

    @property
    def vertices(self):
        return self.V

    @property
    def faces(self):
        return self.F

    def plan(self, n_queries):
        """(workspace bytes, face splits) of a query of n_queries points (dsdf_msdf_plan)."""
        wb, ns = C.c_size_t(), C.c_int32()
        _lib.check(_lib.lib().dsdf_msdf_plan(self.n_faces, int(n_queries), None, C.byref(wb), C.byref(ns)))
        return wb.value, ns.value

    def _query(self, q, sdf=False, dist=False, wind=False, flip_sign=False):
        Q, numpy_out, out_dev = _as_host_or_device(q, "queries", self.device)
        nq = Q.shape[0]
        if nq > INT32_MAX:
            raise ValueError("at most 2^31 - 1 queries per call")
        kw = dict(dtype=torch.float32, device=self.device)
        out = {}
        with torch.cuda.device(self.device):
            if sdf:
                out["sdf"] = torch.empty(nq, **kw)
            if dist:
                out["d2"] = torch.empty(nq, **kw)
                out["face"] = torch.empty(nq, dtype=torch.int32, device=self.device)
                out["closest"] = torch.empty(nq, 3, **kw)
            if wind:
                out["w"] = torch.empty(nq, **kw)
            if nq:
                wb, _ = self.plan(nq)
                ws = torch.empty(max(wb, 1), dtype=torch.uint8, device=self.device)
                _lib.check(_lib.lib().dsdf_msdf_query(
                    _lib.ptr(self.tri), self.n_faces, _lib.ptr(Q), nq, _lib.ptr(out.get("sdf")), _lib.ptr(out.get("d2")), _lib.ptr(out.get("face")),
                    _lib.ptr(out.get("closest")), _lib.ptr(out.get("w")), int(bool(flip_sign)), _lib.ptr(ws), ws.numel(), _lib.stream()))
        if numpy_out:
            return {k: v.cpu().numpy() for k, v in out.items()}
        return {k: v.to(out_dev) for k, v in out.items()}

    def sdf(self, queries, flip_sign=False):
        """Signed distance [n] (negative inside; flip_sign negates)."""
        return self._query(queries, sdf=True, flip_sign=flip_sign)["sdf"]

    def squared_distance(self, queries):
        """(sqrD [n], I [n] closest face, C [n, 3] closest point) -- igl.point_mesh_squared_distance's outputs."""
        o = self._query(queries, dist=True)
        return o["d2"], o["face"], o["closest"]

    def winding_number(self, queries):
        """Generalized winding number [n]: sum of solid angles / 4 pi."""
        return self._query(queries, wind=True)["w"]

    # ---- surface samples (dsdf_surf_*) ----
    def _surface(self):
        if self._surf is None:
            lib = _lib.lib()
            sb, ao, total = C.c_size_t(), C.c_size_t(), C.c_double()
            _lib.check(lib.dsdf_surf_plan(self.n_faces, C.byref(sb), C.byref(ao), None))
            with torch.cuda.device(self.device):
                buf = torch.empty(sb.value, dtype=torch.uint8, device=self.device)
                rc = lib.dsdf_surf_prepare(_lib.ptr(self.V), self.V.shape[0], _lib.ptr(self.F), self.n_faces, _lib.ptr(buf), buf.numel(),
                                           C.byref(total), _lib.stream())
            if rc != 0 and total.value == 0.0:
                raise ValueError("the mesh has no surface area: nothing to sample")
            _lib.check(rc)
            self._surf = (buf, total.value, ao.value)
        return self._surf

    def area(self):
        """Total surface area: the fp64 sum of the fp32 face areas."""
        return self._surface()[1]

    def face_areas(self):
        """(area fp32 [m], cdf fp64 [m]) as the sampler uses them: per-face areas and their inclusive prefix sums."""
        buf, _, ao = self._surface()
        return buf[ao:ao + 4 * self.n_faces].view(torch.float32), buf[:8 * self.n_faces].view(torch.float64)

    def sample_surface(self, count, seed=0, std=0.0, return_bary=False, offset=0):
        """count points drawn uniformly from the surface: (points fp32 [count, 3], face int32 [count]) and, with return_bary,
        bary fp32 [count, 2] (p = a + u ab + v ac), as tensors on the mesh's device.  Sample i depends on (seed, offset + i)
        only, so draws at consecutive offsets continue one another.  std > 0 adds N(0, std^2) noise per coordinate."""
        count, seed, offset = int(count), int(seed), int(offset)
        if count < 0 or count > INT32_MAX:
            raise ValueError("count must lie in [0, 2^31 - 1]")
        if not 0 <= seed < 2 ** 64 or not 0 <= offset <= 2 ** 64 - 1 - count:
            raise ValueError("seed and offset must be unsigned 64-bit integers")
        if not (std >= 0.0 and np.isfinite(std)):
            raise ValueError("std must be finite and >= 0")
        buf, _, _ = self._surface()
        with torch.cuda.device(self.device):
            pts = torch.empty(count, 3, dtype=torch.float32, device=self.device)
            face = torch.empty(count, dtype=torch.int32, device=self.device)
            bary = torch.empty(count, 2, dtype=torch.float32, device=self.device) if return_bary else None
            _lib.check(_lib.lib().dsdf_surf_sample(_lib.ptr(self.V), self.V.shape[0], _lib.ptr(self.F), self.n_faces, _lib.ptr(buf), buf.numel(),
                                                   count, offset, seed, float(std), _lib.ptr(pts), _lib.ptr(face), _lib.ptr(bary), _lib.stream()))
        return (pts, face, bary) if return_bary else (pts, face)


def _mesh_device(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.device.type == "cuda":
            return x.device
    return None


def point_mesh_squared_distance(P, V, F):
    """igl.point_mesh_squared_distance(P, V, F) -> (sqrD [n], I [n], C [n, 3]), on the GPU."""
    return TriangleMesh(V, F, _mesh_device(P, V, F)).squared_distance(P)


def winding_number(V, F, O):
    """igl.winding_number(V, F, O) -> w [n], on the GPU."""
    return TriangleMesh(V, F, _mesh_device(O, V, F)).winding_number(O)
