"""Trivariate tensor-product B-spline fields of latent codes: what the reference takes from splinepy for
create_mesh_microstructure / sdf_struct (``latent_vec_interpolation``), reduced to what those functions use.

The spline lives on the host in fp64 (knots, control points: refinement is exact there); evaluation is on the GPU in fp32 through
the row kernel of csrc/msgrid.hpp (dsdf_ms_rows, point-list mode), from a device copy made on first use and dropped when the
control points are assigned.  Control points are [ncp, L] with the first parametric axis fastest (i + j * nx + k * nx * ny:
splinepy's order).  There is no CPU evaluation."""
import ctypes as C

import numpy as np
import torch

from . import _lib

MAX_DEGREE = 3


class BSplineField:
    def __init__(self, degrees, knot_vectors, control_points):
        degrees = [int(d) for d in degrees]
        if len(degrees) != 3:
            raise ValueError(f"BSplineField is trivariate: 3 degrees, got {len(degrees)}")
        if any(d < 1 or d > MAX_DEGREE for d in degrees):
            raise ValueError(f"degrees must be 1 .. {MAX_DEGREE}, got {degrees}")
        if len(knot_vectors) != 3:
            raise ValueError(f"3 knot vectors, got {len(knot_vectors)}")
        knots = [np.array([float(u) for u in kv], dtype=np.float64) for kv in knot_vectors]
        for a, (p, U) in enumerate(zip(degrees, knots)):
            if U.ndim != 1 or U.size < 2 * (p + 1):
                raise ValueError(f"knot vector {a} needs at least {2 * (p + 1)} entries for degree {p}, got {U.size}")
            if not np.all(np.isfinite(U)) or np.any(np.diff(U) < 0):
                raise ValueError(f"knot vector {a} must be finite and non-decreasing")
            if not U[p] < U[U.size - p - 1]:
                raise ValueError(f"knot vector {a} has an empty range")
        self._degrees = degrees
        self._knots = knots
        self._dev = {}
        self.control_points = control_points

    # ---- what the reference reads from a splinepy BSpline -----------------------------------------------------------------
    @property
    def degrees(self):
        return np.array(self._degrees)

    @property
    def knot_vectors(self):
        return [U.copy() for U in self._knots]

    @property
    def control_mesh_resolutions(self):
        return np.array([U.size - p - 1 for p, U in zip(self._degrees, self._knots)])

    @property
    def control_points(self):
        return self._cp

    @control_points.setter
    def control_points(self, value):
        cp = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
        cp = np.array(cp, dtype=np.float64)
        if cp.ndim == 1:
            cp = cp[:, None]
        ncp = int(np.prod(self.control_mesh_resolutions))
        if cp.ndim != 2 or cp.shape[0] != ncp or cp.shape[1] < 1:
            raise ValueError(f"control points must be [{ncp}, L] for {list(self.control_mesh_resolutions)} per axis, "
                             f"got {tuple(cp.shape)}")
        self._cp = cp
        self._dev = {}

    @property
    def latent_size(self):
        return self._cp.shape[1]

    # ---- device side ------------------------------------------------------------------------------------------------------
    def c_spline(self, device):
        """(DsdfMsSpline, keep-alive) for `device`: the struct points into host and device buffers owned by this object."""
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DsdfError("BSplineField evaluates on a HIP device (no CPU fallback)")
        key = str(device if device.index is not None else torch.device("cuda", torch.cuda.current_device()))
        st = self._dev.get(key)
        if st is None:
            host = [np.ascontiguousarray(U, dtype=np.float32) for U in self._knots]
            kd = torch.from_numpy(np.concatenate(host)).to(device)
            cp = torch.from_numpy(np.ascontiguousarray(self._cp, dtype=np.float32)).to(device)
            s = _lib.DsdfMsSpline()
            res = self.control_mesh_resolutions
            for a in range(3):
                s.degree[a], s.n_cp[a], s.n_knots[a] = self._degrees[a], int(res[a]), host[a].size
                s.knots_host[a] = host[a].ctypes.data_as(C.POINTER(C.c_float))
            s.knots_dev, s.cp, s.ncp, s.L = kd.data_ptr(), cp.data_ptr(), cp.shape[0], cp.shape[1]
            st = self._dev[key] = (s, (host, kd, cp))
        return st

    def evaluate(self, points):
        """Spline values [n, L] at points [n, 3] (clamped to the knot range), computed on the GPU.  A tensor gives a tensor on
        its device (the current HIP device for a host tensor), anything else a numpy array."""
        as_numpy = not torch.is_tensor(points)
        pts = torch.as_tensor(np.asarray(points, dtype=np.float32)) if as_numpy else points
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"points must be [n, 3], got {tuple(pts.shape)}")
        if pts.device.type != "cuda":
            pts = pts.to("cuda")
        pts = pts.detach().to(torch.float32).contiguous()
        from .mesh import ms_point_rows
        out = ms_point_rows(self, [1, 1, 1], pts, inside_test=False, with_xyz=False)
        return out.cpu().numpy() if as_numpy else out

    # ---- refinement (host, fp64) ----------------------------------------------------------------------------------------------
    def insert_knot(self, axis, u):
        """Boehm's algorithm: one more knot u on `axis`, the function unchanged."""
        p, U = self._degrees[axis], self._knots[axis]
        n = U.size - p - 1
        if not U[p] <= u <= U[n]:
            raise ValueError(f"knot {u} outside the range [{U[p]}, {U[n]}] of axis {axis}")
        k = int(np.searchsorted(U, u, side="right")) - 1          # U[k] <= u < U[k + 1]
        k = min(k, n - 1)
        res = list(self.control_mesh_resolutions)
        P = self._cp.reshape(res[2], res[1], res[0], -1)
        P = np.moveaxis(P, 2 - axis, 0)                          # [n, ...]
        Q = np.empty((n + 1,) + P.shape[1:], dtype=np.float64)
        Q[:k - p + 1] = P[:k - p + 1]
        Q[k + 1:] = P[k:]
        for i in range(k - p + 1, k + 1):
            a = (u - U[i]) / (U[i + p] - U[i])
            Q[i] = a * P[i] + (1.0 - a) * P[i - 1]
        self._knots[axis] = np.insert(U, k + 1, u)
        self._cp = np.ascontiguousarray(np.moveaxis(Q, 0, 2 - axis)).reshape(-1, self._cp.shape[1])
        self._dev = {}

    def uniform_refine(self, n=1, axes=(0, 1, 2)):
        """Insert the midpoint of every non-empty knot span of `axes`, n times over (splinepy's uniform_refine)."""
        for _ in range(int(n)):
            for a in axes:
                p, U = self._degrees[a], self._knots[a]
                inner = np.unique(U[p:U.size - p])
                for u in (inner[:-1] + inner[1:]) / 2.0:
                    self.insert_knot(a, float(u))
        return self


def as_field(obj):
    """A BSplineField as it is; any object with degrees, knot_vectors and control_points (a splinepy BSpline) converted."""
    if isinstance(obj, BSplineField):
        return obj
    for name in ("degrees", "knot_vectors", "control_points"):
        if not hasattr(obj, name):
            raise TypeError(f"latent_vec_interpolation needs .{name} (a BSplineField or a splinepy BSpline), got {type(obj).__name__}")
    return BSplineField(list(obj.degrees), [list(kv) for kv in obj.knot_vectors], np.asarray(obj.control_points))
