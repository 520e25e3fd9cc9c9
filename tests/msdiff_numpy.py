"""Numpy fp64 reference for the derivative of a microstructure mesh with respect to the spline's control points, written from the
specification in include/dsdf.h (dsdf_msd_*) and DESIGN 4.12: the grid edges of marching cubes' vertices, the band of grid points
that carry one, the dense tensor-product basis, and the Jacobian

    J[v, c, l] = (voxel_size[a] / 2) * sum_k dt/ds_k * m_k * G_k[l] * B_c(xo_k).

The tests compare the HIP kernels (csrc/msdiff.hpp) against it and pin the formula itself against end-to-end autograd."""
import numpy as np
import torch

from oracle import deepsdf_oracle as orc
from tests import mc_numpy, ms_numpy


def edges(sdf, level=0.0):
    """(edge_point [V] int64, edge_axis [V] int64) of every vertex of mc_numpy.marching_cubes(sdf, level), in its order."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    nx, ny, nz = sdf.shape
    inside = sdf < np.float32(level)
    cross = np.zeros((nx, ny, nz, 3), dtype=bool)
    cross[:-1, :, :, 0] = inside[:-1] != inside[1:]
    cross[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    cross[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    sel = np.nonzero(cross.reshape(-1))[0]
    return sel // 3, sel % 3


def vertices_from_edges(sdf, edge_point, edge_axis, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """origin + (p + t e_a) * spacing in fp32 with every operation rounded on its own: marching cubes' vertices from their edges."""
    sdf = np.ascontiguousarray(sdf, dtype=np.float32)
    F = np.float32
    stride = np.array([sdf.shape[1] * sdf.shape[2], sdf.shape[2], 1], dtype=np.int64)
    f = sdf.reshape(-1)
    p, a = np.asarray(edge_point, dtype=np.int64), np.asarray(edge_axis, dtype=np.int64)
    v0, v1 = f[p], f[p + stride[a]]
    t = (F(level) - v0) / (v1 - v0)
    pos = np.stack(np.unravel_index(p, sdf.shape), 1).astype(F)
    pos[np.arange(len(p)), a] += t
    return (np.asarray(origin, F) + pos * np.asarray(spacing, F)).astype(F)


def band(edge_point, edge_axis, dims):
    """(band [nb] sorted unique grid indices of {p, p + e_a}, row0 [V], row1 [V]: the band rows of the two endpoints)."""
    stride = np.array([dims[1] * dims[2], dims[2], 1], dtype=np.int64)
    p = np.asarray(edge_point, dtype=np.int64)
    q = p + stride[np.asarray(edge_axis, dtype=np.int64)]
    b = np.unique(np.concatenate([p, q]))
    return b, np.searchsorted(b, p), np.searchsorted(b, q)


def dense_basis(degrees, knots, pts):
    """B [n, ncp] fp64: the tensor-product basis weight of every control point (first parametric axis fastest) at pts [n, 3]."""
    Bs = [ms_numpy.basis_matrix(int(degrees[a]), knots[a], np.asarray(pts)[:, a]) for a in range(3)]
    return np.einsum("pk,pj,pi->pkji", Bs[2], Bs[1], Bs[0]).reshape(len(pts), -1)


def dt_factors(s0, s1, level=0.0):
    """(dt/ds0, dt/ds1) of t = (level - s0) / (s1 - s0), fp64."""
    s0, s1 = np.asarray(s0, dtype=np.float64), np.asarray(s1, dtype=np.float64)
    d2 = (s1 - s0) ** 2
    return (level - s1) / d2, -(level - s0) / d2


def jacobian(capped, edge_point, edge_axis, voxel_size, G_band, B_band, m_band, level=0.0):
    """(J [V, ncp, L] fp64, axis [V]).  capped: the grid [nx, ny, nz] whose edges carry the vertices; G_band [nb, L], B_band
    [nb, ncp] and m_band [nb] at the rows of band(edge_point, edge_axis, capped.shape)."""
    capped = np.asarray(capped, dtype=np.float64)
    _, r0, r1 = band(edge_point, edge_axis, capped.shape)
    stride = np.array([capped.shape[1] * capped.shape[2], capped.shape[2], 1], dtype=np.int64)
    a = np.asarray(edge_axis, dtype=np.int64)
    p = np.asarray(edge_point, dtype=np.int64)
    f = capped.reshape(-1)
    d0, d1 = dt_factors(f[p], f[p + stride[a]], level)
    G, B, m = (np.asarray(x, dtype=np.float64) for x in (G_band, B_band, m_band))
    scale = np.asarray(voxel_size, dtype=np.float64)[a] / 2
    J = ((scale * d0 * m[r0])[:, None, None] * B[r0][:, :, None] * G[r0][:, None, :] +
         (scale * d1 * m[r1])[:, None, None] * B[r1][:, :, None] * G[r1][:, None, :])
    return J, a


def check_edges_reproduce(sdf, level=0.0):
    """The edge list is mc_numpy.marching_cubes' own: its vertices recomputed from the edges, bit for bit."""
    p, a = edges(sdf, level)
    v, _ = mc_numpy.marching_cubes(sdf, level)
    assert np.array_equal(vertices_from_edges(sdf, p, a, level).view(np.uint32), v.view(np.uint32))
    return p, a


def clamped(p, inner):
    return [-1.0] * (p + 1) + list(inner) + [1.0] * (p + 1)


# non-uniform, a repeated interior knot each, every value exact in fp32 (the knot vectors of tests/test_gpu_microstructure.py)
KNOTS = {1: clamped(1, [-0.5, 0.25, 0.25, 0.625]), 2: clamped(2, [-0.375, 0.125, 0.125]), 3: clamped(3, [-0.25, 0.25, 0.25, 0.75])}
LINEAR_KNOTS = [[-1.0, -1.0, 1.0, 1.0]] * 3


class Fp64Structure:
    """An fp64 torch restatement of create_mesh_microstructure's forward up to the capped grid, differentiable in the control points:
    cp -> ms_numpy.basis_matrix -> oracle decoder_forward -> caps (torch.maximum / minimum in dict order, then the six planes).
    The coordinates are ms_numpy.grid_axes' fp32 values promoted to double.  The output bias is shifted once so that the given
    quantile (the median by default) of the decoder's values inside the domain is zero: the level set crosses the structure, and a
    small quantile leaves a small surface (few band points: the way to a seed whose every ReLU margin is large in a wide net); `params` are fp32 values held in double."""

    def __init__(self, L, net_kw, seed, degrees, knots, tiling, N, caps, cp_amp, quantile=0.5):
        self.L, self.degrees, self.knots, self.tiling, self.N, self.caps = L, tuple(degrees), knots, list(tiling), list(N), caps
        self.net = orc.make_net(L, **net_kw)
        self.params = {k: v.double() for k, v in orc.init_params(self.net, 100 + seed).items()}
        self.ncp = int(np.prod([len(U) - p - 1 for p, U in zip(degrees, knots)]))
        self.cp = np.random.default_rng(seed).uniform(-cp_amp, cp_amp, size=(self.ncp, L)).astype(np.float32)
        axes = ms_numpy.grid_axes(N, tiling)
        self.dims = [len(a[0]) for a in axes]
        self.xo = ms_numpy.grid_points(axes, 0).astype(np.float64)
        self.folded = torch.from_numpy(ms_numpy.grid_points(axes, 1).astype(np.float64))
        self.inside = ms_numpy.grid_inside(axes)
        self.B = dense_basis(degrees, knots, self.xo) * self.inside[:, None]         # outside rows: a constant zero latent
        self._Bt = torch.from_numpy(self.B)
        self._xs = [torch.from_numpy(a[0].astype(np.float64)).reshape(s) for a, s in zip(axes, [(-1, 1, 1), (1, -1, 1), (1, 1, -1)])]
        self.vs = [2.0 / (n + 2 - 1 - 2) for n in N]
        with torch.no_grad():
            raw = self.decode(self.rows(torch.from_numpy(self.cp).double()))[0].reshape(-1)
            last = f"lin{self.net.n_lin - 1}.bias"
            shifted = self.params[last] - torch.atanh(raw[torch.from_numpy(self.inside)].quantile(quantile))
            self.params[last] = shifted.float().double()                             # every parameter stays an fp32 value

    def rows(self, cp_t):
        return torch.cat([self._Bt @ cp_t, self.folded], 1)

    def decode(self, rows):
        """(raw [dims], Saved with min_abs_pre) of decoder input rows [n, L + 3]."""
        y, sv = orc.decoder_forward(self.net, self.params, rows, training=False, track_margin=True)
        return y.reshape(self.dims), sv

    def cap(self, raw):
        """(capped, [every plane value a cap compares against, each [dims]])."""
        v, planes = raw, []
        for loc, d in self.caps.items():
            dim, m = ms_numpy.LOCATION[loc]
            border = (self._xs[dim] - m * (1 - d["measure"])) * -m
            planes.append((-border if d["cap"] == -1 else border).expand(self.dims))
            v = torch.maximum(v, -border) if d["cap"] == -1 else torch.minimum(v, border)
        for dim in range(3):
            for m in (-1, 1):
                plane = -((self._xs[dim] - m) * -m)
                planes.append(plane.expand(self.dims))
                v = torch.maximum(v, plane)
        return v, planes

    def conditions(self, raw, sv, planes, band_idx):
        """(smallest |raw - cap plane value|, smallest ReLU margin) over the band: the function is smooth where both are positive."""
        r = raw.detach().reshape(-1)[band_idx]
        gap = min(float((r - p.reshape(-1)[band_idx]).abs().min()) for p in planes)
        return gap, float(sv.min_abs_pre.detach()[band_idx].min())
