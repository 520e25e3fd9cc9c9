"""Reconstruction metrics on the GPU: nearest neighbours between point sets and the Chamfer distance.

The reference scores a reconstruction with ``deep_sdf/metrics/chamfer.py compute_trimesh_chamfer``: trimesh draws points from
the generated mesh, two scipy KD-trees answer the nearest-neighbour queries.  Here the points come from
``TriangleMesh.sample_surface`` and the queries from one brute-force HIP kernel (csrc/pointset.hpp, include/dsdf.h ``dsdf_nn_*``,
``dsdf_mean_f64``); neither trimesh nor scipy is needed.

    nearest_neighbor(Q, R)        (sqr_dist fp32 [n], index int32 [n]); the lowest index wins ties
    chamfer_distance(A, B)        mean d^2 A -> B + mean d^2 B -> A, a Python float
    compute_trimesh_chamfer       the reference's function of this name (same parameters, same meaning) plus seed / exact

numpy in gives numpy out; a torch tensor gives tensors on its device.  There is no CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .meshsdf import INT32_MAX, TriangleMesh, _as_host_or_device, _mesh_device


def _device(*xs):
    return _mesh_device(*xs) or torch.device("cuda")


def _nn(Q, R, want_d2=True, want_idx=True):
    """Device tensors [nq, 3], [nr, 3] fp32 contiguous -> (sqr_dist or None, index or None) on their device."""
    nq, nr = Q.shape[0], R.shape[0]
    if nr == 0:
        raise ValueError("nearest_neighbor needs at least one reference point")
    if nq > INT32_MAX or nr > INT32_MAX:
        raise ValueError("at most 2^31 - 1 points per set")
    if not (want_d2 or want_idx):
        raise ValueError("nearest_neighbor: no output requested")
    lib = _lib.lib()
    with torch.cuda.device(Q.device):
        d2 = torch.empty(nq, dtype=torch.float32, device=Q.device) if want_d2 else None
        idx = torch.empty(nq, dtype=torch.int32, device=Q.device) if want_idx else None
        if nq:
            wb = C.c_size_t()
            _lib.check(lib.dsdf_nn_plan(nq, nr, C.byref(wb), None))
            ws = torch.empty(wb.value, dtype=torch.uint8, device=Q.device) if wb.value else None
            _lib.check(lib.dsdf_nn_query(_lib.ptr(Q), nq, _lib.ptr(R), nr, _lib.ptr(d2), _lib.ptr(idx), _lib.ptr(ws), wb.value, _lib.stream()))
    return d2, idx


def nearest_neighbor(Q, R, sqr_dist=True, index=True):
    """For every row of Q [n, 3] the squared distance to its nearest row of R [m, 3] and that row's index (the lowest on ties):
    (sqr_dist fp32 [n], index int32 [n]); an output switched off is None.  ValueError for m == 0 or a shape other than [*, 3]."""
    dev = _device(Q, R)
    Qd, numpy_out, out_dev = _as_host_or_device(Q, "Q", dev)
    Rd, _, _ = _as_host_or_device(R, "R", dev)
    d2, idx = _nn(Qd, Rd, sqr_dist, index)
    if numpy_out:
        return tuple(None if x is None else x.cpu().numpy() for x in (d2, idx))
    return tuple(None if x is None else x.to(out_dev) for x in (d2, idx))


def plan(n_queries, n_refs):
    """(workspace bytes, splits of the reference set) of a query (dsdf_nn_plan)."""
    wb, ns = C.c_size_t(), C.c_int32()
    _lib.check(_lib.lib().dsdf_nn_plan(int(n_queries), int(n_refs), C.byref(wb), C.byref(ns)))
    return wb.value, ns.value


def mean_f64(x):
    """fp64 mean of a 1-D fp32 device tensor as a 0-d fp64 device tensor (dsdf_mean_f64: deterministic, no atomics)."""
    if not (torch.is_tensor(x) and x.device.type == "cuda" and x.dtype == torch.float32 and x.dim() == 1):
        raise ValueError("mean_f64 takes a 1-D fp32 tensor on a HIP device")
    if x.numel() == 0:
        raise ValueError("mean_f64 of no values")
    x = x.contiguous()
    with torch.cuda.device(x.device):
        out = torch.empty((), dtype=torch.float64, device=x.device)
        ws = torch.empty(_lib.MEAN_WS_BYTES, dtype=torch.uint8, device=x.device)
        _lib.check(_lib.lib().dsdf_mean_f64(_lib.ptr(x), x.numel(), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream()))
    return out


def _one_sided(A, B):
    return mean_f64(_nn(A, B, True, False)[0])


def chamfer_distance(A, B):
    """mean over A of the squared distance to the nearest point of B, plus the same from B to A (point sets [n, 3], [m, 3])."""
    dev = _device(A, B)
    Ad, _, _ = _as_host_or_device(A, "A", dev)
    Bd, _, _ = _as_host_or_device(B, "B", dev)
    if Ad.shape[0] == 0 or Bd.shape[0] == 0:
        raise ValueError("chamfer_distance needs two non-empty point sets")
    return float(_one_sided(Ad, Bd) + _one_sided(Bd, Ad))


def _to_gt_frame(P, offset, scale):
    """p / scale - offset in fp64, rounded to fp32 once (points or vertices, a device tensor [n, 3])."""
    off = torch.as_tensor(np.asarray(offset, dtype=np.float64), device=P.device)
    return (P.to(torch.float64) / float(scale) - off).to(torch.float32).contiguous()


def compute_trimesh_chamfer(gt_points, gen_mesh, offset, scale, num_mesh_samples=30000, seed=0, exact=False):
    """Symmetric Chamfer distance of a reconstruction, the sum of both mean squared nearest-neighbour distances
    (deep_sdf/metrics/chamfer.py:9-39): num_mesh_samples points are drawn from gen_mesh, moved into the ground truth's frame by
    ``p / scale - offset`` and compared with gt_points.

    gt_points: an object with .vertices or an array [n, 3]; gen_mesh: an object with .vertices / .faces, a (V, F) pair or a
    .ply / .obj path.  seed selects the surface samples (the reference draws from numpy's global state).  exact=True replaces
    the gt -> gen direction by the true point-to-surface distance to the transformed mesh, which removes that direction's
    sampling noise."""
    from .sdf_sampler import _mesh_arrays
    gt = gt_points.vertices if hasattr(gt_points, "vertices") else gt_points
    dev = _device(gt)
    G, _, _ = _as_host_or_device(gt, "gt_points", dev)
    if G.shape[0] == 0:
        raise ValueError("gt_points is empty")
    V, F = _mesh_arrays(gen_mesh)
    mesh = TriangleMesh(V, F, dev)
    gen = _to_gt_frame(mesh.sample_surface(int(num_mesh_samples), seed=seed)[0], offset, scale)
    if gen.shape[0] == 0:
        raise ValueError("num_mesh_samples must be positive")
    if exact:
        gt_to_gen = mean_f64(TriangleMesh(_to_gt_frame(mesh.vertices, offset, scale), mesh.faces, dev).squared_distance(G)[0])
    else:
        gt_to_gen = _one_sided(G, gen)
    return float(gt_to_gen + _one_sided(gen, G))
