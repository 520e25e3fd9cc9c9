"""Meshes from latent codes: the API of the reference's ``deep_sdf/mesh.py`` (create_mesh :26-83,
convert_sdf_samples_to_ply :86-155) with every step on the GPU.

    grid   sdf_grid         the N^3 grid decoded chunk by chunk: coordinates are generated on the device per chunk (the
                            N^3 x 4 host array of the reference is never built), decoded by Engine.decode_latent (one code,
                            its products hoisted) or Engine.decode for the layer-by-layer variants, written in place
    mesh   marching_cubes   HIP marching cubes (csrc/mcubes.hpp, dsdf_mc_count / dsdf_mc_emit): one host sync per mesh, to
                            read the two totals and allocate exact outputs
    file   write_ply        one header + two buffer writes, byte for byte what plyfile writes for the reference's dtypes

There is no CPU path: the grid and the marching cubes need a HIP device (a grid handed in on the host is moved there).
"""
import ctypes as C
import logging
import time

import numpy as np
import torch

from . import _lib

logger = logging.getLogger(__name__)

INT32_MAX = 2 ** 31 - 1


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _triple(x, what):
    t = [float(v) for v in (x if isinstance(x, (list, tuple, np.ndarray, torch.Tensor)) else [x] * 3)]
    if len(t) != 3:
        raise ValueError(f"{what} needs 3 values, got {len(t)}")
    return t


# ---- marching cubes ---------------------------------------------------------------------------------------------------
def marching_cubes(sdf_grid, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0)):
    """Surface {sdf == level} of a dense device grid sdf_grid [nx, ny, nz] (z fastest; 2 <= n <= 1024 per axis).

    Returns (verts [V, 3] fp32, faces [F, 3] int32) on the grid's device; an empty surface gives empty tensors.  Inside is
    v < level (strictly); vertex of edge (p, a): origin + (p + t e_a) * spacing; order and orientation: include/dsdf.h."""
    g = sdf_grid
    if not torch.is_tensor(g) or g.dim() != 3:
        raise ValueError("marching_cubes expects a 3-D tensor [nx, ny, nz]")
    if g.device.type != "cuda":
        raise _lib.DsdfError("marching_cubes needs a grid on a HIP device (no CPU fallback)")
    g = g.to(torch.float32).contiguous()
    nx, ny, nz = g.shape
    lib = _lib.lib()
    sp, org = (C.c_float * 3)(*_triple(spacing, "spacing")), (C.c_float * 3)(*_triple(origin, "origin"))
    b = C.c_size_t()
    _lib.check(lib.dsdf_mc_workspace_bytes(nx, ny, nz, C.byref(b)))
    with torch.cuda.device(g.device):
        ws = torch.empty(b.value, dtype=torch.uint8, device=g.device)
        totals = torch.empty(2, dtype=torch.int64, device=g.device)
        _lib.check(lib.dsdf_mc_count(_ptr(g), nx, ny, nz, float(level), _ptr(totals), _ptr(ws), ws.numel(), _stream()))
        nv, nf = totals.tolist()                            # the one host sync of a mesh
        if nv > INT32_MAX or nf > INT32_MAX:                # the library refuses before writing anything: raise its error
            _lib.check(lib.dsdf_mc_emit(_ptr(g), nx, ny, nz, float(level), sp, org, nv, nf, None, None, _ptr(ws), ws.numel(),
                                        _stream()))
        verts = torch.empty(nv, 3, dtype=torch.float32, device=g.device)
        faces = torch.empty(nf, 3, dtype=torch.int32, device=g.device)
        _lib.check(lib.dsdf_mc_emit(_ptr(g), nx, ny, nz, float(level), sp, org, nv, nf, _ptr(verts), _ptr(faces), _ptr(ws),
                                    ws.numel(), _stream()))
    return verts, faces


def case_table():
    """The case table compiled into the library (dsdf_mc_case_table): int8 [256, width], edge ids, -1 terminated."""
    lib = _lib.lib()
    w = C.c_int32()
    _lib.check(lib.dsdf_mc_case_table(None, 0, C.byref(w)))
    out = np.empty((256, w.value), dtype=np.int8)
    _lib.check(lib.dsdf_mc_case_table(out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(w)))
    return out


# ---- PLY --------------------------------------------------------------------------------------------------------------
def ply_header(n_verts, n_faces):
    return ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {n_verts}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {n_faces}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")


def write_ply(path, verts, faces):
    """Binary little-endian PLY with the layout plyfile writes for the reference's dtypes (vertex x, y, z f4; face
    `list uchar int vertex_indices`).  verts [V, 3], faces [F, 3]: tensors (any device) or arrays."""
    v = verts.detach().cpu().numpy() if torch.is_tensor(verts) else np.asarray(verts)
    f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
    v = np.ascontiguousarray(v.reshape(-1, 3), dtype="<f4")
    f = f.reshape(-1, 3)
    packed = np.empty(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    packed["n"] = 3
    packed["idx"] = f
    with open(path, "wb") as fh:
        fh.write(ply_header(v.shape[0], f.shape[0]))
        fh.write(v.tobytes())
        fh.write(packed.tobytes())


# ---- grid -------------------------------------------------------------------------------------------------------------
def grid_coords(N, start, end, voxel_origin=(-1, -1, -1), device="cpu"):
    """Coordinates of grid points [start, end) of the N^3 grid (linear index, z fastest), bit for bit the reference's
    create_mesh (mesh.py:42-56): fp32 index * voxel_size, then + origin, voxel_size = 2 / (N - 1).  Axis a takes
    voxel_origin[a] (the reference adds voxel_origin[2 - a]; its origin is the same on every axis)."""
    voxel_size = 2.0 / (N - 1)
    idx = torch.arange(start, end, dtype=torch.int64, device=device)
    out = torch.empty(end - start, 3, dtype=torch.float32, device=device)
    out[:, 2] = idx % N
    out[:, 1] = (idx // N) % N
    out[:, 0] = ((idx // N) // N) % N
    for a in range(3):
        out[:, a] = (out[:, a] * voxel_size) + voxel_origin[a]
    return out


def _unwrap(decoder):
    return decoder.module if isinstance(decoder, torch.nn.DataParallel) else decoder


def _is_hip_decoder(dec):
    from .decoder import Decoder
    return isinstance(dec, Decoder)


def sdf_grid(decoder, latent, N, max_batch=32 ** 3, voxel_origin=(-1, -1, -1), device=None):
    """The decoder's SDF on the N^3 grid of create_mesh, as a device tensor [N, N, N] (axis 0 = x).

    This package's Decoder decodes through its Engine (decode_latent where the library takes the net, decode on [latent |
    xyz] otherwise: LayerNorm, xyz_in_all, latent_dropout), weights materialised once; any other nn.Module is called on the
    chunk's [latent | xyz] -- only its decode leaves the library."""
    dec = _unwrap(decoder)
    hip = _is_hip_decoder(dec)
    if hip:
        device = dec._arena.device
    elif device is None:
        device = torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DsdfError("sdf_grid needs a HIP device (no CPU fallback)")
    n = N ** 3
    out = torch.empty(n, dtype=torch.float32, device=device)
    with torch.no_grad():
        z = latent.detach().to(device, torch.float32).reshape(1, -1)
        if hip:
            eng = dec.engine()
            eng.materialize()                      # once per mesh: no per-chunk re-materialisation
            single = eng.decode_latent_supported()
        for s in range(0, n, max_batch):
            e = min(n, s + max_batch)
            xyz = grid_coords(N, s, e, voxel_origin, device)
            if hip and single:
                y = eng.decode_latent(z, xyz)
            elif hip:
                y = eng.decode(torch.cat([z.expand(e - s, -1), xyz], 1))
            else:
                y = dec(torch.cat([z.expand(e - s, -1), xyz], 1))
            out[s:e] = y.reshape(-1)
    return out.view(N, N, N)


# ---- the reference's API ----------------------------------------------------------------------------------------------
def create_mesh(decoder, latent_vec, filename, N=256, max_batch=32 ** 3, offset=None, scale=None, device=None):
    """deep_sdf/mesh.py create_mesh: decoder.eval(), decode the N^3 grid over [-1, 1]^3, mesh the zero level set and write
    it to `filename` exactly as given (binary PLY)."""
    start = time.time()
    decoder.eval()
    voxel_origin = [-1, -1, -1]
    voxel_size = 2.0 / (N - 1)
    grid = sdf_grid(decoder, latent_vec, N, max_batch, voxel_origin, device)
    logger.debug("sampling takes: %f", time.time() - start)
    convert_sdf_samples_to_ply(grid, voxel_origin, voxel_size, filename, offset, scale)


def convert_sdf_samples_to_ply(pytorch_3d_sdf_tensor, voxel_grid_origin, voxel_size, ply_filename_out, offset=None,
                               scale=None):
    """deep_sdf/mesh.py convert_sdf_samples_to_ply: level-0 marching cubes of the grid (moved to the GPU if it is on the
    host), vertices + origin, then / scale, then - offset, written as binary PLY.  ValueError if 0 is outside the grid's
    value range (as skimage.measure.marching_cubes)."""
    start = time.time()
    g = pytorch_3d_sdf_tensor.detach()
    if g.device.type != "cuda":
        g = g.to("cuda")
    lo, hi = (float(x) for x in torch.aminmax(g.float()))
    if not lo <= 0.0 <= hi:
        raise ValueError("Surface level must be within volume data range.")
    verts, faces = marching_cubes(g, 0.0, _triple(voxel_size, "voxel_size"), _triple(voxel_grid_origin, "voxel_grid_origin"))
    if scale is not None:
        verts = verts / torch.as_tensor(scale, dtype=torch.float32, device=verts.device)
    if offset is not None:
        verts = verts - torch.as_tensor(offset, dtype=torch.float32, device=verts.device)
    write_ply(ply_filename_out, verts, faces)
    logger.debug("converting to ply format and writing to file took %f s", time.time() - start)
