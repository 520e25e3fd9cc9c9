"""Meshes from latent codes: the API of the reference's ``deep_sdf/mesh.py`` (create_mesh :26-83,
convert_sdf_samples_to_ply :86-155) with every step on the GPU.

    grid   sdf_grid         the N^3 grid decoded chunk by chunk: coordinates are generated on the device per chunk (the
                            N^3 x 4 host array of the reference is never built), decoded by Engine.decode_latent (one code,
                            its products hoisted) or Engine.decode for the layer-by-layer variants, written in place
    mesh   marching_cubes   HIP marching cubes (csrc/mcubes.hpp, dsdf_mc_count / dsdf_mc_emit): one host sync per mesh, to
                            read the two totals and allocate exact outputs
    file   write_ply        one header + two buffer writes, byte for byte what plyfile writes for the reference's dtypes
           write_points_ply the vertex-only variant (SurfaceSamples)
    tiled  microstructure_sdf_grid / create_mesh_microstructure / sdf_struct: a B-spline latent field over mirrored unit cells
                            (create_mesh_microstructure :157-342): rows and caps by csrc/msgrid.hpp around the same decode
    diff   microstructure_mesh_diff / create_mesh_microstructure_diff (:346-454): d vertices / d control points assembled in closed
                            form (csrc/msdiff.hpp) from one input-gradient pass over the band of grid points that carry a vertex
    volume tetrahedralize / solid_components / TetMesh (deepsdf_amd/tetmesh.py, re-exported here): the solid {sdf < level} of the
                            same grid as a conforming tetrahedral mesh with its boundary triangles (csrc/tetmesh.hpp)
           MicrostructureMeshDiff.for_tetmesh / VolumeMeshDiff: d vertices / d control points of every moving vertex of that mesh,
                            the face and body diagonals included, on a band of its own (csrc/voldiff.hpp)

    sparse follow_surface   surface following on blocks of the same dense grid (csrc/sparsegrid.hpp): the coarse lattice
                            is decoded, blocks near the surface are seeded and grown across mixed-sign faces, only their points
                            are decoded, the rest is filled with a coarse value of the right sign.  block= / lipschitz= on
                            sdf_grid, microstructure_sdf_grid and microstructure_mesh_diff; the reference-named functions honour
                            the context manager sparse_grid(block, lipschitz).  Off (block=None) by default.

There is no CPU path: the grid and the marching cubes need a HIP device (a grid handed in on the host is moved there).
"""
import contextlib
import ctypes as C
import logging
import math
import operator
import time
from typing import NamedTuple, TypedDict

import numpy as np
import torch

from . import _lib

logger = logging.getLogger(__name__)

INT32_MAX = 2 ** 31 - 1


# ---- marching cubes ---------------------------------------------------------------------------------------------------
def marching_cubes(sdf_grid, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), return_edges=False):
    """Surface {sdf == level} of a dense device grid sdf_grid [nx, ny, nz] (z fastest; 2 <= n <= 1024 per axis).

    Returns (verts [V, 3] fp32, faces [F, 3] int32) on the grid's device; an empty surface gives empty tensors.  Inside is
    v < level (strictly); vertex of edge (p, a): origin + (p + t e_a) * spacing; order and orientation: include/dsdf.h.
    return_edges: also (edge_point [V] int64, edge_axis [V] int32), the grid point p (linear index) and axis a of every vertex."""
    g = sdf_grid
    if not torch.is_tensor(g) or g.dim() != 3:
        raise ValueError("marching_cubes expects a 3-D tensor [nx, ny, nz]")
    if g.device.type != "cuda":
        raise _lib.DsdfError("marching_cubes needs a grid on a HIP device (no CPU fallback)")
    g = g.to(torch.float32).contiguous()
    nx, ny, nz = g.shape
    lib = _lib.lib()
    sp, org = (C.c_float * 3)(*_lib.triple(spacing, "spacing")), (C.c_float * 3)(*_lib.triple(origin, "origin"))
    b = C.c_size_t()
    _lib.check(lib.dsdf_mc_workspace_bytes(nx, ny, nz, C.byref(b)))
    with torch.cuda.device(g.device):
        ws = torch.empty(b.value, dtype=torch.uint8, device=g.device)
        totals = torch.empty(2, dtype=torch.int64, device=g.device)
        _lib.check(lib.dsdf_mc_count(_lib.ptr(g), nx, ny, nz, float(level), _lib.ptr(totals), _lib.ptr(ws), ws.numel(), _lib.stream()))
        nv, nf = totals.tolist()                            # the one host sync of a mesh
        if nv > INT32_MAX or nf > INT32_MAX:                # the library refuses before writing anything: raise its error
            _lib.check(lib.dsdf_mc_emit(_lib.ptr(g), nx, ny, nz, float(level), sp, org, nv, nf, None, None, _lib.ptr(ws), ws.numel(),
                                        _lib.stream()))
        verts = torch.empty(nv, 3, dtype=torch.float32, device=g.device)
        faces = torch.empty(nf, 3, dtype=torch.int32, device=g.device)
        _lib.check(lib.dsdf_mc_emit(_lib.ptr(g), nx, ny, nz, float(level), sp, org, nv, nf, _lib.ptr(verts), _lib.ptr(faces), _lib.ptr(ws),
                                    ws.numel(), _lib.stream()))
        if return_edges:
            edge_point = torch.empty(nv, dtype=torch.int64, device=g.device)
            edge_axis = torch.empty(nv, dtype=torch.int32, device=g.device)
            _lib.check(lib.dsdf_mc_edges(nx, ny, nz, nv, _lib.ptr(edge_point), _lib.ptr(edge_axis), _lib.ptr(ws), ws.numel(), _lib.stream()))
            return verts, faces, edge_point, edge_axis
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


def write_points_ply(path, points):
    """Vertex-only binary little-endian PLY (x, y, z f4): the SurfaceSamples files.  points [n, 3]: a tensor or an array."""
    v = points.detach().cpu().numpy() if torch.is_tensor(points) else np.asarray(points)
    v = np.ascontiguousarray(v.reshape(-1, 3), dtype="<f4")
    with open(path, "wb") as fh:
        fh.write(("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\nend_header\n").encode("ascii"))
        fh.write(v.tobytes())


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


# ---- surface following on blocks of the dense grid (csrc/sparsegrid.hpp, dsdf_sg_*) -------------------------------------
def _check_sparse(block, lipschitz):
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)):
        raise ValueError(f"block must be an integer number of cells, got {block!r}")
    if block < 2:
        raise ValueError(f"block must be at least 2 cells, got {block}")
    try:
        lip = float(lipschitz)
    except (TypeError, ValueError):
        raise ValueError(f"lipschitz must be a number, got {lipschitz!r}") from None
    if not math.isfinite(lip) or lip < 0:
        raise ValueError(f"lipschitz must be finite and >= 0, got {lipschitz!r}")
    return int(block), lip


def sparse_threshold(block, spacing, lipschitz):
    """The seeding distance: lipschitz x half the diagonal of a full block, spacing[a] the grid spacing of axis a in the coordinates
    the decoder sees; computed in double and rounded to fp32 once."""
    return float(np.float32(float(lipschitz) * 0.5 * math.sqrt(sum((block * float(x)) ** 2 for x in _lib.triple(spacing, "spacing")))))


_SPARSE = [(None, 1.0)]


@contextlib.contextmanager
def sparse_grid(block, lipschitz=1.0):
    """Inside this context create_mesh, create_mesh_microstructure and create_mesh_microstructure_diff (whose signatures are the
    reference's) decode only the blocks of `block` cells per edge that the surface passes through (follow_surface).  lipschitz: a
    bound on the field's slope in decoder coordinates; 1.0 is a distance field's, 0 seeds by corner signs alone (fast; a component
    that flips no block corner is lost), a spline latent field adds slope of its own and is a reason to raise it; values that
    saturate far from the surface only ever help.  block=None: the dense path.  Contexts nest; the outer setting returns on exit.
    The setting is the process's, not a thread's."""
    _SPARSE.append((None, 1.0) if block is None else _check_sparse(block, lipschitz))
    try:
        yield
    finally:
        _SPARSE.pop()


def add_sparse_args(parser):
    """--block B and --lipschitz X of the meshing command lines: the arguments of sparse_grid (no --block: the dense grid)."""
    parser.add_argument("--block", type=int, default=None, metavar="B",
                        help="decode only the blocks of B cells per edge that the surface passes through (default: the whole grid)")
    parser.add_argument("--lipschitz", type=float, default=1.0, metavar="X",
                        help="with --block: bound on the field's slope used to seed blocks; 0 seeds by corner signs alone (default 1.0)")


def grid_coords_at(dims, voxel_size, origin, indices):
    """xyz [n, 3] of the listed points (device int64 [n]) of a grid of dims points: fp32 index * voxel_size[a], then + origin[a],
    each rounded on its own -- bit for bit grid_coords at those indices (dsdf_sg_coords)."""
    dims = _int_triple(dims, "dims")
    idx = indices.contiguous()
    vs, org = (C.c_float * 3)(*_lib.triple(voxel_size, "voxel_size")), (C.c_float * 3)(*_lib.triple(origin, "origin"))
    with torch.cuda.device(idx.device):
        xyz = torch.empty(idx.numel(), 3, dtype=torch.float32, device=idx.device)
        _lib.check(_lib.lib().dsdf_sg_coords(*dims, vs, org, _lib.ptr(idx), idx.numel(), _lib.ptr(xyz), _lib.stream()))
    return xyz


def ms_caps_at(values, N, indices, cap_border_dict=None):
    """Caps in place on values [n] (contiguous fp32 device tensor), the values of the listed points (device int64 [n]) of the padded
    grid: bit for bit ms_apply_caps at those points (dsdf_sg_caps_at)."""
    g, _ = _ms_grid(1, N)
    recs, n = cap_records(cap_border_dict)
    idx = indices.contiguous()
    if values.dtype != torch.float32 or not values.is_contiguous() or values.numel() != idx.numel() or values.device.type != "cuda":
        raise ValueError("ms_caps_at expects a contiguous fp32 device tensor with one value per index")
    with torch.cuda.device(values.device):
        _lib.check(_lib.lib().dsdf_sg_caps_at(C.byref(g), _lib.ptr(idx), idx.numel(), recs, n, _lib.ptr(values), _lib.stream()))
    return values


def _padded_chunks(indices, max_batch, pad):
    """(start, end, the chunk's indices) over a list of indices in chunks of max_batch; pad > 0: a short chunk is filled up to
    min(max_batch, pad) rows with its last index, pad being the number of grid points -- the size of the dense path's full chunks,
    so that every decode call picks their kernel family."""
    n = indices.numel()
    full = min(max_batch, pad)
    for s in range(0, n, max_batch):
        e = min(n, s + max_batch)
        chunk = indices[s:e]
        if e - s < full:
            chunk = torch.cat([chunk, chunk[-1:].expand(full - (e - s))])
        yield s, e, chunk


def follow_surface(dims, block, thr, level, values_at, caps_at=None, *, device=None, on_step=None):
    """Surface following on blocks of the dense grid of dims = (nx, ny, nz) points: the grid marching cubes needs, with
    only the blocks the surface passes through decoded.

    values_at(indices) -> values: the only thing that knows about decoders; indices is a device int64 tensor of distinct linear
    grid indices (z fastest), ascending; values an fp32 device tensor of as many.  caps_at(indices, values) -> capped values (a new
    tensor), for grids that are meshed after a cut: states are then decided on the capped values.

    1. the coarse lattice (every block-th point per axis and the last) is decoded; 2. a block is seeded if its 8 corners are not
    all inside (v < level) or all outside, or if min |v - level| over them is <= thr; 3. per round the points of the new blocks that
    have no value yet are decoded; 4. an inactive block becomes active if a face-neighbour decoded in this round has mixed inside
    flags on the shared face; 3 and 4 repeat until a round activates nothing (the host reads two counts per round: one stream
    wait); 5. every point that never got a value takes the coarse value at the low corner of the lowest block that contains it.

    Returns (grid, capped or None, stats): [nx, ny, nz] fp32 device tensors and stats = {blocks, seeds, active, rounds, points
    (decoded), total (grid points)}.  The grid holds the field ONLY at decoded points: elsewhere a value of the right sign.  Its
    marching-cubes mesh is the dense one minus the components that have no cell in a seeded block; none is lost when thr bounds the
    change of the field over half a block diagonal.

    on_step(name, workspace, plan, indices): called after every step has been put on the stream -- "start", "coarse" (indices: the
    lattice), "coarse_decode", "seed", "wait" (the host has read the counts), then per round "emit" (indices: the round's points),
    "decode", "grow", "wait", and last "fill".  workspace is the run's uint8 tensor and plan its DsdfSgPlan (state_offset and
    have_offset locate the block states and the point map): what the tests compare with the oracle and the benchmarks time."""
    dims = _int_triple(dims, "dims")
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise _lib.DsdfError("follow_surface needs a HIP device (no CPU fallback)")
    lib = _lib.lib()
    plan = _lib.DsdfSgPlan()
    _lib.check(lib.dsdf_sg_plan(*dims, int(block), C.byref(plan)))
    npts = plan.n_points
    level, thr = float(level), float(thr)
    with torch.no_grad(), torch.cuda.device(device):
        ws = torch.empty(plan.ws_bytes, dtype=torch.uint8, device=device)
        counts = torch.zeros(2, dtype=torch.int64, device=device)
        n_new, n_pts = C.c_void_p(counts.data_ptr()), C.c_void_p(counts.data_ptr() + 8)
        grid = torch.empty(npts, dtype=torch.float32, device=device)
        capped = torch.empty(npts, dtype=torch.float32, device=device) if caps_at is not None else None
        seen = grid if capped is None else capped           # the grid that is meshed decides the states
        at = (*dims, int(block))
        wsa = (_lib.ptr(ws), ws.numel(), _lib.stream())

        def step(name, indices=None):
            if on_step is not None:
                on_step(name, ws, plan, indices)

        def decode_into(idx):
            vals = values_at(idx).to(torch.float32).reshape(-1).contiguous()
            if vals.numel() != idx.numel():
                raise ValueError(f"values_at returned {vals.numel()} values for {idx.numel()} indices")
            _lib.check(lib.dsdf_sg_scatter(_lib.ptr(idx), idx.numel(), _lib.ptr(vals), _lib.ptr(grid), npts, _lib.stream()))
            if capped is not None:
                cv = caps_at(idx, vals).to(torch.float32).reshape(-1).contiguous()
                _lib.check(lib.dsdf_sg_scatter(_lib.ptr(idx), idx.numel(), _lib.ptr(cv), _lib.ptr(capped), npts, _lib.stream()))

        step("start")
        idx = torch.empty(plan.n_coarse, dtype=torch.int64, device=device)
        _lib.check(lib.dsdf_sg_coarse(*at, _lib.ptr(idx), *wsa))
        step("coarse", idx)
        decode_into(idx)
        step("coarse_decode")
        decoded = plan.n_coarse
        _lib.check(lib.dsdf_sg_seed(_lib.ptr(seen), *at, level, thr, n_new, *wsa))
        _lib.check(lib.dsdf_sg_points_count(*at, n_pts, *wsa))
        step("seed")
        new, pts = counts.tolist()                          # the one stream wait of a round
        step("wait")
        seeds, active, rounds = new, 0, 0
        while new > 0:
            rounds += 1
            active += new
            idx = torch.empty(pts, dtype=torch.int64, device=device)
            _lib.check(lib.dsdf_sg_points_emit(*at, pts, _lib.ptr(idx), *wsa))
            step("emit", idx)
            if pts > 0:
                decode_into(idx)
                decoded += pts
            step("decode")
            _lib.check(lib.dsdf_sg_grow(_lib.ptr(seen), *at, level, n_new, *wsa))
            _lib.check(lib.dsdf_sg_points_count(*at, n_pts, *wsa))
            step("grow")
            new, pts = counts.tolist()
            step("wait")
        _lib.check(lib.dsdf_sg_fill(_lib.ptr(grid), *at, *wsa))
        if capped is not None:
            _lib.check(lib.dsdf_sg_fill(_lib.ptr(capped), *at, *wsa))
        step("fill")
    stats = dict(blocks=int(plan.n_blocks), seeds=seeds, active=active, rounds=rounds, points=decoded, total=int(npts))
    return grid.view(*dims), None if capped is None else capped.view(*dims), stats


def sdf_grid(decoder, latent, N, max_batch=32 ** 3, voxel_origin=(-1, -1, -1), device=None, *, block=None, lipschitz=1.0,
             stats=None, on_step=None):
    """The decoder's SDF on the N^3 grid of create_mesh, as a device tensor [N, N, N] (axis 0 = x).

    This package's Decoder decodes through its Engine (decode_latent where the library takes the net, decode on [latent |
    xyz] otherwise: LayerNorm, xyz_in_all, latent_dropout), weights materialised once; any other nn.Module is called on the
    chunk's [latent | xyz] -- only its decode leaves the library.

    block: decode only the blocks of `block` cells per edge that the surface {sdf == 0} passes through (follow_surface; lipschitz as
    in sparse_grid).  The result then holds the SDF only at decoded points -- elsewhere a value of the right sign -- and its mesh is
    the dense grid's.  A short chunk of a HIP decoder is padded to the dense path's chunk size, min(max_batch, N^3).
    stats: a dict that receives follow_surface's record; on_step: follow_surface's callback."""
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
    if block is not None:
        block, lipschitz = _check_sparse(block, lipschitz)
        voxel_size = 2.0 / (N - 1)
        with torch.no_grad():
            z = latent.detach().to(device, torch.float32).reshape(1, -1)
            if hip:
                eng = dec.engine()
                eng.materialize()
                single = eng.decode_latent_supported()

            def values_at(indices):
                vals = torch.empty(indices.numel(), dtype=torch.float32, device=device)
                for s, e, chunk in _padded_chunks(indices, max_batch, n if hip else 0):
                    xyz = grid_coords_at(N, voxel_size, voxel_origin, chunk)
                    if hip and single:
                        y = eng.decode_latent(z, xyz)
                    elif hip:
                        y = eng.decode(torch.cat([z.expand(chunk.numel(), -1), xyz], 1))
                    else:
                        y = dec(torch.cat([z.expand(chunk.numel(), -1), xyz], 1))
                    vals[s:e] = y.reshape(-1)[:e - s]
                return vals

            grid, _, st = follow_surface(N, block, sparse_threshold(block, voxel_size, lipschitz), 0.0, values_at, device=device,
                                         on_step=on_step)
        if stats is not None:
            stats.update(st)
        return grid
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
    block, lipschitz = _SPARSE[-1]                         # sparse_grid(): the signature is the reference's
    grid = sdf_grid(decoder, latent_vec, N, max_batch, voxel_origin, device, block=block, lipschitz=lipschitz)
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
    verts, faces = marching_cubes(g, 0.0, _lib.triple(voxel_size, "voxel_size"), _lib.triple(voxel_grid_origin, "voxel_grid_origin"))
    if scale is not None:
        verts = verts / torch.as_tensor(scale, dtype=torch.float32, device=verts.device)
    if offset is not None:
        verts = verts - torch.as_tensor(offset, dtype=torch.float32, device=verts.device)
    write_ply(ply_filename_out, verts, faces)
    logger.debug("converting to ply format and writing to file took %f s", time.time() - start)


# ---- microstructures: a spline latent field over tiled, mirrored unit cells ------------------------------------------------
# deep_sdf/mesh.py create_mesh_microstructure and analysis/geometry.py sdf_struct.  Per chunk of the padded grid the row kernel
# (dsdf_ms_rows) writes [spline latent | folded xyz], the decoder turns rows into SDF values, the cap kernel (dsdf_ms_caps) cuts
# the borders in place; the grid never leaves the device.
location_lookup = {"x0": (0, -1), "x1": (0, 1), "y0": (1, -1), "y1": (1, 1), "z0": (2, -1), "z1": (2, 1)}

CapType = TypedDict("CapType", {"cap": int, "measure": float})
CapBorderDict = TypedDict("CapBorderDict", {loc: CapType for loc in location_lookup}, total=False)


def default_cap_border_dict():
    """Cap -1 (cut the structure flush) with measure 0 on all six faces."""
    return {loc: {"cap": -1, "measure": 0} for loc in location_lookup}


def _int_triple(x, what):
    if isinstance(x, (list, tuple, np.ndarray)):
        if len(x) != 3:
            raise ValueError(f"{what} must be a list of 3 integers")
        return [int(v) for v in x]
    if isinstance(x, (int, np.integer)) and not isinstance(x, bool):
        return [int(x)] * 3
    raise ValueError(f"{what} must be a list or an integer")


def _ms_grid(tiling, N):
    """DsdfMsGrid of the padded grid (N + 2 per axis) and its voxel sizes as the reference computes them (double)."""
    t, n = _int_triple(tiling, "Tiling"), _int_triple(N, "Number of grid points")
    if min(t) < 1:
        raise ValueError(f"Tiling must be positive, got {t}")
    if min(n) < 2:
        raise ValueError(f"Number of grid points must be at least 2 per axis, got {n}")
    g = _lib.DsdfMsGrid()
    for a in range(3):
        g.dims[a], g.tiling[a] = n[a] + 2, t[a]
    return g, [2.0 / (n[a] + 2 - 1 - 2) for a in range(3)]


def cap_records(cap_border_dict):
    """The ordered (dim, m, measure, cap) records of a cap dictionary, in the dictionary's own iteration order (a min and a max do
    not commute).  None, or the CapBorderDict class itself (the reference's default argument): the defaults."""
    if cap_border_dict is None or cap_border_dict is CapBorderDict:
        cap_border_dict = default_cap_border_dict()
    if len(cap_border_dict) > _lib.MS_MAX_CAPS:
        raise ValueError(f"at most {_lib.MS_MAX_CAPS} cap entries, got {len(cap_border_dict)}")
    recs = (_lib.DsdfMsCap * max(len(cap_border_dict), 1))()
    for r, (loc, d) in enumerate(cap_border_dict.items()):
        if loc not in location_lookup:
            raise ValueError(f"unknown cap location {loc!r} (one of {list(location_lookup)})")
        cap, measure = d["cap"], d["measure"]
        if cap not in (-1, 1):
            raise ValueError("Cap must be -1 or 1")
        dim, m = location_lookup[loc]
        recs[r].dim, recs[r].cap, recs[r].m, recs[r].c = dim, int(cap), float(m), float(m * (1 - measure))
    return recs, len(cap_border_dict)


def ms_grid_rows(field, tiling, N, start, end, device=None):
    """Decoder input rows [end - start, L + 3] = [spline latent | folded xyz] of points [start, end) of the padded grid."""
    from .spline import as_field
    field = as_field(field)
    g, _ = _ms_grid(tiling, N)
    device = torch.device("cuda" if device is None else device)
    with torch.cuda.device(device):
        s, _keep = field.c_spline(device)
        rows = torch.empty(max(end - start, 0), s.L + 3, dtype=torch.float32, device=device)
        _lib.check(_lib.lib().dsdf_ms_rows(C.byref(s), C.byref(g), start, end, None, 1, 1, _lib.ptr(rows), _lib.stream()))
    return rows


def ms_point_rows(field, tiling, points, inside_test=False, with_xyz=True):
    """Rows for an explicit list of points [n, 3] (device tensor): [spline latent | folded xyz], or the latent columns alone.
    inside_test: rows of points outside [-1, 1]^3 get zero latents as on the grid; off, the point is clamped to the knot range."""
    from .spline import as_field
    field = as_field(field)
    g, _ = _ms_grid(tiling, 2)
    pts = points.detach().to(torch.float32).contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.device.type != "cuda":
        raise ValueError("ms_point_rows expects a device tensor [n, 3]")
    with torch.cuda.device(pts.device):
        s, _keep = field.c_spline(pts.device)
        rows = torch.empty(pts.shape[0], s.L + (3 if with_xyz else 0), dtype=torch.float32, device=pts.device)
        if pts.shape[0] > 0:
            _lib.check(_lib.lib().dsdf_ms_rows(C.byref(s), C.byref(g), 0, pts.shape[0], _lib.ptr(pts), int(bool(inside_test)),
                                               int(bool(with_xyz)), _lib.ptr(rows), _lib.stream()))
    return rows


def ms_rows_at(field, tiling, N, indices):
    """Grid-mode rows at a list of padded-grid linear indices (device int64 tensor [n], any order): (rows [n, L + 3], bit for bit
    ms_grid_rows at those indices; weights [n, 64], slot (k * 4 + j) * 4 + i; base [n] int32, first control point, -1 outside)."""
    from .spline import as_field
    field = as_field(field)
    g, _ = _ms_grid(tiling, N)
    idx = indices
    if not torch.is_tensor(idx) or idx.dim() != 1 or idx.dtype != torch.int64 or idx.device.type != "cuda":
        raise ValueError("ms_rows_at expects a device int64 tensor [n]")
    idx = idx.contiguous()
    n = idx.numel()
    with torch.cuda.device(idx.device):
        s, _keep = field.c_spline(idx.device)
        rows = torch.empty(n, s.L + 3, dtype=torch.float32, device=idx.device)
        weights = torch.empty(n, _lib.MS_WEIGHTS, dtype=torch.float32, device=idx.device)
        base = torch.empty(n, dtype=torch.int32, device=idx.device)
        if n > 0:
            _lib.check(_lib.lib().dsdf_ms_rows_at(C.byref(s), C.byref(g), _lib.ptr(idx), n, _lib.ptr(rows), _lib.ptr(weights), _lib.ptr(base),
                                                  _lib.stream()))
    return rows, weights, base


def ms_apply_caps(sdf, N, start, end, cap_border_dict=None):
    """Caps in place on sdf [end - start] (contiguous fp32 device tensor), the values of points [start, end) of the padded grid."""
    g, _ = _ms_grid(1, N)
    recs, n = cap_records(cap_border_dict)
    if sdf.dtype != torch.float32 or not sdf.is_contiguous() or sdf.numel() != end - start or sdf.device.type != "cuda":
        raise ValueError("ms_apply_caps expects a contiguous fp32 device tensor of end - start values")
    with torch.cuda.device(sdf.device):
        _lib.check(_lib.lib().dsdf_ms_caps(C.byref(g), start, end, recs, n, _lib.ptr(sdf), _lib.stream()))
    return sdf


def _ms_sparse_grids(tiling, decoder, field, N, max_batch, cap_border_dict, device, apply_caps, block, lipschitz, stats=None,
                     on_step=None):
    """(raw, capped or None) of microstructure_sdf_grid by surface following: rows at listed points by dsdf_ms_rows_at, caps at
    listed points by dsdf_sg_caps_at.  The decoder sees folded coordinates, which the fold scales by the tiling: the seeding
    distance uses voxel_size[a] * tiling[a]."""
    from .spline import as_field
    field = as_field(field)
    block, lipschitz = _check_sparse(block, lipschitz)
    dec = _unwrap(decoder)
    hip = _is_hip_decoder(dec)
    if hip:
        device = dec._arena.device
    elif device is None:
        device = torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DsdfError("microstructure_sdf_grid needs a HIP device (no CPU fallback)")
    t, n = _int_triple(tiling, "Tiling"), _int_triple(N, "Number of grid points")
    g, voxel_size = _ms_grid(t, n)
    npts = g.dims[0] * g.dims[1] * g.dims[2]
    cap_records(cap_border_dict)                            # validates before anything runs
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError(f"max_batch must be positive, got {max_batch}")
    if hip:
        eng = dec.engine()
        eng.materialize()

    def values_at(indices):
        vals = torch.empty(indices.numel(), dtype=torch.float32, device=device)
        for s, e, chunk in _padded_chunks(indices, max_batch, npts if hip else 0):
            rows, _, _ = ms_rows_at(field, t, n, chunk)
            y = eng.decode(rows) if hip else dec(rows)
            vals[s:e] = y.reshape(-1)[:e - s]
        return vals

    def caps_at(indices, values):
        return ms_caps_at(values.clone(), n, indices, cap_border_dict)

    thr = sparse_threshold(block, [voxel_size[a] * t[a] for a in range(3)], lipschitz)
    raw, capped, st = follow_surface(list(g.dims), block, thr, 0.0, values_at, caps_at if apply_caps else None, device=device,
                                     on_step=on_step)
    if stats is not None:
        stats.update(st)
    return raw, capped


def microstructure_sdf_grid(tiling, decoder, field, N, max_batch=32 ** 3, cap_border_dict=None, device=None, apply_caps=True, *,
                            block=None, lipschitz=1.0, stats=None, on_step=None):
    """The capped SDF of a microstructure on the padded grid, a device tensor [Nx + 2, Ny + 2, Nz + 2] (axis 0 = x).

    The design domain [-1, 1]^3 is tiled with tiling[a] mirrored copies of the unit cell per axis; `field` (a BSplineField, or a
    splinepy BSpline) gives every point its latent code.  This package's Decoder decodes through its Engine, weights
    materialised once; any other nn.Module is called on the rows.  The result does not depend on max_batch.

    block: decode only the blocks the surface passes through (follow_surface; block and lipschitz as in sparse_grid).  The result
    then holds the SDF only at decoded points -- elsewhere a value of the right sign -- and its mesh is the dense grid's.  stats,
    on_step: as sdf_grid's."""
    if block is not None:
        raw, capped = _ms_sparse_grids(tiling, decoder, field, N, max_batch, cap_border_dict, device, apply_caps, block, lipschitz,
                                       stats, on_step)
        return capped if apply_caps else raw
    from .spline import as_field
    field = as_field(field)
    dec = _unwrap(decoder)
    hip = _is_hip_decoder(dec)
    if hip:
        device = dec._arena.device
    elif device is None:
        device = torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.DsdfError("microstructure_sdf_grid needs a HIP device (no CPU fallback)")
    g, _ = _ms_grid(tiling, N)
    recs, n_caps = cap_records(cap_border_dict)
    dims = list(g.dims)
    n = dims[0] * dims[1] * dims[2]
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError(f"max_batch must be positive, got {max_batch}")
    lib = _lib.lib()
    with torch.no_grad(), torch.cuda.device(device):
        s, _keep = field.c_spline(device)
        out = torch.empty(n, dtype=torch.float32, device=device)
        rows = torch.empty(min(n, max_batch), s.L + 3, dtype=torch.float32, device=device)
        if hip:
            eng = dec.engine()
            eng.materialize()
        for b in range(0, n, max_batch):
            e = min(n, b + max_batch)
            r = rows[:e - b]
            _lib.check(lib.dsdf_ms_rows(C.byref(s), C.byref(g), b, e, None, 1, 1, _lib.ptr(r), _lib.stream()))
            y = eng.decode(r) if hip else dec(r)
            out[b:e] = y.reshape(-1)
            if apply_caps:
                _lib.check(lib.dsdf_ms_caps(C.byref(g), b, e, recs, n_caps, C.c_void_p(out.data_ptr() + 4 * b), _lib.stream()))
    return out.view(*dims)


def create_mesh_microstructure(tiling, decoder, latent_vec_interpolation, filename, N=256, max_batch=32 ** 3, offset=None,
                               scale=None, cap_border_dict=None, save_ply_file=False, use_flexicubes=False, device=None,
                               output_tetmesh=False, compute_derivatives=False):
    """deep_sdf/mesh.py create_mesh_microstructure: mesh the zero level set of the tiled, capped structure.

    save_ply_file: writes ``filename + ".ply"`` (vertices + voxel origin, / scale, - offset) and returns None; otherwise returns
    (verts [V, 3] float64, faces [F, 3] int32) as numpy arrays, verts = (index-space vertices * voxel_size - voxel_size) / 2,
    which maps the design domain onto [0, 1]^3."""
    tiling = _int_triple(tiling, "Tiling")
    n = _int_triple(N, "Number of grid points")
    if use_flexicubes or output_tetmesh or compute_derivatives:
        raise NotImplementedError("use_flexicubes / output_tetmesh / compute_derivatives need kaolin's FlexiCubes, which this "
                                  "package does not carry: only marching cubes is implemented")
    start = time.time()
    decoder.eval()
    _, voxel_size = _ms_grid(tiling, n)
    voxel_origin = [-1 - v for v in voxel_size]
    block, lipschitz = _SPARSE[-1]                         # sparse_grid(): the signature is the reference's
    grid = microstructure_sdf_grid(tiling, decoder, latent_vec_interpolation, n, max_batch, cap_border_dict, device, block=block,
                                   lipschitz=lipschitz)
    logger.debug("sampling takes: %f", time.time() - start)
    if save_ply_file:
        convert_sdf_samples_to_ply(grid, voxel_origin, voxel_size, filename + ".ply", offset, scale)
        return None
    verts, faces = marching_cubes(grid, 0.0, voxel_size)
    vs = np.array(voxel_size)
    return (verts.cpu().numpy() - vs) / 2, faces.cpu().numpy()


def sdf_struct(decoder, queries, tiling, latent_vec_interpolation, device=None):
    """analysis/geometry.py sdf_struct: the structure's SDF (no caps) at queries [n, 3], a numpy array [n].  The spline is
    evaluated at every query (clamped to its knot range), the decoder at the folded coordinate."""
    dec = _unwrap(decoder)
    hip = _is_hip_decoder(dec)
    if hip:
        device = dec._arena.device
    elif device is None:
        device = torch.device("cuda")
    q = torch.as_tensor(queries, dtype=torch.float32).to(device)
    tiling = _int_triple(tiling, "Tiling")
    with torch.no_grad():
        rows = ms_point_rows(latent_vec_interpolation, tiling, q, inside_test=False)
        y = dec.engine().decode(rows) if hip else dec(rows)
    return y.reshape(-1).detach().cpu().numpy()


# ---- d vertices / d control points ------------------------------------------------------------------------------------------------
# deep_sdf/mesh.py create_mesh_microstructure_diff :346-454.  A marching-cubes vertex is a closed-form function of the two grid values
# of its edge, and a grid value depends on the control points through the row's latent columns only, so the Jacobian is assembled
# from d sdf / d latent at the band of grid points that carry a vertex (one forward + one input-gradient pass over the band) and
# the spline weights the row kernel holds (csrc/msdiff.hpp).  The reference's FlexiCubes variant is not implemented.
def _free_device_memory(device):
    return torch.cuda.mem_get_info(device)[0]


def _check_fits(device, what, shape, advice):
    """Raise MemoryError, stating the size, when an fp32 array of `shape` would not fit the free device memory."""
    need = 4 * int(np.prod(shape, dtype=np.int64))
    free = _free_device_memory(device)
    if need > free:
        raise MemoryError(f"{what} {list(shape)} fp32 takes {need} bytes ({need / 2 ** 30:.2f} GiB), the device has {free} bytes "
                          f"free: {advice}")


class _Band(NamedTuple):
    """The grid points that carry an endpoint of a vertex's edge, and what the derivative reads at each (_band_rows)."""
    band: torch.Tensor                                      # [nb] int64 grid indices, sorted
    band_of: torch.Tensor                                   # [npts] int32 grid index -> band row, -1 off the band
    G: torch.Tensor                                         # [nb, L] d sdf / d latent
    weights: torch.Tensor                                   # [nb, 64] basis weights of the row kernel
    base: torch.Tensor                                      # [nb] int32 first control point, -1: outside
    mask: torch.Tensor                                      # [nb] uint8 inside and capped value == raw value


class _MeshDiff:
    """What the surface's and the volume's derivative share: the band's tensors as attributes, and the marshalling of vjp and jvp
    around the entries dsdf_<_entry>_*.  A subclass has grid, _band, _degrees, _n_cp, _structs() -> (mesh struct, band struct),
    _n_rows (the rows of grad_verts and d_verts) and _n_list (the vertices its adjoint walks)."""
    band, band_of, G, weights, base, mask = (property(operator.attrgetter("_band." + k)) for k in _Band._fields)

    @property
    def device(self):
        return self.grid.device

    def _band_struct(self):
        b, G, L = _lib.DsdfMsdBand(), self.G, self.latent_size
        b.G, b.weights, b.base, b.mask = (t.data_ptr() for t in (G, self.weights, self.base, self.mask))
        b.n_band, b.ld_g, b.L = G.shape[0], G.stride(0) if G.shape[0] > 0 else L, L
        for a in range(3):
            b.degree[a], b.n_cp[a] = self._degrees[a], self._n_cp[a]
        return b

    def _call(self, entry, *args):
        m, b = self._structs()
        _lib.check(getattr(_lib.lib(), f"dsdf_{self._entry}_{entry}")(C.byref(m), C.byref(b), *args, _lib.stream()))

    def _operand(self, x, name, shape):
        x = torch.as_tensor(x).to(self.device, torch.float32).contiguous()
        if x.shape != shape:
            raise ValueError(f"{name} must be [{shape[0]}, {shape[1]}], got {tuple(x.shape)}")
        return x

    def vjp_plan(self):
        """(scratch bytes, partial sums of the first stage) of vjp (dsdf_msd_ / dsdf_vd_vjp_workspace_bytes)."""
        nbytes, parts = C.c_size_t(), C.c_int32()
        plan = getattr(_lib.lib(), f"dsdf_{self._entry}_vjp_workspace_bytes")
        _lib.check(plan(self._n_list, self.n_control_points, self.latent_size, C.byref(nbytes), C.byref(parts)))
        return nbytes.value, parts.value

    def vjp(self, grad_verts):
        """grad_verts [V, 3] -> grad_cp [ncp, L] fp32 = sum_v sum_b grad_verts[v, b] * J[v, b]: a fixed-order two-stage sum.  The
        surface: b is the vertex's edge axis.  The volume: over the moving vertices; rows of grid vertices are never read."""
        gv = self._operand(grad_verts, "grad_verts", (self._n_rows, 3))
        with torch.cuda.device(self.device):
            ws = torch.empty(max(self.vjp_plan()[0], 256), dtype=torch.uint8, device=self.device)
            out = torch.empty(self.n_control_points, self.latent_size, dtype=torch.float32, device=self.device)
            self._call("vjp", _lib.ptr(gv), _lib.ptr(out), _lib.ptr(ws), ws.numel())
        return out

    def jvp(self, d_cp):
        """d_cp [ncp, L] -> d_verts [V, 3] fp32.  The surface: zero off each vertex's edge axis.  The volume: every flagged
        coordinate of a moving vertex, zero everywhere else."""
        d = self._operand(d_cp, "d_cp", (self.n_control_points, self.latent_size))
        with torch.cuda.device(self.device):
            out = torch.empty(self._n_rows, 3, dtype=torch.float32, device=self.device)
            self._call("jvp", _lib.ptr(d), _lib.ptr(out))
        return out


class MicrostructureMeshDiff(_MeshDiff):
    """A microstructure mesh with its derivative with respect to the spline's control points (microstructure_mesh_diff).

    verts [V, 3] float64 and faces [F, 3] int32 (device) are create_mesh_microstructure's; edge_point [V] int64 / edge_axis [V] int32
    name the padded-grid edge of every vertex.  Only coordinate edge_axis[v] of vertex v depends on the control points.  band,
    band_of, G, weights, base, mask: the band of the vertices' edges (_Band)."""
    _entry = "msd"

    def __init__(self, verts, faces, edge_point, edge_axis, grid, band, field, scale, voxel_size=None):
        self.verts, self.faces, self.edge_point, self.edge_axis = verts, faces, edge_point, edge_axis
        self.voxel_size = None if voxel_size is None else [float(v) for v in voxel_size]      # the grid's spacing before (v - vs) / 2
        self.grid, self._band = grid, band
        self.n_control_points, self.latent_size = int(field.control_points.shape[0]), int(field.latent_size)
        self._degrees = [int(d) for d in field.degrees]
        self._n_cp = [int(n) for n in field.control_mesh_resolutions]
        self._scale = scale
        self._n_rows = self._n_list = int(verts.shape[0])
        self._rows_of = None                                # microstructure_mesh_diff: band indices -> _Band, for for_tetmesh

    def for_tetmesh(self, tet, t_clamp=0.0):
        """-> VolumeMeshDiff: the derivative of every moving vertex of `tet`, a TetMesh made from self.grid with
        tetrahedralize(..., t_clamp=t_clamp, return_edges=True).  Grid values are read from self.grid: with keep_largest the mesh
        came from a grid whose dropped points were overwritten with the level, and no crossing edge of it has a dropped endpoint,
        so self.grid holds the values both meshes used.  Decodes the volume mesh's own band (one more pass of the band loop)."""
        return _volume_mesh_diff(self, tet, t_clamp)

    def _structs(self):
        m = _lib.DsdfMsdMesh()
        m.grid, m.edge_point, m.edge_axis, m.band_of = (t.data_ptr() for t in (self.grid, self.edge_point, self.edge_axis, self.band_of))
        m.n_verts, m.level = self.verts.shape[0], 0.0
        for a in range(3):
            m.dims[a], m.scale[a] = self.grid.shape[a], self._scale[a]
        return m, self._band_struct()

    def jacobian(self, dense=False):
        """dense=False: (jac [V, ncp, L] fp32, axis [V] int32), jac[v] = d verts[v, axis[v]] / d control points.  dense=True: the
        reference's [V, 3, ncp, L] with the two other coordinates' planes zero.  Raises MemoryError, stating the size, when the
        array would not fit the free device memory."""
        V, ncp, L = self.verts.shape[0], self.n_control_points, self.latent_size
        shape = (V, 3, ncp, L) if dense else (V, ncp, L)
        _check_fits(self.device, "the Jacobian", shape, "use vjp / jvp, or dense=False" + ("" if dense else " with a coarser grid"))
        with torch.cuda.device(self.device):
            jac = torch.empty(shape, dtype=torch.float32, device=self.device)
            axis = torch.empty(V, dtype=torch.int32, device=self.device)
            self._call("jacobian", int(bool(dense)), _lib.ptr(jac), _lib.ptr(axis))
        return jac if dense else (jac, axis)


def microstructure_mesh_diff(tiling, decoder, field, N, max_batch=32 ** 3, cap_border_dict=None, device=None, *, block=None,
                             lipschitz=1.0):
    """The mesh create_mesh_microstructure returns, on the device, with what its derivative needs (MicrostructureMeshDiff).

    Forward: the raw grid, its capped copy and marching cubes, as create_mesh_microstructure.  Band: the sorted unique grid points
    {p, p + e_a} of the vertices' edges.  Per chunk of max_batch band points: rows at the band indices (dsdf_ms_rows_at), the
    decoder's forward and its input gradient with d_sdf = 1 (Engine.module_input_grad; torch.autograd.grad for any other
    nn.Module).  mask = inside and capped value == raw value.

    block: the raw and the capped grid come from one surface-following run (follow_surface; block and lipschitz as in sparse_grid).
    Band points are endpoints of vertex edges and so lie in decoded blocks: mask and Jacobian mean what they mean on the dense grid;
    `grid` holds the SDF only at decoded points."""
    from .spline import as_field
    field = as_field(field)
    tiling, n = _int_triple(tiling, "Tiling"), _int_triple(N, "Number of grid points")
    dec = _unwrap(decoder)
    hip = _is_hip_decoder(dec)
    decoder.eval()
    _, voxel_size = _ms_grid(tiling, n)
    max_batch = int(max_batch)
    if block is None:
        raw = microstructure_sdf_grid(tiling, decoder, field, n, max_batch, cap_border_dict, device, apply_caps=False)
        grid = None
    else:
        raw, grid = _ms_sparse_grids(tiling, decoder, field, n, max_batch, cap_border_dict, device, True, block, lipschitz)
    device = raw.device
    dims = list(raw.shape)
    npts = raw.numel()
    L = int(field.latent_size)
    with torch.cuda.device(device):
        if grid is None:
            grid = raw.clone()
            ms_apply_caps(grid.view(-1), n, 0, npts, cap_border_dict)
        verts, faces, edge_point, edge_axis = marching_cubes(grid, 0.0, voxel_size, return_edges=True)
        vs = torch.tensor(voxel_size, dtype=torch.float64, device=device)
        verts = (verts.double() - vs) / 2
        stride = torch.tensor([dims[1] * dims[2], dims[2], 1], dtype=torch.int64, device=device)
        band = torch.unique(torch.cat([edge_point, edge_point + stride[edge_axis.long()]]))      # sorted

        def rows_of(band):
            return _band_rows(band, dec, hip, field, tiling, n, max_batch, raw, grid)
        band = rows_of(band)
    scale = [float(np.float32(v / 2)) for v in voxel_size]
    d = MicrostructureMeshDiff(verts, faces, edge_point, edge_axis, grid, band, field, scale, voxel_size)
    d._rows_of = rows_of                                   # for_tetmesh: the volume mesh's band goes through the same loop
    return d


def _band_rows(band, dec, hip, field, tiling, n, max_batch, raw, grid):
    """band [nb] sorted grid indices -> _Band: per chunk of max_batch band points the rows at the band indices, the decoder's forward
    and its input gradient; mask = inside and capped value == raw value (microstructure_mesh_diff's band loop; the volume mesh's
    band runs it again on its own points)."""
    device, npts, L = raw.device, raw.numel(), int(field.latent_size)
    with torch.cuda.device(device):
        nb = band.numel()
        band_of = torch.full((npts,), -1, dtype=torch.int32, device=device)
        band_of[band] = torch.arange(nb, dtype=torch.int32, device=device)
        G = torch.empty(nb, L, dtype=torch.float32, device=device)
        weights = torch.empty(nb, _lib.MS_WEIGHTS, dtype=torch.float32, device=device)
        base = torch.empty(nb, dtype=torch.int32, device=device)
        if hip:
            eng = dec.engine()
            eng.materialize()
        ones = torch.ones(min(nb, max_batch), dtype=torch.float32, device=device)
        for b in range(0, nb, max_batch):
            e = min(nb, b + max_batch)
            rows, weights[b:e], base[b:e] = ms_rows_at(field, tiling, n, band[b:e])
            if hip:
                with torch.no_grad():
                    eng.module_forward(rows, False)
                    G[b:e] = eng.module_input_grad(ones[:e - b], e - b)[:, :L]
            else:
                x = rows.detach().requires_grad_(True)
                with torch.enable_grad():
                    y = dec(x)
                    G[b:e] = torch.autograd.grad(y.sum(), x)[0][:, :L]
        flat_raw, flat = raw.view(-1), grid.view(-1)
        mask = ((base >= 0) & (flat[band] == flat_raw[band])).to(torch.uint8)
    return _Band(band, band_of, G, weights, base, mask)


class VolumeMeshDiff(_MeshDiff):
    """The derivative of a volume mesh's vertices with respect to the spline's control points (csrc/voldiff.hpp, dsdf_vd_*;
    DESIGN 4.22): every class >= 1 vertex of tetmesh.tetrahedralize's mesh -- the marching-cubes vertices and those on the face and
    body diagonals -- moves along its edge; grid vertices do not.  Built by MicrostructureMeshDiff.for_tetmesh.

    moving [Vm] int32: the ids of the class >= 1 vertices, ascending (a vertex the clamp holds is in the list and has a zero
    derivative).  band: the sorted unique endpoints of their edges, with its own G / weights / base / mask: an endpoint of a
    crossing diagonal need not be an endpoint of a crossing axis edge, so the surface's band is not enough.  Unstretched, in the
    coordinates of MicrostructureMeshDiff.verts (scale = voxel_size / 2)."""
    _entry = "vd"

    def __init__(self, diff, tet, t_clamp, band):
        self.diff, self.t_clamp = diff, float(t_clamp)
        self.grid, self._band = diff.grid, band
        self.vert_point, self.vert_class = tet.vert_point, tet.vert_class
        self.n_verts = int(tet.verts.shape[0])
        self.moving = torch.nonzero(self.vert_class > 0).reshape(-1).to(torch.int32)          # ascending
        self.n_control_points, self.latent_size = diff.n_control_points, diff.latent_size
        self._degrees, self._n_cp = diff._degrees, diff._n_cp
        self._n_rows, self._n_list = self.n_verts, self.moving.numel()

    def _structs(self, index=None):
        index = self.moving if index is None else index
        m = _lib.DsdfVdMesh()
        m.grid, m.vert_point, m.vert_class, m.vert_index, m.band_of = (t.data_ptr() for t in (self.grid, self.vert_point, self.vert_class,
                                                                                            index, self.band_of))
        m.n_verts, m.n_moving, m.level, m.t_clamp = self.n_verts, index.numel(), 0.0, self.t_clamp
        for a in range(3):
            m.dims[a], m.scale[a] = self.grid.shape[a], self.diff._scale[a]
        return m, self._band_struct()

    def dtheta_moving(self, normals, stretch=(1.0, 1.0, 1.0), clip=0.0):
        """[Vm, 3, ncp * L] fp32: the (stretched, clipped) Jacobian of every moving vertex projected onto its normal
        (dsdf_vd_dtheta); normals [V, 3].  Raises MemoryError, stating the size, when the array would not fit the device."""
        n = self._operand(normals, "normals", (self.n_verts, 3))
        Vm, R = self.moving.numel(), self.n_control_points * self.latent_size
        _check_fits(self.device, "dtheta", (Vm, 3, R), "use vjp / jvp, or a coarser grid")
        with torch.cuda.device(self.device):
            out = torch.empty(Vm, 3, R, dtype=torch.float32, device=self.device)
            st = (C.c_float * 3)(*[float(s) for s in stretch])
            self._call("dtheta", _lib.ptr(n), st, float(clip), _lib.ptr(out))
        return out

    def jacobian(self):
        """[V, 3, ncp, L] fp32, for small meshes: one tangent (jvp) per column, so ncp * L launches.  Raises MemoryError, stating
        the size, when the array would not fit the free device memory."""
        V, ncp, L = self.n_verts, self.n_control_points, self.latent_size
        _check_fits(self.device, "the Jacobian", (V, 3, ncp, L), "use vjp / jvp")
        jac = torch.empty(V, 3, ncp * L, dtype=torch.float32, device=self.device)
        unit = torch.zeros(ncp * L, dtype=torch.float32, device=self.device)
        for r in range(ncp * L):
            unit[r] = 1.0
            jac[:, :, r] = self.jvp(unit.view(ncp, L))
            unit[r] = 0.0
        return jac.view(V, 3, ncp, L)


def _volume_mesh_diff(diff, tet, t_clamp=0.0):
    if tet.vert_point is None or tet.vert_class is None:
        raise ValueError("the TetMesh carries no vertex edges: build it with tetrahedralize(..., return_edges=True)")
    if diff._rows_of is None:
        raise ValueError("this MicrostructureMeshDiff cannot decode a band: build it with microstructure_mesh_diff")
    t_clamp = float(t_clamp)
    if not 0.0 <= t_clamp < 0.5:
        raise ValueError(f"t_clamp must lie in [0, 0.5), got {t_clamp}")
    device = diff.device
    tet = tet.to(device)
    dims = list(diff.grid.shape)
    with torch.cuda.device(device):
        c = tet.vert_class.long()
        mv = c > 0
        p, c = tet.vert_point[mv], c[mv]
        q = p + (c & 1) * (dims[1] * dims[2]) + ((c >> 1) & 1) * dims[2] + ((c >> 2) & 1)
        band = torch.unique(torch.cat([p, q]))                                                  # sorted
        if band.numel() and (int(band[0]) < 0 or int(band[-1]) >= diff.grid.numel()):
            raise ValueError("the TetMesh's vertex edges leave the grid of this MicrostructureMeshDiff")
        band = diff._rows_of(band)
    return VolumeMeshDiff(diff, tet, t_clamp, band)


def create_mesh_microstructure_diff(tiling, decoder, latent_vec_interpolation, N=256, max_batch=32 ** 3, offset=None, scale=None,
                                    cap_border_dict=None, device=None, output_tetmesh=False, compute_derivatives=False):
    """deep_sdf/mesh.py create_mesh_microstructure_diff: (verts [V, 3] float64, faces [F, 3] int32, jac) as numpy arrays, verts and
    faces exactly create_mesh_microstructure's.  compute_derivatives: jac [V, 3, n_control_points, latent_dim] fp32 =
    d verts / d control points of the marching-cubes mesh; otherwise jac = [] (as the reference).  offset and scale are accepted
    and unused, as in the reference's return path."""
    if output_tetmesh:
        raise NotImplementedError("output_tetmesh needs kaolin's FlexiCubes, which this package does not carry: only the "
                                  "marching-cubes surface and its derivative are implemented")
    if not compute_derivatives:
        verts, faces = create_mesh_microstructure(tiling, decoder, latent_vec_interpolation, "unused", N=N, max_batch=max_batch,
                                                  cap_border_dict=cap_border_dict, device=device)
        return verts, faces, []
    block, lipschitz = _SPARSE[-1]                         # sparse_grid(): the signature is the reference's
    d = microstructure_mesh_diff(tiling, decoder, latent_vec_interpolation, N, max_batch, cap_border_dict, device, block=block,
                                 lipschitz=lipschitz)
    return d.verts.cpu().numpy(), d.faces.cpu().numpy(), d.jacobian(dense=True).cpu().numpy()


# ---- volume meshes ----------------------------------------------------------------------------------------------------------------
def microstructure_tetmesh(tiling, decoder, field, N, max_batch=32 ** 3, cap_border_dict=None, device=None, *, t_clamp=0.0,
                           keep_largest=False, block=None, lipschitz=1.0, ply_filename=None):
    """The solid of the tiled, capped structure as a TetMesh (tetmesh.tetrahedralize of the grid create_mesh_microstructure meshes),
    in the coordinates of its PLY file: voxel origin + index * voxel size.  Its axis-class vertices are the PLY's vertices.

    ply_filename: also write the surface of the SAME grid there, byte for byte the file create_mesh_microstructure(...,
    save_ply_file=True) writes: the structure is decoded once for both meshes."""
    tiling, n = _int_triple(tiling, "Tiling"), _int_triple(N, "Number of grid points")
    decoder.eval()
    _, voxel_size = _ms_grid(tiling, n)
    voxel_origin = [-1 - v for v in voxel_size]
    grid = microstructure_sdf_grid(tiling, decoder, field, n, max_batch, cap_border_dict, device, block=block, lipschitz=lipschitz)
    if ply_filename is not None:
        convert_sdf_samples_to_ply(grid, voxel_origin, voxel_size, ply_filename)
    return tetrahedralize(grid, 0.0, voxel_size, voxel_origin, t_clamp=t_clamp, keep_largest=keep_largest)


from .tetmesh import TetMesh, solid_components, tetrahedralize  # noqa: E402,F401  (re-exports; tetmesh.py does not import this module)
