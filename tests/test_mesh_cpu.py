"""CPU (no GPU needed): the marching-cubes case table (generator vs the table compiled into the library, face consistency over
all 256 cases), the numpy reference algorithm on analytic fields, the PLY writer, the grid coordinates of create_mesh, and
argument checking of the dsdf_mc_* entry points (every call here fails before any launch)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from deepsdf_amd import mc_table
from tests import mc_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from deepsdf_amd.build import build_library
    build_library()
    from deepsdf_amd import _lib
    return _lib.lib()


# ---- case table ---------------------------------------------------------------------------------------------------------
def test_generated_header_is_current_and_the_library_ships_it(lib):
    with open(mc_table.HEADER) as f:
        assert f.read() == mc_table.header_text(), "csrc/mc_table.hpp is stale: python -m deepsdf_amd.mc_table"
    from deepsdf_amd.mesh import case_table
    t = case_table()
    assert t.shape == (256, mc_table.WIDTH) and t.dtype == np.int8
    assert np.array_equal(t, np.array(mc_table.table_rows(), dtype=np.int8))
    assert mc_table.WIDTH == 3 * max(len(x) for x in mc_table.TABLE) + 1
    assert len(mc_table.TABLE[0]) == 0 and len(mc_table.TABLE[255]) == 0


def _crossing(case, e):
    c, a = mc_table.EDGES[e]
    return ((case >> c) & 1) != ((case >> (c | (1 << a))) & 1)


def _face_of(e0, e1):
    """The cube face (f, s) holding both edges (two distinct edges share at most one face)."""
    faces = []
    for f in range(3):
        for s in range(2):
            cs = set(mc_table.face_corners(f, s))
            ends = lambda e: {mc_table.EDGES[e][0], mc_table.EDGES[e][0] | (1 << mc_table.EDGES[e][1])}
            if ends(e0) <= cs and ends(e1) <= cs:
                faces.append((f, s))
    assert len(faces) <= 1
    return faces[0] if faces else None


def _boundary(case):
    """Directed triangle edges of a case whose reverse is not in the case: the segments on the cube faces."""
    d = [(t[i], t[(i + 1) % 3]) for t in mc_table.TABLE[case] for i in range(3)]
    return [e for e in d if (e[1], e[0]) not in d]


def test_every_case_is_a_set_of_closed_fans():
    for case in range(256):
        tris = mc_table.TABLE[case]
        used = sorted({e for t in tris for e in t})
        assert used == [e for e in range(12) if _crossing(case, e)], case        # exactly the crossing edges, each used
        d = [(t[i], t[(i + 1) % 3]) for t in tris for i in range(3)]
        assert len(set(d)) == len(d), case                                        # no directed edge twice
        for a, b in d:
            assert a != b
        bnd = _boundary(case)
        interior = [e for e in d if e not in bnd]
        for a, b in interior:                                                     # interior edges: twice, opposite directions
            assert d.count((b, a)) == 1, case
        starts, ends = sorted(a for a, _ in bnd), sorted(b for _, b in bnd)
        assert starts == ends == used, case                                       # boundary: every crossing edge in and out once
        for a, b in bnd:
            assert _face_of(a, b) is not None, (case, a, b)                       # boundary edges lie on a cube face


def _local(case, f, s):
    """Boundary segments of `case` on face (f, s), as positions in the face's edge cycle (0..3)."""
    q = mc_table.face_corners(f, s)
    pos = {mc_table._edge_between(q[i], q[(i + 1) % 4]): i for i in range(4)}
    return sorted((pos[a], pos[b]) for a, b in _boundary(case) if _face_of(a, b) == (f, s))


def test_face_segments_depend_only_on_the_face_and_neighbours_traverse_them_oppositely():
    for f in range(3):
        for s in range(2):
            q = mc_table.face_corners(f, s)
            seen = {}
            for case in range(256):
                signs = tuple((case >> c) & 1 for c in q)
                segs = _local(case, f, s)
                assert seen.setdefault(signs, segs) == segs, (f, s, case)
            assert len(seen) == 16
            if s == 1:
                continue
            # the cell across face (f, 0) sees it as its face (f, 1): corner c of ours is its corner c | (1 << f)
            q1 = mc_table.face_corners(f, 1)
            for signs, segs in seen.items():
                other = None
                for case in range(256):
                    if tuple((case >> c) & 1 for c in q1) == signs:
                        other = _local(case, f, 1)
                        break
                # q and q1 list the corners in the same cyclic order, so edge positions correspond
                assert sorted((b, a) for a, b in segs) == other, (f, signs)


def test_case_one_points_away_from_the_inside_corner():
    (a, b, c), = mc_table.TABLE[1]
    pa, pb, pc = (np.array(mc_table.edge_mid(e)) for e in (a, b, c))
    assert np.cross(pb - pa, pc - pa) @ np.ones(3) > 0


# ---- the reference algorithm on analytic fields ---------------------------------------------------------------------------
def test_numpy_sphere_is_a_closed_outward_surface():
    N, r = 48, 0.5
    sdf, h = mc_numpy.sphere(N, r)
    v, f = mc_numpy.marching_cubes(sdf, 0.0, (h, h, h), (-1, -1, -1))
    ok, euler, vol = mc_numpy.closed_manifold_stats(v, f)
    assert ok and euler == 2
    exact = 4 / 3 * math.pi * r ** 3
    assert vol > 0 and abs(vol - exact) <= 0.01 * exact, (vol, exact)
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - r).max() <= 0.1 * h


def test_numpy_torus_has_euler_characteristic_zero():
    sdf, h = mc_numpy.torus(48)
    v, f = mc_numpy.marching_cubes(sdf, 0.0, (h, h, h), (-1, -1, -1))
    ok, euler, vol = mc_numpy.closed_manifold_stats(v, f)
    assert ok and euler == 0 and vol > 0


# ---- the fp32 vertex arithmetic: the bound against fp64, and inputs that tell a fused last step from the specification ------
# Error of the specification's fp32 vertex against the same formula in fp64 on the same fp32 inputs, u = 2^-24 (round to nearest):
#   t = (level - v0) / (v1 - v0): two subtractions and a division, (1 + u)^3 - 1 <= 3.01 u relative, and 0 <= t <= 1
#   x = p + t (p an exact integer):   3.01 u t + u |x|
#   y = x * spacing:                  (3.01 u t + u |x|) |s| + u |x s| <= u |s| (3.01 + 2 |x|)
#   v = origin + y:                   that + u |v|
# VERTEX_TOL multiplies |s| (3.01 + 2 |x|) + |v|, with 2 % on top for the second-order terms and the fp64 side's own rounding.
VERTEX_TOL = 1.02 * 2.0 ** -24


def _mc_cases():
    """(name, field, level, spacing, origin) of every marching-cubes input whose vertices the GPU tests compare bit for bit with a
    spacing and an origin that make x * spacing inexact."""
    nd = mc_numpy.NON_DYADIC
    yield "non_dyadic", mc_numpy.smooth_field(nd["shape"], nd["seed"]), nd["level"], nd["spacing"], nd["origin"]
    for make, n in ((mc_numpy.sphere, 24), (mc_numpy.sphere, 64), (mc_numpy.torus, 64)):
        sdf, h = make(n)
        yield f"{make.__name__}{n}", sdf, 0.0, (h, h, h), (-1, -1, -1)


def test_fp32_vertices_lie_within_the_rounding_bound_of_fp64():
    from tests import msdiff_numpy
    for name, sdf, level, spacing, origin in _mc_cases():
        v, _ = mc_numpy.marching_cubes(sdf, level, spacing, origin)
        p, a = msdiff_numpy.edges(sdf, level)
        assert np.array_equal(msdiff_numpy.vertices_from_edges(sdf, p, a, level, spacing, origin).view(np.uint32), v.view(np.uint32))
        f = sdf.reshape(-1).astype(np.float64)
        stride = np.array([sdf.shape[1] * sdf.shape[2], sdf.shape[2], 1], dtype=np.int64)
        v0, v1 = f[p], f[p + stride[a]]
        x = np.stack(np.unravel_index(p, sdf.shape), 1).astype(np.float64)
        x[np.arange(len(p)), a] += (np.float64(np.float32(level)) - v0) / (v1 - v0)
        s, o = np.asarray(spacing, np.float32).astype(np.float64), np.asarray(origin, np.float32).astype(np.float64)
        want = o + x * s
        bound = VERTEX_TOL * (np.abs(s) * (3.01 + 2 * np.abs(x)) + np.abs(want))
        err = np.abs(v.astype(np.float64) - want)
        print(f"{name}: {len(v)} vertices, max error / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), name
        assert err.max() > 0, name


def test_a_fused_last_step_shows_on_the_inputs_the_gpu_tests_use():
    """The contracted variant is not the specification: it differs from it in at least a tenth of the coordinates on every input
    above, and in none with origin 0 or a dyadic spacing (where bit-equal vertices would prove nothing about contraction)."""
    for name, sdf, level, spacing, origin in _mc_cases():
        spec, f = mc_numpy.marching_cubes(sdf, level, spacing, origin)
        fused, f2 = mc_numpy.marching_cubes(sdf, level, spacing, origin, contracted=True)
        assert np.array_equal(f, f2)
        d, n = mc_numpy.differing(spec, fused)
        print(f"{name}: {d} of {n} coordinates differ")
        assert d >= 0.1 * n, (name, d, n)
        # ... by no more than the product's rounding error and one rounding of the sum: u |x s| + u |v|, |x s| <= |v| + |origin|
        assert np.abs(spec.astype(np.float64) - fused).max() <= 2.0 ** -23 * (np.abs(spec).max() + np.abs(origin).max())
    nd = mc_numpy.NON_DYADIC
    sdf = mc_numpy.smooth_field(nd["shape"], nd["seed"])
    for spacing, origin in ((nd["spacing"], (0, 0, 0)), ((0.5, 0.25, 2.0), nd["origin"])):
        d, _ = mc_numpy.differing(mc_numpy.marching_cubes(sdf, nd["level"], spacing, origin)[0],
                                  mc_numpy.marching_cubes(sdf, nd["level"], spacing, origin, contracted=True)[0])
        assert d == 0, (spacing, origin, d)


# ---- PLY ----------------------------------------------------------------------------------------------------------------
HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
          b"element face 2\nproperty list uchar int vertex_indices\nend_header\n")


def test_ply_layout_and_round_trip(tmp_path):
    from deepsdf_amd.mesh import write_ply
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.25, -1.5, 3e-7]], dtype=np.float32)
    f = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    p = str(tmp_path / "m.ply")
    write_ply(p, torch.from_numpy(v), torch.from_numpy(f))
    raw = open(p, "rb").read()
    assert raw.startswith(HEADER) and len(raw) == len(HEADER) + 12 * 4 + 13 * 2
    assert raw[len(HEADER) + 48:len(HEADER) + 48 + 13] == b"\x03" + np.array([0, 1, 2], "<i4").tobytes()
    hdr, v2, f2 = mc_numpy.read_ply(p)
    assert hdr.encode() == HEADER and np.array_equal(v2, v) and np.array_equal(f2, f)
    e = str(tmp_path / "empty.ply")
    write_ply(e, torch.empty(0, 3), torch.empty(0, 3, dtype=torch.int32))
    hdr, v3, f3 = mc_numpy.read_ply(e)
    assert open(e, "rb").read() == HEADER.replace(b"vertex 4", b"vertex 0").replace(b"face 2", b"face 0")
    assert v3.shape == (0, 3) and f3.shape == (0, 3)


# ---- grid coordinates of create_mesh ----------------------------------------------------------------------------------------
def _reference_coords(N, start, end):
    """deep_sdf/mesh.py:38-56 restated on the index range [start, end): a float32 [n, 4] samples array."""
    voxel_origin = [-1, -1, -1]
    voxel_size = 2.0 / (N - 1)
    overall_index = torch.arange(start, end, 1, out=torch.LongTensor())
    samples = torch.zeros(end - start, 4)
    samples[:, 2] = overall_index % N
    samples[:, 1] = (overall_index.long() // N) % N
    samples[:, 0] = ((overall_index.long() // N) // N) % N
    samples[:, 0] = (samples[:, 0] * voxel_size) + voxel_origin[2]
    samples[:, 1] = (samples[:, 1] * voxel_size) + voxel_origin[1]
    samples[:, 2] = (samples[:, 2] * voxel_size) + voxel_origin[0]
    return samples[:, :3]


@pytest.mark.parametrize("N", [2, 3, 64, 255])
def test_grid_coordinates_equal_the_reference_bit_for_bit(N):
    from deepsdf_amd.mesh import grid_coords
    n, chunk = N ** 3, 1 << 22
    for s in range(0, n, chunk):
        e = min(n, s + chunk)
        ours = grid_coords(N, s, e, (-1, -1, -1), "cpu")
        ref = _reference_coords(N, s, e)
        assert ours.dtype == torch.float32 and torch.equal(ours.view(torch.int32), ref.contiguous().view(torch.int32)), (N, s)
    if N == 3:
        assert grid_coords(N, 0, 27)[:, 0].unique().tolist() == [-1.0, 0.0, 1.0]


# ---- ABI argument checks (no launch) ----------------------------------------------------------------------------------------
def test_mc_arguments_are_refused_before_any_launch(lib):
    b = C.c_size_t()
    assert lib.dsdf_mc_workspace_bytes(2, 2, 2, C.byref(b)) == 0 and b.value > 0
    small = b.value
    assert lib.dsdf_mc_workspace_bytes(256, 256, 256, C.byref(b)) == 0
    assert 256 ** 3 * 6 <= b.value < 256 ** 3 * 6.2
    for dims in ((1, 8, 8), (8, 0, 8), (8, 8, -3), (1025, 8, 8), (8, 8, 1025)):
        assert lib.dsdf_mc_workspace_bytes(*dims, C.byref(b)) == -1, dims
        assert b"outside" in lib.dsdf_last_error()
    assert lib.dsdf_mc_workspace_bytes(1024, 1024, 1024, C.byref(b)) == 0
    assert lib.dsdf_mc_workspace_bytes(8, 8, 8, None) == -1
    fake = C.c_void_p(1 << 20)         # never dereferenced: every call below is refused before a launch
    sp, org = (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0)
    assert lib.dsdf_mc_count(None, 8, 8, 8, 0.0, fake, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_count(fake, 8, 8, 8, 0.0, None, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_count(fake, 8, 8, 8, 0.0, fake, None, 1 << 30, None) == -1
    assert lib.dsdf_mc_count(fake, 2000, 8, 8, 0.0, fake, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_count(fake, 2, 2, 2, 0.0, fake, fake, small - 1, None) == -2
    assert b"workspace" in lib.dsdf_last_error()
    assert lib.dsdf_mc_emit(fake, 8, 8, 8, 0.0, sp, org, 10, 10, None, fake, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_emit(fake, 8, 8, 8, 0.0, sp, org, 10, 10, fake, None, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_emit(fake, 8, 8, 8, 0.0, None, org, 10, 10, fake, fake, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_emit(fake, 8, 8, 8, 0.0, sp, org, 2 ** 31, 10, fake, fake, fake, 1 << 30, None) == -1
    assert b"int32" in lib.dsdf_last_error()
    assert lib.dsdf_mc_emit(fake, 8, 8, 8, 0.0, sp, org, 10, 2 ** 31, fake, fake, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_emit(fake, 8, 8, 8, 0.0, sp, org, -1, 10, fake, fake, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_emit(fake, 2, 2, 2, 0.0, sp, org, 10, 10, fake, fake, fake, small - 1, None) == -2
    assert lib.dsdf_mc_emit(fake, 0, 2, 2, 0.0, sp, org, 10, 10, fake, fake, fake, 1 << 30, None) == -1
    assert lib.dsdf_mc_emit(fake, 8, 8, 8, 0.0, sp, org, 0, 0, None, None, fake, 1 << 30, None) == 0   # empty: nothing to do
    w = C.c_int32()
    assert lib.dsdf_mc_case_table(None, 0, None) == -1
    assert lib.dsdf_mc_case_table(None, 0, C.byref(w)) == 0 and w.value == mc_table.WIDTH
    buf = (C.c_int8 * (256 * w.value))()
    assert lib.dsdf_mc_case_table(buf, 256 * w.value - 1, C.byref(w)) == -1


def test_deep_sdf_mesh_shim_and_cli_are_importable():
    import deep_sdf.mesh
    from deepsdf_amd import mesh
    assert deep_sdf.mesh.create_mesh is mesh.create_mesh
    assert deep_sdf.mesh.convert_sdf_samples_to_ply is mesh.convert_sdf_samples_to_ply
    import importlib.util
    spec = importlib.util.spec_from_file_location("cpfl", os.path.join(ROOT, "create_ply_files_from_latent.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert callable(m.main)
