"""The tetrahedral mesher's specification, checked on its numpy restatement (tests/tet_numpy.py), and the host side of its ABI:
conformity, orientation, the directly emitted boundary, convergence, components, argument errors, the MFEM writer.  No device."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from deepsdf_amd import _lib
from tests import mc_numpy, tet_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def grid_a():
    return np.random.default_rng(1).uniform(-1, 1, (6, 5, 4)).astype(np.float32)


@pytest.fixture(scope="module")
def mesh_a():
    stats = {}
    return tet_numpy.tetrahedralize(grid_a(), stats=stats), stats


def _volume_identity(m):
    vol, surf, bound = tet_numpy.check_invariants(m)
    print(f"sum of element volumes {vol!r}, boundary volume {surf!r}, |difference| {abs(vol - surf):.3e}, bound {bound:.3e}")
    assert abs(vol - surf) <= bound
    return vol


def test_grid_a_meets_every_case_and_the_specification_counts(mesh_a):
    m, stats = mesh_a
    assert stats["cases"] == {(pi, mask) for pi in range(6) for mask in range(16)}        # all 96 (permutation, inside mask) pairs
    assert stats["diagonal"] == {True, False}                                              # both diagonals of the pyramid's base
    assert (len(m.verts), len(m.tets), len(m.bfaces)) == (339, 726, 668)
    assert tet_numpy.counts(grid_a()) == (339, 726, 668)
    assert m.verts.dtype == np.float32 and len(m.vert_point) == len(m.vert_class) == 339


def test_grid_a_is_positive_conforming_and_closed(mesh_a):
    _volume_identity(mesh_a[0])


def test_grid_a_axis_vertices_are_marching_cubes_vertices(mesh_a):
    m = mesh_a[0]
    mv = mc_numpy.vertices(grid_a())
    sel = np.isin(m.vert_class, [1, 2, 4])
    assert np.array_equal(m.verts[sel].view(np.uint32), mv.view(np.uint32))
    grid = m.vert_class == 0                                                               # a grid vertex sits on its grid point
    assert np.array_equal(m.verts[grid], np.stack(np.unravel_index(m.vert_point[grid], (6, 5, 4)), 1).astype(np.float32))


def test_solid_and_complement_fill_the_box_in_fp64():
    g = grid_a()
    a = tet_numpy.tetrahedralize(g, dtype=np.float64)
    b = tet_numpy.tetrahedralize(-g, dtype=np.float64)
    assert a.verts.dtype == np.float64
    va, vb = tet_numpy.volumes(a.verts, a.tets), tet_numpy.volumes(b.verts, b.tets)
    bound = tet_numpy.volume_bound(a.verts, a.tets, a.bfaces) + tet_numpy.volume_bound(b.verts, b.tets, b.bfaces)
    print(f"volume(g) + volume(-g) - box = {va.sum() + vb.sum() - 60.0:.3e}, bound {bound:.3e}")
    assert abs(va.sum() + vb.sum() - 5 * 4 * 3) <= bound


@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 2, 2)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_cell_thick_grids_touch_every_outer_plane(shape, seed):
    g = np.random.default_rng(seed).uniform(-1, 1, shape).astype(np.float32)
    m = tet_numpy.tetrahedralize(g, 0.25, (0.3, 0.7, 1.1), (-0.9, 0.1, 0.35))
    _volume_identity(m)
    assert set(m.bface_kind.tolist()) == {0, 1, 2, 3, 4, 5, 6}
    assert tet_numpy.counts(g, 0.25) == (len(m.verts), len(m.tets), len(m.bfaces))
    v = m.verts[m.bfaces.astype(np.int64)]                                                 # a plane face lies in its plane, facing out
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(np.float64)
    for kind in range(1, 7):
        axis, sign = (kind - 1) // 2, 1 if kind % 2 == 0 else -1
        sel = m.bface_kind == kind
        assert (n[sel][:, axis] * sign > 0).all() and (n[sel][:, [a for a in range(3) if a != axis]] == 0).all()


def test_t_clamp_keeps_every_element_off_zero_and_zero_is_no_clamp():
    g = grid_a()
    g[2, 2, 2] = 0.0                                          # a value equal to the level: outside, t = 1 on the edges towards it
    m0 = tet_numpy.tetrahedralize(g)
    v0 = tet_numpy.volumes(m0.verts, m0.tets)
    assert (v0 >= 0).all() and (v0 == 0).any()                # the degenerate input the specification documents
    tet_numpy.check_invariants(m0, positive=False)
    mc = tet_numpy.tetrahedralize(g, t_clamp=0.05)
    assert np.array_equal(mc.tets, m0.tets) and np.array_equal(mc.bfaces, m0.bfaces)
    _volume_identity(mc)                                      # every element positive again
    ma = tet_numpy.tetrahedralize(grid_a(), t_clamp=0.0)
    mb = tet_numpy.tetrahedralize(grid_a())
    assert ma.verts.tobytes() == mb.verts.tobytes()


def test_sphere_volume_converges_at_second_order():
    err = []
    for N in (9, 17, 33):
        x = np.linspace(-1, 1, N)
        X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
        h = 2.0 / (N - 1)
        m = tet_numpy.tetrahedralize((np.sqrt(X * X + Y * Y + Z * Z) - 0.6).astype(np.float32), 0.0, (h, h, h), (-1, -1, -1))
        err.append(abs(tet_numpy.volumes(m.verts, m.tets).sum() - 4 / 3 * math.pi * 0.6 ** 3))
    print("sphere volume errors at N = 9, 17, 33:", err)
    assert err[0] > 3 * err[1] and err[1] > 3 * err[2]


# ---- components ---------------------------------------------------------------------------------------------------------------
def serpentine():
    """(12, 12, 2): even rows inside, odd rows outside except one connector at alternating ends: one winding component."""
    g = np.ones((12, 12, 2), dtype=np.float32)
    g[0::2] = -1
    for r in range(1, 12, 2):
        g[r, 0 if (r // 2) % 2 == 0 else 11] = -1
    return g


def diagonal_pairs():
    """Two pairs of inside points in one z layer: across (+1, -1, 0), no Kuhn edge, and across (+1, +1, 0), a class-3 edge."""
    g = np.ones((6, 6, 2), dtype=np.float32)
    g[0, 1, 0] = g[1, 0, 0] = -1
    g[3, 3, 0] = g[4, 4, 0] = -1
    return g


COMPONENT_CASES = {"random": lambda: np.random.default_rng(3).uniform(-1, 1, (9, 8, 7)).astype(np.float32),
                   "serpentine": serpentine, "diagonals": diagonal_pairs}


def test_components_random_grid_against_a_flood_fill():
    g = COMPONENT_CASES["random"]()
    label, size = tet_numpy.components(g)
    ins = (g < 0).reshape(-1)
    assert (label[~ins] == -1).all() and (label[ins] >= 0).all() and size.sum() == ins.sum()
    seen = np.full(g.size, -1)
    idx = np.arange(g.size).reshape(g.shape)
    dirs = [tuple(s * d for d in (c & 1, (c >> 1) & 1, (c >> 2) & 1)) for c in range(1, 8) for s in (1, -1)]
    for start in np.nonzero(ins)[0]:                            # an independent restatement: flood fill from the lowest index
        if seen[start] >= 0:
            continue
        stack, seen[start] = [start], start
        while stack:
            i, j, k = np.unravel_index(stack.pop(), g.shape)
            for d in dirs:
                q = (i + d[0], j + d[1], k + d[2])
                if all(0 <= q[a] < g.shape[a] for a in range(3)) and ins[idx[q]] and seen[idx[q]] < 0:
                    seen[idx[q]] = start
                    stack.append(idx[q])
    assert np.array_equal(label, seen.astype(np.int32))
    roots = np.unique(label[ins])
    assert np.array_equal(size[roots], np.array([(label == r).sum() for r in roots])) and len(roots) > 1


def test_components_serpentine_is_one_component():
    g = serpentine()
    label, size = tet_numpy.components(g)
    ins = (g < 0).reshape(-1)
    assert (label[ins] == 0).all() and size[0] == ins.sum() and (size[1:] == 0).all()


def test_components_follow_the_kuhn_diagonals_only():
    g = diagonal_pairs()
    label, _ = tet_numpy.components(g)
    lab = label.reshape(g.shape)
    assert lab[0, 1, 0] != lab[1, 0, 0]                        # (+1, -1, 0) is no Kuhn edge
    assert lab[3, 3, 0] == lab[4, 4, 0] == np.ravel_multi_index((3, 3, 0), g.shape)
    m = tet_numpy.tetrahedralize(g)                             # and the mesh agrees: three solids
    tet_numpy.check_invariants(m)


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_every_declared_tet_symbol_is_exported_and_bound():
    names = sorted(set(re.findall(r"\b(dsdf_tet_\w+)\s*\(", open(os.path.join(ROOT, "include", "dsdf.h")).read())))
    assert names == ["dsdf_tet_components", "dsdf_tet_count", "dsdf_tet_emit", "dsdf_tet_workspace_bytes"]
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n) and n in _lib.PROTOTYPES
    assert lib.dsdf_abi_version() == 19


def test_argument_errors_come_before_any_launch():
    lib = _lib.lib()
    bad, short = -1, -2
    p, null = C.c_void_p(0x1000), C.c_void_p(0)              # never dereferenced: every call below fails before a launch
    b = C.c_size_t()
    assert lib.dsdf_tet_workspace_bytes(9, 8, 7, C.byref(b)) == 0
    assert 11 * 504 <= b.value <= 11 * 504 + 16 * 256 + 6 * 8 * 3      # about 11 bytes per point + alignment of the small regions
    assert lib.dsdf_tet_workspace_bytes(9, 8, 7, None) == bad
    sp = (C.c_float * 3)(1, 1, 1)
    big = 1 << 20
    rounds = C.c_int32(-5)

    def count(nx=9, ny=8, nz=7, sdf=p, totals=p, ws=p, nbytes=big):
        return lib.dsdf_tet_count(sdf, nx, ny, nz, 0.0, totals, ws, nbytes, null)

    def emit(nx=9, ny=8, nz=7, sdf=p, t_clamp=0.0, nv=10, nt=10, nb=10, verts=p, tets=p, bf=p, kind=p, ws=p, nbytes=big, spacing=sp):
        return lib.dsdf_tet_emit(sdf, nx, ny, nz, 0.0, spacing, sp, t_clamp, nv, nt, nb, verts, tets, bf, kind, null, null, ws, nbytes, null)

    def comps(nx=9, ny=8, nz=7, sdf=p, label=p, ws=p, nbytes=big):
        return lib.dsdf_tet_components(sdf, nx, ny, nz, 0.0, label, p, C.byref(rounds), ws, nbytes, null)

    for f in (count, emit, comps):
        assert f(nx=1) == bad and f(ny=1) == bad and f(nz=1) == bad
        assert f(nx=1025) == bad and f(ny=1025) == bad and f(nz=1025) == bad
        assert f(sdf=null) == bad and f(ws=null) == bad
        assert f(nbytes=b.value - 1) == short
    assert lib.dsdf_tet_workspace_bytes(1, 8, 7, C.byref(b)) == bad and lib.dsdf_tet_workspace_bytes(9, 8, 1025, C.byref(b)) == bad
    assert count(totals=null) == bad
    assert comps(label=null) == bad and rounds.value == 0
    assert emit(t_clamp=-0.1) == bad and emit(t_clamp=0.5) == bad and emit(t_clamp=float("nan")) == bad
    for k in ("nv", "nt", "nb"):
        assert emit(**{k: 2 ** 31}) == bad and emit(**{k: -1}) == bad
    assert b"int32" in lib.dsdf_last_error() or b"boundary" in lib.dsdf_last_error()
    assert emit(verts=null) == bad and emit(tets=null) == bad and emit(bf=null) == bad and emit(kind=null) == bad
    assert emit(spacing=None) == bad
    assert emit(tets=C.c_void_p(0x1004)) == bad and b"aligned" in lib.dsdf_last_error()      # an element is stored as one int4
    assert emit(nv=0, nt=0, nb=0, verts=null, tets=null, bf=null, kind=null) == 0          # nothing to write: no launch


@pytest.mark.parametrize("first", ["deepsdf_amd.tetmesh", "deepsdf_amd.mesh", "deep_sdf.mesh", "analysis.geometry"])
def test_either_module_can_be_imported_first(first):
    """deepsdf_amd.mesh re-exports deepsdf_amd.tetmesh: a fresh interpreter may meet them in any order."""
    code = (f"import {first} as a; import deepsdf_amd.tetmesh as t, deepsdf_amd.mesh as m; "
            "assert m.tetrahedralize is t.tetrahedralize and m.TetMesh is t.TetMesh and m.solid_components is t.solid_components; "
            "from deepsdf_amd.tetmesh import tetrahedralize, TetMesh, solid_components")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_needs_a_device_grid():
    import torch
    from deepsdf_amd.mesh import solid_components, tetrahedralize
    g = torch.zeros(4, 4, 4)
    with pytest.raises(_lib.DsdfError):
        tetrahedralize(g)
    with pytest.raises(_lib.DsdfError):
        solid_components(g)
    with pytest.raises(ValueError):
        tetrahedralize(g, t_clamp=0.5)


# ---- MFEM -----------------------------------------------------------------------------------------------------------------------
def read_mfem(path):
    """A small parser of the MFEM mesh v1.0 files write_mfem writes: (elements [T, 6], boundary [M, 5], vertices [V, 3] fp32)."""
    lines = [ln.strip() for ln in open(path).read().splitlines()]
    assert lines[0] == "MFEM mesh v1.0"
    body = [ln for ln in lines[1:] if ln and not ln.startswith("#")]
    at = {name: body.index(name) for name in ("dimension", "elements", "boundary", "vertices")}
    assert at["dimension"] < at["elements"] < at["boundary"] < at["vertices"] and body[at["dimension"] + 1] == "3"

    def block(name, skip, dtype):
        n = int(body[at[name] + 1])
        rows = body[at[name] + 1 + skip:at[name] + 1 + skip + n]
        assert len(rows) == n
        return np.array([r.split() for r in rows], dtype=dtype).reshape(n, -1)
    assert body[at["vertices"] + 2] == "3"
    el, bd, vx = block("elements", 1, np.int64), block("boundary", 1, np.int64), block("vertices", 2, np.float32)
    assert at["vertices"] + 3 + len(vx) == len(body)
    return el, bd, vx


def reference_attributes(verts, bfaces, tolerance=3e-2):
    """The 1 / 2 / 3 rule of the reference's export_volume_mesh, one triangle at a time."""
    height = verts[:, 2].max()
    out = []
    for f in bfaces:
        if np.max(verts[f, 0]) < tolerance:
            out.append(1)
        elif np.max(verts[f, 2]) > height - tolerance:
            out.append(2)
        else:
            out.append(3)
    return np.array(out)


def test_write_mfem_round_trip_without_a_device(mesh_a, tmp_path):
    from deepsdf_amd.mesh import TetMesh
    m = mesh_a[0]
    tm = TetMesh(m.verts, m.tets, m.bfaces, m.bface_kind)
    assert tm.device.type == "cpu" and (tm.n_verts, tm.n_tets, tm.n_bfaces) == (339, 726, 668)
    path = str(tmp_path / "a.mesh")
    tm.write_mfem(path)
    el, bd, vx = read_mfem(path)
    assert el.shape == (726, 6) and bd.shape == (668, 5) and vx.shape == (339, 3)
    assert (el[:, 0] == 1).all() and (el[:, 1] == 4).all() and (bd[:, 1] == 2).all()          # geometry codes: tetrahedron, triangle
    assert el[:, 2:].min() >= 0 and el[:, 2:].max() < 339 and bd[:, 2:].min() >= 0 and bd[:, 2:].max() < 339
    assert np.array_equal(el[:, 2:], m.tets) and np.array_equal(bd[:, 2:], m.bfaces)
    assert np.array_equal(vx.view(np.uint32), m.verts.view(np.uint32))
    want = reference_attributes(m.verts, m.bfaces.astype(np.int64))
    assert np.array_equal(bd[:, 0], want) and set(want.tolist()) == {1, 2, 3}
    assert np.array_equal(tm.boundary_attributes().numpy(), want)
    assert np.allclose(tm.volumes().numpy(), tet_numpy.volumes(m.verts, m.tets), rtol=1e-12, atol=0) and tm.volume() > 0
    t2 = tm.transformed((2.0, 1.0, 0.5), (1.0, 0.0, -1.0))
    assert np.isclose(t2.volume(), tm.volume(), rtol=1e-5)
    tm.write_mfem(path, attributes=np.full(668, 7))
    assert (read_mfem(path)[1][:, 0] == 7).all()
    with pytest.raises(ValueError):
        tm.write_mfem(path, attributes=[1, 2])


# ---- signatures -----------------------------------------------------------------------------------------------------------------
def test_reference_signatures_stay_and_the_new_methods_exist():
    import deep_sdf.mesh as dm
    from analysis.geometry import DeepSDFMesh
    from deepsdf_amd import mesh
    a = list(inspect.signature(mesh.create_mesh_microstructure).parameters)
    assert a == ["tiling", "decoder", "latent_vec_interpolation", "filename", "N", "max_batch", "offset", "scale", "cap_border_dict",
                 "save_ply_file", "use_flexicubes", "device", "output_tetmesh", "compute_derivatives"]
    b = list(inspect.signature(mesh.create_mesh_microstructure_diff).parameters)
    assert b == ["tiling", "decoder", "latent_vec_interpolation", "N", "max_batch", "offset", "scale", "cap_border_dict", "device",
                 "output_tetmesh", "compute_derivatives"]
    assert list(inspect.signature(DeepSDFMesh.generate_volume_mesh).parameters) == ["self", "t_clamp"]
    assert list(inspect.signature(DeepSDFMesh.export_mfem_mesh).parameters) == ["self", "filename"]
    s = inspect.signature(mesh.tetrahedralize)
    assert list(s.parameters) == ["sdf_grid", "level", "spacing", "origin", "t_clamp", "keep_largest", "return_edges"]
    assert [p.kind for p in s.parameters.values()][4:] == [inspect.Parameter.KEYWORD_ONLY] * 3
    for name in ("tetrahedralize", "solid_components", "TetMesh"):
        assert getattr(dm, name) is getattr(mesh, name)
