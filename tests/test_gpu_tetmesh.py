"""-m gpu: the HIP tetrahedral mesher (dsdf_tet_*, csrc/tetmesh.hpp) against the numpy restatement of tests/tet_numpy.py, array for
array; the mesh invariants on device results; the solid's components; the workspace's red zones; DeepSDFMesh's volume stage and the
command line end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deepsdf_amd import _lib
from tests import mc_numpy, tet_numpy
from tests import ws_guard as G
from tests.test_tetmesh_cpu import COMPONENT_CASES, grid_a, read_mfem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACING, ORIGIN = (0.3, 0.7, 1.1), (-0.9, 0.1, 0.35)          # not dyadic on any axis: x * spacing is inexact
GRIDS = {"A": grid_a, "2x2x2": lambda: np.random.default_rng(7).uniform(-1, 1, (2, 2, 2)).astype(np.float32),
         "3x2x2": lambda: np.random.default_rng(7).uniform(-1, 1, (3, 2, 2)).astype(np.float32),
         "9x8x7": lambda: np.random.default_rng(7).uniform(-1, 1, (9, 8, 7)).astype(np.float32)}       # 504 points: two workgroups
FIELDS = ("verts", "tets", "bfaces", "bface_kind", "vert_point", "vert_class")


def _gpu(grid, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0), **kw):
    from deepsdf_amd.mesh import tetrahedralize
    m = tetrahedralize(torch.as_tensor(grid).cuda(), level, spacing, origin, return_edges=True, **kw)
    assert m.verts.dtype == torch.float32 and m.tets.dtype == torch.int32 and m.bfaces.dtype == torch.int32
    assert m.bface_kind.dtype == torch.int8 and m.vert_point.dtype == torch.int64 and m.vert_class.dtype == torch.int32
    assert all(getattr(m, f).is_cuda for f in FIELDS)
    return m


def _host(m):
    return {f: getattr(m, f).cpu().numpy() for f in FIELDS}


def _same_as_oracle(what, m, r):
    h = _host(m)
    for f in FIELDS[1:]:
        assert h[f].shape == getattr(r, f).shape and np.array_equal(h[f], getattr(r, f)), (what, f)
    d, n = mc_numpy.differing(h["verts"], r.verts)
    if d:
        print(f"{what}: {d} of {n} coordinates differ from the single-rounded specification, by at most "
              f"{mc_numpy.ulp_distance(h['verts'], r.verts)} ulp")
    assert d == 0, (what, d, n)
    return h


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("name", list(GRIDS))
def test_bit_for_bit_against_the_oracle_and_marching_cubes(name, level):
    from deepsdf_amd.mesh import marching_cubes
    g = GRIDS[name]()
    r = tet_numpy.tetrahedralize(g, level, SPACING, ORIGIN)
    d, n = mc_numpy.differing(r.verts, tet_numpy.vertices(g, level, SPACING, ORIGIN, contracted=True)[0])
    print(f"{name} level {level}: a fused last step would change {d} of {n} coordinates")
    assert d > 0 and (n < 1000 or d >= 0.1 * n)                 # the input tells a fused origin + x * spacing from the specification
    h = _same_as_oracle(f"{name} level {level}", _gpu(g, level, SPACING, ORIGIN), r)
    assert len(h["tets"]) > 0 and len(h["bfaces"]) > 0
    mv = marching_cubes(torch.from_numpy(g).cuda(), level, SPACING, ORIGIN)[0].cpu().numpy()
    axis = h["verts"][np.isin(h["vert_class"], [1, 2, 4])]
    assert axis.shape == mv.shape and np.array_equal(axis.view(np.uint32), mv.view(np.uint32))
    # the clamp: the oracle's bits again, every element positive; and t_clamp = 0 is the default call's bytes
    rc = tet_numpy.tetrahedralize(g, level, SPACING, ORIGIN, t_clamp=0.05)
    hc = _same_as_oracle(f"{name} level {level} clamped", _gpu(g, level, SPACING, ORIGIN, t_clamp=0.05), rc)
    assert (tet_numpy.volumes(hc["verts"], hc["tets"]) > 0).all()
    h0 = _host(_gpu(g, level, SPACING, ORIGIN, t_clamp=0.0))
    assert all(h0[f].tobytes() == h[f].tobytes() for f in FIELDS)


def _volume_identity(what, m):
    surf = m.boundary_surface()
    assert surf.is_watertight and surf.is_winding_consistent
    bound = tet_numpy.volume_bound(m.verts.cpu().numpy(), m.tets.cpu().numpy(), m.bfaces.cpu().numpy())
    vol, sv = m.volume(), surf.volume()
    print(f"{what}: sum of element volumes {vol!r}, boundary volume {sv!r}, |difference| {abs(vol - sv):.3e}, bound {bound:.3e}")
    assert abs(vol - sv) <= bound
    return surf


def test_sphere_invariants_on_the_device_result():
    N = 24
    x = torch.linspace(-1, 1, N, dtype=torch.float64, device="cuda")
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    h = 2.0 / (N - 1)
    m = _gpu((torch.sqrt(X * X + Y * Y + Z * Z) - 0.6).float(), 0.0, (h, h, h), (-1, -1, -1))
    surf = _volume_identity("sphere N = 24", m)
    assert surf.n_components == 1 and bool((m.volumes() > 0).all()) and bool((m.bface_kind == 0).all())
    assert abs(m.volume() - 4 / 3 * np.pi * 0.6 ** 3) < 0.02


def test_more_than_one_scan_block():
    """(132, 128, 128): 8448 workgroup totals, more than the 8192 the scan takes per iteration; the sphere straddles the border."""
    c = G.constants()
    dims = (132, 128, 128)
    assert dims[0] * dims[1] * dims[2] // c["TET_BLOCK"] > c["MC_SCAN_THREADS"] * c["MC_SCAN_PER_THREAD"]
    i, j, k = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device="cuda") for n in dims], indexing="ij")
    g = torch.sqrt((i - 125.25) ** 2 + (j - 64.5) ** 2 + (k - 63.75) ** 2) - 6.0
    del i, j, k
    m = _gpu(g)
    assert (m.n_verts, m.n_tets, m.n_bfaces) == tet_numpy.counts(g.cpu().numpy())
    assert int(m.vert_point.min()) < 128 * 128 * 128 <= int(m.vert_point.max())      # vertices on both sides of the scan's border
    _volume_identity("sphere across the scan border", m)
    assert int(m.tets.min()) == 0 and int(m.tets.max()) == m.n_verts - 1 and bool((m.volumes() > 0).all())


# ---- components ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(COMPONENT_CASES))
def test_components_against_the_union_find(name):
    """Labels and sizes are unique and compared exactly.  The number of rounds depends on the order the atomics land in, so it has
    no single oracle value; the oracle bounds it: at least 1, more than 1 where one sweep cannot carry the lowest label to the far
    end, and at most the deepest component's depth from its root plus the round that sees no change (tet_numpy.component_depth)."""
    from deepsdf_amd.mesh import solid_components
    g = COMPONENT_CASES[name]()
    label, size, rounds = solid_components(torch.from_numpy(g).cuda())
    rl, rs = tet_numpy.components(g)
    assert label.dtype == torch.int32 and size.dtype == torch.int32 and label.shape == g.shape
    assert np.array_equal(label.cpu().numpy().reshape(-1), rl) and np.array_equal(size.cpu().numpy().reshape(-1), rs)
    print(f"components {name}: {int((rs > 0).sum())} components, {rounds} rounds")
    depth = tet_numpy.component_depth(g)
    print(f"components {name}: depth {depth}")
    assert 1 <= rounds <= depth + 1
    if name == "serpentine":
        assert depth > 40                                       # the solid winds: a long way from the root to the far end
        assert rounds > 1 and int((rs > 0).sum()) == 1


def test_keep_largest_is_the_large_solid_alone_bit_for_bit():
    i, j, k = np.meshgrid(np.arange(24.0), np.arange(16.0), np.arange(16.0), indexing="ij")
    big = (np.sqrt((i - 6.3) ** 2 + (j - 6.6) ** 2 + (k - 6.9) ** 2) - 5.0).astype(np.float32)
    small = (np.sqrt((i - 20.2) ** 2 + (j - 12.4) ** 2 + (k - 12.6) ** 2) - 2.5).astype(np.float32)
    both = np.minimum(big, small)
    assert int((tet_numpy.components(both)[1] > 0).sum()) == 2
    kept = _host(_gpu(both, 0.0, SPACING, ORIGIN, keep_largest=True))
    alone = _host(_gpu(big, 0.0, SPACING, ORIGIN))
    whole = _host(_gpu(both, 0.0, SPACING, ORIGIN))
    assert len(whole["tets"]) > len(kept["tets"]) > 0
    assert all(kept[f].tobytes() == alone[f].tobytes() for f in FIELDS)


# ---- memory safety and determinism --------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes_inside_their_regions():
    lib = _lib.lib()
    g = torch.from_numpy(GRIDS["9x8x7"]()).cuda()
    shape = tuple(g.shape)
    sp, org = (C.c_float * 3)(*SPACING), (C.c_float * 3)(*ORIGIN)
    with G.redzone():
        outs = []
        for fill in (0x00, 0xFF):
            b = C.c_size_t()
            _lib.check(lib.dsdf_tet_workspace_bytes(*shape, C.byref(b)))
            ws, F = G.poisoned(b.value, fill), G.Fences()
            totals = F.new("totals", 3, torch.int64)
            _lib.check(lib.dsdf_tet_count(G.ptr(g), *shape, 0.0, G.ptr(totals), G.ptr(ws), ws.numel(), G.stream()))
            rows, _ = G.assert_clean(ws, fill, f"tet count fill {fill:#x}")
            assert {r[0] for r in rows} == {"tet_rec", "tet_ne", "tet_nb", "tet_vbase", "tet_bv", "tet_bt", "tet_bb", "tet_ov", "tet_ot",
                                            "tet_ob", "tet_cc_gf", "tet_cc_flags"}
            nv, nt, nb = totals.tolist()
            o = dict(verts=F.new("verts", (nv, 3)), tets=F.new("tets", (nt, 4), torch.int32), bfaces=F.new("bfaces", (nb, 3), torch.int32),
                     bface_kind=F.new("bface_kind", nb, torch.int8), vert_point=F.new("vert_point", nv, torch.int64),
                     vert_class=F.new("vert_class", nv, torch.int32))
            _lib.check(lib.dsdf_tet_emit(G.ptr(g), *shape, 0.0, sp, org, 0.0, nv, nt, nb, *[G.ptr(o[f]) for f in FIELDS], G.ptr(ws),
                                         ws.numel(), G.stream()))
            G.assert_clean(ws, fill, f"tet emit fill {fill:#x}")
            o["label"], o["size"] = F.new("label", g.numel(), torch.int32), F.new("size", g.numel(), torch.int32)
            rounds = C.c_int32()
            _lib.check(lib.dsdf_tet_components(G.ptr(g), *shape, 0.0, G.ptr(o["label"]), G.ptr(o["size"]), C.byref(rounds), G.ptr(ws),
                                               ws.numel(), G.stream()))
            G.assert_clean(ws, fill, f"tet components fill {fill:#x}")
            F.check(f"tet mesh fill {fill:#x}")
            # short buffers: nothing is written past them (the first entries are the full run's)
            short = dict(verts=F.new("short verts", (nv - 5, 3)), tets=F.new("short tets", (nt - 7, 4), torch.int32),
                         bfaces=F.new("short bfaces", (nb - 3, 3), torch.int32), bface_kind=F.new("short kind", nb - 3, torch.int8))
            _lib.check(lib.dsdf_tet_emit(G.ptr(g), *shape, 0.0, sp, org, 0.0, nv - 5, nt - 7, nb - 3, G.ptr(short["verts"]),
                                         G.ptr(short["tets"]), G.ptr(short["bfaces"]), G.ptr(short["bface_kind"]), None, None, G.ptr(ws),
                                         ws.numel(), G.stream()))
            F.check(f"tet mesh short buffers fill {fill:#x}")
            for f in short:
                assert torch.equal(short[f], o[f][:short[f].shape[0]])
            outs.append({f: t.cpu().numpy().tobytes() for f, t in o.items()})
        assert outs[0] == outs[1]
    r = tet_numpy.tetrahedralize(GRIDS["9x8x7"](), 0.0, SPACING, ORIGIN)
    assert outs[0]["tets"] == r.tets.tobytes() and outs[0]["verts"] == r.verts.tobytes()


def test_empty_and_full_grids():
    m = _gpu(np.ones((5, 4, 3), dtype=np.float32))
    assert m.verts.shape == (0, 3) and m.tets.shape == (0, 4) and m.bfaces.shape == (0, 3) and m.bface_kind.shape == (0,)
    m = _gpu(np.zeros((4, 4, 4), dtype=np.float32))              # a value equal to the level is outside
    assert m.n_verts == 0 and m.n_tets == 0 and m.n_bfaces == 0 and m.volume() == 0.0
    g = -np.ones((3, 3, 3), dtype=np.float32)
    m = _gpu(g)
    assert (m.n_verts, m.n_tets, m.n_bfaces) == (27, 48, 48) and bool((m.bface_kind >= 1).all())
    assert sorted(np.bincount(m.bface_kind.cpu().numpy(), minlength=7).tolist()) == [0, 8, 8, 8, 8, 8, 8]
    _same_as_oracle("full 3x3x3", m, tet_numpy.tetrahedralize(g))
    assert abs(m.volume() - 8.0) < 1e-12
    _volume_identity("full 3x3x3", m)


# ---- DeepSDFMesh and the command line ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("remove_orphans", [True, False])
def test_deepsdfmesh_volume_mesh_on_an_experiment_directory(tmp_path, remove_orphans):
    from analysis.geometry import STRETCH, DeepSDFMesh
    from deepsdf_amd.mesh import TetMesh, default_cap_border_dict, solid_components
    from deepsdf_amd.tetmesh import largest_component_only
    from tests.test_gpu_microstructure import _tiny_experiment
    exp = _tiny_experiment(str(tmp_path))
    options = dict(experiment_directory=exp, checkpoint="latest", degrees=[1, 1, 1], refinement=1, cap_border_dict=default_cap_border_dict(),
                   N_base_reconstruction=6, tiling=[2, 1, 1], remove_orphans=remove_orphans)
    dm = DeepSDFMesh(options)
    with pytest.raises(RuntimeError):
        dm.generate_volume_mesh()
    with pytest.raises(RuntimeError):
        dm.export_mfem_mesh(str(tmp_path / "early.mesh"))
    dm.generate_surface_mesh(np.tile(dm.latent[0], (27, 1)))
    vm = dm.generate_volume_mesh()
    assert vm is dm.volume_mesh and isinstance(vm, TetMesh) and vm.n_tets > 0 and vm.verts.dtype == torch.float64
    # caps put grid values on or next to the level: without a clamp such elements are thinner than the fp32 rounding of their
    # vertices and their computed volume is zero or of either sign at that scale; with one every element is positive
    worst = float(vm.volumes().min())
    print(f"remove_orphans={remove_orphans}: smallest element volume without a clamp {worst:.3e}")
    assert worst > -1e-12 * vm.volume()
    assert bool((dm.generate_volume_mesh(t_clamp=0.05).volumes() > 0).all())
    vm = dm.generate_volume_mesh()
    # the volume lies between the cells that are inside at all eight corners and the cells that are inside at any
    grid = largest_component_only(dm.diff.grid) if remove_orphans else dm.diff.grid
    ins = grid < 0
    nx, ny, nz = ins.shape
    corners = torch.stack([ins[a:nx - 1 + a, b:ny - 1 + b, c:nz - 1 + c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    cell = float(np.prod([v / 2 * s for v, s in zip(dm.diff.voxel_size, STRETCH)]))
    lower, upper = float(corners.all(0).sum()) * cell, float(corners.any(0).sum()) * cell
    print(f"remove_orphans={remove_orphans}: {vm.n_tets} elements, volume {vm.volume():.6f} in [{lower:.6f}, {upper:.6f}]")
    assert vm.volume() > 0 and lower * (1 - 1e-12) <= vm.volume() <= upper * (1 + 1e-12)      # the slack: the fp64 sums' rounding
    # its axis-class boundary vertices are the surface's vertices
    sv = dm.surface_mesh.vertices
    axis = vm.verts[(vm.vert_class == 1) | (vm.vert_class == 2) | (vm.vert_class == 4)].float()
    if not remove_orphans:
        assert torch.equal(axis, sv)
    else:
        assert set(map(tuple, axis.cpu().numpy().tolist())) <= set(map(tuple, sv.cpu().numpy().tolist()))
        assert vm.boundary_surface().n_components == 1
        assert int((solid_components(grid)[1] > 0).sum()) == 1
    path = str(tmp_path / "volume.mesh")
    dm.export_mfem_mesh(path)
    el, bd, vx = read_mfem(path)
    assert el.shape == (vm.n_tets, 6) and bd.shape == (vm.n_bfaces, 5) and vx.shape == (vm.n_verts, 3)
    assert set(np.unique(bd[:, 0]).tolist()) <= {1, 2, 3} and np.array_equal(el[:, 2:], vm.tets.cpu().numpy())
    with pytest.raises(NotImplementedError, match="tetgenpy"):
        dm.tetrahedralize_surface()
    with pytest.raises(NotImplementedError, match="gustaf"):
        dm.export_volume_mesh("unused.mesh")


def test_create_microstructure_cli_writes_the_volume_mesh(tmp_path):
    import deep_sdf.mesh
    import deep_sdf.workspace as ws
    from create_microstructure import uniform_clamped_knots
    from deepsdf_amd.spline import BSplineField
    from tests.test_gpu_microstructure import _tiny_experiment
    exp = _tiny_experiment(str(tmp_path))
    out, mesh = str(tmp_path / "structure.ply"), str(tmp_path / "structure.mesh")
    codes = [0, 1, 2, 3, 4, 5, 6, 8]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_microstructure.py"), "-e", exp, "-c", "latest", "--tiling", "2", "1", "1",
                        "--codes", *[str(c) for c in codes], "--resolution", "16", "--tetmesh", mesh, "--t-clamp", "0.05", "-o", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    el, bd, vx = read_mfem(mesh)
    assert len(el) > 0 and len(bd) > 0 and (el[:, 1] == 4).all() and (bd[:, 1] == 2).all() and el[:, 2:].max() == len(vx) - 1
    decoder = ws.load_trained_model(exp, "latest").eval()
    latent = ws.load_latent_vectors(exp, "latest")
    cp = torch.stack([latent[c].detach().reshape(-1).cpu() for c in codes]).numpy()
    field = BSplineField([1, 1, 1], [uniform_clamped_knots(2, 1)] * 3, cp)
    m = deep_sdf.mesh.microstructure_tetmesh([2, 1, 1], decoder, field, 16, 32 ** 3, None, t_clamp=0.05)
    assert (m.n_verts, m.n_tets, m.n_bfaces) == (len(vx), len(el), len(bd))
    assert np.allclose(vx, m.verts.cpu().numpy(), rtol=0, atol=1e-6)
    # the PLY beside it comes from the same grid and is the file the surface path writes
    deep_sdf.mesh.create_mesh_microstructure([2, 1, 1], decoder, field, str(tmp_path / "surface"), N=16, save_ply_file=True)
    sv, sf = mc_numpy.read_ply(str(tmp_path / "surface.ply"))[1:]
    cv, cf = mc_numpy.read_ply(out)[1:]
    assert np.array_equal(cf, sf) and cv.shape == sv.shape and np.allclose(cv, sv, rtol=0, atol=1e-6) and len(cf) > 0
