"""-m gpu: the surface stage (csrc/meshtopo.hpp, deepsdf_amd/surface.py, analysis/geometry.py) against the numpy oracle of
tests/meshtopo_numpy.py: half-edge mates and edge statistics, component labels, degenerate faces, angle-weighted normals, the volume
and its gradients, the normal projection bit for bit, the workspace under red zones, and the chain from a microstructure mesh to
d volume / d control points."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import meshtopo_numpy as mt
from tests import ws_guard as G

pytestmark = pytest.mark.gpu


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _raw_chain(verts, faces, fill=None):
    """Every dsdf_mt_* entry of a mesh through the C ABI, outputs fenced; fill: the workspace is poisoned with that byte and
    checked after each entry that takes it.  Returns (dict of tensors, rounds)."""
    from deepsdf_amd import _lib
    lib = _lib.lib()
    V = torch.as_tensor(np.asarray(verts, dtype=np.float32)).cuda().contiguous()
    Fi = torch.as_tensor(np.asarray(faces, dtype=np.int32)).cuda().contiguous()
    nv, nf = V.shape[0], Fi.shape[0]
    nb = C.c_size_t()
    _lib.check(lib.dsdf_mt_plan(nv, nf, C.byref(nb)))
    ws = G.poisoned(nb.value, fill) if fill is not None else torch.empty(nb.value + 256, dtype=torch.uint8, device="cuda")
    F = G.Fences()
    o = dict(keys=F.new("keys", 3 * nf, torch.int64), mate=F.new("mate", 3 * nf, torch.int32), stats=F.new("stats", 6, torch.int64),
             label=F.new("label", nf, torch.int32), size=F.new("size", nf, torch.int32), degenerate=F.new("degenerate", nf, torch.uint8),
             normals=F.new("normals", (nv, 3)), vol_grad=F.new("vol_grad", (nv, 3)), volume=F.new("volume", 1, torch.float64))
    st = G.stream()
    _lib.check(lib.dsdf_mt_edge_keys(G.ptr(Fi), nf, nv, G.ptr(o["keys"]), st))
    skeys, order = torch.sort(o["keys"], stable=True)
    _lib.check(lib.dsdf_mt_adjacency(G.ptr(Fi), nf, G.ptr(skeys), G.ptr(order), G.ptr(o["mate"]), G.ptr(o["stats"]), G.ptr(ws), nb.value, st))
    if fill is not None:
        G.assert_clean(ws, fill, f"mt_adjacency, {nf} faces")
    rounds = C.c_int32()
    _lib.check(lib.dsdf_mt_components(G.ptr(o["mate"]), nf, G.ptr(o["label"]), G.ptr(o["size"]), C.byref(rounds), G.ptr(ws), nb.value, st))
    if fill is not None:
        G.assert_clean(ws, fill, f"mt_components, {nf} faces")
    _lib.check(lib.dsdf_mt_face_degenerate(G.ptr(V), nv, G.ptr(Fi), nf, G.ptr(o["degenerate"]), st))
    corners, corder = torch.sort(Fi.reshape(-1).long(), stable=True)
    vstart = torch.searchsorted(corners, torch.arange(nv + 1, device="cuda"))
    _lib.check(lib.dsdf_mt_vertex_geometry(G.ptr(V), nv, G.ptr(Fi), nf, G.ptr(corder), G.ptr(vstart), G.ptr(o["normals"]), G.ptr(o["vol_grad"]), st))
    _lib.check(lib.dsdf_mt_volume(G.ptr(V), nv, G.ptr(Fi), nf, G.ptr(o["volume"]), G.ptr(ws), nb.value, st))
    if fill is not None:
        G.assert_clean(ws, fill, f"mt_volume, {nf} faces")
    F.check(f"dsdf_mt_* chain, {nv} vertices, {nf} faces")
    return o, rounds.value


def _check_topology(o, faces, case):
    mate, stats = mt.adjacency(faces)
    assert np.array_equal(o["keys"].cpu().numpy(), mt.edge_keys(faces)), case
    assert np.array_equal(o["mate"].cpu().numpy(), mate), case
    assert o["stats"].tolist() == mt.stats_list(stats), (case, o["stats"].tolist(), stats)
    label, size = mt.components(mate, len(faces))
    assert np.array_equal(o["label"].cpu().numpy(), label) and np.array_equal(o["size"].cpu().numpy(), size), case
    return stats, label, size


def _check_geometry(o, verts, faces, case):
    """The derived bounds: the device works in fp64 and rounds once, and the oracle's margin (tests/test_meshtopo_cpu.py) keeps the
    difference of two fp64 evaluations below 1e-12."""
    n, ls, wsum, g, gabs = mt.vertex_geometry(verts, faces)
    got_n, got_g = o["normals"].cpu().numpy().astype(np.float64), o["vol_grad"].cpu().numpy().astype(np.float64)
    dn = np.abs(got_n - n)
    zero = ~n.any(1)
    bound_g = 2.0 ** -23 * np.abs(g).max(1) + 1e-12 * gabs
    dg = np.abs(got_g - g).max(1)
    vol, mag = mt.volume(verts, faces)
    dv = abs(float(o["volume"]) - vol)
    print(f"{case}: normals worst {dn.max():.3e} (bound {2.0 ** -23:.3e}), {int(zero.sum())} zero normals; volume gradient worst "
          f"error / bound {float((dg / np.maximum(bound_g, 1e-300)).max()):.3f}; volume {vol:.6f} error {dv:.2e} (bound {1e-12 * mag:.2e})")
    assert dn.max() <= 2.0 ** -23, case
    assert not np.abs(got_n[zero]).any(), case
    assert (dg <= bound_g).all(), case
    assert dv <= 1e-12 * mag, case
    assert np.array_equal(o["degenerate"].cpu().numpy().astype(bool), mt.face_degenerate(verts, faces)), case


# ---- 1. hand-made meshes ----------------------------------------------------------------------------------------------------------
def test_adjacency_and_stats_on_hand_made_meshes():
    from deepsdf_amd.surface import SurfaceMesh
    watertight = {"tetrahedron": (True, True), "minus_one_face": (False, False), "one_face_flipped": (True, False),
                  "share_a_vertex": (True, True), "share_an_edge": (False, False), "duplicated_face": (False, False),
                  "repeated_index": (False, False), "runs_at_both_ends": (False, False)}
    ncc = {"tetrahedron": 1, "minus_one_face": 1, "one_face_flipped": 1, "share_a_vertex": 2, "share_an_edge": 2}
    cases = mt.hand_made()
    assert set(cases) == set(watertight)
    for name, (v, f) in cases.items():
        o, _ = _raw_chain(v, f)
        stats, label, size = _check_topology(o, f, name)
        _check_geometry(o, v, f, name)
        m = SurfaceMesh(v, f)
        assert m.edge_stats() == stats, name
        assert (m.is_watertight, m.is_winding_consistent) == watertight[name], name
        assert m.n_components == int((size > 0).sum()) and m.n_components == ncc.get(name, m.n_components), name
        assert np.array_equal(m.face_labels().cpu().numpy(), label) and np.array_equal(m.half_edge_mates().cpu().numpy(), mt.adjacency(f)[0])
    # the largest component, ties to the lowest label; the faces keep their order and the vertices their ids
    v, f = cases["share_a_vertex"]
    m = SurfaceMesh(v, f)
    big = m.keep_largest_component()
    assert big.V.data_ptr() == m.V.data_ptr() and np.array_equal(big.faces.cpu().numpy(), f[:4]) and big.is_watertight and big.n_components == 1
    v, f = cases["repeated_index"]
    kept = SurfaceMesh(v, f).drop_degenerate_faces()
    assert np.array_equal(kept.faces.cpu().numpy(), f[:4]) and kept.is_winding_consistent
    assert abs(kept.volume() - 1 / 6) < 1e-15
    with pytest.raises(ValueError, match="face indices"):
        SurfaceMesh(v, np.array([[0, 1, 4]]))
    with pytest.raises(ValueError, match="from_diff"):
        kept.volume_gradient()


# ---- 2. block boundaries ----------------------------------------------------------------------------------------------------------
def test_open_strips_around_every_block_size():
    sizes = sorted({v for k, v in G.constants().items() if k.startswith("MT_") and k.endswith("BLOCK")})
    assert sizes, "meshtopo.hpp declares no block size"
    for b in sizes:
        counts = {b - 1, b, b + 1}                               # faces (and, with three half-edges a face, half-edge blocks of 3 b)
        counts |= {(b - 1) // 3, (b - 1) // 3 + 1, b // 3 + 1}     # half-edges: 3 F = b - 1 (or the nearest below), and the first counts above b
        counts |= {b - 3, b - 2}                                 # vertices: 2 ((F + 3) // 2) = b
        for nf in sorted(counts):
            v, f = mt.quad_strip(nf)
            o, _ = _raw_chain(v, f)
            stats, label, size = _check_topology(o, f, f"strip {nf}")
            assert stats["boundary"] == nf + 2 and stats["paired"] == nf - 1 and not label.any() and size[0] == nf
            _check_geometry(o, v, f, f"strip {nf}")


# ---- 3. components ----------------------------------------------------------------------------------------------------------------
def _component_meshes():
    for name, (v, f) in mt.field_meshes().items():
        yield name, len(v), f
    yield "tori 2 x 64 x 64", 2 * 64 * 64, mt.torus_pair(64, 64)
    yield "tori 2 x 16 x 2000", 2 * 16 * 2000, mt.torus_pair(16, 2000)


def test_components_in_order_and_shuffled():
    from deepsdf_amd.surface import SurfaceMesh
    expect = {"two_spheres16": [140, 348], "tori 2 x 64 x 64": [8192, 8192], "tori 2 x 16 x 2000": [64000, 64000], "sphere12": [284]}
    for name, nv, f in _component_meshes():
        verts = torch.zeros(nv, 3, device="cuda")
        mate, stats = mt.adjacency(f)
        label, size = mt.components(mate, len(f))
        if name in expect:
            assert sorted(size[size > 0].tolist()) == expect[name]
        if name == "smooth_9_10_11":
            assert int((mate < 0).sum()) == 120
        perm = np.random.default_rng(len(f)).permutation(len(f))
        for tag, faces, want in (("in order", f, (label, size)), ("shuffled", np.ascontiguousarray(f[perm]), mt.relabel(label, perm))):
            runs = []
            for _ in range(2):
                m = SurfaceMesh(verts, faces)
                runs.append((m.face_labels().cpu().numpy(), m.component_sizes().cpu().numpy()))
            print(f"components {name} {tag}: {len(f)} faces, {m.n_components} components, {m.component_rounds} rounds")
            assert np.array_equal(runs[0][0], want[0]) and np.array_equal(runs[0][1], want[1]), (name, tag)
            assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes(), (name, tag)
            assert m.edge_stats() == stats, (name, tag)
            assert m.n_components == int((size > 0).sum())
            big = m.keep_largest_component()
            root = int(np.nonzero(want[1] == want[1].max())[0][0])
            assert np.array_equal(big.faces.cpu().numpy(), faces[want[0] == root]), (name, tag)


# ---- 4. normals, volume gradient, volume -------------------------------------------------------------------------------------------
def test_normals_volume_and_gradient_on_field_meshes():
    from deepsdf_amd.surface import SurfaceMesh
    for name, (v, f) in mt.field_meshes().items():
        # one vertex at the position of vertex f[0][0] closing a zero-area face with distinct indices, and one vertex nobody uses
        nv = len(v)
        v2 = np.concatenate([v, v[f[0, 0]][None], np.array([[0.25, -0.5, 0.125]], np.float32)])
        f2 = np.concatenate([f, np.array([[f[0, 0], f[0, 1], nv]], np.int32)])
        assert mt.face_degenerate(v2, f2).sum() == 1
        o, _ = _raw_chain(v2, f2)
        _check_topology(o, f2, name)
        _check_geometry(o, v2, f2, name)
        again, _ = _raw_chain(v2, f2)
        for k in ("normals", "vol_grad", "volume", "degenerate", "mate", "stats", "label", "size"):
            assert o[k].cpu().numpy().tobytes() == again[k].cpu().numpy().tobytes(), (name, k)
        got = o["normals"].cpu().numpy()
        assert not bits(got[nv:]).any() and bits(got[:nv]).any(1).all()     # only the two added vertices have no normal
        assert not bits(o["vol_grad"][nv + 1]).any()
        m = SurfaceMesh(v2, f2)
        assert np.array_equal(bits(m.vertex_normals()), bits(o["normals"])) and np.array_equal(bits(m.volume_vertex_gradient()), bits(o["vol_grad"]))
        assert m.volume() == float(o["volume"]) and m.degenerate_faces().tolist() == [False] * len(f) + [True]
        clean = m.drop_degenerate_faces()
        assert np.array_equal(clean.faces.cpu().numpy(), f) and clean.is_watertight == (name != "smooth_9_10_11")
        assert np.array_equal(bits(clean.vertex_normals()), bits(m.vertex_normals()))   # the zero-area face added nothing


# ---- 5. projection ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [12, 10])
def test_projection_equals_the_fp32_restatement_bit_for_bit(R):
    from deepsdf_amd import _lib
    lib = _lib.lib()
    V = 301                                                     # V * R / 4 and V * R both leave a partial last workgroup
    rng = np.random.default_rng(R)
    jac = (rng.normal(size=(V, R)) * 0.6).astype(np.float32)
    axis = rng.integers(0, 3, V).astype(np.int32)
    n = rng.normal(size=(V, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    n[5] = 0                                                     # a vertex without a normal
    n[6, 1] = -0.0
    one, half = np.float32(1), np.float32(0.5)
    axis[:4] = [0, 0, 1, 2]
    jac[0, :4] = [half, np.nextafter(half, one), -half, -np.nextafter(half, one)]       # stretched by 2: on the clip, just outside
    jac[1, :2] = [np.nextafter(half, np.float32(0)), 1e-30]
    jac[2, :4] = [one, np.nextafter(one, np.float32(2)), -one, np.nextafter(one, np.float32(0))]
    jac[3, :2] = [np.float32(3), np.float32(-0.0)]
    dj, da, dn = torch.from_numpy(jac).cuda(), torch.from_numpy(axis).cuda(), torch.from_numpy(n).cuda()
    for stretch, clip in (((2, 1, 1), 1.0), ((2, 1, 1), 0.0), ((1, 1, 1), 1.0), ((2, 0.5, 3), 0.75)):
        F = G.Fences()
        out = F.new("dtheta", (V, 3, R))
        _lib.check(lib.dsdf_mt_project(G.ptr(dj), G.ptr(da), G.ptr(dn), V, R, (C.c_float * 3)(*stretch), clip, G.ptr(out), G.stream()))
        F.check(f"mt_project R {R} stretch {stretch} clip {clip}")
        want = mt.project(jac, axis, n, stretch, clip)
        assert np.array_equal(bits(out), bits(want)), (R, stretch, clip)
        if stretch == (2, 1, 1) and clip == 1.0:
            o = out.cpu().numpy()
            assert o[0, :, 0].any() and not o[0, :, 1].any() and o[0, :, 2].any() and not o[0, :, 3].any()
            assert o[2, :, 0].any() and not o[2, :, 1].any() and not o[3, :, 0].any() and not o[5].any()


# ---- 6. red zones -----------------------------------------------------------------------------------------------------------------
def test_workspace_entries_under_red_zones():
    v, f = mt.field_meshes()["two_spheres16"]
    strip = mt.quad_strip(4099)                                  # more than one slice of the volume sum
    for verts, faces in ((v, f), strip, mt.hand_made()["runs_at_both_ends"]):
        plain, _ = _raw_chain(verts, faces)
        with G.redzone():
            outs = [_raw_chain(verts, faces, fill)[0] for fill in (0x00, 0xFF)]
        for k in plain:
            assert plain[k].cpu().numpy().tobytes() == outs[0][k].cpu().numpy().tobytes() == outs[1][k].cpu().numpy().tobytes(), k
    o, _ = _raw_chain(*strip)
    _check_geometry(o, *strip, "strip 4099")


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------------
def test_volume_gradient_and_dtheta_of_a_microstructure_mesh():
    from deepsdf_amd.mesh import microstructure_mesh_diff, microstructure_sdf_grid, ms_grid_rows
    from deepsdf_amd.spline import BSplineField
    from deepsdf_amd.surface import SurfaceMesh
    from tests import msdiff_numpy
    from tests.test_gpu_msdiff import CAPS_SIX, JAC_SEEDS, JAC_TOL, NETS, _decoder
    name, degrees, tiling, N = "w32_4x32", (2, 1, 3), [2, 1, 1], [6, 5, 4]
    L, kw = NETS[name]
    knots = [msdiff_numpy.KNOTS[p] for p in degrees]
    S = msdiff_numpy.Fp64Structure(L, kw, JAC_SEEDS[name], degrees, knots, tiling, N, CAPS_SIX, 0.5 / math.sqrt(L))
    dec = _decoder(L, kw, S.params)
    field = BSplineField(degrees, knots, S.cp)
    d = microstructure_mesh_diff(tiling, dec, field, N, max_batch=37, cap_border_dict=CAPS_SIX)
    stretch = (2.0, 1.0, 1.0)
    m = SurfaceMesh.from_diff(d, stretch)
    V = m.n_verts
    # the fp64 Jacobian, as tests/test_gpu_msdiff.py builds it
    grid = d.grid.cpu().numpy()
    ep, ea = msdiff_numpy.edges(grid)
    band, _, _ = msdiff_numpy.band(ep, ea, S.dims)
    rows = ms_grid_rows(field, tiling, N, 0, int(np.prod(S.dims))).cpu().double().requires_grad_(True)
    raw64, _ = S.decode(rows)
    Gd = torch.autograd.grad(raw64.sum(), rows)[0][:, :L].numpy()
    raw = microstructure_sdf_grid(tiling, dec, field, N, apply_caps=False).cpu().numpy()
    mask = S.inside & (grid.reshape(-1) == raw.reshape(-1))
    J, _ = msdiff_numpy.jacobian(grid, ep, ea, S.vs, Gd[band], S.B[band], mask[band])          # [V, ncp, L]
    verts = m.vertices.cpu().numpy()
    faces = m.faces.cpu().numpy()
    assert np.array_equal(bits(verts), bits((d.verts.cpu().numpy() * np.array(stretch)).astype(np.float32)))
    g = mt.vertex_geometry(verts, faces)[3]
    ga = g[np.arange(V), ea] * np.array(stretch)[ea]
    terms = ga[:, None, None] * J
    want = terms.sum(0)
    got = m.volume_gradient().cpu().numpy().astype(np.float64)
    # every Jacobian entry is good to JAC_TOL of its vertex's largest entry (tests/test_gpu_msdiff.py); the sum over V vertices in
    # d.vjp_plan()[1] parts adds the roundings of test_gpu_msdiff's contraction check
    top = np.abs(J).reshape(V, -1).max(1)
    bound = JAC_TOL * (np.abs(ga) * top).sum() + (2 * V + d.vjp_plan()[1] + 4) * 2.0 ** -24 * np.abs(terms).sum(0)
    err = np.abs(got - want)
    print(f"volume gradient: {V} vertices, largest entry {np.abs(want).max():.3e}, worst error {err.max():.3e}, worst error / bound "
          f"{float((err / bound).max()):.3f}")
    assert got.shape == (S.ncp, L) and np.abs(want).max() > 0 and (err <= bound).all()
    assert abs(m.volume() - mt.volume(verts, faces)[0]) <= 1e-12 * mt.volume(verts, faces)[1]
    # dtheta: the oracle's projection of the device's own Jacobian and normals, bit for bit; clip 0 keeps what clip 1 zeroes
    jac, axis = d.jacobian()
    jn, an, nn = jac.cpu().numpy().reshape(V, -1), axis.cpu().numpy(), m.vertex_normals().cpu().numpy()
    for clip in (1.0, 0.0):
        out = m.dtheta(clip=clip)
        assert out.shape == (V, 3, S.ncp * L)
        assert np.array_equal(bits(out), bits(mt.project(jn, an, nn, stretch, clip))), clip
    # the adjoint of the projection: <dtheta(clip 0), g> = shape_derivative(g)
    gv = torch.randn(V, 3, generator=torch.Generator().manual_seed(2))
    sd = m.shape_derivative(gv).cpu().double().reshape(-1)
    ref = torch.einsum("vdr,vd->r", m.dtheta(clip=0.0).cpu().double(), gv.double())
    mag = torch.einsum("vdr,vd->r", m.dtheta(clip=0.0).cpu().double().abs(), gv.double().abs())
    assert bool(((sd - ref).abs() <= (2 * V + 16) * 2.0 ** -24 * mag + 1e-30).all())


def test_dtheta_memory_guard(monkeypatch):
    from deepsdf_amd import mesh as M
    from deepsdf_amd.surface import SurfaceMesh
    from tests.test_gpu_microstructure import SphereCells, linear_field
    cp = np.array([[0.35 if i % 2 == 0 else 0.6] for i in range(8)], dtype=np.float32)
    d = M.microstructure_mesh_diff([2, 1, 1], SphereCells(), linear_field(cp), [12, 8, 6], max_batch=100)
    m = SurfaceMesh.from_diff(d, (2, 1, 1))
    assert m.is_watertight and m.is_winding_consistent and m.n_components >= 2
    assert m.volume() > 0
    monkeypatch.setattr(M, "_free_device_memory", lambda device: 1000)
    with pytest.raises(MemoryError, match=str(4 * m.n_verts * 3 * 8)):
        m.dtheta()


@pytest.mark.parametrize("remove_orphans", [True, False])
def test_deepsdfmesh_on_an_experiment_directory(tmp_path, remove_orphans):
    from analysis.geometry import DeepSDFMesh
    from deepsdf_amd.mesh import default_cap_border_dict
    from deepsdf_amd.surface import SurfaceMesh
    from tests.test_gpu_microstructure import _tiny_experiment
    exp = _tiny_experiment(str(tmp_path))
    options = dict(experiment_directory=exp, checkpoint="latest", degrees=[1, 1, 1], refinement=1, cap_border_dict=default_cap_border_dict(),
                   N_base_reconstruction=6, tiling=[2, 1, 1], remove_orphans=remove_orphans)
    dm = DeepSDFMesh(options)
    assert dm.get_latent_shape() == 4 and dm.get_n_control_points() == 27
    cp = np.tile(dm.latent[0], (27, 1))
    dm.generate_surface_mesh(cp)
    sm = dm.surface_mesh
    assert isinstance(sm, SurfaceMesh) and sm.n_faces > 0 and sm.n_verts == dm.jacobian.verts.shape[0]
    largest = sm if remove_orphans else sm.keep_largest_component()
    assert largest.is_watertight and largest.n_components == 1
    if remove_orphans:
        assert sm.n_components == 1
    assert float(sm.vertices[:, 0].abs().max()) > 1.0            # x is stretched by 2
    dth = dm.get_dTheta_surface()
    assert dth.shape == (sm.n_verts, 3, 27 * 4) and bool(torch.isfinite(dth).all()) and float(dth.abs().max()) <= 1.0
    vg = dm.volume_gradient()
    assert vg.shape == (27, 4) and bool(torch.isfinite(vg).all()) and dm.volume() > 0
    with pytest.raises(NotImplementedError, match="tetgenpy"):
        dm.tetrahedralize_surface()
    with pytest.raises(NotImplementedError, match="gustaf"):
        dm.export_volume_mesh("unused.mesh")
