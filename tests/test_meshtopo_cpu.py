"""The numpy oracle of the surface stage (tests/meshtopo_numpy.py) against independent references, and the host side of the
dsdf_mt_* entries: the planner and every argument error, reported before anything is launched (no device needed)."""
import ctypes as C

import numpy as np
import pytest

from tests import meshtopo_numpy as mt


def _shuffled(faces, seed):
    return np.ascontiguousarray(faces[np.random.default_rng(seed).permutation(len(faces))])


def _label_cases():
    for name, (_, f) in mt.hand_made().items():
        yield name, f
    for name, (_, f) in mt.field_meshes().items():
        yield name, f
        yield name + " shuffled", _shuffled(f, 3)
    yield "tori 2 x 8 x 9 shuffled", _shuffled(mt.torus_pair(8, 9), 4)
    yield "strip 257", mt.quad_strip(257)[1]


def test_oracle_labels_equal_scipy_connected_components():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    for name, f in _label_cases():
        mate, _ = mt.adjacency(f)
        F = len(f)
        h = np.nonzero(mate >= 0)[0]
        g = sp.coo_matrix((np.ones(len(h)), (h // 3, mate[h] // 3)), shape=(F, F))
        n, lab = connected_components(g, directed=False)
        lowest = np.full(n, F, dtype=np.int64)
        np.minimum.at(lowest, lab, np.arange(F))                 # canonical: the lowest face index of every component
        label, size = mt.components(mate, F)
        assert np.array_equal(label, lowest[lab]), name
        assert (size > 0).sum() == n and size.sum() == F and np.array_equal(size, np.bincount(label, minlength=F)), name


def test_relabel_equals_the_oracle_on_the_permuted_mesh():
    for name in ("two_spheres16", "smooth_9_10_11"):
        f = mt.field_meshes()[name][1]
        perm = np.random.default_rng(5).permutation(len(f))
        label, _ = mt.components(mt.adjacency(f)[0], len(f))
        direct = mt.components(mt.adjacency(f[perm])[0], len(f))
        mapped = mt.relabel(label, perm)
        assert np.array_equal(direct[0], mapped[0]) and np.array_equal(direct[1], mapped[1]), name


def test_oracle_mates_and_stats_on_hand_made_meshes():
    want = {"tetrahedron": [6, 0, 0, 6, 0, 0], "minus_one_face": [6, 3, 0, 3, 0, 0], "one_face_flipped": [6, 0, 0, 6, 3, 0],
            "share_a_vertex": [12, 0, 0, 12, 0, 0], "share_an_edge": [11, 0, 1, 10, 0, 0]}
    ncc = {"tetrahedron": 1, "minus_one_face": 1, "one_face_flipped": 1, "share_a_vertex": 2, "share_an_edge": 2}
    for name, (v, f) in mt.hand_made().items():
        mate, stats = mt.adjacency(f)
        h = np.nonzero(mate >= 0)[0]
        assert np.array_equal(mate[mate[h]], h), name            # an involution without fixed points
        assert (mate[h] != h).all() and np.array_equal(mt.edge_keys(f)[h], mt.edge_keys(f)[mate[h]]), name
        assert stats["edges"] == stats["boundary"] + stats["nonmanifold"] + stats["paired"], name
        if name in want:
            assert mt.stats_list(stats) == want[name], name
            assert (mt.components(mate, len(f))[1] > 0).sum() == ncc[name], name
    sizes = mt.components(mt.adjacency(mt.field_meshes()["two_spheres16"][1])[0], 488)[1]
    assert sorted(sizes[sizes > 0].tolist()) == [140, 348]
    assert (mt.adjacency(mt.field_meshes()["smooth_9_10_11"][1])[0] < 0).sum() == 120


def test_oracle_volume_gradient_matches_a_central_difference():
    for name in ("sphere12", "two_spheres16"):
        v, f = mt.field_meshes()[name]
        g = mt.vertex_geometry(v, f)[3]
        v64 = v.astype(np.float64)
        vol = lambda x: (x[f[:, 0]] * np.cross(x[f[:, 1]], x[f[:, 2]])).sum() / 6.0
        assert abs(vol(v64) - mt.volume(v, f)[0]) < 1e-13
        rng = np.random.default_rng(1)
        for i in rng.choice(len(v), 12, replace=False):
            for a in range(3):
                d = np.zeros_like(v64)
                d[i, a] = 1e-4
                fd = (vol(v64 + d) - vol(v64 - d)) / 2e-4           # the volume is linear in one coordinate: exact up to rounding
                assert abs(fd - g[i, a]) <= 1e-10, (name, i, a, fd, g[i, a])
    # a sphere's volume, coarse: within the faceting error
    assert abs(mt.volume(*mt.field_meshes()["sphere12"])[0] - 4 / 3 * np.pi * 0.125) < 0.05


def test_oracle_normal_margin_on_the_field_meshes():
    """Every referenced vertex of the four field meshes has |s| >= 0.5 sum of its corner angles: no normal of the GPU comparison is
    the quotient of a cancelled sum, so that comparison excludes no vertex."""
    for name, (v, f) in mt.field_meshes().items():
        n, ls, wsum, _, _ = mt.vertex_geometry(v, f)
        ref = np.zeros(len(v), bool)
        ref[f.reshape(-1)] = True
        assert ref.all() and not mt.face_degenerate(v, f).any(), name
        margin = float((ls / wsum).min())
        print(f"{name}: smallest |s| / sum of angles {margin:.3f}")
        assert margin >= 0.5, name
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-14, name
    v, f = mt.field_meshes()["sphere12"]
    n = mt.vertex_geometry(v, f)[0]
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert (n * radial).sum(1).min() > 0.97                     # outward, close to the sphere's own normal


def test_oracle_projection_is_fp32_and_matches_the_formula():
    rng = np.random.default_rng(2)
    jac = rng.normal(size=(5, 7)).astype(np.float32)
    n = rng.normal(size=(5, 3)).astype(np.float32)
    axis = np.array([0, 1, 2, 0, 2])
    out = mt.project(jac, axis, n, (2, 1, 1), 1.0)
    assert out.shape == (5, 3, 7) and out.dtype == np.float32
    j = jac.astype(np.float64) * np.array([2.0, 1, 1])[axis][:, None]
    j[np.abs(j) > 1] = 0
    want = j[:, None, :] * n[np.arange(5), axis].astype(np.float64)[:, None, None] * n.astype(np.float64)[:, :, None]
    assert np.abs(out - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max()


# ---- the host side of the library --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepsdf_amd import _lib
    return _lib.lib()


def test_planner_regions_and_limits(lib):
    from deepsdf_amd import _lib
    from tests import ws_guard
    k = ws_guard.constants()
    nb = C.c_size_t()
    for nf in (0, 1, 85, 86, 4096, 4097, 10 ** 6):
        assert lib.dsdf_mt_plan(7, nf, C.byref(nb)) == 0
        rows, total = _lib.ws_regions()
        assert [r[0] for r in rows] == ["mt_stat_part", "mt_cc_gf", "mt_cc_flags", "mt_vol_part"] and total == nb.value
        assert not ws_guard.table_problems(rows, total, 0)
        size = dict((r[0], r[2]) for r in rows)
        assert size["mt_stat_part"] == max(-(-3 * nf // k["MT_BLOCK"]), 1) * k["MT_STATS"] * 8
        assert size["mt_cc_gf"] == max(nf, 1) * 4 and size["mt_cc_flags"] == 4 * k["MT_CC_GROUP"]
        assert size["mt_vol_part"] == 8 * k["MT_VOL_MAX_BLOCKS"]
    with ws_guard.redzone():
        assert lib.dsdf_mt_plan(7, 100, C.byref(nb)) == 0
        rows, total = _lib.ws_regions()
        assert not ws_guard.table_problems(rows, total, ws_guard.REDZONE)
    for nv, nf in ((7, -1), (7, (2 ** 31 - 1) // 3 + 1), (-1, 4), (2 ** 31, 4)):
        assert lib.dsdf_mt_plan(nv, nf, C.byref(nb)) == _lib_invalid(), (nv, nf)
    assert lib.dsdf_mt_plan(7, 4, None) == _lib_invalid()


def _lib_invalid():
    return -1                                                   # DSDF_E_INVALID


def test_argument_errors_come_before_any_launch(lib):
    """Every pointer below is a small non-NULL integer that no kernel could survive: each call must fail on the host."""
    bad, p = _lib_invalid(), C.c_void_p(256)
    null = C.c_void_p(0)
    st = (C.c_float * 3)(2, 1, 1)
    big = (2 ** 31 - 1) // 3 + 1
    assert lib.dsdf_mt_edge_keys(p, -1, 4, p, null) == bad
    assert lib.dsdf_mt_edge_keys(p, big, 4, p, null) == bad
    assert lib.dsdf_mt_edge_keys(p, 4, 0, p, null) == bad
    assert lib.dsdf_mt_edge_keys(null, 4, 4, p, null) == bad
    assert lib.dsdf_mt_edge_keys(p, 4, 4, null, null) == bad
    assert lib.dsdf_mt_edge_keys(null, 0, 4, null, null) == 0                  # nothing to do, nothing launched
    assert lib.dsdf_mt_adjacency(p, 4, p, p, p, null, p, 1 << 20, null) == bad  # NULL stats
    assert lib.dsdf_mt_adjacency(p, 4, p, p, p, p, null, 1 << 20, null) == bad  # NULL workspace
    assert lib.dsdf_mt_adjacency(p, 4, p, p, p, p, p, 16, null) == -2           # DSDF_E_WORKSPACE
    assert lib.dsdf_mt_adjacency(p, 4, p, p, p, p, C.c_void_p(264), 1 << 20, null) == bad   # misaligned workspace
    assert lib.dsdf_mt_adjacency(p, 4, null, p, p, p, p, 1 << 20, null) == bad
    assert lib.dsdf_mt_adjacency(p, -3, p, p, p, p, p, 1 << 20, null) == bad
    rounds = C.c_int32(-5)
    assert lib.dsdf_mt_components(null, 4, p, p, C.byref(rounds), p, 1 << 20, null) == bad
    assert lib.dsdf_mt_components(p, 4, null, p, C.byref(rounds), p, 1 << 20, null) == bad
    assert lib.dsdf_mt_components(p, 4, p, p, C.byref(rounds), null, 1 << 20, null) == bad
    assert lib.dsdf_mt_components(p, 4, p, p, C.byref(rounds), p, 16, null) == -2
    assert lib.dsdf_mt_components(p, big, p, p, C.byref(rounds), p, 1 << 20, null) == bad
    assert lib.dsdf_mt_components(null, 0, null, null, C.byref(rounds), null, 0, null) == 0 and rounds.value == 0
    assert lib.dsdf_mt_face_degenerate(null, 4, p, 4, p, null) == bad
    assert lib.dsdf_mt_face_degenerate(p, 0, p, 4, p, null) == bad
    assert lib.dsdf_mt_face_degenerate(p, 4, p, 4, null, null) == bad
    assert lib.dsdf_mt_face_degenerate(p, 4, null, 0, null, null) == 0
    assert lib.dsdf_mt_vertex_geometry(p, 4, p, 4, p, p, null, null, null) == bad    # every output NULL
    assert lib.dsdf_mt_vertex_geometry(p, 4, p, 4, null, p, p, p, null) == bad
    assert lib.dsdf_mt_vertex_geometry(p, 4, p, 4, p, null, p, p, null) == bad
    assert lib.dsdf_mt_vertex_geometry(p, 0, p, 4, p, p, p, p, null) == bad
    assert lib.dsdf_mt_volume(p, 4, p, 4, null, p, 1 << 20, null) == bad
    assert lib.dsdf_mt_volume(p, 4, p, 4, C.c_void_p(260), p, 1 << 20, null) == bad  # the result is a double
    assert lib.dsdf_mt_volume(p, 4, p, 4, p, null, 1 << 20, null) == bad
    assert lib.dsdf_mt_volume(p, 4, p, 4, p, p, 16, null) == -2
    assert lib.dsdf_mt_volume(null, 4, p, 4, p, p, 1 << 20, null) == bad
    assert lib.dsdf_mt_project(p, p, p, 4, 0, st, 1.0, p, null) == bad
    assert lib.dsdf_mt_project(p, p, p, -1, 8, st, 1.0, p, null) == bad
    assert lib.dsdf_mt_project(p, p, p, 4, 8, None, 1.0, p, null) == bad
    assert lib.dsdf_mt_project(p, p, p, 4, 8, (C.c_float * 3)(2, float("inf"), 1), 1.0, p, null) == bad
    assert lib.dsdf_mt_project(p, p, p, 4, 8, st, float("nan"), p, null) == bad
    assert lib.dsdf_mt_project(null, p, p, 4, 8, st, 1.0, p, null) == bad
    assert lib.dsdf_mt_project(p, p, p, 4, 8, st, 1.0, null, null) == bad
    assert lib.dsdf_mt_project(null, null, null, 0, 8, st, 1.0, null, null) == 0
    assert b"projection" in lib.dsdf_last_error()


def test_public_names_import_without_a_device():
    from analysis.geometry import DeepSDFMesh, sdf_struct, transform          # noqa: F401
    from deepsdf_amd.surface import SurfaceMesh
    import torch
    with pytest.raises(KeyError, match="experiment_directory"):
        DeepSDFMesh({"checkpoint": "latest"})
    with pytest.raises(KeyError, match="checkpoint"):
        DeepSDFMesh({"experiment_directory": "."})
    with pytest.raises(FileNotFoundError):
        DeepSDFMesh({"experiment_directory": "/nonexistent/experiment", "checkpoint": "latest"})
    from deepsdf_amd import _lib
    with pytest.raises(_lib.DsdfError):
        SurfaceMesh(mt.TET_V, mt.TET_F, device="cpu")                          # no CPU fallback
    x = torch.linspace(-1, 1, 41, dtype=torch.float64)
    for t in (1, 2, 3):
        p = 2 / t
        want = (2 / p) * torch.abs((x - t % 2) % (p * 2) - p) - 1
        assert torch.allclose(transform(x, t), want, atol=1e-12)
