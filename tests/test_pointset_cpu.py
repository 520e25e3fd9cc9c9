"""CPU (no GPU needed): the numpy oracle of the point-set kernels (tests/pointset_numpy.py) against published vectors and scipy,
the host planners dsdf_nn_plan / dsdf_surf_plan at their break points, the deep_sdf.metrics shim and evaluate.py's command
line."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pointset_numpy as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from deepsdf_amd.build import build_library
    build_library()
    from deepsdf_amd import _lib
    return _lib.lib()


def test_philox_known_answers():
    """The known-answer vectors of Philox4x32-10 published with Random123 (kat_vectors): zeros, all ones, digits of pi."""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in pn.philox4x32_10(ctr, key)[0]) == want, (ctr, key)
    # vectorised over counters = one at a time; the sampler's counter layout
    w = pn.sample_words(5, (7 << 32) | 9, offset=(1 << 32) + 3)
    for t in range(5):
        i = (1 << 32) + 3 + t
        assert np.array_equal(w[t], pn.philox4x32_10((i & 0xffffffff, 0, i >> 32, 0), (9, 7))[0])


def test_oracle_nearest_neighbour_equals_ckdtree():
    sp = pytest.importorskip("scipy.spatial")
    g = np.random.default_rng(0)
    Q, R = g.uniform(-1, 1, (700, 3)), g.uniform(-1, 1, (1300, 3))
    d2, idx = pn.nn_bruteforce(Q, R)
    d, i = sp.cKDTree(pn.f32(R)).query(pn.f32(Q))
    assert np.abs(np.sqrt(d2) - d).max() <= 1e-14 and np.array_equal(idx, i)
    assert np.array_equal(pn.pair_d2(Q, R, idx), d2)
    R[40] = R[3]                                                     # ties go to the lowest index
    assert pn.nn_bruteforce(R[40:41], R)[1][0] == 3


def test_oracle_sampler_rule():
    """Two triangles of area 1 and 3 with a zero-area face between them: the zero-area face is never drawn, the shares follow
    the areas, the points lie in their triangles."""
    V = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1]], dtype=np.float64)
    F = np.array([[0, 1, 2], [0, 1, 1], [3, 4, 5]])
    area = pn.face_areas(V, F).astype(np.float32)
    assert area.tolist() == [1.0, 0.0, 3.0]
    s = pn.surface_samples(V, F, area, 20000, seed=5)
    assert set(np.unique(s["face"])) == {0, 2}
    assert abs((s["face"] == 2).mean() - 0.75) < 5 * np.sqrt(0.75 * 0.25 / 20000)
    assert (s["u"] >= 0).all() and (s["v"] >= 0).all() and (s["u"].astype(np.float64) + s["v"] <= 1 + 2.0 ** -24).all()
    assert np.abs(s["point"][:, 2] - (s["face"] == 2)).max() == 0
    two = pn.surface_samples(V, F, area, 100, seed=5, offset=19900)
    assert np.array_equal(two["face"], s["face"][19900:]) and np.array_equal(two["u"], s["u"][19900:])


# Error of the fp32 area (pn.face_areas_f32) against the fp64 area of the same fp32 vertices (pn.face_areas), u = 2^-24, M = |ab| |ac|:
#   ab, ac: fp32 differences, each component within u relative: n = ab x ac moves by at most 2 u M (norm)
#   a normal component p - q: products and the difference rounded, error <= u (|p| + |q|) + u |p - q| <= 2 u |ab'| |ac'| with ab', ac'
#       the two-dimensional projections (Cauchy-Schwarz); over the three components the norm of the errors is <= 2 sqrt(3) u M
#   n.n: squares, two sums: (1 + u)^3 relative; the correctly rounded root of it: 1.5 u + u = 2.5 u relative to |n| <= M
#   |n| within (2 + 3.47 + 2.5) u M = 7.97 u M, the area within half of that.
# AREA_TOL multiplies M, with 2 % on top for the second-order terms and the fp64 side's own rounding.
AREA_TOL = 1.02 * 0.5 * 7.97 * 2.0 ** -24
SOUP_SEED = 13
SOUP_CUTS = (1023, 1024, 1025, pn.SOUP_SPLIT, pn.SOUP_SPLIT + 1, pn.SOUP_SPLIT + 1025)


def _area_cases():
    """(name, V, F, is rounding visible) of the meshes whose areas the GPU tests compare bit for bit."""
    from tests import mc_numpy
    sdf, h = mc_numpy.sphere(24, 0.6)
    v, f = mc_numpy.marching_cubes(sdf, 0.0, (h, h, h), (-1, -1, -1))
    yield "mc_sphere", v, f.astype(np.int64), True
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 0, 0], [0, 0, 2], [0.25, 3, 1], [-1, -1, 0.75]], dtype=np.float32)
    yield "six_faces", V, np.array([[0, 1, 2], [3, 3, 5], [1, 3, 2], [1, 4, 3], [0, 1, 4], [5, 6, 7]]), False      # dyadic: exact products
    V, F = pn.sliver_between_faces()
    yield "sliver", V, F, True
    for nf in SOUP_CUTS:
        V, F = pn.triangle_soup(nf, SOUP_SEED, heavy_tail=True)
        yield f"soup{nf}", V, F, True


def test_fp32_areas_lie_within_the_rounding_bound_of_fp64():
    for name, V, F, _ in _area_cases():
        a32, a64 = pn.face_areas_f32(V, F), pn.face_areas(V, F)
        assert a32.dtype == np.float32 and a32.shape == (len(F),)
        Vd = pn.f32(V)
        M = np.linalg.norm(Vd[F[:, 1]] - Vd[F[:, 0]], axis=1) * np.linalg.norm(Vd[F[:, 2]] - Vd[F[:, 0]], axis=1)
        err = np.abs(a32.astype(np.float64) - a64)
        print(f"{name}: {len(F)} faces, max error / bound {(err[M > 0] / (AREA_TOL * M[M > 0])).max():.3f}")
        assert (err <= AREA_TOL * M).all(), name


def test_a_contracted_cross_product_shows_on_the_inputs_the_gpu_tests_use():
    """The contracted variant is not the specification.  On every mesh whose coordinates are not dyadic it gives at least a tenth
    of the faces another area (the soups hold 3 fresh vertices per face, so no two faces share a rounding), always within the
    bound above; on the dyadic six-face mesh, whose products are exact, it gives the same bits -- that mesh checks the zero-area
    rule, not the rounding."""
    for name, V, F, visible in _area_cases():
        spec, fused = pn.face_areas_f32(V, F), pn.face_areas_f32(V, F, contracted=True)
        d = int((spec.view(np.uint32) != fused.view(np.uint32)).sum())
        print(f"{name}: {d} of {len(F)} areas differ")
        if visible:
            assert d >= 0.1 * len(F), (name, d)
        else:
            assert d == 0, (name, d)


def test_the_doubled_edge_face_has_exactly_no_area_in_the_specification_only():
    V, F = pn.sliver_between_faces()
    spec, fused = pn.face_areas_f32(V, F), pn.face_areas_f32(V, F, contracted=True)
    assert spec[1] == 0.0 and spec[0] > 0 and spec[2] > 0
    assert fused[1] > 0.0                                            # the rounding error of one product survives the fused form
    assert not any(float(c) == int(c * 2 ** 20) / 2 ** 20 for c in V[1])       # d is not dyadic (to 20 bits): the products round
    s = pn.surface_samples(V, F, spec, 65536, seed=3)
    assert set(np.unique(s["face"])) == {0, 2}


def test_soup_is_nested_and_its_tail_carries_half_the_area():
    """The soup's contract: a cut is a prefix of the full soup; with heavy_tail the faces behind the first 256 scan tiles carry
    about half of the area, and the oracle's samples of every cut stay clear of the undecided band."""
    full_V, full_F = pn.triangle_soup(SOUP_CUTS[-1], SOUP_SEED, heavy_tail=True)
    plain_V, _ = pn.triangle_soup(SOUP_CUTS[-1], SOUP_SEED)
    assert np.array_equal(full_V[:3 * pn.SOUP_SPLIT], plain_V[:3 * pn.SOUP_SPLIT])
    edges = np.linalg.norm(plain_V[1::3].astype(np.float64) - plain_V[0::3], axis=1)
    assert 0.03 < edges.mean() < 0.07
    for nf in SOUP_CUTS:
        V, F = pn.triangle_soup(nf, SOUP_SEED, heavy_tail=True)
        assert F.shape == (nf, 3) and np.array_equal(V[:3 * min(nf, pn.SOUP_SPLIT)], full_V[:3 * min(nf, pn.SOUP_SPLIT)])
        area = pn.face_areas_f32(V, F)
        o = pn.surface_samples(V, F, area, 4096, SOUP_SEED)
        assert o["margin"].min() > 1e-12, (nf, o["margin"].min())
        if nf > pn.SOUP_SPLIT:
            share = area[pn.SOUP_SPLIT:].astype(np.float64).sum() / area.astype(np.float64).sum()
            assert 0.45 < share < 0.55 and (o["face"] >= pn.SOUP_SPLIT).mean() >= 0.25, (nf, share)


def test_plans_at_their_break_points(lib):
    """dsdf_nn_plan: n_splits = min(ceil(2048 / ceil(nq / 1024)), floor(nr / 1024), 64), at least 1; the workspace holds 8 bytes
    per (split, query) when there is more than one split.  dsdf_surf_plan: tiles of 1024 faces."""
    wb, ns = C.c_size_t(), C.c_int32()

    def plan(nq, nr):
        assert lib.dsdf_nn_plan(nq, nr, C.byref(wb), C.byref(ns)) == 0, lib.dsdf_last_error()
        return ns.value, wb.value

    for nr, want in ((1, 1), (2047, 1), (2048, 2), (3071, 2), (3072, 3), (65535, 63), (65536, 64), (10 ** 6, 64)):
        assert plan(256, nr) == (want, want * 256 * 8 if want > 1 else 0), nr
    assert plan(1024, 10 ** 6)[0] == 64 and plan(1025, 10 ** 6)[0] == 64          # 1 and 2 tiles: ceil(2048 / tiles) >= 64
    assert plan(32 * 1024, 10 ** 6)[0] == 64 and plan(32 * 1024 + 1, 10 ** 6)[0] == 63
    assert plan(2046 * 1024 + 1, 10 ** 6)[0] == 2 and plan(2047 * 1024, 10 ** 6)[0] == 2
    assert plan(2047 * 1024 + 1, 10 ** 6) == (1, 0) and plan(10 ** 7, 10 ** 6) == (1, 0)
    assert plan(0, 5) == (1, 0)
    assert plan(2 ** 31 - 1, 2 ** 31 - 1) == (1, 0)
    for bad in ((5, 0), (-1, 5), (5, -1), (2 ** 31, 5), (5, 2 ** 31)):
        assert lib.dsdf_nn_plan(*bad, C.byref(wb), C.byref(ns)) == -1, bad
    assert lib.dsdf_nn_plan(5, 5, None, None) == -1
    sb, ao, nt = C.c_size_t(), C.c_size_t(), C.c_int32()
    for nf, tiles in ((1, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 3)):
        assert lib.dsdf_surf_plan(nf, C.byref(sb), C.byref(ao), C.byref(nt)) == 0
        assert nt.value == tiles and ao.value % 256 == 0 and ao.value >= 8 * nf + 8 * tiles and sb.value >= ao.value + 4 * nf
    assert lib.dsdf_surf_plan(0, C.byref(sb), None, None) == -1 and lib.dsdf_surf_plan(2 ** 31, C.byref(sb), None, None) == -1


def test_argument_errors_come_before_any_launch(lib):
    dummy = C.c_void_p(4096)       # never dereferenced
    assert lib.dsdf_nn_query(dummy, 4, dummy, 0, dummy, dummy, None, 0, None) == -1 and b"reference" in lib.dsdf_last_error()
    assert lib.dsdf_nn_query(dummy, 4, dummy, 4, None, None, None, 0, None) == -1 and b"NULL" in lib.dsdf_last_error()
    assert lib.dsdf_nn_query(dummy, 256, dummy, 4096, dummy, dummy, None, 0, None) == -1          # 4 splits need a workspace
    assert lib.dsdf_nn_query(dummy, 256, dummy, 4096, dummy, dummy, dummy, 100, None) == -2
    assert lib.dsdf_nn_query(None, 0, None, 4, dummy, None, None, 0, None) == 0                    # no queries: nothing to do
    assert lib.dsdf_mean_f64(dummy, 0, dummy, dummy, 8192, None) == -1
    assert lib.dsdf_mean_f64(dummy, 4, dummy, dummy, 8191, None) == -2
    assert lib.dsdf_surf_sample(dummy, 3, dummy, 1, dummy, 1 << 20, -1, 0, 0, 0.0, dummy, None, None, None) == -1
    assert lib.dsdf_surf_sample(dummy, 3, dummy, 1, dummy, 1 << 20, 4, 0, 0, -1.0, dummy, None, None, None) == -1
    assert lib.dsdf_surf_sample(dummy, 3, dummy, 1, dummy, 8, 4, 0, 0, 0.0, dummy, None, None, None) == -2
    assert lib.dsdf_surf_sample(dummy, 3, dummy, 1, dummy, 1 << 20, 0, 0, 0, 0.0, None, None, None, None) == 0


def test_shim_exports_the_reference_signature():
    import deep_sdf
    from deep_sdf.metrics.chamfer import compute_trimesh_chamfer
    from deepsdf_amd import metrics
    assert compute_trimesh_chamfer is metrics.compute_trimesh_chamfer is deep_sdf.compute_trimesh_chamfer
    names = list(inspect.signature(compute_trimesh_chamfer).parameters)
    assert names[:5] == ["gt_points", "gen_mesh", "offset", "scale", "num_mesh_samples"]
    assert inspect.signature(compute_trimesh_chamfer).parameters["num_mesh_samples"].default == 30000
    from deepsdf_amd.sdf_sampler import noisy_sample
    assert list(inspect.signature(noisy_sample).parameters)[:3] == ["mesh", "std", "count"]


def test_points_ply_round_trip(tmp_path):
    from deepsdf_amd.mesh import write_points_ply
    from deepsdf_amd.meshsdf import read_mesh, read_points
    P = np.random.default_rng(1).uniform(-1, 1, (37, 3)).astype(np.float32)
    path = str(tmp_path / "p.ply")
    write_points_ply(path, P)
    assert np.array_equal(read_points(path), P.astype(np.float64))
    V, F = read_mesh(path)
    assert F.shape == (0, 3) and len(V) == 37


def test_evaluate_help_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--samples" in r.stdout and "--exact" in r.stdout and "--split" in r.stdout
