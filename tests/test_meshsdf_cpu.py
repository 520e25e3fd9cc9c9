"""CPU (no GPU needed): the fp64 mesh-SDF oracle of tests/meshsdf_numpy.py against analytic answers; the PLY / OBJ readers;
the host side of the sampler against the reference (golden g13: seeded draws, analytic SDFs, the files sample_sdfs writes);
argument checking of the dsdf_msdf_* entry points (every call here fails before any launch); the CLI and the shim import."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import meshsdf_numpy as mn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from deepsdf_amd.build import build_library
    build_library()
    from deepsdf_amd import _lib
    return _lib.lib()


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def test_oracle_cube_is_the_box_sdf():
    V, F = mn.cube()
    P = np.random.default_rng(0).uniform(-2, 2, (3000, 3)).astype(np.float32).astype(np.float64)
    P = np.concatenate([P, [[0, 0, 0], [1, 1, 1], [2, 0, 0], [0.5, 1.0, -0.25], [1.5, 1.5, 0]]])
    assert np.abs(mn.mesh_sdf(V, F, P) - mn.box_sdf(P)).max() <= 1e-12


def test_oracle_icosphere_within_its_sagitta():
    """The icosphere lies inside the unit sphere and no face is deeper than its centroid, so the mesh SDF lies between
    |x| - 1 and |x| - 1 + sagitta (away from the band where the sign may differ)."""
    V, F = mn.icosphere(3)
    sagitta = 1.0 - np.linalg.norm(V[F].mean(1), axis=1).min()
    P = np.random.default_rng(1).uniform(-1.5, 1.5, (2000, 3))
    P = P[np.abs(np.linalg.norm(P, axis=1) - 1) > 2 * sagitta]
    d = mn.mesh_sdf(V, F, P)
    r = np.linalg.norm(P.astype(np.float32).astype(np.float64), axis=1) - 1
    assert np.all(d >= r - 1e-6) and np.all(d <= r + sagitta + 1e-6)


def test_oracle_closed_meshes_have_integer_winding_numbers_and_the_cavity_is_outside():
    P = np.random.default_rng(2).uniform(-1.2, 1.2, (800, 3))
    for V, F in (mn.icosphere(2), mn.torus(), mn.two_parts(), mn.nested_shells(), mn.cube()):
        d2, _, _, w = mn.mesh_query(V, F, P)
        far = np.sqrt(d2) > 1e-6
        assert np.abs(w - np.round(w))[far].max() <= 1e-9
    V, F = mn.nested_shells()
    _, _, _, w = mn.mesh_query(V, F, np.array([[0.0, 0, 0], [0.65, 0, 0], [2, 0, 0]]))
    assert np.allclose(w, [2, 1, 0]) and list(mn.inside(w)) == [False, True, False]
    # with the inner shell reversed the cavity has w = 0: outside either way
    Vi, Fi = mn.icosphere(2, 0.4)
    V2, F2 = mn.concat(mn.icosphere(2, 0.9), (Vi, Fi[:, ::-1]))
    _, _, _, w2 = mn.mesh_query(V2, F2, np.array([[0.0, 0, 0]]))
    assert abs(w2[0]) < 1e-9 and not mn.inside(w2)[0]


def test_oracle_degenerate_faces_are_segments():
    V = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0.0]])
    F = np.array([[0, 1, 2], [0, 0, 2], [3, 3, 3]])
    P = np.array([[1.0, 1, 0], [-1, 0, 0], [3, 0, 0], [0, 2, 0]])
    cp = mn.closest_points(P[:, None], V[F[:, 0]][None], V[F[:, 1]][None], V[F[:, 2]][None])
    assert np.all(np.isfinite(cp))
    assert np.allclose(cp[0, 0], [1, 0, 0]) and np.allclose(cp[1, 1], [0, 0, 0]) and np.allclose(cp[2, 0], [2, 0, 0])
    assert np.allclose(cp[3, 2], [0, 1, 0])


@pytest.mark.parametrize("h", mn.SLIVER_HEIGHTS)
def test_oracle_agrees_with_the_edges_and_plane_formulation_on_slivers(h):
    """A second opinion on the inputs of tests/test_gpu_meshsdf_faces.py's sliver sweep (unit longest edge, height h): the
    oracle's closest point against the nearest of three clamped edges and the plane foot, to 1e-9 of the longest edge.  With
    va, vb, vc from Ericson's dot products the oracle missed this from h = 1e-4 down (2.7e-7 at 1e-5, 1.7e-5 at 1e-6)."""
    worst = 0.0
    for _, V, F, P in mn.sliver_cases(h):
        a, b, c = (V[F[0, k]] for k in range(3))
        assert abs(max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)) - 1.0) <= h * h + 1e-6
        c1, c2 = mn.closest_points(P, a, b, c), mn.closest_points_edges_plane(P, a, b, c)
        worst = max(worst, np.linalg.norm(c1 - c2, axis=1).max(),
                    np.abs(np.linalg.norm(P - c1, axis=1) - np.linalg.norm(P - c2, axis=1)).max())
    print("sliver", h, f"{worst:.2e}")
    assert worst <= 1e-9


def test_oracle_solid_angle_numerator_equals_the_textbook_triple_product():
    """solid_angles takes Van Oosterom-Strackee's numerator A . (B x C) as A . ((b - a) x (c - a)).  On well-shaped faces both
    are sums of products of O(1) numbers in fp64: they agree to 1e-14 of |A||B||C|, the angles to 1e-12 away from the faces."""
    for V, F in (mn.icosphere(2), mn.torus(), mn.cube()):
        P = np.random.default_rng(9).uniform(-1.2, 1.2, (300, 3))[:, None]
        a, b, c = (V[F[:, k]][None] for k in range(3))
        A, B, Cc = a - P, b - P, c - P
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (A, B, Cc))
        det = (A * np.cross(B, Cc)).sum(-1)
        assert np.abs(det - (A * np.cross(b - a, c - a)).sum(-1)).max() <= 1e-14 * (la * lb * lc).max()
        den = la * lb * lc + (A * B).sum(-1) * lc + (B * Cc).sum(-1) * la + (Cc * A).sum(-1) * lb
        far = np.sqrt(mn.mesh_query(V, F, P[:, 0])[0]) > 1e-3
        assert np.abs(2 * np.arctan2(det, den) - mn.solid_angles(P, a, b, c))[far].max() <= 1e-12


def test_oracle_region_names_cover_a_triangle():
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
    P = np.array([[-1, -1, 1], [2, -0.5, 0], [0.5, -1, 2], [-0.5, 2, 0], [-1, 0.5, 0], [1, 1, -1], [0.25, 0.25, 3.0]])
    assert [mn.REGIONS[k] for k in mn.regions(P, a, b, c)] == ["A", "B", "AB", "C", "AC", "BC", "IN"]


# ---- readers ------------------------------------------------------------------------------------------------------------------
def test_ply_round_trip_through_write_ply(tmp_path):
    from deepsdf_amd.mesh import write_ply
    from deepsdf_amd.meshsdf import read_mesh
    V, F = mn.icosphere(1)
    write_ply(str(tmp_path / "m.ply"), V.astype(np.float32), F.astype(np.int32))
    V2, F2 = read_mesh(tmp_path / "m.ply")
    assert V2.dtype == np.float64 and F2.dtype == np.int64
    assert np.array_equal(V2, V.astype(np.float32).astype(np.float64)) and np.array_equal(F2, F)


def test_ascii_ply_with_extra_properties_and_quads(tmp_path):
    from deepsdf_amd.meshsdf import read_mesh
    txt = """ply
format ascii 1.0
comment made by hand
element vertex 5
property float x
property float y
property uchar red
property double z
property float nx
element edge 1
property int vertex1
property int vertex2
element face 2
property uchar flags
property list uchar uint vertex_index
end_header
0 0 255 0 1
1 0 0 0 1
1 1 0 0 1
0 1 0 0 1
0.5 0.5 0 1 1
0 1
7 4 0 1 2 3
0 3 0 1 4
"""
    (tmp_path / "a.ply").write_text(txt)
    V, F = read_mesh(tmp_path / "a.ply")
    assert np.array_equal(V, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]])
    assert np.array_equal(F, [[0, 1, 2], [0, 2, 3], [0, 1, 4]])


_NP = {"float": "f4", "double": "f8", "short": "i2", "int": "i4", "uint": "u4", "uchar": "u1", "int16": "i2"}


def _binary_ply(endian, vtype, itype, V, polys):
    e = ">" if endian == "big" else "<"
    head = ["ply", f"format binary_{endian}_endian 1.0", f"element vertex {len(V)}", f"property {vtype} x",
            f"property {vtype} y", "property ushort quality", f"property {vtype} z",
            f"element face {len(polys)}", f"property list ushort {itype} vertex_indices", "end_header"]
    rows = np.zeros(len(V), dtype=[("x", e + _NP[vtype]), ("y", e + _NP[vtype]), ("q", e + "u2"), ("z", e + _NP[vtype])])
    rows["x"], rows["y"], rows["z"], rows["q"] = V[:, 0], V[:, 1], V[:, 2], 7
    body = rows.tobytes()
    for p in polys:
        body += np.array([len(p)], dtype=e + "u2").tobytes() + np.array(p, dtype=e + _NP[itype]).tobytes()
    return ("\n".join(head) + "\n").encode() + body


@pytest.mark.parametrize("endian,vtype,itype", [("big", "float", "int"), ("big", "double", "uint"),
                                                ("little", "short", "uchar"), ("little", "double", "int16")])
def test_binary_ply_any_endianness_and_types(tmp_path, endian, vtype, itype):
    """Triangles only (the structured fast path) and a quad among triangles (row by row), both endiannesses."""
    from deepsdf_amd.meshsdf import read_mesh
    V = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [1, 1, 3]], dtype=np.float64)
    want = [[0, 1, 2], [0, 2, 3], [0, 1, 4]]
    for polys in ([[0, 1, 2], [0, 2, 3], [0, 1, 4]], [[0, 1, 2, 3], [0, 1, 4]]):
        (tmp_path / "b.ply").write_bytes(_binary_ply(endian, vtype, itype, V, polys))
        V2, F2 = read_mesh(tmp_path / "b.ply")
        assert np.array_equal(V2, V) and np.array_equal(F2, want)


def test_obj_face_forms_and_negative_indices(tmp_path):
    from deepsdf_amd.meshsdf import read_mesh
    txt = """# comment
o thing
v 0 0 0
v 1 0 0
v 1 1 0
vt 0 0
vn 0 0 1
v 0 1 0 1.0
f 1 2 3
f 1/1 3/1 4/1
usemtl x
f 1//1 2//1 4//1
f -4/1/1 -3/1/1 -2/1/1 -1/1/1
s off
"""
    (tmp_path / "m.obj").write_text(txt)
    V, F = read_mesh(tmp_path / "m.obj")
    assert V.shape == (4, 3) and np.array_equal(V[3], [0, 1, 0])
    assert np.array_equal(F, [[0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 2, 3]])


_HDR = b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\n"


@pytest.mark.parametrize("name,content", [
    ("a.ply", b"plx\nformat ascii 1.0\nend_header\n"),
    ("b.ply", _HDR.replace(b"vertex 1", b"vertex 2") + b"end_header\n0 0 0\n"),
    ("c.ply", _HDR.replace(b"ascii", b"binary_little_endian").replace(b"vertex 1", b"vertex 3") + b"end_header\n" + b"\0" * 20),
    ("d.ply", _HDR + b"element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n3 0 0 5\n"),
    ("e.ply", b"ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty floot y\nend_header\n0 0\n"),
    ("f.ply", _HDR + b"end_header\n0 a 0\n"),
    ("g.ply", _HDR + b"element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n3 0 0\n"),
    ("h.ply", _HDR.replace(b"ascii", b"binary_big_endian") + b"element face 1\nproperty list uchar int vertex_indices\n"
              b"end_header\n" + b"\0" * 12 + b"\x03\0\0\0\0"),
    ("i.ply", _HDR),
    ("j.ply", b"ply\nformat utf8 1.0\nend_header\n"),
    ("k.obj", b"v 0 0 0\nv 1 0 0\nf 1 2\n"),
    ("l.obj", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 x\n"),
    ("m.obj", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n"),
    ("n.obj", b"v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n"),
    ("o.obj", b"v 0 0\n"),
    ("p.stl", b"solid x\n"),
])
def test_malformed_files_raise(tmp_path, name, content):
    from deepsdf_amd.meshsdf import read_mesh
    (tmp_path / name).write_bytes(content)
    with pytest.raises(ValueError):
        read_mesh(tmp_path / name)


# ---- the sampler's host side vs the reference (golden g13, tests/golden/make_golden_sdf_sampler.py) -----------------------------
@pytest.fixture(scope="module")
def g13(golden_dir):
    with np.load(os.path.join(golden_dir, "g13_sdf_sampler.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_random_sample_sdf_draws_the_reference_points(g13):
    from deepsdf_amd.sdf_sampler import BoxSDF, random_points_cube, random_sample_sdf
    for t in ("uniform", "plane", "spherical_gaussian"):
        np.random.seed(int(g13["seed"]))
        r = random_sample_sdf(BoxSDF(0.5), (-1, 1), 257, type=t)
        for k, got in (("samples", r.samples), ("distances", r.distances)):
            want = g13[f"draw_{t}_{k}"]
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (t, k)
    np.random.seed(int(g13["seed"]))
    got = random_points_cube(100, 1.5)
    assert got.dtype == g13["cube_points"].dtype and np.array_equal(got, g13["cube_points"])


def test_analytic_sdfs_equal_the_reference(g13):
    from deepsdf_amd.sdf_sampler import BoxSDF, NegatedCallable, RandomSampleSDF, SummedSDF
    q = g13["queries"]
    a, b = BoxSDF(0.5), BoxSDF(0.25, np.array([0.3, -0.2, 0.1]))
    for name, f in (("box", a), ("box2", b), ("sum", a + b), ("sum_cls", SummedSDF(a, b)), ("neg", -a),
                    ("neg_cls", NegatedCallable(b))):
        got, want = f(q), g13[f"sdf_{name}"]
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
    pos, neg = RandomSampleSDF(q, a(q)).split_pos_neg()
    for k, got in (("split_pos", pos.stacked), ("split_neg", neg.stacked), ("split_sum", (pos + neg).stacked)):
        assert got.dtype == g13[k].dtype and np.array_equal(got, g13[k]), k


def test_sample_sdfs_writes_the_reference_files(g13, tmp_path):
    from deepsdf_amd.sdf_sampler import BoxSDF, SDFSampler
    meta = json.loads(str(g13["meta"]))
    s = SDFSampler(str(tmp_path / "SdfSamples"), str(tmp_path / "splits"))
    os.makedirs(tmp_path / "splits")
    info = {"dataset_name": meta["dataset"], "class_name": meta["class"]}
    np.random.seed(int(g13["seed"]))
    sdfs = [BoxSDF(0.5), BoxSDF(0.3, np.array([0.1, 0.2, -0.1])) + BoxSDF(0.2)]
    split = s.sample_sdfs(sdfs, info, n_samples=float(meta["n_samples"]), sampling_strategy="uniform")
    s.write_json(meta["split_name"], info, split)
    assert split == meta["split"]
    with open(tmp_path / "splits" / meta["split_name"]) as fh:
        assert fh.read() == meta["split_json"]
    for i, stem in enumerate(split):
        with np.load(tmp_path / "SdfSamples" / meta["dataset"] / meta["class"] / f"{stem}.npz") as z:
            assert sorted(z.files) == ["neg", "pos"]
            for k in ("pos", "neg"):
                want = g13[f"file{i}_{k}"]
                assert z[k].dtype == want.dtype and np.array_equal(z[k], want), (i, k)
    # an existing file is kept: a second call draws nothing and writes nothing
    state = np.random.get_state()[1].copy()
    assert s.sample_sdfs(sdfs, info, n_samples=10) == split and s.timings == []
    assert np.array_equal(np.random.get_state()[1], state)


def test_mesh_sdf_rows_are_float64_and_plotting_needs_gustaf():
    from deepsdf_amd.sdf_sampler import RandomSampleSDF
    x = np.random.default_rng(0).uniform(-1, 1, (10, 3))
    d = (np.linalg.norm(x, axis=1) - 0.5).astype(np.float32).reshape(-1, 1)      # what SDFfromMesh returns
    pos, neg = RandomSampleSDF(x, d).split_pos_neg()
    assert pos.stacked.dtype == np.float64 and neg.stacked.dtype == np.float64 and len(pos.samples) + len(neg.samples) == 10
    if importlib.util.find_spec("gustaf") is None:
        with pytest.raises(ImportError, match="gustaf"):
            pos.create_gus_plottable()


# ---- ABI argument checks (no launch) ---------------------------------------------------------------------------------------------
def test_msdf_arguments_are_refused_before_any_launch(lib):
    tb, wb, ns = C.c_size_t(), C.c_size_t(), C.c_int32()
    assert lib.dsdf_msdf_plan(12, 100, C.byref(tb), C.byref(wb), C.byref(ns)) == 0
    assert tb.value == 12 * 64 and ns.value == 1 and wb.value == 100 * 12
    assert lib.dsdf_msdf_plan(100000, 100000, None, None, C.byref(ns)) == 0 and ns.value == 6
    assert lib.dsdf_msdf_plan(5120, 300, None, C.byref(wb), C.byref(ns)) == 0 and ns.value == 5 and wb.value == 5 * 300 * 12
    assert lib.dsdf_msdf_plan(5120, 256 * 2048, None, None, C.byref(ns)) == 0 and ns.value == 1
    assert lib.dsdf_msdf_plan(10 ** 7, 1, None, None, C.byref(ns)) == 0 and ns.value == 64
    assert lib.dsdf_msdf_plan(0, 10, C.byref(tb), None, None) == -1 and b"faces" in lib.dsdf_last_error()
    assert lib.dsdf_msdf_plan(-5, 10, C.byref(tb), None, None) == -1
    assert lib.dsdf_msdf_plan(10, -1, C.byref(tb), None, None) == -1
    assert lib.dsdf_msdf_plan(2 ** 31, 10, C.byref(tb), None, None) == -1 and b"int32" in lib.dsdf_last_error()
    assert lib.dsdf_msdf_plan(10, 2 ** 31, C.byref(tb), None, None) == -1
    assert lib.dsdf_msdf_plan(10, 10, None, None, None) == -1
    fake = C.c_void_p(1 << 20)         # never dereferenced: every call below is refused before a launch
    assert lib.dsdf_msdf_prepare(fake, 8, fake, 0, fake, 1 << 30, None) == -1
    assert lib.dsdf_msdf_prepare(fake, 0, fake, 12, fake, 1 << 30, None) == -1
    assert lib.dsdf_msdf_prepare(None, 8, fake, 12, fake, 1 << 30, None) == -1
    assert lib.dsdf_msdf_prepare(fake, 8, None, 12, fake, 1 << 30, None) == -1
    assert lib.dsdf_msdf_prepare(fake, 8, fake, 12, None, 1 << 30, None) == -1
    assert lib.dsdf_msdf_prepare(fake, 8, fake, 12, fake, 12 * 64 - 1, None) == -2
    assert lib.dsdf_msdf_prepare(fake, 8, fake, 2 ** 31, fake, 1 << 40, None) == -1
    assert lib.dsdf_msdf_prepare(fake, 8, fake, 12, C.c_void_p((1 << 20) + 4), 1 << 30, None) == -1
    one = (fake, None, None, None, None)

    def q(nf, nq, outs, ws=fake, wsb=1 << 30):
        return lib.dsdf_msdf_query(fake, nf, fake, nq, *outs, 0, ws, wsb, None)
    assert q(0, 100, one) == -1 and b"faces" in lib.dsdf_last_error()
    assert q(12, 100, (None,) * 5) == -1 and b"NULL" in lib.dsdf_last_error()
    assert q(12, 100, one, wsb=100 * 12 - 1) == -2 and b"workspace" in lib.dsdf_last_error()
    assert q(12, 100, (None, None, None, None, fake), ws=None) == -1
    assert q(12, -1, one) == -1
    assert q(12, 2 ** 31, one) == -1
    assert lib.dsdf_msdf_query(None, 12, fake, 100, fake, None, None, None, None, 0, fake, 1 << 30, None) == -1
    assert lib.dsdf_msdf_query(fake, 12, None, 100, fake, None, None, None, None, 0, fake, 1 << 30, None) == -1
    assert q(12, 0, one, ws=None, wsb=0) == 0           # no queries: nothing to do


# ---- entry points import on CPU ------------------------------------------------------------------------------------------------
def test_shim_package_and_cli_import():
    from sdf_sampler import sdf_sampler as shim
    from deepsdf_amd import sdf_sampler
    for name in ("SDFBase", "SummedSDF", "NegatedCallable", "BoxSDF", "DataSetInfo", "SphereParameters", "RandomSampleSDF",
                 "SDFSampler", "SDFfromMesh", "random_points_cube", "random_sample_sdf"):
        assert getattr(shim, name) is getattr(sdf_sampler, name), name
    spec = importlib.util.spec_from_file_location("ssfm", os.path.join(ROOT, "sample_sdf_from_meshes.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert callable(m.main)
    with pytest.raises(SystemExit):
        m.main(["--help"])


def test_sdf_from_mesh_accepts_the_reference_inputs(tmp_path):
    """Mesh arguments resolve without a GPU (the upload happens on the first call)."""
    from deepsdf_amd.mesh import write_ply
    from deepsdf_amd.sdf_sampler import SDFfromMesh, _mesh_arrays
    V, F = mn.cube()

    class Trimeshlike:
        vertices, faces = V, F
    write_ply(str(tmp_path / "c.ply"), V.astype(np.float32), F.astype(np.int32))
    for m in (Trimeshlike(), (V, F), str(tmp_path / "c.ply"), tmp_path / "c.ply"):
        V2, F2 = _mesh_arrays(m)
        assert np.array_equal(np.asarray(V2), V) and np.array_equal(np.asarray(F2), F)
        s = SDFfromMesh(m)
        assert s.dtype == np.float32 and s.flip_sign is False
    with pytest.raises(TypeError):
        _mesh_arrays(42)
