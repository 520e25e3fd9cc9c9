"""-m gpu: the HIP mesh SDF (dsdf_msdf_*, deepsdf_amd/meshsdf.py) against the fp64 oracle of tests/meshsdf_numpy.py; split
and call determinism; the sampler (deepsdf_amd/sdf_sampler.py) end to end into a short training run; the sampling CLI."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import meshsdf_numpy as mn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # distances and sdf
W_TOL = 1e-4        # winding numbers away from the surface
SIGN_BAND = 1e-4    # the sign is exact wherever |sdf| exceeds this


def _mesh(V, F):
    from deepsdf_amd.meshsdf import TriangleMesh
    return TriangleMesh(V, F)


def _near_surface(V, F, n, seed, scale=0.02):
    """Points on random faces plus a small random offset."""
    g = np.random.default_rng(seed)
    f = g.integers(0, len(F), n)
    u, v = g.random(n), g.random(n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    a, b, c = V[F[f, 0]], V[F[f, 1]], V[F[f, 2]]
    return a + u[:, None] * (b - a) + v[:, None] * (c - a) + g.normal(0, scale, (n, 3))


def _smooth_mc_mesh():
    """marching_cubes of a smooth random field: non-convex, with slivers."""
    from deepsdf_amd.mesh import marching_cubes
    g = np.random.default_rng(3)
    n = 28
    ax = np.meshgrid(*[np.linspace(-1, 1, n)] * 3, indexing="ij")
    f = np.sqrt(ax[0] ** 2 + ax[1] ** 2 + ax[2] ** 2) - 0.7
    for _ in range(5):
        k, ph = g.uniform(2, 6, 3), g.uniform(0, 2 * np.pi, 3)
        f += 0.08 * np.sin(k[0] * ax[0] + ph[0]) * np.sin(k[1] * ax[1] + ph[1]) * np.sin(k[2] * ax[2] + ph[2])
    h = 2.0 / (n - 1)
    v, fc = marching_cubes(torch.tensor(f, dtype=torch.float32, device="cuda"), 0.0, (h, h, h), (-1, -1, -1))
    return v.cpu().numpy().astype(np.float64), fc.cpu().numpy().astype(np.int64)


def _check_against_oracle(V, F, P):
    m = _mesh(V, F)
    sdf = m.sdf(P)
    d2, face, C = m.squared_distance(P)
    w = m.winding_number(P)
    assert sdf.dtype == np.float32 and d2.dtype == np.float32 and face.dtype == np.int32 and C.shape == (len(P), 3)
    rd2, _, _, rw = mn.mesh_query(V, F, P)
    rd = np.sqrt(rd2)
    rsdf = np.where(mn.inside(rw), -rd, rd)
    assert np.all(np.isfinite(sdf)) and np.all(np.isfinite(w))
    err = dict(sdf=np.abs(sdf - rsdf).max(), dist=np.abs(np.sqrt(d2) - rd).max())
    assert err["sdf"] <= TOL and err["dist"] <= TOL, err
    far = np.abs(rsdf) > SIGN_BAND
    assert np.array_equal(np.sign(sdf[far]), np.sign(rsdf[far]))
    # the returned face attains the minimum; the returned point lies on it AND is a closest point (|P - C| = the minimum)
    err["face"] = np.abs(mn.face_distance(V, F, P, face) - rd).max()
    assert err["face"] <= TOL, err
    err["on_face"] = mn.face_distance(V, F, C.astype(np.float64), face).max()
    assert err["on_face"] <= 1e-5, err
    err["closest"] = np.abs(np.linalg.norm(P.astype(np.float32).astype(np.float64) - C, axis=1) - rd).max()
    assert err["closest"] <= TOL, err
    away = rd > 1e-3
    err["w"] = np.abs(w[away] - rw[away]).max()
    assert err["w"] <= W_TOL, err
    return err


def test_cube_equals_the_box_sdf():
    V, F = mn.cube()
    g = np.random.default_rng(0)
    P = np.concatenate([g.uniform(-2, 2, (16000, 3)), _near_surface(V, F, 4000, 1, 1e-3)])
    sdf = _mesh(V, F).sdf(P)
    ref = mn.box_sdf(P.astype(np.float32).astype(np.float64))
    assert np.abs(sdf - ref).max() <= TOL
    far = np.abs(ref) > SIGN_BAND
    assert np.array_equal(np.sign(sdf[far]), np.sign(ref[far]))


@pytest.mark.parametrize("name", ["icosphere", "torus", "nested_shells", "two_parts", "marching_cubes"])
def test_meshes_match_the_oracle(name):
    V, F = _smooth_mc_mesh() if name == "marching_cubes" else dict(
        icosphere=lambda: mn.icosphere(3), torus=mn.torus, nested_shells=mn.nested_shells, two_parts=mn.two_parts)[name]()
    g = np.random.default_rng(7)
    P = np.concatenate([g.uniform(-1.2, 1.2, (2500, 3)), _near_surface(V, F, 1500, 8)])
    err = _check_against_oracle(V, F, P)
    print(name, len(F), {k: f"{v:.2e}" for k, v in err.items()})
    if name == "nested_shells":           # the cavity is outside (w = 2), the shell inside (w = 1)
        sdf = _mesh(V, F).sdf(np.array([[0, 0, 0], [0.65, 0, 0], [1.5, 0, 0]]))
        assert sdf[0] > 0 and sdf[1] < 0 and sdf[2] > 0


def test_orientation_open_surface_and_degenerate_faces():
    V, F = mn.torus()
    g = np.random.default_rng(11)
    P = np.concatenate([g.uniform(-1, 1, (2000, 3)), _near_surface(V, F, 1000, 12)])
    m, r = _mesh(V, F), _mesh(V, F[:, ::-1].copy())        # reversed faces: other vertex order, other rounding
    s, sr = m.sdf(P), r.sdf(P)
    assert np.abs(s - sr).max() <= 1e-6 and np.array_equal(np.sign(s[np.abs(s) > SIGN_BAND]), np.sign(sr[np.abs(s) > SIGN_BAND]))
    assert np.abs(m.winding_number(P) + r.winding_number(P)).max() <= 1e-5
    # open hemisphere: fractional winding numbers
    Vh, Fh = mn.hemisphere(2)
    Ph = g.uniform(-1.2, 1.2, (1500, 3))
    w = _mesh(Vh, Fh).winding_number(Ph)
    _, _, _, rw = mn.mesh_query(Vh, Fh, Ph)
    away = np.sqrt(mn.mesh_query(Vh, Fh, Ph)[0]) > 1e-3
    assert np.abs(w - rw)[away].max() <= W_TOL and np.abs(rw - np.round(rw)).max() > 0.1
    # appended zero-area faces: a repeated vertex, a point, and three collinear vertices
    nv = len(V)
    Vd = np.concatenate([V, [[0.1, 0.2, 0.3], [0.3, 0.2, 0.3], [0.5, 0.2, 0.3]]])
    Fd = np.concatenate([F, [[0, 0, 5], [7, 7, 7], [nv, nv + 1, nv + 2], [nv + 2, nv, nv + 1]]])
    md = _mesh(Vd, Fd)
    sdf = md.sdf(P)
    d2, face, C = md.squared_distance(P)
    assert np.all(np.isfinite(sdf)) and np.all(np.isfinite(d2)) and np.all(np.isfinite(C))
    rd2, _, _, rw = mn.mesh_query(Vd, Fd, P)
    rd = np.sqrt(rd2)
    assert np.abs(np.sqrt(d2) - rd).max() <= TOL
    rs = np.where(mn.inside(rw), -rd, rd)
    assert np.abs(sdf - rs).max() <= TOL
    assert np.abs(mn.face_distance(Vd, Fd, P, face) - rd).max() <= TOL


def test_split_and_call_determinism():
    from deepsdf_amd.meshsdf import TriangleMesh
    V, F = mn.icosphere(4)                                   # 5120 faces
    m = TriangleMesh(V, F)
    small, big = 300, 256 * 2048 + 77
    assert m.plan(small)[1] > 1 and m.plan(big)[1] == 1     # the two sides of the split threshold
    g = torch.Generator().manual_seed(5)
    Q = (torch.rand(big, 3, generator=g) * 2.4 - 1.2).cuda()
    a = m._query(Q[:small], sdf=True, dist=True, wind=True)
    b = m._query(Q, sdf=True, dist=True, wind=True)
    for k in ("d2", "face", "closest"):
        assert torch.equal(a[k], b[k][:small]), k
    assert (a["w"] - b["w"][:small]).abs().max().item() <= 1e-6
    assert torch.equal(a["sdf"], b["sdf"][:small])
    c = m._query(Q, sdf=True, dist=True, wind=True)
    for k in b:
        assert torch.equal(b[k], c[k]), k
    a2 = m._query(Q[:small], sdf=True, dist=True, wind=True)
    for k in a:
        assert torch.equal(a[k], a2[k]), k


def test_input_types_and_empty_queries():
    from deepsdf_amd.meshsdf import point_mesh_squared_distance, winding_number
    V, F = mn.icosphere(2)
    P = np.random.default_rng(2).uniform(-1, 1, (500, 3))
    d_np, i_np, c_np = point_mesh_squared_distance(P, V, F)
    assert isinstance(d_np, np.ndarray) and d_np.shape == (500,) and i_np.shape == (500,) and c_np.shape == (500, 3)
    d_cpu, i_cpu, c_cpu = point_mesh_squared_distance(torch.from_numpy(P), torch.from_numpy(V), torch.from_numpy(F))
    assert torch.is_tensor(d_cpu) and d_cpu.device.type == "cpu"
    d_dev, i_dev, c_dev = point_mesh_squared_distance(torch.from_numpy(P).cuda(), torch.from_numpy(V).cuda(),
                                                      torch.from_numpy(F).cuda())
    assert d_dev.is_cuda and i_dev.is_cuda and c_dev.is_cuda
    assert np.array_equal(d_np, d_cpu.numpy()) and np.array_equal(d_np, d_dev.cpu().numpy())
    assert np.array_equal(i_np, i_dev.cpu().numpy()) and np.array_equal(c_np, c_dev.cpu().numpy())
    w = winding_number(V, F, P)
    assert w.shape == (500,) and np.array_equal(w, winding_number(V, F, torch.from_numpy(P).cuda()).cpu().numpy())
    d0, i0, c0 = point_mesh_squared_distance(np.zeros((0, 3)), V, F)
    assert d0.shape == (0,) and i0.shape == (0,) and c0.shape == (0, 3)
    assert winding_number(V, F, torch.zeros(0, 3, device="cuda")).shape == (0,)


def test_sample_sdfs_into_training(tmp_path):
    from deepsdf_amd import train
    from deepsdf_amd.data import load_scene
    from deepsdf_amd.sdf_sampler import SDFfromMesh, SDFSampler
    meshes = [mn.icosphere(3, 0.6), mn.torus(0.55, 0.2, 40, 20)]
    data = tmp_path / "data"
    sampler = SDFSampler(str(data / "SdfSamples"), str(data / "splits"))
    os.makedirs(data / "splits")
    info = {"dataset_name": "synth", "class_name": "meshes"}
    n = 20000
    np.random.seed(4)
    split = sampler.sample_sdfs([SDFfromMesh(m) for m in meshes], info, n_samples=float(n))
    sampler.write_json("meshes.json", info, split)
    assert split == ["meshes_10000", "meshes_10001"]
    assert json.load(open(data / "splits" / "meshes.json")) == {"synth": {"meshes": split}}
    np.random.seed(4)
    for k, (V, F) in enumerate(meshes):
        xyz = np.random.uniform(-1, 1, (n, 3))
        d = SDFfromMesh((V, F))(xyz)                           # what the file must hold, split by sign
        with np.load(data / "SdfSamples" / "synth" / "meshes" / f"meshes_{10000 + k}.npz") as z:
            pos, neg = z["pos"], z["neg"]
        assert pos.dtype == np.float64 and neg.dtype == np.float64 and len(pos) + len(neg) == n
        assert np.all(pos[:, 3] >= 0) and np.all(neg[:, 3] < 0)
        assert np.array_equal(pos, np.hstack([xyz[d[:, 0] >= 0], d[d[:, 0] >= 0]]))
        assert np.array_equal(neg, np.hstack([xyz[d[:, 0] < 0], d[d[:, 0] < 0]]))
        ref = mn.mesh_sdf(V, F, xyz[:3000])
        assert np.abs(d[:3000, 0] - ref).max() <= TOL
        p_t, n_t = load_scene(str(data / "SdfSamples" / "synth" / "meshes" / f"meshes_{10000 + k}.npz"), 3)
        assert p_t.shape[0] + n_t.shape[0] == n and p_t.dtype == torch.float32
    # a short training run on that dataset
    exp = tmp_path / "exp"
    os.makedirs(exp)
    specs = {
        "Description": "sampled meshes", "DataSource": str(data), "NetworkArch": "deep_sdf_decoder",
        "TrainSplit": str(data / "splits" / "meshes.json"), "TestSplit": str(data / "splits" / "meshes.json"),
        "ReconstructionSplit": "",
        "NetworkSpecs": {"dims": [32] * 4, "dropout": [0, 1, 2, 3], "dropout_prob": 0.2, "norm_layers": [0, 1, 2, 3],
                         "latent_in": [2], "xyz_in_all": False, "use_tanh": False, "latent_dropout": False,
                         "weight_norm": True, "geom_dimension": 3},
        "CodeLength": 2, "NumEpochs": 2, "SnapshotFrequency": 2, "AdditionalSnapshots": [],
        "LearningRateSchedule": [{"Type": "Step", "Initial": 0.0005, "Interval": 500, "Factor": 0.5},
                                 {"Type": "Step", "Initial": 0.001, "Interval": 500, "Factor": 0.5}],
        "SamplesPerScene": 1024, "ScenesPerBatch": 2, "DataLoaderThreads": 1, "ClampingDistance": 0.1,
        "CodeRegularization": True, "CodeRegularizationLambda": 1e-4, "CodeBound": 1.0, "LogFrequency": 1}
    json.dump(specs, open(exp / "specs.json", "w"))
    torch.manual_seed(0)
    train.main_function(str(exp), None, 1)
    logs = torch.load(exp / "Logs.pth", weights_only=True)
    assert logs["epoch"] == 2 and len(logs["loss"]) > 0 and all(math.isfinite(v) for v in logs["loss"])


def test_sampling_cli_on_ply_and_obj(tmp_path):
    from deepsdf_amd.mesh import write_ply
    V, F = mn.icosphere(2, 0.5)
    write_ply(str(tmp_path / "ball.ply"), V.astype(np.float32), F.astype(np.int32))
    Vc, Fc = mn.cube(0.5)
    with open(tmp_path / "box.obj", "w") as fh:
        fh.writelines(f"v {x} {y} {z}\n" for x, y, z in Vc)
        fh.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in Fc)
    args = [sys.executable, os.path.join(ROOT, "sample_sdf_from_meshes.py"), "--data-dir", str(tmp_path / "data"), "--dataset",
            "ds", "--class", "shapes", "--split", "shapes.json", "--samples", "5000", "--seed", "0",
            str(tmp_path / "ball.ply"), str(tmp_path / "box.obj")]
    r = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ball.ply: 320 faces" in r.stdout and "box.obj: 12 faces" in r.stdout and "kernel" in r.stdout
    d = tmp_path / "data" / "SdfSamples" / "ds" / "shapes"
    assert sorted(os.listdir(d)) == ["shapes_10000.npz", "shapes_10001.npz"]
    assert json.load(open(tmp_path / "data" / "splits" / "shapes.json")) == {"ds": {"shapes": ["shapes_10000", "shapes_10001"]}}
    np.random.seed(0)
    np.random.uniform(-1, 1, (5000, 3))
    xyz = np.random.uniform(-1, 1, (5000, 3))                  # the second mesh's draw
    with np.load(d / "shapes_10001.npz") as z:
        rows = np.concatenate([z["pos"], z["neg"]])
    order = np.lexsort(rows[:, :3].T)
    ref = np.lexsort(xyz.T)
    assert np.array_equal(rows[order, :3], xyz[ref])
    assert np.abs(rows[order, 3] - mn.box_sdf(xyz[ref].astype(np.float32).astype(np.float64), 0.5)).max() <= TOL
