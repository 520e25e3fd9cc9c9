"""-m gpu: microstructure meshing.  The row kernel (dsdf_ms_rows) and the cap kernel (dsdf_ms_caps) against the numpy references
of tests/ms_numpy.py -- bit for bit where every operation is a single rounded one, within a derived bound for the spline --, the
grid's independence of the chunk size, an analytic structure end to end, the HIP decoder end to end against the fp64 oracle on
the kernel's own rows, sdf_struct, and the command line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests import mc_numpy, ms_numpy
from tests.golden_io import Golden, rel_err, worst_elem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_TOL = Y_ROW_TOL = 1e-5          # the decode tolerances of tests/test_gpu_parity.py
CASES = [([16, 16, 16], [2, 2, 2]), ([30, 21, 17], [3, 1, 4]), ([64, 48, 33], [5, 2, 7]), ([100, 100, 10], [6, 3, 1])]
# weights are non-negative and sum to one; each is a product of three axis values built in p recursion levels of about three
# roundings each, and the sum has at most 64 terms: error <= about (9p + 64) 2^-24 max|cp| (5.4e-6 for p = 3).  A factor 3 over it:
SPLINE_TOL = 2.0 ** -16


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def clamped(p, inner):
    return [-1.0] * (p + 1) + list(inner) + [1.0] * (p + 1)


# non-uniform, a repeated interior knot each, every value exact in fp32
KNOTS = {1: clamped(1, [-0.5, 0.25, 0.25, 0.625]), 2: clamped(2, [-0.375, 0.125, 0.125]), 3: clamped(3, [-0.25, 0.25, 0.25, 0.75])}


def make_field(degrees, L, seed, lo=-1.0, hi=1.0, knots=None):
    from deepsdf_amd.spline import BSplineField
    knots = knots or [KNOTS[p] for p in degrees]
    n = [len(U) - p - 1 for p, U in zip(degrees, knots)]
    cp = np.random.default_rng(seed).uniform(lo, hi, size=(n[0] * n[1] * n[2], L)).astype(np.float32)
    return BSplineField(degrees, knots, cp), knots, cp


def linear_field(cp):
    from deepsdf_amd.spline import BSplineField
    return BSplineField([1, 1, 1], [[-1, -1, 1, 1]] * 3, cp)


def test_public_names_import():
    from deep_sdf.mesh import CapBorderDict, create_mesh_microstructure      # noqa: F401
    from deepsdf_amd.spline import BSplineField                              # noqa: F401
    from deepsdf_amd import _lib
    assert _lib.lib().dsdf_abi_version() == 19


@pytest.mark.parametrize("N,tiling", CASES)
def test_rows_coordinates_and_inside_pattern_are_exact(N, tiling):
    from deepsdf_amd.mesh import ms_grid_rows
    L = 2
    field, _, _ = make_field((1, 1, 1), L, 1, lo=0.5, hi=1.5)        # positive control points: the spline is non-zero inside
    axes = ms_numpy.grid_axes(N, tiling)
    n = int(np.prod([len(a[0]) for a in axes]))
    rows = ms_grid_rows(field, tiling, N, 0, n).cpu().numpy()
    assert rows.shape == (n, L + 3)
    assert np.array_equal(bits(rows[:, L:]), bits(ms_numpy.grid_points(axes, 1)))
    inside = ms_numpy.grid_inside(axes)
    assert np.array_equal((rows[:, :L] != 0).all(1), inside)
    assert not bits(rows[~inside, :L]).any()                          # exact zeros, +0
    assert 0 < inside.sum() < n
    # a range in the middle of the grid equals the same rows of the whole
    part = ms_grid_rows(field, tiling, N, 777, 777 + 1234).cpu().numpy()
    assert np.array_equal(bits(part), bits(rows[777:777 + 1234]))


@pytest.mark.parametrize("L", [2, 16, 256])
@pytest.mark.parametrize("degrees", [(1, 1, 1), (2, 1, 3), (3, 3, 3)])
def test_rows_spline_columns_against_fp64(degrees, L):
    from deepsdf_amd.mesh import ms_grid_rows
    N, tiling = [30, 21, 17], [3, 1, 4]
    field, knots, cp = make_field(degrees, L, 7 + L)
    axes = ms_numpy.grid_axes(N, tiling)
    pts, inside = ms_numpy.grid_points(axes, 0), ms_numpy.grid_inside(axes)
    rows = ms_grid_rows(field, tiling, N, 0, len(pts)).cpu().numpy()
    want = ms_numpy.bspline_eval(degrees, knots, cp, pts[inside])
    err = np.abs(rows[inside, :L].astype(np.float64) - want).max() / np.abs(cp).max()
    print(f"spline columns degrees {degrees} L {L}: max error {err:.3e} of max|cp| (bound {SPLINE_TOL:.3e})")
    assert err <= SPLINE_TOL
    assert not bits(rows[~inside, :L]).any()


def test_point_list_mode():
    from deepsdf_amd.mesh import ms_grid_rows, ms_point_rows
    N, tiling, degrees, L = [30, 21, 17], [3, 1, 4], (2, 1, 3), 16
    field, knots, cp = make_field(degrees, L, 3)
    axes = ms_numpy.grid_axes(N, tiling)
    pts = ms_numpy.grid_points(axes, 0)
    grid_rows = ms_grid_rows(field, tiling, N, 0, len(pts))
    dev = torch.from_numpy(pts).cuda()
    on = ms_point_rows(field, tiling, dev, inside_test=True)
    assert np.array_equal(bits(on), bits(grid_rows))                  # flag on: the grid's own rows
    # flag off: every row carries the spline at the clamped point, the corners and faces of the domain included
    rng = np.random.default_rng(5)
    q = rng.uniform(-1.1, 1.1, size=(5000, 3)).astype(np.float32)
    q[:8] = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
    q[8:16, 0] = [1.0, -1.0, 1.05, -1.1, 0.25, -0.375, 0.125, 1.0000001]
    off = ms_point_rows(field, tiling, torch.from_numpy(q).cuda(), inside_test=False).cpu().numpy()
    want = ms_numpy.bspline_eval(degrees, knots, cp, np.clip(q, -1, 1))
    err = np.abs(off[:, :L].astype(np.float64) - want).max() / np.abs(cp).max()
    print(f"point list, inside test off: max error {err:.3e} of max|cp|")
    assert err <= SPLINE_TOL
    assert np.array_equal(bits(off[:, L:]), bits(np.stack([ms_numpy.fold(q[:, a], tiling[a]) for a in range(3)], 1)))
    outside = (np.abs(q) > 1).any(1)
    assert outside.sum() > 1000
    onq = ms_point_rows(field, tiling, torch.from_numpy(q).cuda(), inside_test=True).cpu().numpy()
    assert not bits(onq[outside, :L]).any() and np.array_equal(bits(onq[~outside]), bits(off[~outside]))
    # BSplineField.evaluate: the latent columns alone, tensors and arrays
    ev = field.evaluate(torch.from_numpy(q).cuda())
    assert ev.is_cuda and ev.shape == (5000, L) and np.array_equal(bits(ev), bits(off[:, :L]))
    assert np.array_equal(bits(field.evaluate(q)), bits(off[:, :L]))
    # assigning control points takes effect
    field.control_points = cp * 2
    ev2 = field.evaluate(q)
    assert np.abs(ev2.astype(np.float64) - 2 * want).max() <= 2 * SPLINE_TOL * np.abs(cp).max()


def test_caps_equal_numpy_bit_for_bit():
    from deepsdf_amd.mesh import ms_apply_caps
    N = [30, 21, 17]
    axes = ms_numpy.grid_axes(N, [1, 1, 1])
    xo = [a[0] for a in axes]
    dims = [len(x) for x in xo]
    n = int(np.prod(dims))
    sdf = np.random.default_rng(2).uniform(-0.3, 0.3, size=dims).astype(np.float32)
    full = {"x0": {"cap": 1, "measure": 0.1}, "x1": {"cap": -1, "measure": 0.25}, "y0": {"cap": -1, "measure": 0},
            "y1": {"cap": 1, "measure": 0.25}, "z0": {"cap": 1, "measure": 0}, "z1": {"cap": -1, "measure": 0.1}}
    rev = dict(reversed(list(full.items())))
    two = {"z1": {"cap": 1, "measure": 0.25}, "x0": {"cap": -1, "measure": 0.1}}
    results = []
    for d in (full, rev, two, None):
        v = torch.from_numpy(sdf.copy()).cuda().reshape(-1)
        ms_apply_caps(v, N, 0, n, d)
        want = ms_numpy.caps(sdf, xo, d if d is not None else {k: {"cap": -1, "measure": 0} for k in ms_numpy.LOCATION})
        assert np.array_equal(bits(v).reshape(dims), bits(want)), d
        results.append(bits(v).copy())
        # in three pieces: the same
        w = torch.from_numpy(sdf.copy()).cuda().reshape(-1)
        for s, e in ((0, 1000), (1000, 1001), (1001, n)):
            ms_apply_caps(w[s:e], N, s, e, d)
        assert torch.equal(w, v)
    assert not np.array_equal(results[0], results[1])          # the order matters: a min and a max do not commute


class SphereCells(torch.nn.Module):
    """|xyz| - z[0]: a sphere per unit cell whose radius is the (one) latent column."""

    def forward(self, x):
        return x[:, 1:].norm(dim=1, keepdim=True) - x[:, :1]


def _g6_decoder():
    from deepsdf_amd.decoder import Decoder
    g = Golden("g6_real_weights")
    params = g.group("params")
    dec = Decoder(g.meta["L"], **g.meta["net_specs"]).cuda().eval()
    dec.load_state_dict({k: v for k, v in params.items()})
    return g.meta["L"], g.meta["net_specs"], params, dec


def _codes(L, seed):
    c = torch.randn(8, L, generator=torch.Generator().manual_seed(seed)) * (0.5 / math.sqrt(L))
    assert float(c.norm(dim=1).max()) < 1
    return c.numpy()


def test_grid_does_not_depend_on_the_chunk_size():
    from deepsdf_amd.mesh import microstructure_sdf_grid
    N, tiling = [30, 21, 17], [3, 1, 4]
    L, _, _, dec = _g6_decoder()
    caps = {"x1": {"cap": 1, "measure": 0.1}, "z0": {"cap": -1, "measure": 0.25}}
    radius = linear_field(np.array([[0.35 if i % 2 == 0 else 0.6] for i in range(8)]))
    for name, d, field in (("analytic", SphereCells(), radius), ("hip", dec, linear_field(_codes(L, 4)))):
        grids = [microstructure_sdf_grid(tiling, d, field, N, mb, caps) for mb in (1000, 32 ** 3, 10 ** 7)]
        assert grids[0].shape == (32, 23, 19) and grids[0].is_cuda
        assert torch.equal(grids[0].view(torch.int32), grids[1].view(torch.int32)), name
        assert torch.equal(grids[0].view(torch.int32), grids[2].view(torch.int32)), name


def _components(n_verts, faces):
    parent = np.arange(n_verts)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for a, b, c in faces.tolist():
        ra, rb, rc = find(a), find(b), find(c)
        parent[rb] = ra
        parent[find(rc)] = ra
    return len({find(i) for i in range(n_verts)})


def test_analytic_structure_end_to_end():
    from deepsdf_amd.mesh import create_mesh_microstructure, microstructure_sdf_grid
    tiling, N = [3, 2, 1], [96, 64, 32]
    field = linear_field(np.array([[0.35 if i % 2 == 0 else 0.6] for i in range(8)]))
    dec = SphereCells()
    verts, faces = create_mesh_microstructure(tiling, dec, field, "unused", N=N)
    grid = microstructure_sdf_grid(tiling, dec, field, N)
    assert grid.shape == (98, 66, 34)
    vs = [2.0 / (n + 2 - 1 - 2) for n in N]
    vr, fr = mc_numpy.marching_cubes(grid.cpu().numpy(), 0.0, vs)
    vr = (vr - np.array(vs)) / 2
    assert verts.shape == vr.shape and np.array_equal(verts, vr) and np.array_equal(faces, fr)
    assert len(faces) > 1000
    assert _components(len(verts), faces) == 6                  # one blob per cell
    xo = 2.0 * verts - 1.0                                      # vertices come back in [0, 1]^3
    assert np.abs(xo).max() < 1 - 1e-3                          # nothing on a cap plane
    folded = np.empty_like(xo)
    for a, t in enumerate(tiling):
        p = 2.0 / t
        folded[:, a] = (2 / p) * np.abs(np.mod(xo[:, a] - t % 2, 2 * p) - p) - 1
    f = np.linalg.norm(folded, axis=1) - (0.35 + 0.25 * (xo[:, 0] + 1) / 2)
    lip = max(tiling) + 0.125
    diag = float(np.linalg.norm(vs))
    print(f"analytic structure: {len(verts)} vertices, {len(faces)} faces, max |f(v)| {np.abs(f).max():.3e}, bound {lip * diag:.3e}")
    assert np.abs(f).max() <= lip * diag


def _hip_cases():
    """(name, L, specs, params, Decoder, codes): the trained 4x64 net of golden G6 and a seeded 8x512, L = 256 net whose output
    bias is shifted so that its zero level set crosses the structure."""
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.mesh import microstructure_sdf_grid
    L, specs, params, dec = _g6_decoder()
    yield "g6", L, specs, params, dec, _codes(L, 4)
    m = Golden("g8_eval_8x512").meta
    L, specs = m["L"], m["net_specs"]
    net = orc.make_net(L, **specs)
    params = orc.init_params(net, 7)
    codes = _codes(L, 5)
    dec = Decoder(L, **specs).cuda().eval()
    dec.load_state_dict({k: v for k, v in params.items()})
    y = microstructure_sdf_grid([2, 2, 2], dec, linear_field(codes), 32, apply_caps=False)
    params["lin8.bias"] = params["lin8.bias"] - float(torch.atanh(y[1:-1, 1:-1, 1:-1].median()))
    dec.load_state_dict({k: v for k, v in params.items()})
    yield "8x512", L, specs, params, dec, codes


def test_hip_decoder_end_to_end(tmp_path):
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.mesh import (create_mesh_microstructure, microstructure_sdf_grid, ms_apply_caps, ms_grid_rows,
                                  ms_point_rows, sdf_struct)
    tiling, N = [2, 2, 2], 32
    n = 34 ** 3
    for name, L, specs, params, dec, codes in _hip_cases():
        field = linear_field(codes)
        net = orc.make_net(L, **specs)
        p64 = {k: v.double() for k, v in params.items()}
        rows = ms_grid_rows(field, tiling, N, 0, n)
        yo = orc.decoder_forward(net, p64, rows.cpu().double(), training=False)[0].reshape(-1)
        raw = microstructure_sdf_grid(tiling, dec, field, N, apply_caps=False)
        e, w = rel_err(raw.cpu().reshape(-1), yo), worst_elem(raw.cpu().reshape(-1), yo)
        print(f"{name}: grid before caps vs fp64 on the kernel's rows: rel err {e:.2e}, worst row {w:.2e}")
        assert e <= FWD_TOL and w <= Y_ROW_TOL, name
        capped = microstructure_sdf_grid(tiling, dec, field, N)
        again = raw.clone().reshape(-1)
        ms_apply_caps(again, [N] * 3, 0, n)
        assert torch.equal(capped.reshape(-1), again), name
        if name == "8x512":                                         # the same grid with the split GEMMs
            ds = Decoder(L, **dict(specs, gemm_split=True)).cuda().eval()
            ds.load_state_dict({k: v for k, v in params.items()})
            assert ds.engine().spec.gemm_split
            ys = microstructure_sdf_grid(tiling, ds, field, N, apply_caps=False).cpu().reshape(-1)
            es, wsp = rel_err(ys, yo), worst_elem(ys, yo)
            print(f"{name} gemm_split: rel err {es:.2e}, worst row {wsp:.2e}")
            assert es <= FWD_TOL and wsp <= Y_ROW_TOL
        # the PLY of save_ply_file against the mesh returned without it
        base = str(tmp_path / name)
        assert create_mesh_microstructure(tiling, dec, field, base, N=N, save_ply_file=True) is None
        _, v, f = mc_numpy.read_ply(base + ".ply")
        verts, faces = create_mesh_microstructure(tiling, dec, field, base, N=N)
        assert len(f) > 100 and len(v) == len(verts) and len(f) == len(faces), name
        assert np.array_equal(f, faces)
        vs = 2.0 / (N - 1)
        assert np.abs((v.astype(np.float64) + 1) / 2 - verts).max() <= 1e-6        # origin -1 - vs in the file, (v - vs) / 2 here
        # sdf_struct: the rows of the point-list mode, decoded
        q = (torch.rand(1000, 3, generator=torch.Generator().manual_seed(9)) * 2 - 1).numpy()
        want_rows = ms_point_rows(field, tiling, torch.from_numpy(q).cuda(), inside_test=False)
        seen = []

        class Recording(torch.nn.Module):
            def forward(self, x):
                seen.append(x.clone())
                return dec(x)

        via_module = sdf_struct(Recording(), q, tiling, field)
        assert len(seen) == 1 and np.array_equal(bits(seen[0]), bits(want_rows)), name
        direct = sdf_struct(dec, q, tiling, field)
        assert isinstance(direct, np.ndarray) and direct.shape == (1000,) and direct.dtype == np.float32
        yq = orc.decoder_forward(net, p64, want_rows.cpu().double(), training=False)[0].reshape(-1)
        for y in (via_module, direct):
            y = torch.from_numpy(y)
            assert rel_err(y, yq) <= FWD_TOL and worst_elem(y, yq) <= Y_ROW_TOL, name


# ---- the command line ---------------------------------------------------------------------------------------------------------
def _tiny_experiment(root, n_codes=9):
    """An experiment directory (reference layout) with a seeded 4x32 decoder whose zero level set crosses [-1, 1]^3."""
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.mesh import sdf_grid
    specs = {"Description": "microstructure test", "NetworkArch": "deep_sdf_decoder", "CodeLength": 4, "ClampingDistance": 0.1,
             "NetworkSpecs": {"dims": [32, 32, 32, 32], "dropout": [0, 1, 2, 3], "dropout_prob": 0.2, "norm_layers": [0, 1, 2, 3],
                              "latent_in": [2], "xyz_in_all": False, "use_tanh": False, "latent_dropout": False,
                              "weight_norm": True, "geom_dimension": 3}}
    torch.manual_seed(11)
    dec = Decoder(4, **specs["NetworkSpecs"]).cuda().eval()
    codes = torch.randn(n_codes, 4) * 0.01
    with torch.no_grad():
        y = sdf_grid(dec, codes[0].cuda(), 16, 4096)
        dec.lin4.bias -= torch.atanh(y.median())
    exp = os.path.join(root, "exp")
    for sub in ("ModelParameters", "LatentCodes"):
        os.makedirs(os.path.join(exp, sub))
    json.dump(specs, open(os.path.join(exp, "specs.json"), "w"))
    state = {"module." + k: v.detach().cpu() for k, v in dec.state_dict().items()}
    torch.save({"epoch": 5, "model_state_dict": state}, os.path.join(exp, "ModelParameters", "latest.pth"))
    torch.save({"epoch": 5, "latent_codes": {"weight": codes}}, os.path.join(exp, "LatentCodes", "latest.pth"))
    return exp


def test_create_microstructure_cli(tmp_path):
    from deepsdf_amd import meshsdf
    exp = _tiny_experiment(str(tmp_path))
    out = str(tmp_path / "structure.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_microstructure.py"), "-e", exp, "-c", "latest", "--tiling", "2",
                        "3", "1", "--codes", "0", "1", "2", "3", "4", "5", "6", "8", "--resolution", "32", "--cap", "x1=1:0.1",
                        "z0=-1:0", "-o", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert os.path.isfile(out)
    verts, faces = meshsdf.read_mesh(out)
    assert len(verts) > 0 and len(faces) > 0
