"""-m gpu: HIP marching cubes (dsdf_mc_count / dsdf_mc_emit) against the numpy reference of tests/mc_numpy.py, array for array;
the grid decode of create_mesh against Engine.decode_latent and the fp64 oracle; the meshing CLIs end to end."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests import mc_numpy
from tests.golden_io import Golden, rel_err, sphere_npz

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_TOL = 1e-5          # the decode tolerance of tests/test_gpu_parity.py


def _gpu_mc(grid, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0)):
    from deepsdf_amd.mesh import marching_cubes
    v, f = marching_cubes(torch.as_tensor(grid).cuda(), level, spacing, origin)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and f.is_cuda
    return v.cpu().numpy(), f.cpu().numpy()


def _same_bits(what, v, vr):
    """The vertices are the specification's bit for bit; the count of differing coordinates and their distance are printed first."""
    assert v.dtype == np.float32 and vr.dtype == np.float32 and v.shape == vr.shape
    d, n = mc_numpy.differing(v, vr)
    if d:
        print(f"{what}: {d} of {n} coordinates differ from the single-rounded specification, by at most {mc_numpy.ulp_distance(v, vr)} ulp")
    assert d == 0, (what, d, n)


def _has_power(what, grid, level, spacing, origin, vr):
    """The input tells a fused origin + x * spacing from the specification: at least a tenth of the coordinates differ."""
    d, n = mc_numpy.differing(vr, mc_numpy.vertices(np.asarray(grid), level, spacing, origin, contracted=True))
    print(f"{what}: a fused last step would change {d} of {n} coordinates")
    assert d >= 0.1 * n, (what, d, n)


def _same_mesh(grid, level=0.0, spacing=(1, 1, 1), origin=(0, 0, 0), power=False):
    v, f = _gpu_mc(grid, level, spacing, origin)
    vr, fr = mc_numpy.marching_cubes(np.asarray(grid), level, spacing, origin)
    assert f.shape == fr.shape and np.array_equal(f, fr)
    if power:
        _has_power("input", grid, level, spacing, origin, vr)
    _same_bits(f"grid {tuple(np.asarray(grid).shape)}", v, vr)
    return v, f


_smooth = mc_numpy.smooth_field


def test_analytic_fields_match_numpy_and_are_closed():
    for make, chi in ((mc_numpy.sphere, 2), (mc_numpy.torus, 0)):
        sdf, h = make(64)
        v, f = _same_mesh(sdf, 0.0, (h, h, h), (-1, -1, -1), power=True)
        ok, euler, vol = mc_numpy.closed_manifold_stats(v, f)
        assert ok and euler == chi and vol > 0


def test_random_and_quantised_fields_on_a_non_cubic_grid():
    g = _smooth((33, 40, 47), 5)
    v, f = _same_mesh(g, 0.1, (0.5, 0.25, 2.0), (3.0, -1.0, 0.5))
    assert len(f) > 1000
    q = np.round(g * 8) / 8                             # values land exactly on the level
    assert (q == 0.125).sum() > 100
    for level in (0.125, 0.0):
        _same_mesh(q.astype(np.float32), level)


def test_non_dyadic_spacing_and_origin_bit_for_bit_and_from_the_edges():
    """Spacing and origin that are not dyadic on any axis: x * spacing is inexact, so a contracted origin + x * spacing would show in
    the bits (asserted on the oracle first).  Every vertex recomputed from its edge (p, a) and the edge's two grid values with the
    specification's formula is the returned vertex."""
    from deepsdf_amd.mesh import marching_cubes
    from tests import msdiff_numpy
    nd = mc_numpy.NON_DYADIC
    g = _smooth(nd["shape"], nd["seed"])
    level, spacing, origin = nd["level"], nd["spacing"], nd["origin"]
    v, f = _same_mesh(g, level, spacing, origin, power=True)
    assert len(f) > 1000
    verts, faces, ep, ea = marching_cubes(torch.from_numpy(g).cuda(), level, spacing, origin, return_edges=True)
    assert np.array_equal(verts.cpu().numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(faces.cpu().numpy(), f)
    ep, ea = ep.cpu().numpy(), ea.cpu().numpy()
    wp, wa = msdiff_numpy.edges(g, level)
    assert np.array_equal(ep, wp) and np.array_equal(ea, wa) and set(ea.tolist()) == {0, 1, 2}
    _same_bits("vertices from their edges", v, msdiff_numpy.vertices_from_edges(g, ep, ea, level, spacing, origin))


def test_all_256_cases_on_2x2x2_grids():
    from deepsdf_amd import mc_table
    for case in range(256):
        grid = np.ones((2, 2, 2), np.float32)
        for c in range(8):
            if (case >> c) & 1:
                grid[mc_table.corner_pos(c)] = -1.0 - 0.125 * c
        v, f = _same_mesh(grid)
        assert len(f) == len(mc_table.TABLE[case]) and len(v) == sum(
            1 for e in range(12) if e in {x for t in mc_table.TABLE[case] for x in t})


def test_two_runs_give_identical_bytes():
    g = torch.from_numpy(_smooth((40, 40, 40), 9)).cuda()
    from deepsdf_amd.mesh import marching_cubes
    a, b = marching_cubes(g, 0.05), marching_cubes(g, 0.05)
    assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes()
    assert a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()


def test_empty_surface(tmp_path):
    from deepsdf_amd.mesh import convert_sdf_samples_to_ply, marching_cubes
    g = torch.full((9, 10, 11), 0.5, device="cuda")
    v, f = marching_cubes(g)
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.is_cuda
    v, f = marching_cubes(g, level=0.5)                 # equal to the level counts as outside: still empty
    assert v.shape == (0, 3)
    with pytest.raises(ValueError):
        convert_sdf_samples_to_ply(g.cpu(), [-1, -1, -1], 0.1, str(tmp_path / "x.ply"))
    assert not os.path.exists(tmp_path / "x.ply")


def test_large_sphere_n256():
    sdf, h = mc_numpy.sphere(256)
    v, f = _same_mesh(sdf, 0.0, (h, h, h), (-1, -1, -1), power=True)
    ok, euler, vol = mc_numpy.closed_manifold_stats(v, f)
    assert ok and euler == 2 and abs(vol - 4 / 3 * math.pi * 0.125) <= 2e-3 * vol


# ---- create_mesh -------------------------------------------------------------------------------------------------------------
def _nets():
    """(name, Decoder, params, latent): the trained 4x64 net of golden G6 and a seeded 8x512 net whose output bias is shifted
    so that its zero level set crosses the grid."""
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.mesh import grid_coords
    out = []
    g = Golden("g6_real_weights")
    p6 = g.group("params")
    out.append(("g6", g.meta["L"], g.meta["net_specs"], p6, torch.zeros(g.meta["L"])))
    m = Golden("g8_eval_8x512").meta
    net = orc.make_net(m["L"], **m["net_specs"])
    p8 = orc.init_params(net, 7)
    z8 = torch.randn(m["L"], generator=torch.Generator().manual_seed(1)) / math.sqrt(m["L"])
    xyz = grid_coords(12, 0, 12 ** 3)
    y = orc.decoder_forward(net, p8, torch.cat([z8.expand(xyz.shape[0], -1), xyz], 1), training=False)[0]
    p8["lin8.bias"] = p8["lin8.bias"] - float(torch.atanh(y.median()))
    out.append(("8x512", m["L"], m["net_specs"], p8, z8))
    res = []
    for name, L, specs, params, z in out:
        dec = Decoder(L, **specs).cuda()
        dec.load_state_dict({k: v for k, v in params.items()})
        res.append((name, L, specs, params, z, dec))
    return res


def test_create_mesh_on_real_and_seeded_weights(tmp_path):
    from deepsdf_amd.mesh import create_mesh, grid_coords, sdf_grid
    N, mb = 64, 32 ** 3
    h = 2.0 / (N - 1)
    for name, L, specs, params, z, dec in _nets():
        dec.eval()
        grid = sdf_grid(dec, z.cuda(), N, mb)
        eng = dec.engine()
        assert eng.decode_latent_supported()
        ref = torch.cat([eng.decode_latent(z.cuda(), grid_coords(N, s, min(N ** 3, s + mb), device="cuda")).reshape(-1)
                         for s in range(0, N ** 3, mb)])
        assert torch.equal(grid.reshape(-1).view(torch.int32), ref.view(torch.int32)), name
        net = orc.make_net(L, **specs)
        sel = torch.arange(0, N ** 3, 1 if name == "g6" else 61)
        xyz = grid_coords(N, 0, N ** 3)[sel]
        yo = orc.decoder_forward(net, {k: v.double() for k, v in params.items()},
                                 torch.cat([z.double().expand(len(sel), -1), xyz.double()], 1), training=False)[0]
        assert rel_err(grid.reshape(-1)[sel.cuda()].cpu(), yo) <= FWD_TOL, name
        path = str(tmp_path / f"{name}")                # written exactly as given: no suffix added
        create_mesh(dec, z.cuda(), path, N=N, max_batch=mb)
        _, v, f = mc_numpy.read_ply(path)
        vr, fr = mc_numpy.marching_cubes(grid.cpu().numpy(), 0.0, (h, h, h), (-1, -1, -1))
        assert len(f) > 100 and np.array_equal(f, fr), name
        _has_power(name, grid.cpu().numpy(), 0.0, (h, h, h), (-1, -1, -1), vr)
        _same_bits(name, v, vr)                          # no host arithmetic between the kernel and the file


def test_create_mesh_offset_scale_and_stock_module(tmp_path):
    from deepsdf_amd.mesh import create_mesh

    class Sphere(torch.nn.Module):       # a decoder that is not this package's: called on the chunk's [latent | xyz]
        def forward(self, x):
            return (x[:, 1:].norm(dim=1, keepdim=True) - 0.5) + 0 * x[:, :1]

    N = 40
    h = 2.0 / (N - 1)
    create_mesh(Sphere(), torch.zeros(1), str(tmp_path / "s.ply"), N=N, max_batch=5000, offset=np.array([0.5, 0, -1.0]),
                scale=2.0)
    _, v, f = mc_numpy.read_ply(str(tmp_path / "s.ply"))
    from deepsdf_amd.mesh import grid_coords, sdf_grid
    grid = sdf_grid(Sphere(), torch.zeros(1), N, 5000).cpu().numpy()
    assert np.abs(grid - (grid_coords(N, 0, N ** 3).norm(dim=1) - 0.5).reshape(N, N, N).numpy()).max() <= 1e-6
    vr, fr = mc_numpy.marching_cubes(grid, 0.0, (h, h, h), (-1, -1, -1))
    assert np.array_equal(f, fr)
    _has_power("sphere", grid, 0.0, (h, h, h), (-1, -1, -1), vr)
    # the host step as convert_sdf_samples_to_ply does it: an fp32 division by the scale, then an fp32 subtraction of the offset
    _same_bits("offset and scale", v, (vr / np.float32(2.0)) - np.array([0.5, 0, -1.0], np.float32))


def test_variant_net_takes_the_engine_decode_path():
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.mesh import grid_coords, marching_cubes, sdf_grid
    torch.manual_seed(4)
    dec = Decoder(3, [64, 64, 64], 3, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=False, xyz_in_all=True).cuda().eval()
    assert not dec.engine().decode_latent_supported()
    z = torch.randn(3) * 0.1
    N, mb = 32, 4096
    grid = sdf_grid(dec, z.cuda(), N, mb)
    with torch.no_grad():
        fwd = torch.cat([dec(torch.cat([z.cuda().expand(min(N ** 3, s + mb) - s, -1),
                                        grid_coords(N, s, min(N ** 3, s + mb), device="cuda")], 1)).reshape(-1)
                         for s in range(0, N ** 3, mb)])
    med = float(fwd.median())
    assert torch.equal(grid.reshape(-1), fwd)
    a, b = marching_cubes(grid, med), marching_cubes(fwd.view(N, N, N), med)
    assert len(a[1]) > 0 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the CLIs ----------------------------------------------------------------------------------------------------------------
def _tiny_experiment(root, n_codes=9):
    """An experiment directory (reference layout) with a seeded 4x32 decoder whose zero level set crosses [-1, 1]^3."""
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.mesh import sdf_grid
    specs = {"Description": "mesh test", "NetworkArch": "deep_sdf_decoder", "CodeLength": 4, "ClampingDistance": 0.1,
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


def _run(args, timeout=300):
    r = subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_create_ply_files_from_latent_cli(tmp_path):
    exp = _tiny_experiment(str(tmp_path))
    _run([os.path.join(ROOT, "create_ply_files_from_latent.py"), "-e", exp, "-c", "latest", "--resolution", "32", "-b", "16"])
    base = os.path.join(exp, "Reconstructions", "latest", "Meshes", "latent_recon")
    want = [os.path.join(base, "all", f"{i}.ply") for i in range(9)]
    want += [os.path.join(base, "interpolation", f"interpolate_{a}_{a + 1}_{s}.ply") for a in range(1, 8) for s in range(11)]
    missing = [w for w in want if not os.path.isfile(w)]
    assert not missing, missing[:5]
    _, v, f = mc_numpy.read_ply(want[0])
    assert len(f) > 0 and len(v) > 0
    r = _run([os.path.join(ROOT, "create_ply_files_from_latent.py"), "-e", exp, "-c", "latest", "--resolution", "32"])
    assert r.stdout.count("Skipping") == len(want)      # the skip check works on the files it writes


def test_reconstruct_cli_writes_its_mesh(tmp_path):
    exp = _tiny_experiment(str(tmp_path))
    data = os.path.join(str(tmp_path), "data")
    os.makedirs(os.path.join(data, "SdfSamples", "synth", "spheres"))
    sphere_npz(os.path.join(data, "SdfSamples", "synth", "spheres", "s0.npz"), 0, n=2000)
    split = os.path.join(str(tmp_path), "split.json")
    json.dump({"synth": {"spheres": ["s0"]}}, open(split, "w"))
    _run([os.path.join(ROOT, "reconstruct.py"), "-e", exp, "-c", "latest", "-d", data, "-s", split, "--iters", "3",
          "--samples", "512", "--mesh", "32"])
    code = os.path.join(exp, "Reconstructions", "5", "Codes", "synth", "spheres", "s0.pth")
    mesh = os.path.join(exp, "Reconstructions", "5", "Meshes", "synth", "spheres", "s0.ply")
    assert os.path.isfile(code) and os.path.isfile(mesh)
    _, v, f = mc_numpy.read_ply(mesh)
    assert len(f) > 0 and len(v) > 0
