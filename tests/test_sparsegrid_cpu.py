"""Surface following on blocks of the dense grid, without a GPU: the numpy oracle (tests/sparsegrid_numpy.py) against the properties
DESIGN 4.16 proves, on the dense field it is handed; argument validation, the sparse_grid context manager, the command lines."""
import inspect
import math

import numpy as np
import pytest
import torch

from tests import mc_numpy, meshtopo_numpy as mt, sparsegrid_numpy as sg

DIMS = [(33, 33, 33), (38, 38, 38), (14, 10, 8), (5, 5, 5), (3, 2, 2), (2, 2, 2)]
BLOCKS = [2, 4, 8]


def _dense(field):
    """(verts, faces, the cell of every face, the component label of every face) of the dense mesh."""
    v, f = mc_numpy.marching_cubes(field)
    inside = field < 0
    nx, ny, nz = field.shape
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = mc_numpy.OFFS[c]
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    ntri = mc_numpy.NTRI[case].reshape(-1)
    cell = np.repeat(np.arange(ntri.size), ntri)                   # cells in linear order, then table order: the faces' order
    assert len(cell) == len(f)
    label = mt.components(mt.adjacency(f)[0], len(f))[0] if len(f) else np.zeros(0, np.int32)
    return v, f, cell, label


def _check(field, dense, b, lip, what):
    """The two properties of one run; returns the number of faces the run dropped."""
    v, f, cell, label = dense
    dims = field.shape
    r = sg.follow_surface(field, b, sg.threshold(b, sg.spacing(dims), lip))
    active = sg.cell_active(r, dims).reshape(-1)[cell] if len(f) else np.zeros(0, bool)
    touched = np.isin(label, np.unique(label[active]))
    assert np.array_equal(touched, active), (what, "a component leaves the active blocks")
    used = np.zeros(len(v), dtype=bool)
    used[f[touched].reshape(-1)] = True
    renumber = np.cumsum(used) - 1
    vs, fs = mc_numpy.marching_cubes(r.grid)
    assert np.array_equal(fs, renumber[f[touched]].astype(np.int32)), what
    assert np.array_equal(vs.view(np.uint32), v[used].view(np.uint32)), what
    assert r.stats["points"] == int(r.have.sum()) <= r.stats["total"] and r.stats["active"] == int(r.active.sum())
    assert r.stats["rounds"] == len(r.indices) and sum(len(i) for i in r.indices) + len(r.coarse) == r.stats["points"]
    return int((~touched).sum())


@pytest.mark.parametrize("dims", DIMS)
def test_oracle_meshes_are_the_dense_mesh_minus_unseeded_components(dims):
    fields = [(f"blobs{seed}", sg.blobs(dims, seed), False) for seed in range(20)]
    fields += [(name, fn(dims), name in sg.DISTANCE_FIELDS) for name, fn in sg.FIELDS.items()]
    dropped = faces = 0
    for name, field, distance in fields:
        dense = _dense(field)
        faces += len(dense[1])
        for b in BLOCKS:
            dropped += _check(field, dense, b, 0, (name, dims, b, 0))
            if distance:                                               # a true distance field at lipschitz 1: nothing is lost
                assert _check(field, dense, b, 1, (name, dims, b, 1)) == 0, (name, dims, b)
    if dims == (33, 33, 33):
        assert faces > 10000 and dropped > 0                           # the sign-only mode does lose components here


def test_the_issue_cases():
    rods = sg.rods((33, 33, 33))
    r = sg.follow_surface(rods, 4, 0.0)
    assert r.stats["seeds"] == 0 and r.stats["rounds"] == 0 and len(mc_numpy.marching_cubes(r.grid)[1]) == 0
    assert len(mc_numpy.marching_cubes(rods)[1]) > 1000
    for name, dims, b in (("sphere", (38,) * 3, 4), ("torus", (50,) * 3, 8)):
        assert sg.follow_surface(sg.FIELDS[name](dims), b, 0.0).stats["rounds"] >= 2
    g = sg.follow_surface(sg.gyroid((33,) * 3), 4, 0.0).stats
    assert g["active"] / g["blocks"] > 0.8
    assert sg.threshold(4, [0.5, 0.25, 0.125], 1.0) == np.float32(0.5 * math.sqrt(4 + 1 + 0.25))
    assert sg.coarse_coords(38, 4).tolist() == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 37] and sg.coarse_coords(2, 2).tolist() == [0, 1]
    assert sg.coarse_coords(33, 4).tolist() == list(range(0, 33, 4)) and sg.coarse_coords(5, 8).tolist() == [0, 4]


# ---- arguments ----------------------------------------------------------------------------------------------------------------------
class _Module(torch.nn.Module):
    def forward(self, x):
        return x[:, :1]


@pytest.mark.parametrize("block,lipschitz", [(1, 1.0), (0, 1.0), (-4, 1.0), (4.0, 1.0), ("4", 1.0), (True, 1.0), (4, -0.5),
                                             (4, float("nan")), (4, float("inf")), (4, "x"), (4, None)])
def test_bad_block_or_lipschitz_raise_value_error(block, lipschitz):
    from deepsdf_amd import mesh as M
    from deepsdf_amd.spline import BSplineField
    field = BSplineField([1, 1, 1], [[-1, -1, 1, 1]] * 3, np.zeros((8, 1), np.float32))
    with pytest.raises(ValueError):
        M.sdf_grid(_Module(), torch.zeros(1), 9, block=block, lipschitz=lipschitz)
    with pytest.raises(ValueError):
        M.microstructure_sdf_grid([1, 1, 1], _Module(), field, 8, block=block, lipschitz=lipschitz)
    with pytest.raises(ValueError):
        M.microstructure_mesh_diff([1, 1, 1], _Module(), field, 8, block=block, lipschitz=lipschitz)
    with pytest.raises(ValueError):
        with M.sparse_grid(block, lipschitz):
            pass
    assert M._SPARSE == [(None, 1.0)]


def test_sparse_grid_nests_and_restores():
    from deep_sdf.mesh import sparse_grid
    from deepsdf_amd import mesh as M
    assert M._SPARSE[-1] == (None, 1.0)
    with sparse_grid(4):
        assert M._SPARSE[-1] == (4, 1.0)
        with sparse_grid(np.int64(8), lipschitz=0):
            assert M._SPARSE[-1] == (8, 0.0)
            with sparse_grid(None):
                assert M._SPARSE[-1] == (None, 1.0)
            assert M._SPARSE[-1] == (8, 0.0)
        assert M._SPARSE[-1] == (4, 1.0)
        with pytest.raises(RuntimeError, match="inside"):
            with sparse_grid(2, 3.5):
                assert M._SPARSE[-1] == (2, 3.5)
                raise RuntimeError("inside")
        assert M._SPARSE[-1] == (4, 1.0)
    assert M._SPARSE == [(None, 1.0)]
    assert M.sparse_threshold(4, 0.5, 1.0) == float(np.float32(0.5 * math.sqrt(12.0))) and M.sparse_threshold(4, [1, 2, 3], 0) == 0.0


def test_reference_named_functions_keep_their_signatures():
    from deep_sdf import mesh as R
    names = lambda fn: list(inspect.signature(fn).parameters)                      # noqa: E731
    assert names(R.create_mesh) == ["decoder", "latent_vec", "filename", "N", "max_batch", "offset", "scale", "device"]
    assert names(R.create_mesh_microstructure) == [
        "tiling", "decoder", "latent_vec_interpolation", "filename", "N", "max_batch", "offset", "scale", "cap_border_dict",
        "save_ply_file", "use_flexicubes", "device", "output_tetmesh", "compute_derivatives"]
    assert names(R.create_mesh_microstructure_diff) == [
        "tiling", "decoder", "latent_vec_interpolation", "N", "max_batch", "offset", "scale", "cap_border_dict", "device",
        "output_tetmesh", "compute_derivatives"]
    from deepsdf_amd import mesh as M
    for fn in (M.sdf_grid, M.microstructure_sdf_grid, M.microstructure_mesh_diff):
        p = inspect.signature(fn).parameters
        assert p["block"].kind is p["lipschitz"].kind is inspect.Parameter.KEYWORD_ONLY
        assert p["block"].default is None and p["lipschitz"].default == 1.0
    assert names(M.follow_surface)[:6] == ["dims", "block", "thr", "level", "values_at", "caps_at"]


def test_command_lines_parse_block_and_lipschitz():
    import create_microstructure
    import create_ply_files_from_latent
    import reconstruct
    cases = [(create_ply_files_from_latent, ["-e", "exp"]),
             (create_microstructure, ["-e", "exp", "--tiling", "1", "1", "1", "--codes", "0", "-o", "out"]),
             (reconstruct, ["-e", "exp", "-d", "data", "-s", "split.json", "--mesh", "64"])]
    for mod, base in cases:
        a = mod.build_parser().parse_args(base)
        assert a.block is None and a.lipschitz == 1.0
        a = mod.build_parser().parse_args(base + ["--block", "4", "--lipschitz", "0"])
        assert a.block == 4 and a.lipschitz == 0.0
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(base + ["--block", "4.5"])


def test_library_refuses_bad_plans_on_the_host():
    import ctypes as C
    from deepsdf_amd import _lib
    lib = _lib.lib()
    plan = _lib.DsdfSgPlan()
    for args in ((33, 33, 33, 1), (33, 33, 33, 0), (1, 33, 33, 4), (33, 1025, 33, 4), (33, 33, 33, -2)):
        assert lib.dsdf_sg_plan(*args, C.byref(plan)) == -1, args
    assert lib.dsdf_sg_plan(33, 33, 33, 4, None) == -1
    for dims, b in (((38, 38, 38), 4), ((14, 10, 8), 4), ((5, 5, 5), 8), ((2, 2, 2), 2), ((1024, 2, 7), 2 ** 31 - 1)):
        _lib.check(lib.dsdf_sg_plan(*dims, b, C.byref(plan)))
        c = [sg.coarse_coords(n, min(b, 1024)) for n in dims]
        assert list(plan.blocks) == [len(x) - 1 for x in c] and plan.n_coarse == int(np.prod([len(x) for x in c]))
        assert plan.n_points == int(np.prod(dims)) and plan.n_blocks == int(np.prod(plan.blocks))
        rows, total = _lib.ws_regions()
        assert total == plan.ws_bytes and [r[0] for r in rows] == ["sg_state", "sg_pend", "sg_have", "sg_part", "sg_offs"]
    assert lib.dsdf_abi_version() == 19                                              # additions only
