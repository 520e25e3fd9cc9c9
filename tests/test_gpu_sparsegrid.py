"""-m gpu: surface following on blocks of the dense grid (csrc/sparsegrid.hpp, deepsdf_amd.mesh.follow_surface) against the numpy
oracle of tests/sparsegrid_numpy.py, array for array; the sparse meshing paths against the dense ones."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import mc_numpy, meshtopo_numpy as mt, sparsegrid_numpy as sg, ws_guard as G
from tests.golden_io import Golden, rel_err

pytestmark = pytest.mark.gpu

FWD_TOL = 1e-5          # the decode tolerance of tests/test_gpu_parity.py


def bits(x):
    x = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _lookup(table, chunk=None):
    """values_at / caps_at by table look-up; chunk: in pieces of that many indices, ragged tail included, as the decoders' closures."""
    from deepsdf_amd.mesh import _padded_chunks
    t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).cuda().reshape(-1)
    if chunk is None:
        return lambda idx, *_: t[idx]

    def values_at(idx, *_):
        out = torch.empty(idx.numel(), dtype=torch.float32, device="cuda")
        for s, e, piece in _padded_chunks(idx, chunk, 0):
            assert piece.numel() == e - s <= chunk
            out[s:e] = t[piece]
        return out
    return values_at


class _Trace:
    """follow_surface's on_step: the arrays of every step, copied from the run's workspace."""

    def __init__(self):
        self.items = []

    def __call__(self, name, ws, plan, indices):
        states = lambda: ws[plan.state_offset:plan.state_offset + plan.n_blocks].clone()      # noqa: E731
        if name in ("coarse", "emit"):
            self.items.append(("coarse" if name == "coarse" else "indices", indices.clone()))
        elif name == "seed":
            self.items.append(("seeds", states()))
        elif name == "grow":
            self.items.append(("states", states()))
        elif name == "fill":
            self.items.append(("have", ws[plan.have_offset:plan.have_offset + plan.n_points].clone()))


def _follow(field, b, thr, capped=None, chunk=None):
    from deepsdf_amd.mesh import follow_surface
    tr = _Trace()
    grid, cap, stats = follow_surface(list(field.shape), b, thr, 0.0, _lookup(field, chunk),
                                      None if capped is None else _lookup(capped, chunk), on_step=tr)
    return grid, cap, stats, tr.items


# ---- 3. the machinery against the oracle ------------------------------------------------------------------------------------------
# (field, dims, b, lipschitz, rounds at least)
MACHINERY = [
    ("sphere", (38, 38, 38), 4, 0, 2),             # short last block; grows
    ("torus", (50, 50, 50), 8, 0, 2),              # grows
    ("gyroid", (33, 33, 33), 4, 0, 1),             # most blocks active
    ("rods", (33, 33, 33), 4, 0, 0),               # zero seeds: no decode round
    ("rods", (33, 33, 33), 4, 1, 1),               # all seeded by distance
    ("sphere_bubble", (33, 33, 33), 4, 0, 1),      # the bubble's 8 cells are lost
    ("sphere_bubble", (33, 33, 33), 4, 1, 1),      # none lost
    ("sphere", (33, 33, 33), 4, 0, 1),             # exact zeros at block corners
    ("gyroid", (14, 10, 8), 4, 0, 1),              # anisotropic, short blocks on every axis
    ("sphere", (14, 10, 8), 4, 1, 1),
    ("sphere", (5, 5, 5), 8, 0, 0),                # one block, larger than the grid
    ("sphere", (5, 5, 5), 8, 1, 1),
    ("sphere", (2, 2, 2), 2, 1, 0),                # the minimal grid
    ("gyroid", (2, 2, 2), 2, 0, 0),
]


def _compare(case, field, b, thr, capped=None, chunk=None):
    r = sg.follow_surface(field, b, thr, 0.0, capped)
    grid, cap, stats, dbg = _follow(field, b, thr, capped, chunk)
    got = {}
    for name, t in dbg:
        got.setdefault(name, []).append(t.cpu().numpy())
    assert np.array_equal(got["coarse"][0], r.coarse), case
    assert np.array_equal(got["seeds"][0], r.seeds), case
    assert len(got.get("indices", [])) == len(r.indices) == len(got.get("states", [])), (case, len(r.indices))
    for k, want in enumerate(r.indices):
        assert got["indices"][k].dtype == np.int64 and np.array_equal(got["indices"][k], want), (case, "round", k)
        assert np.array_equal(got["states"][k], r.states[k]), (case, "states after round", k)
    assert np.array_equal(got["have"][0], r.have), case
    assert np.array_equal(bits(grid), bits(r.grid)), case
    if capped is not None:
        assert np.array_equal(bits(cap), bits(r.capped)), case
    assert stats == r.stats, (case, stats, r.stats)
    return r


@pytest.mark.parametrize("name,dims,b,lip,min_rounds", MACHINERY)
def test_machinery_equals_the_oracle_array_for_array(name, dims, b, lip, min_rounds):
    field = sg.FIELDS[name](dims)
    thr = sg.threshold(b, sg.spacing(dims), lip)
    r = _compare((name, dims, b, lip), field, b, thr, chunk=37 if dims == (38, 38, 38) else None)    # rounds over many ragged chunks
    print(f"{name} {dims} b={b} lipschitz={lip}: {r.stats}")
    assert r.stats["rounds"] >= min_rounds, r.stats           # a case that never grows shows nothing about growth
    dense = mc_numpy.marching_cubes(field)[1]
    sparse = mc_numpy.marching_cubes(r.grid)[1]
    if name == "rods" and lip == 0:
        assert r.stats["seeds"] == 0 and len(sparse) == 0 and len(dense) > 0
    elif name == "sphere_bubble" and lip == 0:
        lost = (mc_numpy.NTRI[_cases(field)] > 0).sum() - (mc_numpy.NTRI[_cases(r.grid)] > 0).sum()
        assert lost == 8, lost
    elif lip == 1 or name != "sphere" or dims != (5, 5, 5):
        assert len(sparse) == len(dense)
    if name == "sphere" and dims == (33, 33, 33):
        corner = field[np.ix_(*r.coords)]
        assert (corner == 0).any() and not (corner < 0).all()
        # a block all of whose corners are outside, seeded by the exact zero alone
        assert r.stats["seeds"] > sg.follow_surface(np.where(field == 0, np.float32(1e-6), field), b, thr).stats["seeds"]


def test_emitted_points_on_both_sides_of_the_offset_scan_pass_border():
    """The points pass has more per-workgroup totals than one pass of offset_scan_kernel takes, and the emitted indices lie on both
    sides of that border: their offsets are right only if the scan's carry is."""
    k = G.constants()
    dims, b, h = (132, 128, 128), 8, 2.0 / 127
    i, j, kk = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in dims], indexing="ij")
    r2 = (i - np.float32(125.25)) ** 2 + (j - np.float32(64.5)) ** 2 + (kk - np.float32(63.75)) ** 2
    field = ((np.sqrt(r2) - np.float32(6)) * np.float32(h)).astype(np.float32)
    r = _compare(("small sphere at the far end", dims, b, 1), field, b, sg.threshold(b, (h, h, h), 1))
    print(f"{dims} b={b}: {r.stats}, indices {[(int(x.min()), int(x.max())) for x in r.indices]}")
    assert r.stats["rounds"] == 1 and r.stats["seeds"] > 0
    per_pass = k["MC_SCAN_THREADS"] * k["MC_SCAN_PER_THREAD"]             # totals per pass; one total per SG_BLOCK points
    assert -(-field.size // k["SG_BLOCK"]) > per_pass
    assert r.indices[0].min() // k["SG_BLOCK"] < per_pass <= r.indices[0].max() // k["SG_BLOCK"]


def _cases(grid):
    inside = grid < 0
    nx, ny, nz = grid.shape
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        dx, dy, dz = mc_numpy.OFFS[c]
        case |= inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].astype(np.int64) << c
    return case


def test_machinery_with_a_capped_grid_and_a_padded_anisotropic_grid():
    dims = (12 + 2, 8 + 2, 6 + 2)
    X = np.meshgrid(*[np.linspace(-1, 1, n) for n in dims], indexing="ij")[0]
    for name in ("gyroid", "sphere"):
        raw = sg.FIELDS[name](dims)
        capped = np.maximum(raw, (X - 0.3).astype(np.float32))      # a cut that removes surface and adds a plane
        r = _compare((name, "capped"), raw, 4, sg.threshold(4, sg.spacing(dims), 0), capped, chunk=37)
        assert r.stats["active"] > 0 and not np.array_equal(r.grid, r.capped)
        assert len(mc_numpy.marching_cubes(r.capped)[1]) == len(mc_numpy.marching_cubes(capped)[1])


# ---- 9. every entry under red zones, on a poisoned workspace ----------------------------------------------------------------------
def _raw_run(field, b, thr, fill=None):
    """The run of follow_surface through the C entries, with assert_clean after every call when `fill` is given."""
    from deepsdf_amd import _lib
    lib = _lib.lib()
    dims = field.shape
    plan = _lib.DsdfSgPlan()
    _lib.check(lib.dsdf_sg_plan(*dims, b, C.byref(plan)))
    ws = G.poisoned(plan.ws_bytes, fill) if fill is not None else torch.zeros(plan.ws_bytes, dtype=torch.uint8, device="cuda")
    f = G.Fences()
    table = torch.from_numpy(field).cuda().reshape(-1)
    grid = f.new("grid", plan.n_points)
    counts = f.new("counts", 2, torch.int64)
    at, wsa = (*dims, b), (G.ptr(ws), plan.ws_bytes, G.stream())
    n_new, n_pts = C.c_void_p(counts.data_ptr()), C.c_void_p(counts.data_ptr() + 8)
    out = []

    def clean(what):
        if fill is not None:
            G.assert_clean(ws, fill, (dims, b, what))
            f.check((dims, b, what))

    def decode(idx):
        vals = table[idx].contiguous()
        _lib.check(lib.dsdf_sg_scatter(G.ptr(idx), idx.numel(), G.ptr(vals), G.ptr(grid), plan.n_points, G.stream()))
        out.append(idx.cpu().numpy())

    idx = f.new("coarse", plan.n_coarse, torch.int64)
    _lib.check(lib.dsdf_sg_coarse(*at, G.ptr(idx), *wsa))
    clean("coarse")
    decode(idx)
    _lib.check(lib.dsdf_sg_seed(G.ptr(grid), *at, 0.0, float(thr), n_new, *wsa))
    clean("seed")
    _lib.check(lib.dsdf_sg_points_count(*at, n_pts, *wsa))
    clean("points_count")
    new, pts = counts.tolist()
    while new > 0:
        idx = f.new(f"round{len(out)}", pts, torch.int64)
        _lib.check(lib.dsdf_sg_points_emit(*at, pts, G.ptr(idx), *wsa))
        clean("points_emit")
        decode(idx)
        _lib.check(lib.dsdf_sg_grow(G.ptr(grid), *at, 0.0, n_new, *wsa))
        clean("grow")
        _lib.check(lib.dsdf_sg_points_count(*at, n_pts, *wsa))
        clean("points_count")
        new, pts = counts.tolist()
    _lib.check(lib.dsdf_sg_fill(G.ptr(grid), *at, *wsa))
    clean("fill")
    out.append(bits(grid))
    return out


@pytest.mark.parametrize("name,dims,b", [("sphere", (38, 38, 38), 4), ("torus", (50, 50, 50), 8), ("gyroid", (33, 33, 33), 4),
                                         ("gyroid", (14, 10, 8), 4)])
def test_workspace_entries_under_red_zones(name, dims, b):
    from deepsdf_amd import _lib
    field = sg.FIELDS[name](dims)
    plain = _raw_run(field, b, 0.0)
    with G.redzone():
        runs = [_raw_run(field, b, 0.0, fill) for fill in (0x00, 0xFF)]
    for run in runs:
        assert len(run) == len(plain) and all(np.array_equal(a, c) for a, c in zip(run, plain))
    assert np.array_equal(plain[-1], bits(sg.follow_surface(field, b, 0.0).grid).reshape(-1))
    plan = _lib.DsdfSgPlan()
    _lib.check(_lib.lib().dsdf_sg_plan(*dims, b, C.byref(plan)))
    rows, total = _lib.ws_regions()
    assert total == plan.ws_bytes and not G.table_problems(rows, total, 0) and [r[0] for r in rows] == [
        "sg_state", "sg_pend", "sg_have", "sg_part", "sg_offs"]


def test_listed_point_entries_write_nothing_outside_their_buffers():
    from deepsdf_amd import _lib
    lib = _lib.lib()
    f = G.Fences()
    n = 1000
    idx = torch.randperm(40 ** 3)[:n].cuda()
    xyz, vals, grid = f.new("xyz", (n, 3)), f.new("vals", n, zero=True), f.new("grid", 40 ** 3, zero=True)
    vs, org = (C.c_float * 3)(0.1, 0.2, 0.3), (C.c_float * 3)(-1, -1, -1)
    _lib.check(lib.dsdf_sg_coords(40, 40, 40, vs, org, G.ptr(idx), n, G.ptr(xyz), G.stream()))
    bad = idx.clone()
    bad[::7] = 40 ** 3                                              # outside the grid: nothing is written
    bad[3::7] = -1
    _lib.check(lib.dsdf_sg_scatter(G.ptr(bad), n, G.ptr(xyz[:, 0].contiguous()), G.ptr(grid), 40 ** 3, G.stream()))
    g = _lib.DsdfMsGrid()
    for a in range(3):
        g.dims[a], g.tiling[a] = 40, 1
    _lib.check(lib.dsdf_sg_caps_at(C.byref(g), G.ptr(idx), n, None, 0, G.ptr(vals), G.stream()))
    f.check("listed points")
    ok = (bad >= 0) & (bad < 40 ** 3)
    assert int((grid != 0).sum()) <= int(ok.sum()) and torch.equal(grid[bad[ok]], xyz[:, 0][ok])


# ---- 5. coordinates ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [40, 64, 255])
def test_coords_equal_grid_coords_bit_for_bit(N):
    from deepsdf_amd.mesh import grid_coords, grid_coords_at
    h = 2.0 / (N - 1)
    idx = torch.cat([torch.arange(0, N ** 3, 7), torch.tensor([N ** 3 - 1])]).cuda()
    want = grid_coords(N, 0, N ** 3, device="cuda")[idx]
    # the inputs tell a fused index * h + origin from the two rounded operations: formed in fp64 from the fp32 operands (the product
    # is exact there) and rounded once
    ijk = np.stack(np.unravel_index(idx.cpu().numpy(), (N, N, N)), 1).astype(np.float64)
    fused = (ijk * np.float64(np.float32(h)) - 1.0).astype(np.float32)
    d, n = mc_numpy.differing(want.cpu().numpy(), fused)
    print(f"N = {N}: a fused multiply-add would change {d} of {n} coordinates")
    assert d >= 0.1 * n
    got = grid_coords_at(N, h, (-1, -1, -1), idx)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert grid_coords_at(N, h, (-1, -1, -1), idx[:0]).shape == (0, 3)


# ---- 4. end to end with stock modules ---------------------------------------------------------------------------------------------
class Sphere(torch.nn.Module):                     # as tests/test_gpu_mesh.py: called on the chunk's [latent | xyz]
    def forward(self, x):
        return (x[:, 1:].norm(dim=1, keepdim=True) - 0.5) + 0 * x[:, :1]


class Analytic(torch.nn.Module):
    """torus, rods, or sphere + bubble of tests/sparsegrid_numpy.py in fp32 torch."""

    def __init__(self, kind):
        super().__init__()
        self.kind = kind

    def forward(self, r):
        x, y, z = r[:, 1], r[:, 2], r[:, 3]
        if self.kind == "torus":
            v = torch.sqrt((torch.sqrt(x * x + y * y) - 0.6) ** 2 + z * z) - 0.11
        elif self.kind == "rods":
            u, w = sg.ROD_AT
            v = torch.minimum(torch.minimum(torch.sqrt((y - u) ** 2 + (z - w) ** 2), torch.sqrt((x - w) ** 2 + (z - u) ** 2)),
                              torch.sqrt((x - u) ** 2 + (y - w) ** 2)) - 0.07
        else:
            c = 0.8125
            v = torch.minimum(torch.sqrt(x * x + y * y + z * z) - 0.5, torch.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - 0.04)
        return v[:, None]


def test_create_mesh_writes_the_dense_ply_bytes(tmp_path):
    from deep_sdf.mesh import create_mesh, sparse_grid
    kw = dict(N=40, max_batch=5000, offset=np.array([0.5, 0, -1.0]), scale=2.0)
    create_mesh(Sphere(), torch.zeros(1), str(tmp_path / "dense.ply"), **kw)
    with sparse_grid(4):
        create_mesh(Sphere(), torch.zeros(1), str(tmp_path / "sparse.ply"), **kw)
    with sparse_grid(4, lipschitz=0):
        create_mesh(Sphere(), torch.zeros(1), str(tmp_path / "signs.ply"), **kw)
    dense = open(tmp_path / "dense.ply", "rb").read()
    assert len(mc_numpy.read_ply(str(tmp_path / "dense.ply"))[2]) > 1000
    assert open(tmp_path / "sparse.ply", "rb").read() == dense and open(tmp_path / "signs.ply", "rb").read() == dense


@pytest.mark.parametrize("kind,lip,N", [("torus", 1, 50), ("torus", 0, 50), ("rods", 1, 33), ("sphere_bubble", 1, 33)])
def test_stock_module_meshes_equal_dense(kind, lip, N):
    from deepsdf_amd.mesh import marching_cubes, sdf_grid
    h = 2.0 / (N - 1)
    dense = sdf_grid(Analytic(kind), torch.zeros(1), N, 5000)
    stats = {}
    sparse = sdf_grid(Analytic(kind), torch.zeros(1), N, 5000, block=4, lipschitz=lip, stats=stats)
    print(kind, lip, stats)
    assert 0 < stats["points"] < 0.75 * stats["total"]
    vd, fd = marching_cubes(dense, 0.0, (h, h, h), (-1, -1, -1))
    vs, fs = marching_cubes(sparse, 0.0, (h, h, h), (-1, -1, -1))
    assert len(fd) > 500 and torch.equal(fd, fs) and torch.equal(vd.view(torch.int32), vs.view(torch.int32))
    have = sparse != dense
    assert bool(have.any())                                          # filled points: the grid is not the SDF everywhere


def test_sign_only_mode_loses_what_the_oracle_loses(tmp_path):
    from deep_sdf.mesh import create_mesh, sparse_grid
    from deepsdf_amd.mesh import marching_cubes, sdf_grid
    N = 33
    dense = sdf_grid(Analytic("rods"), torch.zeros(1), N, 5000)
    stats = {}
    sparse = sdf_grid(Analytic("rods"), torch.zeros(1), N, 5000, block=4, lipschitz=0, stats=stats)
    r = sg.follow_surface(dense.cpu().numpy(), 4, 0.0)
    assert stats == r.stats and stats["seeds"] == 0 and stats["rounds"] == 0
    assert np.array_equal(bits(sparse), bits(r.grid)) and marching_cubes(sparse)[1].shape[0] == 0 and marching_cubes(dense)[1].shape[0] > 0
    with sparse_grid(4, lipschitz=0), pytest.raises(ValueError, match="Surface level must be within volume data range"):
        create_mesh(Analytic("rods"), torch.zeros(1), str(tmp_path / "rods.ply"), N=N, max_batch=5000)
    with pytest.raises(ValueError, match="Surface level must be within volume data range"):      # the dense grid without a crossing
        create_mesh(Analytic("rods"), torch.zeros(1) + 0, str(tmp_path / "none.ply"), N=5, max_batch=5000)
    # the bubble: eight cells at lipschitz 0, as the oracle on the dense grid's values
    dense = sdf_grid(Analytic("sphere_bubble"), torch.zeros(1), N, 5000)
    sparse = sdf_grid(Analytic("sphere_bubble"), torch.zeros(1), N, 5000, block=4, lipschitz=0)
    r = sg.follow_surface(dense.cpu().numpy(), 4, 0.0)
    assert np.array_equal(bits(sparse), bits(r.grid))
    assert (mc_numpy.NTRI[_cases(dense.cpu().numpy())] > 0).sum() - (mc_numpy.NTRI[_cases(r.grid)] > 0).sum() == 8


# ---- 10. determinism and chunking -------------------------------------------------------------------------------------------------
def test_two_runs_and_two_chunk_sizes_give_identical_bytes():
    from deepsdf_amd.mesh import sdf_grid
    runs = [sdf_grid(Sphere(), torch.zeros(1), 40, mb, block=4) for mb in (37, 37, 10 ** 6)]
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    assert torch.equal(runs[0].view(torch.int32), runs[2].view(torch.int32))
    field = sg.gyroid((33, 33, 33))
    a, b = _follow(field, 4, 0.0), _follow(field, 4, 0.0)
    assert all(n1 == n2 and torch.equal(t1, t2) for (n1, t1), (n2, t2) in zip(a[3], b[3])) and len(a[3]) == len(b[3])


# ---- 6. a HIP decoder ---------------------------------------------------------------------------------------------------------------
def test_hip_decoder_padded_chunks_and_mesh(tmp_path):
    from deep_sdf.mesh import create_mesh, sparse_grid
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.mesh import follow_surface, grid_coords_at, sdf_grid, sparse_threshold
    g = Golden("g6_real_weights")
    dec = Decoder(g.meta["L"], **g.meta["net_specs"]).cuda().eval()
    dec.load_state_dict({k: v for k, v in g.group("params").items()})
    z = torch.zeros(g.meta["L"]).cuda()
    N, b, mb = 64, 4, 32 ** 3                                # mb < N^3: the dense path's full chunks have mb rows
    h = 2.0 / (N - 1)
    eng = dec.engine()
    eng.materialize()
    assert eng.decode_latent_supported()
    lists = []

    def values_at(idx):                                  # the same Engine.decode_latent call on the same padded chunks
        lists.append(idx)
        out = []
        for s in range(0, idx.numel(), mb):
            chunk = idx[s:s + mb]
            k = chunk.numel()
            if k < mb:
                chunk = torch.cat([chunk, chunk[-1:].expand(mb - k)])
            out.append(eng.decode_latent(z.reshape(1, -1), grid_coords_at(N, h, (-1, -1, -1), chunk)).reshape(-1)[:k].clone())
        return torch.cat(out)

    tr = _Trace()
    ref, _, rstats = follow_surface(N, b, sparse_threshold(b, h, 1.0), 0.0, values_at, on_step=tr)
    dbg = tr.items
    stats = {}
    grid = sdf_grid(dec, z, N, mb, block=b, stats=stats)
    assert stats == rstats and torch.equal(grid.view(torch.int32), ref.view(torch.int32))
    print("g6, N = 64, b = 4:", stats)
    assert any(i.numel() % mb for i in lists[1:]) and stats["rounds"] >= 1          # a padded tail was decoded
    dense = sdf_grid(dec, z, N, mb)
    have = dict(dbg)["have"].bool().reshape(N, N, N)
    assert int(have.sum()) == stats["points"] < N ** 3
    e = rel_err(grid[have].cpu(), dense[have].cpu().double())
    print(f"decoded points against the dense grid: rel_err {e:.3e} (bound {FWD_TOL:.0e})")
    assert e <= FWD_TOL
    # the mesh of the filled grid, and every crossing cell inside an active block
    path = str(tmp_path / "g6")
    with sparse_grid(b):
        create_mesh(dec, z, path, N=N, max_batch=mb)
    _, v, f = mc_numpy.read_ply(path)
    filled = grid.cpu().numpy()
    vr, fr = mc_numpy.marching_cubes(filled, 0.0, (h, h, h), (-1, -1, -1))
    assert len(f) > 100 and np.array_equal(f, fr) and mc_numpy.differing(v, vr)[0] == 0
    state = [t for n, t in dbg if n == "states"][-1].cpu().numpy()
    r = sg.Result()
    r.coords = [sg.coarse_coords(N, b)] * 3
    r.active = (state == sg.VALUED).reshape([len(c) - 1 for c in r.coords])
    crossing = mc_numpy.NTRI[_cases(filled)] > 0
    assert crossing.sum() > 100 and not (crossing & ~sg.cell_active(r, (N, N, N))).any()


# ---- 7. microstructures -----------------------------------------------------------------------------------------------------------
class SphereCells(torch.nn.Module):
    """|xyz| - z[0]: a sphere per unit cell whose radius is the (one) latent column (as tests/test_gpu_microstructure.py)."""

    def forward(self, x):
        return x[:, 1:].norm(dim=1, keepdim=True) - x[:, :1]


CAPS_SIX = {"x0": {"cap": 1, "measure": 0.1}, "x1": {"cap": -1, "measure": 0.25}, "y0": {"cap": -1, "measure": 0},
            "y1": {"cap": 1, "measure": 0.25}, "z0": {"cap": 1, "measure": 0}, "z1": {"cap": -1, "measure": 0.1}}


def _cells_field():
    from deepsdf_amd.spline import BSplineField
    cp = np.array([[0.35 if i % 2 == 0 else 0.6] for i in range(8)], dtype=np.float32)
    return BSplineField([1, 1, 1], [[-1, -1, 1, 1]] * 3, cp)


def test_microstructure_grid_and_derivative_equal_dense_bit_for_bit():
    from deepsdf_amd.mesh import marching_cubes, microstructure_mesh_diff, microstructure_sdf_grid
    tiling, N, kw = [2, 1, 1], [12, 8, 6], dict(max_batch=100, cap_border_dict=CAPS_SIX)
    dense = microstructure_sdf_grid(tiling, SphereCells(), _cells_field(), N, **kw)
    stats = {}
    sparse = microstructure_sdf_grid(tiling, SphereCells(), _cells_field(), N, block=4, stats=stats, **kw)
    print("SphereCells:", stats)
    assert stats["rounds"] >= 1 and stats["points"] > 100
    (vd, fd), (vs, fs) = marching_cubes(dense), marching_cubes(sparse)
    assert len(fd) > 50 and torch.equal(fd, fs) and torch.equal(vd.view(torch.int32), vs.view(torch.int32))
    a = microstructure_mesh_diff(tiling, SphereCells(), _cells_field(), N, **kw)
    s = microstructure_mesh_diff(tiling, SphereCells(), _cells_field(), N, block=4, **kw)
    for name in ("verts", "faces", "edge_point", "edge_axis", "band", "mask"):
        x, y = getattr(a, name), getattr(s, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), name
    (ja, aa), (js, as_) = a.jacobian(), s.jacobian()
    assert ja.numel() > 0 and ja.cpu().numpy().tobytes() == js.cpu().numpy().tobytes() and torch.equal(aa, as_)


def test_caps_at_equal_apply_caps_bit_for_bit():
    from deepsdf_amd.mesh import ms_apply_caps, ms_caps_at
    N = [30, 21, 17]
    dims = [n + 2 for n in N]
    n = int(np.prod(dims))
    sdf = torch.from_numpy(np.random.default_rng(2).uniform(-0.3, 0.3, size=n).astype(np.float32)).cuda()
    rev = dict(reversed(list(CAPS_SIX.items())))
    two = {"z1": {"cap": 1, "measure": 0.25}, "x0": {"cap": -1, "measure": 0.1}}
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:5000].cuda()
    seen = []
    for d in (CAPS_SIX, rev, two, None):
        want = ms_apply_caps(sdf.clone(), N, 0, n, d)[idx]
        got = ms_caps_at(sdf[idx].contiguous(), N, idx, d)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), d
        seen.append(got)
    assert not torch.equal(seen[0], seen[1])                      # the order matters here too


def test_microstructure_derivative_with_a_hip_decoder():
    """The sparse Jacobian against the dense one at JAC_TOL of the vertex's largest entry, the tolerance tests/test_gpu_msdiff.py
    holds the dense one to."""
    from deepsdf_amd.mesh import microstructure_mesh_diff
    from deepsdf_amd.spline import BSplineField
    from tests import msdiff_numpy
    from tests.test_gpu_msdiff import JAC_SEEDS, JAC_TOL, NETS, _decoder
    name, degrees, tiling, N = "w32_4x32", (2, 1, 3), [2, 1, 1], [6, 5, 4]
    L, kw = NETS[name]
    knots = [msdiff_numpy.KNOTS[p] for p in degrees]
    S = msdiff_numpy.Fp64Structure(L, kw, JAC_SEEDS[name], degrees, knots, tiling, N, CAPS_SIX, 0.5 / math.sqrt(L))
    dec = _decoder(L, kw, S.params)
    field = BSplineField(degrees, knots, S.cp)
    a = microstructure_mesh_diff(tiling, dec, field, N, max_batch=37, cap_border_dict=CAPS_SIX)
    s = microstructure_mesh_diff(tiling, dec, field, N, max_batch=37, cap_border_dict=CAPS_SIX, block=4)
    assert torch.equal(a.faces, s.faces) and torch.equal(a.edge_point, s.edge_point) and torch.equal(a.mask, s.mask)
    ja, js = a.jacobian()[0].cpu().double(), s.jacobian()[0].cpu().double()
    V = ja.shape[0]
    top = ja.abs().reshape(V, -1).max(1).values
    err = (ja - js).abs().reshape(V, -1).max(1).values
    worst = float((err[top > 0] / top[top > 0]).max())
    print(f"sparse against dense Jacobian: {V} vertices, worst {worst:.3e} of the vertex's largest entry (bound {JAC_TOL:.0e})")
    assert V >= 6 and worst <= JAC_TOL and not err[top == 0].any()


# ---- 8. DeepSDFMesh ---------------------------------------------------------------------------------------------------------------
def _tiny_experiment(root, n_codes=9):
    """An experiment directory (reference layout) with a seeded 4x32 decoder whose zero level set crosses [-1, 1]^3 (as
    tests/test_gpu_microstructure.py builds it)."""
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


def test_deepsdfmesh_with_sparse_block(tmp_path):
    """The sparse volume gradient against the dense one at the existing test's tolerance (tests/test_gpu_surface.py): per entry,
    JAC_TOL x sum over vertices of |the volume's vertex gradient along the vertex's axis, stretched| x the vertex's largest
    Jacobian entry, plus the roundings of the sum over V vertices in vjp_plan()[1] parts."""
    from analysis.geometry import DeepSDFMesh
    from deepsdf_amd.mesh import default_cap_border_dict
    from tests.test_gpu_msdiff import JAC_TOL
    exp = _tiny_experiment(str(tmp_path))
    options = dict(experiment_directory=exp, checkpoint="latest", degrees=[1, 1, 1], refinement=1, cap_border_dict=default_cap_border_dict(),
                   N_base_reconstruction=6, tiling=[2, 1, 1], remove_orphans=False)
    out = []
    for extra in ({}, {"sparse_block": 4}, {"sparse_block": 4, "sparse_lipschitz": 2.0}):
        dm = DeepSDFMesh(dict(options, **extra))
        dm.generate_surface_mesh(np.tile(dm.latent[0], (27, 1)))
        sm = dm.surface_mesh
        v, f = sm.vertices.cpu().numpy(), sm.faces.cpu().numpy()
        out.append((sm.is_watertight, sm.n_components, dm.volume(), mt.volume(v, f), dm.volume_gradient().cpu().double().numpy(),
                    sm.n_faces))
        if not extra:                                                # the bound's ingredients, from the dense run
            d = dm.jacobian
            jac, axis = d.jacobian()
            J, ea = jac.cpu().double().numpy(), axis.cpu().numpy()
            V = J.shape[0]
            ga = mt.vertex_geometry(v, f)[3][np.arange(V), ea] * np.array([2.0, 1.0, 1.0])[ea]
            terms = ga[:, None, None] * J
            top = np.abs(J).reshape(V, -1).max(1)
            bound = JAC_TOL * (np.abs(ga) * top).sum() + (2 * V + d.vjp_plan()[1] + 4) * 2.0 ** -24 * np.abs(terms).sum(0)
    dense = out[0]
    assert dense[5] > 0 and V == sm.n_verts
    for got in out[1:]:
        assert got[0] == dense[0] and got[1] == dense[1] and got[5] == dense[5]
        assert abs(got[2] - dense[2]) <= 1e-12 * dense[3][1]
        assert abs(got[2] - got[3][0]) <= 1e-12 * got[3][1]
        err = np.abs(got[4] - dense[4])
        print(f"volume gradient, sparse against dense: worst error {err.max():.3e}, worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
