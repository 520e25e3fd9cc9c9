"""CPU (no GPU needed): the numpy references of microstructure meshing (tests/ms_numpy.py) against a torch restatement of the
reference's grid arithmetic and against B-spline identities, knot refinement of BSplineField, and argument checking of
BSplineField, create_mesh_microstructure and the dsdf_ms_* entry points (every call here fails before any launch)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ms_numpy

CASES = [([16, 16, 16], [2, 2, 2]), ([30, 21, 17], [3, 1, 4]), ([64, 48, 33], [5, 2, 7]), ([100, 100, 10], [6, 3, 1])]


@pytest.fixture(scope="module")
def lib():
    from deepsdf_amd.build import build_library
    build_library()
    from deepsdf_amd import _lib
    return _lib.lib()


# ---- grid coordinates -----------------------------------------------------------------------------------------------------
def torch_grid(N, tiling):
    """deep_sdf/mesh.py create_mesh_microstructure :226-259 restated with torch on the CPU: (samples_orig [n, 3], folded [n, 3],
    inside [n]) of the padded grid."""
    tiling = np.array(tiling)
    N = np.array(N) + 2
    n_tot = int(N[0] * N[1] * N[2])
    index = torch.arange(0, n_tot, 1, out=torch.LongTensor())
    orig = torch.zeros(n_tot, 3)
    orig[:, 2] = index % N[2]
    orig[:, 1] = (index // N[2]) % N[1]
    orig[:, 0] = ((index // N[2]) // N[1]) % N[0]
    size = [2.0 / (N[a] - 1 - 2) for a in range(3)]
    origin = [-1 - size[a] for a in range(3)]
    for a in range(3):
        orig[:, a] = (orig[:, a] * size[a]) + origin[a]

    def transform(x, t):
        p = 2 / t
        return (2 / p) * torch.abs((x - t % 2) % (p * 2) - p) - 1

    folded = torch.zeros(n_tot, 3)
    for a in range(3):
        folded[:, a] = transform(orig[:, a], tiling[a])
    inside = torch.ones(n_tot, dtype=torch.bool)
    for a in range(3):
        inside &= (orig[:, a] >= -1) & (orig[:, a] <= 1)
    return orig.numpy(), folded.numpy(), inside.numpy()


def test_grid_axes_equal_the_torch_arithmetic_bit_for_bit():
    above, at_or_below = 0, 0
    for N, tiling in CASES:
        axes = ms_numpy.grid_axes(N, tiling)
        orig, folded, inside = torch_grid(N, tiling)
        assert np.array_equal(ms_numpy.grid_points(axes, 0).view(np.uint32), orig.view(np.uint32)), (N, tiling)
        assert np.array_equal(ms_numpy.grid_points(axes, 1).view(np.uint32), folded.view(np.uint32)), (N, tiling)
        assert np.array_equal(ms_numpy.grid_inside(axes), inside), (N, tiling)
        for xo, _, ins in axes:
            assert xo.dtype == np.float32 and ins[1] == (xo[1] >= -1)
            last = xo[-2]                                  # the last interior grid point: 1 up to one rounding
            assert abs(float(last) - 1.0) < 2e-7
            above += int(last > 1)
            at_or_below += int(last <= 1)
            assert bool(ins[-2]) == bool(last <= 1)
    # both kinds occur: a border layer with a zero latent, and one with the spline's end value
    assert above > 0 and at_or_below > 0, (above, at_or_below)


def test_fold_maps_every_cell_onto_the_unit_cell():
    for t in (1, 2, 3, 4, 7):
        x = np.linspace(-1, 1, 2001).astype(np.float32)
        f = ms_numpy.fold(x, t).astype(np.float64)
        assert f.min() >= -1 - 1e-6 and f.max() <= 1 + 1e-6
        cell = np.minimum(np.floor((x.astype(np.float64) + 1) / (2 / t)), t - 1)
        local = (x.astype(np.float64) + 1 - cell * (2 / t)) * t - 1          # in [-1, 1] within the cell
        assert np.abs(np.abs(f) - np.abs(local)).max() < 1e-5, t              # mirrored copies: equal up to the sign


def test_caps_reference_equals_numpy_maximum_and_minimum():
    """ms_numpy.caps selects by comparison so that the sign of a zero is specified; as values it is np.maximum / np.minimum, the
    reference's operations.  The order of the entries matters."""
    N = [30, 21, 17]
    xo = [a[0] for a in ms_numpy.grid_axes(N, [1, 1, 1])]
    sdf = np.random.default_rng(2).uniform(-0.3, 0.3, size=[len(x) for x in xo]).astype(np.float32)
    d = {"x0": {"cap": 1, "measure": 0.1}, "x1": {"cap": -1, "measure": 0.25}, "y0": {"cap": -1, "measure": 0},
         "y1": {"cap": 1, "measure": 0.25}, "z0": {"cap": 1, "measure": 0}, "z1": {"cap": -1, "measure": 0.1}}
    rev = dict(reversed(list(d.items())))
    for caps in (d, rev, {"z1": {"cap": 1, "measure": 0.25}}):
        a, b = ms_numpy.caps(sdf, xo, caps), ms_numpy.caps(sdf, xo, caps, np.maximum, np.minimum)
        assert a.dtype == np.float32 and np.array_equal(a, b)
    assert not np.array_equal(ms_numpy.caps(sdf, xo, d), ms_numpy.caps(sdf, xo, rev))
    inner = ms_numpy.caps(sdf, xo, {})
    assert np.all(inner >= sdf) and inner[0].min() > 0 and inner[:, :, -1].min() > 0        # the layer outside the cube is outside
    assert np.array_equal(inner[10:20, 8:14, 7:11], sdf[10:20, 8:14, 7:11])                   # deep inside nothing changes
    with pytest.raises(ValueError):
        ms_numpy.caps(sdf, xo, {"x0": {"cap": 2, "measure": 0}})


# ---- B-splines ------------------------------------------------------------------------------------------------------------
def clamped(p, inner):
    return [-1.0] * (p + 1) + list(inner) + [1.0] * (p + 1)


KNOTS = {1: clamped(1, [-0.4, 0.1, 0.1, 0.5]), 2: clamped(2, [-0.5, 0.2, 0.2]), 3: clamped(3, [-0.3, 0.25, 0.25, 0.6])}


def random_spline(degrees, L, seed):
    rng = np.random.default_rng(seed)
    knots = [KNOTS[p] for p in degrees]
    n = [len(U) - p - 1 for p, U in zip(degrees, knots)]
    return knots, rng.uniform(-1, 1, size=(n[0] * n[1] * n[2], L))


@pytest.mark.parametrize("degrees", [(1, 1, 1), (2, 1, 3), (3, 3, 3)])
def test_bspline_eval_identities(degrees):
    rng = np.random.default_rng(3)
    pts = rng.uniform(-1, 1, size=(500, 3))
    pts[:8] = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)])
    pts[8:12] = [[0.1, 0.2, 0.25], [0.1, -0.5, 0.6], [-0.4, 0.2, -0.3], [0.5, 1.0, 0.25]]     # on knots
    knots, cp = random_spline(degrees, 3, 5)
    n = [len(U) - p - 1 for p, U in zip(degrees, knots)]
    for a in range(3):
        B = ms_numpy.basis_matrix(degrees[a], knots[a], pts[:, a])
        assert B.shape == (500, n[a]) and B.min() >= 0
        assert np.abs(B.sum(1) - 1).max() < 1e-13                                  # partition of unity
    # linear functions are reproduced when the control points sit at the Greville abscissae
    grev = [np.array([np.mean(U[i + 1:i + p + 1]) for i in range(len(U) - p - 1)]) for p, U in zip(degrees, knots)]
    G = np.stack([g.reshape(-1) for g in np.meshgrid(grev[2], grev[1], grev[0], indexing="ij")][::-1], 1)   # x fastest
    lin = G @ np.array([[0.3, -1.0], [0.7, 0.5], [-0.2, 2.0]]) + np.array([0.1, -0.4])
    want = pts @ np.array([[0.3, -1.0], [0.7, 0.5], [-0.2, 2.0]]) + np.array([0.1, -0.4])
    assert np.abs(ms_numpy.bspline_eval(degrees, knots, lin, pts) - want).max() < 1e-13
    # both ends of the domain take the corner control points
    v = ms_numpy.bspline_eval(degrees, knots, cp, pts[:8])
    C3 = cp.reshape(n[2], n[1], n[0], -1)
    for r, (i, j, k) in enumerate((i, j, k) for i in (0, -1) for j in (0, -1) for k in (0, -1)):
        assert np.abs(v[r] - C3[k, j, i]).max() < 1e-14


def test_basis_matrix_agrees_with_scipy():
    interpolate = pytest.importorskip("scipy.interpolate")
    u = np.linspace(-1, 1, 301)
    for p, U in KNOTS.items():
        n = len(U) - p - 1
        B = ms_numpy.basis_matrix(p, U, u)
        for i in range(n):
            c = np.zeros(n)
            c[i] = 1
            assert np.abs(B[:, i] - interpolate.BSpline(np.array(U), c, p, extrapolate=False)(u)).max() < 1e-13, (p, i)


@pytest.mark.parametrize("degrees", [(1, 1, 1), (2, 1, 3), (3, 3, 3)])
def test_uniform_refine_keeps_the_function(degrees):
    from deepsdf_amd.spline import BSplineField
    knots, cp = random_spline(degrees, 4, 11)
    f = BSplineField(degrees, knots, cp)
    pts = np.random.default_rng(1).uniform(-1, 1, size=(400, 3))
    before = ms_numpy.bspline_eval(degrees, knots, cp, pts)
    res0 = f.control_mesh_resolutions.copy()
    f.uniform_refine(1)
    assert np.all(f.control_mesh_resolutions > res0)
    assert f.control_points.shape == (int(np.prod(f.control_mesh_resolutions)), 4)
    assert np.abs(ms_numpy.bspline_eval(degrees, f.knot_vectors, f.control_points, pts) - before).max() < 1e-12
    f.uniform_refine(2)
    assert np.abs(ms_numpy.bspline_eval(degrees, f.knot_vectors, f.control_points, pts) - before).max() < 1e-12
    for U in f.knot_vectors:
        assert np.all(np.diff(U) >= 0)


# ---- argument checks --------------------------------------------------------------------------------------------------------
def test_bspline_field_refuses_bad_arguments():
    from deepsdf_amd.spline import BSplineField, as_field
    kv = [[-1, -1, 1, 1]] * 3
    cp = np.zeros((8, 2))
    f = BSplineField([1, 1, 1], kv, cp)
    assert list(f.degrees) == [1, 1, 1] and list(f.control_mesh_resolutions) == [2, 2, 2] and f.control_points.shape == (8, 2)
    f.control_points = np.ones((8, 5))                       # assignable, another latent size
    assert f.latent_size == 5
    for bad in (np.zeros((7, 2)), np.zeros((8, 2, 1)), np.zeros((8, 0))):
        with pytest.raises(ValueError):
            f.control_points = bad
    with pytest.raises(ValueError):
        BSplineField([1, 1], kv[:2], cp)
    with pytest.raises(ValueError):
        BSplineField([0, 1, 1], kv, cp)
    with pytest.raises(ValueError):
        BSplineField([4, 1, 1], [[-1] * 5 + [1] * 5, kv[1], kv[2]], cp)
    with pytest.raises(ValueError):
        BSplineField([1, 1, 1], [[-1, -1, 0.5, 0.2, 1, 1], kv[1], kv[2]], np.zeros((16, 2)))      # decreasing
    with pytest.raises(ValueError):
        BSplineField([1, 1, 1], [[-1, -1, 1], kv[1], kv[2]], cp)                                  # too short
    with pytest.raises(ValueError):
        BSplineField([1, 1, 1], [[1, 1, 1, 1], kv[1], kv[2]], cp)                                 # empty range

    class Stand:                                             # what a splinepy BSpline offers
        degrees = np.array([1, 1, 1])
        knot_vectors = [np.array(k, dtype=float) for k in kv]
        control_points = np.arange(16.0).reshape(8, 2)

    g = as_field(Stand())
    assert isinstance(g, BSplineField) and np.array_equal(g.control_points, Stand.control_points)
    assert as_field(f) is f
    with pytest.raises(TypeError):
        as_field(object())


def test_create_mesh_microstructure_checks_its_arguments():
    import deep_sdf.mesh
    from deepsdf_amd import mesh
    from deepsdf_amd.spline import BSplineField
    for name in ("create_mesh_microstructure", "sdf_struct", "CapBorderDict", "CapType", "location_lookup"):
        assert getattr(deep_sdf.mesh, name) is getattr(mesh, name)
    assert mesh.location_lookup == ms_numpy.LOCATION
    f = BSplineField([1, 1, 1], [[-1, -1, 1, 1]] * 3, np.zeros((8, 1)))
    dec = torch.nn.Identity()
    with pytest.raises(ValueError, match="Tiling"):
        mesh.create_mesh_microstructure("a", dec, f, "x")
    with pytest.raises(ValueError, match="Tiling"):
        mesh.create_mesh_microstructure([1, 2], dec, f, "x")
    with pytest.raises(ValueError, match="grid points"):
        mesh.create_mesh_microstructure(2, dec, f, "x", N=[1, 2])
    with pytest.raises(ValueError, match="grid points"):
        mesh.create_mesh_microstructure(2, dec, f, "x", N=2.5)
    with pytest.raises(NotImplementedError, match="kaolin"):
        mesh.create_mesh_microstructure(2, dec, f, "x", N=8, use_flexicubes=True)
    with pytest.raises(ValueError, match="Cap must be -1 or 1"):
        mesh.cap_records({"x0": {"cap": 0, "measure": 0.1}})
    with pytest.raises(ValueError):
        mesh.cap_records({"w0": {"cap": 1, "measure": 0.1}})
    recs, n = mesh.cap_records(None)
    assert n == 6 and [(recs[i].dim, recs[i].m, recs[i].cap, recs[i].c) for i in range(6)] == [
        (0, -1, -1, -1), (0, 1, -1, 1), (1, -1, -1, -1), (1, 1, -1, 1), (2, -1, -1, -1), (2, 1, -1, 1)]
    recs, n = mesh.cap_records({"z1": {"cap": 1, "measure": 0.1}, "x0": {"cap": -1, "measure": 0.25}})
    assert n == 2 and (recs[0].dim, recs[0].m, recs[0].cap) == (2, 1, 1) and recs[0].c == np.float32(0.9)
    assert (recs[1].dim, recs[1].m, recs[1].cap, recs[1].c) == (0, -1, -1, -0.75)


def _spline_struct(deg=(1, 1, 1), n_cp=(2, 2, 2), knots=None, ncp=None, L=4):
    from deepsdf_amd import _lib
    s = _lib.DsdfMsSpline()
    keep = []
    for a in range(3):
        U = np.array(knots[a] if knots else [-1] * (deg[a] + 1) + [1] * (deg[a] + 1), dtype=np.float32)
        keep.append(U)
        s.degree[a], s.n_cp[a], s.n_knots[a] = deg[a], n_cp[a], U.size
        s.knots_host[a] = U.ctypes.data_as(C.POINTER(C.c_float))
    s.knots_dev = s.cp = 1 << 20                           # never dereferenced
    s.ncp = n_cp[0] * n_cp[1] * n_cp[2] if ncp is None else ncp
    s.L = L
    return s, keep


def _grid_struct(dims=(10, 10, 10), tiling=(2, 2, 2)):
    from deepsdf_amd import _lib
    g = _lib.DsdfMsGrid()
    for a in range(3):
        g.dims[a], g.tiling[a] = dims[a], tiling[a]
    return g


def test_ms_arguments_are_refused_before_any_launch(lib):
    from deepsdf_amd import _lib
    assert lib.dsdf_abi_version() == 19
    fake = C.c_void_p(1 << 20)          # never dereferenced: every call below is refused before a launch
    g = _grid_struct()
    s, keep = _spline_struct()
    rows = lambda sp, gr, a=0, b=10, out=fake: lib.dsdf_ms_rows(C.byref(sp) if sp else None, C.byref(gr) if gr else None, a, b,
                                                                None, 1, 1, out, None)
    assert rows(None, g) == -1 and rows(s, None) == -1 and rows(s, g, out=None) == -1
    assert rows(s, g, 5, 5) == -1 and b"empty" in lib.dsdf_last_error()
    assert rows(s, g, 7, 3) == -1
    assert rows(s, g, -1, 3) == -1 and rows(s, g, 0, 1001) == -1 and b"outside" in lib.dsdf_last_error()
    assert rows(s, _grid_struct(dims=(3, 10, 10))) == -1 and rows(s, _grid_struct(dims=(10, 10, 1025))) == -1
    assert rows(s, _grid_struct(tiling=(2, 0, 2))) == -1 and b"tiling" in lib.dsdf_last_error()
    for deg in ((0, 1, 1), (4, 1, 1)):
        bad, k2 = _spline_struct(deg=deg, n_cp=(5, 5, 5))
        assert rows(bad, g) == -1 and b"degree" in lib.dsdf_last_error()
    bad, k2 = _spline_struct(n_cp=(3, 2, 2))                 # 4 knots given, 3 + 1 + 1 = 5 needed
    assert rows(bad, g) == -1 and b"knot vector" in lib.dsdf_last_error()
    bad, k2 = _spline_struct(n_cp=(4, 2, 2), knots=[[-1, -1, 0.5, 0.2, 1, 1], [-1, -1, 1, 1], [-1, -1, 1, 1]])
    assert rows(bad, g) == -1 and b"decreasing" in lib.dsdf_last_error()
    bad, k2 = _spline_struct(knots=[[1, 1, 1, 1], [-1, -1, 1, 1], [-1, -1, 1, 1]])
    assert rows(bad, g) == -1 and b"empty range" in lib.dsdf_last_error()
    bad, k2 = _spline_struct(ncp=9)
    assert rows(bad, g) == -1 and b"control points" in lib.dsdf_last_error()
    bad, k2 = _spline_struct(L=0)
    assert rows(bad, g) == -1
    bad, k2 = _spline_struct()
    bad.cp = None
    assert rows(bad, g) == -1 and b"NULL" in lib.dsdf_last_error()
    bad, k2 = _spline_struct()
    bad.knots_host[1] = C.POINTER(C.c_float)()
    assert rows(bad, g) == -1 and b"NULL" in lib.dsdf_last_error()

    cap = (_lib.DsdfMsCap * 7)()
    for r in range(7):
        cap[r].dim, cap[r].cap, cap[r].m, cap[r].c = r % 3, 1, 1.0, 0.9
    caps = lambda gr, a, b, n, sdf=fake, recs=cap: lib.dsdf_ms_caps(C.byref(gr) if gr else None, a, b, recs, n, sdf, None)
    assert caps(None, 0, 10, 6) == -1 and caps(g, 0, 10, 6, sdf=None) == -1 and caps(g, 0, 10, 2, recs=None) == -1
    assert caps(g, 4, 4, 6) == -1 and caps(g, 0, 1001, 6) == -1 and caps(g, -2, 10, 6) == -1
    assert caps(g, 0, 10, 7) == -1 and caps(g, 0, 10, -1) == -1 and b"records" in lib.dsdf_last_error()
    cap[1].cap = 0
    assert caps(g, 0, 10, 6) == -1 and b"must be -1 or 1" in lib.dsdf_last_error()
    cap[1].cap, cap[2].dim = -1, 3
    assert caps(g, 0, 10, 6) == -1 and b"axis" in lib.dsdf_last_error()
    cap[2].dim, cap[0].m = 2, 0.5
    assert caps(g, 0, 10, 6) == -1 and b"multiplier" in lib.dsdf_last_error()
