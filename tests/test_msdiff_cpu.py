"""CPU (no GPU needed): the derivative of a microstructure mesh with respect to the spline's control points.

1. The closed-form assembly of tests/msdiff_numpy.py (the formula the HIP kernels of csrc/msdiff.hpp implement) against
   torch.autograd.functional.jacobian through an fp64 restatement of the whole forward: control points -> basis -> decoder -> caps ->
   marching cubes' interpolation -> vertex coordinate.
2. The new entry points refuse bad arguments with DSDF_E_INVALID before anything could be launched."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests import msdiff_numpy


SEED = 3
NET_4X32 = dict(dims=[32] * 4, geom_dimension=3, latent_in=[2], norm_layers=[0, 1, 2, 3], weight_norm=True)
CAPS_TWO = {"x1": {"cap": 1, "measure": 0.3}, "z0": {"cap": -1, "measure": 0.25}}       # a min and a max


def test_fp64_assembly_equals_end_to_end_autograd():
    degrees = (2, 1, 3)
    S = msdiff_numpy.Fp64Structure(3, NET_4X32, SEED, degrees, [msdiff_numpy.KNOTS[p] for p in degrees], [2, 1, 1], [6, 5, 4], CAPS_TWO, 0.5)
    cp = torch.from_numpy(S.cp).double()
    rows = S.rows(cp).requires_grad_(True)
    raw, sv = S.decode(rows)
    capped, planes = S.cap(raw)
    ep, ea = msdiff_numpy.check_edges_reproduce(capped.detach().numpy().astype(np.float32))
    V = len(ep)
    assert V >= 20 and set(ea.tolist()) == {0, 1, 2}
    band, r0, r1 = msdiff_numpy.band(ep, ea, S.dims)
    # the conditions under which the function is differentiable at this point: asserted, never skipped
    gap, margin = S.conditions(raw, sv, planes, band)
    print(f"seed {SEED}: {V} vertices, band {len(band)}, nearest cap plane value {gap:.3e}, smallest ReLU margin {margin:.3e}")
    assert gap > 1e-6 and margin > 1e-6
    G = torch.autograd.grad(raw.sum(), rows)[0][:, :S.L].numpy()
    m = S.inside & (capped.detach().reshape(-1) == raw.detach().reshape(-1)).numpy()
    assert m[band].any() and (~m[band]).any() and (~S.inside[band]).any()          # kept, capped and border-layer endpoints
    J, axis = msdiff_numpy.jacobian(capped.detach().numpy(), ep, ea, S.vs, G[band], S.B[band], m[band])
    assert J.shape == (V, S.ncp, S.L)

    stride = torch.tensor([S.dims[1] * S.dims[2], S.dims[2], 1])
    p_t, a_t = torch.from_numpy(ep), torch.from_numpy(ea)
    idx_a = torch.from_numpy(np.stack(np.unravel_index(ep, S.dims), 1)[np.arange(V), ea]).double()
    vs_a = torch.tensor(S.vs, dtype=torch.float64)[a_t]

    def vertex_coordinate(cp_t):
        s = S.cap(S.decode(S.rows(cp_t))[0])[0].reshape(-1)
        s0, s1 = s[p_t], s[p_t + stride[a_t]]
        t = (0.0 - s0) / (s1 - s0)
        return ((idx_a + t) * vs_a - vs_a) / 2

    want = torch.autograd.functional.jacobian(vertex_coordinate, cp).numpy()
    assert want.shape == J.shape
    top = np.abs(want).reshape(V, -1).max(1)
    err = np.abs(J - want).reshape(V, -1).max(1)
    assert (top > 0).sum() > V // 2
    assert not err[top == 0].any()                           # a vertex between two masked endpoints does not move at all
    worst = float((err[top > 0] / top[top > 0]).max())
    print(f"assembly vs autograd: worst entry error {worst:.3e} of the vertex's largest entry (bound 1e-10)")
    assert worst <= 1e-10


# ---- argument checks (host code; nothing is launched) ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from deepsdf_amd.build import build_library
    build_library()
    from deepsdf_amd import _lib
    return _lib.lib()


DUMMY = C.c_void_p(4096)                 # never dereferenced: every check below fails on the host


def _spline(L=4, degree=1):
    from deepsdf_amd import _lib
    host = [np.array([-1, -1, 1, 1], dtype=np.float32) for _ in range(3)]
    s = _lib.DsdfMsSpline()
    for a in range(3):
        s.degree[a], s.n_cp[a], s.n_knots[a] = degree, 2, 4
        s.knots_host[a] = host[a].ctypes.data_as(C.POINTER(C.c_float))
    s.knots_dev, s.cp, s.ncp, s.L = 4096, 4096, 8, L
    return s, host


def _grid(n=8):
    from deepsdf_amd import _lib
    g = _lib.DsdfMsGrid()
    for a in range(3):
        g.dims[a], g.tiling[a] = n, 1
    return g


def _msd(n_verts=4, L=4, dims=(8, 8, 8), degree=1, n_band=4):
    from deepsdf_amd import _lib
    m, b = _lib.DsdfMsdMesh(), _lib.DsdfMsdBand()
    m.grid = m.edge_point = m.edge_axis = m.band_of = 4096
    b.G = b.weights = b.base = b.mask = 4096
    m.n_verts, m.level, b.n_band, b.ld_g, b.L = n_verts, 0.0, n_band, max(L, 1), L
    for a in range(3):
        m.dims[a], m.scale[a], b.degree[a], b.n_cp[a] = dims[a], 0.1, degree, 2
    return m, b


def test_new_entry_points_refuse_bad_arguments(lib):
    from deepsdf_amd.net import NetSpec
    assert lib.dsdf_abi_version() == 19
    bad = lambda rc: rc == -1                                                                       # noqa: E731  DSDF_E_INVALID
    # dsdf_mc_edges
    assert bad(lib.dsdf_mc_edges(1, 8, 8, 4, DUMMY, DUMMY, DUMMY, 1 << 30, None))                   # grid outside 2 .. 1024
    assert bad(lib.dsdf_mc_edges(8, 8, 1025, 4, DUMMY, DUMMY, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_mc_edges(8, 8, 8, -1, DUMMY, DUMMY, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_mc_edges(8, 8, 8, 2 ** 31, DUMMY, DUMMY, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_mc_edges(8, 8, 8, 4, DUMMY, DUMMY, None, 1 << 30, None)) and b"NULL" in lib.dsdf_last_error()
    assert bad(lib.dsdf_mc_edges(8, 8, 8, 4, None, DUMMY, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_mc_edges(8, 8, 8, 4, DUMMY, None, DUMMY, 1 << 30, None))
    assert lib.dsdf_mc_edges(8, 8, 8, 4, DUMMY, DUMMY, DUMMY, 16, None) == -2                       # DSDF_E_WORKSPACE
    assert lib.dsdf_mc_edges(8, 8, 8, 0, None, None, DUMMY, 1 << 30, None) == 0                     # empty surface: nothing to do
    # dsdf_ms_rows_at
    s, _keep = _spline()
    g = _grid()
    assert bad(lib.dsdf_ms_rows_at(None, C.byref(g), DUMMY, 4, DUMMY, DUMMY, DUMMY, None))
    assert bad(lib.dsdf_ms_rows_at(C.byref(s), None, DUMMY, 4, DUMMY, DUMMY, DUMMY, None))
    assert bad(lib.dsdf_ms_rows_at(C.byref(s), C.byref(g), None, 4, DUMMY, DUMMY, DUMMY, None)) and b"NULL" in lib.dsdf_last_error()
    assert bad(lib.dsdf_ms_rows_at(C.byref(s), C.byref(g), DUMMY, 4, None, DUMMY, DUMMY, None))
    assert bad(lib.dsdf_ms_rows_at(C.byref(s), C.byref(g), DUMMY, -1, DUMMY, DUMMY, DUMMY, None))
    assert bad(lib.dsdf_ms_rows_at(C.byref(s), C.byref(g), DUMMY, 2 ** 31, DUMMY, DUMMY, DUMMY, None))
    s0, _keep0 = _spline(L=0)
    assert bad(lib.dsdf_ms_rows_at(C.byref(s0), C.byref(g), DUMMY, 4, DUMMY, DUMMY, DUMMY, None)) and b"latent" in lib.dsdf_last_error()
    assert bad(lib.dsdf_ms_rows_at(C.byref(s), C.byref(_grid(3)), DUMMY, 4, DUMMY, DUMMY, DUMMY, None))
    assert lib.dsdf_ms_rows_at(C.byref(s), C.byref(g), DUMMY, 0, DUMMY, None, None, None) == 0
    # dsdf_module_input_grad
    net = NetSpec(4, [32] * 4, 3, latent_in=[2]).c_struct()
    assert bad(lib.dsdf_module_input_grad(C.byref(net), DUMMY, DUMMY, DUMMY, -1, DUMMY, 7, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_module_input_grad(C.byref(net), DUMMY, DUMMY, None, 8, DUMMY, 7, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_module_input_grad(C.byref(net), DUMMY, DUMMY, DUMMY, 8, None, 7, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_module_input_grad(C.byref(net), None, DUMMY, DUMMY, 8, DUMMY, 7, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_module_input_grad(C.byref(net), DUMMY, DUMMY, DUMMY, 8, DUMMY, 7, None, 1 << 30, None))
    assert bad(lib.dsdf_module_input_grad(None, DUMMY, DUMMY, DUMMY, 8, DUMMY, 7, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_module_input_grad(C.byref(net), DUMMY, DUMMY, DUMMY, 8, DUMMY, 6, DUMMY, 1 << 30, None))      # ld_din < L + G
    assert lib.dsdf_module_input_grad(C.byref(net), DUMMY, DUMMY, DUMMY, 8, DUMMY, 7, DUMMY, 16, None) == -2
    # dsdf_msd_*
    nb, parts = C.c_size_t(), C.c_int32()
    assert lib.dsdf_msd_vjp_workspace_bytes(1025, 8, 4, C.byref(nb), C.byref(parts)) == 0 and parts.value == 3 and nb.value >= 3 * 32 * 4
    assert lib.dsdf_msd_vjp_workspace_bytes(0, 8, 4, C.byref(nb), C.byref(parts)) == 0 and parts.value == 0
    for args in ((-1, 8, 4), (4, 8, 0), (4, 0, 4), (2 ** 31, 8, 4), (4, 2 ** 30, 4)):
        assert bad(lib.dsdf_msd_vjp_workspace_bytes(*args, C.byref(nb), C.byref(parts))), args
    assert bad(lib.dsdf_msd_vjp_workspace_bytes(4, 8, 4, None, None))
    m, b = _msd()
    calls = {"jacobian": lambda m, b, out=DUMMY: lib.dsdf_msd_jacobian(m, b, 0, out, DUMMY, None),
             "jvp": lambda m, b, out=DUMMY: lib.dsdf_msd_jvp(m, b, DUMMY, out, None),
             "vjp": lambda m, b, out=DUMMY: lib.dsdf_msd_vjp(m, b, DUMMY, out, DUMMY, 1 << 30, None)}
    for name, call in calls.items():
        assert bad(call(None, C.byref(b))) and bad(call(C.byref(m), None)), name
        assert bad(call(C.byref(m), C.byref(b), None)) and b"NULL" in lib.dsdf_last_error(), name
        for kw in (dict(n_verts=-1), dict(L=0), dict(dims=(8, 1, 8)), dict(dims=(8, 8, 1025)), dict(degree=0), dict(degree=4),
                   dict(n_band=-1)):
            mm, bb = _msd(**kw)
            assert bad(call(C.byref(mm), C.byref(bb))), (name, kw)
        for field in ("grid", "edge_point", "edge_axis", "band_of"):
            mm, bb = _msd()
            setattr(mm, field, None)
            assert bad(call(C.byref(mm), C.byref(bb))), (name, field)
        for field in ("G", "weights", "base", "mask"):
            mm, bb = _msd()
            setattr(bb, field, None)
            assert bad(call(C.byref(mm), C.byref(bb))), (name, field)
        mm, bb = _msd()
        bb.ld_g = 3                                                                                 # < L
        assert bad(call(C.byref(mm), C.byref(bb))), name
    assert bad(lib.dsdf_msd_jvp(C.byref(m), C.byref(b), None, DUMMY, None))
    assert bad(lib.dsdf_msd_vjp(C.byref(m), C.byref(b), None, DUMMY, DUMMY, 1 << 30, None))
    assert bad(lib.dsdf_msd_vjp(C.byref(m), C.byref(b), DUMMY, DUMMY, None, 1 << 30, None))
    assert lib.dsdf_msd_vjp(C.byref(m), C.byref(b), DUMMY, DUMMY, DUMMY, 16, None) == -2


def test_vjp_workspace_follows_the_planner_conventions(lib):
    """One region, 256-aligned, the debug red zone behind it, recorded for dsdf_debug_ws_regions."""
    from deepsdf_amd import _lib
    from tests.ws_guard import table_problems
    tot = {}
    try:
        for G in (0, 512):
            assert lib.dsdf_debug_ws_redzone(G) == 0
            b, parts = C.c_size_t(), C.c_int32()
            assert lib.dsdf_msd_vjp_workspace_bytes(5000, 27, 16, C.byref(b), C.byref(parts)) == 0
            rows, tot[G] = _lib.ws_regions()
            assert tot[G] == b.value and [r[0] for r in rows] == ["msd_vjp_part"] and rows[0][2] == parts.value * 27 * 16 * 4
            assert not table_problems(rows, tot[G], G)
        assert tot[512] == tot[0] + 512
    finally:
        assert lib.dsdf_debug_ws_redzone(0) == 0


def test_public_names_and_signature():
    import inspect
    from deep_sdf.mesh import create_mesh_microstructure_diff, microstructure_mesh_diff        # noqa: F401
    sig = inspect.signature(create_mesh_microstructure_diff)
    assert list(sig.parameters) == ["tiling", "decoder", "latent_vec_interpolation", "N", "max_batch", "offset", "scale",
                                    "cap_border_dict", "device", "output_tetmesh", "compute_derivatives"]
    assert sig.parameters["N"].default == 256 and sig.parameters["max_batch"].default == 32 ** 3
    with pytest.raises(NotImplementedError):
        create_mesh_microstructure_diff([1, 1, 1], None, None, output_tetmesh=True)


# ---- the kernel-level tests' oracle, inputs and wrong variants (tests/test_gpu_msdiff_kernels.py runs them on the GPU) ----------------
SCALE = np.asarray(msdiff_numpy.SPACING, dtype=np.float32) / 2


@pytest.fixture(scope="module")
def surface_cases():
    """{case: (degrees, n_cp, L, sb, spec, contractions)} on the 6 x 5 x 4 grid, computed once and left unchanged."""
    grid = msdiff_numpy.seeded_grid()
    ep, ea = msdiff_numpy.edges(grid)
    out = {}
    for case, (degrees, n_cp, L) in msdiff_numpy.CASES.items():
        sb = msdiff_numpy.surface_band(grid.shape, ep, ea, degrees, n_cp, L)
        spec = msdiff_numpy.surface_spec(grid, ep, ea, sb, degrees, n_cp, SCALE)
        w, dcp = msdiff_numpy.contraction_inputs(len(ep), int(np.prod(n_cp)), L)
        out[case] = (degrees, n_cp, L, sb, spec, msdiff_numpy.contractions(spec, w, dcp))
    return grid, ep, ea, out


@pytest.mark.parametrize("case", list(msdiff_numpy.CASES))
def test_the_two_fp64_oracles_agree(surface_cases, case):
    """msdiff_numpy.jacobian (the formula pinned against autograd above) and scale * voldiff_numpy.tangent on classes 1 << axis (what
    the kernel-level tests compare the GPU with): a few fp64 operations per entry on both sides."""
    grid, ep, ea, cases = surface_cases
    degrees, n_cp, L, sb, spec, _ = cases[case]
    band, _, _ = msdiff_numpy.band(ep, ea, grid.shape)
    assert np.array_equal(band, sb["band"])
    B, support = msdiff_numpy.scatter_weights(sb["weights"], sb["base"], sb["base"] >= 0, degrees, n_cp)
    assert np.array_equal(B, sb["B"]) and np.array_equal(support, sb["support"])
    J, axis = msdiff_numpy.jacobian(grid, ep, ea, msdiff_numpy.SPACING, sb["G"], sb["B"], sb["mask"])
    assert np.array_equal(axis, spec["axis"]) and J.shape == spec["J"].shape == (len(ep), int(np.prod(n_cp)), L)
    worst = float(np.abs(J - spec["J"]).max() / np.abs(J).max())
    print(f"{case}: jacobian against scale * tangent, worst difference {worst:.2e} of max |J| (bound 1e-14)")
    assert worst <= 1e-14
    assert not spec["J"][spec["Jabs"] == 0].any() and (np.abs(spec["J"]) <= spec["Jabs"]).all()


@pytest.mark.parametrize("case", list(msdiff_numpy.CASES))
def test_the_kernel_level_inputs_carry_the_edges(surface_cases, case):
    from tests import ws_guard
    grid, ep, ea, cases = surface_cases
    degrees, n_cp, L, sb, spec, _ = cases[case]
    V = len(ep)
    assert grid.shape == (6, 5, 4) and V == 143 and np.bincount(ea).tolist() == [51, 44, 48]
    _, r0, r1 = msdiff_numpy.band(ep, ea, grid.shape)
    one_masked = (sb["mask"][r0] == 0) != (sb["mask"][r1] == 0)
    outside = (sb["base"][r0] < 0) | (sb["base"][r1] < 0)
    none = ~spec["end"].any(1)
    print(f"{case}: {int(one_masked.sum())} vertices with one masked endpoint, {int(outside.sum())} with an endpoint outside the domain, "
          f"{int(none.sum())} with no valid endpoint")
    assert one_masked.sum() >= 18 and outside.sum() >= 13 and none.sum() >= 3
    assert not spec["Jabs"][none].any() and spec["vert"].all()
    assert sb["weights"][sb["base"] < 0].any(1).all()                       # rows outside the domain carry weights nobody may read
    K = ws_guard.constants()
    assert (K["MSD_DENSE_STORES"], K["MSD_DENSE_VERTS"], K["MSD_VJP_VERTS"], K["MSD_VJP_TILE"]) == (2048, 64, 512, 8192)
    assert V % 34 == 7 and V % 64 == 15 and V % 21 == 17                    # the dense kernel's last workgroup is short (vpw 34, 64, 21)
    if case == "deg313_L128":
        assert int(np.prod(n_cp)) * L == 10240 > K["MSD_VJP_TILE"]
    big = msdiff_numpy.edges(msdiff_numpy.seeded_grid((9, 9, 9)))[0]
    assert len(big) == 966 > K["MSD_VJP_VERTS"]


def _misses(grid, ep, ea, sb, degrees, n_cp, L, variant):
    """How far a wrong variant lies from the specification, in units of the GPU bound at the entry, for dense / jvp / vjp; computed
    from the oracle alone."""
    spec = msdiff_numpy.surface_spec(grid, ep, ea, sb, degrees, n_cp, SCALE)
    wrong = msdiff_numpy.surface_spec(grid, ep, ea, sb, degrees, n_cp, SCALE, variant=variant)
    w, dcp = msdiff_numpy.contraction_inputs(len(ep), int(np.prod(n_cp)), L)
    c, cw = msdiff_numpy.contractions(spec, w, dcp), msdiff_numpy.contractions(wrong, w, dcp)
    parts = -(-len(ep) // 512)
    pairs = {"dense": (wrong["J"], spec["J"], msdiff_numpy.dense_bound(spec["Jabs"])),
             "jvp": (cw["jvp"][0], c["jvp"][0], msdiff_numpy.jvp_bound(degrees, L, c["jvp"][1])),
             "vjp": (cw["vjp"][0], c["vjp"][0], msdiff_numpy.vjp_bound(c["n_terms"], parts, c["vjp"][1]))}
    out = {}
    for what, (a, b, bound) in pairs.items():
        d = np.abs(a - b)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[what] = float(np.max(np.where(d > 0, d / bound, 0.0)))       # a miss where the bound is zero: inf
    return out


@pytest.mark.parametrize("case", list(msdiff_numpy.CASES))
def test_every_wrong_variant_misses_the_specification(surface_cases, case):
    grid, ep, ea, cases = surface_cases
    degrees, n_cp, L, sb, _, _ = cases[case]
    bad = msdiff_numpy.invalid_entries(grid, ep, ea, sb, degrees, n_cp)
    for variant in msdiff_numpy.VARIANTS:
        healthy = _misses(grid, ep, ea, sb, degrees, n_cp, L, variant)
        invalid = _misses(grid, bad[0], bad[1], bad[2], degrees, n_cp, L, variant)
        print(f"{case} {variant}: worst miss / bound on the healthy input {healthy}, with entries out of range {invalid}")
        if variant == "wrapped_edge_counts":
            assert set(healthy.values()) == {0.0}                           # marching cubes emits no such edge: the same on valid meshes
        else:
            assert min(healthy.values()) > 1e3, (variant, healthy)
        assert min(invalid.values()) > 1e3, (variant, invalid)


@pytest.mark.parametrize("case", list(msdiff_numpy.CASES))
def test_entries_out_of_range_in_the_oracle(surface_cases, case):
    """The input of the GPU test of entries out of range: what is written over, and what the entry rule makes of it."""
    grid, ep, ea, cases = surface_cases
    degrees, n_cp, L, sb, spec, _ = cases[case]
    bp, ba, bsb, touched, zero = msdiff_numpy.invalid_entries(grid, ep, ea, sb, degrees, n_cp)
    npts, nb, ncp = grid.size, len(sb["band"]), int(np.prod(n_cp))
    assert zero.sum() == 7 and set(ba[zero].tolist()) == {-1, 0, 1, 2, 3} and {-1, npts + 5} <= set(bp[zero].tolist())
    idx = np.stack(np.unravel_index(np.clip(bp, 0, npts - 1), grid.shape), 1)
    for a in range(3):
        assert ((ba == a) & zero & (idx[:, a] == grid.shape[a] - 1) & (bp >= 0) & (bp < npts)).sum() >= 1
    assert {-1, nb, nb + 7} <= set(bsb["band_of"].tolist()) and {-2, ncp, n_cp[0] - degrees[0]} <= set(bsb["base"].tolist())
    assert 7 < touched.sum() < len(ep) // 2 and (~touched).sum() > 100
    got = msdiff_numpy.surface_spec(grid, bp, ba, bsb, degrees, n_cp, SCALE)
    assert not got["J"][zero].any() and not got["vert"][zero].any() and got["vert"][~zero].all()
    assert np.array_equal(got["J"][~touched], spec["J"][~touched]) and np.abs(got["J"][touched & ~zero]).max() > 0
    assert (got["end"][touched & ~zero].sum(1) < spec["end"][touched & ~zero].sum(1)).all()        # each lost an endpoint
    assert np.array_equal(got["axis"][zero], np.where((ba[zero] >= 0) & (ba[zero] <= 2), ba[zero], 0))
