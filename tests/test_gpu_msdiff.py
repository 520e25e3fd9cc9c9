"""-m gpu: d(mesh vertices) / d(spline control points) of a microstructure mesh.  The vertex edges of marching cubes, the rows at a
list of grid indices, the input gradient without weight gradients, the assembled Jacobian against the fp64 reference of
tests/msdiff_numpy.py (whose formula tests/test_msdiff_cpu.py pins against autograd), an analytic module, the adjoint and the
tangent against the GPU's own dense Jacobian, and the public interface.

The kernel level -- dsdf_msd_jacobian / dsdf_msd_jvp / dsdf_msd_vjp on a synthetic band against an fp64 specification of their own, entry
by entry at bounds counted from the kernels, every form of the dense kernel, part and tile boundaries of the adjoint, entries out of
range -- is tests/test_gpu_msdiff_kernels.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests import mc_numpy, ms_numpy, msdiff_numpy, ws_guard
from tests.golden_io import rel_err, worst_elem
from tests.test_gpu_microstructure import SPLINE_TOL, SphereCells, _tiny_experiment, bits, linear_field, make_field
from tests.test_gpu_parity import BIG, GRAD_ELEM_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SMALL = dict(dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)), xyz_in_all=False, latent_dropout=False,
              weight_norm=True, geom_dimension=3)
# one net per kernel family of the module path: wave-private, narrow, full size (fused), layer by layer
NETS = {
    "w32_4x32": (2, dict(_SMALL, dims=[32] * 4, latent_in=[2], use_tanh=False)),
    "n128_6x128": (16, dict(_SMALL, dims=[128] * 6, latent_in=[2], use_tanh=False)),
    "fused_8x512": (256, BIG),
    "xyz_in_all": (5, dict(dims=[64, 72, 64], dropout=[0], dropout_prob=0.2, norm_layers=[0, 1], latent_in=[2], weight_norm=True,
                           xyz_in_all=True, geom_dimension=3)),
}
CAPS_SIX = {"x0": {"cap": 1, "measure": 0.1}, "x1": {"cap": -1, "measure": 0.25}, "y0": {"cap": -1, "measure": 0},
            "y1": {"cap": 1, "measure": 0.25}, "z0": {"cap": 1, "measure": 0}, "z1": {"cap": -1, "measure": 0.1}}
JAC_TOL = 1e-4            # the d_input bound of the break-point table
# seeds at which no band point lies within 1e-6 of a cap plane value and every ReLU margin exceeds 1e-6 (asserted in the tests).
# 8x512: 4096 hidden units per row put the smallest of a hundred rows' margins near 1e-7 at every seed, so its level is set at the 4 %
# quantile of the decoder's values -- a small surface, a dozen band rows -- and the seed is chosen among those.
JAC_SEEDS = {"w32_4x32": 2, "n128_6x128": 7, "fused_8x512": 8, "xyz_in_all": 6}
JAC_QUANTILE = {"fused_8x512": 0.04}


def _decoder(L, kw, params, **extra):
    from deepsdf_amd.decoder import Decoder
    dec = Decoder(L, **dict(kw, **extra)).cuda().eval()
    dec.load_state_dict({k: v.float() for k, v in params.items()})
    return dec


# ---- 3. vertex edges ------------------------------------------------------------------------------------------------------------
def _mc_grids():
    for N in (9, (5, 9, 17)):
        n = (N,) * 3 if isinstance(N, int) else N
        x, y, z = np.meshgrid(*[np.linspace(-1, 1, k) for k in n], indexing="ij")
        yield f"sphere{n}", (np.sqrt(x * x + y * y + z * z) - 0.5).astype(np.float32)
        yield f"torus{n}", (np.sqrt((np.sqrt(x * x + y * y) - 0.5) ** 2 + z * z) - 0.2).astype(np.float32)
    yield "sphere9", mc_numpy.sphere(9)[0]
    yield "torus9", mc_numpy.torus(9)[0]


def test_vertex_edges_reproduce_the_vertices_bit_for_bit():
    from deepsdf_amd.mesh import marching_cubes
    spacing, origin = (0.25, 0.5, 0.125), (-1.0, 0.5, 0.25)
    for name, sdf in _mc_grids():
        g = torch.from_numpy(sdf).cuda()
        verts, faces, ep, ea = marching_cubes(g, 0.0, spacing, origin, return_edges=True)
        v2, f2 = marching_cubes(g, 0.0, spacing, origin)                        # the default return value is unchanged
        assert torch.equal(verts, v2) and torch.equal(faces, f2), name
        assert ep.dtype == torch.int64 and ea.dtype == torch.int32 and ep.shape == ea.shape == (verts.shape[0],)
        wp, wa = msdiff_numpy.edges(sdf)
        assert len(wp) > 20 and set(wa.tolist()) == {0, 1, 2}, name
        assert np.array_equal(ep.cpu().numpy(), wp) and np.array_equal(ea.cpu().numpy(), wa), name       # mc_numpy's order
        again = msdiff_numpy.vertices_from_edges(sdf, ep.cpu().numpy(), ea.cpu().numpy(), 0.0, spacing, origin)
        assert np.array_equal(bits(again), bits(verts)), name
    empty = torch.ones(5, 6, 7, device="cuda")
    verts, faces, ep, ea = marching_cubes(empty, 0.0, return_edges=True)
    assert verts.shape == (0, 3) and faces.shape == (0, 3) and ep.shape == (0,) and ea.shape == (0,)


def test_vertex_edges_write_nothing_outside_their_buffers():
    from deepsdf_amd import _lib
    sdf = torch.from_numpy(mc_numpy.torus(9)[0]).cuda()
    lib = _lib.lib()
    b = C.c_size_t()
    _lib.check(lib.dsdf_mc_workspace_bytes(9, 9, 9, C.byref(b)))
    ws = torch.empty(b.value, dtype=torch.uint8, device="cuda")
    totals = torch.empty(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.dsdf_mc_count(ws_guard.ptr(sdf), 9, 9, 9, 0.0, ws_guard.ptr(totals), ws_guard.ptr(ws), ws.numel(), ws_guard.stream()))
    nv = int(totals[0])
    F = ws_guard.Fences()
    ep, ea = F.new("edge_point", nv, torch.int64), F.new("edge_axis", nv, torch.int32)
    before = ws.clone()
    _lib.check(lib.dsdf_mc_edges(9, 9, 9, nv, ws_guard.ptr(ep), ws_guard.ptr(ea), ws_guard.ptr(ws), ws.numel(), ws_guard.stream()))
    F.check("mc_edges")
    assert torch.equal(ws, before)                                              # the count pass's workspace is only read
    wp, wa = msdiff_numpy.edges(sdf.cpu().numpy())
    assert np.array_equal(ep.cpu().numpy(), wp) and np.array_equal(ea.cpu().numpy(), wa)
    # fewer than the counted total: the first ones, nothing behind them
    F2 = ws_guard.Fences()
    ep2, ea2 = F2.new("edge_point", nv - 7, torch.int64), F2.new("edge_axis", nv - 7, torch.int32)
    _lib.check(lib.dsdf_mc_edges(9, 9, 9, nv - 7, ws_guard.ptr(ep2), ws_guard.ptr(ea2), ws_guard.ptr(ws), ws.numel(), ws_guard.stream()))
    F2.check("mc_edges, short")
    assert torch.equal(ep2, ep[:nv - 7]) and torch.equal(ea2, ea[:nv - 7])


# ---- 4. rows at indices -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [2, 16, 67])
@pytest.mark.parametrize("degrees", [(1, 1, 1), (2, 1, 3), (3, 3, 3)])
def test_rows_at_indices_equal_the_grid_rows(degrees, L):
    from deepsdf_amd import _lib
    from deepsdf_amd.mesh import _ms_grid, ms_grid_rows
    N, tiling = [30, 21, 17], [3, 1, 4]
    field, knots, cp = make_field(degrees, L, 11 + L)
    axes = ms_numpy.grid_axes(N, tiling)
    dims = [len(a[0]) for a in axes]
    npts = int(np.prod(dims))
    whole = ms_grid_rows(field, tiling, N, 0, npts)
    inside = ms_numpy.grid_inside(axes)
    xo = ms_numpy.grid_points(axes, 0)
    border = np.nonzero(~inside)[0]
    # the first and last inside layer of every axis: where a coordinate rounded differently would flip the inside test
    ijk = np.stack(np.unravel_index(np.arange(npts), dims), 1)
    edge_layer = np.nonzero(inside & ((ijk == 1) | (ijk == np.array(dims) - 2)).any(1))[0]
    ncp_axis = [len(U) - p - 1 for p, U in zip(degrees, knots)]
    g, _ = _ms_grid(tiling, N)
    s, _keep = field.c_spline(torch.device("cuda"))
    lib = _lib.lib()
    rng = np.random.default_rng(5 + L)
    for n in (1, 63, 65, 130):
        pick = np.concatenate([rng.choice(border, n // 3), rng.choice(edge_layer, n // 3), rng.choice(npts, n - 2 * (n // 3))])
        rng.shuffle(pick)
        idx = torch.from_numpy(pick).cuda()
        F = ws_guard.Fences()
        rows, w, base = F.new("rows", (n, L + 3)), F.new("weights", (n, 64)), F.new("base", n, torch.int32)
        _lib.check(lib.dsdf_ms_rows_at(C.byref(s), C.byref(g), ws_guard.ptr(idx), n, ws_guard.ptr(rows), ws_guard.ptr(w), ws_guard.ptr(base),
                                       ws_guard.stream()))
        F.check(f"rows_at {degrees} L {L} n {n}")
        assert np.array_equal(bits(rows), bits(whole[idx])), (degrees, L, n)
        base, w = base.cpu().numpy(), w.cpu().numpy().astype(np.float64)
        assert np.array_equal(base < 0, ~inside[pick]) and (base[base < 0] == -1).all()
        assert np.array_equal(base < 0, ~bits(whole[idx][:, :L]).any(1))             # exactly where the grid row is all zero
        assert not w[base < 0].any()
        # scatter the 64 slots into [n, ncp] and compare with the fp64 basis
        dense = np.zeros((n, int(np.prod(ncp_axis))))
        for k in range(degrees[2] + 1):
            for j in range(degrees[1] + 1):
                for i in range(degrees[0] + 1):
                    c = base + i + ncp_axis[0] * (j + ncp_axis[1] * k)
                    ok = base >= 0
                    dense[np.nonzero(ok)[0], c[ok]] += w[ok, (k * 4 + j) * 4 + i]
        used = np.zeros(64, dtype=bool)
        for k in range(degrees[2] + 1):
            for j in range(degrees[1] + 1):
                used[[(k * 4 + j) * 4 + i for i in range(degrees[0] + 1)]] = True
        assert not w[:, ~used].any()
        want = msdiff_numpy.dense_basis(degrees, knots, xo[pick]) * inside[pick][:, None]
        err = np.abs(dense - want).max()
        again = np.abs(dense @ cp.astype(np.float64) - rows.cpu().numpy()[:, :L]).max() / np.abs(cp).max()
        assert err <= SPLINE_TOL and again <= SPLINE_TOL, (degrees, L, n, err, again)
    # through the wrapper, an index outside the grid: a zero row, zero weights, base -1
    from deepsdf_amd.mesh import ms_rows_at
    idx = torch.tensor([0, npts - 1, npts, -1, int(np.nonzero(inside)[0][0])], device="cuda")
    rows, w, base = ms_rows_at(field, tiling, N, idx)
    assert base.tolist()[:4] == [-1] * 4 and base[4] >= 0 and not bits(rows[2:4]).any() and not bits(w[:4]).any()
    assert np.array_equal(bits(rows[[0, 1, 4]]), bits(whole[idx[[0, 1, 4]]]))


# ---- 5. the input gradient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(NETS))
def test_module_input_grad_equals_module_backward(name):
    L, kw = NETS[name]
    net = orc.make_net(L, **kw)
    params = orc.init_params(net, 41)
    p64 = {k: v.double() for k, v in params.items()}
    dec = _decoder(L, kw, params)
    eng = dec.engine()
    assert eng.spec.xyz_in_all == (name == "xyz_in_all")
    gen = torch.Generator().manual_seed(5)
    for n in (1, 33, 130):
        # rows off every ReLU kink (oracle margin > 1e-6): the first n such rows of 2 n + 8 drawn
        c = torch.cat([torch.randn(2 * n + 8, L, generator=gen) / math.sqrt(L), torch.rand(2 * n + 8, 3, generator=gen) * 2 - 1], 1)
        keep = orc.decoder_forward(net, p64, c.double(), training=False, track_margin=True)[1].min_abs_pre > 1e-6
        x = c[keep][:n].contiguous()
        assert x.shape[0] == n, (name, n)
        d = torch.randn(n, generator=gen)
        y64, sv = orc.decoder_forward(net, p64, x.double(), training=False, track_margin=True)
        assert float(sv.min_abs_pre.min()) > 1e-6, (name, n)
        _, want = orc.decoder_backward(net, p64, sv, d.double().reshape(-1, 1), training=False)
        xc, dc = x.cuda().contiguous(), d.cuda()
        eng.module_forward(xc, False)
        eng.grads.fill_(-7.25)                                                   # sentinel: the arena must come back unchanged
        got = eng.module_input_grad(dc, n)
        assert bool((eng.grads == -7.25).all()), (name, n)
        eng.module_forward(xc, False)
        again = eng.module_input_grad(dc, n)                                     # two identical calls, identical bytes
        assert np.array_equal(bits(got), bits(again)), (name, n)
        eng.module_forward(xc, False)
        ref = eng.module_backward(dc, n, False, True, False)
        assert np.array_equal(bits(got), bits(ref)), (name, n)                   # the dX launches are module_backward's own
        e, w = rel_err(got.cpu(), want), worst_elem(got.cpu(), want)
        print(f"module_input_grad {name} n {n}: rel err {e:.2e} (bound {GRAD_TOL:.0e}), worst element {w:.2e} (bound {GRAD_ELEM_TOL:.0e})")
        assert e <= GRAD_TOL and w <= GRAD_ELEM_TOL, (name, n)


# ---- 6. the Jacobian against fp64 ---------------------------------------------------------------------------------------------
def _jacobian_case(name, gemm_split=False):
    from deepsdf_amd.mesh import microstructure_mesh_diff, microstructure_sdf_grid, ms_grid_rows
    from deepsdf_amd.spline import BSplineField
    L, kw = NETS[name]
    big = name == "fused_8x512"
    degrees = (1, 1, 1) if big else (2, 1, 3)
    knots = msdiff_numpy.LINEAR_KNOTS if big else [msdiff_numpy.KNOTS[p] for p in degrees]
    N, tiling = ([6, 6, 6] if big else [6, 5, 4]), [2, 1, 1]
    S = msdiff_numpy.Fp64Structure(L, kw, JAC_SEEDS[name], degrees, knots, tiling, N, CAPS_SIX, 0.5 / math.sqrt(L),
                                   quantile=JAC_QUANTILE.get(name, 0.5))
    max_batch = 5 if big else 37
    dec = _decoder(L, kw, S.params, **({"gemm_split": True} if gemm_split else {}))
    assert dec.engine().spec.gemm_split == gemm_split
    field = BSplineField(degrees, knots, S.cp)
    npts = int(np.prod(S.dims))
    d = microstructure_mesh_diff(tiling, dec, field, N, max_batch=max_batch, cap_border_dict=CAPS_SIX)
    jac, axis = d.jacobian()
    V = d.verts.shape[0]
    assert jac.shape == (V, S.ncp, L) and V >= 6
    grid = d.grid.cpu().numpy()
    ep, ea = msdiff_numpy.edges(grid)
    assert np.array_equal(d.edge_point.cpu().numpy(), ep) and np.array_equal(d.edge_axis.cpu().numpy(), ea)
    assert np.array_equal(axis.cpu().numpy(), ea)
    band, r0, r1 = msdiff_numpy.band(ep, ea, S.dims)
    assert np.array_equal(d.band.cpu().numpy(), band) and len(band) > max_batch      # more than one chunk of max_batch
    # fp64: the oracle's G on the kernel's own rows, ms_numpy's basis, the GPU's capped fp32 values for the dt factors
    rows = ms_grid_rows(field, tiling, N, 0, npts).cpu().double().requires_grad_(True)
    raw64, sv = S.decode(rows)
    _, planes = S.cap(raw64)
    gap, margin = S.conditions(raw64, sv, planes, band)
    G = torch.autograd.grad(raw64.sum(), rows)[0][:, :L].numpy()
    raw = microstructure_sdf_grid(tiling, dec, field, N, apply_caps=False).cpu().numpy()
    m = S.inside & (grid.reshape(-1) == raw.reshape(-1))
    m64 = S.inside & (S.cap(raw64)[0].detach().reshape(-1) == raw64.detach().reshape(-1)).numpy()
    J, _ = msdiff_numpy.jacobian(grid, ep, ea, S.vs, G[band], S.B[band], m[band])
    got = jac.cpu().numpy().astype(np.float64)
    top = np.abs(J).reshape(V, -1).max(1)
    err = np.abs(got - J).reshape(V, -1).max(1)
    worst = float((err[top > 0] / top[top > 0]).max())
    seen = dict(axes=set(ea.tolist()), one_capped=bool((S.inside[band][r0] & S.inside[band][r1] & (m[band][r0] != m[band][r1])).any()),
                border=bool((~S.inside[band][r0] | ~S.inside[band][r1]).any()))
    print(f"jacobian {name}{' gemm_split' if gemm_split else ''}: {V} vertices, band {len(band)}, worst entry error {worst:.3e} of the "
          f"vertex's largest entry (bound {JAC_TOL:.0e}); cap gap {gap:.2e}, ReLU margin {margin:.2e}; {seen}")
    assert gap > 1e-6 and margin > 1e-6, (name, gap, margin)
    assert np.array_equal(m[band], m64[band]) and np.array_equal(d.mask.cpu().numpy().astype(bool), m[band])
    assert not err[top == 0].any()
    assert worst <= JAC_TOL, name
    return seen


@pytest.mark.parametrize("name", list(NETS))
def test_jacobian_against_fp64(name):
    seen = _jacobian_case(name)
    if name == "w32_4x32":           # asserted to occur in at least one case: this one
        assert seen["axes"] == {0, 1, 2} and seen["one_capped"] and seen["border"], seen


def test_jacobian_against_fp64_gemm_split():
    _jacobian_case("fused_8x512", gemm_split=True)


# ---- 7. an analytic module: G = (-1, 0, ...) ------------------------------------------------------------------------------------
def test_analytic_module_jacobian():
    from deepsdf_amd.mesh import microstructure_mesh_diff
    tiling, N = [2, 1, 1], [12, 8, 6]
    cp = np.array([[0.35 if i % 2 == 0 else 0.6] for i in range(8)], dtype=np.float32)
    d = microstructure_mesh_diff(tiling, SphereCells(), linear_field(cp), N, max_batch=100)
    jac, axis = d.jacobian()
    V = d.verts.shape[0]
    assert V > 50 and jac.shape == (V, 8, 1)
    assert bool((d.G[d.base >= 0] == -1).all())                                # autograd's gradient of |xyz| - z[0] in z
    axes = ms_numpy.grid_axes(N, tiling)
    dims = [len(a[0]) for a in axes]
    grid = d.grid.cpu().numpy()
    ep, ea = d.edge_point.cpu().numpy(), d.edge_axis.cpu().numpy()
    band, r0, r1 = msdiff_numpy.band(ep, ea, dims)
    inside = ms_numpy.grid_inside(axes)
    B = msdiff_numpy.dense_basis((1, 1, 1), msdiff_numpy.LINEAR_KNOTS, ms_numpy.grid_points(axes, 0)[band]) * inside[band][:, None]
    m = d.mask.cpu().numpy().astype(bool)
    assert m.all()                                                              # the spheres stay clear of the caps and the border
    vs = [2.0 / (n + 2 - 1 - 2) for n in N]
    J, _ = msdiff_numpy.jacobian(grid, ep, ea, vs, -np.ones((len(band), 1)), B, m)
    got = jac.cpu().numpy().astype(np.float64)
    top = np.abs(J).reshape(V, -1).max(1)
    err = np.abs(got - J).reshape(V, -1).max(1)
    assert not err[top == 0].any() and (top > 0).sum() > V // 2
    worst = float((err[top > 0] / top[top > 0]).max())
    # a weight carries the basis bound 2^-16 (of 1, the largest weight); the fp32 dt factor, the scale and the two products add a few ulp
    bound = SPLINE_TOL + 16 * 2.0 ** -24
    print(f"analytic module: {V} vertices, worst entry error {worst:.3e} of the vertex's largest entry (bound {bound:.3e})")
    assert worst <= bound


# ---- 8. adjoint and tangent against the GPU's own dense Jacobian ------------------------------------------------------------------------
def _contraction_check(d, tag):
    jac, axis = d.jacobian()
    V, ncp, L = jac.shape
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(V, 3, generator=gen)
    dcp = torch.randn(ncp, L, generator=gen)
    J = jac.cpu().double()
    wa = w.double()[torch.arange(V), axis.cpu().long()]
    # vjp: sum over vertices; the terms of one entry are the (at most 2 per vertex) products the kernel adds one by one
    terms = wa[:, None, None] * J
    want, mag = terms.sum(0), terms.abs().sum(0)
    got = d.vjp(w.cuda()).cpu().double()
    assert d.vjp_plan()[1] == -(-V // ws_guard.constants()["MSD_VJP_VERTS"])
    nz = int((J != 0).any(2).any(1).sum())
    bound = (2 * V + d.vjp_plan()[1] + 4) * 2.0 ** -24 * mag                      # n roundings of a sum of n terms, each |term| (1 + 3 u)
    bad = (got - want).abs() > bound
    print(f"{tag}: vjp of {V} vertices ({nz} moving) in {d.vjp_plan()[1]} parts, worst error / bound "
          f"{float(((got - want).abs() / bound.clamp_min(1e-300)).max()):.3f}")
    assert not bool(bad.any()), tag
    assert np.array_equal(bits(d.vjp(w.cuda())), bits(got.float()))             # two calls, identical bytes
    # jvp: per vertex a sum over (control point, latent column)
    terms = J * dcp.double()[None]
    want, mag = terms.reshape(V, -1).sum(1), terms.abs().reshape(V, -1).sum(1)
    out = d.jvp(dcp.cuda()).cpu().double()
    off = torch.ones(V, 3, dtype=torch.bool)
    off[torch.arange(V), axis.cpu().long()] = False
    assert not bool(out[off].any())                                             # exact zeros off the edge axis
    got = out[torch.arange(V), axis.cpu().long()]
    nterm = 2 * 64 * L
    bound = (nterm + 8) * 2.0 ** -24 * mag
    print(f"{tag}: jvp worst error / bound {float(((got - want).abs() / bound.clamp_min(1e-300)).max()):.3f}")
    assert not bool(((got - want).abs() > bound).any()), tag
    assert np.array_equal(bits(d.jvp(dcp.cuda())), bits(out.float()))
    return d.vjp_plan()[1]


def test_vjp_and_jvp_equal_the_contraction_of_the_dense_jacobian():
    from deepsdf_amd.mesh import microstructure_mesh_diff
    from deepsdf_amd.spline import BSplineField
    # a band large enough for more than one partial of the adjoint's first stage
    name = "w32_4x32"
    L, kw = NETS[name]
    degrees = (2, 1, 3)
    knots = [msdiff_numpy.KNOTS[p] for p in degrees]
    S = msdiff_numpy.Fp64Structure(L, kw, JAC_SEEDS[name], degrees, knots, [2, 1, 1], [6, 5, 4], CAPS_SIX, 0.5 / math.sqrt(L))
    dec = _decoder(L, kw, S.params)
    field = BSplineField(degrees, knots, S.cp)
    big = microstructure_mesh_diff([2, 1, 1], dec, field, 24, cap_border_dict=CAPS_SIX)
    assert _contraction_check(big, "4x32, N = 24") > 1
    small = microstructure_mesh_diff([2, 1, 1], dec, field, [6, 5, 4], cap_border_dict=CAPS_SIX)
    assert _contraction_check(small, "4x32, N = [6, 5, 4]") == 1
    # 256 latent columns: float4 stores in the dense kernel, four passes of a wave over an endpoint's products in the tangent
    L, kw = NETS["fused_8x512"]
    S = msdiff_numpy.Fp64Structure(L, kw, JAC_SEEDS["fused_8x512"], (1, 1, 1), msdiff_numpy.LINEAR_KNOTS, [2, 1, 1], [6, 6, 6], CAPS_SIX,
                                   0.5 / math.sqrt(L))
    wide = microstructure_mesh_diff([2, 1, 1], _decoder(L, kw, S.params), BSplineField((1, 1, 1), msdiff_numpy.LINEAR_KNOTS, S.cp), 6,
                                    cap_border_dict=CAPS_SIX)
    _contraction_check(wide, "8x512, N = 6")


def test_vjp_over_several_output_tiles_and_under_red_zones():
    """ncp * L = 288 * 67 = 19296 floats: three LDS tiles of the adjoint's first stage, an odd L (dword stores of the dense kernel);
    the scratch buffer poisoned and fenced by the planner's red zone."""
    from deepsdf_amd import _lib
    from deepsdf_amd.mesh import microstructure_mesh_diff
    L, degrees = 67, (2, 1, 3)
    field, knots, cp = make_field(degrees, L, 9, lo=0.2, hi=0.7)

    class FirstColumn(torch.nn.Module):
        def forward(self, x):
            return x[:, L:].norm(dim=1, keepdim=True) - x[:, :1] + 0.002 * torch.sin(x[:, 1:L]).sum(1, keepdim=True)

    d = microstructure_mesh_diff([2, 1, 1], FirstColumn(), field, [12, 8, 6], max_batch=100)
    assert d.n_control_points * L > 2 * ws_guard.constants()["MSD_VJP_TILE"]
    _contraction_check(d, "67 columns, 288 control points")
    V = d.verts.shape[0]
    lib = _lib.lib()
    gv = torch.randn(V, 3, generator=torch.Generator().manual_seed(1)).cuda()
    plain = d.vjp(gv)
    with ws_guard.redzone():
        nb, parts = C.c_size_t(), C.c_int32()
        _lib.check(lib.dsdf_msd_vjp_workspace_bytes(V, d.n_control_points, L, C.byref(nb), C.byref(parts)))
        ws = ws_guard.poisoned(nb.value, 0xC3)
        F = ws_guard.Fences()
        out = F.new("grad_cp", (d.n_control_points, L))
        m, b = d._structs()
        _lib.check(lib.dsdf_msd_vjp(C.byref(m), C.byref(b), ws_guard.ptr(gv), ws_guard.ptr(out), ws_guard.ptr(ws), nb.value, ws_guard.stream()))
        ws_guard.assert_clean(ws, 0xC3, "msd_vjp")
        F.check("msd_vjp")
    assert np.array_equal(bits(out), bits(plain))
    F = ws_guard.Fences()
    jac, axis = F.new("jac", (V, d.n_control_points, L)), F.new("axis", V, torch.int32)
    m, b = d._structs()
    _lib.check(lib.dsdf_msd_jacobian(C.byref(m), C.byref(b), 0, ws_guard.ptr(jac), ws_guard.ptr(axis), ws_guard.stream()))
    dv = F.new("d_verts", (V, 3))
    _lib.check(lib.dsdf_msd_jvp(C.byref(m), C.byref(b), ws_guard.ptr(torch.ones(d.n_control_points, L, device="cuda")), ws_guard.ptr(dv),
                                ws_guard.stream()))
    F.check("msd_jacobian / msd_jvp")
    assert np.array_equal(bits(jac), bits(d.jacobian()[0]))


# ---- 9. the interface ---------------------------------------------------------------------------------------------------------
def test_create_mesh_microstructure_diff_interface(monkeypatch):
    from deep_sdf.mesh import create_mesh_microstructure, create_mesh_microstructure_diff
    from deepsdf_amd import mesh as M
    from deepsdf_amd.spline import BSplineField
    name = "w32_4x32"
    L, kw = NETS[name]
    degrees = (2, 1, 3)
    knots = [msdiff_numpy.KNOTS[p] for p in degrees]
    tiling, N = [2, 1, 1], [6, 5, 4]
    S = msdiff_numpy.Fp64Structure(L, kw, JAC_SEEDS[name], degrees, knots, tiling, N, CAPS_SIX, 0.5 / math.sqrt(L))
    dec = _decoder(L, kw, S.params)
    field = BSplineField(degrees, knots, S.cp)
    verts, faces = create_mesh_microstructure(tiling, dec, field, "unused", N=N, cap_border_dict=CAPS_SIX)
    v0, f0, none = create_mesh_microstructure_diff(tiling, dec, field, N=N, cap_border_dict=CAPS_SIX)
    assert none == [] and v0.tobytes() == verts.tobytes() and f0.tobytes() == faces.tobytes()
    results = []
    for mb in (32 ** 3, 29, 32 ** 3):
        v, f, jac = create_mesh_microstructure_diff(tiling, dec, field, N=N, max_batch=mb, cap_border_dict=CAPS_SIX, compute_derivatives=True)
        assert v.dtype == verts.dtype and f.dtype == faces.dtype and v.tobytes() == verts.tobytes() and f.tobytes() == faces.tobytes()
        assert jac.shape == (len(verts), 3, S.ncp, L) and jac.dtype == np.float32
        results.append(jac)
    assert results[0].tobytes() == results[1].tobytes() == results[2].tobytes()          # no dependence on max_batch; repeatable
    d = M.microstructure_mesh_diff(tiling, dec, field, N, cap_border_dict=CAPS_SIX)
    compact, axis = d.jacobian()
    axis = axis.cpu().numpy()
    V = len(verts)
    for a in range(3):
        on = axis == a
        assert np.array_equal(bits(results[0][on, a]), bits(compact.cpu().numpy()[on]))
        assert not bits(results[0][~on, a]).any()                                         # zero in the two off-axis coordinates
    assert np.abs(results[0]).max() > 0 and V > 10
    with pytest.raises(NotImplementedError):
        create_mesh_microstructure_diff(tiling, dec, field, N=N, output_tetmesh=True)
    with pytest.raises(NotImplementedError):
        create_mesh_microstructure(tiling, dec, field, "unused", N=N, compute_derivatives=True)    # untouched
    monkeypatch.setattr(M, "_free_device_memory", lambda device: 1000)
    with pytest.raises(MemoryError, match=str(4 * V * 3 * S.ncp * L)):
        d.jacobian(dense=True)
    with pytest.raises(MemoryError, match=str(4 * V * S.ncp * L)):
        d.jacobian()


def test_create_microstructure_cli_writes_the_jacobian(tmp_path):
    exp = _tiny_experiment(str(tmp_path))
    out, jf = str(tmp_path / "structure.ply"), str(tmp_path / "jac.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "create_microstructure.py"), "-e", exp, "-c", "latest", "--tiling", "2", "1", "1",
                        "--codes", "0", "1", "2", "3", "4", "5", "6", "8", "--resolution", "12", "--cap", "x1=1:0.1", "z0=-1:0",
                        "--jacobian", jf, "-o", out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(jf)
    V = len(z["verts"])
    assert V > 0 and z["faces"].shape[1] == 3 and z["jac"].shape == (V, 8, 4) and z["axis"].shape == (V,)
    assert set(np.unique(z["axis"]).tolist()) <= {0, 1, 2} and np.isfinite(z["jac"]).all() and np.abs(z["jac"]).max() > 0
