"""-m gpu: d(volume mesh vertices) / d(spline control points) (csrc/voldiff.hpp, dsdf_vd_*).  Kernel level: the tangent
and the adjoint against the fp64 oracle of tests/voldiff_numpy.py on a synthetic band, at bounds counted from the kernels; the
dense projected derivative bit for bit against its stated fp32 sequence; entries that are out of range; red zones.  Structure
level: DeepSDFMesh's volume stage on a tiny experiment, and the optimisation driver."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tests import tet_numpy, voldiff_numpy as vd, ws_guard

pytestmark = pytest.mark.gpu

GRID = np.random.default_rng(1).uniform(-1, 1, (6, 5, 4)).astype(np.float32)
SPACING = (0.5, 0.25, 0.75)
CASES = {"deg131_L2": ((1, 3, 1), (3, 5, 2), 2), "deg313_L128": ((3, 1, 3), (4, 4, 5), 128)}


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Band:
    """The grid, its mesh's (vert_point, vert_class) and a synthetic band, on the host (oracle) and on the device (kernels)."""

    def __init__(self, grid, degrees, n_cp, L, tau, seed=7, scale=None):
        self.grid, self.degrees, self.n_cp, self.L, self.tau = grid, degrees, n_cp, L, tau
        _, _, self.vp, self.vc = tet_numpy.vertices(grid, 0.0, SPACING, (0, 0, 0), tau)
        self.sb = vd.synthetic_band(grid.shape, self.vp, self.vc, degrees, n_cp, L, seed)
        self.scale = np.asarray([s / 2 for s in SPACING] if scale is None else scale, dtype=np.float32)
        self.index = np.nonzero(self.vc > 0)[0].astype(np.int32)
        self.ncp = int(np.prod(n_cp))

    def upload(self):
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        self.dev = dict(grid=cu(self.grid), vp=cu(self.vp.astype(np.int64)), vc=cu(self.vc.astype(np.int32)), index=cu(self.index),
                        **{k: cu(self.sb[k]) for k in ("band_of", "G", "weights", "base", "mask")})
        return self

    def structs(self):
        from deepsdf_amd import _lib
        d = self.dev
        m, b = _lib.DsdfVdMesh(), _lib.DsdfMsdBand()
        m.grid, m.vert_point, m.vert_class, m.vert_index, m.band_of = (d[k].data_ptr() for k in ("grid", "vp", "vc", "index", "band_of"))
        m.n_verts, m.n_moving, m.level, m.t_clamp = d["vp"].numel(), d["index"].numel(), 0.0, self.tau
        b.G, b.weights, b.base, b.mask = (d[k].data_ptr() for k in ("G", "weights", "base", "mask"))
        b.n_band, b.ld_g, b.L = d["G"].shape[0], d["G"].stride(0), self.L
        for a in range(3):
            m.dims[a], m.scale[a] = self.grid.shape[a], float(self.scale[a])
            b.degree[a], b.n_cp[a] = self.degrees[a], self.n_cp[a]
        return m, b

    def parts(self):
        from deepsdf_amd import _lib
        nb, parts = C.c_size_t(), C.c_int32()
        _lib.check(_lib.lib().dsdf_vd_vjp_workspace_bytes(self.dev["index"].numel(), self.ncp, self.L, C.byref(nb), C.byref(parts)))
        return nb.value, parts.value

    def jvp(self, dcp, out=None):
        from deepsdf_amd import _lib
        out = torch.empty(self.dev["vp"].numel(), 3, device="cuda") if out is None else out
        m, b = self.structs()
        _lib.check(_lib.lib().dsdf_vd_jvp(C.byref(m), C.byref(b), ws_guard.ptr(dcp), ws_guard.ptr(out), ws_guard.stream()))
        return out

    def vjp(self, gv, out=None, ws=None):
        from deepsdf_amd import _lib
        out = torch.empty(self.ncp, self.L, device="cuda") if out is None else out
        nbytes = self.parts()[0]
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device="cuda") if ws is None else ws
        m, b = self.structs()
        _lib.check(_lib.lib().dsdf_vd_vjp(C.byref(m), C.byref(b), ws_guard.ptr(gv), ws_guard.ptr(out), ws_guard.ptr(ws), nbytes, ws_guard.stream()))
        return out

    def dtheta(self, normals, stretch, clip, out=None):
        from deepsdf_amd import _lib
        out = torch.empty(self.dev["index"].numel(), 3, self.ncp * self.L, device="cuda") if out is None else out
        m, b = self.structs()
        _lib.check(_lib.lib().dsdf_vd_dtheta(C.byref(m), C.byref(b), ws_guard.ptr(normals), (C.c_float * 3)(*stretch), float(clip),
                                             ws_guard.ptr(out), ws_guard.stream()))
        return out

    def oracle(self):
        """(T [V, ncp, L], dm * scale [V, 3], terms per control point of the adjoint, the endpoints, sum_e |endpoint's term|)."""
        sb = self.sb
        T, dm, (ok0, ok1, r0, r1), Tabs = vd.tangent(self.grid, self.vp, self.vc, self.tau, sb["band"], sb["G"], sb["B"], sb["mask"])
        n_terms = (ok0[:, None] & sb["support"][r0]).sum(0) + (ok1[:, None] & sb["support"][r1]).sum(0)
        return T, dm * self.scale.astype(np.float64), n_terms, (ok0, ok1, r0, r1), Tabs


def _check_contractions(B, tag, keep=None):
    """jvp and vjp against the oracle's fp64 contraction at the bounds counted in tests/voldiff_numpy.py; returns (worst jvp error /
    bound, worst vjp error / bound).  keep [V] bool: the caller has listed only these vertices in B.index, and only their terms are in
    the oracle's sums; the rows of the others must be exact zeros (dsdf_vd_jvp zeroes all of d_verts before it writes a listed row)."""
    T, ds, n_terms, (ok0, ok1, r0, r1), Tabs = B.oracle()
    if keep is not None:
        T[~keep], Tabs[~keep] = 0, 0
        n_terms = ((ok0 & keep)[:, None] & B.sb["support"][r0]).sum(0) + ((ok1 & keep)[:, None] & B.sb["support"][r1]).sum(0)
    V = len(B.vp)
    rng = np.random.default_rng(3)
    w = rng.standard_normal((V, 3)).astype(np.float32)
    dcp = rng.standard_normal((B.ncp, B.L)).astype(np.float32)
    want = (ds[:, :, None] * (T * dcp.astype(np.float64)[None]).reshape(V, 1, -1)).sum(2)
    mag = (ds[:, :, None] * (Tabs * np.abs(dcp).astype(np.float64)[None]).reshape(V, 1, -1)).sum(2)
    got = B.jvp(torch.from_numpy(dcp).cuda())
    assert np.array_equal(bits(got), bits(B.jvp(torch.from_numpy(dcp).cuda())))                   # two runs, identical bytes
    got = got.cpu().numpy().astype(np.float64)
    bound = vd.jvp_bound(B.degrees, B.L, mag)
    assert not got[mag == 0].any()                                                                # exact zeros where nothing moves
    with np.errstate(divide="ignore", invalid="ignore"):
        rj = float(np.nanmax(np.where(mag > 0, np.abs(got - want) / bound, 0.0)))
    terms = (ds * w.astype(np.float64)).sum(1)[:, None, None] * T
    want, mag = terms.sum(0), (np.abs(ds * w).sum(1)[:, None, None] * Tabs).sum(0)
    gv = torch.from_numpy(w).cuda()
    got = B.vjp(gv)
    assert np.array_equal(bits(got), bits(B.vjp(gv)))
    got = got.cpu().numpy().astype(np.float64)
    parts = B.parts()[1]
    assert parts == -(-len(B.index) // ws_guard.constants()["MSD_VJP_VERTS"])
    bound = vd.vjp_bound(n_terms, parts, mag)
    assert not got[mag == 0].any()
    with np.errstate(divide="ignore", invalid="ignore"):
        rv = float(np.nanmax(np.where(mag > 0, np.abs(got - want) / bound, 0.0)))
    print(f"{tag}: {len(B.index)} listed vertices, {parts} parts; jvp worst error / bound {rj:.3f}, vjp worst error / bound {rv:.3f}")
    assert rj <= 1 and rv <= 1, tag
    return rj, rv


@pytest.mark.parametrize("tau", [0.0, 0.25])
@pytest.mark.parametrize("case", list(CASES))
def test_jvp_and_vjp_against_the_fp64_oracle(case, tau):
    degrees, n_cp, L = CASES[case]
    B = Band(GRID, degrees, n_cp, L, tau).upload()
    _, _, _, (ok0, ok1, r0, r1), _ = B.oracle()
    mv = vd.moves(GRID, B.vp, B.vc, tau)
    assert set(B.vc[mv].tolist()) == set(range(1, 8))                                             # all seven classes move
    sb = B.sb
    one_masked = mv & ((sb["mask"][r0] == 0) != (sb["mask"][r1] == 0))
    outside = mv & ((sb["base"][r0] < 0) | (sb["base"][r1] < 0))
    assert one_masked.any() and outside.any() and (tau == 0 or ((B.vc > 0) & ~mv).sum() >= 63)
    if case == "deg313_L128":
        assert B.ncp * L == 10240 > ws_guard.constants()["MSD_VJP_TILE"]
    _check_contractions(B, f"{case}, tau {tau}")


def test_more_than_one_part_of_the_adjoint():
    grid = np.random.default_rng(1).uniform(-1, 1, (9, 9, 9)).astype(np.float32)
    degrees, n_cp, L = CASES["deg131_L2"]
    B = Band(grid, degrees, n_cp, L, 0.1).upload()
    assert len(B.index) > ws_guard.constants()["MSD_VJP_VERTS"] and len(B.index) % 4 != 0 and B.parts()[1] >= 2
    _check_contractions(B, "9 x 9 x 9")


# ---- the dense projected derivative ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degrees,n_cp,L", [((1, 1, 1), (2, 2, 2), 1), ((1, 1, 3), (2, 2, 5), 2)])
def test_dtheta_is_its_stated_sequence_bit_for_bit(degrees, n_cp, L):
    """R = 8 (the smallest control net there is: 2 x 2 x 2, one latent column) and R = 40; stretch * scale = 1 on every axis, so
    j = T, and entries are planted at exactly +clip and -clip (kept) and just outside (zeroed); one zero normal."""
    tau, clip, stretch, scale = 0.25, 1.0, (2.0, 1.0, 1.0), (0.5, 1.0, 1.0)
    B = Band(GRID, degrees, n_cp, L, tau, scale=scale)
    sb, F = B.sb, np.float32
    mv = vd.moves(GRID, B.vp, B.vc, tau)
    _, r0, r1 = vd.band(GRID.shape, B.vp, B.vc)
    v0 = int(np.nonzero(mv & (r0 != r1))[0][0])                                                   # a vertex that moves
    a, b = r0[v0], r1[v0]
    sb["mask"][a], sb["mask"][b], sb["base"][a] = 1, 0, 0                                         # only endpoint p contributes
    f = GRID.reshape(-1)
    s0, s1 = f[B.vp[v0]], f[B.vp[v0] + vd.directions(B.vc[v0:v0 + 1])[0][0] @ vd.strides(GRID.shape)]
    d = F(s1 - s0)
    dt0 = F(F(0) - s1) / F(d * d)
    g = F(1) / dt0
    cand, up, dn = [g], g, g
    for _ in range(8):
        up, dn = np.nextafter(up, F(np.inf)), np.nextafter(dn, F(-np.inf))
        cand += [up, dn]
    g1 = next(x for x in cand if F(dt0 * F(x)) == F(1))                                           # dt0 * g1 rounds to exactly 1
    sb["weights"][a] = 0
    sb["weights"][a, 0], sb["weights"][a, 1] = 1.0, -1.0                                          # control points 0 and 1: T = +-1
    sb["G"][a, 0] = g1
    if L > 1:
        sb["G"][a, 1] = F(g1 * F(1 + 2.0 ** -10))                                                 # just outside the clip
    else:
        sb["weights"][a, 4] = F(1 + 2.0 ** -10)                                                   # control point (0, 1, 0)
    sb["B"][a], sb["support"][a] = 0, False
    for k in range(degrees[2] + 1):
        for j in range(degrees[1] + 1):
            for i in range(degrees[0] + 1):
                c = i + n_cp[0] * (j + n_cp[1] * k)
                sb["B"][a, c], sb["support"][a, c] = sb["weights"][a, (k * 4 + j) * 4 + i], True
    B.upload()
    rng = np.random.default_rng(5)
    normals = rng.standard_normal((len(B.vp), 3)).astype(np.float32)
    zero_at = int(np.nonzero(mv)[0][3])
    assert zero_at != v0
    normals[zero_at] = 0
    want = vd.dtheta_fp32(GRID, B.vp, B.vc, B.index, tau, sb, scale, normals, stretch, clip, degrees, n_cp)
    free = vd.dtheta_fp32(GRID, B.vp, B.vc, B.index, tau, sb, scale, normals, stretch, 0.0, degrees, n_cp)
    got = B.dtheta(torch.from_numpy(normals).cuda(), stretch, clip)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(B.dtheta(torch.from_numpy(normals).cuda(), stretch, 0.0)), bits(free))
    i0, iz = int(np.nonzero(B.index == v0)[0][0]), int(np.nonzero(B.index == zero_at)[0][0])
    R = B.ncp * L
    assert want.shape == (len(B.index), 3, R) and not bits(want[iz]).any() and free[i0].any()
    kept = [0 * L, 1 * L]                                                                         # T = +1 and -1: exactly at the clip
    gone = [0 * L + 1, 1 * L + 1] if L > 1 else [2]                                               # |T| = 1 + 2^-10
    assert want[i0][:, kept].any(0).all() and np.array_equal(bits(want[i0][:, kept]), bits(free[i0][:, kept]))
    assert not want[i0][:, gone].any() and free[i0][:, gone].any(0).all()         # zero of either sign
    changed = (bits(want) != bits(free)).any(1)
    print(f"R = {R}: {int(changed.sum())} of {changed.size} (vertex, column) pairs have a clipped coordinate; "
          f"{int((~bits(want).any(2).any(1)).sum())} zero rows of {len(B.index)}")
    assert changed.sum() > 4 and (~changed).sum() > 4                                             # entries on both sides of the clip
    assert not bits(want[~mv[B.index]]).any() and (~mv[B.index]).sum() >= 63                      # held by the clamp: zero rows


# ---- robustness -------------------------------------------------------------------------------------------------------------------
def test_out_of_range_entries_contribute_nothing_under_red_zones():
    from deepsdf_amd import _lib
    degrees, n_cp, L = CASES["deg131_L2"]
    tau = 0.25
    B = Band(GRID, degrees, n_cp, L, tau)
    V, npts = len(B.vp), GRID.size
    clean = Band(GRID, degrees, n_cp, L, tau).upload()
    # four more vertices: class 8, class -1, p = -1, and the last grid point with class 7 (q past the grid); then list entries out of range
    B.vp = np.concatenate([B.vp, [B.vp[5], B.vp[6], -1, npts - 1, npts]]).astype(np.int64)
    B.vc = np.concatenate([B.vc, [8, -1, 3, 7, 1]]).astype(np.int32)
    B.index = np.concatenate([[-1], B.index[:100], [V + 5, 2 ** 31 - 1], np.arange(V, V + 5), B.index[100:], [-(2 ** 31)]]).astype(np.int32)
    B.upload()
    rng = np.random.default_rng(9)
    dcp = torch.from_numpy(rng.standard_normal((B.ncp, L)).astype(np.float32)).cuda()
    gv = torch.from_numpy(rng.standard_normal((V + 5, 3)).astype(np.float32)).cuda()
    normals = torch.from_numpy(rng.standard_normal((V + 5, 3)).astype(np.float32)).cuda()
    want_j, want_v = clean.jvp(dcp), clean.vjp(gv[:V].contiguous())
    want_d = clean.dtheta(normals[:V].contiguous(), (2.0, 1.0, 1.0), 1.0)
    results = []
    with ws_guard.redzone():
        for fill in (0x00, 0xFF):
            nbytes = B.parts()[0]
            ws = ws_guard.poisoned(nbytes, fill)
            F = ws_guard.Fences()
            dv, gc = F.new("d_verts", (V + 5, 3)), F.new("grad_cp", (B.ncp, L))
            dt = F.new("dtheta", (len(B.index), 3, B.ncp * L))
            B.jvp(dcp, dv)
            B.dtheta(normals, (2.0, 1.0, 1.0), 1.0, dt)
            B.vjp(gv, gc, ws)
            ws_guard.assert_clean(ws, fill, "vd_vjp")
            rows, _ = _lib.ws_regions()
            assert [r[0] for r in rows] == ["vd_vjp_part"]
            F.check("vd_jvp / vd_vjp / vd_dtheta")
            results.append((dv.clone(), gc.clone(), dt.clone()))
    for dv, gc, dt in results:
        assert np.array_equal(bits(dv[:V]), bits(want_j)) and not bits(dv[V:]).any()
        assert np.array_equal(bits(gc), bits(want_v))
        keep = np.ones(len(B.index), dtype=bool)
        keep[[0, 101, 102, 103, 104, 105, 106, 107, len(B.index) - 1]] = False
        assert np.array_equal(bits(dt[torch.from_numpy(keep).cuda()]), bits(want_d))
        assert not bits(dt[torch.from_numpy(~keep).cuda()]).any()                    # list entries, classes, points out of range: zero rows
    lib = _lib.lib()
    m, b = clean.structs()
    m.t_clamp = 0.5
    assert lib.dsdf_vd_jvp(C.byref(m), C.byref(b), ws_guard.ptr(dcp), ws_guard.ptr(want_j), ws_guard.stream()) == -1
    assert b"t_clamp" in lib.dsdf_last_error()
    m, b = clean.structs()
    m.vert_index = 0
    assert lib.dsdf_vd_vjp(C.byref(m), C.byref(b), ws_guard.ptr(gv), ws_guard.ptr(want_v), None, 0, ws_guard.stream()) == -1


# ---- structure level --------------------------------------------------------------------------------------------------------------
def _geometry(tmp_path, remove_orphans, t_clamp):
    from analysis.geometry import DeepSDFMesh
    from deepsdf_amd.mesh import default_cap_border_dict
    from tests.test_gpu_microstructure import _tiny_experiment
    exp = _tiny_experiment(str(tmp_path))
    options = dict(experiment_directory=exp, checkpoint="latest", degrees=[1, 1, 1], refinement=1, cap_border_dict=default_cap_border_dict(),
                   N_base_reconstruction=4, tiling=[2, 1, 1], remove_orphans=remove_orphans)
    dm = DeepSDFMesh(options)
    with pytest.raises(RuntimeError):
        dm.get_dTheta()
    dm.generate_surface_mesh(np.tile(dm.latent[0], (27, 1)))
    dm.generate_volume_mesh(t_clamp=t_clamp)
    return dm, options


def _structure_oracle(dm):
    """(T [V, ncp, L] fp64 from the volume band's own fp32 rows, d * scale * STRETCH [V, 3], terms per control point, parts,
    sum_e |endpoint's term|)."""
    from analysis.geometry import STRETCH
    v = dm.volume_diff
    n_cp, deg = v.diff._n_cp, v.diff._degrees
    band, base, w = v.band.cpu().numpy(), v.base.cpu().numpy(), v.weights.cpu().numpy().astype(np.float64)
    ncp = int(np.prod(n_cp))
    Bd, support = np.zeros((len(band), ncp)), np.zeros((len(band), ncp), dtype=bool)
    rows = np.nonzero(base >= 0)[0]
    for k in range(deg[2] + 1):
        for j in range(deg[1] + 1):
            for i in range(deg[0] + 1):
                c = base[rows] + i + n_cp[0] * (j + n_cp[1] * k)
                Bd[rows, c], support[rows, c] = w[rows, (k * 4 + j) * 4 + i], True
    grid, vp, vc = v.grid.cpu().numpy(), v.vert_point.cpu().numpy(), v.vert_class.cpu().numpy()
    T, dm_, (ok0, ok1, r0, r1), Tabs = vd.tangent(grid, vp, vc, v.t_clamp, band, v.G.cpu().numpy(), Bd, v.mask.cpu().numpy())
    n_terms = (ok0[:, None] & support[r0]).sum(0) + (ok1[:, None] & support[r1]).sum(0)
    ds = dm_ * np.asarray(v.diff._scale, dtype=np.float64) * np.asarray(STRETCH, dtype=np.float64)
    return T, ds, n_terms, v.vjp_plan()[1], Tabs


@pytest.mark.parametrize("remove_orphans", [True, False])
def test_deepsdfmesh_volume_derivative(tmp_path, remove_orphans):
    from analysis.geometry import CLIP, STRETCH
    from analysis.problems.CantileverBeam import CantileverBeam
    tau = 0.05
    dm, _ = _geometry(tmp_path, remove_orphans, tau)
    vm, v = dm.volume_mesh, dm.volume_diff
    V, R = vm.n_verts, v.n_control_points * v.latent_size
    vp, vc = v.vert_point.cpu().numpy(), v.vert_class.cpu().numpy()
    assert np.array_equal(v.moving.cpu().numpy(), np.nonzero(vc > 0)[0]) and {0, 1, 2, 4} <= set(vc.tolist()) and set(vc.tolist()) & {3, 5, 6, 7}
    # 1. the vertices from (vert_point, vert_class, diff.grid, t_clamp) alone
    vs = dm.diff.voxel_size
    again = vd.vertices_from_edges(dm.diff.grid.cpu().numpy(), vp, vc, tau, 0.0, vs)
    again = (again.astype(np.float64) - np.asarray(vs, dtype=np.float64)) / 2 * np.asarray(STRETCH, dtype=np.float64)
    assert np.array_equal(again.view(np.uint64), vm.verts.cpu().numpy().view(np.uint64))
    # 2. classes 1 / 2 / 4 of an unclamped mesh: the surface derivative's tangent, bit for bit (both unstretched)
    dm.generate_volume_mesh(t_clamp=0.0)
    v0 = dm.volume_diff
    dcp = torch.randn(v.n_control_points, v.latent_size, generator=torch.Generator().manual_seed(2)).cuda()
    sj, vj = dm.diff.jvp(dcp), v0.jvp(dcp)
    key = {int(p) * 8 + (1 << int(a)): i for i, (p, a) in enumerate(zip(dm.diff.edge_point.cpu().numpy(), dm.diff.edge_axis.cpu().numpy()))}
    p0, c0 = v0.vert_point.cpu().numpy(), v0.vert_class.cpu().numpy()
    ids = np.nonzero(np.isin(c0, (1, 2, 4)))[0]
    match = np.array([key[int(p0[i]) * 8 + int(c0[i])] for i in ids])
    assert len(ids) > 50 and (remove_orphans or len(ids) == sj.shape[0])
    assert np.array_equal(bits(vj[torch.from_numpy(ids).cuda()]), bits(sj[torch.from_numpy(match).cuda()])) and bits(sj).any()
    assert bits(vj[torch.from_numpy(np.nonzero(np.isin(c0, (3, 5, 6, 7)))[0]).cuda()]).any() and not bits(vj[torch.from_numpy(np.nonzero(c0 == 0)[0]).cuda()]).any()
    dm.generate_volume_mesh(t_clamp=tau)
    vm, v = dm.volume_mesh, dm.volume_diff
    # 3. the elasticity gradients through the dense array and through the adjoint
    beam = CantileverBeam(str(tmp_path))
    beam.set_mesh(vm)
    beam.set_up()
    beam.solve()
    T, ds, n_terms, parts, Tabs = _structure_oracle(dm)
    normals = dm.volume_normals()
    dT = dm.get_dTheta()
    mvi = v.moving.long()
    assert dT.shape == (V, 3, R) and dT.dtype == torch.float32
    assert np.array_equal(bits(dT[mvi]), bits(v.dtheta_moving(normals, STRETCH, CLIP)))
    still = torch.ones(V, dtype=torch.bool, device=dT.device)
    still[mvi] = False
    assert not bits(dT[still]).any()
    free = torch.zeros_like(dT)
    free[mvi] = v.dtheta_moving(normals, STRETCH, 0.0)
    print(f"remove_orphans={remove_orphans}: {V} vertices, {mvi.numel()} listed, {int((bits(dT) != bits(free)).sum())} entries clipped")
    n64 = normals.cpu().numpy().astype(np.float64)
    nn = (n64 * n64).sum(1)
    gC = beam.ElasticitySolver.compliance_shape_gradient("mean")
    g64 = gC.cpu().numpy().astype(np.float64)
    # every elementary term of entry (k, l) is bounded by (sum_b |g_b n_b|) (sum_b |n_b| ds_b) / (n . n) |dt m G B|
    proj = np.where(nn > 0, np.abs(g64 * n64).sum(1) * np.abs(n64 * ds).sum(1) / np.where(nn > 0, nn, 1.0), 0.0)
    mag = (proj[:, None, None] * Tabs).sum(0)
    dense = (g64[:, :, None] * free.cpu().numpy().astype(np.float64)).sum((0, 1)).reshape(mag.shape)
    adj = beam.compute_compliance_gradient(dm).reshape(mag.shape)
    assert adj.dtype == np.float64 and np.abs(adj).max() > 0
    # the adjoint: the kernel's 11 + its n_terms + parts additions, and the projection in fp32 (gC to fp32, three products and two
    # sums of n . g, the same for n . n, the quotient, times n, times the stretch: 1 + 3 + 3 + 1 + 1 + 1); the dense array: T (dt 5, two
    # products, one sum), stretch * scale, j, n j and its three sums, n . n 3, the quotient, times n: 19; its contraction runs in fp64
    bound = (n_terms[:, None] + parts + 11 + 10 + 19) * vd.U * mag
    ratio = float(np.nanmax(np.where(mag > 0, np.abs(dense - adj) / np.where(mag > 0, bound, 1.0), 0.0)))
    print(f"remove_orphans={remove_orphans}: dense dTheta . gC against compute_compliance_gradient, worst difference / bound {ratio:.3f}")
    assert ratio <= 1
    if not bool((bits(dT) != bits(free)).any()):                                                     # nothing clipped: the reference's route too
        assert np.abs(beam.compute_compliance(dT)[1].reshape(mag.shape) - adj).max() <= float(bound.max())
    # 4. the volume's gradient without the projection against the oracle's J^T S gV
    gV = beam.ElasticitySolver.volume_shape_gradient()
    gv64 = gV.cpu().numpy().astype(np.float64)
    terms = (ds * gv64).sum(1)[:, None, None] * T
    want, mag = terms.sum(0), (np.abs(ds * gv64).sum(1)[:, None, None] * Tabs).sum(0)
    got = dm.shape_gradient(gV, project=False).cpu().numpy().astype(np.float64)
    bound = vd.vjp_bound(n_terms, parts, mag) + 2 * vd.U * mag                                       # + gV to fp32, times the stretch
    ratio = float(np.nanmax(np.where(mag > 0, np.abs(got - want) / np.where(mag > 0, bound, 1.0), 0.0)))
    print(f"remove_orphans={remove_orphans}: shape_gradient(gV, project=False) against the oracle, worst error / bound {ratio:.3f}")
    assert ratio <= 1 and np.abs(want).max() > 0
    assert np.array_equal(beam.compute_volume_gradient(dm), dm.shape_gradient(gV).double().reshape(-1).cpu().numpy())
    with pytest.raises(ValueError):
        dm.shape_gradient(gV[:-1])


def test_volume_jacobian_and_memory_guard(tmp_path, monkeypatch):
    from deepsdf_amd import mesh as M
    dm, _ = _geometry(tmp_path, False, 0.05)
    v = dm.volume_diff
    jac = v.jacobian()
    V, ncp, L = v.n_verts, v.n_control_points, v.latent_size
    assert jac.shape == (V, 3, ncp, L)
    g = torch.randn(V, 3, generator=torch.Generator().manual_seed(4)).cuda()
    terms = g.double()[:, :, None, None] * jac.double()
    want, mag = terms.sum((0, 1)), terms.abs().sum((0, 1))
    got = v.vjp(g).double()
    # both sides in fp32: the adjoint's 2 Vm + parts additions and 11 factor roundings, the tangent's 16 for a unit vector
    bound = (2 * v.moving.numel() + v.vjp_plan()[1] + 11 + 16) * vd.U * mag
    assert not bool(((got - want).abs() > bound).any()) and float(want.abs().max()) > 0
    monkeypatch.setattr(M, "_free_device_memory", lambda device: 1000)
    with pytest.raises(MemoryError, match=str(4 * V * 3 * ncp * L)):
        v.jacobian()
    with pytest.raises(MemoryError, match=str(4 * v.moving.numel() * 3 * ncp * L)):
        v.dtheta_moving(dm.volume_normals())


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def test_struct_optimization_evaluates_once_and_caches(tmp_path):
    from deepsdf_amd.mesh import default_cap_border_dict
    from optimization.opti import struct_optimization
    from tests.test_gpu_microstructure import _tiny_experiment
    exp = _tiny_experiment(str(tmp_path))
    mesh = dict(experiment_directory=exp, checkpoint="latest", degrees=[1, 1, 1], refinement=1, cap_border_dict=default_cap_border_dict(),
                N_base_reconstruction=4, tiling=[2, 1, 1], remove_orphans=True)
    runs = {}
    for name, dense in (("adjoint", False), ("dense", True)):
        folder = tmp_path / name
        folder.mkdir()
        cfg = dict(mesh=mesh, optimization=dict(method="COBYLA", maxiter=1), general=dict(volume_constraint=0.5, t_clamp=0.05, dense_dtheta=dense))
        json.dump(cfg, open(folder / "config.json", "w"))
        so = struct_optimization(folder)
        so.set_x0()
        assert so.start_values.shape == (27 * 4,) and so.bounds == [(-1, 1)] * 108
        x = np.tile(so.geometry.latent[0], 27).astype(np.float64)
        comp, dcomp = so.objective(x)
        assert so.iteration == 1
        cons, dvol = so.constraint(x.copy())
        assert so.iteration == 1 and len(so.cache) == 1
        res = json.load(open(folder / "results.json"))
        assert res["compliance"] == [comp] and [w - 0.5 for w in res["volume"]] == [cons] and res["design_vector"] == [x.tolist()]
        assert dcomp.shape == dvol.shape == (108,) and dcomp.dtype == np.float64 and comp > 0 and np.abs(dvol).max() > 0
        runs[name] = (so, comp, dcomp, cons, dvol)
    (so, comp, dcomp, cons, dvol), (sd, comp_d, dcomp_d, cons_d, dvol_d) = runs["adjoint"], runs["dense"]
    assert comp == comp_d and cons == cons_d
    # the bound of test_deepsdfmesh_volume_derivative, for both gradients
    from analysis.geometry import CLIP, STRETCH
    dm = so.geometry
    T, ds, n_terms, parts, Tabs = _structure_oracle(dm)
    n64 = dm.volume_normals().cpu().numpy().astype(np.float64)
    nn = (n64 * n64).sum(1)
    v = dm.volume_diff
    normals = dm.volume_normals()
    cut = v.dtheta_moving(normals, STRETCH, CLIP).cpu().numpy().astype(np.float64)
    free = v.dtheta_moving(normals, STRETCH, 0.0).cpu().numpy().astype(np.float64)
    mvi = v.moving.cpu().numpy()
    print(f"driver: {int((cut != free).sum())} entries of the dense dTheta clipped")
    for what, g, a, d in (("compliance", so.problem.ElasticitySolver.compliance_shape_gradient("mean"), dcomp, dcomp_d),
                          ("volume", so.problem.ElasticitySolver.volume_shape_gradient(), dvol, dvol_d)):
        g64 = g.cpu().numpy().astype(np.float64)
        # the dense route zeroes the entries outside [-CLIP, CLIP], the adjoint cannot: what they contribute is added back exactly
        d = d + (g64[mvi][:, :, None] * (free - cut)).sum((0, 1))
        proj = np.where(nn > 0, np.abs(g64 * n64).sum(1) * np.abs(n64 * ds).sum(1) / np.where(nn > 0, nn, 1.0), 0.0)
        mag = (proj[:, None, None] * Tabs).sum(0)
        bound = (n_terms[:, None] + parts + 11 + 10 + 19) * vd.U * mag
        ratio = float(np.nanmax(np.where(mag > 0, np.abs(a.reshape(mag.shape) - d.reshape(mag.shape)) / np.where(mag > 0, bound, 1.0), 0.0)))
        print(f"driver: {what} gradient, dense against adjoint, worst difference / bound {ratio:.3f}")
        assert ratio <= 1 and np.abs(a).max() > 0
    cfg["optimization"]["method"] = "MMA"
    json.dump(cfg, open(tmp_path / "dense" / "config.json", "w"))
    with pytest.raises(NotImplementedError, match="mmapy"):
        struct_optimization(tmp_path / "dense").run_optimization()
    cfg["optimization"]["method"] = "SGD"
    json.dump(cfg, open(tmp_path / "dense" / "config.json", "w"))
    with pytest.raises(ValueError, match="not one of"):
        struct_optimization(tmp_path / "dense")
    del cfg["general"]
    json.dump(cfg, open(tmp_path / "dense" / "config.json", "w"))
    with pytest.raises(KeyError):
        struct_optimization(tmp_path / "dense")
