"""-m gpu: the exact discrete compliance gradient (dsdf_fem_stiffness_gradient / dsdf_fem_load_gradient, csrc/fem.hpp,
LinearElasticity.stiffness_gradient / load_gradient / compliance_discrete_gradient) against the fp64 oracle of tests/femgrad_numpy.py
entry by entry at bounds counted in DESIGN 4.21.6, against a central difference of the device's own compliance, determinism, the
entries under red zones and poison, and the chain through CantileverBeam and struct_optimization to the control points."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from deepsdf_amd import _lib
from tests import fem_numpy as F
from tests import femgrad_numpy as FG
from tests import ws_guard as G
from tests.test_gpu_fem import LAM, MU, TRACTION, Case, _within

pytestmark = pytest.mark.gpu

U = F.U
NAMES = ("one tet", "2x2x2", "3x3x3", "cut", "degenerate")
# Roundings between a term and the value compared, kernel + oracle.  The stored gradients are the oracle's bits: 0.
C_E = 2 * 26                 # emt: the w term: w 24 (4.21.3), the subtraction, V * ; the H^T S terms take 19


def c_gk(nc):
    return 2 * (26 + 3 + nc)     # gK: emt's 26, the product with g_a, two additions of the row, nc additions over the corners


def c_gl(nfc):
    return 2 * (9 + nfc)         # gL: c_f 6 (two additions of u~, the product, two additions, / 3), the cross product 2, c_f * 1, nfc
                                 # additions over the faces; N, |N|, n^ and the edges are single-rounded in the oracle's order: 0


H = 1e-4
FD_MARGIN = 10.0             # the margin of the existing solve tests (test_gpu_fem.py: ten times what the oracle leaves)


class Solved:
    """A case of test_gpu_fem.py with attribute 1 clamped and TRACTION on attribute 2 (3 where no face carries 2), solved once."""

    def __init__(self, case):
        self.c = c = case
        self.loaded = 2 if (c.attr == 2).any() else 3
        self.sel = c.attr == self.loaded
        self.mask = c.mask(True)
        self.s = c.solver(True).add_traction(self.loaded, TRACTION)
        self.s.solve()
        self.u = self.s.u.cpu().numpy()
        self.N = F.face_normals(c.v, c.bf)
        self.flat = (self.N == 0).all(1)


@pytest.fixture(scope="module")
def cases():
    from deepsdf_amd.mesh import TetMesh, tetrahedralize
    cuda = lambda g: torch.from_numpy(g).cuda()                   # noqa: E731
    out = {"one tet": Case("one tet", TetMesh(*F.ONE_TET).to("cuda")),
           "2x2x2": Case("2x2x2", tetrahedralize(cuda(F.inside_grid(2)))),
           "3x3x3": Case("3x3x3", tetrahedralize(cuda(F.inside_grid(3)))),
           "cut": Case("cut", tetrahedralize(cuda(F.random_grid()), t_clamp=0.05)),
           "degenerate": Case("degenerate", tetrahedralize(cuda(F.degenerate_grid())))}
    assert out["cut"].nv > 2 * 256 and len(out["cut"].t) > 2 * 256              # several workgroups of vertices and of elements
    out = {k: Solved(c) for k, c in out.items()}
    d = out["degenerate"]
    assert d.c.skipped.sum() == 53 and d.flat.sum() == 44 and (d.flat & d.sel).sum() == 1 and not out["cut"].c.skipped.any()
    return out


def _load_gradient(s, sel, u):
    """dsdf_fem_load_gradient for one selection [M] bool through the C entry (the class sums over its own tractions)."""
    sel_t = torch.from_numpy(np.asarray(sel, dtype=np.uint8)).cuda()
    g = torch.empty(s.nv, 3, dtype=torch.float64, device="cuda")
    _lib.check(_lib.lib().dsdf_fem_load_gradient(*s._boundary_args(), G.ptr(sel_t), (C.c_double * 3)(*TRACTION), G.ptr(s.mask), G.ptr(u),
                                                 G.ptr(g), G.stream()))
    return g.cpu().numpy()


# ---- 1. values against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["solved", "random"])
@pytest.mark.parametrize("name", NAMES)
def test_values_entry_by_entry_against_the_counted_bounds(cases, name, field):
    k = cases[name]
    c, s = k.c, k.s
    u = k.u if field == "solved" else np.random.default_rng(23).standard_normal((c.nv, 3))        # random: nonzero at masked vertices too
    assert np.isfinite(u).all() and np.abs(u).max() > 0
    ut = torch.from_numpy(u).cuda()
    gK, emt = s.stiffness_gradient(ut)
    gL = s.load_gradient(ut)
    gK, emt, gL = gK.cpu().numpy(), emt.cpu().numpy(), gL.cpu().numpy()
    assert emt.shape == (9, len(c.t)) and gK.shape == gL.shape == (c.nv, 3)
    tag = f"{name} {field} u"
    _within(f"emt {tag}", emt, FG.emt(c.v, c.t, c.lam, c.mu, u), C_E * U * FG.emt(c.v, c.t, c.lam, c.mu, u, absolute=True))
    _within(f"gK {tag}", gK, FG.stiffness_gradient(c.v, c.t, c.lam, c.mu, u),
            c_gk(c.nc) * U * FG.stiffness_gradient(c.v, c.t, c.lam, c.mu, u, absolute=True))
    _within(f"gL {tag}", gL, FG.load_gradient(c.v, c.bf, k.sel, TRACTION, k.mask, u),
            c_gl(c.nfc) * U * FG.load_gradient(c.v, c.bf, k.sel, TRACTION, k.mask, u, absolute=True))
    assert np.abs(gK).max() > 0 and np.abs(gL).max() > 0
    # skipped elements and zero-area faces: exact zeros
    assert not emt[:, c.skipped].any() and emt[:, ~c.skipped].any()
    if k.flat.any():
        assert not _load_gradient(s, k.flat, ut).any()
        assert np.array_equal(_load_gradient(s, k.sel, ut), _load_gradient(s, k.sel & ~k.flat, ut)) and np.array_equal(_load_gradient(s, k.sel, ut), gL)
    if field == "solved":
        gC = s.compliance_discrete_gradient().cpu().numpy()
        assert np.array_equal(gC, gK + 2.0 * gL)


# ---- 2. central difference on the device ----------------------------------------------------------------------------------------------
def _device_pi(k, X):
    """Pi = 2 work() - compliance() of the device's solve on the fp64 vertices X, attributes from the unperturbed mesh: second-order
    accurate in the CG error."""
    from deepsdf_amd.fem import LinearElasticity
    from deepsdf_amd.mesh import TetMesh
    c = k.c
    m = TetMesh(torch.from_numpy(X), c.mesh.tets.cpu(), c.mesh.bfaces.cpu(), c.mesh.bface_kind.cpu()).to("cuda")
    s = LinearElasticity(m, c.lam, c.mu, attributes=c.attr)
    s.fix_faces(1).add_traction(k.loaded, TRACTION)
    assert s.verts.dtype == torch.float64 and np.array_equal(s.verts.cpu().numpy(), X)
    it, conv, _ = s.solve(rel_tol=1e-12)
    assert conv
    return 2.0 * s.work() - s.compliance()


_oracle = {}


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["3x3x3", "cut"])
def test_central_difference_of_the_devices_own_compliance(cases, name, seed):
    k = cases[name]
    c = k.c
    X = c.v.astype(np.float64)
    th = FG.theta(c.nv, seed)
    if name not in _oracle:                                      # the oracle's problem and gradient: once per mesh, never changed
        p = FG.Problem((c.v, c.t, c.bf, None), c.lam, c.mu)
        assert np.array_equal(p.mask, k.mask) and np.array_equal(p.sel, k.sel)
        _oracle[name] = (p, p.gradient())
    p, g_exact = _oracle[name]
    fd_np = FG.central_difference(p.pi, X, th, H)
    ratio_np = FG.fd_error(fd_np, g_exact, g_exact, th)
    s = c.solver(True).add_traction(k.loaded, TRACTION)
    assert s.solve(rel_tol=1e-12)[1]
    g = s.compliance_discrete_gradient().cpu().numpy()
    ratio = FG.fd_error(FG.central_difference(lambda Y: _device_pi(k, Y), X, th, H), g, g_exact, th)
    print(f"{name} seed {seed} h {H:g}: |fd - g . theta| / sum |g . theta| GPU {ratio:.3e} / oracle {ratio_np:.3e}")
    assert ratio <= FD_MARGIN * ratio_np
    # the boundary formula on the same difference, for scale
    gb = s.compliance_shape_gradient("mean").cpu().numpy()
    assert FG.fd_error(fd_np, gb, g_exact, th) > 1000.0 * ratio_np


def test_central_difference_of_the_volume(cases):
    from deepsdf_amd.fem import LinearElasticity
    from deepsdf_amd.mesh import TetMesh
    k = cases["cut"]
    c = k.c
    X = c.v.astype(np.float64)

    def vol_np(Y):
        return float(F.geometry(Y, c.t)[0][9].sum())

    def vol_gpu(Y):
        m = TetMesh(torch.from_numpy(Y), c.mesh.tets.cpu(), c.mesh.bfaces.cpu(), c.mesh.bface_kind.cpu()).to("cuda")
        return LinearElasticity(m, c.lam, c.mu, attributes=c.attr).volume()
    g_exact = F.boundary_gradient(X, c.bf)
    g = k.s.volume_shape_gradient().cpu().numpy()
    for seed in range(4):
        th = FG.theta(c.nv, seed)
        ratio_np = FG.fd_error(FG.central_difference(vol_np, X, th, H), g_exact, g_exact, th)
        ratio = FG.fd_error(FG.central_difference(vol_gpu, X, th, H), g, g_exact, th)
        print(f"volume, cut seed {seed} h {H:g}: GPU {ratio:.3e} / oracle {ratio_np:.3e}")
        assert ratio <= FD_MARGIN * ratio_np


# ---- 3. robustness ----------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes(cases):
    for name in ("cut", "degenerate"):
        s = cases[name].s
        a, b = s.stiffness_gradient(), s.stiffness_gradient()
        assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes()
        assert s.load_gradient().cpu().numpy().tobytes() == s.load_gradient().cpu().numpy().tobytes()
        assert s.compliance_discrete_gradient().cpu().numpy().tobytes() == s.compliance_discrete_gradient().cpu().numpy().tobytes()


def test_entries_under_red_zones_and_poison(cases):
    lib = _lib.lib()
    k = cases["cut"]
    c, s = k.c, k.s
    nt, nv = len(c.t), c.nv
    u = torch.from_numpy(np.random.default_rng(9).standard_normal((nv, 3))).cuda()
    sel = torch.from_numpy(k.sel.astype(np.uint8)).cuda()
    with G.redzone():
        outs = []
        for fill in (0x00, 0xFF):
            b = C.c_size_t()
            _lib.check(lib.dsdf_fem_plan(nv, nt, len(c.bf), C.byref(b)))
            ws, Fn = G.poisoned(b.value, fill), G.Fences()
            o = dict(emt=Fn.new("emt", (9, nt), torch.float64), gK=Fn.new("gK", (nv, 3), torch.float64), gL=Fn.new("gL", (nv, 3), torch.float64))
            op = s._op()
            _lib.check(lib.dsdf_fem_stiffness_gradient(C.byref(op), G.ptr(u), G.ptr(o["emt"]), G.ptr(o["gK"]), G.ptr(ws), ws.numel(), G.stream()))
            rows, _ = G.assert_clean(ws, fill, f"fem stiffness gradient fill {fill:#x}")
            assert {r[0] for r in rows} == {"fem_sigma", "fem_r", "fem_z", "fem_p", "fem_ap", "fem_part0", "fem_part1", "fem_cnt", "fem_scal"}
            assert bool((ws == fill).all())                     # emt is the caller's: the entry writes nothing into the workspace
            _lib.check(lib.dsdf_fem_load_gradient(*s._boundary_args(), G.ptr(sel), (C.c_double * 3)(*TRACTION), G.ptr(s.mask), G.ptr(u),
                                                  G.ptr(o["gL"]), G.stream()))
            Fn.check(f"fem gradient fill {fill:#x}")
            outs.append({n: t.cpu().numpy().tobytes() for n, t in o.items()})
        assert outs[0] == outs[1]                                # nothing read a byte it had not written
    assert all(np.frombuffer(v, dtype=np.float64).std() > 0 for v in outs[0].values())
    assert outs[0]["gK"] == s.stiffness_gradient(u)[0].cpu().numpy().tobytes()


# ---- 4. the chain through the driver ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """{name: (struct_optimization, compliance, d compliance, constraint, d volume)} on the tiny experiment of the existing driver
    test: general.gradient absent, "boundary" and "discrete"; one evaluation each."""
    from deepsdf_amd.mesh import default_cap_border_dict
    from optimization.opti import struct_optimization
    from tests.test_gpu_microstructure import _tiny_experiment
    root = tmp_path_factory.mktemp("femgrad")
    exp = _tiny_experiment(str(root))
    mesh = dict(experiment_directory=exp, checkpoint="latest", degrees=[1, 1, 1], refinement=1, cap_border_dict=default_cap_border_dict(),
                N_base_reconstruction=4, tiling=[2, 1, 1], remove_orphans=True)
    runs = {"root": root, "mesh": mesh}
    for name in ("absent", "boundary", "discrete"):
        folder = root / name
        folder.mkdir()
        general = dict(volume_constraint=0.5, t_clamp=0.05)
        if name != "absent":
            general["gradient"] = name
        json.dump(dict(mesh=mesh, optimization=dict(method="COBYLA", maxiter=1), general=general), open(folder / "config.json", "w"))
        so = struct_optimization(folder)
        so.set_x0()
        x = np.tile(so.geometry.latent[0], 27).astype(np.float64)
        comp, dcomp = so.objective(x)
        cons, dvol = so.constraint(x)
        assert so.iteration == 1
        runs[name] = (so, comp, dcomp, cons, dvol)
    return runs


def test_boundary_is_the_default_and_gives_todays_bytes(driver):
    (so, comp, dcomp, cons, dvol), (sb, comp_b, dcomp_b, cons_b, dvol_b) = driver["absent"], driver["boundary"]
    assert comp == comp_b and cons == cons_b and dcomp.tobytes() == dcomp_b.tobytes() and dvol.tobytes() == dvol_b.tobytes()
    s, geo = so.problem.ElasticitySolver, so.geometry
    assert dcomp.tobytes() == geo.shape_gradient(s.compliance_shape_gradient("mean")).double().reshape(-1).cpu().numpy().tobytes()
    assert dvol.tobytes() == geo.shape_gradient(s.volume_shape_gradient()).double().reshape(-1).cpu().numpy().tobytes()


def test_discrete_is_the_unprojected_adjoint_of_the_exact_vertex_gradient(driver):
    from analysis.geometry import STRETCH
    from tests import voldiff_numpy as vd
    so, comp, dcomp, cons, dvol = driver["discrete"]
    assert comp == driver["absent"][1] and cons == driver["absent"][3]
    s, geo = so.problem.ElasticitySolver, so.geometry
    gC = s.compliance_discrete_gradient()
    assert dcomp.dtype == np.float64 and dcomp.shape == (108,)
    assert dcomp.tobytes() == geo.shape_gradient(gC, project=False).double().reshape(-1).cpu().numpy().tobytes()
    assert dvol.tobytes() == geo.shape_gradient(s.volume_shape_gradient(), project=False).double().reshape(-1).cpu().numpy().tobytes()
    assert dcomp.tobytes() != driver["absent"][2].tobytes() and np.abs(dcomp).max() > 0
    # grad . d against sum gC . dX with dX = STRETCH * jvp(d): the adjoint and the tangent of one Jacobian.  The bound is that of
    # test_gpu_voldiff.py's test_volume_jacobian_and_memory_guard, (2 Vm + parts + 11 + 16) 2^-24 sum |terms|, on the operand the
    # adjoint receives (gC in fp32 times the stretch)
    v = geo.volume_diff
    ncp, L = v.n_control_points, v.latent_size
    d = torch.randn(ncp, L, generator=torch.Generator().manual_seed(6)).cuda()
    stretch = torch.tensor(STRETCH, dtype=torch.float32, device=d.device)
    dX = (v.jvp(d) * stretch).double()
    jac =v.jacobian().double()                                                                # [V, 3, ncp, L], unstretched
    for what, gv, grad in (("compliance", gC, dcomp), ("volume", s.volume_shape_gradient(), dvol)):
        g32 = gv.float() * stretch
        mag = float((g32.double().abs()[:, :, None, None] * jac.abs() * d.double().abs()[None, None]).sum())
        bound = (2 * v.moving.numel() + v.vjp_plan()[1] + 11 + 16) * vd.U * mag
        lhs = float((torch.from_numpy(grad).cuda() * d.double().reshape(-1)).sum())
        rhs = float((gv * dX).sum())
        print(f"driver, discrete {what}: grad . d {lhs!r}, sum g . dX {rhs!r}, |difference| / bound {abs(lhs - rhs) / bound:.3e}")
        assert abs(lhs - rhs) <= bound and abs(rhs) > 0


def test_gradient_setting_errors(driver):
    from optimization.opti import struct_optimization
    folder = driver["root"] / "errors"
    folder.mkdir()
    for general, word in ((dict(gradient="discrete", dense_dtheta=True), "dense_dtheta"), (dict(gradient="exact"), "not one of"),
                          (dict(gradient=None), "not one of")):
        cfg = dict(mesh=driver["mesh"], optimization=dict(method="COBYLA", maxiter=1), general=dict(volume_constraint=0.5, **general))
        json.dump(cfg, open(folder / "config.json", "w"))
        with pytest.raises(ValueError, match=word):
            struct_optimization(folder)
    cfg["general"] = dict(volume_constraint=0.5, gradient="boundary", dense_dtheta=True)             # the reference's route stays
    json.dump(cfg, open(folder / "config.json", "w"))
    struct_optimization(folder)
