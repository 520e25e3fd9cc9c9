"""-m gpu: the HIP elasticity solver (dsdf_fem_*, csrc/fem.hpp, deepsdf_amd/fem.py) against the fp64 oracle of tests/fem_numpy.py:
the operator row by row against a counted rounding bound, the set-up, the load, the solve against spsolve and the oracle's own PCG,
determinism, every post-processing quantity, the errors, the workspace under red zones and poison, and CantileverBeam end to end.
Every bound is derived in DESIGN 4.21.3 from the roundings counted there; tests/test_fem_cpu.py shows that each wrong variant misses
the truth by more than 1e9 times these bounds."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from deepsdf_amd import _lib
from tests import fem_numpy as F
from tests import ws_guard as G

pytestmark = pytest.mark.gpu

LAM, MU = 0.7, 1.3
U = F.U
TRACTION = (0.0, 0.0, -0.01)
SMALL = ("one tet", "2x2x2", "3x3x3", "cut", "degenerate")
ALL = SMALL + ("large",)
C_W = 48                     # roundings of w_e, kernel + oracle


def large_n():
    """The smallest all-inside grid whose vertex partials (one per FEM_BLOCK vertices) outnumber the FEM_BLOCK lanes of the final
    pass, so that a lane of it adds more than one: n^3 > FEM_BLOCK^2 = 65536, n = 41 (270 partials; 1500 for its elements)."""
    b = G.constants()["FEM_BLOCK"]
    n = 2
    while -(-n ** 3 // b) <= b:
        n += 1
    assert n == 41 and b == 256
    return n


class Case:
    """A device mesh, its host arrays, and what the oracle says about it (computed once, never changed)."""

    def __init__(self, name, mesh, attributes=None, lam=LAM, mu=MU, assemble=True):
        self.name, self.mesh, self.lam, self.mu = name, mesh, lam, mu
        self.v = mesh.verts.cpu().numpy()
        self.t, self.bf = mesh.tets.cpu().numpy(), mesh.bfaces.cpu().numpy()
        self.nv = len(self.v)
        self.attr = F.attributes(self.v, self.bf) if attributes is None else np.asarray(attributes, dtype=np.int32)
        self.geom, self.skipped = F.geometry(self.v, self.t)
        self.held = F.held_vertices(self.t, self.skipped, self.nv)
        self.fixed = F.fixed_vertices(self.bf, self.attr == 1, self.nv)
        self.nc = int(F.corner_counts(self.t, self.nv).max())
        self.nfc = int(F.corner_counts(self.bf, self.nv).max())
        self.K = F.assemble(self.v, self.t, lam, mu) if assemble else None
        self.Kabs = F.assemble(self.v, self.t, lam, mu, absolute=True) if assemble else None

    def mask(self, fixed):
        return self.held | self.fixed if fixed else self.held.copy()

    def solver(self, fixed=True):
        from deepsdf_amd.fem import LinearElasticity
        s = LinearElasticity(self.mesh, self.lam, self.mu, attributes=self.attr)
        if fixed:
            s.fix_faces(1)
        return s


@pytest.fixture(scope="module")
def cases():
    from deepsdf_amd.mesh import TetMesh, tetrahedralize
    cuda = lambda g: torch.from_numpy(g).cuda()
    out = {"one tet": Case("one tet", TetMesh(*F.ONE_TET).to("cuda")),
           "2x2x2": Case("2x2x2", tetrahedralize(cuda(F.inside_grid(2)))),
           "3x3x3": Case("3x3x3", tetrahedralize(cuda(F.inside_grid(3)))),
           "cut": Case("cut", tetrahedralize(cuda(F.random_grid()), t_clamp=0.05)),
           "degenerate": Case("degenerate", tetrahedralize(cuda(F.degenerate_grid()))),
           "large": Case("large", tetrahedralize(cuda(F.inside_grid(large_n()))), assemble=False)}
    assert out["degenerate"].skipped.sum() > 0 and not out["cut"].skipped.any()
    # the device mesh of the tied grid is the numpy mesher's, array for array and bit for bit: the zero-volume elements the solver
    # skips are the specification's, not an accident of the kernel's
    from tests import tet_numpy
    want, got = tet_numpy.tetrahedralize(F.degenerate_grid()), out["degenerate"]
    assert got.t.shape == want.tets.shape and np.array_equal(got.t, want.tets)
    assert got.bf.shape == want.bfaces.shape and np.array_equal(got.bf, want.bfaces)
    assert np.array_equal(got.mesh.bface_kind.cpu().numpy(), want.bface_kind)
    assert got.v.dtype == np.float32 and got.v.shape == want.verts.shape and got.v.tobytes() == want.verts.tobytes()
    assert (tet_numpy.volumes(want.verts, want.tets) == 0).sum() > 0
    assert out["cut"].nv > 2 * 256 and len(out["cut"].t) > 2 * 256          # several workgroups of vertices and of elements
    return out


def _within(what, got, ref, bound):
    got, ref, bound = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (got, ref, bound))
    assert np.isfinite(got).all(), what
    ratio = np.abs(got - ref) / np.maximum(bound, 1e-300)
    worst = float(np.where(np.abs(got - ref) == 0.0, 0.0, ratio).max()) if len(got) else 0.0
    print(f"{what}: worst |difference| / bound = {worst:.3e} over {len(got)} values")
    assert worst <= 1.0, (what, worst)


# ---- 1. the operator ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
@pytest.mark.parametrize("name", ALL)
def test_apply_row_by_row_against_the_counted_bound(cases, name, fixed):
    c = cases[name]
    s = c.solver(fixed)
    x = np.random.default_rng(21).standard_normal((c.nv, 3))
    y = s.apply(torch.from_numpy(x).cuda()).cpu().numpy()
    mask = c.mask(fixed)
    assert np.array_equal(s.mask.cpu().numpy().astype(bool), mask)
    if c.K is not None:
        A = F.masked(c.K, mask)
        ref = A @ x.reshape(-1)
        bound = F.apply_bound_c(c.nc, int(np.diff(A.indptr).max())) * U * (F.masked(c.Kabs, mask) @ np.abs(x).reshape(-1))
    else:           # the large grid: assembling 55 M entries takes longer than a test may; the oracle's element-by-element operator
        ref = F.apply_free(c.v, c.t, c.lam, c.mu, mask, x)
        bound = F.apply_bound_c(c.nc) * U * F.apply_free(c.v, c.t, c.lam, c.mu, mask, x, absolute=True)
    _within(f"apply {name} fixed={fixed}", y, ref, bound)
    assert np.array_equal(y.reshape(-1, 3)[mask], x[mask])             # (I - P): the masked rows pass x through


# ---- 2. set-up and load -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_setup_geometry_counts_and_preconditioner(cases, name):
    c = cases[name]
    s = c.solver(True)
    assert (s.n_skipped_elements, s.n_held_vertices) == (int(c.skipped.sum()), int(c.held.sum()))
    geom = s.geom.cpu().numpy()
    assert np.isfinite(geom).all() and np.array_equal(geom.view(np.uint64), c.geom.view(np.uint64))     # the oracle's bits
    mask = c.mask(True)
    A, Aabs = F.masked(c.K, mask), F.masked(c.Kabs, mask)
    diag, dinv = s.diag.cpu().numpy(), s.dinv.cpu().numpy()
    _within(f"diagonal blocks {name}", diag, F.diag_blocks(A), 2 * (10 + c.nc) * U * F.diag_blocks(Aabs))
    assert np.isfinite(dinv).all()
    D, Di = F.sym3(diag), F.sym3(dinv)
    res = np.abs(np.einsum("vij,vjk->vik", Di, D) - np.eye(3)).max((1, 2))
    cond = np.linalg.cond(D)
    print(f"block inverses {name}: worst residual / (64 u cond) = {(res / (64 * U * cond)).max():.3e}")
    assert (res <= 64 * U * cond).all()
    assert (Di[mask] == np.eye(3)).all() and (D[mask] == np.eye(3)).all()


@pytest.mark.parametrize("name", ALL)
def test_load_against_the_oracle(cases, name):
    c = cases[name]
    s = c.solver(True)
    s.add_traction(2, TRACTION)
    extra = np.random.default_rng(3).standard_normal((c.nv, 3))
    mask = c.mask(True)
    f0 = s.load().cpu().numpy()
    ref = F.load(c.v, c.bf, c.attr == 2, TRACTION, mask)
    cl = 2 * (7 + c.nfc)
    _within(f"load {name}", f0, ref, cl * U * np.abs(ref))
    total = F.load(c.v, c.bf, c.attr == 2, TRACTION).sum(0)
    n = F.face_normals(c.v, c.bf)[c.attr == 2]
    area = 0.5 * np.sqrt((n * n).sum(1)).sum()
    assert np.allclose(total, area * np.asarray(TRACTION), rtol=1e-12, atol=0)                         # total load = t x loaded area
    s.add_nodal_forces(extra)
    f1 = s.load().cpu().numpy()
    keep = ~mask
    _within(f"load + nodal forces {name}", f1, np.where(keep[:, None], ref + extra, 0.0), (cl + 1) * U * (np.abs(ref) + np.abs(extra)))
    assert (f1[mask] == 0).all()


# ---- 3. the solve -------------------------------------------------------------------------------------------------------------------
def _bar_case(n, h):
    from deepsdf_amd.mesh import tetrahedralize
    m = tetrahedralize(torch.from_numpy(F.inside_grid(n)).cuda(), spacing=(h, h, h))
    return Case(f"bar {n}", m, attributes=m.bface_kind.cpu().numpy(), lam=0.0, mu=105.0)


def _cut_solve_case():
    from deepsdf_amd.mesh import tetrahedralize
    m = tetrahedralize(torch.from_numpy(F.random_grid()).cuda(), t_clamp=0.05, keep_largest=True)
    c = Case("cut, largest component", m, attributes=F.reference_attributes(m.verts.cpu().numpy(), m.bfaces.cpu().numpy()))
    assert c.fixed.sum() > 10 and (c.attr == 2).sum() > 10 and not c.held.any()
    return c


SOLVE = {"bar 3": (lambda: _bar_case(3, 0.5), (0.3, 0.0, 0.0)), "bar 7": (lambda: _bar_case(7, 0.25), (0.3, 0.0, 0.0)),
         "cut": (_cut_solve_case, TRACTION)}


@pytest.fixture(scope="module")
def solved():
    """{name: (case, solver after solve(), (iterations, converged, ratio), oracle dict)}: one solve and one oracle per mesh."""
    out = {}
    for name, (make, trac) in SOLVE.items():
        c = make()
        s = c.solver(True).add_traction(2, trac)
        res = s.solve()
        mask = c.mask(True)
        A = F.masked(c.K, mask)
        f = F.load(c.v, c.bf, c.attr == 2, trac, mask)
        d = F.diag_blocks(A)
        Dinv = F.block_inverse(d)
        u_np, it_np, conv_np, _ = F.pcg(A, Dinv, f)
        ref = F.spsolve(A, f)
        o = dict(A=A, f=f, Dinv=Dinv, ref=ref, it_np=it_np, conv_np=conv_np, res_np=F.true_residual(A, Dinv, f, u_np),
                 dist_np=F.energy_distance(A, u_np, ref), kappa=F.kappa(A, d), trac=trac)
        out[name] = (c, s, res, o)
    return out


def _solver_tolerance(o, rel_tol=1e-10):
    """Relative energy-norm error a converged solve may leave: ||e||_A / ||u||_A <= sqrt(kappa(D^-1 A) * true residual ratio), and the
    true ratio is allowed ten times rel_tol^2 (below); 1e-12 for the rounding of the oracle's own solve."""
    return math.sqrt(10.0 * o["kappa"]) * rel_tol + 1e-12


@pytest.mark.parametrize("name", list(SOLVE))
def test_solve_against_spsolve_and_the_oracles_own_pcg(solved, name):
    c, s, (it, conv, ratio), o = solved[name]
    u = s.u.cpu().numpy()
    assert conv and o["conv_np"] and it <= 10000 and ratio <= 1e-20 and np.isfinite(u).all()
    res = F.true_residual(o["A"], o["Dinv"], o["f"], u)
    dist = F.energy_distance(o["A"], u, o["ref"])
    print(f"{name}: iterations GPU {it} / numpy {o['it_np']}; true preconditioned residual GPU {res:.3e} / numpy {o['res_np']:.3e}; "
          f"energy-norm distance from spsolve GPU {dist:.3e} / numpy {o['dist_np']:.3e}; kappa {o['kappa']:.1f}")
    assert res <= 10.0 * o["res_np"]
    assert dist <= 10.0 * o["dist_np"]
    assert (u[c.mask(True)] == 0).all()
    tol = _solver_tolerance(o)
    work, comp = s.work(), s.compliance()
    print(f"{name}: work {work!r}, compliance {comp!r}, solver tolerance {tol:.3e}")
    assert abs(work - comp) <= 3 * tol * abs(comp)
    if name.startswith("bar"):
        t, mu = o["trac"][0], c.mu
        exact = np.zeros_like(u)
        exact[:, 0] = t * c.v[:, 0].astype(np.float64) / (2 * mu)
        assert F.energy_distance(o["A"], u, exact) <= tol
        L = float(c.v[:, 0].max())
        assert abs(comp - t * t * L * L * L / (2 * mu)) <= 3 * tol * comp


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------
def test_two_solves_and_any_check_every_give_identical_bytes(solved):
    c, s, (it, conv, ratio), o = solved["cut"]
    first = s.u.cpu().numpy().tobytes()
    for kw in (dict(), dict(check_every=1), dict(check_every=10 ** 6)):
        s2 = c.solver(True).add_traction(2, o["trac"])
        again = s2.solve(**kw)
        assert again == (it, conv, ratio), (kw, again)
        assert s2.u.cpu().numpy().tobytes() == first, kw
    assert it > 32                   # the default check_every met the flag late: the frozen state is what came back


# ---- 5. after the solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_post_processing_against_the_oracle_on_the_gpus_own_u(cases, name):
    c = cases[name]
    s = c.solver(True).add_traction(2, TRACTION)
    s.solve(max_iter=20)                        # any displacement serves: the oracle gets the GPU's own
    u = s.u.cpu().numpy()
    assert np.isfinite(u).all() and np.abs(u).max() > 0
    w, V = F.energy_density(c.v, c.t, c.lam, c.mu, u)
    wabs = F.energy_density(c.v, c.t, c.lam, c.mu, u, absolute=True)[0]
    nt = len(c.t)
    _within(f"w per element {name}", s.strain_energy_density().cpu().numpy(), w, C_W * U * wabs)
    mean_abs = F.nodal_density(c.t, wabs, V, c.nv, "mean")
    last_abs = F.nodal_density(c.t, wabs, V, c.nv, "last")
    c_mean = C_W + 2 * (2 + 2 * c.nc)
    wv = {"mean": s.strain_energy_density("mean").cpu().numpy(), "last": s.strain_energy_density("last").cpu().numpy()}
    _within(f"nodal mean {name}", wv["mean"], F.nodal_density(c.t, w, V, c.nv, "mean"), c_mean * U * mean_abs)
    _within(f"nodal last {name}", wv["last"], F.nodal_density(c.t, w, V, c.nv, "last"), C_W * U * last_abs)
    cs = F.sum_roundings(nt)
    _within(f"compliance {name}", s.compliance(), (V * w).sum(), (C_W + 1 + cs) * U * (V * wabs).sum())
    _within(f"volume {name}", s.volume(), V.sum(), cs * U * V.sum())
    gabs = F.boundary_gradient(c.v, c.bf, absolute=True)
    c_g = 2 * c.nfc + 2
    gv = s.volume_shape_gradient().cpu().numpy()
    _within(f"volume shape gradient {name}", gv, F.boundary_gradient(c.v, c.bf), c_g * U * gabs)
    for mode, wabs_v, cw in (("mean", mean_abs, c_mean), ("last", last_abs, C_W)):
        ref = F.boundary_gradient(c.v, c.bf, weight=-F.nodal_density(c.t, w, V, c.nv, mode))
        _within(f"compliance shape gradient {mode} {name}", s.compliance_shape_gradient(mode).cpu().numpy(), ref,
                (cw + c_g + 2) * U * wabs_v[:, None] * gabs)
    # a closed boundary: the gradients of the volume sum to zero, up to the rounding of their terms
    assert (np.abs(gv.sum(0)) <= (c_g + F.sum_roundings(c.nv)) * U * gabs.sum(0)).all()
    # ... and are the surface stage's d volume / d vertex on the same ids, to that kernel's fp32 accuracy: its vertices and its output
    # are fp32, so each of the two factors of a term b x c / 6 and the result carry 2^-24: 3 * 2^-24 <= 2^-22 of sum |b| |c| / 6
    g32 = c.mesh.boundary_surface().volume_vertex_gradient().cpu().numpy().astype(np.float64)
    x = c.v.astype(np.float32).astype(np.float64)[c.bf.astype(np.int64)]
    S = np.zeros(c.nv)
    for k in range(3):
        np.add.at(S, c.bf[:, k].astype(np.int64), np.linalg.norm(x[:, (k + 1) % 3], axis=1) * np.linalg.norm(x[:, (k + 2) % 3], axis=1) / 6.0)
    assert (np.abs(gv - g32) <= 2.0 ** -22 * S[:, None]).all()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def test_errors(cases, solved, tmp_path):
    c = cases["cut"]
    with pytest.raises(ValueError, match="fixed"):
        c.solver(False).add_traction(2, TRACTION).solve()
    cs = solved["cut"][0]
    s = cs.solver(True).add_traction(2, TRACTION)
    it, conv, ratio = s.solve(max_iter=3)
    assert (it, conv) == (3, False) and ratio > 1e-20 and bool(torch.isfinite(s.u).all())
    with pytest.raises(ValueError):
        s.add_nodal_forces(np.zeros((cs.nv + 1, 3)))
    with pytest.raises(ValueError):
        s.strain_energy_density("first")
    from analysis.problems.CantileverBeam import CantileverBeam
    cb = CantileverBeam(str(tmp_path))
    cb.set_mesh(cs.mesh)
    cb.set_up()
    cb.solve(max_iter=3)
    for shape in ((cs.nv, 3), (cs.nv + 1, 3, 2), (cs.nv, 2, 2)):
        with pytest.raises(ValueError, match="dTheta"):
            cb.compute_compliance(np.zeros(shape))
        with pytest.raises(ValueError, match="dTheta"):
            cb.compute_volume(np.zeros(shape))


# ---- 7. the workspace -----------------------------------------------------------------------------------------------------------------
def test_workspace_under_red_zones_and_poison(cases):
    lib = _lib.lib()
    c = cases["cut"]
    s = c.solver(True).add_traction(2, TRACTION)               # the tensors the calls below read
    nt, nv = len(c.t), c.nv
    names = {"fem_sigma", "fem_r", "fem_z", "fem_p", "fem_ap", "fem_part0", "fem_part1", "fem_cnt", "fem_scal"}
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((nv, 3))).cuda()
    with G.redzone():
        outs = []
        for fill in (0x00, 0xFF):
            b = C.c_size_t()
            _lib.check(lib.dsdf_fem_plan(nv, nt, len(c.bf), C.byref(b)))
            ws, Fn = G.poisoned(b.value, fill), G.Fences()
            o = dict(geom=Fn.new("geom", (10, nt), torch.float64), diag=Fn.new("diag", (nv, 6), torch.float64),
                     dinv=Fn.new("dinv", (nv, 6), torch.float64), mask=Fn.new("mask", nv, torch.uint8), counts=Fn.new("counts", 2, torch.int64),
                     y=Fn.new("y", (nv, 3), torch.float64), u=Fn.new("u", (nv, 3), torch.float64), we=Fn.new("we", nt, torch.float64),
                     wv=Fn.new("wv", nv, torch.float64), totals=Fn.new("totals", 2, torch.float64), f=Fn.new("f", (nv, 3), torch.float64),
                     g=Fn.new("g", (nv, 3), torch.float64))
            op = _lib.DsdfFemOp(s.tets.data_ptr(), s.corder.data_ptr(), s.vstart.data_ptr(), o["geom"].data_ptr(), o["dinv"].data_ptr(),
                                o["mask"].data_ptr(), nv, nt, LAM, MU)
            args = (G.ptr(ws), ws.numel(), G.stream())
            _lib.check(lib.dsdf_fem_setup(C.byref(op), G.ptr(s.verts), G.ptr(s.fixed), G.ptr(o["diag"]), G.ptr(o["counts"]), *args))
            rows, _ = G.assert_clean(ws, fill, f"fem setup fill {fill:#x}")
            assert {r[0] for r in rows} == names
            _lib.check(lib.dsdf_fem_apply(C.byref(op), G.ptr(x), G.ptr(o["y"]), *args))
            G.assert_clean(ws, fill, f"fem apply fill {fill:#x}")
            sel = (s.attributes == 2).to(torch.uint8).contiguous()
            bargs = (G.ptr(s.verts), nv, G.ptr(s.bfaces), len(c.bf), G.ptr(s.border), G.ptr(s.bvstart))
            _lib.check(lib.dsdf_fem_load(*bargs, G.ptr(sel), (C.c_double * 3)(*TRACTION), G.ptr(o["mask"]), G.ptr(o["f"]), G.stream()))
            it, conv, ratio = C.c_int32(), C.c_int32(), C.c_double()
            _lib.check(lib.dsdf_fem_solve(C.byref(op), G.ptr(o["f"]), G.ptr(o["u"]), 1e-10, 40, 7, C.byref(it), C.byref(conv), C.byref(ratio), *args))
            G.assert_clean(ws, fill, f"fem solve fill {fill:#x}")
            assert it.value == 40 and conv.value == 0
            _lib.check(lib.dsdf_fem_energy(C.byref(op), G.ptr(o["u"]), G.ptr(o["we"]), 1, G.ptr(o["wv"]), G.ptr(o["totals"]), *args))
            G.assert_clean(ws, fill, f"fem energy fill {fill:#x}")
            _lib.check(lib.dsdf_fem_boundary_gradient(*bargs, G.ptr(o["wv"]), G.ptr(o["g"]), G.stream()))
            Fn.check(f"fem fill {fill:#x}")
            outs.append({k: t.cpu().numpy().tobytes() for k, t in o.items()})
        assert outs[0] == outs[1]                                # nothing read a byte it had not written
    assert np.frombuffer(outs[0]["u"], dtype=np.float64).std() > 0


# ---- 8. end to end ----------------------------------------------------------------------------------------------------------------------
def _beam_with_holes():
    """A 2 x 0.6 x 1 beam with two holes along y, on a 21 x 5 x 11 grid: sdf < 0 in the solid."""
    x, y, z = np.meshgrid(np.linspace(0, 2, 21), np.linspace(0, 0.6, 5), np.linspace(0, 1, 11), indexing="ij")
    holes = [0.22 - np.sqrt((x - cx) ** 2 + (z - 0.5) ** 2) for cx in (0.7, 1.4)]
    return np.maximum(np.maximum(*holes), -0.5).astype(np.float32), (0.1, 0.15, 0.1)


def test_cantilever_beam_end_to_end(tmp_path):
    from analysis.problems.CantileverBeam import CantileverBeam
    from deepsdf_amd.mesh import TetMesh, tetrahedralize
    grid, spacing = _beam_with_holes()
    m32 = tetrahedralize(torch.from_numpy(grid).cuda(), spacing=spacing, t_clamp=0.05, keep_largest=True)
    m = TetMesh(m32.verts.double(), m32.tets, m32.bfaces, m32.bface_kind)       # fp64 vertices (generate_volume_mesh's): the file returns them exactly
    path = str(tmp_path / "beam.mesh")
    m.write_mfem(path)
    assert np.array_equal(TetMesh.read_mfem(path)[0].verts.numpy(), m.verts.cpu().numpy())
    nv = m.n_verts
    dTheta = np.random.default_rng(17).standard_normal((nv, 3, 3))
    routes = []
    for route in ("file", "mesh"):
        cb = CantileverBeam(str(tmp_path))
        cb.read_mesh(path) if route == "file" else cb.set_mesh(m)
        cb.set_up()
        vol, dvol = cb.compute_volume(dTheta)
        it, conv, _ = cb.solve()
        comp, dcomp = cb.compute_compliance(torch.from_numpy(dTheta))
        assert conv and dvol.shape == (3,) and dcomp.shape == (3,) and dvol.dtype == np.float64 and dcomp.dtype == np.float64
        routes.append((vol, dvol.tobytes(), comp, dcomp.tobytes(), cb.u_data.tobytes(), cb.strain_energy_density_data.tobytes()))
        none = cb.compute_volume()
        assert none[0] == vol and none[1].shape == () and none[1].item() is None
    assert routes[0] == routes[1]
    u = cb.ElasticitySolver.u.cpu().numpy()
    assert cb.u_data.shape == (3 * nv,) and np.array_equal(cb.u_data.reshape(-1, 3, order="F"), u)      # by component
    assert np.array_equal(cb.u_data[:nv], u[:, 0]) and cb.strain_energy_density_data.shape == (nv,)
    # the oracle: the reference's problem on the same arrays
    c = Case("beam", m.to("cuda"), attributes=F.reference_attributes(m.verts.cpu().numpy(), m.bfaces.cpu().numpy()), lam=0.0, mu=105.0)
    assert c.fixed.sum() > 10 and (c.attr == 2).sum() > 10 and not c.skipped.any()
    assert np.array_equal(cb.attributes.cpu().numpy(), c.attr)
    mask = c.mask(True)
    A = F.masked(c.K, mask)
    f = F.load(c.v, c.bf, c.attr == 2, TRACTION, mask)
    d = F.diag_blocks(A)
    ref = F.spsolve(A, f)
    tol = _solver_tolerance(dict(kappa=F.kappa(A, d)))
    comp_ref = float(ref.reshape(-1) @ (c.K @ ref.reshape(-1)))
    print(f"beam: {nv} vertices, {m.n_tets} elements, {it} iterations, compliance {comp!r} (spsolve {comp_ref!r}), tolerance {tol:.3e}")
    assert F.energy_distance(A, u, ref) <= tol and abs(comp - comp_ref) <= 3 * tol * comp_ref
    w, V = F.energy_density(c.v, c.t, 0.0, 105.0, u)
    wabs = F.energy_density(c.v, c.t, 0.0, 105.0, u, absolute=True)[0]
    cs = F.sum_roundings(len(c.t))
    _within("beam volume", vol, V.sum(), cs * U * V.sum())
    _within("beam compliance on the GPU's u", comp, (V * w).sum(), (C_W + 1 + cs) * U * (V * wabs).sum())
    gabs = F.boundary_gradient(c.v, c.bf, absolute=True)
    c_g, cd = 2 * c.nfc + 2, 2 * 3 * nv                 # the contraction: a product and at most 3 V - 1 additions in any order, twice
    _within("beam volume derivative", dvol, np.einsum("vi,vir->r", F.boundary_gradient(c.v, c.bf), dTheta),
            (c_g + cd) * U * np.einsum("vi,vir->r", gabs, np.abs(dTheta)))
    wv = F.nodal_density(c.t, w, V, nv, "mean")
    wv_abs = F.nodal_density(c.t, wabs, V, nv, "mean")
    _within("beam compliance derivative", dcomp, np.einsum("vi,vir->r", F.boundary_gradient(c.v, c.bf, weight=-wv), dTheta),
            (C_W + 2 * (2 + 2 * c.nc) + c_g + 2 + cd) * U * np.einsum("vi,vir->r", wv_abs[:, None] * gabs, np.abs(dTheta)))
    _within("beam nodal density", cb.strain_energy_density_data, wv, (C_W + 2 * (2 + 2 * c.nc)) * U * wv_abs)
