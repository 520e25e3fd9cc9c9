"""CPU: the oracle of the elasticity solver (tests/fem_numpy.py) proves itself -- symmetry, rigid-body motions, linear
fields, the exact bar -- the MFEM reader, the dsdf_fem_* argument checks without a device, and the discrimination of every tolerance
tests/test_gpu_fem.py and tests/test_gpu_fem_cg.py use: each wrong variant misses the truth by far more than the bound the GPU result
is held to; the spread of the CG's four restatements, and every ending of the CG reached by the oracle on the inputs the GPU tests use."""
import ctypes as C

import numpy as np
import pytest

from tests import fem_numpy as F

LAM, MU = 0.7, 1.3
U = F.U


@pytest.fixture(scope="module")
def meshes():
    return F.cpu_meshes()


def _field(verts, B, c):
    return np.asarray(verts, dtype=np.float64) @ np.asarray(B).T + np.asarray(c)


def test_k_is_symmetric_and_annihilates_rigid_motions(meshes):
    for name, (v, t, _, _) in meshes.items():
        K = F.assemble(v, t, LAM, MU)
        Kabs = F.assemble(v, t, LAM, MU, absolute=True)
        assert abs(K - K.T).max() == 0.0 or abs(K - K.T).max() <= 8 * U * abs(Kabs).max(), name
        W = np.array([[0.0, -0.3, 0.2], [0.3, 0.0, -0.5], [-0.2, 0.5, 0.0]])
        for u in (_field(v, np.zeros((3, 3)), [0.4, -1.1, 0.6]), _field(v, W, [0.0, 0.0, 0.0])):
            r = K @ u.reshape(-1)
            bound = 64 * U * (Kabs @ np.abs(u).reshape(-1))
            assert (np.abs(r) <= bound + 1e-300).all(), (name, np.abs(r).max())


def test_linear_fields_balance_inside_and_carry_the_energy_of_their_strain():
    from tests import tet_numpy
    v, t, bf, _ = F.arrays(tet_numpy.tetrahedralize(F.inside_grid(4), spacing=(0.5, 0.7, 0.9)))
    B = np.array([[0.3, -0.2, 0.1], [0.4, 0.5, -0.6], [0.2, 0.1, -0.3]])
    u = _field(v, B, [0.1, 0.2, 0.3])
    K = F.assemble(v, t, LAM, MU)
    r = (K @ u.reshape(-1)).reshape(-1, 3)
    interior = np.ones(len(v), dtype=bool)
    interior[np.asarray(bf).reshape(-1)] = False
    assert interior.sum() == 8 and np.abs(r[interior]).max() <= 1e-13 and np.abs(r[~interior]).max() > 1e-2
    eps = 0.5 * (B + B.T)
    sig = LAM * np.trace(B) * np.eye(3) + 2 * MU * eps
    w, V = F.energy_density(v, t, LAM, MU, u)
    vol = V.sum()                                                  # the fp32 vertices' box, not quite 1.5 x 2.1 x 2.7
    assert np.isclose(vol, 1.5 * 2.1 * 2.7, rtol=1e-6)
    assert np.isclose(u.reshape(-1) @ (K @ u.reshape(-1)), vol * np.sum(sig * eps), rtol=1e-12)
    assert np.allclose(w, np.sum(sig * eps), rtol=1e-12)


def _bar(n, h, t, mu):
    from tests import tet_numpy
    v, te, bf, kind = F.arrays(tet_numpy.tetrahedralize(F.inside_grid(n), spacing=(h, h, h)))
    fixed = F.fixed_vertices(bf, kind == 1, len(v))
    A = F.masked(F.assemble(v, te, 0.0, mu), fixed)
    f = F.load(v, bf, kind == 2, (t, 0.0, 0.0), fixed)
    return v, te, bf, kind, fixed, A, f


def test_the_exact_bar():
    """All-inside grid, -x clamped, traction t e_x on +x, lam = 0: u_x = t x / (2 mu) lies in the P1 space."""
    n, h, t, mu = 4, 0.25, 0.3, 105.0
    v, te, bf, kind, fixed, A, f = _bar(n, h, t, mu)
    L = (n - 1) * h
    assert np.isclose(f.sum(0)[0], t * L * L, rtol=1e-14) and np.abs(f.sum(0)[1:]).max() == 0.0       # total load = t x loaded area
    u = F.spsolve(A, f)
    exact = np.zeros_like(u)
    exact[:, 0] = t * v[:, 0].astype(np.float64) / (2 * mu)
    assert np.abs(u - exact).max() <= 1e-12 * np.abs(exact).max()
    w, V = F.energy_density(v, te, 0.0, mu, u)
    closed = t * t * L * L * L / (2 * mu)
    assert np.isclose((V * w).sum(), closed, rtol=1e-11) and np.isclose((f * u).sum(), closed, rtol=1e-11)
    Dinv = F.block_inverse(F.diag_blocks(A))
    up, it, conv, ratio = F.pcg(A, Dinv, f)
    assert conv and ratio <= 1e-20 and it < 200 and F.energy_distance(A, up, u) < 1e-8


def test_oracle_apply_without_a_matrix_is_the_matrix(meshes):
    rng = np.random.default_rng(11)
    for name, (v, t, bf, kind) in meshes.items():
        geom, skipped = F.geometry(v, t)
        mask = F.held_vertices(t, skipped, len(v)) | F.fixed_vertices(bf, F.clamped_faces(v, bf), len(v))
        x = rng.standard_normal((len(v), 3))
        A = F.masked(F.assemble(v, t, LAM, MU), mask)
        Aabs = F.masked(F.assemble(v, t, LAM, MU, absolute=True), mask)
        nc = int(F.corner_counts(t, len(v)).max())
        c = F.apply_bound_c(nc, int(np.diff(A.indptr).max()))
        bound = c * U * (Aabs @ np.abs(x).reshape(-1))
        assert (np.abs(F.apply_free(v, t, LAM, MU, mask, x).reshape(-1) - A @ x.reshape(-1)) <= bound).all(), name
        ab = F.apply_free(v, t, LAM, MU, mask, x, absolute=True).reshape(-1)
        assert np.allclose(ab, Aabs @ np.abs(x).reshape(-1), rtol=1e-12), name
    assert skipped.sum() > 0 and mask.sum() > 0                         # the last mesh: zero-volume elements


def test_zero_volume_elements_are_skipped_and_counted(meshes):
    v, t, bf, _ = meshes["degenerate"]
    geom, skipped = F.geometry(v, t)
    assert 0 < skipped.sum() < len(t) and np.isfinite(geom).all() and (geom[:, skipped] == 0).all()
    assert not F.geometry(*meshes["cut"][:2])[1].any()


def test_read_mfem_returns_what_write_mfem_wrote(meshes, tmp_path):
    from deepsdf_amd.mesh import TetMesh
    v, t, bf, kind = meshes["cut"]
    attr = F.reference_attributes(v, bf)
    for verts in (v, v.astype(np.float64) * (1 + 2.0 ** -30)):                 # fp32 digits and fp64 digits
        path = str(tmp_path / "m.mesh")
        TetMesh(verts, t, bf, kind).write_mfem(path, attributes=attr)
        m, a = TetMesh.read_mfem(path)
        assert m.verts.dtype.is_floating_point and m.verts.element_size() == 8
        # the file holds the shortest digits that read back as the stored value IN ITS TYPE: fp64 vertices return exactly, fp32 ones
        # after rounding to fp32 again
        assert np.array_equal(m.verts.numpy().astype(verts.dtype), verts) and np.array_equal(m.tets.numpy(), t)
        assert np.array_equal(m.bfaces.numpy(), bf) and np.array_equal(a.numpy(), attr) and a.numpy().dtype == np.int32
    bad = tmp_path / "hex.mesh"
    bad.write_text("MFEM mesh v1.0\n\ndimension\n3\n\nelements\n1\n1 5 0 1 2 3 4 5 6 7\n\nboundary\n0\n\nvertices\n8\n3\n" + "0 0 0\n" * 8)
    with pytest.raises(ValueError, match="tetrahedra"):
        TetMesh.read_mfem(str(bad))
    bad.write_text("MFEM mesh v1.0\n\ndimension\n3\n\nelements\n1\n1 4 0 1 2 3\n\nboundary\n1\n1 3 0 1 2 3\n\nvertices\n4\n3\n" + "0 0 0\n" * 4)
    with pytest.raises(ValueError, match="triangles"):
        TetMesh.read_mfem(str(bad))
    bad.write_text("not a mesh\n")
    with pytest.raises(ValueError, match="MFEM mesh v1.0"):
        TetMesh.read_mfem(str(bad))


def test_fem_argument_errors_come_before_any_launch():
    from deepsdf_amd import _lib
    lib = _lib.lib()
    bad, short = -1, -2
    p, null = 0x1000, 0                                              # never dereferenced: every call below fails before a launch
    P, N = C.c_void_p(p), C.c_void_p(0)
    b = C.c_size_t()
    assert lib.dsdf_fem_plan(100, 300, 50, C.byref(b)) == 0 and b.value >= 300 * 48 + 4 * 100 * 24
    assert lib.dsdf_fem_plan(100, 300, 50, None) == bad and lib.dsdf_fem_plan(0, 300, 50, C.byref(b)) == bad
    assert lib.dsdf_fem_plan(100, 0, 50, C.byref(b)) == bad and lib.dsdf_fem_plan(100, 2 ** 29, 50, C.byref(b)) == bad
    big = 1 << 24

    def op(**kw):
        d = dict(tets=p, corner_order=p, vstart=p, geom=p, dinv=p, mask=p, n_verts=100, n_tets=300, lam=0.0, mu=105.0)
        d.update(kw)
        return C.byref(_lib.DsdfFemOp(**d))
    it, cv, ratio = C.c_int32(-3), C.c_int32(-3), C.c_double(-3.0)
    calls = {"setup": lambda o, ws=P, nb=big: lib.dsdf_fem_setup(o, P, N, P, P, ws, nb, N),
             "apply": lambda o, ws=P, nb=big: lib.dsdf_fem_apply(o, P, C.c_void_p(0x2000), ws, nb, N),
             "solve": lambda o, ws=P, nb=big: lib.dsdf_fem_solve(o, P, C.c_void_p(0x2000), 1e-10, 10, 1, C.byref(it), C.byref(cv), C.byref(ratio), ws, nb, N),
             "energy": lambda o, ws=P, nb=big: lib.dsdf_fem_energy(o, P, P, 0, N, P, ws, nb, N)}
    for name, f in calls.items():
        assert f(None) == bad, name
        for k in ("tets", "corner_order", "vstart", "geom", "dinv", "mask"):
            assert f(op(**{k: null})) == bad, (name, k)
        assert f(op(tets=0x1004)) == bad and b"aligned" in lib.dsdf_last_error()
        assert f(op(n_verts=0)) == bad and f(op(n_tets=0)) == bad and f(op(mu=0.0)) == bad and f(op(lam=float("nan"))) == bad
        assert f(op(lam=-300.0)) == bad
        assert f(op(), ws=N) == bad and f(op(), ws=C.c_void_p(0x1010)) == bad and f(op(), nb=b.value - 1) == short, name
    assert it.value == 0 and cv.value == 0 and ratio.value == 0.0
    o = op()
    assert lib.dsdf_fem_setup(o, N, N, P, P, P, big, N) == bad and lib.dsdf_fem_setup(o, P, N, N, P, P, big, N) == bad
    assert lib.dsdf_fem_apply(o, P, P, P, big, N) == bad and lib.dsdf_fem_apply(o, N, P, P, big, N) == bad
    assert lib.dsdf_fem_solve(o, P, C.c_void_p(0x2000), -1.0, 10, 1, None, None, None, P, big, N) == bad
    assert lib.dsdf_fem_solve(o, P, C.c_void_p(0x2000), 1e-10, -1, 1, None, None, None, P, big, N) == bad
    assert lib.dsdf_fem_solve(o, P, C.c_void_p(0x2000), 1e-10, 10, 0, None, None, None, P, big, N) == bad
    assert lib.dsdf_fem_energy(o, P, P, 1, N, P, P, big, N) == bad and lib.dsdf_fem_energy(o, P, P, 3, P, P, P, big, N) == bad
    assert lib.dsdf_fem_energy(o, P, P, 0, P, P, P, big, N) == bad and lib.dsdf_fem_energy(o, P, N, 0, N, P, P, big, N) == bad
    t3 = (C.c_double * 3)(0.0, 0.0, -0.01)
    assert lib.dsdf_fem_load(N, 100, P, 50, P, P, N, t3, N, P, N) == bad and lib.dsdf_fem_load(P, 100, P, 50, P, P, N, None, N, P, N) == bad
    assert lib.dsdf_fem_load(P, 0, P, 50, P, P, N, t3, N, P, N) == bad and lib.dsdf_fem_load(P, 100, N, 50, P, P, N, t3, N, P, N) == bad
    assert lib.dsdf_fem_load(P, 100, P, 50, P, P, N, (C.c_double * 3)(0.0, float("inf"), 0.0), N, P, N) == bad
    assert lib.dsdf_fem_boundary_gradient(P, 100, P, 50, P, P, N, N, N) == bad and lib.dsdf_fem_boundary_gradient(P, 100, P, -1, P, P, N, P, N) == bad
    # dsdf_fem_solve's own arguments: each refused, and the three outputs zeroed before the refusal
    Q, nan, inf = C.c_void_p(0x2000), float("nan"), float("inf")
    for f, u, rel_tol, max_iter, check_every in ((P, Q, -1.0, 10, 1), (P, Q, -1e-300, 10, 1), (P, Q, nan, 10, 1), (P, Q, inf, 10, 1),
                                                 (P, Q, -inf, 10, 1), (P, Q, 1e-10, -1, 1), (P, Q, 1e-10, 10, 0), (P, Q, 1e-10, 10, -5),
                                                 (P, P, 1e-10, 10, 1), (N, Q, 1e-10, 10, 1), (P, N, 1e-10, 10, 1)):
        it, cv, ratio = C.c_int32(-3), C.c_int32(-3), C.c_double(-3.0)
        rc = lib.dsdf_fem_solve(o, f, u, rel_tol, max_iter, check_every, C.byref(it), C.byref(cv), C.byref(ratio), P, big, N)
        assert rc == bad and (it.value, cv.value, ratio.value) == (0, 0, 0.0), (rel_tol, max_iter, check_every)


def test_linear_elasticity_needs_a_device_mesh(meshes):
    from deepsdf_amd import _lib
    from deepsdf_amd.fem import LinearElasticity
    from deepsdf_amd.mesh import TetMesh
    with pytest.raises(_lib.DsdfError):
        LinearElasticity(TetMesh(*meshes["2x2x2"]), 0.0, 105.0)


def test_cantilever_beam_refuses_what_it_does_not_carry(tmp_path):
    from analysis.problems.CantileverBeam import CantileverBeam
    cb = CantileverBeam(str(tmp_path))
    for call, word in ((lambda: cb.set_up(ref_levels=1), "refinement"), (lambda: cb.set_up(order=2), "order"), (cb.show_mesh, "gustaf"),
                       (lambda: cb.show_solution("u_mag"), "gustaf")):
        with pytest.raises(NotImplementedError, match=word):
            call()
    with pytest.raises(ValueError):
        cb.compute_compliance()


# ---- discrimination ---------------------------------------------------------------------------------------------------------------
def test_every_wrong_variant_misses_the_truth_by_far_more_than_the_gpu_bounds(meshes):
    rng = np.random.default_rng(5)
    for name, (v, t, bf, kind) in meshes.items():
        nv = len(v)
        geom, skipped = F.geometry(v, t)
        fixed = F.fixed_vertices(bf, F.clamped_faces(v, bf), nv)
        mask = F.held_vertices(t, skipped, nv) | fixed
        assert mask.any() and not mask.all(), name
        x = rng.standard_normal((nv, 3))
        K = F.assemble(v, t, LAM, MU)
        A = F.masked(K, mask)
        Aabs = F.masked(F.assemble(v, t, LAM, MU, absolute=True), mask)
        nc = int(F.corner_counts(t, nv).max())
        bound = F.apply_bound_c(nc, int(np.diff(A.indptr).max())) * U * (Aabs @ np.abs(x).reshape(-1))
        truth = A @ x.reshape(-1)
        wrong = {"swap": F.masked(F.assemble(v, t, LAM, MU, "swap"), mask) @ x.reshape(-1),
                 "no_transpose": F.masked(F.assemble(v, t, LAM, MU, "no_transpose"), mask) @ x.reshape(-1),
                 "no_mask": K @ x.reshape(-1)}
        for k, y in wrong.items():
            worst = (np.abs(y - truth) / np.maximum(bound, 1e-300)).max()
            assert worst > 1e9, (name, k, worst)
        # the nodal modes and the normal's sign, on a smooth displacement
        u = _field(v, [[0.3, -0.2, 0.1], [0.4, 0.5, -0.6], [0.2, 0.1, -0.3]], [0, 0, 0]) + \
            0.05 * np.sin(np.asarray(v, dtype=np.float64) @ np.array([1.0, 2.0, 3.0]))[:, None] * np.array([1.0, -2.0, 0.5])
        w, V = F.energy_density(v, t, LAM, MU, u)
        wabs = F.energy_density(v, t, LAM, MU, u, absolute=True)[0]
        mean, last = F.nodal_density(t, w, V, nv, "mean"), F.nodal_density(t, w, V, nv, "last")
        nbound = (48 + 2 * (2 + 2 * nc)) * U * F.nodal_density(t, wabs, V, nv, "mean")
        if name != "one tet":                                           # one element: both modes are its value
            assert (np.abs(mean - last) / np.maximum(nbound, 1e-300)).max() > 1e9, name
        g, gf = F.boundary_gradient(v, bf), F.boundary_gradient(v, bf, flip=True)
        nfc = int(F.corner_counts(bf, nv).max())
        gbound = (2 * nfc + 2) * U * F.boundary_gradient(v, bf, absolute=True)
        assert (np.abs(g - gf) / np.maximum(gbound, 1e-300)).max() > 1e9, name


# ---- the CG step by step: the restatements' spread, the wrong variants, and every ending (tests/test_gpu_fem_cg.py runs the kernels) ---
def _window(traces):
    its = [t["it"] for t in traces.values()]
    return 0.9 * min(its) - 2, 1.1 * max(its) + 2


@pytest.mark.parametrize("name", F.CG_TRAJECTORY)
def test_cg_restatements_stay_together_and_every_wrong_variant_leaves_at_once(name):
    pr = F.cg_problem(name)
    A, ref, tr = pr["A"], pr["ref"], pr["traces"]
    u, it, conv, ratio = F.pcg(A, pr["Dinv"], pr["f"])
    base = tr["csr"]
    assert u.tobytes() == base["x"].tobytes() and (it, conv, ratio) == (base["it"], base["conv"], base["ratio"])    # pcg_trace is pcg
    assert all(t["conv"] for t in tr.values())
    K = pr["k_max"]
    s, q = pr["s"], pr["q"]
    bs, bq = F.cg_iterate_bound(s), F.cg_ratio_bound(q)
    err = [F.energy_distance(A, F.iterate(base, k), ref) for k in range(K + 1)]
    ks = sorted({1, 2, 3, 5, 8, 13, 21, 34, 55, 89, K // 2, base["it"], K} & set(range(K + 1)))
    print(f"{name}: iterations {[t['it'] for t in tr.values()]}; error {err[0]:.2e} -> {err[base['it']]:.2e}")
    print("  k: spread s_k / ratio spread q_k / error: " + "; ".join(f"{k}: {s[k]:.1e} / {q[k]:.1e} / {err[k]:.1e}" for k in ks))
    # the energy-norm error of CG falls at every step: where it stands above 1e3 x the GPU bound the oracle's own must not rise
    assert all(err[k + 1] <= err[k] for k in range(K) if err[k] > 1e3 * bs[k]), name
    lo, hi = _window(tr)
    for w in F.CG_WRONG:
        wt = F.pcg_trace(A, pr["Dinv"], pr["f"], wrong=w, max_iter=int(hi) + 1)       # past the window is all that is asked
        k = next(k for k in range(1, 4) if F.iterate(wt, k).tobytes() != F.iterate(base, k).tobytes())
        assert k == (2 if w in ("steepest", "dir_from_r") else 3)           # beta_1 enters x_2; the rho before rho_1 is rho0 in all three
        miss = F.energy_norm(A, F.iterate(wt, k) - F.iterate(base, k)) / F.energy_norm(A, ref) / bs[k]
        miss_q = abs(wt["ratios"][k] - base["ratios"][k]) / base["ratios"][k] / bq[k]
        print(f"  {w}: {wt['it']} iterations, converged {wt['conv']}; iterate {k} misses by {miss:.2e} x the GPU bound, its ratio by {miss_q:.2e} x")
        assert miss > 1e9 and miss_q > 1e9, (name, w, miss, miss_q)
        assert not (wt["conv"] and lo <= wt["it"] <= hi), (name, w, wt["it"])       # ... and its count, if it has one, falls outside


def test_pcg_trace_takes_the_operator_as_a_callable_and_keeps_every_scalar():
    pr = F.cg_problem("3x3x3")
    A, f = pr["A"], pr["f"]
    a, b = pr["traces"]["csr"], F.pcg_trace(lambda x: A @ x, pr["Dinv"], f)
    assert a["x"].tobytes() == b["x"].tobytes() and a["scal"] == b["scal"] and len(a["scal"]) == a["it"] == len(a["xs"]) - 1
    rho, x, p = a["rho0"], np.zeros(A.shape[0]), a["ps"][0]
    for k, (rn, alpha, beta, pap) in enumerate(a["scal"]):                  # the recorded scalars rebuild the iterates
        assert pap == a["paps"][k] and alpha == rho / pap and beta == rn / rho and a["ratios"][k + 1] == rn / a["rho0"]
        x = x + alpha * a["ps"][k]
        assert x.tobytes() == a["xs"][k + 1].tobytes()
        rho = rn
    for k in (0, 1, 5, a["it"]):                                            # max_iter = k returns iterate k
        c = F.pcg_trace(A, pr["Dinv"], f, max_iter=k)
        assert c["it"] == k and c["x"].tobytes() == a["xs"][k].tobytes() and c["conv"] == (k == a["it"])
    assert F.iterate(a, a["it"] + 7).tobytes() == a["x"].tobytes()


@pytest.mark.parametrize("name", list(F.CG_ENDINGS))
def test_the_oracle_reaches_every_ending_by_a_margin(name):
    pr = F.cg_problem(name)
    mesh, lam, mu, kind, j = F.CG_ENDINGS[name]
    assert mu > 0 and lam + 2 * mu > 0                                      # dsdf_fem_* accepts the material
    tr, A, mask = pr["traces"], pr["A"], pr["mask"]
    v, t, bf, _ = pr["mesh"]
    triples = [(x["it"], x["conv"], x["ratio"]) for x in tr.values()]
    print(f"{name}: {triples}")
    if kind == "zero":
        assert all(x == (0, True, 0.0) for x in triples) and all((x["x"] == 0).all() for x in tr.values())
    elif kind == "nan":
        assert np.isnan(pr["f"][~mask]).sum() == 1 and not np.isnan(pr["f"][mask]).any()
        assert all(x == (0, False, 0.0) for x in triples) and all((x["x"] == 0).all() for x in tr.values())
    elif kind == "vertex":
        # one free vertex: block Jacobi is the inverse.  alpha A p = r (1 + d), |d| <= c U cond(D) for the c <= 64 roundings through
        # the operator, the preconditioner and the update, so rho' / rho0 <= cond(D) (c U cond(D))^2
        assert (~mask).sum() == 1
        cond = np.linalg.cond(np.linalg.inv(pr["Dinv"][~mask][0]))
        bound = cond * (64 * U * cond) ** 2
        print(f"  cond(D) {cond:.3f}, ratio bound {bound:.2e}")
        assert all(x[0] == 1 and x[1] and 0.0 <= x[2] <= bound for x in triples) and bound < 1e-20
    elif kind == "random":
        assert 3 * lam + 2 * mu < 0                                          # K is indefinite ...
        blocks = np.linalg.eigvalsh(F.sym3(F.diag_blocks(A))).min()
        assert blocks > 0.2                                                  # ... its diagonal blocks are not
        Aabs = F.masked(F.assemble(v, t, lam, mu, absolute=True), mask)
        for k, x in tr.items():
            assert (x["it"], x["conv"]) == (j, False) and len(x["paps"]) == j + 1, (name, k)
            margin = [pap / (U * float(np.abs(p) @ (Aabs @ np.abs(p)))) for pap, p in zip(x["paps"], x["ps"])]
            print(f"  {k}: p.Ap / (U |p|^T |A| |p|) = {[f'{m:.2e}' for m in margin]}, smallest block eigenvalue {blocks:.3f}")
            assert all(m > 1e6 for m in margin[:-1]) and margin[-1] < -1e6, (name, k, margin)      # rounding cannot move the stop
        assert triples[0][2] == 1.0 if j == 0 else abs(triples[0][2] - 1.0) > 0.1
    elif kind == "overflow":
        # at scale 1 the three products of <z, r> and of <p, A p> at the loaded vertex are positive and of order 0.01 to 1; everywhere
        # else p is exactly 0.  Times 1e320 each of them is +inf (the largest double is 1.8e308) in any order and with any contraction
        one = F.cg_variants(v, t, lam, mu, mask, pr["f"] / F.OVERFLOW_SCALE, max_iter=1)[2]["csr"]
        p = one["ps"][0].reshape(-1, 3)
        ap = (A @ p.reshape(-1)).reshape(-1, 3)
        loaded = np.abs(pr["f"]).sum(1) > 0
        assert loaded.sum() == 1 and (p[~loaded] == 0).all() and np.isfinite(pr["f"]).all()
        terms = np.concatenate([(p * pr["f"] / F.OVERFLOW_SCALE)[loaded], (p * ap)[loaded]]).reshape(-1)
        print(f"  products at scale 1: {terms}; the load's scale {F.OVERFLOW_SCALE:g} enters each twice")
        assert (terms > 1e-3).all() and np.abs(A @ p.reshape(-1)).max() * F.OVERFLOW_SCALE < 1e300       # A p itself stays finite
        for k, x in tr.items():
            assert x["rho0"] == np.inf and x["paps"] == [np.inf] and (x["it"], x["conv"]) == (1, False) and np.isnan(x["ratio"]), k
            assert np.isnan(x["x"]).all()
    else:
        raise AssertionError(kind)
