"""-m gpu: the elasticity solver's CG (dsdf_fem_solve, csrc/fem.hpp fem_cg_*) followed step by step and through every way it can end,
through LinearElasticity.solve alone: solve(max_iter=k) returns iterate k, so k solves give the kernels' path u_1 .. u_k with their
(iterations, converged, ratio).  The path is held to the fp64 restatement of tests/fem_numpy.py within 16 times the spread of four
correct restatements among themselves; tests/test_fem_cpu.py shows that every wrong CG leaves that bound by more than
1e9 at iterate 2 or 3, and that the oracle reaches each ending on the inputs used here by a margin no rounding can cross."""
import math

import numpy as np
import pytest
import torch

from tests import fem_numpy as F
from tests.test_gpu_fem import Case

pytestmark = pytest.mark.gpu

U = F.U
REFERENCE = "csr"                # the restatement the kernels' path is compared with: F.pcg itself
CHECK_EVERY = (1, 7, 10 ** 6)
_cases = {}


def _case(pr):
    """The problem's mesh on the device: the CPU tests' arrays themselves, so that what they prove holds for what runs here."""
    from deepsdf_amd.mesh import TetMesh
    key = (pr["name"], pr["lam"], pr["mu"])
    if key not in _cases:
        _cases[key] = Case(pr["name"], TetMesh(*pr["mesh"]).to("cuda"), lam=pr["lam"], mu=pr["mu"], assemble=False)
    return _cases[key]


def _solver(pr, f=None):
    """A fresh solver (its own workspace and scalar record) with the problem's mask and the oracle's load, bit for bit."""
    s = _case(pr).solver(True)
    assert np.array_equal(s.mask.cpu().numpy().astype(bool), pr["mask"])
    return s.add_nodal_forces(pr["f"] if f is None else f)


def _set_load(s, f):
    s.f.zero_()
    return s.add_nodal_forces(f)


def _run(s, **kw):
    """((iterations, converged, ratio), u as host bytes' owner)."""
    res = s.solve(**kw)
    return res, s.u.cpu().numpy().copy()


def _same(a, b):
    """Two results of _run: equal triples (NaN matching NaN) and identical bytes of u."""
    (ra, ua), (rb, ub) = a, b
    same_ratio = (math.isnan(ra[2]) and math.isnan(rb[2])) or ra[2] == rb[2]
    return ra[:2] == rb[:2] and same_ratio and ua.tobytes() == ub.tobytes()


def _ladder(it_full):
    """1, 2, 3, 5, 8, ... and the four counts around the end."""
    ks, a, b = set(), 1, 2
    while a < it_full:
        ks.add(a)
        a, b = b, a + b
    return sorted(ks | {it_full - 1, it_full, it_full + 1, it_full + 2})


@pytest.fixture(scope="module")
def paths():
    """name -> (problem, the full solve, {k: solve(max_iter=k) on a fresh solver}): run once per mesh, never changed."""
    cache = {}

    def get(name):
        if name not in cache:
            pr = F.cg_problem(name)
            full = _run(_solver(pr))
            it_full = full[0][0]
            ks = _ladder(it_full) if name == "cut" else list(range(1, it_full + 3))
            cache[name] = (pr, full, {k: _run(_solver(pr), max_iter=k) for k in ks})
        return cache[name]
    return get


def _at(a, k):
    return a[min(k, len(a) - 1)]


def _oracles(pr):
    """The restatements the kernels are held to: {name: trace}, REFERENCE among them."""
    return pr["traces"]


# ---- 1. the path --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.CG_TRAJECTORY)
def test_every_iterate_follows_the_oracles_path(paths, name):
    pr, (full_res, full_u), runs = paths(name)
    it_full, conv_full, _ = full_res
    A, ref, o = pr["A"], pr["ref"], _oracles(pr)[REFERENCE]
    nref = F.energy_norm(A, ref)
    bound = F.cg_iterate_bound(pr["s"])
    assert conv_full and np.isfinite(full_u).all()
    rows = []
    for k, (res, u) in runs.items():
        assert res[0] == min(k, it_full) and res[1] == (k >= it_full), (name, k, res)
        assert np.isfinite(u).all() and (u[pr["mask"]] == 0).all(), (name, k)
        if k >= it_full:
            assert _same((res, u), (full_res, full_u)), (name, k)                  # past the end: the bytes of the iteration that ended it
        rows.append((k, F.energy_norm(A, u - F.iterate(o, k)) / nref, _at(bound, k), F.energy_distance(A, u, ref)))
    worst = max(rows, key=lambda r: r[1] / r[2])
    print(f"{name}: iterations GPU {it_full} / oracle {[t['it'] for t in _oracles(pr).values()]}; worst distance from iterate k of "
          f"'{REFERENCE}' / (16 max(s_k, U)) = {worst[1] / worst[2]:.3e} at k = {worst[0]} (distance {worst[1]:.2e}, s_k {worst[2] / 16:.2e})")
    print("  k: distance / bound / error: " + "; ".join(f"{k}: {d:.1e} / {b:.1e} / {e:.1e}" for k, d, b, e in rows[:: max(1, len(rows) // 16)]))
    assert worst[1] <= worst[2], (name, worst)
    for (k, _, b, e), (k1, _, _, e1) in zip(rows, rows[1:]):                       # CG's energy-norm error falls at every step
        if e > 1e3 * b:
            assert e1 <= e, (name, k, k1, e, e1)


@pytest.mark.parametrize("name", F.CG_TRAJECTORY)
def test_every_returned_ratio_is_the_oracles_recursive_one(paths, name):
    pr, _, runs = paths(name)
    o = _oracles(pr)[REFERENCE]
    bound = F.cg_ratio_bound(pr["q"])
    rows = [(k, abs(res[2] - _at(o["ratios"], k)) / _at(o["ratios"], k), _at(bound, k)) for k, (res, _) in runs.items()]
    worst = max(rows, key=lambda r: r[1] / r[2])
    print(f"{name}: worst |ratio_k - rho_k / rho0| / rho_k / rho0 / max(16 q_k, 64 U) = {worst[1] / worst[2]:.3e} at k = {worst[0]} "
          f"(relative difference {worst[1]:.2e}, q_k {worst[2] / 16:.2e})")
    assert all(math.isfinite(r[1]) for r in rows) and worst[1] <= worst[2], (name, worst)


@pytest.mark.parametrize("name", F.CG_TRAJECTORY)
def test_the_iteration_count_is_the_oracles(paths, name):
    pr, (full_res, _), _ = paths(name)
    its = [t["it"] for t in _oracles(pr).values()]
    print(f"{name}: iterations GPU {full_res[0]}, oracle {its}")
    assert 0.9 * min(its) - 2 <= full_res[0] <= 1.1 * max(its) + 2, (name, full_res[0], its)


def test_no_iteration_at_all_returns_the_start():
    pr = F.cg_problem("2x2x2")
    for ce in CHECK_EVERY:
        res, u = _run(_solver(pr), max_iter=0, check_every=ce)
        assert res == (0, False, 1.0) and u.tobytes() == bytes(u.nbytes)


# ---- 2. the endings -----------------------------------------------------------------------------------------------------------------
MAX_ITER = 1000                   # far past every ending below: a solve that ran on would report it


def _end(name, **kw):
    pr = F.cg_problem(name)
    return pr, _run(_solver(pr), max_iter=MAX_ITER, **kw)


@pytest.mark.parametrize("name", list(F.CG_ENDINGS))
def test_every_ending_returns_what_the_oracle_returns(name):
    kind, j = F.CG_ENDINGS[name][3:]
    pr, first = _end(name, check_every=CHECK_EVERY[0])
    for ce in CHECK_EVERY[1:]:
        assert _same(_end(name, check_every=ce)[1], first), (name, ce)
    (it, conv, ratio), u = first
    o = _oracles(pr)[REFERENCE]
    print(f"{name}: GPU {(it, conv, ratio)}, oracle {(o['it'], o['conv'], o['ratio'])}")
    assert (it, conv) == (o["it"], o["conv"]) and it == j, name
    zero = bytes(u.nbytes)
    if kind in ("zero", "nan"):
        assert ratio == 0.0 == o["ratio"] and u.tobytes() == zero
    elif kind == "overflow":
        assert math.isnan(ratio) and math.isnan(o["ratio"]) and not np.isfinite(u).any() and not np.isfinite(o["x"]).any()
    elif kind == "vertex":             # the bound of tests/test_fem_cpu.py: rho' / rho0 <= cond(D) (64 U cond(D))^2, u the solution to 64 U cond(D)
        cond = np.linalg.cond(np.linalg.inv(pr["Dinv"][~pr["mask"]][0]))
        assert 0.0 <= ratio <= cond * (64 * U * cond) ** 2
        assert F.energy_distance(pr["A"], u, o["x"]) <= 64 * U * cond and (u[pr["mask"]] == 0).all()
    else:                              # p . A p <= 0 after j iterations: the state of iteration j, frozen
        assert _same(first, _run(_solver(pr), max_iter=j)), name
        if j == 0:
            assert ratio == 1.0 == o["ratio"] and u.tobytes() == zero
        else:
            rel, bound = abs(ratio - o["ratio"]) / o["ratio"], F.cg_ratio_bound(pr["q"])[j]
            print(f"  |ratio - oracle's| / oracle's / max(16 q_j, 64 U) = {rel / bound:.3e}")
            assert rel <= bound and np.isfinite(u).all() and np.abs(u).max() > 0


# ---- 3. one solver, one workspace, one scalar record: a second solve starts from nothing ---------------------------------------------
def _good_load(pr):
    v, _, bf, _ = pr["mesh"]
    return F.cg_load("traction", v, bf, pr["mask"]) if len(v) > 4 else -0.5 * F.cg_load("vertex", v, bf, pr["mask"])


@pytest.mark.parametrize("name", list(F.CG_ENDINGS) + ["2x2x2", "2x2x2 stopped at 3"])
def test_a_solve_after_any_ending_gives_a_fresh_solvers_bytes(name):
    pr = F.cg_problem(name.split(" stopped")[0])
    s = _solver(pr)
    res, _ = _run(s, max_iter=3 if "stopped" in name else MAX_ITER)
    if name in F.CG_ENDINGS:
        assert res[0] == F.CG_ENDINGS[name][4]                                  # the ending was reached
    g = _good_load(pr)
    second = _run(_set_load(s, g), max_iter=MAX_ITER)
    fresh = _run(_solver(pr, g), max_iter=MAX_ITER)
    print(f"{name}: first {res}, then {second[0]}; a fresh solver {fresh[0]}")
    assert _same(second, fresh) and np.isfinite(second[1]).all() and np.abs(second[1]).max() > 0, name
    if pr["lam"] == F.CG_LAM:
        assert second[0][1]                                                     # a definite material: the good load converges
    third = _run(_set_load(s, np.zeros_like(g)), max_iter=MAX_ITER)             # ... and the zero load after a good solve
    assert third[0] == (0, True, 0.0) and third[1].tobytes() == bytes(third[1].nbytes), name


# ---- 4. what is not finite at a masked vertex never enters -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x3x3", "cut"])
def test_a_non_finite_load_at_a_fixed_vertex_changes_nothing(paths, name):
    pr, full, _ = paths(name)
    clean = _solver(pr)
    assert _same(_run(clean), full)
    f = pr["f"].copy()
    fixed = np.flatnonzero(pr["mask"])
    assert len(fixed) >= 3 and (f[fixed] == 0).all()
    f[fixed[0]], f[fixed[1], 1], f[fixed[-1], 2] = np.nan, np.inf, -np.inf
    s = _solver(pr, f)
    assert not bool(torch.isfinite(s.f).all())
    assert _same(_run(s), full), name
    assert s.load().cpu().numpy().tobytes() == clean.load().cpu().numpy().tobytes() == pr["f"].tobytes()
    w = s.work()
    assert math.isfinite(w) and w == clean.work() and w > 0
