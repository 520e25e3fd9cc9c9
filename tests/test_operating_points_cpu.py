"""CPU: the operating points of tests/operating_points.py, with the oracle and stock torch alone.

  1. The oracle against stock torch at EVERY point -- the goldens pin it to the reference at one point only (two more since g14a / g14b).
  2. The populations of every batch tests/test_gpu_operating_points.py uses: every region of the loss head is visited.
  3. The points discriminate and the old point did not: each wrong variant a point claims to cover moves the compared quantity by at
     least 100 times the bound the GPU test asserts for it; at the reference's point the three renorm variants move nothing at all.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import deepsdf_oracle as orc
from oracle.torch_native import NativeStep
from tests import operating_points as OP
from tests import optim_numpy as O
from tests.golden_io import rel_err

POINT_NAMES = [p.name for p in OP.POINTS]
FP64 = 1e-12                 # two float64 evaluations of the same expressions in another order


# ---- 1. the oracle against stock torch -------------------------------------------------------------------------------------------------
def test_the_table_has_the_points_the_design_names():
    P = OP.BY_NAME
    cbs = {p.code_bound for p in OP.POINTS}
    assert {0.6, 2.5, None, 0.0} <= cbs
    assert {0.03, 0.4} <= {p.delta for p in OP.POINTS}
    assert {(p.lam, p.epoch) for p in OP.POINTS} >= {(1e-2, 37), (1e-2, 130)} and P["lam1e-2_epoch37"].ramp == 0.37
    assert any(not p.code_reg for p in OP.POINTS)
    assert P["betas_eps"].betas == (0.8, 0.95) and P["betas_eps"].eps == 1e-5
    assert P["eps_only"].betas == (0.9, 0.999) and P["eps_only"].eps == 1e-5
    assert P["lr_swapped"].lr[0] > P["lr_swapped"].lr[1]
    assert P["n_norm_3N"].n_norm_factor == 3
    assert P["clip_fires"].clip_factor < 1 < P["clip_idle"].clip_factor
    assert {p.dropout_prob for p in OP.POINTS} == {0.0, 0.2}
    for v in OP.VARIANTS:                           # every variant is claimed by some point
        assert any(v in p.covers for p in OP.POINTS), v


@pytest.mark.parametrize("layout", sorted(OP.LAYOUTS))
@pytest.mark.parametrize("name", POINT_NAMES)
def test_renorm_rows_against_torch_embedding(name, layout):
    """renorm_rows_ against F.embedding(max_norm=) in float64 on the point's own table, and the rows the design promises: for 0.6 one
    row each in (0.6, sqrt 0.6), (sqrt 0.6, 1) and above 1, all scaled, and one below 0.6, untouched; for 2.5 one each in (1, sqrt 2.5)
    and (sqrt 2.5, 2.5), untouched, and one above; rows not looked up, and every row under None or a bound <= 0, bit for bit as before."""
    p = OP.BY_NAME[name]
    scenes, lens = OP.LAYOUTS[layout]
    idx = torch.tensor(scenes).repeat_interleave(torch.tensor(lens))
    lat0 = OP.latent_table(5, p.code_bound, 123).double()
    mine, theirs = lat0.clone(), lat0.clone()
    cb = None if p.code_bound is None else O.f32(p.code_bound)
    orc.renorm_rows_(mine, idx, cb)
    off = cb is None or cb <= 0
    with torch.no_grad():                           # (torch reads max_norm = 0 as a bound of zero; the C ABI, and the oracle, as "none")
        F.embedding(idx, theirs, max_norm=None if off else cb)
    assert rel_err(mine, theirs) <= 1e-15
    norms = lat0.norm(dim=1)
    used = sorted(set(scenes))
    assert used == [0, 1, 3, 4] and (len(scenes) > len(used)) == (layout == "ragged")    # ragged: one scene in two segments
    for r in range(OP.TABLE_ROWS):
        scaled = (r in used) and not off and float(norms[r]) > cb
        if scaled:
            assert abs(float(mine[r].norm()) - cb) < 1e-6 * cb, (r, float(mine[r].norm()))           # scaled ONCE: lands on the bound
            assert torch.allclose(mine[r], lat0[r] * (cb / (norms[r] + 1e-7)), rtol=1e-15, atol=0)
        else:
            assert torch.equal(mine[r], lat0[r]) and torch.equal(theirs[r], lat0[r]), r
    n = {r: float(norms[r]) for r in used}
    if p.code_bound == 0.6:
        assert sorted(n.values())[0] < 0.6 < sorted(n.values())[1] < 0.6 ** 0.5 < sorted(n.values())[2] < 1 < 1.5 < sorted(n.values())[3]
        assert sum(not torch.equal(mine[r], lat0[r]) for r in used) == 3
    if p.code_bound == 2.5:
        assert sorted(n.values())[1] > 1 and sorted(n.values())[1] < 2.5 ** 0.5 < sorted(n.values())[2] < 2.5 < sorted(n.values())[3]
        assert sum(not torch.equal(mine[r], lat0[r]) for r in used) == 1
    if off:
        assert torch.equal(mine, lat0)
    assert all(float(norms[r]) > 1.6 for r in range(OP.TABLE_ROWS) if r not in used)     # a renorm of an unused row would show


@pytest.mark.parametrize("name", POINT_NAMES)
def test_loss_head_and_regulariser_against_autograd(name):
    """clamped_l1 and code_regulariser against autograd of the reference's own expressions (train_deep_sdf.py:493, 517-531) on the
    point's batches: delta, n_norm, lambda x ramp as the point sets them."""
    for kind, layout in OP.ROUTE_CASES[:2]:
        c = OP.get_case(name, kind, layout)
        p = c.point
        for s in range(c.steps):
            y = c.results[s]["y"].clone().requires_grad_(True)
            gt, delta = c.batches[s][2].double(), c.deltas[s]
            loss = F.l1_loss(torch.clamp(y, -delta, delta), torch.clamp(gt, -delta, delta), reduction="sum") / c.n_norm
            loss.backward()
            mine, dy = orc.clamped_l1(y.detach(), gt, delta, c.n_norm)
            assert abs(float(mine) - float(loss.detach())) <= FP64 * abs(float(loss.detach())) and rel_err(dy, y.grad) <= FP64
            assert 0.2 < float((dy == 0).double().mean()) < 0.8                        # both branches of the head
            z = c.lat_ren[s][c.batches[s][0]].clone().requires_grad_(True)
            r = p.lam * min(1, p.epoch / 100) * torch.sum(torch.norm(z, dim=1)) / c.n_norm
            r.backward()
            mine, dz = orc.code_regulariser(z.detach(), p.lam, p.epoch, c.n_norm)
            assert abs(float(mine) - float(r.detach())) <= FP64 * float(r.detach()) and rel_err(dz, z.grad) <= FP64
            # ... and as Case hands it over: lambda x ramp in one float32-rounded coefficient
            mine32, _ = orc.code_regulariser(z.detach(), c.reg_coef if p.code_reg else O.f32(p.lam * p.ramp), 100, c.n_norm)
            assert abs(float(mine32) - float(r.detach())) <= 1e-7 * float(r.detach())


ADAM_CONSTANTS = sorted({(p.lr[1], p.betas, p.eps) for p in OP.POINTS})


@pytest.mark.parametrize("lr,betas,eps", ADAM_CONSTANTS)
def test_adam_against_torch_optim_over_ten_steps(lr, betas, eps):
    """adam_update_ and optim_numpy.adam_ref against torch.optim.Adam(betas=, eps=) in float64, ten steps from an aged state's
    parameters with a new gradient every step."""
    n = 1000
    p0, g0, _, _ = O.make_state(n, 5)
    rng = np.random.default_rng(6)
    tp = torch.from_numpy(p0.astype(np.float64)).clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps)
    po, mo, vo = torch.from_numpy(p0.astype(np.float64)).clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    pn, mn, vn = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 11):
        g = g0.astype(np.float64) * rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)
        tp.grad = torch.from_numpy(g).clone()
        opt.step()
        orc.adam_update_(po, torch.from_numpy(g), mo, vo, t, lr, betas[0], betas[1], eps)
        r = O.adam_ref(pn, g, mn, vn, lr=lr, t=t, b1=betas[0], b2=betas[1], eps=eps)
        pn, mn, vn = r["p"], r["m"], r["v"]
        st = opt.state[tp]
        for mine in (po, torch.from_numpy(pn)):
            assert rel_err(mine - torch.from_numpy(p0).double(), tp.detach() - torch.from_numpy(p0).double()) <= 1e-11, t     # the MOVEMENT
        for mine in (mo, torch.from_numpy(mn)):
            assert rel_err(mine, st["exp_avg"]) <= FP64, t
        for mine in (vo, torch.from_numpy(vn)):
            assert rel_err(mine, st["exp_avg_sq"]) <= FP64, t


@pytest.mark.parametrize("kind,layout", [("main", "segment"), ("w32", "ragged")])
@pytest.mark.parametrize("name", POINT_NAMES)
def test_train_step_against_the_stock_torch_restatement(name, kind, layout):
    """oracle.train_step against oracle/torch_native.NativeStep (F.linear + autograd + nn.Embedding(max_norm) + torch.optim.Adam with
    betas and eps + clip_grad_norm_) in float64, two steps at every point: loss, parameters, table."""
    c = OP.get_case(name, kind, layout)
    p = c.point
    off = c.code_bound is None or c.code_bound <= 0
    nat = NativeStep(c.net, {k: v.double() for k, v in c.params.items()}, c.lat0.double(), code_bound=None if off else c.code_bound,
                     lr_decoder=c.lr[0], lr_latent=c.lr[1], betas=c.betas, eps=c.eps)
    for s in range(c.steps):
        idx, xyz, gt = c.batches[s]
        loss = nat.step(idx, xyz.double(), gt.double(), delta=c.deltas[s], code_reg=p.code_reg, code_reg_lambda=c.reg_coef, epoch=100,
                        seed=OP.DROP_SEED, n_norm=c.n_norm, grad_clip=c.grad_clip[s])
        r = c.results[s]
        assert abs(loss - float(r["loss"])) <= 1e-12 * abs(loss), (s, loss, float(r["loss"]))
        base = {k: v.double() for k, v in c.params.items()}
        for k in r["params"]:                       # the movement since the start, not the parameter: lr-sized, and all Adam's
            assert rel_err(nat.params[k].detach() - base[k], r["params"][k] - base[k]) <= 1e-9, (s, k)
        assert rel_err(nat.lat.weight.detach() - c.lat0.double(), r["latents"] - c.lat0.double()) <= 1e-9, s
    if p.clip_factor is not None:                   # the clip fires where the point says so, and only there
        gn = float(c.results[0]["grad_norm"])
        assert (gn > c.grad_clip[0]) == (p.clip_factor < 1), (gn, c.grad_clip[0])


# ---- 2. the populations ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", OP.all_gpu_cases(), ids=lambda a: "-".join(str(x) for x in a))
def test_every_region_of_the_head_is_populated(args):
    """Each inside region >= 10 % of the points, outside >= 20 %, loss-carrying and zero-loss outside points >= 5 % each, every non-zero
    |clamp(y) - clamp(gt)| >= 1e-3, safe_batch's margins -- asserted on the fp64 oracle's y for every step of every GPU case."""
    c = OP.get_case(*args)
    seen = {k: 0 for k in OP.REGIONS}
    for s in range(c.steps):
        idx, xyz, gt = c.batches[s]
        y = c.results[s]["y"]
        f = OP.check_populations(y, gt, c.deltas[s])
        assert float(((y.abs() - c.deltas[s]).abs()).min()) >= OP.MARGIN
        assert c.deltas[s] == O.f32(c.deltas[s]) and xyz.dtype == gt.dtype == torch.float32
        for k in seen:
            seen[k] += round(f[k] * c.N)
        looked = sorted(set(idx.tolist()))
        assert looked == [0, 1, 3, 4] and idx.numel() == c.N
        if c.code_bound is not None and c.code_bound > 0:          # no looked-up row sits ON the bound, where fp32 and fp64 may decide apart
            found = (c.lat0.double() if s == 0 else c.results[s - 1]["latents"])[looked].norm(dim=1)
            assert float((found - c.code_bound).abs().min()) >= 1e-5, (s, found)
    assert min(seen.values()) >= 2, seen           # all six regions, the two mirror images included, on every net


def test_fixed_deltas_survive_where_the_oracle_allows_them():
    """The per-case quantile replaces a point's delta only where |y| does not straddle it: 0.03 is kept on the main net."""
    assert OP.get_case("cb0.6_delta0.03", "main", "segment").deltas == [O.f32(0.03)] * 2
    assert OP.get_case("betas_eps", "main", "ragged").deltas == [O.f32(0.03)] * 2
    for kind, layout in OP.ROUTE_CASES:             # 0.4 on every net: that point's output layer is scaled up so that |y| straddles it
        assert OP.get_case("cb2.5_delta0.4", kind, layout).deltas == [O.f32(0.4)] * 2, (kind, layout)


def test_the_fp32_cpu_oracle_is_far_inside_every_bound():
    """The fp32 CPU oracle's own distance from the fp64 one, per quantity, on every GPU case: below a quarter of the bound, so no case
    of the GPU test needs the allowance tests/test_gpu_breakpoints.py grants (four times this distance) and none is granted."""
    worst = {}
    for args in OP.all_gpu_cases():
        c = OP.get_case(*args)
        if c.net_bf16 is not None:
            continue
        before = (c.lat0.clone(), {k: v.clone() for k, v in c.params.items()})
        r32 = c.rerun(torch.float32)
        assert torch.equal(c.lat0, before[0]) and all(torch.equal(c.params[k], v) for k, v in before[1].items())     # a shared case is read-only
        for q, (_, bound) in OP.QUANTITIES.items():
            d = OP.distance(r32, c.results, q) / bound
            if d > worst.get(q, (0, ""))[0]:
                worst[q] = (d, c.id)
    print("\n".join(f"fp32 oracle / bound  {q:<16s} {d:.3f}  at {w}" for q, (d, w) in worst.items()))
    assert all(d <= 0.25 for d, _ in worst.values()), worst


# ---- 3. the points discriminate --------------------------------------------------------------------------------------------------------
def _adam_element_ratio(c, b1, b2, eps):
    """The isolated Adam comparison of the GPU test: the worst |spec(point's constants) - spec(b1, b2, eps)| over the spec's bound."""
    p0, g0, m0, v0 = O.make_state(4096, 17)
    t = 1000
    a = O.adam_ref(p0, g0, m0, v0, lr=c.lr[1], t=t, b1=c.betas[0], b2=c.betas[1], eps=c.eps)
    b = O.adam_ref(p0, g0, m0, v0, lr=c.lr[1], t=t, b1=b1, b2=b2, eps=eps)
    return float(np.max(np.abs(a["p"] - b["p"]) / O.p_bound(a["p"], a["upd_scale"])))


@pytest.mark.parametrize("name", POINT_NAMES)
def test_each_point_tells_its_variants_from_the_truth(name):
    """Every wrong variant a point covers, patched into the oracle, on both renorm sites' cases: the compared quantity moves by at least
    100 times the bound the GPU test asserts for it."""
    p = OP.BY_NAME[name]
    for layout in ("segment", "ragged"):
        c = OP.get_case(name, "main", layout)
        for v in p.covers:
            q = OP.VARIANTS[v][2]
            with OP.patched(v, c):
                alt = c.rerun()
            ratio = OP.distance(alt, c.results, q) / OP.QUANTITIES[q][1]
            assert ratio >= 100, (name, layout, v, q, ratio)
            if v == "default_eps":                  # ... and in the isolated, element-wise Adam comparison at its counted bound
                assert _adam_element_ratio(c, c.betas[0], c.betas[1], OP.EPS_DEFAULT) >= 100
            assert OP.distance(c.rerun(), c.results, q) == 0.0      # the patch is gone


def test_adam_variants_move_the_isolated_comparison():
    c = OP.get_case("betas_eps", "main", "segment")
    assert _adam_element_ratio(c, OP.B1_DEFAULT, c.betas[1], c.eps) >= 100
    assert _adam_element_ratio(c, c.betas[0], OP.B2_DEFAULT, c.eps) >= 100
    assert _adam_element_ratio(c, c.betas[0], c.betas[1], OP.EPS_DEFAULT) >= 100
    assert _adam_element_ratio(c, c.betas[0], c.betas[1], c.eps) == 0.0


@pytest.mark.parametrize("layout", ["segment", "ragged"])
def test_at_the_reference_point_the_renorm_variants_move_nothing(layout):
    """CodeBound 1.0: a scale without max_norm, a threshold of 1 and a compare on the sum of squares give the right formula's bits --
    every quantity of both steps is EXACTLY what the true oracle computes.  This is the gap the operating points close."""
    c = OP.get_case("reference", "main", layout)
    assert float(c.lat0[1].norm()) > 1.5            # the renorm fires at this point too
    assert not torch.equal(c.lat_ren[0][1], c.lat0[1].double())
    for v in ("renorm_threshold_one", "renorm_no_max_norm", "renorm_compare_ss"):
        with OP.patched(v, c):
            alt = c.rerun()
        for q in OP.QUANTITIES:
            assert OP.distance(alt, c.results, q) == 0.0, (v, q)
