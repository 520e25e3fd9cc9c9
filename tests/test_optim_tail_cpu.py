"""CPU: tests/optim_numpy.py (the spec the GPU tail tests compare every Adam form with) against torch's own optimiser in float64,
and the properties of its bound functions and of its input generator.  No GPU, no library call."""
import math

import numpy as np
import pytest
import torch

from tests import optim_numpy as O

# Both sides are float64 evaluations of the same formula in different operation orders: at most ~20 roundings of 1.1e-16 per step,
# ten steps, and the early steps' conditioning 1 / (1 - b1) = 10: 20 * 10 * 10 * 1.1e-16 = 2.2e-13 of the state's scale.
F64_TOL = 2.2e-13


def _run_torch(p0, grads, lr, weight_decay=0.0):
    p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=lr, betas=(O.B1, O.B2), eps=O.EPS, weight_decay=weight_decay, foreach=False)
    out = []
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
    return out


@pytest.mark.parametrize("variant", ["plain", "grad_scale", "l2"])
def test_spec_equals_torch_adam_in_float64_over_ten_steps(variant):
    n, lr = 4096, O.f32(1e-3)
    p0, g0, _, _ = O.make_state(n, 11, aged=False)
    rng = np.random.default_rng(5)
    grads = [g0.astype(np.float64) * rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n) for _ in range(10)]
    gs = 0.37 if variant == "grad_scale" else 1.0
    l2 = 0.02 if variant == "l2" else 0.0
    ref = _run_torch(p0.astype(np.float64), [g * gs for g in grads], lr, weight_decay=l2)      # Adam's weight_decay IS g + l2 p
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        r = O.adam_ref(p, g, m, v, lr=lr, t=t, grad_scale=gs, l2=l2)
        p, m, v = r["p"], r["m"], r["v"]
        tp, tm, tv = ref[t - 1]
        assert np.abs(m - tm).max() <= F64_TOL * np.abs(tm).max(), t
        assert np.abs(v - tv).max() <= F64_TOL * np.abs(tv).max(), t
        assert np.abs(p - tp).max() <= F64_TOL * (np.abs(tp).max() + t * lr), t
    assert np.abs(p - p0).max() > 5 * lr          # the ten steps moved something: the comparison is not between two no-ops


def test_spec_equals_the_oracle_adam_update():
    from oracle import deepsdf_oracle as orc
    n, lr = 1000, O.f32(5e-4)
    p0, g0, m0, v0 = O.make_state(n, 3)
    p, m, v = (torch.tensor(x, dtype=torch.float64) for x in (p0, m0, v0))
    orc.adam_update_(p, torch.tensor(g0, dtype=torch.float64), m, v, 1000, lr, O.B1, O.B2, O.EPS)
    r = O.adam_ref(p0, g0, m0, v0, lr=lr, t=1000)
    assert np.abs(r["p"] - p.numpy()).max() <= F64_TOL * 0.2 and np.abs(r["m"] - m.numpy()).max() <= F64_TOL * 0.2
    assert (np.abs(r["v"] - v.numpy()) <= F64_TOL * r["v"]).all()


def test_sched_scalars_equal_lr_and_step():
    p0, g0, m0, v0 = O.make_state(500, 4)
    lr, t = O.f32(1e-3), 7
    ss, bq = O.step_scalars(lr, O.B1, O.B2, t)
    a = O.adam_ref(p0, g0, m0, v0, lr=lr, t=t, l2=0.01)
    b = O.adam_ref(p0, g0, m0, v0, lr=None, t=None, l2=0.01, step_size=ss, bc2_sqrt=bq)
    for k in ("p", "m", "v"):
        assert np.array_equal(a[k], b[k])


@pytest.mark.parametrize("max_norm", [0.5, 1.0, 1e3])
def test_clip_coefficient_equals_clip_grad_norm(max_norm):
    rng = np.random.default_rng(2)
    gs = [rng.normal(0, 0.3, s) for s in ((7, 5), (33,), (4, 4, 2))]
    ps = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = torch.tensor(g, dtype=torch.float64)
    norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
    mine = math.sqrt(sum(float((g * g).sum()) for g in gs))
    assert abs(norm - mine) <= 1e-14 * mine
    c = O.clip_coef_ref(mine, max_norm)
    assert (c == 1.0) == (mine + 1e-6 <= max_norm)
    for p, g in zip(ps, gs):
        assert np.abs(p.grad.numpy() - c * g).max() <= 1e-14 * np.abs(g).max()


def test_row_scale_is_torch_weight_norm():
    rng = np.random.default_rng(8)
    v, g = rng.normal(0, 0.1, (9, 70)), rng.uniform(0.5, 2.0, 9)
    W = torch._weight_norm(torch.tensor(v), torch.tensor(g).reshape(-1, 1), 0).numpy()
    assert np.abs(W - v * O.row_scale_ref(g, v)[:, None]).max() <= 1e-15


def test_bound_functions_count_what_their_docstrings_state():
    assert O.U == 2.0 ** -24 and O.gamma(1) > O.U and abs(O.gamma(8) / (8 * O.U) - 1) < 1e-6
    one = np.ones(1)
    assert O.m_bound(one, one)[0] == O.gamma(2) and O.m_bound(one, one, True)[0] == O.gamma(3)
    assert O.v_bound(one)[0] == O.gamma(4) and O.v_bound(one, True)[0] == O.gamma(6)
    assert O.p_bound(0 * one, one)[0] == O.gamma(11) and O.p_bound(one, 0 * one)[0] == O.U
    assert O.p_bound(0 * one, one, True)[0] == O.gamma(13)
    assert O.sum_bound(1.0, 8, 6) == O.gamma(15)
    assert [O.row_scale_k(i) for i in (7, 64, 65, 507, 515)] == [6, 6, 7, 10, 10]     # ceil((1 + ceil(in/64) + 6) / 2) + 2
    assert O.grad_norm_counts(1) == (1, 1 + 1 + 8 + 1 + 8) and O.grad_norm_counts(4097) == (2, 1 + 9 + 8 + 1 + 8)
    assert O.grad_norm_counts(4096 * 1024 + 1) == (1024, 1 + 17 + 8 + 4 + 8)
    # a bound is never looser than a few hundred roundoffs: nothing here can hide a wrong formula
    assert O.gamma(13) < 1e-6 and O.grad_norm_bound(1.0, 1843195) < 2e-6


def test_bounds_hold_for_a_float32_evaluation_and_catch_a_wrong_one():
    """The un-contracted fp32 evaluation of the kernels' expressions (numpy float32, one rounding per operation) meets every bound at
    every step of the tests; the same evaluation with one wrong term misses them."""
    f = np.float32
    n = 20000
    p0, g0, m0, v0 = O.make_state(n, 6)
    O.check_state(p0, g0, m0, v0)
    lr = O.f32(1e-3)
    for t in (1, 2, 10, 1000, 100000):
        ss, bq = O.step_scalars(lr, O.B1, O.B2, t)
        ss, bq, omb1, b2, omb2, eps = f(ss), f(bq), f(1) - f(0.9), f(0.999), f(1) - f(0.999), f(1e-8)
        mi = omb1 * (g0 - m0) + m0
        vi = b2 * v0 + omb2 * g0 * g0
        pi = p0 - ss * (mi / (np.sqrt(vi) / bq + eps))
        r = O.adam_ref(p0, g0, m0, v0, lr=lr, t=t)
        assert (np.abs(mi - r["m"]) <= O.m_bound(m0, r["g_eff"])).all()
        assert (np.abs(vi - r["v"]) <= O.v_bound(r["v"])).all()
        assert (np.abs(pi - r["p"]) <= O.p_bound(r["p"], r["upd_scale"])).all()
        wrong = p0 - ss * (mi / (np.sqrt(vi + eps) / bq))          # eps inside the square root
        assert not (np.abs(wrong - r["p"]) <= O.p_bound(r["p"], r["upd_scale"])).all()
        if t <= 1000:
            wrong = p0 - ss * (mi / (np.sqrt(vi) + eps))           # the second bias correction dropped
            assert not (np.abs(wrong - r["p"]) <= O.p_bound(r["p"], r["upd_scale"])).all()


@pytest.mark.parametrize("n", [1, 255, 257, 5000, 2048 * 256 + 1])
@pytest.mark.parametrize("aged", [True, False])
def test_generator_properties(n, aged):
    s = O.make_state(n, 100 + n, aged=aged)
    O.check_state(*s, aged=aged)
    assert all(x.dtype == np.float32 and x.size == n for x in s)
    s2 = O.make_state(n, 100 + n, aged=aged)
    assert all(np.array_equal(a, b) for a, b in zip(s, s2))        # fixed: the same inputs every run
