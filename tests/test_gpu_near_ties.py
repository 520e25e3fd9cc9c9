"""-m gpu: the training step AT its decision sites.  Every other oracle comparison runs on a batch that keeps a margin
around the ReLUs, the loss's sign and the clamp edges (tests/safe_batch.py); here the batch sits on them.

  near-ties   tests/near_ties.py plants one pre-activation per hidden unit within a rounding of zero, targets on the output itself and
              the clamp edge on one point's |y|.  The kernel's own decisions are read back from what it stored, checked against a counted
              rounding band around fp64 values recomputed from the kernel's own layer inputs, and the fp64 oracle -- forced onto those
              decisions -- must give the kernel's loss and gradients at the suite's ordinary bounds.
  exact ties  built so that no summation order can move them; the specification (the oracle) says which branch is right and the
              result is compared exactly: a unit whose pre-activation is +-0 everywhere, the output exactly on the clamp edge,
              a latent row whose norm is exactly CodeBound.

Both run on every training kernel family (the route table below restates pick_path's precedence to check that the switches
reach the family they are meant to), in segment mode and down the general path."""
import math

import pytest
import torch

from deepsdf_amd import _lib
from deepsdf_amd.net import NetSpec
from oracle import deepsdf_oracle as orc
from tests import near_ties as NT
from tests import optim_numpy as O
from tests import ws_guard as G
from tests.golden_io import rel_err, worst_elem
from tests.hip_helpers import HipTrainer
from tests.operating_points import renorm_roundings
from tests.test_gpu_parity import FWD_TOL, GRAD_ELEM_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu
K_ = G.constants()
SWITCHES = ("DSDF_NO_FUSED", "DSDF_NO_NARROW", "DSDF_FROWS", "DSDF_NO_W32", "DSDF_NO_W32X2", "DSDF_NO_MERGE")

# route id -> (net of near_ties.nets(), environment, NetworkSpecs extras, the family pick_path must choose, merged launch)
ROUTES = {
    "w32": ("w32", {}, {}, "FAM_W32", True),
    "h32_narrow": ("w32", {"DSDF_NO_W32": "1"}, {}, "FAM_H32", True),
    "n128": ("w32", {"DSDF_FROWS": "64"}, {}, "FAM_N128", True),
    "w32x2": ("w64", {}, {}, "FAM_W32X2", True),
    "h32": ("w136", {}, {}, "FAM_H32", True),
    "fp32": ("w136", {"DSDF_FROWS": "64"}, {}, "FAM_FP32", True),
    "fp32_unmerged": ("w136", {"DSDF_NO_MERGE": "1"}, {}, "FAM_FP32", False),
    "n128_unmerged": ("w64", {"DSDF_NO_MERGE": "1"}, {}, "FAM_N128", False),
    "split": ("w136", {}, dict(gemm_split=True), "FAM_SPLIT", True),
    "layered": ("w136", {"DSDF_NO_FUSED": "1"}, {}, "FAM_LAYERED", False),
    "bf16": ("w136", {}, dict(forward_bf16=True), "FAM_BF16", True),
    "bf16_split": ("w136", {}, dict(forward_bf16=True, gemm_split=True), "FAM_BF16_SPLIT", True),
}
LAYOUTS = [{}, dict(force_ragged=True)]


def family_of(spec, n, env):
    """pick_path (dsdf_api.hip) for a training call of n points, restated on the host: (family, merged)."""
    if env.get("DSDF_NO_FUSED") == "1":
        return "FAM_LAYERED", False
    merged = "DSDF_NO_MERGE" not in env
    if spec.forward_bf16 or spec.gemm_split:
        return ("FAM_SPLIT" if not spec.forward_bf16 else "FAM_BF16_SPLIT" if spec.gemm_split else "FAM_BF16"), merged
    wmax = max(list(spec.in_dim) + list(spec.out_dim[:-1]))
    narrow = env.get("DSDF_NO_NARROW") != "1" and wmax <= 128
    fam = "FAM_N128" if narrow else "FAM_FP32"
    if not merged or env.get("DSDF_FROWS") == "64":
        return fam, merged
    if narrow and "DSDF_NO_W32" not in env and (wmax <= K_["FWW"] or (wmax <= K_["FWW2"] and "DSDF_NO_W32X2" not in env)):
        return ("FAM_W32" if wmax <= K_["FWW"] else "FAM_W32X2"), merged
    if n <= 32 * G.chip_cus():
        return "FAM_H32", merged
    return fam, merged


def spec_of(route, **over):
    name, _, extra, _, _ = ROUTES[route]
    L, kw = NT.nets()[name]
    return NetSpec(L, **dict(kw, **extra, **over))


def test_the_routes_reach_every_family():
    got = {}
    for r, (name, env, extra, fam, merged) in ROUTES.items():
        assert family_of(spec_of(r), NT.B_SEG * NT.S_SEG, env) == (fam, merged), r
        got.setdefault(fam, []).append(merged)
    assert set(got) == {"FAM_LAYERED", "FAM_FP32", "FAM_SPLIT", "FAM_BF16", "FAM_BF16_SPLIT", "FAM_H32", "FAM_N128", "FAM_W32", "FAM_W32X2"}
    assert False in got["FAM_FP32"] and True in got["FAM_FP32"]          # the un-merged training launch runs too


class Env:
    """The route's switches for the duration of a block; every switch of the list is cleared first and on exit."""

    def __init__(self, monkeypatch, env):
        self.mp, self.env = monkeypatch, env

    def __enter__(self):
        for k in SWITCHES:
            self.mp.delenv(k, raising=False)
        for k, v in self.env.items():
            self.mp.setenv(k, v)

    def __exit__(self, *a):
        for k in SWITCHES:
            self.mp.delenv(k, raising=False)


def tols(spec):
    """tests/test_gpu_parity.py's: the fp32 bounds, or test_random_specs_bf16_forward_vs_oracle's for the bf16 forward."""
    if spec.forward_bf16:
        return dict(loss=1e-4, g=1e-2, g_el=None, fwd=1e-4)
    return dict(loss=1e-5, g=GRAD_TOL, g_el=GRAD_ELEM_TOL, fwd=FWD_TOL)


def hip_step(spec, params, lat, idx, xyz, gt, delta, code_bound=NT.CODE_BOUND, **layout):
    """One dsdf_train_forward_backward (accumulate 0, no Adam) through HipTrainer: (result, trainer, region table of its plan)."""
    tr = HipTrainer(spec, params, lat)
    r = tr.step(idx, xyz, gt, delta=delta, code_bound=code_bound, code_reg=True, lam=NT.LAM, epoch=NT.EPOCH, lr=(5e-4, 1e-3),
                seed=NT.DROP_SEED, want_y=True, do_adam=False, **layout)
    torch.cuda.synchronize()
    rows, _ = _lib.ws_regions()
    return r, tr, rows


def hold(got, ref, t, what):
    """Loss, every decoder gradient tensor (norm-wise and by its worst entry) and dlat against one oracle step."""
    assert abs(got["loss"] - float(ref["loss"])) <= t["loss"] * abs(float(ref["loss"])), (what, got["loss"], float(ref["loss"]))
    for k in ref["grads"]:
        if float(ref["grads"][k].abs().max()) == 0.0:
            assert float(got["grads"][k].abs().max()) == 0.0, (what, k)
            continue
        e, w = rel_err(got["grads"][k], ref["grads"][k]), worst_elem(got["grads"][k], ref["grads"][k])
        assert e <= t["g"] and (t["g_el"] is None or w <= t["g_el"]), (what, k, e, w)
    assert rel_err(got["dlat"], ref["dlat"]) <= t["g"], what


# ---- near-ties --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_near_ties_gradient_of_the_kernels_own_branch(route, monkeypatch):
    name, env, extra, fam, merged = ROUTES[route]
    spec = spec_of(route)
    c = NT.build_case(name, bf16=spec.forward_bf16)
    net, N, t = c["net"], c["xyz"].shape[0], tols(spec)
    for layout in LAYOUTS:
        what = (route, layout)
        with Env(monkeypatch, env):
            r, tr, rows = hip_step(spec, c["params"], c["lat0"], c["idx"], c["xyz"], c["gt"], c["delta"], **layout)
            acts, dp_last = NT.decisions_from_workspace(tr.eng._ws, rows, spec.in_dim, spec.out_dim[:-1], N, merged)
        assert torch.equal(tr.lat.cpu(), c["lat0"]), what                           # rows inside the bound: untouched
        x0 = torch.cat([tr.lat.cpu()[c["idx"]], c["xyz"]], 1)
        an = NT.analyse(net, c["params"], x0, acts, r["y"], c["gt"], c["delta"], c["masks"], dp_last=dp_last, fwd_tol=t["fwd"])
        assert not an["problems"], (what, an["problems"])                           # (b), (c)
        n_flip = NT.flips(c["planted"], an["relu_keep"], c["z_ref"])
        s64 = NT.head_decisions(c["y_ref"], c["gt"].double(), c["delta"])[0]
        tied = c["head"]["tied"]
        print(f"\nnear-ties {route} {'ragged' if layout else 'segment'} ({fam}{'' if merged else ', un-merged'}): {n_flip} of "
              f"{len(c['planted'])} planted entries decided differently from fp64, {int((an['head'][0][tied] != s64[tied]).sum())} of "
              f"{tied.numel()} tied targets with another sign, {int((an['head'][0][tied] == 0).sum())} exact ties; band {an['band']}")   # (d)
        forced = NT.oracle_step(c, decisions=dict(relu_keep=an["relu_keep"], head=an["head"]))
        hold(r, forced, t, what)                                                    # (a)


@pytest.mark.parametrize("name", sorted(NT.nets()))
def test_near_ties_through_the_module_seam(name, monkeypatch):
    """The same planted batch through Decoder autograd in training mode: forward, backward and d_input."""
    from deepsdf_amd.decoder import Decoder
    c = NT.build_case(name)
    net, N = c["net"], c["xyz"].shape[0]
    with Env(monkeypatch, {}):
        dec = Decoder(c["L"], **c["kw"]).cuda()
        dec.load_state_dict(c["params"])
        dec.train(True)
        dec.dropout_seed, dec._fwd_calls = NT.DROP_SEED, -1                          # the planted masks are those of step 0
        x0 = torch.cat([c["lat0"][c["idx"]], c["xyz"]], 1)
        xg = x0.cuda().requires_grad_(True)
        y = dec(xg)
        sign, inside = NT.head_decisions(y.detach().cpu(), c["gt"], c["delta"])
        dy = sign * inside.float() / N
        y.backward(dy.cuda())
        torch.cuda.synchronize()
        rows, _ = _lib.ws_regions()
        eng = dec._engine_for(xg.device)
        acts, _ = NT.decisions_from_workspace(eng._ws, rows, eng.spec.in_dim, eng.spec.out_dim[:-1], N, merged=False)
    an = NT.analyse(net, c["params"], x0, acts, y.detach().cpu(), c["gt"], c["delta"], c["masks"])
    assert not an["problems"], (name, an["problems"])
    print(f"\nnear-ties module seam {name}: {NT.flips(c['planted'], an['relu_keep'], c['z_ref'])} of {len(c['planted'])} planted entries decided "
          f"differently from fp64")
    p64 = NT.dbl(c["params"])
    yo, sv = orc.decoder_forward(net, p64, x0.double(), training=True, masks=c["masks"], relu_keep=an["relu_keep"])
    assert rel_err(y.detach().cpu(), yo) <= FWD_TOL
    go, dx0 = orc.decoder_backward(net, p64, sv, dy.double(), True)
    for pname, p in dec.named_parameters():
        ref = go[pname].reshape(p.shape)
        assert rel_err(p.grad.cpu(), ref) <= GRAD_TOL and worst_elem(p.grad.cpu(), ref) <= GRAD_ELEM_TOL, (name, pname)
    assert rel_err(xg.grad.cpu(), dx0) <= GRAD_TOL and worst_elem(xg.grad.cpu(), dx0) <= GRAD_ELEM_TOL, name


# ---- exact ties -------------------------------------------------------------------------------------------------------------------
_EXACT = {}


def exact_case(name, bf16, use_tanh=None):
    """A normally drawn net and batch of near_ties.nets()[name] (no planting), table rows inside the bound."""
    key = (name, bf16, use_tanh)
    if key not in _EXACT:
        from tests.safe_batch import big_batch
        L, kw = NT.nets()[name]
        kw = dict(kw) if use_tanh is None else dict(kw, use_tanh=use_tanh)
        net = orc.make_net(L, forward_bf16=bf16, **kw)
        seed = 8300 + 10 * sorted(NT.nets()).index(name)
        params = orc.init_params(net, seed)
        lat0 = torch.randn(NT.B_SEG, L, generator=torch.Generator().manual_seed(seed + 1)) / math.sqrt(L)
        lat0 *= torch.clamp(0.9 / lat0.norm(dim=1, keepdim=True), max=1.0)
        idx, xyz, gt = big_batch(NT.B_SEG, NT.S_SEG, seed + 2, kw["geom_dimension"])
        _EXACT[key] = dict(net=net, L=L, kw=kw, params=params, lat0=lat0, idx=idx, xyz=xyz, gt=gt, delta=0.1,
                           masks=orc.dropout_masks(net, NT.DROP_SEED, 0, xyz.shape[0]))
    return _EXACT[key]


def zero_unit_case(name, bf16):
    """exact_case with two units per hidden layer whose effective weight row is zero (g_j = 0 under weight norm, a zero row on a plain
    layer), one with bias +0.0 and one with -0.0, on a batch that is margin-safe for every OTHER unit and for the head."""
    key = ("zero", name, bf16)
    if key in _EXACT:
        return _EXACT[key]
    base = exact_case(name, bf16)
    c = dict(base, params={k: v.clone() for k, v in base["params"].items()}, xyz=base["xyz"].clone(), gt=base["gt"].clone())
    net, units = c["net"], {}
    for l in range(net.n_lin - 1):
        units[l] = (1, net.layers[l].out_dim - 2)
        for j, b in zip(units[l], (0.0, -0.0)):
            if net.layers[l].weight_norm:
                c["params"][f"lin{l}.parametrizations.weight.original0"][j] = 0.0
            else:
                c["params"][f"lin{l}.weight"][j] = 0.0
            c["params"][f"lin{l}.bias"][j] = b
    gen = torch.Generator().manual_seed(8399)
    x_lat = c["lat0"].double()[c["idx"]]
    for _ in range(12):                     # tests/safe_batch.py's re-drawing, with the zero units left out of the ReLU margin
        y, _, zs, _ = NT.pre_activations(net, NT.dbl(c["params"]), torch.cat([x_lat, c["xyz"].double()], 1), c["masks"])
        d = torch.clamp(y, -c["delta"], c["delta"]) - torch.clamp(c["gt"].double(), -c["delta"], c["delta"])
        risky = (((y.abs() - c["delta"]).abs() < 2e-5) | ((d != 0) & (d.abs() < 2e-5))).reshape(-1)
        for l, z in enumerate(zs):
            za = z.abs().clone()
            za[:, list(units[l])] = float("inf")
            risky |= za.amin(dim=1) < 1e-6
            assert bool((z[:, list(units[l])] == 0).all())
        if not bool(risky.any()):
            break
        k = int(risky.sum())
        c["xyz"][risky] = torch.rand(k, c["xyz"].shape[1], generator=gen) * 2 - 1
        c["gt"][risky] = (torch.rand(k, 1, generator=gen) - 0.5) * 0.4
    else:
        raise RuntimeError("could not build a margin-safe batch")
    c["units"] = units
    _EXACT[key] = c
    return c


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_exact_tie_a_unit_that_is_zero_everywhere(route, monkeypatch):
    """relu'(0) = 0: the unit's stored activation, its bias gradient, its g gradient and its row of the v / weight gradient are 0,
    compared with == 0; everything else against the oracle as usual."""
    name, env, extra, fam, merged = ROUTES[route]
    spec = spec_of(route)
    c = zero_unit_case(name, spec.forward_bf16)
    net, N, t = c["net"], c["xyz"].shape[0], tols(spec)
    ref = NT.oracle_step(c)
    for layout in LAYOUTS:
        what = (route, layout)
        with Env(monkeypatch, env):
            r, tr, rows = hip_step(spec, c["params"], c["lat0"], c["idx"], c["xyz"], c["gt"], c["delta"], **layout)
            acts, dp_last = NT.decisions_from_workspace(tr.eng._ws, rows, spec.in_dim, spec.out_dim[:-1], N, merged)
        for l, (ja, jb) in c["units"].items():
            for j in (ja, jb):
                if acts[l] is not None:
                    assert bool((acts[l][:, j] == 0).all()), (what, l, j, "stored activation")
                else:
                    assert bool((dp_last[:, j] == 0).all()), (what, l, j, "gradient in front of the ReLU")
                assert float(r["grads"][f"lin{l}.bias"][j]) == 0.0, (what, l, j, "bias gradient")
                if net.layers[l].weight_norm:
                    assert float(r["grads"][f"lin{l}.parametrizations.weight.original0"][j]) == 0.0, (what, l, j, "g gradient")
                    assert bool((r["grads"][f"lin{l}.parametrizations.weight.original1"][j] == 0).all()), (what, l, j, "v gradient row")
                else:
                    assert bool((r["grads"][f"lin{l}.weight"][j] == 0).all()), (what, l, j, "weight gradient row")
        hold(r, ref, t, what)


def _spread_targets(N, delta, side):
    """Targets around the clamp edge the output sits on (side +1: y = +delta, -1: y = -delta): beyond the edge, on it, one ulp inside
    it, well inside -- a quarter of the batch each."""
    e = torch.tensor(side * delta, dtype=torch.float32)
    inner = torch.nextafter(e, torch.tensor(0.0))
    gt = torch.empty(N, 1)
    gt[0::4] = float(e) * 1.5
    gt[1::4] = e
    gt[2::4] = inner
    gt[3::4] = torch.linspace(-0.7, 0.7, len(gt[3::4])).reshape(-1, 1) * float(delta)
    return gt


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_exact_tie_the_output_on_the_clamp_edge(route, monkeypatch):
    """The last Linear's effective weight is zero, so y is one float y* at every point; delta = |y*| puts every point ON a clamp edge.
    clamped_l1 (inclusive edges, sign(0) = 0) gives the decisions exactly; the oracle forced onto them gives loss and gradients, and
    the last bias gradient has the closed form (1 - y*^2) [* (1 - t1^2)] * sum(sign) / n_norm."""
    name, env, extra, fam, merged = ROUTES[route]
    spec0 = spec_of(route)
    t = tols(spec0)
    for use_tanh in (False, True):
        spec = spec_of(route, use_tanh=use_tanh)
        base = exact_case(name, spec.forward_bf16, use_tanh)
        net, N = base["net"], base["xyz"].shape[0]
        last = net.n_lin - 1
        for b in (0.3, -0.3):
            what = (route, use_tanh, b)
            c = dict(base, params={k: v.clone() for k, v in base["params"].items()})
            if net.layers[last].weight_norm:
                c["params"][f"lin{last}.parametrizations.weight.original0"][:] = 0.0
            else:
                c["params"][f"lin{last}.weight"][:] = 0.0
            c["params"][f"lin{last}.bias"][:] = b
            with Env(monkeypatch, env):
                r0, _, _ = hip_step(spec, c["params"], c["lat0"], c["idx"], c["xyz"], c["gt"], 0.1)
                ys = r0["y"].reshape(-1)
                assert bool((ys.view(torch.int32) == ys.view(torch.int32)[0]).all()), (what, "y differs between points")
                ystar = float(ys[0])
                delta, side = abs(ystar), (1 if b > 0 else -1)
                assert ystar * side > 0
                c["gt"], c["delta"] = _spread_targets(N, delta, side), delta
                r, _, _ = hip_step(spec, c["params"], c["lat0"], c["idx"], c["xyz"], c["gt"], delta)
            assert torch.equal(r["y"].reshape(-1), ys), what
            sign, inside = NT.head_decisions(ys.reshape(-1, 1), c["gt"], delta)              # the specification, on the device's own y*
            assert bool(inside.all()) and int((sign == 0).sum()) == N // 2 and int((sign == side).sum()) == N // 2, what
            forced = NT.oracle_step(c, decisions=dict(head=(sign.double(), inside)))
            hold(r, forced, t, what)
            t1 = math.tanh(b)
            closed = (1.0 - ystar * ystar) * ((1.0 - t1 * t1) if use_tanh else 1.0) * float(sign.sum()) / N
            got = float(r["grads"][f"lin{last}.bias"].reshape(-1)[0])
            print(f"\nclamp edge {route} use_tanh {use_tanh} b {b}: y* {ystar!r}, last bias gradient {got!r}, closed form {closed!r}, "
                  f"{abs(got - closed) / (abs(closed) * 2.0 ** -23):.2f} ulp")
            assert abs(got - closed) <= 4 * 2.0 ** -23 * abs(closed), what


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_exact_tie_a_latent_row_on_the_bound(route, monkeypatch):
    """renorm_rows_ (torch's norm > max_norm): a row whose norm IS CodeBound, and the row one ulp below, come back bit for bit; the rows
    above are scaled within the counted bound of operating_points.renorm_roundings; the row no segment looks up stays as it is.
    Segment mode (the hoist kernel's renorm) and the general path (latent_renorm_kernel)."""
    name, env, extra, fam, merged = ROUTES[route]
    spec = spec_of(route)
    c = exact_case(name, spec.forward_bf16)
    L = c["L"]
    k = renorm_roundings(L)
    for bound in (1.0, 0.5):
        cb = torch.tensor(bound, dtype=torch.float32)
        lat = torch.zeros(5, L)
        lat[0, 0] = cb
        lat[1, 0] = torch.nextafter(cb, torch.tensor(float("inf")))
        lat[2, 0] = torch.nextafter(cb, torch.tensor(0.0))
        lat[3] = torch.randn(L, generator=torch.Generator().manual_seed(5)) * bound
        lat[3] *= 1.7 * bound / lat[3].norm()
        lat[4, 1] = 2.0 * bound                                                  # above the bound, never looked up
        ref = lat.double().clone()
        orc.renorm_rows_(ref, c["idx"], bound)
        assert torch.equal(ref[0], lat[0].double()) and torch.equal(ref[2], lat[2].double()) and not torch.equal(ref[1], lat[1].double())
        for layout in LAYOUTS:
            what = (route, bound, layout)
            with Env(monkeypatch, env):
                _, tr, _ = hip_step(spec, c["params"], lat, c["idx"], c["xyz"], c["gt"], 0.1, code_bound=bound, **layout)
            after = tr.lat.cpu()
            for row in (0, 2, 4):
                assert torch.equal(after[row].view(torch.int32), lat[row].view(torch.int32)), (what, row, after[row], lat[row])
            for row in (1, 3):
                assert not torch.equal(after[row], lat[row]), (what, row, "not scaled")
                err = (after[row].double() - ref[row]).abs()
                assert bool((err <= O.gamma(k) * ref[row].abs()).all()), (what, row, after[row], ref[row])
