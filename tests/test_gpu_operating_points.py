"""-m gpu: the training step AWAY from the one set of constants every other test runs at.

Two optimiser steps at every operating point of tests/operating_points.py against the float64 oracle, on batches whose targets are
chosen from the oracle's own y so that every region of the loss head is populated, along every route the library can take:

  route        net      selected by                               renorm site             loss head
  h32          main     default (small batch: 32-point workgroups) hoist kernel / latent_renorm_kernel   fused
  n128         main     DSDF_FROWS=64 (narrow-net kernels)         "                       fused
  fp32         main     DSDF_FROWS=64 DSDF_NO_NARROW=1             "                       fused
  layered      main     DSDF_NO_FUSED=1                            latent_renorm_kernel    last_layer_kernel
  variant      variant  an xyz_in_all net (layer-by-layer only)    latent_renorm_kernel    last_layer_kernel
  w32          w32      default (every layer <= 32 wide)           hoist / latent_renorm   fused (wave-private)
  w32_off      w32      DSDF_NO_W32=1                              "                       fused (four-wave)
  gemm_split   main     NetSpec(gemm_split=True)                   "                       fused, fp32 bounds
  forward_bf16 main     NetSpec(forward_bf16=True), once           "                       against the oracle's own bf16 emulation
  one-call     main     Engine.train_step (no clip, no split)      "                       also against the two-call path
  split 2      main     batch_split = 2 (accumulate, row_offset)

each in segment mode (4 scenes x 64 points: the workspace plan has a hoistU region) and on a ragged batch (force_ragged, 40 + 33 + 40 +
40 + 7 points with one scene in two segments: it has none).
The hoistU region is the one thing about the route a test can ask the library: the ABI has no query for the kernel family a call ran, so
the family is selected, not asserted, with the switches tests/test_gpu_parity.py and tests/test_gpu_breakpoints.py select it with.

Bounds: tests/test_gpu_parity.py's constants and test_gpu_breakpoints._tols, nothing else: the fp32 CPU oracle sits below a quarter of
every one of them on every case (tests/test_operating_points_cpu.py asserts it), so no case carries an allowance.  The renormed table
is held element by element to the counted bound of operating_points.renorm_roundings, rows the spec leaves alone bit for bit.

Adam away from torch's betas and eps: a first step from zero moments hides both betas, so every Adam form runs from aged moments at a
late step against optim_numpy.adam_ref(b1=, b2=, eps=) of the gradient it consumed, through tests/test_gpu_optim_tail.py's own
(parametrised) helpers, at that file's counted bounds.
"""
import pytest
import torch

from deepsdf_amd import _lib
from tests import operating_points as OP
from tests import optim_numpy as O
from tests import test_gpu_optim_tail as T
from tests.golden_io import rel_err, worst_elem
from tests.hip_helpers import HipTrainer, spec_from_meta
from tests.test_gpu_breakpoints import _tols
from tests.test_gpu_parity import FWD_TOL, GRAD_ELEM_TOL, GRAD_TOL, PARAM_TOL, Y_ROW_TOL

pytestmark = pytest.mark.gpu
assert (FWD_TOL, GRAD_TOL, GRAD_ELEM_TOL, PARAM_TOL) == (OP.FWD_TOL, OP.GRAD_TOL, OP.GRAD_ELEM_TOL, OP.PARAM_TOL)      # what the CPU proof used

SWITCHES = ("DSDF_FROWS", "DSDF_NO_NARROW", "DSDF_NO_W32", "DSDF_NO_FUSED")
# route -> (net kind, environment, NetSpec flags, fused?)
ROUTES = {
    "h32": ("main", {}, {}, True),
    "n128": ("main", {"DSDF_FROWS": "64"}, {}, True),
    "fp32": ("main", {"DSDF_FROWS": "64", "DSDF_NO_NARROW": "1"}, {}, True),
    "layered": ("main", {"DSDF_NO_FUSED": "1"}, {}, False),
    "variant": ("variant", {}, {}, False),
    "w32": ("w32", {}, {}, True),
    "w32_off": ("w32", {"DSDF_NO_W32": "1"}, {}, True),
    "gemm_split": ("main", {}, {"gemm_split": True}, True),
}
POINT_NAMES = [p.name for p in OP.POINTS]


class Misses:
    """Every comparison of a test is made and printed; the misses are reported together."""

    def __init__(self):
        self.fails, self.n, self.worst = [], 0, {}

    def check(self, qty, val, tol, where):
        self.n += 1
        if not val <= tol:
            self.fails.append(f"{where}: {qty} {val:.3e} > {tol:.1e}")
        if not val / tol <= self.worst.get(qty, (-1.0, ""))[0]:
            self.worst[qty] = (val / tol, where)

    def same(self, what, ok, where):
        self.n += 1
        if not ok:
            self.fails.append(f"{where}: {what}")

    def done(self, title):
        print(f"\n{title}: {self.n} comparisons; worst figure / bound per quantity:")
        for q, (v, w) in sorted(self.worst.items()):
            print(f"    {q:<28s} {v:7.3f}   at {w}")
        assert not self.fails, f"{len(self.fails)} of {self.n} comparisons miss their bound:\n" + "\n".join(self.fails[:40])


def _spec(c, **flags):
    return spec_from_meta(dict(L=c.L, net_specs=dict(c.kw, **flags)))


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def hold_renormed_table(book, before, after, c, where):
    """The table a forward leaves against the spec applied to the table it found (the device's own float32 rows, in float64): scaled
    rows within gamma(k) |entry| (operating_points.renorm_roundings), every other row -- below the bound, not looked up, or any row
    when the bound is None or <= 0 -- bit for bit as it was."""
    ref = before.double().clone()
    idx = torch.tensor(sorted(set(c.scenes)))
    OP.orc.renorm_rows_(ref, idx, c.code_bound)
    k = OP.renorm_roundings(c.L)
    for r in range(OP.TABLE_ROWS):
        if torch.equal(ref[r], before[r].double()):
            book.same(f"table row {r} is not scaled by the spec but changed", torch.equal(after[r], before[r]), where)
        else:
            err = (after[r].double() - ref[r]).abs() / (O.gamma(k) * ref[r].abs())
            book.check("renormed row (counted)", float(err.max()), 1.0, f"{where} row {r}")
            book.same(f"table row {r} was not scaled", not torch.equal(after[r], before[r]), where)


def compare_step(book, tol, got, ref, where, state=True):
    """One step's outputs, both moments of every tensor and (state) the post-step parameters and table against one step of the oracle."""
    book.check("loss", abs(got["loss"] - float(ref["loss"])) / abs(float(ref["loss"])), tol["loss"], where)
    if got.get("y") is not None:
        book.check("sdf", rel_err(got["y"], ref["y"].reshape(-1)), tol["y"], where)
        if tol["y_el"] is not None:
            book.check("sdf worst row", worst_elem(got["y"], ref["y"].reshape(-1)), tol["y_el"], where)
    raw = OP.raw_grads(ref)
    if got.get("grads") is not None:
        book.same("gradient tensor names", set(got["grads"]) == set(raw), where)
        for k in raw:
            book.check("gradients", rel_err(got["grads"][k], raw[k]), tol["g"], f"{where} {k}")
            if tol["g_el"] is not None:
                book.check("gradients worst entry", worst_elem(got["grads"][k], raw[k]), tol["g_el"], f"{where} {k}")
    if got.get("dlat") is not None:
        book.check("dlat", rel_err(got["dlat"], ref["dlat"]), tol["g"], where)
        if tol["g_el"] is not None:
            book.check("dlat worst entry", worst_elem(got["dlat"], ref["dlat"]), tol["g_el"], where)
    if got.get("grad_norm") is not None:
        book.check("gradient norm", abs(got["grad_norm"] - float(ref["grad_norm"])) / float(ref["grad_norm"]), tol["g"], where)
    for k in ref["params"]:
        if state:
            book.check("parameters after the step", rel_err(got["params"][k], ref["params"][k]), tol["p"], f"{where} {k}")
        book.check("exp_avg", rel_err(got["m"][k], ref["m"][k]), tol["m"], f"{where} {k}")
        book.check("exp_avg_sq", rel_err(got["v"][k], ref["v"][k]), tol["v"], f"{where} {k}")
    if state:
        book.check("latent table after the step", rel_err(got["latents"], ref["latents"]), tol["p"], where)
    book.check("latent exp_avg", rel_err(got["m_lat"], ref["m_lat"]), tol["m"], where)
    book.check("latent exp_avg_sq", rel_err(got["v_lat"], ref["v_lat"]), tol["v"], where)


def _state(tr):
    return dict(params=tr.params(), m=tr.adam_m(), v=tr.adam_v(), latents=tr.lat.cpu().clone(), m_lat=tr.lat_m.cpu().clone(),
                v_lat=tr.lat_v.cpu().clone())


def run_two_call(c, spec, book, where, force_ragged, fused):
    """train_forward_backward per chunk (+ grad_norm) + adam_step, c.steps times; returns the per-step results.  forward_bf16: the
    bounds test_gpu_parity states for it cover the loss, the forward and the gradients; both moments, linear and quadratic in the gradient,
    are held to the 1e-2 / 2e-2 test_gpu_breakpoints._tols names for them; the parameters and the table after the step are not compared
    (a first Adam step is lr x sign(g) wherever |g| >> eps: two bf16 forwards that differ in one ReLU differ there by whole steps)."""
    tr = HipTrainer(spec, c.params, c.lat0)
    bf16 = c.net_bf16 is not None
    tol = _tols(bf16)
    out = []
    for s, (idx, xyz, gt) in enumerate(c.batches):
        before = tr.lat.cpu().clone()
        r = tr.step(idx, xyz, gt, delta=c.deltas[s], code_bound=c.code_bound, code_reg=True, lam=c.reg_coef, epoch=100, lr=c.lr,
                    batch_split=c.batch_split, grad_clip=c.grad_clip[s], seed=OP.DROP_SEED, want_y=True, do_adam=False,
                    force_ragged=force_ragged, n_norm=c.n_norm)
        names = [x[0] for x in _lib.ws_regions()[0]]             # the last plan laid out: the step's, or dsdf_grad_norm's when clipping
        if c.grad_clip[s] is None:
            book.same(f"segment mode (a hoistU region) expected {fused and not force_ragged}: {names}",
                      ("hoistU" in names) == (fused and not force_ragged), where)
        hold_renormed_table(book, before, tr.lat.cpu(), c, f"{where} step {s}")
        absent = [j for j in range(OP.TABLE_ROWS) if j not in c.scenes]
        book.same("latent gradient rows of absent scenes are not zero", not bool(r["dlat"][absent].any()), where)
        tr.eng.adam_step(tr.lat, tr.dlat, tr.lat_m, tr.lat_v, c.lr[0], c.lr[1], clip=c.grad_clip[s] is not None, betas=c.point.betas,
                         eps=c.point.eps)
        r.update(_state(tr))
        compare_step(book, tol, r, c.reference()[s], f"{where} step {s}", state=not bf16)
        out.append(r)
    return out


def run_one_call(c, spec, book, where, force_ragged, two_call):
    """Engine.train_step, c.steps times, against the oracle and (first step: same starting state) against the two-call path."""
    from deepsdf_amd.engine import make_segments
    tr = HipTrainer(spec, c.params, c.lat0)
    tol = _tols(False)
    for s, (idx, xyz, gt) in enumerate(c.batches):
        sc, so = make_segments(idx.cuda())
        tr.eng.train_step(tr.lat, tr.dlat, tr.lat_m, tr.lat_v, sc, so, xyz.cuda().contiguous(), gt.reshape(-1).cuda().contiguous(),
                          n_norm=c.n_norm, clamp_dist=c.deltas[s], reg_coef=c.reg_coef, code_bound=c.code_bound, lr_decoder=c.lr[0],
                          lr_latent=c.lr[1], seed=OP.DROP_SEED, seg_len=0 if force_ragged else c.lens[0], betas=c.point.betas, eps=c.point.eps)
        r = dict(loss=float(tr.eng.loss.item()), dlat=tr.dlat.cpu().clone(), **_state(tr))
        compare_step(book, tol, r, c.reference()[s], f"{where} step {s}")
        if s == 0:                                  # (later steps start from states that differ by the first step's roundings)
            t = two_call[0]
            book.check("one-call loss vs two-call", abs(r["loss"] - t["loss"]) / abs(t["loss"]), 1e-6, where)
            for k in t["params"]:
                book.check("one-call parameters vs two-call", rel_err(r["params"][k], t["params"][k]), 1e-6, f"{where} {k}")
                book.check("one-call exp_avg vs two-call", rel_err(r["m"][k], t["m"][k]), 1e-6, f"{where} {k}")
                book.check("one-call exp_avg_sq vs two-call", rel_err(r["v"][k], t["v"][k]), 1e-6, f"{where} {k}")
            book.check("one-call latent table vs two-call", rel_err(r["latents"], t["latents"]), 1e-6, where)
            book.same("one-call dlat differs from the two-call path's", torch.equal(r["dlat"], t["dlat"]), where)


@pytest.mark.parametrize("name", POINT_NAMES)
def test_every_route_at_the_operating_point_vs_oracle(name, monkeypatch):
    """Every route of the module's table, segment mode and ragged, two optimiser steps at one operating point against the fp64 oracle:
    loss, sdf, every gradient tensor (norm-wise and by its worst entry), dlat, the renormed table element by element, parameters,
    moments and table after each step; the one-call step where the point has neither clipping nor a split."""
    p = OP.BY_NAME[name]
    book = Misses()
    try:
        for route, (kind, env, flags, fused) in ROUTES.items():
            for layout in ("segment", "ragged"):
                if route == "variant" and layout == "segment":
                    continue                        # (a layer-by-layer net has no segment mode: the main net's layered route shows it)
                c = OP.get_case(name, kind, layout)
                _set_env(monkeypatch, env)
                where = f"{name} {route} {layout}"
                two = run_two_call(c, _spec(c, **flags), book, where, layout == "ragged", fused)
                if p.clip_factor is None and route in ("h32", "fp32", "w32"):
                    run_one_call(c, _spec(c, **flags), book, where + " one-call", layout == "ragged", two)
    finally:
        _set_env(monkeypatch, {})
    book.done(name)


def test_the_regulariser_carries_weight_in_the_loss_at_lambda_1e_2():
    """At lambda 1e-2 the regulariser is a visible share of the loss the kernels report (the 1e-5 bound on the loss sees a 1 % error of
    the term), at the reference's 1e-4 it is not: why the points with lambda 1e-2 exist."""
    for name, lo in (("lam1e-2_epoch37", 0.02), ("lam1e-2_epoch130", 0.02), ("n_norm_3N", 0.02)):
        c = OP.get_case(name, "main", "segment")
        z = c.lat_ren[0][c.batches[0][0]]
        share = float(OP.orc.code_regulariser(z, c.reg_coef, 100, c.n_norm)[0]) / float(c.results[0]["loss"])
        assert share >= lo, (name, share)
        tr = HipTrainer(_spec(c), c.params, c.lat0)
        idx, xyz, gt = c.batches[0]
        with_reg = tr.step(idx, xyz, gt, delta=c.deltas[0], code_bound=c.code_bound, code_reg=True, lam=c.reg_coef, epoch=100, lr=c.lr,
                           seed=OP.DROP_SEED, do_adam=False, n_norm=c.n_norm)["loss"]
        tr = HipTrainer(_spec(c), c.params, c.lat0)
        without = tr.step(idx, xyz, gt, delta=c.deltas[0], code_bound=c.code_bound, code_reg=False, lam=0.0, epoch=100, lr=c.lr,
                          seed=OP.DROP_SEED, do_adam=False, n_norm=c.n_norm)["loss"]
        assert abs((with_reg - without) / with_reg - share) <= 1e-4, (name, with_reg, without, share)


def test_forward_bf16_at_an_operating_point_vs_its_own_emulation():
    """forward_bf16 once, at code_bound 0.6 / delta 0.03, against the oracle's bf16-forward step in fp32 at test_gpu_parity's bounds for
    it (1e-4 forward and loss, 1e-2 gradients; exp_avg 1e-2 and exp_avg_sq 2e-2 as test_gpu_breakpoints._tols names them).  The renorm bound is the fp32 one:
    the hoist kernel rounds the table to bf16 only on its way into the GEMM."""
    c = OP.get_case(*OP.BF16_CASE)
    book = Misses()
    for layout_ragged in (False, True):
        run_two_call(c, _spec(c, forward_bf16=True), book, f"{c.id} {'ragged' if layout_ragged else 'segment'}", layout_ragged, True)
    book.done(c.id)


@pytest.mark.parametrize("args", OP.SPLIT_CASES, ids=lambda a: f"{a[0]}-{a[2]}")
def test_batch_split_2_at_an_operating_point_vs_oracle(args, monkeypatch):
    """batch_split = 2 (the second chunk accumulates, its dropout rows continue at row_offset) on the fused and the layer-by-layer
    kernels: the renorm of the second chunk must find the first chunk's rows already scaled, n_norm is the whole step's."""
    c = OP.get_case(*args)
    book = Misses()
    try:
        for route in ("h32", "fp32", "layered"):
            _set_env(monkeypatch, ROUTES[route][1])
            run_two_call(c, _spec(c), book, f"{c.id} {route}", c.layout == "ragged", ROUTES[route][3])
    finally:
        _set_env(monkeypatch, {})
    book.done(c.id)


# ---- Adam away from torch's betas and eps: every form, from aged moments at late steps ---------------------------------------------------
ADAM_POINTS = {"betas_eps": ((0.8, 0.95), 1e-5), "eps_only": ((0.9, 0.999), 1e-5)}
LATE_STEPS = (2, 1000)


@pytest.mark.parametrize("n", [257, T.CAP + 1])
@pytest.mark.parametrize("point", sorted(ADAM_POINTS))
def test_flat_adam_forms_off_the_default_constants(point, n, tiny_engine_op):
    """dsdf_adam_latent_only (Engine.adam_latents' entry), dsdf_adam_latent_sched and the ride on dsdf_adam_step."""
    betas, eps = ADAM_POINTS[point]
    assert (betas, eps) == (OP.BY_NAME[point].betas, OP.BY_NAME[point].eps)
    T.flat_adam_forms(n, tiny_engine_op, betas=betas, eps=eps, steps=LATE_STEPS)


@pytest.fixture(scope="module")
def tiny_engine_op():
    from deepsdf_amd.engine import Engine
    from deepsdf_amd.net import NetSpec
    eng = Engine(NetSpec(4, [32, 32], 3, norm_layers=[0, 1], weight_norm=True), "cuda")
    eng.init_like_reference(generator=torch.Generator().manual_seed(1))
    return eng


@pytest.mark.parametrize("clip", ["noclip", "coef<1"])
@pytest.mark.parametrize("point", sorted(ADAM_POINTS))
def test_decoder_arena_adam_off_the_default_constants(point, clip):
    """adam_rows_kernel with and without the clip coefficient (and adam_kernel on LayerNorm parameters)."""
    betas, eps = ADAM_POINTS[point]
    for net in ("wn_rows_1145", "layernorm_40_64"):
        T.decoder_arena_adam(net, clip, betas=betas, eps=eps, steps=LATE_STEPS)


@pytest.mark.parametrize("mode", ["segment", "ragged"])
@pytest.mark.parametrize("point", sorted(ADAM_POINTS))
def test_fused_finalize_adam_off_the_default_constants(point, mode):
    """finalize_row_wave<K> + Adam on the fused path (the sentinel in the gradient arena survives), the ride and the latent Adam of
    dsdf_train_step, and a net that falls back to dsdf_adam_step."""
    betas, eps = ADAM_POINTS[point]
    for net in ("in<=64_w40", "in<=128_w72", "skip_layer", "falls_back_w520"):
        T.fused_finalize_adam(net, mode, betas=betas, eps=eps)
