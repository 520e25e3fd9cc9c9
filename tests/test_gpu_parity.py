"""-m gpu: the HIP path (through the C ABI) against the reference-generated goldens and the oracle.

Tolerances (north_star): forward SDF <= 1e-5 rel, gradients <= 1e-4 rel (norm-wise), post-Adam state <= 1e-5 rel."""
import math

import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests.golden_io import Golden, rel_err, worst_elem
from tests.hip_helpers import HipTrainer, spec_from_meta
from tests.safe_batch import big_batch, safe_batch

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL, PARAM_TOL = 1e-5, 1e-4, 1e-5
# element-wise companions of the norm-wise bounds (worst row of y against max|y|, worst entry of a gradient tensor against that
# tensor's max|g|): same figures as north_star's tolerances.  Post-Adam parameters: an entry whose gradient is ~Adam's eps
# (1e-8) moves by lr * g / (|g| + eps), which turns a 1e-11 absolute gradient difference into 5e-7 of parameter -- the entry-wise
# bound is therefore stated against the step size lr, not against max|p|: no entry may differ by more than 0.2 % of one Adam step
# per step taken (measured on MI355X, profiles/r03_worst_element.log: y rows 2e-7, gradient entries 5e-6, parameter entries 8e-4 of a
# step).  gemm_split's gradient entries are 7e-6 of their tensor's max instead of 8e-7 (its dropped cross terms scale with the sum of
# |products|, not with the partial sums), which the eps-sized Adam entries turn into 9e-3 of a step: its own bound, 2 %.
Y_ROW_TOL, GRAD_ELEM_TOL, PARAM_STEP_FRAC, PARAM_STEP_FRAC_SPLIT = 1e-5, 1e-4, 2e-3, 2e-2

TRAIN_CASES = ["g1a_tiny_full", "g1b_lastnorm_tanh", "g1c_plain_clip", "g2_8x512_slice", "g3a_dropout_tiny",
               "g3b_dropout_8x512", "g4_batch_split2",
               # Decoder variants no shipped spec uses (deep_sdf_decoder.py:90-91, 79-82, 60-65/97-103): reference-generated goldens
               "g11a_xyz_in_all", "g11b_latent_dropout", "g11c_layer_norm",
               # away from CodeBound 1.0 / ClampingDistance 0.1 / lambda 1e-4 / torch's Adam defaults
               "g14a_off_point_tight", "g14b_off_point_loose"]


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_golden_train_cases(name):
    _golden_train_case(name, gemm_split=False)


@pytest.mark.parametrize("name", ["g1a_tiny_full", "g1b_lastnorm_tanh", "g2_8x512_slice", "g3b_dropout_8x512", "g4_batch_split2"])
def test_golden_train_cases_gemm_split(name):
    """The reference-generated goldens with NetworkSpecs gemm_split (the fused kernels' GEMMs as 6 bf16 MFMAs on 3-way cut fp32
    operands): the same tolerances."""
    _golden_train_case(name, gemm_split=True)


def _golden_train_case(name, gemm_split):
    g = Golden(name)
    m = g.meta
    spec = spec_from_meta(dict(m, net_specs=dict(m["net_specs"], gemm_split=gemm_split)))
    net = orc.make_net(m["L"], **m["net_specs"])
    params = g.group("params0") if m["store"] == "full" else orc.init_params(net, m["seed"])
    tr = HipTrainer(spec, params, g.get("lat0/w"))
    for si in range(m["n_steps"]):
        i = g.group(f"step{si}/in")
        r = tr.step(i["idx"], i["xyz"], i["gt"], delta=m["delta"], code_bound=m["code_bound"], code_reg=m["code_reg"],
                    lam=m["lam"], epoch=m["epoch"], lr=m["lr"], batch_split=m["batch_split"], grad_clip=m["grad_clip"],
                    seed=m["drop_seed"], want_y=True, betas=tuple(m.get("betas", (0.9, 0.999))), eps=m.get("eps", 1e-8))
        o = g.group(f"step{si}/out")
        assert rel_err(r["y"], o["y"]) <= FWD_TOL, (name, si, "y")
        assert worst_elem(r["y"], o["y"]) <= Y_ROW_TOL, (name, si, "y worst row")
        assert abs(r["loss"] - float(o["loss"])) <= 1e-5 * abs(float(o["loss"])) + 1e-9, (name, si, "loss")
        assert rel_err(r["dlat"], g.get(f"step{si}/dlat/w")) <= GRAD_TOL, (name, si, "dlat")
        for k, ref in g.group(f"step{si}/grads").items():
            if m["grad_clip"] is None:
                assert rel_err(r["grads"][k], ref) <= GRAD_TOL, (name, si, k)
                assert worst_elem(r["grads"][k], ref) <= GRAD_ELEM_TOL, (name, si, k, "worst entry")
        if m["grad_clip"] is not None:
            assert abs(r["grad_norm"] - float(o["grad_norm"])) <= 1e-4 * float(o["grad_norm"])
        for k, ref in g.group(f"step{si}/grads_fro").items():
            assert abs(float(r["grads"][k].double().norm()) - float(ref)) <= GRAD_TOL * float(ref), (name, si, k)
        for k, ref in g.group(f"step{si}/grads_corner").items():
            scale = float(r["grads"][k].abs().max())
            assert float((r["grads"][k][:8, :8] - ref).abs().max()) <= GRAD_TOL * scale, (name, si, k)
        P = tr.params()
        for k, ref in g.group(f"step{si}/params_after").items():
            assert rel_err(P[k], ref) <= PARAM_TOL, (name, si, k)
        for k, ref in g.group(f"step{si}/params_after_fro").items():
            assert abs(float(P[k].double().norm()) - float(ref)) <= PARAM_TOL * float(ref), (name, si, k)
        assert rel_err(tr.lat.cpu(), g.get(f"step{si}/lat_after/w")) <= PARAM_TOL, (name, si, "lat")
        am, av = tr.adam_m(), tr.adam_v()
        for k, ref in g.group(f"step{si}/adam_m").items():
            mine = tr.lat_m.cpu() if k == "latent" else am[k]
            assert rel_err(mine, ref) <= GRAD_TOL, (name, si, "m", k)
        for k, ref in g.group(f"step{si}/adam_v").items():
            mine = tr.lat_v.cpu() if k == "latent" else av[k]
            assert rel_err(mine, ref) <= 2 * GRAD_TOL, (name, si, "v", k)


@pytest.mark.parametrize("name", ["g8_eval_8x512", "g8_eval_6x128"])
def test_golden_eval_forward(name):
    from deepsdf_amd.engine import Engine
    g = Golden(name)
    net = orc.make_net(g.meta["L"], **g.meta["net_specs"])
    eng = Engine(spec_from_meta(g.meta))
    eng.load_params(orc.init_params(net, g.meta["seed"]))
    y = eng.decode(g.get("in/x").cuda())
    assert rel_err(y.cpu().reshape(-1), g.get("out/y")) <= FWD_TOL


@pytest.mark.parametrize("name", ["g8_eval_8x512", "g8_eval_6x128"])
def test_decode_latent_single_code(name):
    """dsdf_decode_latent (ONE code for all points, its products hoisted) == dsdf_decode on the materialised [n, L+G] input
    == the oracle, for n off the 64 grid; and deep_sdf.utils.decode_sdf takes that path in eval mode."""
    from deepsdf_amd.engine import Engine
    from deepsdf_amd.decoder import Decoder
    from deepsdf_amd.utils import decode_sdf
    g = Golden(name)
    L = g.meta["L"]
    net = orc.make_net(L, **g.meta["net_specs"])
    params = orc.init_params(net, g.meta["seed"])
    eng = Engine(spec_from_meta(g.meta))
    eng.load_params(params)
    gen = torch.Generator().manual_seed(3)
    z = torch.randn(L, generator=gen) / math.sqrt(L)
    for n in (1, 63, 1000, 70001):
        xyz = torch.rand(n, 3, generator=gen) * 2 - 1
        x = torch.cat([z.expand(n, -1), xyz], 1)
        yo = orc.decoder_forward(net, params, x, training=False)[0].reshape(-1)
        yl = eng.decode_latent(z.cuda(), xyz.cuda()).cpu().reshape(-1)
        yd = eng.decode(x.cuda()).cpu().reshape(-1)
        assert rel_err(yl, yo) <= FWD_TOL and rel_err(yl, yd) <= FWD_TOL, n
    dec = Decoder(L, **g.meta["net_specs"]).cuda().eval()
    dec.load_state_dict({k: v for k, v in params.items()})
    with torch.no_grad():
        ys = decode_sdf(dec, z.cuda()[None, :], xyz.cuda())
    assert ys.shape == (xyz.shape[0], 1) and rel_err(ys.cpu().reshape(-1), yo) <= FWD_TOL
    # config 5: the same entry point with the bf16 forward (hoisted products on bf16-rounded operands) against the oracle's
    # bf16 emulation, and against the materialised-input bf16 path
    netb = orc.make_net(L, forward_bf16=True, **g.meta["net_specs"])
    engb = Engine(spec_from_meta(dict(L=L, net_specs=dict(g.meta["net_specs"], forward_bf16=True))))
    engb.load_params(params)
    x = torch.cat([z.expand(xyz.shape[0], -1), xyz], 1)
    yob = orc.decoder_forward(netb, params, x, training=False)[0].reshape(-1)
    ylb = engb.decode_latent(z.cuda(), xyz.cuda()).cpu().reshape(-1)
    ydb = engb.decode(x.cuda()).cpu().reshape(-1)
    assert rel_err(ylb, yob) <= 1e-4 and rel_err(ydb, yob) <= 1e-4 and rel_err(ylb, yo) >= 1e-5      # bf16 really is in the loop


def test_bf16_forward_is_bit_reproducible_and_has_no_outlier_rows():
    """The 8-wave bf16 forward runs two waves per SIMD; its first version let a load reuse the registers of the MFMA just before it
    and ~3 % of the rows differed from run to run (always rows 48-63 of a workgroup, errors up to 7e-2 of the output range).  Pin:
    identical bits across runs in both modes, and no row further from the oracle's bf16 emulation than rounding flips explain
    (measured max 9.5e-4 of the range on this net; the norm-wise bound of the other tests would not see a handful of bad rows)."""
    from deepsdf_amd.engine import Engine
    g = Golden("g8_eval_8x512")
    L = g.meta["L"]
    params = orc.init_params(orc.make_net(L, **g.meta["net_specs"]), g.meta["seed"])
    netb = orc.make_net(L, forward_bf16=True, **g.meta["net_specs"])
    engb = Engine(spec_from_meta(dict(L=L, net_specs=dict(g.meta["net_specs"], forward_bf16=True))))
    engb.load_params(params)
    gen = torch.Generator().manual_seed(11)
    z = torch.randn(L, generator=gen) / math.sqrt(L)
    n = 70001
    xyz = torch.rand(n, 3, generator=gen) * 2 - 1
    x = torch.cat([z.expand(n, -1), xyz], 1)
    yo = orc.decoder_forward(netb, params, x, training=False)[0].reshape(-1)
    zc, qc, xc = z.cuda(), xyz.cuda(), x.cuda()
    for name, fn in (("decode_latent", lambda: engb.decode_latent(zc, qc)), ("decode", lambda: engb.decode(xc))):
        runs = [fn().cpu().reshape(-1).clone() for _ in range(4)]
        for k in range(1, 4):
            assert torch.equal(runs[k], runs[0]), (name, k, int((runs[k] != runs[0]).sum()))
        worst = float((runs[0] - yo).abs().max() / yo.abs().max())
        print(f"{name}: worst row {worst:.2e} of the output range")
        assert worst <= 3e-3, (name, worst)


BF16X8_NETS = {
    # every wave of the 8-wave kernel holds ONE n-tile in every layer (8 tiles of 32 columns): a k-loop step is 2 MFMAs, the shortest
    # distance between an MFMA and a load into its source registers the kernel ever runs with
    "4x256_one_tile_per_wave": dict(L=29, net=dict(dims=[256] * 4, dropout=[0, 1, 2, 3], dropout_prob=0.2, norm_layers=[0, 1, 2, 3],
                                                   latent_in=[2], weight_norm=True, geom_dimension=3)),
    # ragged widths, one tile per wave: layers whose last k-unit / last n-tile are partial, waves without a tile in some layers
    "ragged_narrow": dict(L=11, net=dict(dims=[200, 72, 136, 252], dropout=[], dropout_prob=0.0, norm_layers=[0, 1, 2, 3], latent_in=[3],
                                         weight_norm=True, geom_dimension=3)),
    # ragged widths mixing waves with two tiles and waves with one
    "ragged_wide": dict(L=40, net=dict(dims=[500, 300, 420, 512, 268], dropout=[0, 2], dropout_prob=0.2, norm_layers=[0, 1, 2, 3, 4],
                                       latent_in=[2], weight_norm=True, geom_dimension=3)),
}


@pytest.mark.parametrize("name", sorted(BF16X8_NETS))
def test_bf16_8wave_forward_reproducible_on_short_steps_and_ragged_widths(name):
    """The determinism / outlier pin of the 8-wave bf16 forward on the shapes the g8 net does not have: nets whose waves hold ONE n-tile
    (a k-loop step of 2 MFMAs instead of 4 -- half the distance between an MFMA and the loads that reuse its source registers) and
    ragged widths (partial last k-units and n-tiles, guarded tail steps, waves with no tile).  4 runs x 2 entry points, bit-identical,
    and no row further from the oracle's bf16 emulation than rounding flips explain."""
    from deepsdf_amd.engine import Engine
    c = BF16X8_NETS[name]
    L = c["L"]
    netb = orc.make_net(L, forward_bf16=True, **c["net"])
    params = orc.init_params(orc.make_net(L, **c["net"]), 123)
    engb = Engine(spec_from_meta(dict(L=L, net_specs=dict(c["net"], forward_bf16=True))))
    engb.load_params(params)
    gen = torch.Generator().manual_seed(12)
    z = torch.randn(L, generator=gen) / math.sqrt(L)
    n = 40003
    xyz = torch.rand(n, 3, generator=gen) * 2 - 1
    x = torch.cat([z.expand(n, -1), xyz], 1)
    yo = orc.decoder_forward(netb, params, x, training=False)[0].reshape(-1)
    zc, qc, xc = z.cuda(), xyz.cuda(), x.cuda()
    for entry, fn in (("decode_latent", lambda: engb.decode_latent(zc, qc)), ("decode", lambda: engb.decode(xc))):
        runs = [fn().cpu().reshape(-1).clone() for _ in range(4)]
        for k in range(1, 4):
            assert torch.equal(runs[k], runs[0]), (name, entry, k, int((runs[k] != runs[0]).sum()))
        worst = float((runs[0] - yo).abs().max() / yo.abs().max())
        print(f"{name} {entry}: worst row {worst:.2e} of the output range, rel err {rel_err(runs[0], yo):.2e}")
        assert worst <= 3e-3 and rel_err(runs[0], yo) <= 2e-4, (name, entry, worst)


def test_real_weights_known_answer():
    from deepsdf_amd.engine import Engine
    g = Golden("g6_real_weights")
    eng = Engine(spec_from_meta(g.meta))
    eng.load_params(g.group("params"))
    y = eng.decode(torch.zeros(1, g.meta["L"] + 3, device="cuda"))
    assert abs(float(y) - g.meta["f0_survey"]) < 5e-5


BIG = dict(dims=[512] * 8, dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)), latent_in=[4],
           xyz_in_all=False, use_tanh=False, latent_dropout=False, weight_norm=True, geom_dimension=3)


# the batch builders live in tests/safe_batch.py (shared with tests/test_gpu_breakpoints.py); same names, same draws
_big_batch, _safe_batch = big_batch, safe_batch


class _Snapshot:
    """The oracle's optimiser state after a step (copies; attribute names of oracle.TrainState)."""

    def __init__(self, st):
        cp = lambda d: {k: v.clone() for k, v in d.items()}   # noqa: E731
        self.params, self.m, self.v = cp(st.params), cp(st.m), cp(st.v)
        self.latents, self.m_lat, self.v_lat, self.step = st.latents.clone(), st.m_lat.clone(), st.v_lat.clone(), st.step


_HEADLINE = dict(L=256, B=64, S=256, param_seed=5, lat_seed=6, batch_seed=100, drop_seed=4242, epoch=57, st64=None, steps=[])


def _headline_trajectory(n_steps):
    """ONE float64 oracle trajectory of BASELINE config 2 at full size (64 scenes x 256 points, L = 256, 8x512, dropout 0.2, one code
    above CodeBound, margin-safe batches), shared by every full-size test of the headline shape: the float64 steps are most of the
    GPU suite's wall time (a 16384-point step plus the margin search is ~15 s of CPU), so they are computed once per session and
    extended on demand.  Returns (net, params, lat0, steps); steps[i] = dict(idx, xyz, gt, r64 = the oracle's step result,
    after = the oracle's state after the step)."""
    H = _HEADLINE
    net = orc.make_net(H["L"], **BIG)
    params = orc.init_params(net, H["param_seed"])
    lat0 = torch.randn(H["B"], H["L"], generator=torch.Generator().manual_seed(H["lat_seed"])) / math.sqrt(H["L"])
    lat0[3] *= 2.5 / lat0[3].norm()
    if H["st64"] is None:
        H["st64"] = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    st64 = H["st64"]
    while len(H["steps"]) < n_steps:
        step = len(H["steps"])
        idx, xyz, gt = _safe_batch(net, st64, H["B"], H["S"], H["batch_seed"] + step, 0.1, 1.0, H["drop_seed"])
        r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=H["epoch"], seed=H["drop_seed"])
        H["steps"].append(dict(idx=idx, xyz=xyz, gt=gt, r64=r64, after=_Snapshot(st64)))
    return net, params, lat0, H["steps"][:n_steps]


def test_full_size_step_vs_oracle():
    """BASELINE config 2 at full size: 64 scenes x 256 pts = 16384 pts, L=256, 8x512, dropout 0.2: two optimiser
    steps of the HIP path against the oracle run in float64 (the truth) on identical seeded inputs; the fp32
    oracle's own distance from that truth is printed for scale."""
    L = 256
    net, params, lat0, traj = _headline_trajectory(2)
    spec = spec_from_meta(dict(L=L, net_specs=BIG))
    st32 = orc.TrainState.create({k: v.clone() for k, v in params.items()}, lat0.clone())
    tr = HipTrainer(spec, params, lat0)
    for step, t in enumerate(traj):
        idx, xyz, gt, r64, st64 = t["idx"], t["xyz"], t["gt"], t["r64"], t["after"]
        rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=57, lr=(5e-4, 1e-3), seed=4242,
                     want_y=True)
        assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"])
        worst_h = max(rel_err(rh["grads"][k], r64["grads"][k]) for k in r64["grads"])
        if step == 0:      # the fp32 CPU oracle's own distance from the float64 truth, for scale (one step: it is a print, not a check)
            r32 = orc.train_step(net, st32, idx, xyz, gt, delta=0.1, code_bound=1.0, epoch=57, seed=4242)
            worst_o = max(rel_err(r32["grads"][k], r64["grads"][k]) for k in r64["grads"])
            print(f"step {step}: max grad rel err vs fp64 truth: HIP {worst_h:.2e}, fp32 CPU oracle {worst_o:.2e}")
        else:
            print(f"step {step}: max grad rel err vs fp64 truth: HIP {worst_h:.2e}")
        for k in r64["grads"]:
            assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (step, k)
        assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL
        P = tr.params()
        for k in st64.params:
            assert rel_err(P[k], st64.params[k]) <= PARAM_TOL, (step, k)
        assert rel_err(tr.lat.cpu(), st64.latents) <= PARAM_TOL
        # element-wise: worst ROW of the forward, worst ENTRY of every gradient tensor, worst entry of the post-Adam state
        y_row = worst_elem(rh["y"], r64["y"])
        g_el = {k: worst_elem(rh["grads"][k], r64["grads"][k]) for k in r64["grads"]}
        g_el["latent"] = worst_elem(rh["dlat"], r64["dlat"])
        p_el = max(float((P[k].double() - st64.params[k]).abs().max()) for k in st64.params) / 5e-4
        print(f"step {step}: worst y row {y_row:.2e} of max|y|; worst gradient entry {max(g_el.values()):.2e} of its tensor's max "
              f"({max(g_el, key=g_el.get)}); worst post-Adam parameter entry {p_el:.2e} of one Adam step (lr)")
        assert y_row <= Y_ROW_TOL, step
        for k, e in g_el.items():
            assert e <= GRAD_ELEM_TOL, (step, k, e)
        assert p_el <= PARAM_STEP_FRAC, step


def test_gemm_split_full_size_step_and_decode_vs_oracle():
    """NetworkSpecs gemm_split (opt-in): the fused kernels' hidden GEMMs as 6 bf16 MFMAs on 3-way split fp32 operands.  Claimed to
    be fp32-accurate, so it gets the fp32 tests' tolerances against the float64 oracle: two optimiser steps of config 2 at full size
    (loss 1e-5, gradients 1e-4, post-Adam state), the forward on 70001 points (1e-5, and no ROW further than 1e-5 of the range), and
    bit-identical reruns."""
    from deepsdf_amd.engine import Engine
    L = 256
    net, params, lat0, traj = _headline_trajectory(2)        # the float64 steps test_full_size_step_vs_oracle compares with
    spec = spec_from_meta(dict(L=L, net_specs=dict(BIG, gemm_split=True)))
    assert spec.gemm_split and spec.c_struct().gemm_split == 1
    gen = torch.Generator().manual_seed(6)
    tr = HipTrainer(spec, params, lat0)
    for step, t in enumerate(traj):
        idx, xyz, gt, r64, st64 = t["idx"], t["xyz"], t["gt"], t["r64"], t["after"]
        rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=57, lr=(5e-4, 1e-3), seed=4242)
        assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"])
        worst = max(rel_err(rh["grads"][k], r64["grads"][k]) for k in r64["grads"])
        print(f"gemm_split step {step}: max grad rel err vs fp64 truth {worst:.2e}")
        for k in r64["grads"]:
            assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (step, k)
        assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL
        P = tr.params()
        for k in st64.params:
            assert rel_err(P[k], st64.params[k]) <= PARAM_TOL, (step, k)
        assert rel_err(tr.lat.cpu(), st64.latents) <= PARAM_TOL
    # forward alone, ragged size, both entry points; run-to-run bits
    eng = Engine(spec)
    eng.load_params(params)
    n = 70001
    z = torch.randn(L, generator=gen) / math.sqrt(L)
    xyz = torch.rand(n, 3, generator=gen) * 2 - 1
    x = torch.cat([z.expand(n, -1), xyz], 1)
    yo = orc.decoder_forward(net, {k: v.double() for k, v in params.items()}, x.double(), training=False)[0].reshape(-1)
    for name, fn in (("decode_latent", lambda: eng.decode_latent(z.cuda(), xyz.cuda())), ("decode", lambda: eng.decode(x.cuda()))):
        runs = [fn().cpu().reshape(-1).clone() for _ in range(3)]
        assert torch.equal(runs[1], runs[0]) and torch.equal(runs[2], runs[0]), name
        worst_row = float((runs[0].double() - yo).abs().max() / yo.abs().max())
        print(f"gemm_split {name}: rel err {rel_err(runs[0], yo):.2e}, worst row {worst_row:.2e} of the range")
        assert rel_err(runs[0], yo) <= FWD_TOL and worst_row <= 1e-5, name


@pytest.mark.parametrize("split", [True, False], ids=["split", "fp32mfma"])
@pytest.mark.parametrize("ragged", [False, True], ids=["segments", "ragged"])
def test_gemm_split_256_wide_net_vs_oracle(ragged, split):
    """gemm_split on a net whose weight-gradient tiles form exactly ONE 2 x 2 block per layer and split (4 x 256, skip at layer 2), in
    segment mode and through the general path (x0 gathered, its columns inside the dW GEMMs; the K-split chunks are not multiples of the
    dW kernel's 16-point step either way), beside the fp32-MFMA kernels on the same batch: the fp32 tolerances."""
    L, B, S = 61, 12, 192
    kw = dict(dims=[256] * 4, dropout=[0, 1, 2, 3], dropout_prob=0.2, norm_layers=[0, 1, 2, 3], latent_in=[2], weight_norm=True,
              geom_dimension=3)
    net = orc.make_net(L, **kw)
    spec = spec_from_meta(dict(L=L, net_specs=dict(kw, gemm_split=split)))
    params = orc.init_params(net, 17)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(18)) / math.sqrt(L)
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    tr = HipTrainer(spec, params, lat0)
    for step in range(2):
        idx, xyz, gt = _safe_batch(net, st64, B, S, 900 + step, 0.1, 1.0, 55)
        r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=130, seed=55)
        rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=130, lr=(5e-4, 1e-3), seed=55,
                     **(dict(force_ragged=True) if ragged else {}))
        assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), step
        print(f"step {step}: worst gradient rel err {max(rel_err(rh['grads'][k], r64['grads'][k]) for k in r64['grads']):.2e}")
        for k in r64["grads"]:
            assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (step, k)
        assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL, step
        P = tr.params()
        for k in st64.params:
            assert rel_err(P[k], st64.params[k]) <= 5e-5, (step, k)      # (small net: Adam's eps-sized entries, as in the odd-shapes test)


def test_full_size_properties():
    """Size-independent properties at 16384 pts: bit-exact determinism, and batch_split=4 == unsplit."""
    L, B, S = 256, 64, 256
    net = orc.make_net(L, **BIG)
    spec = spec_from_meta(dict(L=L, net_specs=BIG))
    params = orc.init_params(net, 9)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(1)) / math.sqrt(L)
    idx, xyz, gt = _big_batch(B, S, 77)
    outs = []
    for bs in (1, 1, 4):
        tr = HipTrainer(spec, params, lat0)
        outs.append(tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=200, lr=(5e-4, 1e-3),
                            batch_split=bs, seed=1, do_adam=False))
    for k in outs[0]["grads"]:
        assert torch.equal(outs[0]["grads"][k], outs[1]["grads"][k]), k          # deterministic reductions
        assert rel_err(outs[2]["grads"][k], outs[0]["grads"][k]) <= 1e-5, k        # accumulation == one pass
    assert torch.equal(outs[0]["dlat"], outs[1]["dlat"])
    assert abs(outs[2]["loss"] - outs[0]["loss"]) <= 1e-6 * abs(outs[0]["loss"])


def _packed_floats_without_split_planes(eng):
    import ctypes as C
    from deepsdf_amd import _lib
    net = eng.spec.c_struct()
    net.gemm_split = 0
    n = C.c_int64()
    _lib.check(_lib.lib().dsdf_packed_floats(C.byref(net), C.byref(n)))
    return int(n.value)


def test_train_step_fast_path_equals_two_call_path():
    """dsdf_train_step (finalize + Adam + weight-norm scales fused, gradient arena not written) == forward_backward +
    adam_step FROM THE SAME STATE: identical Adam arithmetic per element; only the row-norm summation order of the new
    scales differs.  (The state is re-synchronised before every step: left alone, the ~1e-7 scale rounding feeds Adam's
    early steps -- update ~ lr * g / (|g| + eps) -- and the two trajectories drift apart by ~1e-5 within three steps.)"""
    from deepsdf_amd.engine import make_segments
    L, B, S = 256, 8, 256
    net = orc.make_net(L, **BIG)
    spec = spec_from_meta(dict(L=L, net_specs=BIG))
    params = orc.init_params(net, 21)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(2)) / math.sqrt(L)
    a, b = HipTrainer(spec, params, lat0), HipTrainer(spec, params, lat0)
    for step in range(3):
        for name in ("params", "exp_avg", "exp_avg_sq", "packed"):
            getattr(b.eng, name).copy_(getattr(a.eng, name))
        for name in ("lat", "lat_m", "lat_v"):
            getattr(b, name).copy_(getattr(a, name))
        assert b.eng.step == a.eng.step
        idx, xyz, gt = _big_batch(B, S, 300 + step)
        a.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=150, lr=(5e-4, 1e-3), seed=5)
        sc, so = make_segments(idx.cuda())
        b.eng.train_step(b.lat, b.dlat, b.lat_m, b.lat_v, sc, so, xyz.cuda().contiguous(), gt.reshape(-1).cuda().contiguous(),
                         n_norm=B * S, clamp_dist=0.1, reg_coef=1e-4, code_bound=1.0, lr_decoder=5e-4, lr_latent=1e-3, seed=5,
                         seg_len=S)
        assert abs(float(a.eng.loss) - float(b.eng.loss)) <= 1e-6 * abs(float(a.eng.loss))
        pa, pb = a.params(), b.params()
        for k in pa:
            assert rel_err(pb[k], pa[k]) <= 1e-6, (step, k)
        assert rel_err(b.lat.cpu(), a.lat.cpu()) <= 1e-6
        assert rel_err(b.eng.exp_avg.cpu(), a.eng.exp_avg.cpu()) <= 1e-6
        assert rel_err(b.eng.exp_avg_sq.cpu(), a.eng.exp_avg_sq.cpu()) <= 1e-6
        npk = _packed_floats_without_split_planes(a.eng)   # (gemm_split: the bf16 planes behind it are not floats; the kernels check them)
        assert rel_err(b.eng.packed.cpu()[:npk], a.eng.packed.cpu()[:npk]) <= 2e-6       # W, W^T, fragment copies and scales


SEG_SHAPES = {
    # segment mode (deepsdf_amd/csrc/fused.hpp FusedSeg) on shapes that are NOT the headline: widths off the 32/64 grid,
    # latent sizes off the float4 grid, no skip layer / skip right after layer 0, 2-D geometry, chunked batches
    # BASELINE configs[0] / SURVEY config 1: one shape, latent 4, 4 x 128 decoder with latent_in=[2], 4096 points per step
    "config1_4x128": dict(L=4, B=1, S=4096, split=1, net=dict(dims=[128] * 4, dropout=[0, 1, 2, 3], dropout_prob=0.2,
                                                             norm_layers=[0, 1, 2, 3], latent_in=[2], weight_norm=True,
                                                             geom_dimension=3)),
    "skip2_w64": dict(L=8, B=3, S=64, split=1, net=dict(dims=[64] * 4, dropout=[], dropout_prob=0.0, norm_layers=[0, 1, 2, 3],
                                                      latent_in=[2], weight_norm=True, geom_dimension=3)),
    "noskip_w40_L6_drop": dict(L=6, B=2, S=128, split=1, net=dict(dims=[40, 40, 40], dropout=[0, 1], dropout_prob=0.2,
                                                                  norm_layers=[0, 1, 2], latent_in=[], weight_norm=True,
                                                                  geom_dimension=3)),
    "skip1_w96_split2": dict(L=20, B=4, S=64, split=2, net=dict(dims=[96] * 3, dropout=[0, 1, 2], dropout_prob=0.2,
                                                                norm_layers=[0, 2], latent_in=[1], weight_norm=True,
                                                                geom_dimension=3)),
    # more segments than one pass of the segment-chunked kernels handles (seg_dw: 64 per pass, seg_hoist: 16 per wave)
    "many_segments": dict(L=12, B=150, S=64, split=1, net=dict(dims=[48, 48, 48], dropout=[1], dropout_prob=0.2,
                                                              norm_layers=[0, 1, 2], latent_in=[1], weight_norm=True,
                                                              geom_dimension=3)),
    # long segments: 64 workgroups per scene (the shipped specs go up to SamplesPerScene 16384)
    "long_segments": dict(L=8, B=2, S=4096, split=1, net=dict(dims=[64, 64, 64], dropout=[0, 2], dropout_prob=0.2,
                                                               norm_layers=[0, 1, 2], latent_in=[1], weight_norm=True,
                                                               geom_dimension=3)),
    # one scene of 8192 points: 128 workgroups per segment (the per-segment sums take their parallel form)
    # (ONE scene: many weight-gradient entries are ~1e-8 = Adam's eps, where the first step's update lr*g/(|g|+eps) turns a
    # 1e-5 relative gradient difference into a few 1e-5 of the parameter scale -> its own post-Adam tolerance)
    "one_long_scene": dict(L=8, B=1, S=8192, split=1, param_tol=5e-5, net=dict(dims=[64, 64, 64], dropout=[1], dropout_prob=0.2,
                                                              norm_layers=[0, 1, 2], latent_in=[1], weight_norm=True,
                                                              geom_dimension=3)),
    # 96 = 3 x 32 points per scene: segment mode exists for this batch on 32-point workgroups only (64-point ones take the ragged path)
    "s96_three_h32_workgroups": dict(L=6, B=3, S=96, split=1, net=dict(dims=[96, 96, 96], dropout=[0, 1], dropout_prob=0.2,
                                                                         norm_layers=[0, 1, 2], latent_in=[2], weight_norm=True,
                                                                         geom_dimension=3)),
    # latent_in names the OUTPUT layer (deep_sdf_decoder.py:88-89 runs for the last Linear too): sdf = tanh(<[a | x0], w> + b).  No
    # segment mode for such a net; the backward heads hand the x0 columns' gradient to d/dx0 unmasked (found by the random specs below)
    "skip_into_the_output_layer": dict(L=5, B=3, S=64, split=1, net=dict(dims=[64, 72, 72], dropout=[0, 1, 2], dropout_prob=0.2,
                                                                          norm_layers=[0, 1, 2, 3], latent_in=[3], weight_norm=True,
                                                                          geom_dimension=3)),
    "geom2_plain": dict(L=16, B=2, S=192, split=1, net=dict(dims=[72, 72, 72, 72], dropout=[], dropout_prob=0.0, norm_layers=[],
                                                            latent_in=[2], weight_norm=False, geom_dimension=2)),
}


@pytest.mark.parametrize("name", sorted(SEG_SHAPES))
def test_segment_mode_odd_shapes_vs_oracle(name, monkeypatch):
    """Two optimiser steps in segment mode (every scene a whole number of workgroups) against the float64 oracle, and the SAME
    batch through the general (ragged) path: both must meet the gradient tolerance.  Batches this small run on 32-point workgroups
    (fused_fwd_bwd_h32_kernel: at most 32 x #CUs points); DSDF_FROWS=64 sends the same batches through 64-point workgroups -- the
    narrow-net kernels for nets of at most 128 columns, and with DSDF_NO_NARROW=1 the full-size kernels -- so every shape is
    checked on all three kernel families."""
    c = SEG_SHAPES[name]
    L, B, S, G = c["L"], c["B"], c["S"], c["net"]["geom_dimension"]
    net = orc.make_net(L, **c["net"])
    spec = spec_from_meta(dict(L=L, net_specs=c["net"]))
    params = orc.init_params(net, 31)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(32)) / math.sqrt(L)
    lat0[-1] *= 1.7 / lat0[-1].norm()                    # one row above the max-norm bound
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    seg, rag, seg64, rag64, segfull, ragfull = (HipTrainer(spec, params, lat0) for _ in range(6))
    for step in range(2):
        idx, xyz, gt = _safe_batch(net, st64, B, S, 500 + step, 0.1, 1.0, 77, G=G)
        r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=130, seed=77,
                             batch_split=c["split"])
        # rows None: 32-point workgroups (these batches are small); "64": 64-point workgroups -- for nets of at most 128 columns the
        # narrow-net kernels (fused_fwd_bwd_n128_kernel, two workgroups per CU); "64 full": ... and those switched off, i.e. the
        # full-size kernel the headline runs on
        for tr, kw, rows in ((seg, {}, None), (rag, dict(force_ragged=True), None), (seg64, {}, "64"), (rag64, dict(force_ragged=True), "64"),
                             (segfull, {}, "64 full"), (ragfull, dict(force_ragged=True), "64 full")):
            monkeypatch.delenv("DSDF_FROWS", raising=False)
            monkeypatch.delenv("DSDF_NO_NARROW", raising=False)
            if rows is not None:
                monkeypatch.setenv("DSDF_FROWS", "64")
                if rows.endswith("full"):
                    monkeypatch.setenv("DSDF_NO_NARROW", "1")
            rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=130, lr=(5e-4, 1e-3), seed=77,
                         batch_split=c["split"], **kw)
            assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), (step, kw, rows)
            for k in r64["grads"]:
                assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (step, k, kw, rows)
            assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL, (step, kw, rows)
            P = tr.params()
            ptol = c.get("param_tol", PARAM_TOL)
            for k in st64.params:
                assert rel_err(P[k], st64.params[k]) <= ptol, (step, k, kw, rows)
            assert rel_err(tr.lat.cpu(), st64.latents) <= ptol, (step, kw, rows)
    monkeypatch.delenv("DSDF_FROWS", raising=False)
    monkeypatch.delenv("DSDF_NO_NARROW", raising=False)


def _random_case(seed):
    """A seeded random NetworkSpecs + batch shape inside what the reference's Decoder constructor accepts and the fused kernels take:
    2-6 hidden layers of widths 32 ... 264 (not all on the 32-column tile grid), any / no skip layer (also in front of the output
    layer), weight norm on a random subset (or none), dropout on a random subset with p in {0, 0.2, 0.5}, use_tanh, 2-D / 3-D
    geometry, latent sizes 1 ... 64, 1-5 scenes of 32 ... 264 samples (multiples of 32 and not), --batch_split 1 or 2."""
    import random
    rng = random.Random(1000 + seed)
    nh = rng.randint(2, 6)
    G = rng.choice([2, 3, 3, 3])
    L = rng.choice([1, 2, 3, 5, 8, 16, 29, 64])
    W0 = L + G
    widths = [w for w in (32, 40, 64, 72, 96, 128, 136, 160, 200, 264) if w - W0 >= 8]
    dims = [rng.choice(widths) for _ in range(nh)]
    latent_in = [] if rng.random() < 0.3 else [rng.randint(1, nh)]
    wn = rng.random() < 0.8
    norm_layers = sorted(rng.sample(range(nh + 1), rng.randint(1, nh + 1))) if wn else []
    dropout = sorted(rng.sample(range(nh), rng.randint(0, nh)))
    p = rng.choice([0.0, 0.2, 0.5]) if dropout else 0.0
    B = rng.randint(1, 5)
    S = rng.choice([32, 64, 96, 128, 160, 256, 40, 100, 264])
    split = 2 if (B * S) % 2 == 0 and rng.random() < 0.3 else 1
    net = dict(dims=dims, dropout=dropout, dropout_prob=p, norm_layers=norm_layers, latent_in=latent_in, weight_norm=wn,
               use_tanh=rng.random() < 0.3, geom_dimension=G)
    return dict(L=L, B=B, S=S, split=split, net=net)


@pytest.mark.parametrize("seed", range(36))
def test_random_specs_and_shapes_vs_oracle(seed, monkeypatch):
    """Seeded random decoders and batch shapes (see _random_case), one optimiser step each against the float64 oracle, segment and
    ragged, rotated over the three kernel families (32-point workgroups / narrow-net or full 64-point kernels / full-size kernels
    only).  The hand-picked shapes above cover the cases somebody thought of; the 65536-point overrun of rounds 1-3 was one nobody
    had."""
    c = _random_case(seed)
    L, B, S, G = c["L"], c["B"], c["S"], c["net"]["geom_dimension"]
    family = seed % 3
    monkeypatch.delenv("DSDF_FROWS", raising=False)
    monkeypatch.delenv("DSDF_NO_NARROW", raising=False)
    if family >= 1:
        monkeypatch.setenv("DSDF_FROWS", "64")
    if family == 2:
        monkeypatch.setenv("DSDF_NO_NARROW", "1")
    net = orc.make_net(L, **c["net"])
    spec = spec_from_meta(dict(L=L, net_specs=c["net"]))
    params = orc.init_params(net, 200 + seed)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(300 + seed)) / math.sqrt(L)
    lat0[-1] *= 1.7 / lat0[-1].norm()                    # one row above the max-norm bound
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    idx, xyz, gt = _safe_batch(net, st64, B, S, 400 + seed, 0.1, 1.0, 77, G=G)
    r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=130, seed=77, batch_split=c["split"])
    for kw in ({}, dict(force_ragged=True)):
        tr = HipTrainer(spec, params, lat0)
        rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=130, lr=(5e-4, 1e-3), seed=77,
                     batch_split=c["split"], **kw)
        what = (seed, c, kw, family)
        assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), what
        for k in r64["grads"]:
            assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (k, what)
            assert worst_elem(rh["grads"][k], r64["grads"][k]) <= GRAD_ELEM_TOL, (k, what)
        assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL, what
        P = tr.params()
        for k in st64.params:
            assert rel_err(P[k], st64.params[k]) <= 5e-5, (k, what)      # (tiny batches: gradient entries near Adam's eps, see one_long_scene)
        assert rel_err(tr.lat.cpu(), st64.latents) <= 5e-5, what


def _random_w32_case(seed):
    """A seeded random decoder whose every layer is at most 32 wide (the reference's double_lattice_3D_small_network family): what the
    wave-private merged kernel (fused_fwd_bwd_w32_kernel: a workgroup = ONE wave with 32 points) takes.  2-5 hidden layers of 16 ... 32
    columns, any / no skip layer (also in front of the output layer), dropout, weight norm, use_tanh, 2-D / 3-D, scenes of 32 ... 1000
    samples (multiples of 32 and not, so both segment mode and the ragged path)."""
    import random
    rng = random.Random(7000 + seed)
    nh = rng.randint(2, 5)
    G = rng.choice([2, 3, 3])
    L = rng.choice([1, 2, 3, 5, 8])
    W0 = L + G
    # seeds >= 16: layers of up to 64 columns (the corner_spheres_only_small_network family): the two-n-tile form, fused_fwd_bwd_w32x2_kernel
    widths = [w for w in ((16, 20, 24, 28, 32) if seed < 16 else (24, 32, 40, 48, 56, 64, 64)) if w - W0 >= 8]
    dims = [rng.choice(widths) for _ in range(nh)]
    latent_in = [] if rng.random() < 0.3 else [rng.randint(1, nh)]
    wn = rng.random() < 0.8
    norm_layers = sorted(rng.sample(range(nh + 1), rng.randint(1, nh + 1))) if wn else []
    dropout = sorted(rng.sample(range(nh), rng.randint(0, nh)))
    p = rng.choice([0.0, 0.2, 0.5]) if dropout else 0.0
    B = rng.randint(1, 6)
    S = rng.choice([32, 64, 96, 320, 992, 40, 100, 1000])
    split = 2 if (B * S) % 2 == 0 and rng.random() < 0.3 else 1
    net = dict(dims=dims, dropout=dropout, dropout_prob=p, norm_layers=norm_layers, latent_in=latent_in, weight_norm=wn,
               use_tanh=rng.random() < 0.3, geom_dimension=G)
    return dict(L=L, B=B, S=S, split=split, net=net)


@pytest.mark.parametrize("seed", range(28))
def test_wave_private_kernel_vs_oracle_and_the_four_wave_kernels(seed, monkeypatch):
    """Nets of at most 32-wide (seeds 16 ...: 64-wide) layers train on the wave-private merged kernels at every batch size.  One optimiser step of seeded random
    such nets against the float64 oracle, segment and ragged -- and the same step with DSDF_NO_W32=1 (the 64-row narrow kernels /
    32-row four-wave workgroups) must agree with it to fp32 summation order: same loss, gradients, parameters."""
    c = _random_w32_case(seed)
    L, B, S, G = c["L"], c["B"], c["S"], c["net"]["geom_dimension"]
    monkeypatch.delenv("DSDF_FROWS", raising=False)
    monkeypatch.delenv("DSDF_NO_NARROW", raising=False)
    net = orc.make_net(L, **c["net"])
    spec = spec_from_meta(dict(L=L, net_specs=c["net"]))
    params = orc.init_params(net, 7200 + seed)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(7300 + seed)) / math.sqrt(L)
    lat0[-1] *= 1.7 / lat0[-1].norm()                    # one row above the max-norm bound
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    idx, xyz, gt = _safe_batch(net, st64, B, S, 7400 + seed, 0.1, 1.0, 79, G=G)
    r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=130, seed=79, batch_split=c["split"])
    for kw in ({}, dict(force_ragged=True)):
        res = {}
        for no_w32 in (False, True):
            monkeypatch.delenv("DSDF_NO_W32", raising=False)
            if no_w32:
                monkeypatch.setenv("DSDF_NO_W32", "1")
            tr = HipTrainer(spec, params, lat0)
            rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=130, lr=(5e-4, 1e-3), seed=79,
                         batch_split=c["split"], **kw)
            what = (seed, c, kw, no_w32)
            assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), what
            for k in r64["grads"]:
                assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (k, what)
                assert worst_elem(rh["grads"][k], r64["grads"][k]) <= GRAD_ELEM_TOL, (k, what)
            assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL, what
            P = tr.params()
            for k in st64.params:
                assert rel_err(P[k], st64.params[k]) <= 5e-5, (k, what)
            assert rel_err(tr.lat.cpu(), st64.latents) <= 5e-5, what
            res[no_w32] = rh
        for k in res[False]["grads"]:
            assert rel_err(res[False]["grads"][k], res[True]["grads"][k]) <= 1e-5, (k, seed, kw)
        assert abs(res[False]["loss"] - res[True]["loss"]) <= 2e-6 * abs(res[True]["loss"]), (seed, kw)
    monkeypatch.delenv("DSDF_NO_W32", raising=False)


@pytest.mark.parametrize("seed", range(12))
def test_random_specs_gemm_split_vs_oracle(seed):
    """The same random decoders with NetworkSpecs gemm_split (the fused kernels' hidden GEMMs as 6 bf16 MFMAs on 3-way cut fp32
    operands): its k-loops are kernels of their own (woven asm for four n-tiles per wave, compiler-scheduled for fewer), so they
    get their own walk over widths, skips and batch shapes -- with the fp32 tolerances, as everywhere for this mode."""
    c = _random_case(200 + seed)
    L, B, S, G = c["L"], c["B"], c["S"], c["net"]["geom_dimension"]
    net = orc.make_net(L, **c["net"])
    spec = spec_from_meta(dict(L=L, net_specs=dict(c["net"], gemm_split=True)))
    assert spec.gemm_split
    params = orc.init_params(net, 210 + seed)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(310 + seed)) / math.sqrt(L)
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    idx, xyz, gt = _safe_batch(net, st64, B, S, 410 + seed, 0.1, 1.0, 78, G=G)
    r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=130, seed=78, batch_split=c["split"])
    for kw in ({}, dict(force_ragged=True)):
        tr = HipTrainer(spec, params, lat0)
        rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=130, lr=(5e-4, 1e-3), seed=78,
                     batch_split=c["split"], **kw)
        what = (seed, c, kw)
        assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), what
        for k in r64["grads"]:
            assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (k, what)
        assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL, what


def _random_variant_case(seed):
    """_random_case plus what only the layer-by-layer kernels run: xyz_in_all, latent_dropout, LayerNorm (norm_layers WITHOUT
    weight_norm) and hidden widths beyond the fused kernels' 512."""
    import random
    rng = random.Random(5000 + seed)
    nh = rng.randint(2, 5)
    G, L = 3, rng.choice([2, 5, 8, 16, 29])
    W0 = L + G
    wide = rng.random() < 0.35
    widths = [w for w in ((40, 72, 136, 264, 520, 640) if wide else (40, 64, 72, 136, 200)) if w - W0 - G >= 8]
    dims = [rng.choice(widths) for _ in range(nh)]
    latent_in = [] if rng.random() < 0.3 else [rng.randint(1, nh)]
    kind = rng.choice(["xyz", "latdrop", "ln", "all", "wide_only"]) if wide else rng.choice(["xyz", "latdrop", "ln", "all"])
    ln = kind in ("ln", "all")
    wn = (not ln) and rng.random() < 0.7
    norm_layers = sorted(rng.sample(range(nh + 1), rng.randint(1, nh + 1))) if (wn or ln) else []
    dropout = sorted(rng.sample(range(nh), rng.randint(0, nh)))
    p = rng.choice([0.2, 0.5]) if dropout else 0.0
    if kind == "wide_only" and not any(d > 512 for d in dims):
        dims[rng.randrange(nh)] = 640
    B, S = rng.randint(1, 4), rng.choice([32, 64, 96, 40, 100])
    net = dict(dims=dims, dropout=dropout, dropout_prob=p, norm_layers=norm_layers, latent_in=latent_in, weight_norm=wn,
               xyz_in_all=kind in ("xyz", "all"), latent_dropout=kind in ("latdrop", "all"), use_tanh=rng.random() < 0.3, geom_dimension=G)
    return dict(L=L, B=B, S=S, split=1, net=net)


@pytest.mark.parametrize("seed", range(16))
def test_random_variant_specs_vs_oracle(seed):
    """Seeded random decoders of the kinds only the layer-by-layer MFMA GEMM path runs (xyz_in_all, latent_dropout, LayerNorm, widths
    above 512 -- none in any shipped spec), one optimiser step against the float64 oracle."""
    c = _random_variant_case(seed)
    L, B, S = c["L"], c["B"], c["S"]
    net = orc.make_net(L, **c["net"])
    spec = spec_from_meta(dict(L=L, net_specs=c["net"]))
    params = orc.init_params(net, 220 + seed)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(320 + seed)) / math.sqrt(L)
    lat0[0] *= 1.5 / lat0[0].norm()
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    idx, xyz, gt = _safe_batch(net, st64, B, S, 420 + seed, 0.1, 1.0, 79)
    r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=130, seed=79)
    tr = HipTrainer(spec, params, lat0)
    rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=130, lr=(5e-4, 1e-3), seed=79)
    what = (seed, c)
    assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), what
    for k in r64["grads"]:
        if float(r64["grads"][k].abs().max()) == 0.0:       # the unused bn module of the last Linear
            assert float(rh["grads"][k].abs().max()) == 0.0, (k, what)
        else:
            assert rel_err(rh["grads"][k], r64["grads"][k]) <= GRAD_TOL, (k, what)
    assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL, what
    P = tr.params()
    for k in st64.params:
        assert rel_err(P[k], st64.params[k]) <= 5e-5, (k, what)


@pytest.mark.parametrize("seed", range(10))
def test_random_specs_bf16_forward_vs_oracle(seed):
    """BASELINE config 5's kernels (bf16 forward GEMMs, fp32 accumulate; training form merged with the fp32 backward, and the 8-wave
    inference form) on the random decoders: the training step against the oracle's bf16-forward step (fp32; the config's own
    tolerances: loss 1e-4, gradients 1e-2 -- ReLU-flip noise between two bf16 forwards), the eval forward against the oracle's
    bf16 emulation (1e-4) through decode and decode_latent."""
    from deepsdf_amd.engine import Engine
    c = _random_case(300 + seed)
    L, B, S, G = c["L"], c["B"], c["S"], c["net"]["geom_dimension"]
    if len(c["net"]["dims"]) in c["net"]["latent_in"]:
        with pytest.raises(NotImplementedError, match="output layer"):      # refused, not computed wrongly (this test's first run:
            spec_from_meta(dict(L=L, net_specs=dict(c["net"], forward_bf16=True)))   # the 8-wave kernel ignored the x0 columns)
        return
    net = orc.make_net(L, forward_bf16=True, **c["net"])
    spec = spec_from_meta(dict(L=L, net_specs=dict(c["net"], forward_bf16=True)))
    params = orc.init_params(net, 230 + seed)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(330 + seed)) / math.sqrt(L)
    st = orc.TrainState.create({k: v.clone() for k, v in params.items()}, lat0.clone())
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    idx, xyz, gt = _safe_batch(net, st64, B, S, 430 + seed, 0.1, 1.0, 80, G=G)
    # inference first (the step below changes nothing it uses, but keeps the order of the config-5 test)
    eng = Engine(spec)
    eng.load_params(params)
    x = torch.cat([lat0[idx], xyz], 1)
    yo = orc.decoder_forward(net, params, x, training=False)[0].reshape(-1)
    assert rel_err(eng.decode(x.cuda()).cpu().reshape(-1), yo) <= 1e-4, (seed, c)
    if eng.decode_latent_supported():
        x1 = torch.cat([lat0[:1].expand(xyz.shape[0], -1), xyz], 1)
        y1 = orc.decoder_forward(net, params, x1, training=False)[0].reshape(-1)
        assert rel_err(eng.decode_latent(lat0[0].cuda(), xyz.cuda()).cpu().reshape(-1), y1) <= 1e-4, (seed, c)
    ro = orc.train_step(net, st, idx, xyz, gt, delta=0.1, code_bound=1.0, epoch=130, seed=80, batch_split=c["split"])
    for kw in ({}, dict(force_ragged=True)):
        tr = HipTrainer(spec, params, lat0)
        rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=130, lr=(5e-4, 1e-3), seed=80,
                     batch_split=c["split"], **kw)
        what = (seed, c, kw)
        assert abs(rh["loss"] - ro["loss"]) <= 1e-4 * abs(ro["loss"]), what
        for k in ro["grads"]:
            assert rel_err(rh["grads"][k], ro["grads"][k]) <= 1e-2, (k, what)
        assert rel_err(rh["dlat"], ro["dlat"]) <= 1e-2, what


@pytest.mark.parametrize("seed", range(8))
def test_random_specs_phased_backward_equals_the_single_call(seed):
    """The K-bucket phased backward (K drawn from 2 ... 8) on the random decoders: loss / forward bit-identical to the single call, weight
    gradients to summation order, and after the last phase nothing is left unwritten."""
    import random
    from deepsdf_amd.engine import make_segments
    c = _random_case(400 + seed)
    K = random.Random(seed).randint(2, 8)
    L, B, S, G = c["L"], c["B"], c["S"], c["net"]["geom_dimension"]
    spec = spec_from_meta(dict(L=L, net_specs=c["net"]))
    params = orc.init_params(orc.make_net(L, **c["net"]), 240 + seed)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(340 + seed)) / math.sqrt(L)
    idx, xyz, gt = _big_batch(B, S, 440 + seed, G=G)
    one, ph = HipTrainer(spec, params, lat0), HipTrainer(spec, params, lat0)
    if not one.eng.dw_phase_supported():
        pytest.skip("not a fused-path net")
    sc, so = make_segments(idx.cuda())
    xc, gc = xyz.cuda().contiguous(), gt.reshape(-1).cuda().contiguous()
    kw = dict(n_norm=B * S, clamp_dist=0.1, reg_coef=1e-4, code_bound=1.0, training=True, seed=6, seg_len=S)
    one.eng.train_forward_backward(one.lat, one.dlat, sc, so, xc, gc, **kw)
    ph.eng.grads.fill_(float("nan"))
    for p in range(1, K + 1):
        ph.eng.train_forward_backward(ph.lat, ph.dlat, sc, so, xc, gc, dw_phase=p, dw_buckets=K, **kw)
    assert not bool(torch.isnan(ph.eng.grads).any()) and torch.equal(one.eng.loss, ph.eng.loss), (seed, K, c)
    g1, g2 = one.eng.named_views(one.eng.grads), ph.eng.named_views(ph.eng.grads)
    for n in g1:
        assert rel_err(g2[n].cpu(), g1[n].cpu()) <= 2e-6 and worst_elem(g2[n].cpu(), g1[n].cpu()) <= 1e-5, (n, seed, K, c)
    assert rel_err(ph.dlat.cpu(), one.dlat.cpu()) <= 1e-6, (seed, K, c)


@pytest.mark.parametrize("seed", list(range(8)) + ["w32_3", "w32_6", "w32_9", "w32_17", "w32_21", "w32_26"])
def test_random_specs_reconstruction_vs_oracle(seed):
    """Latent-only reconstruction (frozen decoder, eval mode, Adam on the codes: BASELINE config 4's path) on the random decoders and
    shape counts: three iterations of reconstruct() against oracle.latent_step in float64, every shape following its own single-code
    trajectory -- sample counts on and off the 32-point grid (segment mode / the ragged frozen path).  The w32_* cases are nets of at
    most 32- / 64-wide layers (_random_w32_case): the frozen-decoder form of the wave-private kernels."""
    from deepsdf_amd.engine import Engine
    from deepsdf_amd.reconstruct import reconstruct
    if isinstance(seed, str):
        c = _random_w32_case(int(seed.split("_")[1]))
        seed = 40 + int(seed.split("_")[1])
    else:
        c = _random_case(500 + seed)
    L, B, S, G = c["L"], c["B"], c["S"], c["net"]["geom_dimension"]
    net = orc.make_net(L, **c["net"])
    params = orc.init_params(net, 250 + seed)
    p64 = {k: v.double() for k, v in params.items()}
    eng = Engine(spec_from_meta(dict(L=L, net_specs=c["net"])))
    eng.load_params(params)
    gen = torch.Generator().manual_seed(350 + seed)
    z0 = torch.randn(B, L, generator=gen) * 0.05
    xyz = torch.rand(B, S, G, generator=gen) * 2 - 1
    sdf = xyz.norm(dim=2) - 0.3 - 0.3 * torch.rand(B, 1, generator=gen)
    zo = z0.double().clone()
    mo, vo = torch.zeros_like(zo), torch.zeros_like(zo)
    iters = 3
    for it in range(iters):
        for b in range(B):
            zb, mb, vb = zo[b:b + 1], mo[b:b + 1], vo[b:b + 1]           # views: latent_step mutates them in place
            orc.latent_step(net, p64, zb, mb, vb, it + 1, xyz[b].double(), sdf[b].double(), delta=0.1, lr=5e-3, l2reg=1e-4)
    zh, _ = reconstruct(eng, xyz.cuda(), sdf.cuda(), num_iterations=iters, clamp_dist=0.1, lr=5e-3, l2reg=1e-4, z0=z0, lr_drop_every=0)
    # (no margin screening here: a clamp / sign flip of one point moves 1/S of a code's gradient and Adam's first steps pass the
    # sign on -- the bound is the step size, 3 iterations x lr, not the 1e-5 of the margin-safe full-size test)
    err = float((zh.cpu().double() - zo).abs().max())
    assert err <= 0.05 * iters * 5e-3, (seed, err, c)


_CONFIG5 = {}


def _config5_oracle(net, params, lat0, B, S):
    """The oracle's bf16-forward step of config 5 (fp32, the rounding points of Net.forward_bf16) on one margin-safe batch: computed
    once, shared by the two parametrisations below."""
    if not _CONFIG5:
        st = orc.TrainState.create({k: v.clone() for k, v in params.items()}, lat0.clone())
        st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
        idx, xyz, gt = _safe_batch(net, st64, B, S, 100, 0.1, 1.0, 4242)   # clamp/sign margins; ReLU flips cannot be excluded here:
        _CONFIG5.update(idx=idx, xyz=xyz, gt=gt, ro=orc.train_step(net, st, idx, xyz, gt, delta=0.1, code_bound=1.0, epoch=57, seed=4242))
    return _CONFIG5["idx"], _CONFIG5["xyz"], _CONFIG5["gt"], _CONFIG5["ro"]


@pytest.mark.parametrize("split", [False, True], ids=["fp32_backward", "split_backward"])
def test_config5_bf16_forward_vs_oracle_and_fp32(split):
    """BASELINE config 5: hidden-layer forward GEMMs with bf16 inputs / fp32 accumulate (v_mfma_f32_32x32x16_bf16), backward and
    Adam in fp32, on the 8x512 decoder at 16384 points.  Compared with (a) the oracle's bf16 emulation (same rounding
    points; what differs is the accumulation order and the ~1e-7 differences that decide a few bf16 roundings) and (b) the
    fp32 forward -- the tolerance the config asks to be RE-STATED: measured 2-3e-3 of the output range, asserted <= 1e-2."""
    from deepsdf_amd.engine import Engine
    L, B, S = 256, 64, 256
    kw = dict(BIG)
    net = orc.make_net(L, forward_bf16=True, **kw)
    spec = spec_from_meta(dict(L=L, net_specs=dict(kw, forward_bf16=True, gemm_split=split)))   # split: the backward dX chain in split mode
    spec32 = spec_from_meta(dict(L=L, net_specs=kw))
    params = orc.init_params(net, 5)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(6)) / math.sqrt(L)
    # (1) inference: decode
    x = torch.cat([lat0[torch.arange(B).repeat_interleave(S)], torch.rand(B * S, 3, generator=torch.Generator().manual_seed(7)) * 2 - 1], 1)
    eb, e32 = Engine(spec), Engine(spec32)
    eb.load_params(params); e32.load_params(params)
    yb, y32 = eb.decode(x.cuda()).cpu().reshape(-1), e32.decode(x.cuda()).cpu().reshape(-1)
    yo = orc.decoder_forward(net, params, x, training=False)[0].reshape(-1)
    e_or, e_32 = rel_err(yb, yo), rel_err(yb, y32)
    print(f"bf16 forward: vs oracle bf16 emulation {e_or:.2e}; vs the fp32 forward {e_32:.2e}")
    assert e_or <= 1e-4
    assert 1e-4 <= e_32 <= 1e-2                      # bf16 really is in the loop, and inside the re-stated tolerance
    # (2) one optimiser step: gradients and post-Adam state against the oracle's bf16-forward step
    idx, xyz, gt, ro = _config5_oracle(net, params, lat0, B, S)
    tr = HipTrainer(spec, params, lat0)
    rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=57, lr=(5e-4, 1e-3), seed=4242)
    assert abs(rh["loss"] - ro["loss"]) <= 1e-4 * abs(ro["loss"])
    worst = max(rel_err(rh["grads"][k], ro["grads"][k]) for k in ro["grads"])
    print(f"bf16 forward: max gradient rel err vs the oracle's bf16-forward step {worst:.2e}")
    # the two bf16 forwards differ by ~1e-5 in the pre-activations (which roundings tip), so a few thousand of the 67 M ReLUs
    # flip (fp32 mode: ~10) and each moves a gradient entry by O(1/N): discontinuity noise, measured 1-3e-3
    assert worst <= 1e-2
    assert rel_err(rh["dlat"], ro["dlat"]) <= 1e-2


def test_fused_and_layered_paths_agree_on_ragged_batches(monkeypatch):
    """The two product paths (fused persistent kernels vs layer-by-layer GEMM launches, DSDF_NO_FUSED=1) on a batch the
    fast paths do not special-case: N not a multiple of 64, ragged segments, a repeated scene, odd dropout row offset
    through --batch_split 3."""
    L = 256
    net = orc.make_net(L, **BIG)
    spec = spec_from_meta(dict(L=L, net_specs=BIG))
    params = orc.init_params(net, 33)
    lat0 = torch.randn(6, L, generator=torch.Generator().manual_seed(8)) / math.sqrt(L)
    gen = torch.Generator().manual_seed(9)
    lens = [700, 129, 1, 333, 64, 2100]
    scenes = [3, 0, 5, 3, 1, 4]                       # scene 3 appears in two segments
    idx = torch.cat([torch.full((n,), s, dtype=torch.int64) for n, s in zip(lens, scenes)])
    N = idx.numel()
    xyz = torch.rand(N, 3, generator=gen) * 2 - 1
    gt = xyz.norm(dim=1, keepdim=True) - 0.5
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DSDF_NO_FUSED", mode)
        spec = spec_from_meta(dict(L=L, net_specs=BIG))   # (after the switch: the DSDF_GEMM_SPLIT default of a lab run does not apply to the layered path)
        tr = HipTrainer(spec, params, lat0)
        outs[mode] = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=300, lr=(5e-4, 1e-3),
                             batch_split=3, seed=77, want_y=True)
        outs[mode]["params"] = tr.params()
        outs[mode]["lat"] = tr.lat.cpu()
    a, b = outs["0"], outs["1"]
    assert rel_err(a["y"], b["y"]) <= 1e-6
    assert abs(a["loss"] - b["loss"]) <= 1e-6 * abs(b["loss"])
    # the two paths sum in different orders, so a few of the 13.6 M pre-activations flip their ReLU (not margin-safe)
    for k in a["grads"]:
        assert rel_err(a["grads"][k], b["grads"][k]) <= 3e-4, k
    assert rel_err(a["dlat"], b["dlat"]) <= 3e-4
    for k in a["params"]:   # Adam's first step is ~lr*sign(g): an element whose tiny gradient differs moves differently
        assert rel_err(a["params"][k], b["params"][k]) <= 1e-4, k
    # and against the oracle (fp32) for the same batch
    st = orc.TrainState.create({k: v.clone() for k, v in params.items()}, lat0.clone())
    ro = orc.train_step(net, st, idx, xyz, gt, delta=0.1, code_bound=1.0, epoch=300, batch_split=3, seed=77)
    assert abs(a["loss"] - ro["loss"]) <= 1e-5 * abs(ro["loss"])
    assert rel_err(a["dlat"], ro["dlat"]) <= 2e-4
    for k in ro["grads"]:
        assert rel_err(a["grads"][k], ro["grads"][k]) <= 3e-4, k     # not margin-safe: a few ReLU flips are expected


def test_empty_and_invalid_batches_are_rejected():
    import ctypes as C
    from deepsdf_amd import _lib
    from deepsdf_amd.engine import Engine, make_segments
    spec = spec_from_meta(dict(L=4, net_specs=dict(dims=[32] * 2, dropout=None, dropout_prob=0.0, norm_layers=[0, 1],
                                                   latent_in=(), weight_norm=True, geom_dimension=3)))
    eng = Engine(spec)
    eng.init_like_reference(torch.Generator().manual_seed(0))
    lat = torch.zeros(2, 4, device="cuda")
    dl = torch.zeros_like(lat)
    sc, so = make_segments(torch.zeros(8, dtype=torch.int64, device="cuda"))
    xyz, gt = torch.zeros(8, 3, device="cuda"), torch.zeros(8, device="cuda")
    with pytest.raises(_lib.DsdfError, match="n_norm must be positive"):
        eng.train_forward_backward(lat, dl, sc, so, xyz, gt, n_norm=0, clamp_dist=0.1, reg_coef=0.0, code_bound=None)
    with pytest.raises(_lib.DsdfError, match="empty batch"):
        eng.train_forward_backward(lat, dl, sc[:0], so[:1], xyz[:0], gt[:0], n_norm=8, clamp_dist=0.1, reg_coef=0.0, code_bound=None)
    with pytest.raises(_lib.DsdfError, match="n_norm must be positive"):      # the one-call fast path: a rejected step ...
        eng.train_step(lat, dl, torch.zeros_like(lat), torch.zeros_like(lat), sc, so, xyz, gt, n_norm=0, clamp_dist=0.1, reg_coef=0.0,
                       code_bound=None, lr_decoder=5e-4, lr_latent=1e-3)
    assert eng.step == 0                                                        # ... leaves Adam's bias-correction step alone
    with pytest.raises(ValueError, match="expected input"):
        eng.decode(torch.zeros(4, 3, device="cuda"))
    assert eng.decode(torch.zeros(0, 7, device="cuda")).shape == (0, 1)      # empty inference batch is a no-op


def test_fast_path_train_step_vs_oracle_full_size():
    """THE BENCHMARKED CALL (bench.py / FusedTrainStep: Engine.train_step -> dsdf_train_step, Adam folded into the finalize
    pass, gradient arena never written) against the float64 oracle at BASELINE config 2: 64 scenes x 256 pts, L=256, 8x512,
    dropout 0.2, THREE CONSECUTIVE steps without any re-synchronisation (train_deep_sdf.py:505-545).  Gradients are not
    observable on this path; they are pinned through Adam's first moment (step 1: exp_avg = 0.1 g) and second moment.
    After the last step the re-materialised packed weights (W, W^T, fragment copies, scales) are pinned by an eval forward
    through them against the oracle's forward with the oracle's post-Adam parameters."""
    from deepsdf_amd.engine import make_segments
    L, B, S = 256, 64, 256
    net, params, lat0, traj = _headline_trajectory(3)        # (one code above CodeBound: the renorm fires on the fast path)
    spec = spec_from_meta(dict(L=L, net_specs=BIG))
    tr = HipTrainer(spec, params, lat0)
    eng = tr.eng
    grads_before = eng.grads.clone()
    batches = []
    for step, t in enumerate(traj):
        idx, xyz, gt, r64, st64 = t["idx"], t["xyz"], t["gt"], t["r64"], t["after"]
        sc, so = make_segments(idx.cuda())
        eng.train_step(tr.lat, tr.dlat, tr.lat_m, tr.lat_v, sc, so, xyz.cuda().contiguous(), gt.reshape(-1).cuda().contiguous(),
                       n_norm=B * S, clamp_dist=0.1, reg_coef=1e-4 * min(1, 57 / 100), code_bound=1.0, lr_decoder=5e-4,
                       lr_latent=1e-3, seed=4242, seg_len=S)
        assert eng.step == st64.step == step + 1
        assert abs(float(eng.loss) - r64["loss"]) <= 1e-5 * abs(r64["loss"]), step
        P, M, V = tr.params(), tr.adam_m(), tr.adam_v()
        worst = dict(p=0.0, m=0.0, v=0.0)
        for k in st64.params:
            worst["p"] = max(worst["p"], rel_err(P[k], st64.params[k]))
            worst["m"] = max(worst["m"], rel_err(M[k], st64.m[k]))
            worst["v"] = max(worst["v"], rel_err(V[k], st64.v[k]))
            assert rel_err(P[k], st64.params[k]) <= PARAM_TOL, (step, k)
            assert rel_err(M[k], st64.m[k]) <= GRAD_TOL, (step, k)
            assert rel_err(V[k], st64.v[k]) <= 2 * GRAD_TOL, (step, k)
        print(f"fast path step {step}: worst rel err params {worst['p']:.2e}, exp_avg {worst['m']:.2e}, exp_avg_sq {worst['v']:.2e}")
        # element-wise: Adam's first moment IS the gradient here (exp_avg = 0.1 g after step 1), so its worst entry gets the
        # gradient's entry-wise bound; the parameters the Adam-step bound
        m_el = {k: worst_elem(M[k], st64.m[k]) for k in st64.params}
        p_el = max(float((P[k].double() - st64.params[k]).abs().max()) for k in st64.params) / 5e-4
        l_el = float((tr.lat.cpu().double() - st64.latents).abs().max()) / 1e-3
        print(f"fast path step {step}: worst exp_avg entry {max(m_el.values()):.2e} of its tensor's max ({max(m_el, key=m_el.get)}); "
              f"worst parameter entry {p_el:.2e}, worst code entry {l_el:.2e} of one Adam step")
        for k, e in m_el.items():
            assert e <= GRAD_ELEM_TOL, (step, k, e)
        assert worst_elem(tr.lat_m.cpu(), st64.m_lat) <= GRAD_ELEM_TOL, step
        assert p_el <= (step + 1) * PARAM_STEP_FRAC and l_el <= (step + 1) * PARAM_STEP_FRAC, step
        batches.append((sc, so, xyz.cuda().contiguous(), gt.reshape(-1).cuda().contiguous()))
        assert rel_err(tr.lat.cpu(), st64.latents) <= PARAM_TOL, step
        assert rel_err(tr.lat_m.cpu(), st64.m_lat) <= GRAD_TOL, step
        assert rel_err(tr.lat_v.cpu(), st64.v_lat) <= 2 * GRAD_TOL, step
    assert torch.equal(eng.grads, grads_before)             # the fast path really is the one that ran
    assert not eng.weights_dirty
    x = torch.cat([st64.latents[idx].float(), xyz], 1)
    yo = orc.decoder_forward(net, st64.params, x.double(), training=False)[0].reshape(-1)
    yh = eng.decode(x.cuda()).cpu().reshape(-1)
    assert rel_err(yh, yo) <= FWD_TOL and worst_elem(yh, yo) <= Y_ROW_TOL
    # the same three calls again from the same initial state: every reduction is fixed-order, so the whole optimiser state
    # must come out BIT-identical (parameters, both moments, codes and their moments, the re-materialised packed weights)
    tr2 = HipTrainer(spec, params, lat0)
    for sc, so, xc, gc in batches:
        tr2.eng.train_step(tr2.lat, tr2.dlat, tr2.lat_m, tr2.lat_v, sc, so, xc, gc, n_norm=B * S, clamp_dist=0.1,
                           reg_coef=1e-4 * min(1, 57 / 100), code_bound=1.0, lr_decoder=5e-4, lr_latent=1e-3, seed=4242, seg_len=S)
    for name in ("params", "exp_avg", "exp_avg_sq", "packed", "loss"):
        assert torch.equal(getattr(tr2.eng, name), getattr(eng, name)), name
    for name in ("lat", "lat_m", "lat_v", "dlat"):
        assert torch.equal(getattr(tr2, name), getattr(tr, name)), name


@pytest.mark.parametrize("S", [8000, 8001], ids=["8000_segment_mode", "8001_ragged"])
def test_config4_reconstruct_full_size_vs_oracle(S):
    """BASELINE config 4 at full size: reconstruct() (frozen 8x512 decoder in eval mode, Adam on the codes only) against
    oracle.latent_step in float64, 6 iterations, TWO shapes at once (each shape must follow its own single-code oracle
    trajectory).  S = 8000 = 125 x 64 is the configured count and what reconstruct.py uses: whole 64-point workgroups per shape,
    i.e. SEGMENT MODE (the code's products hoisted, the latent gradient from per-workgroup column sums).  S = 8001 is not a
    multiple of 64 and takes the general (ragged) frozen-decoder path: gather + full per-point dX chain + seg_reduce."""
    from deepsdf_amd.engine import Engine
    from deepsdf_amd.reconstruct import reconstruct
    L, Bz, iters = 256, 2, 6
    net = orc.make_net(L, **BIG)
    params = orc.init_params(net, 41)
    p64 = {k: v.double() for k, v in params.items()}
    eng = Engine(spec_from_meta(dict(L=L, net_specs=BIG)))
    eng.load_params(params)
    gen = torch.Generator().manual_seed(42)
    z0 = torch.randn(Bz, L, generator=gen) * 0.01
    c = (torch.rand(Bz, 3, generator=gen) - 0.5) * 0.6
    r = 0.3 + 0.3 * torch.rand(Bz, generator=gen)
    zo = z0.double().clone()
    mo, vo = torch.zeros_like(zo), torch.zeros_like(zo)
    batches = []
    for it in range(iters):
        xyz = torch.rand(Bz, S, 3, generator=gen) * 2 - 1
        half = S // 2
        d = torch.randn(Bz, half, 3, generator=gen)
        xyz[:, :half] = c[:, None, :] + r[:, None, None] * d / d.norm(dim=2, keepdim=True) + 0.05 * torch.randn(Bz, half, 3, generator=gen)
        sdf = (xyz - c[:, None, :]).norm(dim=2) - r[:, None]
        for b in range(Bz):
            assert (S % 64 == 0) == (S == 8000)
            # margin-safe points (as _safe_batch: a clamp / sign flip of ONE point moves 1/S = 1.3e-4 of the code's gradient, and
            # Adam's early steps ~ lr * g / |g| pass that on undamped): re-draw what the float64 oracle calls close
            for _ in range(12):
                x0 = torch.cat([zo[b:b + 1].expand(S, -1), xyz[b].double()], 1)
                y, sv = orc.decoder_forward(net, p64, x0, training=False, track_margin=True)
                dd = torch.clamp(y, -0.1, 0.1) - torch.clamp(sdf[b].double().reshape(-1, 1), -0.1, 0.1)
                risky = (((y.abs() - 0.1).abs() < 2e-5) | ((dd != 0) & (dd.abs() < 2e-5))).reshape(-1) | (sv.min_abs_pre < 1e-6)
                if not bool(risky.any()):
                    break
                k = int(risky.sum())
                xyz[b, risky] = torch.rand(k, 3, generator=gen) * 2 - 1
                sdf[b, risky] = (torch.rand(k, generator=gen) - 0.5) * 0.4
            else:
                raise RuntimeError("could not build a margin-safe batch")
            zb, mb, vb = zo[b:b + 1], mo[b:b + 1], vo[b:b + 1]           # views: latent_step mutates them in place
            orc.latent_step(net, p64, zb, mb, vb, it + 1, xyz[b].double(), sdf[b].double(), delta=0.1,
                            lr=5e-3 * (0.1 if it >= 3 else 1.0), l2reg=1e-4)
        batches.append((xyz, sdf))
    grads_before = eng.grads.clone()
    zh, loss = reconstruct(eng, batches[0][0].cuda(), batches[0][1].cuda(), num_iterations=iters, clamp_dist=0.1, lr=5e-3,
                           l2reg=1e-4, z0=z0, lr_drop_every=3, callback=lambda it: (batches[it][0].cuda(), batches[it][1].cuda()))
    e = rel_err(zh.cpu(), zo)
    print(f"config 4, S={S}: code rel err vs fp64 oracle after {iters} iterations {e:.2e}")
    assert e <= PARAM_TOL
    assert torch.equal(eng.grads, grads_before)


def test_all_decoder_variants_together_vs_oracle():
    """xyz_in_all + latent_dropout + LayerNorm in ONE net (deep_sdf_decoder.py:79-82, 90-91, 60-65/97-103; each is pinned
    separately by the reference-generated goldens g11a/b/c), a skip layer, dropout, use_tanh, widths off every tile grid:
    two optimiser steps against the float64 oracle, unsplit and with --batch_split 3 (ragged chunks)."""
    kw = dict(dims=[70, 70, 70, 72], dropout=[0, 1, 2, 3], dropout_prob=0.2, norm_layers=[0, 1, 3, 4], latent_in=[2], weight_norm=False,
              xyz_in_all=True, latent_dropout=True, use_tanh=True, geom_dimension=3)
    L, B, S = 9, 5, 96
    net = orc.make_net(L, **kw)
    spec = spec_from_meta(dict(L=L, net_specs=kw))
    params = orc.init_params(net, 91)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(92)) / math.sqrt(L)
    lat0[1] *= 1.4 / lat0[1].norm()
    for split in (1, 3):
        st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
        tr = HipTrainer(spec, params, lat0)
        for step in range(2):
            if split == 1:
                idx, xyz, gt = _safe_batch(net, st64, B, S, 800 + step, 0.1, 1.0, 55)
            else:
                idx, xyz, gt = _big_batch(B, S, 810 + step)          # chunked masks restart per chunk: margins not pre-screened
            r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=40, seed=55,
                                 batch_split=split)
            rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=40, lr=(5e-4, 1e-3), seed=55,
                         batch_split=split)
            tol = GRAD_TOL if split == 1 else 5 * GRAD_TOL
            assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), (split, step)
            for k in r64["grads"]:
                if float(r64["grads"][k].abs().max()) == 0.0:       # the unused bn module of the last Linear
                    assert float(rh["grads"][k].abs().max()) == 0.0, k
                else:
                    assert rel_err(rh["grads"][k], r64["grads"][k]) <= tol, (split, step, k)
            assert rel_err(rh["dlat"], r64["dlat"]) <= tol, (split, step)
            if split == 1:
                P = tr.params()
                for k in st64.params:
                    assert rel_err(P[k], st64.params[k]) <= PARAM_TOL, (step, k)
                assert rel_err(tr.lat.cpu(), st64.latents) <= PARAM_TOL, step


def test_fast_path_with_a_512_scene_table_vs_oracle():
    """BASELINE config 3's per-rank state on the one-call fast path: a latent table of 512 scenes of which a step touches 64
    (different ones each step): the dense Adam keeps moving rows that are absent from the batch by their momentum
    (train_deep_sdf.py:400-411,545), the max-norm renorm only fires for looked-up rows.  Three steps, fp64 oracle."""
    from deepsdf_amd.engine import make_segments
    L, T, B, S = 256, 512, 64, 64
    net = orc.make_net(L, **BIG)
    spec = spec_from_meta(dict(L=L, net_specs=BIG))
    params = orc.init_params(net, 71)
    gen = torch.Generator().manual_seed(72)
    lat0 = torch.randn(T, L, generator=gen) / math.sqrt(L)
    lat0[::37] *= 1.5                                        # several rows above CodeBound, only some of them ever looked up
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    tr = HipTrainer(spec, params, lat0)
    seen = torch.zeros(T, dtype=torch.bool)
    for step in range(3):
        scenes = torch.randperm(T, generator=gen)[:B].sort().values
        idx, xyz, gt = _safe_batch(net, st64, B, S, 950 + step, 0.1, 1.0, 7, scenes=scenes)
        before = st64.latents.clone()
        r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=57, seed=7)
        sc, so = make_segments(idx.cuda())
        tr.eng.train_step(tr.lat, tr.dlat, tr.lat_m, tr.lat_v, sc, so, xyz.cuda().contiguous(), gt.reshape(-1).cuda().contiguous(),
                          n_norm=B * S, clamp_dist=0.1, reg_coef=1e-4 * 0.57, code_bound=1.0, lr_decoder=5e-4, lr_latent=1e-3,
                          seed=7, seg_len=S)
        assert abs(float(tr.eng.loss) - r64["loss"]) <= 1e-5 * abs(r64["loss"]), step
        lat = tr.lat.cpu()
        absent_moved = (~seen) & (~torch.isin(torch.arange(T), scenes))
        assert torch.equal(lat[absent_moved], lat0[absent_moved])                            # never-seen rows do not move at all
        prev_seen_absent = seen & (~torch.isin(torch.arange(T), scenes))
        if bool(prev_seen_absent.any()):                                                       # seen before, absent now: momentum only
            assert float((st64.latents[prev_seen_absent] - before[prev_seen_absent]).abs().max()) > 0
        assert rel_err(lat, st64.latents) <= PARAM_TOL, step
        assert rel_err(tr.lat_m.cpu(), st64.m_lat) <= GRAD_TOL and rel_err(tr.lat_v.cpu(), st64.v_lat) <= 2 * GRAD_TOL, step
        seen |= torch.isin(torch.arange(T), scenes)
    P = tr.params()
    for k in st64.params:
        assert rel_err(P[k], st64.params[k]) <= PARAM_TOL, k


@pytest.mark.parametrize("L", [2, 16])
def test_shipped_experiment_shapes_vs_oracle(L):
    """The shapes the reference actually SHIPS for its 8 x 512 experiments: CodeLength 2 (experiments/double_lattice_3D/specs.json:9-38,
    snappy_and_cylinders) and 16 (simple_geom/specs.json:20, snappy3D, corner_spheres_only), SamplesPerScene 16000, latent_in [4]:
    the skip layer is 507 / 493 wide and x0 has 5 / 19 columns (the headline's L = 256 makes them 253 / 259).  Two optimiser steps
    of 2 scenes x 16000 points against the float64 oracle on margin-safe batches, through all four product paths: segment mode
    (16000 = 250 workgroups per scene) and the general (ragged) path, fp32 MFMA and gemm_split -- the headline's tolerances,
    norm-wise and element-wise."""
    B, S = 2, 16000
    net = orc.make_net(L, **BIG)
    params = orc.init_params(net, 200 + L)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(201 + L)) / math.sqrt(L)
    lat0[1] *= 1.3 / lat0[1].norm()                          # above CodeBound: the renorm fires
    st64 = orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double())
    assert net.layers[3].out_dim == 512 - (L + 3) and net.layers[0].in_dim == L + 3
    paths = {(ragged, split): HipTrainer(spec_from_meta(dict(L=L, net_specs=dict(BIG, gemm_split=split))), params, lat0)
             for ragged in (False, True) for split in (False, True)}
    for step in range(2):
        idx, xyz, gt = _safe_batch(net, st64, B, S, 1200 + 10 * L + step, 0.1, 1.0, 31)
        r64 = orc.train_step(net, st64, idx, xyz.double(), gt.double(), delta=0.1, code_bound=1.0, epoch=57, seed=31)
        for (ragged, split), tr in paths.items():
            tag = (L, step, "ragged" if ragged else "segments", "gemm_split" if split else "fp32mfma")
            rh = tr.step(idx, xyz, gt, delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=57, lr=(5e-4, 1e-3), seed=31,
                         want_y=True, **(dict(force_ragged=True) if ragged else {}))
            assert abs(rh["loss"] - r64["loss"]) <= 1e-5 * abs(r64["loss"]), tag
            assert rel_err(rh["y"], r64["y"]) <= FWD_TOL and worst_elem(rh["y"], r64["y"]) <= Y_ROW_TOL, tag
            g_rel = {k: rel_err(rh["grads"][k], r64["grads"][k]) for k in r64["grads"]}
            g_el = {k: worst_elem(rh["grads"][k], r64["grads"][k]) for k in r64["grads"]}
            P = tr.params()
            p_rel = max(rel_err(P[k], st64.params[k]) for k in st64.params)
            p_el = max(float((P[k].double() - st64.params[k]).abs().max()) for k in st64.params) / 5e-4
            print(f"{tag}: gradients rel {max(g_rel.values()):.2e} / worst entry {max(g_el.values()):.2e} ({max(g_el, key=g_el.get)}); "
                  f"y worst row {worst_elem(rh['y'], r64['y']):.2e}; params rel {p_rel:.2e} / worst entry {p_el:.2e} of an Adam step; "
                  f"codes rel {rel_err(tr.lat.cpu(), st64.latents):.2e}")
            for k in r64["grads"]:
                assert g_rel[k] <= GRAD_TOL and g_el[k] <= GRAD_ELEM_TOL, (tag, k, g_rel[k], g_el[k])
            assert rel_err(rh["dlat"], r64["dlat"]) <= GRAD_TOL and worst_elem(rh["dlat"], r64["dlat"]) <= GRAD_ELEM_TOL, tag
            assert p_rel <= PARAM_TOL and p_el <= (step + 1) * (PARAM_STEP_FRAC_SPLIT if split else PARAM_STEP_FRAC), tag
            assert rel_err(tr.lat.cpu(), st64.latents) <= PARAM_TOL, tag


_SHIPPED_SMALL = dict(dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)), xyz_in_all=False, latent_dropout=False,
                      weight_norm=True, geom_dimension=3)
BIG_BATCH_NETS = {
    "8x512": (16, BIG, "lin8.bias"),
    # the reference's shipped small specs (experiments/*/specs.json; bench.py --network): the narrow-net kernels and a weight-gradient
    # launch made of narrow items only, at a batch size their parity tests do not reach
    "6x128": (1, dict(_SHIPPED_SMALL, dims=[128] * 6, latent_in=[2], use_tanh=False), "lin6.bias"),
    "4x64_tanh": (2, dict(_SHIPPED_SMALL, dims=[64] * 4, latent_in=[1], use_tanh=True), "lin4.bias"),
    "4x32": (2, dict(_SHIPPED_SMALL, dims=[32] * 4, latent_in=[2], use_tanh=False), "lin4.bias"),
}


@pytest.mark.parametrize("name", sorted(BIG_BATCH_NETS))
def test_batch_above_65536_points_equals_its_accumulated_chunks(name):
    """A size-independent property at a size the oracle cannot reach in seconds: one call on 98304 points (6 scenes x 16384: 1536
    workgroups) must equal the same batch fed as three accumulated --batch_split chunks of 32768 points (512 workgroups each,
    every chunk with the full batch's normaliser and its own row offset into the dropout hash) -- loss, every decoder gradient and
    the latent gradient, up to fp32 summation order.  Rounds 1-3 sized the fused head's per-workgroup partials for at most 1024
    workgroups: above 65536 points they overran into the loss / last-bias partials (the reference's shipped 10 x 16000 batches)."""
    L, kwn, last_bias = BIG_BATCH_NETS[name]
    B, S = 6, 16384
    net = orc.make_net(L, **kwn)
    spec = spec_from_meta(dict(L=L, net_specs=kwn))
    params = orc.init_params(net, 91)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(92)) / math.sqrt(L)
    idx, xyz, gt = _big_batch(B, S, 93)
    kw = dict(delta=0.1, code_bound=1.0, code_reg=True, lam=1e-4, epoch=57, lr=(5e-4, 1e-3), seed=12, do_adam=False)
    one, three = HipTrainer(spec, params, lat0), HipTrainer(spec, params, lat0)
    r1 = one.step(idx, xyz, gt, **kw)
    r3 = three.step(idx, xyz, gt, batch_split=3, **kw)
    assert math.isfinite(r1["loss"]) and r1["loss"] > 0
    print(f"98304 points, one call vs three chunks: loss {r1['loss']:.8f} / {r3['loss']:.8f}; worst gradient rel diff "
          f"{max(rel_err(r1['grads'][k], r3['grads'][k]) for k in r1['grads']):.2e}")
    assert abs(r1["loss"] - r3["loss"]) <= 2e-6 * abs(r3["loss"])
    for k in r1["grads"]:
        assert rel_err(r1["grads"][k], r3["grads"][k]) <= 1e-5 and worst_elem(r1["grads"][k], r3["grads"][k]) <= 1e-4, k
    assert rel_err(r1["dlat"], r3["dlat"]) <= 1e-5
    # the last layer's bias gradient is the head's other per-workgroup partial: pinned on its own
    kb = [k for k in r1["grads"] if k.endswith(last_bias)]
    assert len(kb) == 1 and abs(float(r1["grads"][kb[0]]) - float(r3["grads"][kb[0]])) <= 1e-5 * abs(float(r3["grads"][kb[0]])) + 1e-9


PHASE_NETS = {
    "8x512_headline": dict(L=256, B=64, S=256, net=BIG),
    "8x512_shipped_L2": dict(L=2, B=4, S=1024, net=BIG),
    "3x72_noskip": dict(L=7, B=3, S=128, net=dict(dims=[72, 72, 72], dropout=[0, 1], dropout_prob=0.2, norm_layers=[0, 1, 2], latent_in=[],
                                                    weight_norm=True, geom_dimension=3)),
    "2x64_skip1": dict(L=9, B=2, S=192, net=dict(dims=[64, 64], dropout=[], dropout_prob=0.0, norm_layers=[0, 1], latent_in=[1],
                                                  weight_norm=True, geom_dimension=3)),
}


@pytest.mark.parametrize("ragged", [False, True], ids=["segments", "ragged"])
@pytest.mark.parametrize("K", [2, 4, 8], ids=["K2", "K4", "K8"])
@pytest.mark.parametrize("name", sorted(PHASE_NETS))
def test_phased_backward_equals_the_single_call(name, K, ragged):
    """DsdfLossCfg.dw_phase / dw_buckets (the K-bucket gradient exchange of a data-parallel step): phase 1 = forward, backward and
    the weight gradients of bucket 0 (the LAST layers), phase p = the weight gradients of bucket p - 1 from what phase 1 left in
    the workspace.  Against the single call on the same batch: loss, forward and latent gradient bit-identical (the same launches
    produce them), weight gradients equal to summation order (a bucket's launch splits K finer); after phase p the buckets
    [0, p) are final and the others untouched.  K = 8 on the small nets leaves trailing buckets EMPTY (fewer layers than
    buckets)."""
    if K == 8 and ragged and name.startswith("8x512"):
        pytest.skip("K = 8 on the big net is covered in segment mode; the ragged path differs only in launches phase 1 owns")
    c = PHASE_NETS[name]
    L, B, S = c["L"], c["B"], c["S"]
    spec = spec_from_meta(dict(L=L, net_specs=c["net"]))
    params = orc.init_params(orc.make_net(L, **c["net"]), 77)
    lat0 = torch.randn(B, L, generator=torch.Generator().manual_seed(78)) / math.sqrt(L)
    idx, xyz, gt = _big_batch(B, S, 79)
    from deepsdf_amd.engine import make_segments
    one, two = HipTrainer(spec, params, lat0), HipTrainer(spec, params, lat0)
    assert one.eng.dw_phase_supported()
    first, off = one.eng.grad_buckets(K)
    assert off[0] == spec.n_params and off[K] == 0 and all(off[b + 1] <= off[b] for b in range(K))
    assert off[1] < spec.n_params and first[K - 1] == 0 and all(first[b + 1] <= first[b] for b in range(K - 1))
    for b in range(K):                                          # a bucket's arena range is exactly its layers' parameters
        lo_l, hi_l = first[b], (first[b - 1] if b else spec.n_layers)
        assert off[b] - off[b + 1] == sum(p.numel for p in spec.params if lo_l <= p.layer < hi_l), b
    if K == 2:
        assert one.eng.grad_bucket_split() == (first[0], off[1])
    sc, so = make_segments(idx.cuda())
    xc, gc = xyz.cuda().contiguous(), gt.reshape(-1).cuda().contiguous()
    kw = dict(n_norm=B * S, clamp_dist=0.1, reg_coef=1e-4, code_bound=1.0, training=True, seed=5, seg_len=0 if ragged else S)
    y1, y2 = torch.empty(B * S, device="cuda"), torch.empty(B * S, device="cuda")
    one.eng.train_forward_backward(one.lat, one.dlat, sc, so, xc, gc, sdf_out=y1, **kw)
    two.eng.grads.fill_(float("nan"))                          # whatever a phase does not write stays NaN
    for p in range(1, K + 1):
        before = two.eng.grads.clone()
        two.eng.train_forward_backward(two.lat, two.dlat, sc, so, xc, gc, sdf_out=y2 if p == 1 else None, dw_phase=p, dw_buckets=K, **kw)
        g = two.eng.grads
        assert bool(torch.isnan(g[:off[p]]).all()) and not bool(torch.isnan(g[off[p]:]).any()), p
        assert torch.equal(g[off[p - 1]:], before[off[p - 1]:]), p      # phase p leaves the finished buckets alone
    assert torch.equal(y1, y2) and torch.equal(one.eng.loss, two.eng.loss)
    # the latent gradient: the same per-workgroup column sums go through the per-segment role, which exists in two forms with their
    # own (fixed) summation orders -- riding on a weight-gradient launch with spare workgroups, or as a launch of its own -- and a
    # bucket's launch need not make the same choice as the whole launch: equal to rounding, not to the bit
    assert rel_err(two.dlat.cpu(), one.dlat.cpu()) <= 1e-6 and worst_elem(two.dlat.cpu(), one.dlat.cpu()) <= 1e-5
    assert torch.equal(one.lat, two.lat)                        # (the renorm ran once, in phase 1)
    g1, g2 = one.eng.named_views(one.eng.grads), two.eng.named_views(two.eng.grads)
    worst = max(rel_err(g2[n].cpu(), g1[n].cpu()) for n in g1)
    print(f"{name} K={K} {'ragged' if ragged else 'segments'}: phased vs single-call weight gradients, worst rel {worst:.2e}")
    for n in g1:
        assert rel_err(g2[n].cpu(), g1[n].cpu()) <= 2e-6 and worst_elem(g2[n].cpu(), g1[n].cpu()) <= 1e-5, n
    # a second phased run reproduces the first bit for bit
    again = HipTrainer(spec, params, lat0)
    for p in range(1, K + 1):
        again.eng.train_forward_backward(again.lat, again.dlat, sc, so, xc, gc, dw_phase=p, dw_buckets=K, **kw)
    assert torch.equal(again.eng.grads, two.eng.grads)
    # phases are refused where they cannot work: gradient accumulation (batch_split chunks), a frozen decoder, a phase without or
    # beyond its bucket count
    from deepsdf_amd._lib import DsdfError
    with pytest.raises(DsdfError, match="dw_phase"):
        two.eng.train_forward_backward(two.lat, two.dlat, sc, so, xc, gc, dw_phase=1, dw_buckets=K, accumulate=True, **kw)
    with pytest.raises(DsdfError, match="dw_phase"):
        two.eng.train_forward_backward(two.lat, two.dlat, sc, so, xc, gc, dw_phase=2, dw_buckets=K, frozen_decoder=True, **kw)
    with pytest.raises(DsdfError, match="dw_phase"):
        two.eng.train_forward_backward(two.lat, two.dlat, sc, so, xc, gc, dw_phase=K + 1, dw_buckets=K, **kw)
    with pytest.raises(DsdfError, match="dw_phase"):
        two.eng.train_forward_backward(two.lat, two.dlat, sc, so, xc, gc, dw_phase=1, dw_buckets=1, **kw)
