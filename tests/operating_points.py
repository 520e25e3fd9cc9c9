"""Operating points of the training step away from the reference's one set of constants, the cases the tests run them on, and a batch
builder that populates every region of the loss head (torch and numpy on the CPU only).

Every continuous input of the step that the C ABI carries -- clamp_dist, code_bound, reg_coef (lambda x ramp), n_norm, and Adam's lr, beta1,
beta2, eps -- is an argument a user sets through specs.json, yet every other test runs them at CodeBound 1.0, ClampingDistance 0.1,
lambda 1e-4 and torch's Adam defaults.  At code_bound = 1 a renorm scale 1 / (nu + 1e-7), a threshold nu > 1 and a compare ss > max_norm
all give the bits of the right formula; a hard-coded 0.1 or 0.999 passes everywhere.  POINTS moves each input off that point at least
once, `covers` names the wrong variants (VARIANTS: small pure functions patched into the oracle) a point must tell from the truth, and
tests/test_operating_points_cpu.py proves on the CPU that it does -- by at least 100 times the bound the GPU test asserts.

The oracle is evaluated at the float32-rounded values the ABI carries (optim_numpy.f32), as optim_numpy does for Adam's constants:
float(0.03) differs from 0.03 by 2e-9 relative, which is an input of the kernels, not an error of theirs.
"""
import contextlib
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import deepsdf_oracle as orc
from tests.golden_io import rel_err
from tests.optim_numpy import f32

MARGIN, RELU_MARGIN, MIN_DIFF, REDRAWS = 2e-5, 1e-6, 1e-3, 12      # safe_batch's two margins; the smallest non-zero |clamp(y) - clamp(gt)|
DROP_SEED = 91


@dataclass(frozen=True)
class Point:
    name: str
    delta: float = 0.1
    code_bound: Optional[float] = 1.0
    lam: float = 1e-4
    epoch: int = 130
    code_reg: bool = True
    lr: Tuple[float, float] = (5e-4, 1e-3)          # (decoder, latent)
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    n_norm_factor: int = 1                          # n_norm / N
    clip_factor: Optional[float] = None             # grad_clip = clip_factor x the oracle's own gradient norm (< 1: fires, > 1: does not)
    dropout_prob: float = 0.2
    out_gain: Tuple[Tuple[str, float], ...] = ()    # per net kind: the output layer's initial weight and bias times this (absent: 1)
    covers: Tuple[str, ...] = ()                    # the VARIANTS this point must tell from the truth

    @property
    def ramp(self):
        return min(1, self.epoch / 100)

    @property
    def reg_coef(self):                             # what the trainer hands to the ABI as DsdfLossCfg.reg_coef
        return self.lam * self.ramp if self.code_reg else 0.0


HEAD = ("sign_minus_one", "inside_mask_dropped")    # told apart wherever the head's regions are populated, i.e. at every point
REFERENCE = Point("reference")                      # the one point of every other test (code_bound 1: the three renorm variants move NOTHING)
POINTS = [
    Point("cb0.6_delta0.03", delta=0.03, code_bound=0.6, covers=("renorm_threshold_one", "renorm_no_max_norm", "renorm_compare_ss", "delta_fixed") + HEAD),
    # (a freshly initialised decoder's |y| stays below 0.2: here the output layer is scaled up, by a factor chosen per net, so that 40-75 %
    # of the oracle's |y| lie inside 0.4 at both steps and the point runs at the delta it names)
    Point("cb2.5_delta0.4", delta=0.4, code_bound=2.5, dropout_prob=0.0, out_gain=(("main", 16.0), ("w32", 12.0), ("variant", 10.0)),
          covers=("renorm_threshold_one", "renorm_no_max_norm", "renorm_compare_ss", "delta_fixed") + HEAD),
    Point("cb_none", code_bound=None, covers=HEAD),
    Point("cb_zero", code_bound=0.0, dropout_prob=0.0, covers=HEAD),
    Point("lam1e-2_epoch37", lam=1e-2, epoch=37, covers=("reg_dropped", "reg_no_ramp") + HEAD),
    Point("lam1e-2_epoch130", lam=1e-2, epoch=130, code_bound=0.6, covers=("reg_dropped",) + HEAD),
    Point("no_code_reg", code_reg=False, lam=1e-2, covers=HEAD),
    Point("betas_eps", betas=(0.8, 0.95), eps=1e-5, delta=0.03, covers=("default_betas", "default_eps") + HEAD),
    Point("eps_only", eps=1e-5, dropout_prob=0.0, covers=("default_eps",) + HEAD),
    Point("lr_swapped", lr=(2e-3, 3e-4), code_bound=2.5, covers=HEAD),
    Point("n_norm_3N", n_norm_factor=3, lam=1e-2, covers=("reg_by_N", "inv_n_from_N") + HEAD),
    Point("clip_fires", clip_factor=0.37, delta=0.4, covers=HEAD),
    Point("clip_idle", clip_factor=2.0, dropout_prob=0.0, covers=HEAD),
]
BY_NAME = {p.name: p for p in POINTS + [REFERENCE]}


# ---- nets, tables and segment layouts: the smallest shapes that still reach the code ---------------------------------------------------
def net_kw(kind, dropout_prob):
    """main: three hidden layers of 64 / 72 / 64 with L = 5, a skip layer (in front of the second hidden layer: a skip in front of the
    deepest one has no segment mode) and weight norm on some layers (the fused kernels: 32-point
    workgroups, the narrow-net kernels, the full-size kernels); w32: two layers of 32 with L = 2 (the wave-private kernels); variant: the
    main net with xyz_in_all, which only the layer-by-layer kernels run (last_layer_kernel's head)."""
    drop = dict(dropout=[0, 1], dropout_prob=dropout_prob) if dropout_prob > 0 else dict(dropout=[], dropout_prob=0.0)
    if kind == "w32":
        return 2, dict(dims=[32, 32], norm_layers=[0, 1], latent_in=[], weight_norm=True, geom_dimension=3, **drop)
    kw = dict(dims=[64, 72, 64], norm_layers=[0, 2], latent_in=[1], weight_norm=True, geom_dimension=3, **drop)
    if kind == "variant":
        kw["xyz_in_all"] = True
    return 5, kw


# initialisation seed offset per net: the 32-wide net's y is positive throughout at most seeds, which would leave the two mirror regions
# (y < -delta) to the other nets; at this one its y straddles 0 at every point
KIND_SEED = {"main": 0, "variant": 0, "w32": 6}
TABLE_ROWS = 7
SCENES = (3, 0, 4, 1)                               # rows 2, 5 and 6 of the table are never looked up
LAYOUTS = {
    "segment": (SCENES, (64, 64, 64, 64)),          # B = 4 scenes of 64 points: segment mode, renorm in the hoist kernel
    "ragged": (SCENES + (0,), (40, 33, 40, 40, 7)),  # scene 0 in two segments: the general path, latent_renorm_kernel
}


def table_norms(code_bound):
    """Row norms of the 7-row table, by table row.  The looked-up rows 3, 0, 4, 1 sit, for code_bound 0.6, below 0.6 (untouched), in
    (0.6, sqrt 0.6), in (sqrt 0.6, 1) and well above 1 (all three scaled); for 2.5 in (1, sqrt 2.5), in (sqrt 2.5, 2.5) (both untouched),
    above 2.5 (scaled) and below 1.  Rows 2, 5, 6 are above every bound: a renorm that touched them would show."""
    if code_bound is not None and code_bound > 1.5:
        return {3: 1.3, 0: 2.0, 4: 3.1, 1: 0.8, 2: 3.3, 5: 2.7, 6: 4.0}
    return {3: 0.4, 0: 0.7, 4: 0.9, 1: 1.9, 2: 2.2, 5: 1.7, 6: 3.0}


def latent_table(L, code_bound, seed):
    lat = torch.randn(TABLE_ROWS, L, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    for r, n in table_norms(code_bound).items():
        lat[r] *= n / lat[r].norm()
    return lat.float()                              # what the device holds; the oracle runs on its exact double image


# ---- the batch builder -----------------------------------------------------------------------------------------------------------------
REGIONS = ("in_neg", "in_pos", "hi_loss", "hi_zero", "lo_loss", "lo_zero")


def regions(y, gt, delta):
    """Region of every point, by the oracle's y: inside the band with diff < 0 / > 0; y > delta with gt < delta (loss, no gradient) or
    gt >= delta (exactly zero loss); the two mirror images for y < -delta.  Returns (dict name -> bool mask, diff)."""
    y, gt = y.reshape(-1).double(), gt.reshape(-1).double()
    d = torch.clamp(y, -delta, delta) - torch.clamp(gt, -delta, delta)
    ins, hi, lo = y.abs() <= delta, y > delta, y < -delta
    return {"in_neg": ins & (d < 0), "in_pos": ins & (d > 0), "hi_loss": hi & (gt < delta), "hi_zero": hi & (gt >= delta),
            "lo_loss": lo & (gt > -delta), "lo_zero": lo & (gt <= -delta)}, d


def check_populations(y, gt, delta):
    """The conditions of DESIGN.md 4.19 on a batch, from the oracle alone.  Returns the fractions."""
    reg, d = regions(y, gt, delta)
    n = y.numel()
    f = {k: float(v.sum()) / n for k, v in reg.items()}
    assert abs(sum(f.values()) - 1.0) < 1e-12, f                  # every point is in exactly one region (no diff == 0 inside the band)
    assert f["in_neg"] >= 0.10 and f["in_pos"] >= 0.10, f
    out = f["hi_loss"] + f["hi_zero"] + f["lo_loss"] + f["lo_zero"]
    assert out >= 0.20, f
    assert f["hi_loss"] + f["lo_loss"] >= 0.05 and f["hi_zero"] + f["lo_zero"] >= 0.05, f      # (5 % of ALL points: the stronger reading)
    assert bool((d[reg["hi_zero"] | reg["lo_zero"]] == 0).all())
    nz = d[d != 0].abs()
    assert float(nz.min()) >= MIN_DIFF, float(nz.min())
    return f


def choose_delta(abs_y, delta):
    """The point's delta where it leaves at least 40 % of |y| inside the band and a quarter outside; else the 0.65 quantile of the oracle's |y|, rounded to
    float32 (a random decoder's |y| can all lie inside 0.4, or nearly all outside 0.03)."""
    below = float((abs_y < delta).double().mean())
    if 0.40 <= below <= 0.75:
        return f32(delta)
    return f32(float(torch.quantile(abs_y.double(), 0.65)))


def _targets(y, delta, gen, k0=0):
    """Targets from the oracle's own y, regions dealt round-robin so every one is populated by construction.  Inside the band two
    points in three get diff < 0: dealt evenly, the signs would cancel the output layer's bias gradient (sum of sign x (1 - y^2) / n) to
    1e-3 of its terms, and the fp32 CPU oracle itself would sit 1e-3 from the fp64 one on that tensor -- conditioning, not a kernel's error."""
    y = y.reshape(-1)
    gt = torch.empty_like(y)
    u = torch.rand(y.numel(), generator=gen, dtype=torch.float64)
    count = {0: k0, 1: k0, -1: k0}                   # a counter per side (inside, above, below): a region's turn does not depend on
    for i in range(y.numel()):                       # where in the batch its points happen to sit
        yi = float(y[i])
        side = 0 if abs(yi) <= delta else (1 if yi > 0 else -1)
        k = count[side]
        count[side] += 1
        if side == 0:                         # inside: diff < 0 (target above y, possibly above the band) or > 0
            off = 2 * MIN_DIFF + u[i] * 0.5 * delta
            gt[i] = yi - off if k % 3 == 0 else yi + off
        else:
            s = 1.0 if yi > 0 else -1.0
            if k % 2 == 0:                           # zero loss: the target beyond the same edge
                gt[i] = s * (delta + 2 * MIN_DIFF + u[i] * 0.3)
            elif k % 4 == 1:                         # loss without gradient: the target inside the band ...
                gt[i] = s * (delta - 2 * MIN_DIFF - u[i] * (2 * delta - 4 * MIN_DIFF))
            else:                                    # ... or beyond the opposite edge
                gt[i] = -s * (delta + u[i] * 0.2)
    return gt


def region_batch(net, st64, scenes, lens, seed, delta, code_bound, drop_seed=DROP_SEED, row_offset=0):
    """A batch on safe_batch's rules -- no point within 2e-5 of a clamp or sign decision, no hidden pre-activation within 1e-6 of 0, decided
    by the fp64 oracle on the renormed table and the step's own dropout masks -- whose targets are chosen FROM the oracle's y, so that every
    region of the head is populated.  Inside the band a diff with |diff| < 1e-3 cannot arise except where a target is clamped: such points
    are re-drawn, like the risky ones.  Raises after REDRAWS rounds.  Returns (idx, xyz float32 [N, G], gt float32 [N, 1], delta used)."""
    G = net.geom_dimension
    idx = torch.tensor(scenes, dtype=torch.int64).repeat_interleave(torch.tensor(lens, dtype=torch.int64))
    N = idx.numel()
    gen = torch.Generator().manual_seed(seed)
    xyz = torch.rand(N, G, generator=gen) * 2 - 1
    lat = st64.latents.clone()
    orc.renorm_rows_(lat, idx, code_bound)
    masks = orc.dropout_masks(net, drop_seed, st64.step, N, row_offset=row_offset)
    lmask = orc.latent_dropout_mask(net, drop_seed, st64.step, N, row_offset=row_offset) if net.latent_dropout else None

    def fwd():
        x0 = torch.cat([lat[idx], xyz.double()], 1)
        y, sv = orc.decoder_forward(net, st64.params, x0, training=True, masks=masks, track_margin=True, latent_mask=lmask)
        return y.reshape(-1), sv.min_abs_pre

    y, pre = fwd()
    delta = choose_delta(y.abs(), delta)
    gt = _targets(y, delta, gen).float()
    for rnd in range(REDRAWS):
        d = torch.clamp(y, -delta, delta) - torch.clamp(gt.double(), -delta, delta)
        risky = ((y.abs() - delta).abs() < MARGIN) | ((d != 0) & (d.abs() < MIN_DIFF)) | (pre < RELU_MARGIN)
        risky |= (d == 0) & (y.abs() <= delta)                    # (a float32 target that landed exactly on y: measure zero, re-drawn)
        if not bool(risky.any()):
            return idx, xyz, gt.reshape(-1, 1), delta
        where = torch.nonzero(risky).reshape(-1)
        xyz[where] = torch.rand(where.numel(), G, generator=gen) * 2 - 1
        y, pre = fwd()
        gt[where] = _targets(y[where], delta, gen, k0=rnd + 1).float()
    raise RuntimeError("could not build a region-populated margin-safe batch")


# ---- a case = (point, net kind, layout): inputs and the fp64 oracle's results ---------------------------------------------------------
class Case:
    """Inputs of `steps` optimiser steps at one operating point and what oracle.train_step computes from them in `dtype`.  Step s's batch
    is built from the fp64 state BEFORE step s.  forward_bf16: the oracle's own bf16-forward emulation is the specification, in fp32."""

    def __init__(self, point, kind="main", layout="segment", steps=2, seed=0, forward_bf16=False, batch_split=1):
        self.point, self.kind, self.layout, self.steps, self.batch_split = point, kind, layout, steps, batch_split
        self.id = f"{point.name}-{kind}-{layout}" + ("-bf16" if forward_bf16 else "") + (f"-split{batch_split}" if batch_split > 1 else "")
        self.L, self.kw = net_kw(kind, point.dropout_prob)
        self.net = orc.make_net(self.L, **self.kw)
        self.net_bf16 = orc.make_net(self.L, forward_bf16=True, **self.kw) if forward_bf16 else None
        self.scenes, self.lens = LAYOUTS[layout]
        self.N = sum(self.lens)
        self.n_norm = point.n_norm_factor * self.N
        base = 9000 + 7 * (seed + KIND_SEED[kind]) + {"main": 0, "w32": 1, "variant": 2}[kind]
        self.params = orc.init_params(self.net, base)
        gain = dict(point.out_gain).get(kind, 1.0)
        if gain != 1.0:
            last = self.net.n_lin - 1               # (a plain layer on all three nets: no weight norm on the output)
            assert not self.net.layers[last].weight_norm
            self.params[f"lin{last}.weight"] *= gain
            self.params[f"lin{last}.bias"] *= gain
        self.lat0 = latent_table(self.L, point.code_bound, base + 1)
        self.code_bound = None if point.code_bound is None else f32(point.code_bound)
        self.lr = (f32(point.lr[0]), f32(point.lr[1]))
        self.betas, self.eps = (f32(point.betas[0]), f32(point.betas[1])), f32(point.eps)
        self.reg_coef = f32(point.reg_coef)
        st = self.fresh_state()
        self.batches, self.deltas, self.grad_clip = [], [], []
        self.results = []
        self.lat_ren = []                           # the table as step s's forward leaves it
        for s in range(steps):
            idx, xyz, gt, delta = region_batch(self.net_bf16 or self.net, st, self.scenes, self.lens, base + 100 + s, point.delta, self.code_bound)
            clip = None
            if point.clip_factor is not None:       # relative to this step's own unclipped gradient norm, rounded as the ABI carries it
                probe = self.fresh_state(st)
                r = self._step(probe, idx, xyz, gt, delta, None)
                gn = math.sqrt(sum(float((g.double() ** 2).sum()) for g in r["grads"].values()))
                clip = f32(point.clip_factor * gn)
            self.batches.append((idx, xyz, gt))
            self.deltas.append(delta)
            self.grad_clip.append(clip)
            ren = st.latents.clone()
            orc.renorm_rows_(ren, idx, self.code_bound)
            self.lat_ren.append(ren)
            r = self._step(st, idx, xyz, gt, delta, clip)
            self.results.append(dict(r, lat_ren=ren, params={k: v.clone() for k, v in st.params.items()}, m={k: v.clone() for k, v in st.m.items()},
                                     v={k: v.clone() for k, v in st.v.items()}, latents=st.latents.clone(), m_lat=st.m_lat.clone(),
                                     v_lat=st.v_lat.clone()))

    def fresh_state(self, like=None, dtype=torch.float64):
        if like is None:
            # (.clone(): .to() of a float32 tensor to float32 is the tensor itself, and a step writes its state in place)
            return orc.TrainState.create({k: v.clone().to(dtype) for k, v in self.params.items()}, self.lat0.clone().to(dtype))
        st = orc.TrainState.create({k: v.clone() for k, v in like.params.items()}, like.latents.clone())
        st.m, st.v = {k: v.clone() for k, v in like.m.items()}, {k: v.clone() for k, v in like.v.items()}
        st.m_lat, st.v_lat, st.step = like.m_lat.clone(), like.v_lat.clone(), like.step
        return st

    def _step(self, st, idx, xyz, gt, delta, clip, net=None):
        """oracle.train_step with the regulariser's coefficient as the ABI carries it: lambda x ramp in ONE float (code_reg_lambda =
        reg_coef at epoch 100), everything else float32-rounded likewise."""
        dt = st.latents.dtype
        return orc.train_step(net or self.net_bf16 or self.net, st, idx, xyz.to(dt), gt.to(dt), delta=delta, code_bound=self.code_bound,
                              code_reg=self.point.code_reg, code_reg_lambda=self.reg_coef, epoch=100, lr_decoder=self.lr[0],
                              lr_latent=self.lr[1], batch_split=self.batch_split, grad_clip=clip, seed=DROP_SEED, betas=self.betas,
                              eps=self.eps, n_norm=self.n_norm)

    def reference(self):
        """What the HIP path is compared with: the fp64 results, or for a forward_bf16 case the oracle's bf16-forward step in fp32 (its
        rounding points are the specification: test_config5_bf16_forward_vs_oracle_and_fp32)."""
        if self.net_bf16 is None:
            return self.results
        if not hasattr(self, "_ref32"):
            self._ref32 = self.rerun(torch.float32, net=self.net_bf16)
        return self._ref32

    def rerun(self, dtype=torch.float64, net=None):
        """The same inputs through the oracle again (under a patched variant, in fp32, or on the bf16-forward net): a list of per-step
        dicts like self.results."""
        st, out = self.fresh_state(dtype=dtype), []
        for s in range(self.steps):
            idx, xyz, gt = self.batches[s]
            ren = st.latents.clone()
            orc.renorm_rows_(ren, idx, self.code_bound)
            r = self._step(st, idx, xyz, gt, self.deltas[s], self.grad_clip[s], net=net)
            out.append(dict(r, lat_ren=ren, params={k: v.clone() for k, v in st.params.items()}, m={k: v.clone() for k, v in st.m.items()},
                            v={k: v.clone() for k, v in st.v.items()}, latents=st.latents.clone(), m_lat=st.m_lat.clone(),
                            v_lat=st.v_lat.clone()))
        return out


@functools.lru_cache(maxsize=None)
def get_case(point, kind="main", layout="segment", forward_bf16=False, batch_split=1):
    """One Case per (point name, net kind, layout), built once and shared by every test that needs it; nobody writes to it."""
    return Case(BY_NAME[point], kind, layout, forward_bf16=forward_bf16, batch_split=batch_split)


ROUTE_CASES = (("main", "segment"), ("main", "ragged"), ("w32", "segment"), ("w32", "ragged"), ("variant", "ragged"))
# (point, kind, layout, forward_bf16, batch_split) of the cases that run once
BF16_CASE = ("cb0.6_delta0.03", "main", "segment", True, 1)
SPLIT_CASES = (("cb0.6_delta0.03", "main", "segment", False, 2), ("n_norm_3N", "main", "ragged", False, 2))


def all_gpu_cases():
    """Every case tests/test_gpu_operating_points.py runs, as get_case arguments."""
    return [(p.name, k, l, False, 1) for p in POINTS for k, l in ROUTE_CASES] + [BF16_CASE] + list(SPLIT_CASES)


# quantity -> (tensors of one step's result dict, the bound the GPU test asserts for it: tests/test_gpu_parity.py's constants)
FWD_TOL, GRAD_TOL, GRAD_ELEM_TOL, PARAM_TOL, LOSS_TOL = 1e-5, 1e-4, 1e-4, 1e-5, 1e-5
QUANTITIES = {
    "loss": (lambda r: [torch.tensor([float(r["loss"])], dtype=torch.float64)], LOSS_TOL),
    "sdf": (lambda r: [r["y"]], FWD_TOL),
    "gradients": (lambda r: [raw_grads(r)[k] for k in sorted(r["grads"])], GRAD_TOL),
    "dlat": (lambda r: [r["dlat"]], GRAD_TOL),
    "renormed table": (lambda r: [r["lat_ren"]], PARAM_TOL),
    "parameters": (lambda r: [r["params"][k] for k in sorted(r["params"])], PARAM_TOL),
    "exp_avg": (lambda r: [r["m"][k] for k in sorted(r["m"])] + [r["m_lat"]], GRAD_TOL),
    "exp_avg_sq": (lambda r: [r["v"][k] for k in sorted(r["v"])] + [r["v_lat"]], 2 * GRAD_TOL),
    "latent table": (lambda r: [r["latents"]], PARAM_TOL),
}


def raw_grads(r):
    """The gradients as the backward pass leaves them in the arena: the library clips inside Adam, never in place."""
    return r["grads"] if r.get("grads_unclipped") is None else r["grads_unclipped"]


def distance(a, b, q):
    """Worst tensor of quantity q, each relative to its own norm in b (all-zero tensors: absolute), over the steps of two runs."""
    pick = QUANTITIES[q][0]
    return max(rel_err(x, y) for ra, rb in zip(a, b) for x, y in zip(pick(ra), pick(rb)))


# ---- wrong variants, each a small pure function in the oracle's place -------------------------------------------------------------------
def _renorm(threshold, scale):
    def f(table, indices, max_norm):
        if max_norm is None or max_norm <= 0:
            return
        for j in torch.unique(indices).tolist():
            nu = table[j].norm(2)
            if threshold(nu, max_norm):
                table[j] *= scale(nu, max_norm)
    return f


def _l1(delta_of=lambda d: d, n_of=lambda y, n: n, sign=torch.sign, mask=True):
    def f(y, sdf_gt, delta, n_norm):
        delta, n = delta_of(delta), n_of(y, n_norm)
        diff = torch.clamp(y, -delta, delta) - torch.clamp(sdf_gt, -delta, delta)
        inside = ((y >= -delta) & (y <= delta)).to(y.dtype) if mask else torch.ones_like(y)
        return diff.abs().sum() / n, sign(diff) * inside / n
    return f


def _reg(c_of):
    def f(z, lam, epoch, n_norm):
        c = c_of(z, lam, epoch, n_norm)
        nrm = z.norm(dim=1, keepdim=True)
        return c * nrm.sum(), torch.where(nrm > 0, c * z / nrm, torch.zeros_like(z))
    return f


def _adam(b1=None, b2=None, eps=None):
    true = orc.adam_update_

    def f(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps_=1e-8):
        true(p, g, m, v, step, lr, beta1 if b1 is None else b1, beta2 if b2 is None else b2, eps_ if eps is None else eps)
    return f


B1_DEFAULT, B2_DEFAULT, EPS_DEFAULT = f32(0.9), f32(0.999), f32(1e-8)
# name: (attribute of the oracle it replaces, the replacement, the quantity it must move)
VARIANTS = {
    "renorm_threshold_one": ("renorm_rows_", _renorm(lambda nu, mx: nu > 1.0, lambda nu, mx: mx / (nu + 1e-7)), "renormed table"),
    "renorm_no_max_norm": ("renorm_rows_", _renorm(lambda nu, mx: nu > mx, lambda nu, mx: 1.0 / (nu + 1e-7)), "renormed table"),
    "renorm_compare_ss": ("renorm_rows_", _renorm(lambda nu, mx: nu * nu > mx, lambda nu, mx: mx / (nu + 1e-7)), "renormed table"),
    "delta_fixed": ("clamped_l1", _l1(delta_of=lambda d: f32(0.1)), "loss"),
    "inv_n_from_N": ("clamped_l1", _l1(n_of=lambda y, n: y.shape[0]), "gradients"),
    "sign_minus_one": ("clamped_l1", _l1(sign=lambda d: -torch.ones_like(d)), "gradients"),
    "inside_mask_dropped": ("clamped_l1", _l1(mask=False), "gradients"),
    "reg_dropped": ("code_regulariser", _reg(lambda z, lam, ep, n: 0.0), "dlat"),
    # (Case hands the oracle lambda x ramp as one coefficient at epoch 100; the variant without the ramp is handed lambda itself)
    "reg_no_ramp": ("code_regulariser", None, "dlat"),
    "reg_by_N": ("code_regulariser", _reg(lambda z, lam, ep, n: lam * min(1, ep / 100) / z.shape[0]), "dlat"),
    "default_betas": ("adam_update_", _adam(b1=B1_DEFAULT, b2=B2_DEFAULT), "exp_avg"),
    "default_eps": ("adam_update_", _adam(eps=EPS_DEFAULT), "parameters"),
}


@contextlib.contextmanager
def patched(name, case):
    attr, fn, _ = VARIANTS[name]
    if name == "reg_no_ramp":
        ramp = case.point.ramp
        fn = _reg(lambda z, lam, ep, n: (lam / ramp) / n)
    old = getattr(orc, attr)
    setattr(orc, attr, fn)
    try:
        yield
    finally:
        setattr(orc, attr, old)


def renorm_roundings(L):
    """fp32 roundings of one renormed entry, both renorm sites: row[c] * (max_norm / (sqrtf(ss) + 1e-7f)).
      ss: one wave sums the squares -- a lane squares (1) and adds its ceil(L / 64) columns (the first addition is to 0: exact, but
          counted), then six shuffle additions: 1 + ceil(L / 64) + 6 roundings, every term non-negative, so all relative to ss;
      sqrtf halves what came before and rounds once:  ceil(kss / 2) + 1;
      + 1e-7f: the constant's own rounding (relative to 1e-7 <= the sum) and the addition: 2;   the division: 1;   the product: 1.
    k = ceil((7 + ceil(L / 64)) / 2) + 5.  The bound on an entry is gamma(k) |entry| (optim_numpy.gamma); a row the spec leaves alone
    must be left bit for bit."""
    kss = 1 + -(-L // 64) + 6
    return -(-kss // 2) + 5


def np64(t):
    return t.detach().cpu().numpy().astype(np.float64)
