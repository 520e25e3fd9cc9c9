"""-m gpu: the VALUES every entry point computes at the planners' break points, against the float64 oracle.

tests/test_gpu_workspace.py visits these shapes and checks that no launch writes or reads outside its regions; it never looks at a
number.  A mistake that stays inside its own region -- a slab count rounded down, a grid one workgroup short, a slice of a long
segment counted twice, a partial row read with the other workgroup size's stride -- is deterministic, free of NaN and memory-safe.
This module runs the same shapes (imported from that sweep: thresholds(), n_values(), BIG_N, NETS, R_VALUES, segments(), SEG_RS,
SEG_GENERAL and the sweep's own (N, R) pairs per family), the same entry points and the same kernel families, and compares every
output with oracle/deepsdf_oracle.py in float64 on a margin-safe batch (tests/safe_batch.py).

The oracle's CPU time is the cost, so the unit of work is a GROUP = (oracle net, segment lengths): one margin search and one fp64
optimiser step (plus an fp64 forward / backward / jvp where an inference or module entry asks for one), compared with EVERY launch on
that shape: segment mode and the forced general path, the env-selected kernel families of the same net (DSDF_NO_FUSED,
DSDF_NO_NARROW + DSDF_FROWS=64, DSDF_NO_W32), gemm_split, and the chunked / frozen / phased / one-call entries.

Tolerances are tests/test_gpu_parity.py's: FWD_TOL / Y_ROW_TOL (sdf), 1e-5 (loss), GRAD_TOL / GRAD_ELEM_TOL (gradients, dlat, exp_avg),
PARAM_TOL norm-wise (parameters, latent table), GRAD_TOL and twice that for Adam's two moments, 2e-5 for the jvp
(test_decoder_jvp_vs_oracle); `packed` after the one-call step is bit-equal to a fresh materialize of the new parameters.  The
bf16-forward nets are compared with the oracle's own forward_bf16 step in fp32 at test_config5_bf16_forward_vs_oracle_and_fp32's
figures (1e-4 forward and loss, 1e-2 gradients and dlat; the bounds it does not state are named in _tols).  At the small batches
of this sweep that reference is not sharp: the same oracle code with float64 accumulation (same rounding points) lands up to
1.9e-4 (sdf), 1e-2 (gradients) and 2e-3 (post-Adam state: Adam's first step is lr * sign(g) wherever |g| >> eps) away from it.
Where that spread is above a quarter of a bound, the bound is restated as four times the spread: the pinned table BF16_RESTATED,
case by case, each figure from the oracle alone; any other pair keeps the stated bound.  The
entry-wise post-Adam bound PARAM_STEP_FRAC is not asserted here: the fp32 oracle alone uses half of it at one of these shapes.

GROUPS is a plain list, importable without a GPU: tests/test_abi_cpu.py checks its conditions on the host."""
import math
import time

import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests import test_gpu_workspace as W
from tests.golden_io import rel_err, worst_elem
from tests.safe_batch import safe_batch
from tests.test_gpu_parity import FWD_TOL, GRAD_ELEM_TOL, GRAD_TOL, PARAM_TOL, Y_ROW_TOL, _packed_floats_without_split_planes
from tests.test_gpu_workspace import BIG_N, K_, NETS, R_VALUES, SEG_GENERAL, SEG_RS, n_values, segments, spec_of, thresholds

pytestmark = pytest.mark.gpu

PRODUCT_NETS = ("w32_4x32", "n128_6x128")
# nets that run on another net's oracle result: the same parameters and batch, another kernel family
ORACLE_OF = {"split_8x512": "fused_8x512", "layered_8x512": "fused_8x512", "bf16_split_8x512": "bf16_8x512",
             "layered_6x128": "n128_6x128", "n128_as_64row": "n128_6x128", "w32_off": "w32_4x32"}
EXCLUDED = {"L0": "latent_size 0: every training entry refuses it (the sweep lists it as expected-invalid); nothing to compare"}
# the families the sweep lists beyond the issue's tier 2 (a second latent size of 8x512, the seeded random specs, which
# tests/test_gpu_parity.py already runs against the oracle at their own shapes): the three smallest N of the sweep's list only
EXTRA_NETS = ("fused_8x512_L2", "random3", "random11", "random20", "random_w32_2", "random_w32_19", "random_variant1", "random_variant6")
SEGMENT_NETS = ("w32_4x32", "w32x2_4x64", "n128_6x128", "L257", "fused_8x512")
PART = K_["LAST_BLOCKS_MAX"] * K_["FROWS"]                       # the head partials' old size (make_plan's part_rows)
PLUS1 = sorted({v + 1 for v in thresholds().values()})           # N exactly one above a threshold
SPLIT_AT = {**{n: n - 1 for n in PLUS1}, PART + 64: PART}       # fb_acc: two accumulated chunks cut AT the break point
DELTA, CODE_BOUND, EPOCH, LAM, DROP_SEED, LR_DEC, LR_LAT = 0.1, 1.0, 130, 1e-4, 77, 5e-4, 1e-3
REG = LAM * min(1, EPOCH / 100)


# forward_bf16 nets: the (group, quantity) pairs held to a bound other than the stated one, with the spread of the oracle's two
# accumulation widths recorded for each (measured on the CPU from oracle/ alone; every pair listed is at least 1.25 x a quarter of
# its stated bound, every pair not listed is below that and keeps the stated bound).  The asserted bound is 4 x the figure here.
BF16_RESTATED = {
    ("bf16_8x512-N63-R1-s63", "sdf"): 1.874e-04,                  # stated 1e-04
    ("bf16_8x512-N63-R1-s63", "gradients"): 8.295e-03,            # stated 1e-02
    ("bf16_8x512-N63-R1-s63", "exp_avg"): 8.295e-03,              # stated 1e-02
    ("bf16_8x512-N63-R1-s63", "exp_avg_sq"): 1.183e-02,           # stated 2e-02
    ("bf16_8x512-N63-R1-s63", "state after the step"): 2.236e-03, # stated 1e-05
    ("bf16_8x512-N63-R1-s63", "decode sdf"): 1.295e-04,           # stated 1e-04
    ("bf16_8x512-N63-R1-s63", "decode_latent sdf"): 1.295e-04,    # stated 1e-04
    ("bf16_8x512-N65-R64-s0", "sdf"): 1.124e-04,                  # stated 1e-04
    ("bf16_8x512-N65-R64-s0", "state after the step"): 1.967e-05, # stated 1e-05
    ("bf16_8x512-N65-R64-s0", "decode sdf"): 1.305e-04,           # stated 1e-04
    ("bf16_8x512-N65-R64-s0", "decode_latent sdf"): 1.548e-04,    # stated 1e-04
    ("bf16_8x512-N65-R64-s0", "module sdf"): 1.124e-04,           # stated 1e-04
    ("bf16_8x512-N129-R129-s1", "sdf"): 1.403e-04,                # stated 1e-04
    ("bf16_8x512-N129-R129-s1", "dlat"): 1.025e-02,               # stated 1e-02
    ("bf16_8x512-N129-R129-s1", "gradients"): 9.002e-03,          # stated 1e-02
    ("bf16_8x512-N129-R129-s1", "exp_avg"): 9.002e-03,            # stated 1e-02
    ("bf16_8x512-N129-R129-s1", "exp_avg_sq"): 7.661e-03,         # stated 2e-02
    ("bf16_8x512-N129-R129-s1", "latent exp_avg"): 1.025e-02,     # stated 1e-02
    ("bf16_8x512-N129-R129-s1", "latent exp_avg_sq"): 1.193e-02,  # stated 2e-02
    ("bf16_8x512-N129-R129-s1", "state after the step"): 8.966e-04,# stated 1e-05
    ("bf16_8x512-N129-R129-s1", "decode sdf"): 1.558e-04,         # stated 1e-04
    ("bf16_8x512-N129-R129-s1", "decode_latent sdf"): 1.198e-04,  # stated 1e-04
    ("bf16_8x512-N129-R129-s1", "module sdf"): 1.373e-04,         # stated 1e-04
    ("bf16_8x512-N129-R129-s1", "module gradients"): 7.161e-03,   # stated 1e-02
    ("bf16_8x512-N129-R129-s1", "d_input"): 6.804e-03,            # stated 1e-02
    ("bf16_8x512-N129-R129-s1", "jvp"): 7.910e-03,                # stated 1e-02
    ("bf16_8x512-N8192-R64-s128", "sdf"): 1.310e-04,              # stated 1e-04
    ("bf16_8x512-N8192-R64-s128", "gradients"): 3.247e-03,        # stated 1e-02
    ("bf16_8x512-N8192-R64-s128", "exp_avg"): 3.247e-03,          # stated 1e-02
    ("bf16_8x512-N8192-R64-s128", "state after the step"): 1.637e-03,# stated 1e-05
    ("bf16_8x512-N8192-R64-s128", "decode sdf"): 1.080e-04,       # stated 1e-04
    ("bf16_8x512-N8192-R64-s128", "decode_latent sdf"): 7.912e-05,# stated 1e-04
    ("bf16_8x512-N8193-R1-s8193", "sdf"): 1.406e-04,              # stated 1e-04
    ("bf16_8x512-N8193-R1-s8193", "state after the step"): 3.434e-04,# stated 1e-05
    ("bf16_8x512-N8193-R1-s8193", "decode sdf"): 1.182e-04,       # stated 1e-04
    ("bf16_8x512-N8193-R1-s8193", "decode_latent sdf"): 1.182e-04,# stated 1e-04
    ("bf16_8x512-N16385-R2-s0", "sdf"): 1.345e-04,                # stated 1e-04
    ("bf16_8x512-N16385-R2-s0", "state after the step"): 1.587e-03,# stated 1e-05
    ("bf16_8x512-N16385-R2-s0", "decode sdf"): 1.055e-04,         # stated 1e-04
    ("bf16_8x512-N16385-R2-s0", "decode_latent sdf"): 1.261e-04,  # stated 1e-04
}


class Group:
    """One oracle run and every launch compared with it.  launches: [(net, entry)], entry one of ENTRIES."""

    def __init__(self, tier, onet, lens):
        self.tier, self.onet, self.lens, self.launches = tier, onet, tuple(lens), []
        self.N, self.R = sum(lens), len(lens)
        self.seg_len = lens[0] if len(set(lens)) == 1 else 0

    @property
    def id(self):
        return f"{self.onet}-N{self.N}-R{self.R}-s{self.seg_len}"


ENTRIES = ("fb", "fb_acc", "fb_frozen", "step", "phase2", "phase4", "decode", "decode_latent", "mod_bwd", "mod_jvp")


def build_groups():
    groups = {}

    def add(tier, net, lens, entries):
        onet = ORACLE_OF.get(net, net)
        g = groups.setdefault((onet, tuple(lens)), Group(tier, onet, lens))
        for e in entries:
            assert e in ENTRIES
            if (net, e) not in g.launches:
                g.launches.append((net, e))
        return g

    def entries_for(net, N, module):
        e = ["fb", "step", "decode"]
        if W._decode_latent_ok(net):
            e.append("decode_latent")
        if N in SPLIT_AT:
            e += ["fb_acc", "fb_frozen"] + (["phase2", "phase4"] if W._fused(net) else [])
        if module:
            e += ["mod_bwd", "mod_jvp"]
        return e

    # 1. the full product on the two cheap nets: every N of the sweep, R by the sweep's rule
    tier1_lens = {}
    for net in PRODUCT_NETS:
        for k, N in enumerate(n_values() + BIG_N):
            lens, _ = segments(N, W._r_for(N, k))
            tier1_lens[net, N] = lens
            add(1, net, lens, entries_for(net, N, module=N in PLUS1))
    # 2. every other family at the sweep's own (N, R) pairs for it (its `near` list, + the old partials' size + 64 where it has it)
    for net in NETS:
        if net in PRODUCT_NETS or net in EXCLUDED:
            continue
        pairs = sorted({(c.N, c.R) for c in W.CASES if c.family == "family_" + net and c.N not in BIG_N})
        if max(spec_of(net).in_dim + spec_of(net).out_dim) >= 512 and net != "L257":
            pairs = [(N, R) for N, R in pairs if N <= thresholds()["last_blocks"] + 1]      # above: the 3 x 512 L257 net stands in
        if net == "L257":
            pairs.append((PART + 64, W._r_for(PART + 64, 0)))
        if net in EXTRA_NETS:
            pairs = pairs[:3]
        for N, R in pairs:
            onet = ORACLE_OF.get(net, net)
            lens = tier1_lens[onet, N] if onet in PRODUCT_NETS else segments(N, R)[0]     # (no oracle run of their own)
            add(2, net, lens, entries_for(net, N, module=N in (K_["FROWS"] + 1, K_["BM"] + 1)))
    # 3. the sweep's segment shapes: (R, seg_len) in segment mode and on the general path, and the explicit length lists
    for net in SEGMENT_NETS:
        for lens in [[sl] * R for R, sl in SEG_RS] + [list(l) for l in SEG_GENERAL]:
            if net == "fused_8x512" and sum(lens) > thresholds()["last_blocks"]:
                continue
            add(3, net, lens, ["fb", "step"])
    return list(groups.values())


GROUPS = build_groups()
TESTS = sorted({(g.tier, g.onet) for g in GROUPS})


# ---- the oracle's side ----------------------------------------------------------------------------------------------------------
def _oracle_net(onet):
    L, kw, _ = NETS[onet]
    return orc.make_net(L, **{k: v for k, v in kw.items() if k != "gemm_split"})


class Ref:
    """One arithmetic of the oracle on a group's batch: float64, or fp32 (a forward_bf16 net's reference: its rounding points are the
    specification, as in _config5_oracle)."""

    def __init__(self, T, double):
        self.T, self.double = T, double
        self.p = T.p64 if double else T.params
        st = orc.TrainState.create({k: v.clone() for k, v in self.p.items()}, self.cast(T.lat0).clone())
        self.r = orc.train_step(T.net, st, T.idx, self.cast(T.xyz), self.cast(T.gt), delta=DELTA, code_bound=CODE_BOUND, epoch=EPOCH,
                                seed=DROP_SEED, lr_decoder=LR_DEC, lr_latent=LR_LAT)
        self.after, self._memo = st, {}

    def cast(self, x):
        return x.double() if self.double else x.float()

    def _once(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def decode(self):
        return self._once("decode", lambda: orc.decoder_forward(self.T.net, self.p, self.cast(self.T.x), training=False)[0].reshape(-1))

    def decode_latent(self):
        x = torch.cat([self.T.z.expand(self.T.g.N, -1), self.T.xyz], 1)
        return self._once("dl", lambda: orc.decoder_forward(self.T.net, self.p, self.cast(x), training=False)[0].reshape(-1))

    def _masks(self):
        net, N = self.T.net, self.T.g.N
        return orc.dropout_masks(net, DROP_SEED, 0, N), (orc.latent_dropout_mask(net, DROP_SEED, 0, N) if net.latent_dropout else None)

    def module_backward(self):
        """(sdf [N], parameter gradients, d_input) of the training-mode forward on the batch's own rows and masks, for dy = T.d."""
        def run():
            masks, lmask = self._masks()
            y, sv = orc.decoder_forward(self.T.net, self.p, self.cast(self.T.x), training=True, masks=masks, latent_mask=lmask)
            grads, dx0 = orc.decoder_backward(self.T.net, self.p, sv, self.cast(self.T.d).reshape(-1, 1), True)
            return y.reshape(-1), grads, dx0
        return self._once("mb", run)

    def module_jvp(self):
        def run():
            masks, lmask = self._masks()
            f = lambda inp: orc.decoder_forward(self.T.net, self.p, inp, training=True, masks=masks, latent_mask=lmask)[0]   # noqa: E731
            return torch.autograd.functional.jvp(f, self.cast(self.T.x), self.cast(self.T.tangent))[1].reshape(-1)
        return self._once("mj", run)


def _vals(d):
    return [d[k] for k in sorted(d)]


# quantity -> the oracle tensors it covers (of one Ref).  A bound is asserted per tensor; a restated bound (BF16_RESTATED) is per quantity.
QUANTITIES = {
    "loss": lambda r: [torch.tensor([r.r["loss"]], dtype=torch.float64)],
    "sdf": lambda r: [r.r["y"]],
    "dlat": lambda r: [r.r["dlat"]],
    "gradients": lambda r: _vals(r.r["grads"]),
    "exp_avg": lambda r: _vals(r.after.m),
    "exp_avg_sq": lambda r: _vals(r.after.v),
    "latent exp_avg": lambda r: [r.after.m_lat],
    "latent exp_avg_sq": lambda r: [r.after.v_lat],
    "state after the step": lambda r: _vals(r.after.params) + [r.after.latents],
    "decode sdf": lambda r: [r.decode()],
    "decode_latent sdf": lambda r: [r.decode_latent()],
    "module sdf": lambda r: [r.module_backward()[0]],
    "module gradients": lambda r: _vals(r.module_backward()[1]),
    "d_input": lambda r: [r.module_backward()[2]],
    "jvp": lambda r: [r.module_jvp()],
}


class Truth:
    """The inputs of one group and the oracle's results on them.  `ref` is what the HIP path is compared with: float64, or for a
    forward_bf16 net the oracle's own bf16-forward arithmetic in fp32.  For such a net `alt` is the SAME oracle code with float64
    accumulation (same rounding points): the distance between the two is how far the reference is from itself (which bf16 roundings
    tip), and decides whether a stated bound means anything at that case -- see Launcher.cmp."""

    def __init__(self, g):
        self.g, self.net = g, _oracle_net(g.onet)
        net, L, R, N = self.net, self.net.latent_size, g.R, g.N
        self.bf16 = net.forward_bf16
        self.params = orc.init_params(net, 4000 + len(g.onet))
        gen = torch.Generator().manual_seed(5000 + N + R)
        T = R + 3                                                  # a latent table larger than R, read through a permuted scenes vector
        self.scenes = torch.randperm(T, generator=gen)[:R].to(torch.int64)
        self.lat0 = torch.randn(T, L, generator=gen) / math.sqrt(L)
        hot = int(self.scenes[R // 2])
        self.lat0[hot] *= 1.7 / self.lat0[hot].norm()              # one row in use above code_bound: the renorm fires
        self.p64 = {k: v.double() for k, v in self.params.items()}
        st64 = orc.TrainState.create({k: v.clone() for k, v in self.p64.items()}, self.lat0.double())
        self.idx, self.xyz, self.gt = safe_batch(net, st64, None, None, 6000 + N, DELTA, CODE_BOUND, DROP_SEED, G=net.geom_dimension,
                                                 scenes=self.scenes, lens=list(g.lens))
        self.lat_ren = self.lat0.double().clone()                  # the table as every training entry leaves it: looked-up rows renormed
        orc.renorm_rows_(self.lat_ren, self.idx, CODE_BOUND)
        self.x = torch.cat([self.lat_ren[self.idx].float(), self.xyz], 1).contiguous()       # the decoder's input rows, [N, L + G]
        self.z = self.lat_ren[int(self.scenes[0])].float()                                   # decode_latent's one code
        self.d = torch.randn(N, generator=torch.Generator().manual_seed(7000 + N))           # module backward's d(sdf)
        self.tangent = torch.randn(N, self.x.shape[1], generator=torch.Generator().manual_seed(8000 + N))
        self.ref = Ref(self, double=not self.bf16)
        self.alt = Ref(self, double=True) if self.bf16 else None
        self._spread = {}

    def spread(self, q):
        """forward_bf16 nets: how far the oracle's fp32 run and its float64-accumulated run are apart on quantity q: the worst tensor of
        QUANTITIES[q], each relative to its own norm.  Nothing of the HIP path enters it."""
        if q not in self._spread:
            self._spread[q] = max(rel_err(a, b) for a, b in zip(QUANTITIES[q](self.ref), QUANTITIES[q](self.alt)))
        return self._spread[q]

    def prepare(self, entries):
        for r in (self.ref, self.alt):
            for e, fn in (("decode", "decode"), ("decode_latent", "decode_latent"), ("mod_bwd", "module_backward"), ("mod_jvp", "module_jvp")):
                if r is not None and e in entries:
                    getattr(r, fn)()


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------------
class Book:
    def __init__(self):
        self.worst, self.fails, self.n, self.launches, self.groups, self.oracle_s, self.spreads = {}, [], 0, 0, 0, 0.0, {}

    def check(self, qty, val, tol, where):
        self.n += 1
        if not val <= tol:                                          # (a NaN fails)
            self.fails.append(f"{where}: {qty} {val:.3e} > {tol:.1e}")
        w = self.worst.get(qty)
        if w is None or not val <= w[0]:
            self.worst[qty] = (val, where)

    def same(self, qty, ok, where):
        self.n += 1
        if not ok:
            self.fails.append(f"{where}: {qty}")

    def merge(self, o):
        for q, (v, where) in o.worst.items():
            if q not in self.worst or not v <= self.worst[q][0]:
                self.worst[q] = (v, where)
        for k in ("n", "launches", "groups", "oracle_s"):
            setattr(self, k, getattr(self, k) + getattr(o, k))
        self.spreads.update(o.spreads)

    def report(self, title):
        lines = [f"{title}: {self.groups} oracle runs ({self.oracle_s:.1f} s), {self.launches} launches, {self.n} comparisons"]
        lines += [f"    worst {q:<46s} {v:.2e}   at {where}" for q, (v, where) in sorted(self.worst.items())]
        for (gid, q), (st, d) in sorted(self.spreads.items()):
            pin = BF16_RESTATED.get((gid, q))
            lines.append(f"    oracle spread {gid:<28s} {q:<22s} {d:.2e}  stated bound {st:.0e}  asserted <= "
                         + (f"{4 * pin:.2e} (restated: 4 x the recorded {pin:.2e})" if pin is not None else f"{st:.0e}"))
        return "\n".join(lines)


TOTAL = Book()


def _tols(bf16):
    if bf16:        # test_config5_bf16_forward_vs_oracle_and_fp32 states 1e-4 (forward, loss) and 1e-2 (gradients, dlat).  By analogy, NOT
        # stated there: the jvp and exp_avg (linear in the gradient) 1e-2, exp_avg_sq (quadratic) 2e-2, the post-Adam state PARAM_TOL
        # as for fp32.  No element-wise bound exists for this mode: None = the figure is reported, nothing is asserted or counted
        return dict(y=1e-4, y_el=None, loss=1e-4, g=1e-2, g_el=None, p=PARAM_TOL, m=1e-2, v=2e-2, jvp=1e-2)
    return dict(y=FWD_TOL, y_el=Y_ROW_TOL, loss=1e-5, g=GRAD_TOL, g_el=GRAD_ELEM_TOL, p=PARAM_TOL, m=GRAD_TOL, v=2 * GRAD_TOL, jvp=2e-5)


# ---- the HIP side ---------------------------------------------------------------------------------------------------------------
class Launcher:
    """Drives one entry point for one (net, group) the way run_net_case and HipTrainer do, and books every comparison."""

    def __init__(self, t, net, book):
        from deepsdf_amd.engine import Engine
        self.t, self.g, self.net, self.book, self.tol = t, t.g, net, book, _tols(t.bf16)
        self.spec = spec_of(net)
        self.tag = "bf16 forward: " if t.bf16 else ""              # (reported apart: another reference, other bounds)
        self.Engine = Engine
        d = "cuda"
        self.sc = t.scenes.to(d)
        off = torch.zeros(self.g.R + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.tensor(self.g.lens, dtype=torch.int64), 0)
        self.off, self.xyz, self.gt = off.to(d), t.xyz.to(d).contiguous(), t.gt.reshape(-1).to(d).contiguous()
        self.kw = dict(n_norm=self.g.N, clamp_dist=DELTA, reg_coef=REG, code_bound=CODE_BOUND, training=True, seed=DROP_SEED)

    def fresh(self):
        eng = self.Engine(self.spec, "cuda")
        eng.load_params(self.t.params)
        lat = self.t.lat0.to("cuda", torch.float32).contiguous().clone()
        return eng, lat, torch.zeros_like(lat)

    def where(self, entry, mode=""):
        return f"{self.net} {entry}{mode} N{self.g.N} R{self.g.R} s{self.g.seg_len}"

    # -- comparisons
    def bound(self, q, tol):
        """The bound of quantity q at this group.  fp32 nets: the stated one.  forward_bf16 nets: the stated one too, except for the
        (group, quantity) pairs pinned in BF16_RESTATED, where the oracle's own two accumulation widths are further apart than a
        quarter of it and it says nothing about a kernel: there it is four times the RECORDED spread (a constant of this file, from
        the oracle alone), and the spread measured now must still be above that quarter.  Every spread is printed."""
        stated = self.tol[tol]
        if self.t.alt is None:
            return stated
        d, key = self.t.spread(q), (self.g.id, q)
        self.book.spreads[key] = (stated, d)
        if key not in BF16_RESTATED:
            return stated
        if not d > stated / 4:
            self.book.fails.append(f"{self.g.id}: {q}: the oracle's spread is {d:.2e} now, no more than a quarter of the stated {stated:.0e}: "
                                   f"the restated bound has lost its reason")
        return 4 * BF16_RESTATED[key]

    def cmp(self, qty, mine, pick, tol, w, name="", el=None, q=None):
        """`mine` against pick(ref), norm-wise (and its worst entry where `el` names a bound); q: the QUANTITIES key (default qty)."""
        bound = self.bound(q or qty, tol)
        ref, qty = pick(self.t.ref), self.tag + qty
        ref = ref if torch.is_tensor(ref) else torch.tensor([float(ref)], dtype=torch.float64)
        mine = mine if torch.is_tensor(mine) else torch.tensor([float(mine)])
        self.book.check(qty, rel_err(mine.cpu(), ref), bound, f"{w} {name}".rstrip())
        if el is not None:
            e = worst_elem(mine.cpu(), ref)
            if self.tol[el] is not None:
                self.book.check(qty + " worst entry", e, self.tol[el], f"{w} {name}".rstrip())
            elif not e <= self.book.worst.get(qty + " worst entry (reported only)", (-1.0, ""))[0]:
                self.book.worst[qty + " worst entry (reported only)"] = (e, f"{w} {name}".rstrip())

    def cmp_train(self, eng, y, lat, dlat, w, grads=True):
        self.cmp("loss", eng.loss, lambda r: r.r["loss"], "loss", w)
        self.cmp("sdf", y, lambda r: r.r["y"].reshape(-1), "y", w, el="y_el")
        self.cmp("dlat", dlat, lambda r: r.r["dlat"], "g", w, el="g_el")
        self.book.check(self.tag + "renormed latent rows", rel_err(lat.cpu(), self.t.lat_ren), PARAM_TOL, w)
        if grads:
            self.cmp_grads(eng, lambda r: r.r["grads"], w)

    def cmp_grads(self, eng, pick, w, q="gradients"):
        mine = eng.named_views(eng.grads)
        self.book.same("gradient tensor names", set(mine) == set(pick(self.t.ref)), w)
        for k in pick(self.t.ref):
            self.cmp("gradients", mine[k], lambda r, k=k: pick(r)[k], "g", w, name=k, el="g_el", q=q)

    # -- entries
    def fb(self, seg_len, mode, frozen=False, K=0):
        eng, lat, dlat = self.fresh()
        y = torch.full((self.g.N,), float("nan"), device="cuda")
        w = self.where("fb_frozen" if frozen else (f"phase{K}" if K else "fb"), mode)
        if frozen:
            eng.grads.fill_(0.5)
        for p in range(1, K + 1) if K else (0,):
            eng.train_forward_backward(lat, dlat, self.sc, self.off, self.xyz, self.gt, sdf_out=y if p <= 1 else None, seg_len=seg_len,
                                       frozen_decoder=frozen, dw_phase=p, dw_buckets=K if K else None, **self.kw)
        self.cmp_train(eng, y, lat, dlat, w, grads=not frozen)
        if frozen:
            self.book.same("the gradient arena changed under frozen_decoder", bool((eng.grads == 0.5).all()), w)

    def fb_acc(self):
        from deepsdf_amd.engine import make_segments
        eng, lat, dlat = self.fresh()
        cut, N = SPLIT_AT[self.g.N], self.g.N
        y = torch.full((N,), float("nan"), device="cuda")
        idx = self.t.idx.cuda()
        for ci, (a, b) in enumerate(((0, cut), (cut, N))):
            sc, so = make_segments(idx[a:b])
            eng.train_forward_backward(lat, dlat, sc, so, self.xyz[a:b].contiguous(), self.gt[a:b].contiguous(), sdf_out=y[a:b], row_offset=a,
                                       accumulate=ci > 0, seg_len=0, **self.kw)
        self.cmp_train(eng, y, lat, dlat, self.where("fb_acc", f"[{cut}+{N - cut}]"))

    def step(self, seg_len):
        eng, lat, dlat = self.fresh()
        m, v = torch.zeros_like(lat), torch.zeros_like(lat)
        w = self.where("step")
        eng.train_step(lat, dlat, m, v, self.sc, self.off, self.xyz, self.gt, n_norm=self.g.N, clamp_dist=DELTA, reg_coef=REG,
                       code_bound=CODE_BOUND, lr_decoder=LR_DEC, lr_latent=LR_LAT, seed=DROP_SEED, seg_len=seg_len)
        self.cmp("loss", eng.loss, lambda r: r.r["loss"], "loss", w)
        P, M, V = eng.named_views(), eng.named_views(eng.exp_avg), eng.named_views(eng.exp_avg_sq)
        for k in self.t.ref.after.params:
            self.cmp("parameters after the step", P[k], lambda r, k=k: r.after.params[k], "p", w, name=k, q="state after the step")
            self.cmp("exp_avg", M[k], lambda r, k=k: r.after.m[k], "m", w, name=k, el="g_el")
            self.cmp("exp_avg_sq", V[k], lambda r, k=k: r.after.v[k], "v", w, name=k)
        self.cmp("latent table after the step", lat, lambda r: r.after.latents, "p", w, q="state after the step")
        self.cmp("latent exp_avg", m, lambda r: r.after.m_lat, "m", w)
        self.cmp("latent exp_avg_sq", v, lambda r: r.after.v_lat, "v", w)
        self.book.same("weights_dirty after the one-call step", not eng.weights_dirty, w)
        ref = self.Engine(self.spec, "cuda")                        # `packed` against a fresh materialize of the NEW parameters
        ref.load_params({k: t.clone() for k, t in P.items()})
        ref.materialize()
        npk = _packed_floats_without_split_planes(eng)              # (gemm_split: the bf16 planes behind the floats are not floats)
        self.book.same("packed differs from a fresh materialize of the new parameters", torch.equal(eng.packed[:npk], ref.packed[:npk]), w)

    def decode(self):
        eng, _, _ = self.fresh()
        self.cmp("sdf", eng.decode(self.t.x.cuda()).reshape(-1), lambda r: r.decode(), "y", self.where("decode"), el="y_el", q="decode sdf")

    def decode_latent(self):
        eng, _, _ = self.fresh()
        self.cmp("sdf", eng.decode_latent(self.t.z.cuda(), self.xyz).reshape(-1), lambda r: r.decode_latent(), "y", self.where("decode_latent"),
                 el="y_el", q="decode_latent sdf")

    def mod_bwd(self):
        eng, _, _ = self.fresh()
        w, N = self.where("mod_bwd"), self.g.N
        y = eng.module_forward(self.t.x.cuda(), True, seed=DROP_SEED, step=0)
        d_in = eng.module_backward(self.t.d.cuda().contiguous(), N, True, True, False)
        self.cmp("sdf", y.reshape(-1), lambda r: r.module_backward()[0], "y", w, el="y_el", q="module sdf")
        self.cmp_grads(eng, lambda r: r.module_backward()[1], w, q="module gradients")
        self.cmp("d_input", d_in, lambda r: r.module_backward()[2], "g", w, el="g_el")

    def mod_jvp(self):
        eng, _, _ = self.fresh()
        eng.module_forward(self.t.x.cuda(), True, seed=DROP_SEED, step=0)
        j = eng.module_jvp(self.t.tangent.cuda(), self.g.N, True)
        self.cmp("jvp", j.reshape(-1), lambda r: r.module_jvp(), "jvp", self.where("mod_jvp"))

    def run(self, entry):
        sl = self.g.seg_len
        if entry == "fb":                       # segment mode where the lengths are equal, and always the forced general path
            if sl:
                self.fb(sl, "[seg]")
            self.fb(0, "[general]")
            return 2 if sl else 1
        if entry == "step":
            self.step(sl)
        elif entry == "fb_frozen":
            self.fb(sl, "", frozen=True)
        elif entry in ("phase2", "phase4"):
            self.fb(sl, "", K=int(entry[5:]))
        else:
            getattr(self, entry)()
        return 1


def run_group(g, book, monkeypatch):
    t0 = time.time()
    t = Truth(g)
    t.prepare({e for _, e in g.launches})
    book.oracle_s += time.time() - t0
    book.groups += 1
    for net in dict.fromkeys(n for n, _ in g.launches):
        env = NETS[net][2]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            L = Launcher(t, net, book)
            for n, entry in g.launches:
                if n == net:
                    book.launches += L.run(entry)
        finally:
            for k in env:
                monkeypatch.delenv(k, raising=False)
    del t
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _report_of_the_whole_sweep():
    """After the module's last test: the worst distance from the oracle per compared quantity over everything that ran."""
    yield
    print("\n" + TOTAL.report("break-point value sweep"))


@pytest.mark.parametrize("tier,onet", TESTS, ids=[f"tier{t}-{n}" for t, n in TESTS])
def test_values_at_the_break_points_vs_oracle(tier, onet, monkeypatch):
    """Every launch of every group of one (tier, oracle net) against the float64 oracle; all misses are collected and reported together,
    each naming the launch, the tensor, the figure and its bound."""
    book = Book()
    mine = [g for g in GROUPS if (g.tier, g.onet) == (tier, onet)]
    for g in mine:
        run_group(g, book, monkeypatch)
    print("\n" + book.report(f"tier {tier} {onet}"))
    TOTAL.merge(book)
    assert not book.fails, f"{len(book.fails)} of {book.n} comparisons miss their bound:\n" + "\n".join(book.fails[:40])
