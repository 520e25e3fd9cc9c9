"""-m gpu: memory safety of every workspace layout (dsdf_api.hip make_plan / mc_plan / msdf_plan and the two ad-hoc ones), by plain
byte compares on torch tensors (tests/ws_guard.py) -- no oracle, so the sweep can visit every planner threshold.

Every case is run twice from identical inputs, once on a workspace filled with 0x00 and once with 0xFF (every fp32 word a NaN,
every int32 -1), with a 256-byte red zone behind every region, the workspace exactly as large as the ABI answers plus one red
zone of tail, and every caller-sized output a view into a sentinel-filled tensor.  Three properties per case:

  A  no byte outside the regions of the plan the call recorded changed (red zones, rounding padding, tail)        [both runs]
  B  every output is bit-identical between the two runs and free of NaN: nothing a result depends on is read from workspace
     bytes that nobody wrote.  Every path here is documented as deterministic (fixed-order reductions, no atomics),
     so every comparison is torch.equal.  Sequences that carry state in the workspace (module forward -> backward / jvp, the K
     phases of a phased backward, marching cubes count -> emit) are filled once, before their first call
  C  the bytes in front of and behind every caller-sized output are unchanged                                      [both runs]

The shapes sit at the planners' own break points, computed from the constants in the kernel sources (ws_guard.constants) and
the device's CU count, never copied: see thresholds().  CASES is a plain list (importable without a GPU: tests/test_abi_cpu.py
checks the region-table invariants of every plan in it on the host)."""
import ctypes as C
import math
from collections import Counter

import pytest
import torch

from deepsdf_amd import _lib
from deepsdf_amd.net import NetSpec, dropout_layer_key
from tests import ws_guard as G
from tests.test_gpu_parity import (BIG, BIG_BATCH_NETS, PHASE_NETS, _random_case, _random_variant_case, _random_w32_case)

pytestmark = pytest.mark.gpu
MAX_WS = 16 << 30          # no case's workspace may exceed this (computed from the ABI's answer before allocating)
K_ = G.constants()


def thresholds():
    """N at which a planner or a launch changes shape, each with the constants it comes from."""
    cus = G.chip_cus()
    t = {
        "BK": K_["BK"],                                          # split-K chunk granularity of the dW GEMMs
        "FROWS": K_["FROWS"],                                    # rows per fused workgroup
        "BM": K_["BM"],                                          # rows per column-sum block (Plan.mt)
        "256": 256,                                              # points per split-K slab (ns = ceil(N / 256))
        "LAT_SLICES": 128 * 2 * K_["LAT_SLICES_MAX"],            # one ragged segment cut into LAT_SLICES_MAX slices of >= 128 rows
        "pick_frows": 32 * cus,                                  # 32-row workgroups up to here, 64 above
        "NSPLIT": 256 * K_["NSPLIT_MAX"],                        # ns reaches NSPLIT_MAX
        "last_blocks": 16 * K_["LAST_BLOCKS_MAX"],               # last_layer_kernel's grid reaches LAST_BLOCKS_MAX
        "nwg_cus": K_["FROWS"] * cus,                            # one 64-row workgroup per CU (the K = 2 reserve, nslice)
    }
    return t


def n_values():
    t = thresholds()
    ns = {1, 3000}
    for v in t.values():
        ns |= {v - 1, v, v + 1}
    part = K_["LAST_BLOCKS_MAX"] * K_["FROWS"]                   # the head partials' old size: part_rows (make_plan)
    ns |= {part - 64, part, part + 64}
    return sorted(n for n in ns if n > 0)


BIG_N = [K_["LAST_BLOCKS_MAX"] * 96, 160000, 262144]             # 98304 (1.5 x the old cap), the shipped 10 x 16000, 2^18: width <= 128 only

# ---- nets, one per kernel family ------------------------------------------------------------------------------------------------
_SMALL = BIG_BATCH_NETS
NETS = {
    "w32_4x32": (_SMALL["4x32"][0], _SMALL["4x32"][1], {}),
    "w32x2_4x64": (_SMALL["4x64_tanh"][0], _SMALL["4x64_tanh"][1], {}),
    "n128_6x128": (_SMALL["6x128"][0], _SMALL["6x128"][1], {}),
    "fused_8x512": (256, BIG, {}),
    "fused_8x512_L2": (PHASE_NETS["8x512_shipped_L2"]["L"], BIG, {}),
    "split_8x512": (256, dict(BIG, gemm_split=True), {}),
    "bf16_8x512": (256, dict(BIG, forward_bf16=True), {}),
    "bf16_split_8x512": (256, dict(BIG, forward_bf16=True, gemm_split=True), {}),
    "layered_6x128": (_SMALL["6x128"][0], _SMALL["6x128"][1], {"DSDF_NO_FUSED": "1"}),
    "layered_8x512": (256, BIG, {"DSDF_NO_FUSED": "1"}),
    "n128_as_64row": (_SMALL["6x128"][0], _SMALL["6x128"][1], {"DSDF_NO_NARROW": "1", "DSDF_FROWS": "64"}),
    "w32_off": (_SMALL["4x32"][0], _SMALL["4x32"][1], {"DSDF_NO_W32": "1"}),
    "wide_3x640": (8, dict(dims=[640] * 3, dropout=[0, 2], dropout_prob=0.2, norm_layers=[0, 1, 2, 3], latent_in=[2], weight_norm=True,
                           geom_dimension=3), {}),
    "layernorm": (5, dict(dims=[64, 72, 136], dropout=[1], dropout_prob=0.2, norm_layers=[0, 1, 2, 3], latent_in=[2], weight_norm=False,
                          geom_dimension=3), {}),
    "xyz_in_all": (5, dict(dims=[64, 72, 64], dropout=[0], dropout_prob=0.2, norm_layers=[0, 1], latent_in=[2], weight_norm=True,
                           xyz_in_all=True, geom_dimension=3), {}),
    "latent_dropout": (8, dict(dims=[64, 64, 64], dropout=[0, 1], dropout_prob=0.5, norm_layers=[], latent_in=[], weight_norm=False,
                               latent_dropout=True, geom_dimension=3), {}),
    "L1_g2": (1, dict(dims=[48, 40, 48], dropout=[], dropout_prob=0.0, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=True,
                      geom_dimension=2), {}),
    "L16_g4": (16, dict(dims=[96, 96, 96], dropout=[1], dropout_prob=0.2, norm_layers=[0, 1, 2], latent_in=[1], weight_norm=True,
                        geom_dimension=4), {}),
    # the hoist kernel's k-unit switch ((L + 63) >> 6 in run_hoist) and HOIST_MAXL
    "L64": (64, dict(dims=[128, 128, 128], dropout=[], dropout_prob=0.0, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=True, geom_dimension=3), {}),
    "L65": (65, dict(dims=[128, 128, 128], dropout=[], dropout_prob=0.0, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=True, geom_dimension=3), {}),
    "L129": (129, dict(dims=[256, 256, 256], dropout=[], dropout_prob=0.0, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=True, geom_dimension=3), {}),
    "L257": (257, dict(dims=[512, 512, 512], dropout=[], dropout_prob=0.0, norm_layers=[0, 1, 2], latent_in=[2], weight_norm=True, geom_dimension=3), {}),
    "L509": (K_["HOIST_MAXL"] - 3, dict(dims=[512, 64], dropout=[], dropout_prob=0.0, norm_layers=[], latent_in=[], weight_norm=False, geom_dimension=3), {}),
    "L512": (K_["HOIST_MAXL"], dict(dims=[520, 64], dropout=[], dropout_prob=0.0, norm_layers=[], latent_in=[], weight_norm=False, geom_dimension=3), {}),
    "L0": (0, dict(dims=[32, 32, 32], dropout=[], dropout_prob=0.0, norm_layers=[], latent_in=[], weight_norm=False, geom_dimension=3), {}),
}
for _s in (3, 11, 20):
    NETS[f"random{_s}"] = (_random_case(_s)["L"], _random_case(_s)["net"], {})
for _s in (2, 19):
    NETS[f"random_w32_{_s}"] = (_random_w32_case(_s)["L"], _random_w32_case(_s)["net"], {})
for _s in (1, 6):
    NETS[f"random_variant{_s}"] = (_random_variant_case(_s)["L"], _random_variant_case(_s)["net"], {})

TRAIN = ["fb", "fb_acc", "fb_frozen", "fb_sdf", "step"]
PHASED = ["phase2", "phase4", "phase8"]
MODULE = ["mod_bwd", "mod_bwd_noinput", "mod_jvp"]
INFER = ["decode", "decode_latent"]
ALL_ENTRIES = TRAIN + PHASED + MODULE + INFER
R_VALUES = [1, 2, 3, 64, 512, 2000]


# section 3 of build_cases(): (R, seg_len) pairs in segment mode, and explicit lengths sent down the general path (seg_len 0)
SEG_RS = ((3, 32), (3, 64), (3, 96), (2, 40), (3, 100), (64, 64), (512, 32), (2000, 3), (2000, 32), (1, 16 * K_["FROWS"] * 2 * K_["LAT_SLICES_MAX"]))
SEG_GENERAL = ([1, 63, 64, 65, 300, 507],      # ragged by construction
               [96] * 3)                       # equal, but sent down the general path


def spec_of(net):
    L, kw, _ = NETS[net]
    return NetSpec(L, **kw)


def _fused(net):          # what fused_eligible() sees (host restatement, used only to pick which entries to LIST for a net)
    s, env = spec_of(net), NETS[net][2]
    return (env.get("DSDF_NO_FUSED") != "1" and not (s.xyz_in_all or s.latent_dropout or any(s.ln))
            and max(s.in_dim) <= K_["FMAXW"] and max(s.out_dim[:-1]) <= K_["FMAXW"])


def _decode_latent_ok(net):
    s = spec_of(net)
    return _fused(net) and 1 <= s.latent_size <= K_["HOIST_MAXL"] and s.geom_dimension <= K_["FGEO"] and s.n_layers >= 3 and not s.skip[-1]


def segments(N, R):
    """Segment lengths of N points in R segments: equal when R divides N (seg_len = N / R, segment mode when the kernels take it),
    ragged otherwise (seg_len 0: the general path)."""
    R = max(1, min(R, N))
    lens = [N // R + (1 if i < N % R else 0) for i in range(R)]
    return lens, (N // R if N % R == 0 else 0)


class Case:
    def __init__(self, family, net, entry, N, R=1, lens=None, seg_len=None, invalid=None):
        self.family, self.net, self.entry, self.N = family, net, entry, int(N)
        if lens is None:
            lens, sl = segments(N, R)
            seg_len = sl if seg_len is None else seg_len
        self.lens, self.seg_len = lens, int(seg_len)
        self.R = len(lens)
        self.invalid = invalid          # None, or the error text this case is EXPECTED to be refused with (listed beforehand)
        assert sum(lens) == self.N

    @property
    def id(self):
        return f"{self.net}-{self.entry}-N{self.N}-R{self.R}-s{self.seg_len}"

    @property
    def K(self):
        return int(self.entry[5:]) if self.entry.startswith("phase") else 0

    def ws_query(self, lib, cnet):
        """The ABI's size answer for this case's entry point (with whatever red zone is set)."""
        b = C.c_size_t()
        if self.entry == "decode":
            _lib.check(lib.dsdf_decode_workspace_bytes(C.byref(cnet), self.N, C.byref(b)))
        elif self.entry == "decode_latent":      # (Engine.decode_latent's rule, include/dsdf.h)
            _lib.check(lib.dsdf_decode_workspace_bytes(C.byref(cnet), max(self.N, 64), C.byref(b)))
            b.value = max(b.value, 16384)
        elif self.K > 2:
            _lib.check(lib.dsdf_workspace_bytes_buckets(C.byref(cnet), self.N, self.R, self.K, C.byref(b)))
        else:
            _lib.check(lib.dsdf_workspace_bytes(C.byref(cnet), self.N, self.R if self.entry in TRAIN + PHASED else 0, C.byref(b)))
        return b.value

    def plans(self):
        """Every (kind, N, R, segmode, buckets, frows) a launch of this case can choose: what the CPU test lays out."""
        if self.entry == "decode":
            return [(_lib.WS_PLAN_DECODE, self.N, 0, 0, 2, fr) for fr in (32, 64)]
        if self.entry == "decode_latent":
            return [(_lib.WS_PLAN_DECODE_LATENT, self.N, 0, 0, 2, fr) for fr in (32, 64)]
        if self.entry in MODULE:
            return [(_lib.WS_PLAN_TRAIN, self.N, 0, 0, 2, 64)]
        return [(_lib.WS_PLAN_TRAIN, self.N, self.R, seg, self.K, fr) for seg in (0, 1) for fr in (32, 64)]


def _entries_for(net):
    e = list(TRAIN) + list(MODULE) + ["decode"]
    if _fused(net):
        e += PHASED
    if _decode_latent_ok(net):
        e += ["decode_latent"]
    return e


def _r_for(N, k):
    special = {160000: 10, 262144: 2000, K_["LAST_BLOCKS_MAX"] * K_["FROWS"]: 512, 32 * G.chip_cus(): 64}
    if N in special:
        return special[N]
    return 1 if N < 64 else R_VALUES[k % len(R_VALUES)]


def build_cases():
    cases, dropped = [], []
    ns = n_values()
    # 1. the full product N x entry point on the two cheap nets
    for net in ("w32_4x32", "n128_6x128"):
        for k, N in enumerate(ns + BIG_N):
            for entry in _entries_for(net):
                cases.append(Case("product_" + net, net, entry, N, _r_for(N, k)))
    # 2. every other family: N next to the thresholds that move ITS plan, on a representative entry set
    t = thresholds()
    near = sorted({t["FROWS"] - 1, t["FROWS"] + 1, t["BM"] + 1, t["pick_frows"], t["pick_frows"] + 1, t["last_blocks"] + 1})
    part = K_["LAST_BLOCKS_MAX"] * K_["FROWS"]
    for net in NETS:
        if net in ("w32_4x32", "n128_6x128", "L0"):
            continue
        spec = spec_of(net)
        narrow = max(spec.in_dim + spec.out_dim) <= 128
        entries = [e for e in ("fb_sdf", "step", "phase4", "mod_bwd", "mod_jvp", "decode", "decode_latent") if e in _entries_for(net)]
        for k, N in enumerate(near + ([part + 64] if narrow or net == "fused_8x512" else [])):
            for entry in entries:
                cases.append(Case("family_" + net, net, entry, N, _r_for(N, k + 2)))
        if narrow:
            for N in BIG_N:
                cases.append(Case("family_" + net, net, "fb", N, _r_for(N, 0)))
    cases.append(Case("family_fused_8x512", "fused_8x512", "fb", 160000, 10))          # the shipped batch on the shipped net, once
    cases.append(Case("family_fused_8x512", "fused_8x512", "step", 160000, 10))
    # 3. segment shapes: seg_len at multiples and non-multiples of 32 and 64, many short segments (R > N / 32), ragged
    for net in ("w32_4x32", "w32x2_4x64", "n128_6x128", "fused_8x512", "bf16_8x512", "split_8x512", "L257"):
        for R, sl in SEG_RS:
            for entry in ("fb", "step", "phase2"):
                cases.append(Case("segments_" + net, net, entry, R * sl, R))
        for lens in SEG_GENERAL:
            cases.append(Case("segments_" + net, net, "fb", sum(lens), lens=list(lens), seg_len=0))
    # 4. latent_size 0: the general inference path takes it; every training entry refuses it BEFORE it plans anything
    for N in (1, 65, 3000):
        cases.append(Case("L0", "L0", "decode", N))
        cases.append(Case("L0", "L0", "mod_bwd", N))
        cases.append(Case("L0", "L0", "mod_jvp", N))
    cases.append(Case("L0", "L0", "fb", 256, 4, invalid="training needs latent_size > 0"))
    cases.append(Case("L0", "L0", "step", 256, 4, invalid="training needs latent_size > 0"))
    # the entries a net's kernels do not offer: refused with an error, listed here so that a silent fall-back would show
    cases.append(Case("refused", "layernorm", "phase2", 256, 4, invalid="dw_phase needs the fused kernels"))
    cases.append(Case("refused", "wide_3x640", "decode_latent", 256, invalid="dsdf_decode_latent needs the fused forward"))
    from deepsdf_amd.build import build_library
    build_library()                      # (the size answers below come from the library: build it if this is the first module to ask)
    lib = _lib.lib()
    keep = []
    for c in cases:
        if c.ws_query(lib, spec_of(c.net).c_struct()) > MAX_WS:
            dropped.append(c.id)
        else:
            keep.append(c)
    seen, uniq = set(), []
    for c in keep:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq, dropped


CASES, DROPPED_OVER_16GIB = build_cases()          # DROPPED_OVER_16GIB: shapes cut for the 16 GiB rule (none at the MI355X's CU count)
FAMILIES = sorted({c.family for c in CASES})
MC_GRIDS = [((2, 2, 2), "sphere"), ((3, 5, 7), "sphere"), ((33, 33, 33), "sphere"), ((64, 65, 66), "sphere"), ((33, 33, 33), "inside"),
            ((33, 33, 33), "outside"), ((2, 2, 2), "inside"), ((K_["MC_BLOCK"], 2, 2), "sphere")]
_QB = K_["MSDF_TARGET_WG"] * K_["MSDF_BLOCK"]
MSDF_CASES = [   # (faces, queries): both sides of every branch of msdf_plan's split rule
    (12, 1), (K_["MSDF_MIN_SPLIT_FACES"] * 2 - 1, 10), (K_["MSDF_MIN_SPLIT_FACES"] * 2, 10), (K_["MSDF_MIN_SPLIT_FACES"] * 5 + 7, 255),
    (K_["MSDF_MIN_SPLIT_FACES"] * K_["MSDF_MAX_SPLITS"] + 1000, 100), (K_["MSDF_MIN_SPLIT_FACES"] * 2, _QB - K_["MSDF_BLOCK"]),
    (K_["MSDF_MIN_SPLIT_FACES"] * 2, _QB - K_["MSDF_BLOCK"] + 1), (K_["MSDF_MIN_SPLIT_FACES"] * 2, _QB + 1), (12, 300000), (300, 5000)]
GEMM_TN = [(M, N, K) for (M, N) in ((128, 128), (253, 259), (1, 48)) for K in
           (K_["BK"] - 1, 255, 256, 257, 256 * K_["NSPLIT_MAX"] - 1, 256 * K_["NSPLIT_MAX"], 256 * K_["NSPLIT_MAX"] + 1)]
GRAD_NORM_N = [1, 4095, 4096, 4097, 4096 * 1023 + 1, 4096 * 1024, 4096 * 1024 + 1, 1843195]


# ---- running one case -----------------------------------------------------------------------------------------------------------
_SNAP = {}


def _params_snapshot(net):
    """One seeded parameter arena per net (device tensor), shared by every run on it."""
    if net not in _SNAP:
        from deepsdf_amd.engine import Engine
        e = Engine(spec_of(net), "cuda")
        e.init_like_reference(generator=torch.Generator().manual_seed(4000 + len(net)))
        _SNAP[net] = e.params.clone()
    return _SNAP[net]


def _keys(seed=9, step=3):
    return (C.c_uint32 * _lib.MAX_LAYERS)(*[dropout_layer_key(seed, step, l) for l in range(_lib.MAX_LAYERS)])


def run_net_case(c, fill):
    """One run of case c on a workspace filled with `fill`: returns ({output name: tensor}, Fences, ws).  Asserts A for the run."""
    from deepsdf_amd.engine import Engine
    spec = spec_of(c.net)
    F = G.Fences()
    params = F.new("params", spec.n_params)
    grads = F.new("grads", spec.n_params, zero=True)
    eng = Engine(spec, "cuda", params=params, grads=grads)
    eng.exp_avg, eng.exp_avg_sq = F.new("exp_avg", spec.n_params, zero=True), F.new("exp_avg_sq", spec.n_params, zero=True)
    eng.packed = F.new("packed", eng.packed.numel(), zero=True)          # (dsdf_materialize_weights: the caller zeroes it once)
    params.copy_(_params_snapshot(c.net))
    eng.materialize()
    lib, cnet, N, W0, Gd, L = eng.lib, eng.cnet, c.N, spec.in_dim[0], spec.geom_dimension, spec.latent_size
    gen = torch.Generator().manual_seed(17 + N)
    xyz = (torch.rand(N, Gd, generator=gen) * 2 - 1).cuda()
    ws = G.poisoned(c.ws_query(lib, cnet), fill)
    eng._ws, eng._ws_sizes = ws, {}
    out = {}
    if c.entry in TRAIN + PHASED:
        R = c.R
        lat = F.new("latent_table", (R, max(L, 1)))
        lat.copy_((torch.randn(R, max(L, 1), generator=gen) / math.sqrt(max(L, 1))).cuda())
        dlat = F.new("dlat", (R, max(L, 1)), zero=True)
        scenes = torch.randperm(R, generator=gen).to(torch.int64).cuda()
        off = torch.zeros(R + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.tensor(c.lens, dtype=torch.int64), 0)
        off = off.cuda()
        gt = (xyz.norm(dim=1) - 0.5).contiguous()
        kw = dict(n_norm=N, clamp_dist=0.1, reg_coef=1e-4, code_bound=1.0, training=True, seed=5, seg_len=c.seg_len)
        loss = F.new("loss", 1, zero=True)
        if c.entry == "step":
            m, v = F.new("lat_m", (R, max(L, 1)), zero=True), F.new("lat_v", (R, max(L, 1)), zero=True)
            eng.train_step(lat, dlat, m, v, scenes, off, xyz, gt, lr_decoder=5e-4, lr_latent=1e-3, loss_out=loss, **kw)
            out.update(lat_m=m, lat_v=v, params=eng.params, exp_avg=eng.exp_avg, exp_avg_sq=eng.exp_avg_sq, packed=eng.packed)
        elif c.entry in PHASED:
            y = F.new("sdf_out", N)
            for p in range(1, c.K + 1):          # the phases share the workspace: filled once, before phase 1
                eng.train_forward_backward(lat, dlat, scenes, off, xyz, gt, sdf_out=y if p == 1 else None, loss_out=loss, dw_phase=p,
                                           dw_buckets=c.K, **kw)
            out.update(sdf=y)
        else:
            acc = c.entry == "fb_acc"
            if acc:                              # gradients of an earlier chunk: accumulated onto, not overwritten
                grads.fill_(0.5); dlat.fill_(0.25); loss.fill_(2.0)
            y = F.new("sdf_out", N) if c.entry in ("fb_sdf", "fb_acc") else None
            eng.train_forward_backward(lat, dlat, scenes, off, xyz, gt, sdf_out=y, loss_out=loss, accumulate=acc,
                                       frozen_decoder=c.entry == "fb_frozen", **kw)
            if y is not None:
                out.update(sdf=y)
        out.update(loss=loss, grads=eng.grads, dlat=dlat, latent_table=lat)
    elif c.entry in MODULE:
        x = torch.cat([(torch.randn(N, L, generator=gen) / math.sqrt(max(L, 1))).cuda(), xyz], 1).contiguous()
        keys, y = _keys(), F.new("sdf_out", N)
        _lib.check(lib.dsdf_module_forward(C.byref(cnet), G.ptr(eng.packed), G.ptr(params), G.ptr(x), W0, N, 1, keys, G.ptr(y), G.ptr(ws),
                                           ws.numel(), G.stream()))
        out.update(sdf=y)
        if c.entry == "mod_jvp":                 # (forward -> jvp and forward -> backward: the forward's state stays in the workspace)
            t, j = torch.randn(N, W0, generator=gen).cuda(), F.new("jvp", N)
            _lib.check(lib.dsdf_module_jvp(C.byref(cnet), G.ptr(eng.packed), G.ptr(params), G.ptr(t), W0, N, 1, keys, G.ptr(j), G.ptr(ws),
                                           ws.numel(), G.stream()))
            out.update(jvp=j)
        else:
            d = torch.randn(N, generator=gen).cuda()
            d_in = F.new("d_input", (N, W0)) if c.entry == "mod_bwd" else None
            _lib.check(lib.dsdf_module_backward(C.byref(cnet), G.ptr(eng.packed), G.ptr(params), G.ptr(d), N, 1, keys, G.ptr(grads), 0,
                                                G.ptr(d_in), W0, G.ptr(ws), ws.numel(), G.stream()))
            out.update(grads=grads)
            if d_in is not None:
                out.update(d_input=d_in)
    elif c.entry == "decode":
        x = torch.cat([(torch.randn(N, L, generator=gen) / math.sqrt(max(L, 1))).cuda(), xyz], 1).contiguous()
        y = F.new("sdf_out", N)
        _lib.check(lib.dsdf_decode(C.byref(cnet), G.ptr(eng.packed), G.ptr(params), G.ptr(x), W0, N, G.ptr(y), G.ptr(ws), ws.numel(),
                                   G.stream()))
        out.update(sdf=y)
    elif c.entry == "decode_latent":
        z = (torch.randn(max(L, 1), generator=gen) / math.sqrt(max(L, 1))).cuda()
        y = F.new("sdf_out", N)
        _lib.check(lib.dsdf_decode_latent(C.byref(cnet), G.ptr(eng.packed), G.ptr(params), G.ptr(z), G.ptr(xyz), N, G.ptr(y), G.ptr(ws),
                                          ws.numel(), G.stream()))
        out.update(sdf=y)
    else:
        raise AssertionError(c.entry)
    assert eng._ws is ws, f"{c.id}: the Engine replaced the guarded workspace (the ABI's size answer was too small for its own call)"
    G.assert_clean(ws, fill, f"{c.id} [A]")
    F.check(f"{c.id} [C]")
    return out, F, ws


def same_and_finite(a, b, case):
    """Property B on two runs' outputs."""
    assert a.keys() == b.keys()
    for k in a:
        assert not bool(torch.isnan(a[k]).any()) and not bool(torch.isnan(b[k]).any()), f"{case} [B]: NaN in '{k}'"
        if not torch.equal(a[k], b[k]):
            diff = (a[k] != b[k]).reshape(-1).nonzero().reshape(-1)
            raise AssertionError(f"{case} [B]: '{k}' depends on what the workspace held: {diff.numel()} of {a[k].numel()} elements differ "
                                 f"between the 0x00 and the 0xFF run, first at flat index {int(diff[0])}, last at {int(diff[-1])}")


def check_case(c, monkeypatch):
    for k, v in NETS[c.net][2].items():
        monkeypatch.setenv(k, v)
    try:
        with G.redzone():
            if c.invalid is not None:
                with pytest.raises(_lib.DsdfError, match=c.invalid):
                    run_net_case(c, 0x00)
                return
            o0, f0, w0 = run_net_case(c, 0x00)
            o0 = {k: v.clone() for k, v in o0.items()}
            del f0, w0
            o1, f1, w1 = run_net_case(c, 0xFF)
            same_and_finite(o0, o1, c.id)
            del o0, o1, f1, w1
    finally:
        for k in NETS[c.net][2]:
            monkeypatch.delenv(k, raising=False)


def test_case_list_is_what_the_issue_asks_for():
    """Not a measurement: the list's own conditions.  At most 5 % expected-invalid, nothing above 16 GiB, the thresholds present."""
    n_inv = sum(c.invalid is not None for c in CASES)
    per = Counter(c.family for c in CASES)
    print(f"\nworkspace sweep: {len(CASES)} net cases in {len(per)} families, {n_inv} expected-invalid ({100.0 * n_inv / len(CASES):.1f} %), "
          f"{len(DROPPED_OVER_16GIB)} dropped for the 16 GiB rule {DROPPED_OVER_16GIB}")
    assert n_inv <= 0.05 * len(CASES)
    ns = {c.N for c in CASES if c.family.startswith("product_")}
    for name, v in thresholds().items():
        assert {v - 1, v, v + 1} <= ns | {0}, name
    assert {160000, 262144, K_["LAST_BLOCKS_MAX"] * 96} <= ns
    assert {c.entry for c in CASES} == set(ALL_ENTRIES)
    assert {c.R for c in CASES} >= set(R_VALUES)
    assert any(c.R > c.N / 32 and c.R >= 2000 for c in CASES)
    assert not DROPPED_OVER_16GIB


@pytest.mark.parametrize("family", FAMILIES)
def test_workspace_regions_results_and_outputs(family, monkeypatch):
    """Properties A, B and C (module docstring) for every case of one family."""
    mine = [c for c in CASES if c.family == family]
    try:
        for c in mine:
            check_case(c, monkeypatch)
    finally:
        _SNAP.clear()
        torch.cuda.empty_cache()
    print(f"\n{family}: {len(mine)} cases run ({sum(c.invalid is not None for c in mine)} expected-invalid), each with a 0x00 and a 0xFF workspace")


# ---- net-free entry points ------------------------------------------------------------------------------------------------------
def _two_fills(run, case):
    with G.redzone():
        outs = []
        for fill in (0x00, 0xFF):
            out, F, ws = run(fill)
            G.assert_clean(ws, fill, f"{case} [A]")
            F.check(f"{case} [C]")
            outs.append({k: v.clone() for k, v in out.items()})
            del out, F, ws
        same_and_finite(outs[0], outs[1], case)


def _mc_grid(shape, kind):
    nx, ny, nz = shape
    if kind != "sphere":
        return torch.full(shape, -1.0 if kind == "inside" else 1.0, device="cuda")
    ax = [torch.linspace(-1, 1, n) for n in shape]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    noise = 0.05 * torch.rand(shape, generator=torch.Generator().manual_seed(nx * 7 + ny * 3 + nz))
    return ((X * X + Y * Y + Z * Z).sqrt() - 0.6 + noise).to(torch.float32).cuda().contiguous()


def test_marching_cubes_count_then_emit():
    lib = _lib.lib()
    try:
        for shape, kind in MC_GRIDS:
            g = _mc_grid(shape, kind)
            sp, org = (C.c_float * 3)(0.1, 0.2, 0.3), (C.c_float * 3)(-1.0, -1.0, -1.0)

            def run(fill):
                b = C.c_size_t()
                _lib.check(lib.dsdf_mc_workspace_bytes(*shape, C.byref(b)))
                ws, F = G.poisoned(b.value, fill), G.Fences()
                totals = F.new("totals", 2, torch.int64)
                _lib.check(lib.dsdf_mc_count(G.ptr(g), *shape, 0.0, G.ptr(totals), G.ptr(ws), ws.numel(), G.stream()))
                nv, nf = totals.tolist()                              # (count -> emit share the workspace: filled once)
                verts, faces = F.new("verts", (nv, 3)), F.new("faces", (nf, 3), torch.int32)
                _lib.check(lib.dsdf_mc_emit(G.ptr(g), *shape, 0.0, sp, org, nv, nf, G.ptr(verts), G.ptr(faces), G.ptr(ws), ws.numel(), G.stream()))
                if kind == "sphere" and min(shape) > 2:
                    assert nv > 0 and nf > 0
                if kind != "sphere":
                    assert nv == 0 and nf == 0
                return dict(totals=totals, verts=verts, faces=faces), F, ws
            _two_fills(run, f"marching cubes {shape} {kind}")
    finally:
        torch.cuda.empty_cache()
    print(f"\nmarching cubes: {len(MC_GRIDS)} grids run")


def test_mesh_sdf_prepare_and_query():
    lib = _lib.lib()
    try:
        for nf, nq in MSDF_CASES:
            gen = torch.Generator().manual_seed(nf + nq)
            V = (torch.rand(nf + 2, 3, generator=gen) * 2 - 1).cuda()
            Fi = torch.stack([torch.arange(nf), torch.arange(nf) + 1, torch.arange(nf) + 2], 1).to(torch.int32).cuda().contiguous()
            Q = (torch.rand(nq, 3, generator=gen) * 2.4 - 1.2).cuda()

            def run(fill):
                tb, wb, ns = C.c_size_t(), C.c_size_t(), C.c_int32()
                _lib.check(lib.dsdf_msdf_plan(nf, nq, C.byref(tb), C.byref(wb), C.byref(ns)))
                F = G.Fences()
                tri = F.new("tri", tb.value, torch.uint8, zero=True)
                _lib.check(lib.dsdf_msdf_prepare(G.ptr(V), V.shape[0], G.ptr(Fi), nf, G.ptr(tri), tri.numel(), G.stream()))
                ws = G.poisoned(wb.value, fill)
                o = dict(sdf=F.new("sdf", nq), d2=F.new("d2", nq), face=F.new("face", nq, torch.int32), closest=F.new("closest", (nq, 3)),
                         winding=F.new("winding", nq))
                _lib.check(lib.dsdf_msdf_query(G.ptr(tri), nf, G.ptr(Q), nq, G.ptr(o["sdf"]), G.ptr(o["d2"]), G.ptr(o["face"]), G.ptr(o["closest"]),
                                               G.ptr(o["winding"]), 0, G.ptr(ws), ws.numel(), G.stream()))
                return dict(o, tri=tri), F, ws
            _two_fills(run, f"mesh sdf {nf} faces x {nq} queries")
    finally:
        torch.cuda.empty_cache()
    print(f"\nmesh sdf: {len(MSDF_CASES)} (faces, queries) pairs run")


def _tn_ws_bytes(M, N, K, g):       # include/dsdf.h, dsdf_gemm_tn
    ns = max(1, min(K_["NSPLIT_MAX"], (K + 255) // 256))
    kchunk = ((K + ns - 1) // ns + K_["BK"] - 1) // K_["BK"] * K_["BK"]
    nsplit = (K + kchunk - 1) // kchunk
    return nsplit * ((M * N + 63) // 64 * 64) * 4 + g + M * 4 + g


def test_gemm_tn_and_grad_norm_workspaces():
    lib = _lib.lib()
    try:
        for M, N, K in GEMM_TN:
            gen = torch.Generator().manual_seed(M + N + K)
            lda, ldb = (M + 3) // 4 * 4, (N + 3) // 4 * 4
            A, B = torch.zeros(K, lda), torch.zeros(K, ldb)
            A[:, :M], B[:, :N] = torch.randn(K, M, generator=gen), torch.randn(K, N, generator=gen)
            A, B = A.cuda(), B.cuda()

            def run(fill):
                F = G.Fences()
                Cd = F.new("C", (M, N))
                ws = G.poisoned(_tn_ws_bytes(M, N, K, G.REDZONE), fill, tail=G.REDZONE)
                _lib.check(lib.dsdf_gemm_tn(G.ptr(A), lda, G.ptr(B), ldb, G.ptr(Cd), N, M, N, K, G.ptr(ws), ws.numel(), G.stream()))
                return dict(C=Cd), F, ws
            _two_fills(run, f"gemm_tn M{M} N{N} K{K}")
        for n in GRAD_NORM_N:
            g = torch.randn(n, generator=torch.Generator().manual_seed(n)).cuda()

            def run(fill):
                F = G.Fences()
                o = F.new("norm_coef", 2)
                ws = G.poisoned(min(1024, (n + 4095) // 4096) * 4 + G.REDZONE, fill)
                _lib.check(lib.dsdf_grad_norm(G.ptr(g), n, 1.0, G.ptr(o), C.c_void_p(o.data_ptr() + 4), G.ptr(ws), ws.numel(), G.stream()))
                return dict(norm_coef=o), F, ws
            _two_fills(run, f"grad_norm n{n}")
    finally:
        torch.cuda.empty_cache()
    print(f"\ngemm_tn: {len(GEMM_TN)} shapes, grad_norm: {len(GRAD_NORM_N)} sizes run")


def test_caller_sized_outputs_of_calls_without_a_workspace():
    """Property C for dsdf_ms_rows (grid range and point list), dsdf_ms_caps (in-place range) and dsdf_materialize_weights."""
    from deepsdf_amd import mesh
    from deepsdf_amd.engine import Engine
    from tests.test_gpu_microstructure import make_field
    lib = _lib.lib()
    n_run = 0
    try:
        for degrees, L, N, tiling in (([1, 1, 1], 3, 5, 1), ([2, 3, 1], 16, 9, (2, 1, 3)), ([3, 3, 3], 65, 12, 2)):
            field = make_field(degrees, L, 5)[0]
            g, _ = mesh._ms_grid(tiling, N)
            npts = int(g.dims[0]) * int(g.dims[1]) * int(g.dims[2])
            s, _keep = field.c_spline(torch.device("cuda"))
            for start, end in ((0, npts), (1, 2), (K_["MS_TILE"] - 1, 2 * K_["MS_TILE"] + 1), (npts - 1, npts)):
                F = G.Fences()
                rows = F.new("rows", (end - start, L + 3))
                _lib.check(lib.dsdf_ms_rows(C.byref(s), C.byref(g), start, end, None, 1, 1, G.ptr(rows), G.stream()))
                F.check(f"ms_rows grid {degrees} L{L} [{start}, {end})")
                assert not bool(torch.isnan(rows).any())
                sdf = F.new("sdf", end - start)
                sdf.copy_(torch.linspace(-1, 1, end - start).cuda())
                recs, n = mesh.cap_records(mesh.default_cap_border_dict())
                _lib.check(lib.dsdf_ms_caps(C.byref(g), start, end, recs, n, G.ptr(sdf), G.stream()))
                F.check(f"ms_caps N{N} [{start}, {end})")
                n_run += 2
            for nq, with_xyz in ((1, 1), (K_["MS_TILE"] + 1, 0), (1000, 1)):
                pts = (torch.rand(nq, 3, generator=torch.Generator().manual_seed(nq)) * 2.2 - 1.1).cuda()
                F = G.Fences()
                rows = F.new("rows", (nq, L + (3 if with_xyz else 0)))
                _lib.check(lib.dsdf_ms_rows(C.byref(s), C.byref(g), 0, nq, G.ptr(pts), 1, with_xyz, G.ptr(rows), G.stream()))
                F.check(f"ms_rows points {degrees} L{L} n{nq}")
                n_run += 1
        for net in ("w32_4x32", "fused_8x512", "split_8x512", "bf16_8x512", "layernorm", "wide_3x640", "L1_g2"):
            spec = spec_of(net)
            F = G.Fences()
            params = F.new("params", spec.n_params)
            eng = Engine(spec, "cuda", params=params, grads=F.new("grads", spec.n_params, zero=True))
            eng.packed = F.new("packed", eng.packed.numel(), zero=True)
            params.copy_(_params_snapshot(net))
            eng.materialize()
            F.check(f"materialize_weights {net}")
            assert not bool(torch.isnan(eng.packed).any())
            n_run += 1
    finally:
        _SNAP.clear()
        torch.cuda.empty_cache()
    print(f"\ncalls without a workspace: {n_run} run")


# ---- the checker checks itself (torch only, the test's own tensor) --------------------------------------------------------------
def test_checker_reports_the_right_region_and_nothing_inside_one():
    g, fill = G.REDZONE, 0x5C
    # a layout as the planners make it: 'a' ends on a 256 boundary, 'b' does not (100 bytes of rounding padding), 'c' is last
    rows = [("a", 0, 512), ("b", 512 + g, 924), ("c", 512 + g + 1024 + g, 4096)]
    total = rows[-1][1] + 4096 + g
    ws = G.poisoned(total, fill)
    assert not G.table_problems(rows, total, g) and G.damage(ws, fill, rows) == []
    assert [p for p, _, _ in G.gaps(rows, ws.numel())] == ["a", "b", "c"]

    def flipped(at):
        w = ws.clone()
        w[at] = fill ^ 0xFF
        return G.damage(w, fill, rows)
    assert flipped(512 + 7) == [("a", 519, 519)]                                  # (a) a red zone
    pad = rows[1][1] + rows[1][2] + 5                                             # (b) rounding padding of 'b' (924 is no multiple of 256)
    assert rows[1][2] % 256 and flipped(pad) == [("b", pad, pad)]
    assert flipped(ws.numel() - 1) == [("c", ws.numel() - 1, ws.numel() - 1)]     # (c) the tail
    assert flipped(total + 3) == [("c", total + 3, total + 3)]
    for name, off, nb in rows:                                                    # inside a region: nothing to report
        assert flipped(off) == [] and flipped(off + nb - 1) == [] and flipped(off + nb // 2) == []
    w = ws.clone()                                                                # first and last changed byte of one damaged gap
    w[512 + 3] = 0; w[512 + 200] = 0
    assert G.damage(w, fill, rows) == [("a", 515, 712)]
    big = [("a", 0, 512)]                                                         # a gap too large for the gather: compared as slices
    wbig = G.poisoned(512 + G.SMALL_GAP + 1000, fill, tail=0)
    wbig[512 + G.SMALL_GAP + 500] = 1
    assert G.damage(wbig, fill, big) == [("a", 512 + G.SMALL_GAP + 500, 512 + G.SMALL_GAP + 500)]
    with pytest.raises(AssertionError, match="behind 'b'"):                       # the assertion names the region and the case
        wb = ws.clone(); wb[pad] = 0
        hits = G.damage(wb, fill, rows)
        assert not hits, "case x: " + "; ".join(f"behind '{p}': first {a}, last {b}" for p, a, b in hits)
    F = G.Fences()                                                                # the output fences, both sides
    v = F.new("out", 10)
    assert F.problems() == []
    v.fill_(1.0)
    assert F.problems() == []
    F.items[0][1][G.FENCE + 40] = 0
    F.items[0][1][G.FENCE - 1] = 0
    assert len(F.problems()) == 2 and "behind" in F.problems()[1] and "in front of" in F.problems()[0]
    del ws, w, wbig, F, v
    torch.cuda.empty_cache()
