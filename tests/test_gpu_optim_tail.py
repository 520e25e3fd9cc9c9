"""-m gpu: every form of Adam in the optimiser step's tail, each in isolation, ELEMENT BY ELEMENT against the float64 spec of
tests/optim_numpy.py at bounds counted from the fp32 roundings of the kernels' expressions (stated there; none is a measured figure).

What the end-to-end parity tests cannot see -- late steps, aged moments, gradients around eps, the second pass of the grid-stride
loops, beta1 / beta2 / both bias corrections (which almost cancel out of a first step from zero moments) -- is what the inputs
here are made of (optim_numpy.make_state; its properties are asserted on the CPU before the GPU sees them).  Because the reference
of every comparison is the spec applied to the very gradient the kernel consumed, the gradients' own conditioning (early Adam:
update ~ lr g / (|g| + eps)) is not part of any bound.

Forms and how a test knows it is on one:
  adam_kernel            dsdf_adam_latent_only (by entry point); the bn parameters of a LayerNorm net through dsdf_adam_step
  adam_sched_kernel      dsdf_adam_latent_sched (by entry point)
  the ride               dsdf_adam_step with n_latent_floats > 0 (by entry point: its only latent path)
  adam_rows_kernel       dsdf_adam_step's decoder arena
  clip                   dsdf_grad_norm (sumsq_partial_kernel + clip_coef_kernel)
  finalize_row_wave<K>   dsdf_train_step on nets whose widest layer input selects K = 1, 2, 4, 8 (by width), the fused path by a
                         sentinel in the gradient arena, which the fused finalize never writes
  finalize_row + Adam    NOT reachable: the block form serves rows wider than 512 inputs, the fused kernels take widths <= 512 only,
                         so dsdf_train_step falls back to dsdf_adam_step on such a net -- asserted by the sentinel being overwritten.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from deepsdf_amd import _lib
from deepsdf_amd.engine import Engine, make_segments
from deepsdf_amd.net import NetSpec
from tests import optim_numpy as O

pytestmark = pytest.mark.gpu

STEPS = (1, 2, 10, 1000, 100000)
CAP = 2048 * 256           # elements one pass of the flat kernels' grid covers (2048 blocks of 256 threads)
FLAT_N = (1, 255, 256, 257, CAP - 1, CAP, CAP + 1, 2 * CAP + 77)      # the last three: a second pass of the grid-stride loop, with a tail
LR_DEC, LR_LAT, L2 = O.f32(5e-4), O.f32(1e-3), O.f32(0.03)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hold(tag, got, ref, bound):
    """Every element of `got` within its own bound of `ref` (the worst element decides, not a norm); prints the worst ratio first."""
    got = got.detach().cpu().numpy().astype(np.float64).reshape(-1) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64).reshape(-1)
    ref, bound = np.asarray(ref, np.float64).reshape(-1), np.asarray(bound, np.float64).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (tag, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), f"{tag}: non-finite values"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    w = int(np.argmax(ratio))
    print(f"{tag}: worst err/bound {ratio[w]:.3f} at element {w} of {got.size} (err {err[w]:.3e}, bound {bound[w]:.3e}, ref {ref[w]:.6e})")
    assert ratio[w] <= 1.0, f"{tag}: element {w}: got {got[w]!r}, spec {ref[w]!r}, error {err[w]:.3e} > bound {bound[w]:.3e} ({ratio[w]:.2f} x)"


def hold_adam(tag, got_p, got_m, got_v, r, m0, scaled=False):
    hold(tag + " exp_avg", got_m, r["m"], O.m_bound(m0, r["g_eff"], scaled))
    hold(tag + " exp_avg_sq", got_v, r["v"], O.v_bound(r["v"], scaled))
    hold(tag + " param", got_p, r["p"], O.p_bound(r["p"], r["upd_scale"], scaled))


@pytest.fixture(scope="module")
def tiny_engine():
    """A decoder for dsdf_adam_step to carry the ride: its own gradient arena stays zero."""
    eng = Engine(NetSpec(4, [32, 32], 3, norm_layers=[0, 1], weight_norm=True), "cuda")
    eng.init_like_reference(generator=torch.Generator().manual_seed(1))
    return eng


# ---- flat forms ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", FLAT_N)
def test_flat_adam_forms_hold_the_spec_at_every_step(n, tiny_engine):
    """dsdf_adam_latent_only, dsdf_adam_latent_sched (one schedule row holding step t's scalars) and the ride, from the same aged and
    fresh states at steps 1 .. 100000.  (|g| >= 1e-12 keeps g^2 and (1 - b2) g^2 normal fp32 numbers: the bounds stay relative.)"""
    flat_adam_forms(n, tiny_engine)


def flat_adam_forms(n, tiny_engine, betas=(0.9, 0.999), eps=1e-8, steps=STEPS):
    """The three flat forms at Adam constants of the caller's choice (tests/test_gpu_operating_points.py: away from torch's defaults);
    the spec is evaluated at their float32 images, as the ABI carries them."""
    lib = _lib.lib()
    b1, b2, ep = O.f32(betas[0]), O.f32(betas[1]), O.f32(eps)
    assert 1.0 - b1 <= 0.5                                         # m_bound's condition
    blocks = min(2048, -(-n // 256))
    assert (n > blocks * 256) == (n > CAP)                       # sizes past the cap take a second pass; the last one has a tail
    for aged in (True, False):
        p0, g0, m0, v0 = O.make_state(n, 1000 + n % 997, aged=aged)
        O.check_state(p0, g0, m0, v0, aged=aged)
        g = _dev(g0)
        for t in steps:
            tag = f"n{n} {'aged' if aged else 'fresh'} t{t}"
            r = O.adam_ref(p0, g0, m0, v0, lr=LR_LAT, t=t, b1=b1, b2=b2, eps=ep)
            cfg = _lib.DsdfAdamCfg(t, 0.0, LR_LAT, betas[0], betas[1], eps, None)
            # adam_kernel
            p, m, v = _dev(p0), _dev(m0), _dev(v0)
            _lib.check(lib.dsdf_adam_latent_only(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, C.byref(cfg), _stream()))
            hold_adam(tag + " latent_only", p, m, v, r, m0)
            assert torch.equal(g.cpu(), torch.from_numpy(g0))      # the gradient is read, never written
            # the ride on the materialise launch
            p, m, v = _dev(p0), _dev(m0), _dev(v0)
            e = tiny_engine
            _lib.check(lib.dsdf_adam_step(C.byref(e.cnet), _ptr(e.params), _ptr(e.grads), _ptr(e.exp_avg), _ptr(e.exp_avg_sq), _ptr(p),
                                          _ptr(g), _ptr(m), _ptr(v), n, C.byref(cfg), _ptr(e.packed), _stream()))
            hold_adam(tag + " ride", p, m, v, r, m0)
            # adam_sched_kernel: the two scalars as the device schedule carries them (fp32), the regulariser folded in
            ss, bq = (O.f32(x) for x in O.step_scalars(LR_LAT, b1, b2, t))
            rs = O.adam_ref(p0, g0, m0, v0, lr=None, t=None, b1=b1, b2=b2, eps=ep, l2=L2, step_size=ss, bc2_sqrt=bq)
            p, m, v = _dev(p0), _dev(m0), _dev(v0)
            sched = torch.tensor([[ss, bq]], dtype=torch.float64).to(torch.float32).cuda()
            counter = torch.zeros(1, dtype=torch.int64, device="cuda")
            _lib.check(lib.dsdf_adam_latent_sched(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, _ptr(sched), 1, _ptr(counter), betas[0], betas[1], eps,
                                                  L2, _stream()))
            hold_adam(tag + " sched", p, m, v, rs, m0, scaled=True)
            assert int(counter.item()) == 1


def test_sched_form_walks_its_schedule_and_stays_on_the_last_row():
    """Seven schedule rows with a learning-rate drop after the fourth, l2 != 0, nine calls: the device counter reads k after k calls,
    call k uses row min(k, 7) - 1 (the eighth and ninth the last one).  Every call is compared with the spec applied to the state
    the previous call left on the device, so nothing accumulates.  (Captured-graph replay of this entry point is
    test_reconstruction_as_a_captured_graph_equals_the_eager_loop's subject: graphs are left alone here.)"""
    lib = _lib.lib()
    n, rows = 5000, 7
    p0, g0, m0, v0 = O.make_state(n, 77)
    O.check_state(p0, g0, m0, v0)
    sc = [[(LR_LAT * (0.1 if it >= 4 else 1.0)) / (1.0 - O.B1 ** (it + 1)), math.sqrt(1.0 - O.B2 ** (it + 1))] for it in range(rows)]
    sched = torch.tensor(sc, dtype=torch.float64).to(torch.float32)
    assert float(sched[4, 0]) < 0.2 * float(sched[3, 0])            # the drop is in the schedule
    sd = sched.cuda()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    p, m, v = _dev(p0), _dev(m0), _dev(v0)
    rng = np.random.default_rng(3)
    for k in range(1, 10):
        gk = g0 * rng.choice([-1.0, 1.0], n).astype(np.float32)          # a new gradient every call: fresh signs, the same decades
        O.check_state(p0, gk, m0, v0)
        pc, mc, vc = (x.cpu().numpy() for x in (p, m, v))
        row = min(k, rows) - 1
        r = O.adam_ref(pc, gk, mc, vc, lr=None, t=None, l2=L2, step_size=float(sched[row, 0]), bc2_sqrt=float(sched[row, 1]))
        g = _dev(gk)
        _lib.check(lib.dsdf_adam_latent_sched(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, _ptr(sd), rows, _ptr(counter), 0.9, 0.999, 1e-8, L2,
                                              _stream()))
        assert int(counter.item()) == k
        hold_adam(f"sched call {k} (row {row})", p, m, v, r, mc, scaled=True)
    assert torch.equal(sd.cpu(), sched)


# ---- decoder arena: adam_rows_kernel, adam_kernel on the bn parameters -------------------------------------------------------------

ARENA_NETS = {
    # input widths 7, 65, 507, 515 (above 512) and 64; 1152 rows = a multiple of 4; the output layer is plain
    "wn_7_65_507_515_64": dict(L=4, dims=[65, 507, 515, 64], norm_layers=[0, 1, 2, 3], weight_norm=True),
    # the same input widths with a skip layer: 65 + 500 + 515 + 64 + 1 = 1145 rows, not a multiple of 4; a plain hidden layer
    "wn_rows_1145": dict(L=4, dims=[65, 507, 515, 64], norm_layers=[0, 1, 3, 4], weight_norm=True, latent_in=[2]),
    "plain_7_65_72_64": dict(L=4, dims=[65, 72, 64], weight_norm=False),
    # LayerNorm variant: bn{l}.weight / bn{l}.bias go through adam_kernel with grad_scale
    "layernorm_40_64": dict(L=4, dims=[40, 64], norm_layers=[0, 1, 2], weight_norm=False),
}


def arena_spec(name, **flags):
    kw = dict(ARENA_NETS[name])
    return NetSpec(kw.pop("L"), kw.pop("dims"), 3, **kw, **flags)


def scale_rows(spec):
    """[(layer, row0, g ParamInfo or None, v ParamInfo)] of the scale vector."""
    out, r0 = [], 0
    for l in range(spec.n_layers):
        byk = {p.kind: p for p in spec.params if p.layer == l}
        out.append((l, r0, byk.get("g"), byk.get("v", byk.get("weight"))))
        r0 += spec.out_dim[l]
    return out


def hold_scale_vector(tag, spec, scale, params):
    """The scale vector against g' / ||v'_row|| in float64 of the parameters it was computed from: the lane-strided sum of squares
    (ceil(in / 64) additions), six shuffle additions, one square root, one division (optim_numpy.row_scale_k); plain rows exactly 1."""
    scale, params = np.asarray(scale, np.float32), np.asarray(params, np.float32)
    for l, r0, g, v in scale_rows(spec):
        o, i = spec.out_dim[l], spec.in_dim[l]
        if g is None:
            assert (scale[r0:r0 + o] == np.float32(1.0)).all(), f"{tag}: plain layer {l} must have scale exactly 1"
            continue
        ref = O.row_scale_ref(params[g.offset:g.offset + o], params[v.offset:v.offset + o * i].reshape(o, i))
        hold(f"{tag} scale layer {l} (in {i})", scale[r0:r0 + o], ref, O.row_scale_bound(ref, i))


def packed_of_fresh_engine(spec, params):
    """`packed` of a fresh engine (zeroed buffer) after dsdf_materialize_weights of `params`."""
    e = Engine(spec, "cuda")
    e.params.copy_(params)
    e.materialize()
    return e.packed


def bits_equal(a, b):
    return a.numel() == b.numel() and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("clip", ["noclip", "coef<1", "coef=1"])
@pytest.mark.parametrize("name", list(ARENA_NETS))
def test_decoder_arena_adam_holds_the_spec(name, clip):
    """Engine.adam_step on arenas the test writes: parameters, both moments and the scale vector against the spec; `packed` bit-equal
    to a fresh dsdf_materialize_weights of the new parameters (padding included: the fresh engine's buffer starts zeroed, too).
    With clipping the spec's grad_scale is the fp32 coefficient Engine.grad_norm left on the device (its own value is
    test_grad_norm_and_clip_coefficient_hold_the_spec's subject): below 1, and exactly 1."""
    decoder_arena_adam(name, clip)


def decoder_arena_adam(name, clip, betas=(0.9, 0.999), eps=1e-8, steps=STEPS):
    """adam_rows_kernel (and adam_kernel on bn parameters) at Adam constants of the caller's choice."""
    b1, b2, ep = O.f32(betas[0]), O.f32(betas[1]), O.f32(eps)
    spec = arena_spec(name)
    rows = sum(spec.out_dim)
    if name.startswith("wn_"):
        assert sorted(spec.in_dim) == [7, 64, 65, 507, 515]
        assert (rows % 4 != 0) == (name == "wn_rows_1145")        # adam_rows_kernel: four rows per block, with and without a ragged last block
    lay_scale = None
    for aged in (True, False):
        p0, g0, m0, v0 = O.make_state(spec.n_params, 31 + len(name), aged=aged)
        O.check_state(p0, g0, m0, v0, aged=aged)
        for t in steps:
            eng = Engine(spec, "cuda")
            eng.params.copy_(_dev(p0)); eng.grads.copy_(_dev(g0)); eng.exp_avg.copy_(_dev(m0)); eng.exp_avg_sq.copy_(_dev(v0))
            eng.step = t - 1
            gs = 1.0
            if clip != "noclip":      # the coefficient is the one dsdf_grad_norm leaves on the device for this arena: the step's own pipeline
                norm = float(np.sqrt((g0.astype(np.float64) ** 2).sum()))
                gs = float(eng.grad_norm(O.f32(norm * (0.37 if clip == "coef<1" else 2.0)))[1].item())
                assert (0.36 < gs < 0.38) if clip == "coef<1" else gs == 1.0, gs
            eng.adam_step(None, None, None, None, LR_DEC, LR_LAT, clip=clip != "noclip", betas=betas, eps=eps)
            assert eng.step == t
            r = O.adam_ref(p0, g0, m0, v0, lr=LR_DEC, t=t, grad_scale=gs, b1=b1, b2=b2, eps=ep)
            tag = f"{name} {clip} {'aged' if aged else 'fresh'} t{t}"
            hold_adam(tag, eng.params, eng.exp_avg, eng.exp_avg_sq, r, m0, scaled=clip != "noclip")
            assert torch.equal(eng.grads.cpu(), torch.from_numpy(g0))
            if lay_scale is None:
                from tests.packed_numpy import layout_of
                lay_scale = layout_of(spec)["scale_off"]
            hold_scale_vector(tag, spec, eng.packed[lay_scale:lay_scale + rows].cpu().numpy(), eng.params.cpu().numpy())
            assert bits_equal(eng.packed, packed_of_fresh_engine(spec, eng.params)), f"{tag}: packed != materialize(new parameters)"


# ---- dsdf_grad_norm ------------------------------------------------------------------------------------------------------------

def test_grad_norm_and_clip_coefficient_hold_the_spec():
    """sumsq_partial_kernel + clip_coef_kernel at the sizes tests/test_gpu_workspace.py runs without looking at a value: the norm
    against float64, the coefficient for max_norm below the norm (< 1, at its bound) and above it (EXACTLY 1.0f once the norm is
    below max_norm - 1e-6 by more than the norm's own bound)."""
    from tests.test_gpu_workspace import GRAD_NORM_N
    lib = _lib.lib()
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    for n in GRAD_NORM_N:
        g0 = (torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64) * 0.01).to(torch.float32)
        if n >= 4096:
            g0[:: 20] = 0
        norm = float(torch.linalg.vector_norm(g0.double()))
        assert norm > 1e-6
        g = g0.cuda()
        out = torch.zeros(2, device="cuda")
        for factor in (0.5, 1.01, 2.0):
            mx = O.f32(norm * factor)
            _lib.check(lib.dsdf_grad_norm(_ptr(g), n, mx, _ptr(out), C.c_void_p(out.data_ptr() + 4), _ptr(ws), ws.numel(), _stream()))
            got_norm, got_coef = (float(x) for x in out.cpu())
            hold(f"grad_norm n{n}", [got_norm], [norm], [O.grad_norm_bound(norm, n)])
            ref = O.clip_coef_ref(norm, mx)
            if factor > 1:
                assert norm * (1 + O.grad_norm_bound(1.0, n)) + 1e-6 < mx            # above the norm by more than its bound
                assert ref == 1.0 and got_coef == 1.0, (n, factor, got_coef)
            else:
                assert ref < 1.0
                hold(f"clip coef n{n} x{factor}", [got_coef], [ref], [O.clip_coef_bound(ref, n)])


# ---- the fused finalize Adam of dsdf_train_step ------------------------------------------------------------------------------------

FUSED_NETS = {
    # name: (spec keywords, widest class K of finalize_row_wave<K> = ceil(max layer input / 64) rounded up to 1, 2, 4, 8; fused?)
    "in<=64_w40": (dict(L=5, dims=[40, 64, 40], dropout=[0, 1], dropout_prob=0.2, norm_layers=[0, 1, 2], weight_norm=True), 1, True),
    "in<=128_w72": (dict(L=13, dims=[72, 128, 72], dropout=[1], dropout_prob=0.2, norm_layers=[0, 1, 2], weight_norm=True), 2, True),
    "in<=256_w200": (dict(L=5, dims=[200, 256, 200], norm_layers=[0, 1, 2], weight_norm=True), 4, True),
    "in<=512_w507": (dict(L=5, dims=[320, 507, 508], dropout=[0], dropout_prob=0.2, norm_layers=[0, 1, 2], weight_norm=True), 8, True),
    "plain_layer": (dict(L=5, dims=[72, 72, 72], norm_layers=[0, 2], weight_norm=True), 2, True),
    "skip_layer": (dict(L=5, dims=[72, 72, 72], norm_layers=[0, 1, 2, 3], latent_in=[1], weight_norm=True), 2, True),
    # wider than the fused kernels take: the layer-by-layer path, whose finalize is the block form WITHOUT Adam -> dsdf_adam_step
    "falls_back_w520": (dict(L=5, dims=[520, 64], norm_layers=[0, 1], weight_norm=True), 16, False),
}


def fused_spec(name, **flags):
    kw = dict(FUSED_NETS[name][0])
    return NetSpec(kw.pop("L"), kw.pop("dims"), 3, **kw, **flags)


def wave_class(n_in):
    ku = -(-n_in // 64)
    return 1 if ku <= 1 else 2 if ku == 2 else 4 if ku <= 4 else 8 if ku <= 8 else 16      # 16: the block form (in > 512)


def tail_batch(mode, n_scenes=5):
    """(seg_scene, seg_offset, xyz, gt, seg_len): segment mode = 3 scenes x 64 points (hoisted columns), ragged = 70 + 59 points; both
    leave latent rows out of the batch (whole zero rows of the latent gradient)."""
    scenes, lens = ([0, 2, 3], [64, 64, 64]) if mode == "segment" else ([1, 4], [70, 59])
    assert max(scenes) < n_scenes
    idx = torch.repeat_interleave(torch.tensor(scenes), torch.tensor(lens))
    gen = torch.Generator().manual_seed(len(idx))
    xyz = torch.rand(len(idx), 3, generator=gen) * 2 - 1
    gt = xyz.norm(dim=1) - 0.5
    sc, so = make_segments(idx.cuda())
    return sc, so, xyz.cuda().contiguous(), gt.cuda().contiguous(), (64 if mode == "segment" else 0)


SENTINEL = 12345.0
STEP0 = 999


def aged_engine(spec, seed, n_scenes=5):
    """An engine at step 999 with reference-initialised parameters, aged moments, and its latent table with aged moments."""
    eng = Engine(spec, "cuda")
    eng.init_like_reference(generator=torch.Generator().manual_seed(seed))
    _, _, m0, v0 = O.make_state(spec.n_params, seed)
    eng.exp_avg.copy_(_dev(m0)); eng.exp_avg_sq.copy_(_dev(v0))
    eng.step = STEP0
    L = spec.latent_size
    lat = (torch.randn(n_scenes, L, generator=torch.Generator().manual_seed(seed + 1)) / math.sqrt(L)).cuda()
    _, _, lm, lv = O.make_state(n_scenes * L, seed + 2, row=L)
    return eng, lat, torch.zeros_like(lat), _dev(lm).view(n_scenes, L), _dev(lv).view(n_scenes, L)


# (clamp_dist 1: |tanh| <= 1, so no point of these small batches is clamped out of the loss -- a randomly initialised narrow decoder can put
# EVERY prediction of a 129-point batch outside a 0.1 band, and an all-zero gradient arena would test nothing)
STEP_KW = dict(clamp_dist=1.0, reg_coef=1e-4, code_bound=1.0, seed=5)


def test_finalize_row_wave_classes_are_all_reached_by_width():
    reached = set()
    for name, (_, k, fused) in FUSED_NETS.items():
        spec = fused_spec(name)
        assert max(wave_class(i) for i in spec.in_dim) == k, name
        assert fused == (max(spec.in_dim + spec.out_dim[:-1]) <= 512), name
        if fused:
            reached |= {wave_class(i) for i in spec.in_dim}
    assert reached == {1, 2, 4, 8}
    assert [fused_spec(n).in_dim[-1] for n in list(FUSED_NETS)[:4]] == [40, 72, 200, 508]          # ragged widths (not multiples of 64)
    assert 507 in fused_spec("in<=512_w507").in_dim


@pytest.mark.parametrize("mode", ["segment", "ragged"])
@pytest.mark.parametrize("name", list(FUSED_NETS))
def test_fused_finalize_adam_holds_the_spec_of_its_own_gradient(name, mode):
    """Two engines from one aged state at step 999, same batch, seed and latents: A runs train_forward_backward only, B train_step.
    The reference is the float64 spec applied to A's gradient arena and dlat; B's parameters, moments, latent table and latent
    moments are held to it at the spec's bounds -- both paths form every gradient entry with the same expressions (the finalize pass
    computes d once and either stores it or hands it to adam_elem), so nothing looser is needed.  The sentinel B's gradient arena is
    filled with tells the paths apart: the fused finalize never writes the arena; a net that falls back to dsdf_adam_step does."""
    fused_finalize_adam(name, mode)


def fused_finalize_adam(name, mode, betas=(0.9, 0.999), eps=1e-8):
    """finalize_row_wave<K> + Adam, the ride and the latent Adam of dsdf_train_step at Adam constants of the caller's choice."""
    b1, b2, ep = O.f32(betas[0]), O.f32(betas[1]), O.f32(eps)
    spec = fused_spec(name)
    fused = FUSED_NETS[name][2] and os.environ.get("DSDF_NO_FUSED") != "1"      # (the switch sends every net down the fallback)
    sc, so, xyz, gt, seg_len = tail_batch(mode)
    n = xyz.shape[0]
    A, latA, dlatA, lmA, lvA = aged_engine(spec, 40 + len(name))
    B, latB, dlatB, lmB, lvB = aged_engine(spec, 40 + len(name))
    assert torch.equal(A.params, B.params) and torch.equal(latA, latB) and torch.equal(lmA, lmB)
    p0, m0, v0 = (x.cpu().numpy() for x in (A.params, A.exp_avg, A.exp_avg_sq))
    lm0, lv0 = lmA.cpu().numpy().reshape(-1), lvA.cpu().numpy().reshape(-1)
    A.train_forward_backward(latA, dlatA, sc, so, xyz, gt, n_norm=n, training=True, seg_len=seg_len, **STEP_KW)
    names = [r[0] for r in _lib.ws_regions()[0]]
    assert ("hoistU" in names) == (mode == "segment" and fused), names      # segment mode (hoisted x0 columns) exactly where expected
    B.grads.fill_(SENTINEL)
    B.train_step(latB, dlatB, lmB, lvB, sc, so, xyz, gt, n_norm=n, lr_decoder=LR_DEC, lr_latent=LR_LAT, training=True, seg_len=seg_len,
                 betas=betas, eps=eps, **STEP_KW)
    assert A.step == STEP0 and B.step == STEP0 + 1
    survived = bool((B.grads == SENTINEL).all())
    assert survived == fused, f"{name}: expected the {'fused finalize' if fused else 'two-call fallback'} path"
    if not fused:
        assert not bool((B.grads == SENTINEL).any()) and torch.equal(B.grads, A.grads)
    assert torch.equal(A.loss, B.loss) and torch.equal(dlatA, dlatB)          # same forward, same backward
    g = A.grads.cpu().numpy()
    assert np.isfinite(g).all() and (g != 0).mean() > 0.5
    tag = f"{name} {mode}"
    r = O.adam_ref(p0, g, m0, v0, lr=LR_DEC, t=STEP0 + 1, b1=b1, b2=b2, eps=ep)
    hold_adam(tag + " decoder", B.params, B.exp_avg, B.exp_avg_sq, r, m0)
    dl = dlatA.cpu().numpy().reshape(-1)
    absent = [s for s in range(latA.shape[0]) if s not in sc.cpu().tolist()]
    assert absent and not dlatA[absent].any()                                 # latent rows absent from the batch: zero gradient rows
    rl = O.adam_ref(latA.cpu().numpy().reshape(-1), dl, lm0, lv0, lr=LR_LAT, t=STEP0 + 1, b1=b1, b2=b2, eps=ep)     # (A's table: renormed by the forward, as B's)
    hold_adam(tag + " latent", latB, lmB, lvB, rl, lm0)
    from tests.packed_numpy import layout_of
    so_ = layout_of(spec)["scale_off"]
    hold_scale_vector(tag, spec, B.packed[so_:so_ + sum(spec.out_dim)].cpu().numpy(), B.params.cpu().numpy())
