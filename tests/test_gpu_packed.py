"""-m gpu: the packed-weight buffer against its STATED layout, bit for bit, padding included.

`packed` is what every forward and backward kernel reads its weights from; until now it was only ever compared with another
`packed` or judged through a forward pass.  tests/packed_numpy.py builds the whole expected buffer from the parameter arena, the
layout dsdf_debug_packed_layout states and the scale vector: W, W^T, the fragment-ordered Wf / WTf, the phase-major bf16 Wfb
(round to nearest even) and the three-plane splits Ws / WTs, zeros everywhere else.  Compared in the three situations that write the
buffer: dsdf_materialize_weights on a zeroed buffer, dsdf_adam_step, dsdf_train_step.  The padding counts because the kernels rely on
the zeros there and nothing else checks that a step leaves them.

The scale vector is held to its float64 value g / ||v_row|| at the counted bound of optim_numpy.row_scale_bound; every other region
is a function of the scale vector that is IN the buffer (one fp32 product per entry, exact copies and bit cuts after that), so it is
compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

from deepsdf_amd import _lib
from deepsdf_amd.engine import Engine
from deepsdf_amd.net import NetSpec
from tests import optim_numpy as O
from tests import packed_numpy as P
from tests.test_gpu_optim_tail import (ARENA_NETS, FUSED_NETS, LR_DEC, LR_LAT, STEP_KW, _dev, arena_spec, fused_spec, hold_scale_vector,
                                       tail_batch)
from tests.test_gpu_parity import BIG

pytestmark = pytest.mark.gpu

FLAGS = [dict(), dict(forward_bf16=True), dict(gemm_split=True), dict(forward_bf16=True, gemm_split=True)]


def make_spec(name, flags):
    flags = {"forward_bf16": False, "gemm_split": False, **flags}          # explicit: the environment's default does not apply
    if name == "big_8x512_L256":
        return NetSpec(256, **{**BIG, **flags})
    return arena_spec(name, **flags) if name in ARENA_NETS else fused_spec(name, **flags)


def admitted(name, flags):
    """validate()'s conditions on fwd_bf16 / gemm_split (dsdf_api.hip): every width <= 512, none of the layer-by-layer variants."""
    plain = make_spec(name, {})
    if not flags:
        return True
    narrow = max(plain.in_dim + plain.out_dim[:-1]) <= 512
    return narrow and not any(plain.ln) and not plain.xyz_in_all and not plain.latent_dropout and not plain.skip[-1]


NAMES = list(ARENA_NETS) + list(FUSED_NETS) + ["big_8x512_L256"]
CASES = [(n, f) for n in NAMES for f in FLAGS if admitted(n, f)]


def _id(c):
    return c[0] + "".join("+" + k for k in c[1])


def test_the_admitted_flag_combinations_are_the_librarys():
    lib, n = _lib.lib(), C.c_int64()
    count = 0
    for name in NAMES:
        for f in FLAGS[1:]:
            net = make_spec(name, {}).c_struct()
            net.fwd_bf16, net.gemm_split = int(f.get("forward_bf16", False)), int(f.get("gemm_split", False))
            assert (lib.dsdf_packed_floats(C.byref(net), C.byref(n)) == 0) == admitted(name, f), (name, f)
            count += admitted(name, f)
    assert count == 3 * (len(FUSED_NETS) - 1 + 1 + 1)          # every fused net, the 8 x 512 net and the narrow plain arena net


def check_packed(tag, eng, lay):
    spec = eng.spec
    packed, params = eng.packed.cpu().numpy(), eng.params.cpu().numpy()
    rows = sum(spec.out_dim)
    assert packed.size == lay["total"]
    scale = packed[lay["scale_off"]:lay["scale_off"] + rows].copy()
    hold_scale_vector(tag, spec, scale, params)
    want, regions = P.expected_packed(spec, lay, params, scale)
    if spec.forward_bf16:
        assert "Wfb" in regions
    if spec.gemm_split:
        assert "WTs.l" in regions and "Ws.h" in regions
    diff = P.first_difference(packed, want, regions)
    assert diff is None, f"{tag}: {diff}"
    nz = int((want.view(np.uint32) != 0).sum())
    print(f"{tag}: {packed.size} words bit-equal ({nz} non-zero, {packed.size - nz} zero)")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_packed_buffer_is_its_stated_layout_in_all_three_situations(case):
    name, flags = case
    spec = make_spec(name, flags)
    assert spec.forward_bf16 == bool(flags.get("forward_bf16")) and spec.gemm_split == bool(flags.get("gemm_split"))
    lay = P.layout_of(spec)
    eng = Engine(spec, "cuda")
    eng.init_like_reference(generator=torch.Generator().manual_seed(7 + len(name)))
    assert not bool(eng.packed.any())                                  # the caller zeroes the buffer once
    tag = _id(case)
    eng.materialize()
    check_packed(tag + " materialize", eng, lay)

    _, g0, m0, v0 = O.make_state(spec.n_params, 5 + len(name))
    eng.grads.copy_(_dev(g0)); eng.exp_avg.copy_(_dev(m0)); eng.exp_avg_sq.copy_(_dev(v0))
    eng.step = 999
    before = eng.params.clone()
    eng.adam_step(None, None, None, None, LR_DEC, LR_LAT)
    assert not torch.equal(before, eng.params)
    check_packed(tag + " adam_step", eng, lay)

    mode = "ragged" if name in ARENA_NETS else "segment"
    sc, so, xyz, gt, seg_len = tail_batch(mode)
    L = spec.latent_size
    lat = (torch.randn(5, L, generator=torch.Generator().manual_seed(3)) / L ** 0.5).cuda()
    dlat, lm, lv = torch.zeros_like(lat), torch.zeros_like(lat), torch.zeros_like(lat)
    before = eng.params.clone()
    eng.train_step(lat, dlat, lm, lv, sc, so, xyz, gt, n_norm=xyz.shape[0], lr_decoder=LR_DEC, lr_latent=LR_LAT, training=True,
                   seg_len=seg_len, **STEP_KW)
    assert not torch.equal(before, eng.params) and bool(torch.isfinite(eng.loss).all())
    check_packed(tag + " train_step", eng, lay)
