"""CPU: the building blocks of tests/packed_numpy.py (the stated layout of the packed-weight buffer): bf16 rounding against
torch.bfloat16, the three-plane split, the fragment maps, and the layout dsdf_debug_packed_layout reports.  No GPU."""
import numpy as np
import pytest
import torch

from tests import packed_numpy as P


def _random_f32(n, seed, min_exp=-100, max_exp=100):
    """Random sign, exponent and ALL 23 significand bits: |x| in [2^min_exp, 2^max_exp)."""
    rng = np.random.default_rng(seed)
    bits = (rng.integers(0, 2, n, dtype=np.uint32) << 31) | (rng.integers(127 + min_exp, 127 + max_exp, n, dtype=np.uint32) << 23) \
        | rng.integers(0, 1 << 23, n, dtype=np.uint32)
    return bits.view(np.float32)


def test_bf16_rounding_is_torch_bfloat16():
    x = _random_f32(200000, 1)
    ties = ((_random_f32(4096, 2).view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)).view(np.float32)   # exactly half way
    x = np.concatenate([x, ties, np.float32([0.0, -0.0, 1.0, -1.0, 3.3895314e38])])       # the last: rounds up across a binade
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(P.bf16_rne_bits(x), want)
    assert not np.array_equal(P.bf16_trunc_bits(x), want)                                  # truncation is a different function
    lo = ties.view(np.uint32) >> 16
    assert np.array_equal(P.bf16_rne_bits(ties), (lo + (lo & 1)).astype(np.uint16))         # ties go to the even neighbour


def test_three_planes_sum_back_exactly():
    x = np.concatenate([_random_f32(300000, 3), np.float32([2.0 ** -100, -(2.0 ** -100), 1.0, 0.0, -0.0]),
                        (np.float32(2.0 ** -100) * (1 + np.arange(1, 200, dtype=np.float32) * np.float32(2.0 ** -23)))])
    assert float(np.abs(x[x != 0]).min()) >= 2.0 ** -100
    h, m, l = (P.bf16_bits_to_f32(b).astype(np.float64) for b in P.split3_bits(x))
    assert np.array_equal(h + m + l, x.astype(np.float64))
    nz = x != 0
    assert (np.abs(m[nz]) <= np.abs(h[nz]) * 2.0 ** -7).all() and (np.abs(l[nz]) <= np.abs(h[nz]) * 2.0 ** -15).all()
    assert (l != 0).mean() > 0.9                        # the low plane is not idle: a test that zeroed it would see it


@pytest.mark.parametrize("N,K", [(1, 1), (32, 16), (33, 17), (40, 72), (253, 507), (512, 512)])
def test_fragment_maps_are_bijections_onto_the_in_range_entries(N, K):
    nt, U = (N + 31) // 32, 2 * ((K + 31) // 32)
    n, k = np.meshgrid(np.arange(32 * nt), np.arange(16 * U), indexing="ij")
    for idx, size in ((P.frag_index(n, k, U), nt * U * 512), (P.frag_index_bf16(n, k, U), nt * U * 512)):
        assert idx.min() == 0 and idx.max() == size - 1 and np.unique(idx).size == idx.size == size      # all slots, each once
    inr = (n < N) & (k < K)
    assert np.unique(P.frag_index(n, k, U)[inr]).size == N * K
    # the formula of kernels.hpp, read the other way: slot -> (row, column)
    s = np.arange(nt * U * 512)
    e, lane, i, u, t = s % 4, (s // 4) % 64, (s // 256) % 2, (s // 512) % U, s // (512 * U)
    assert np.array_equal(P.frag_index(32 * t + (lane & 31), 16 * u + 8 * (lane >> 5) + 4 * i + e, U), s)
    if K <= 512:         # phase-major: 32 slots per n-tile, units of even 32-column tiles in slots 0.., of odd ones in slots 16..
        nn, kk = np.meshgrid(np.arange(32 * nt), np.arange(16 * U), indexing="ij")
        idx = P.frag_index_bf16(nn, kk, 0, phase_major=True)
        assert np.unique(idx).size == idx.size and idx.max() < nt * 32 * 512
        slot = (idx // 512) % 32
        cb = kk // 32
        assert np.array_equal(slot, (cb & 1) * 16 + 2 * (cb >> 1) + (kk // 16) % 2)


def test_layout_entry_and_expected_buffer_on_the_host():
    """dsdf_debug_packed_layout against dsdf_packed_floats and its own invariants (regions in order, disjoint, inside the buffer),
    and expected_packed's own consistency: W^T is W transposed, the fragment copies hold exactly W's multiset of values."""
    from deepsdf_amd.build import build_library
    build_library()
    import ctypes as C
    from deepsdf_amd import _lib
    from deepsdf_amd.net import NetSpec
    for kw in (dict(), dict(forward_bf16=True), dict(gemm_split=True), dict(forward_bf16=True, gemm_split=True)):
        spec = NetSpec(5, [40, 72, 200], 3, norm_layers=[0, 1, 3], latent_in=[2], weight_norm=True, **kw)
        lay = P.layout_of(spec)
        n = C.c_int64()
        _lib.check(_lib.lib().dsdf_packed_floats(C.byref(spec.c_struct()), C.byref(n)))
        assert lay["total"] == n.value and lay["total"] % 64 == 0
        for l in range(spec.n_layers):
            o, i = spec.out_dim[l], spec.in_dim[l]
            assert lay["ldw"][l] == (i + 31) // 32 * 32 and lay["ldwt"][l] == (o + 31) // 32 * 32
            assert lay["uf"][l] == 2 * ((i + 31) // 32) and lay["utf"][l] == 2 * ((o + 31) // 32)
            assert lay["w_off"][l] + o * lay["ldw"][l] <= lay["wt_off"][l] and lay["wt_off"][l] + i * lay["ldwt"][l] <= lay["scale_off"]
            assert lay["wf_off"][l] >= lay["scale_off"] + sum(spec.out_dim) and lay["wf_off"][l] < lay["wtf_off"][l] <= lay["wfb_off"][l]
            assert lay["ws_plane"][l] * 2 == (lay["wtf_off"][l] - lay["wf_off"][l]) * 2      # as many bf16 per plane as floats in Wf
            assert lay["ws_off"][l] <= lay["wts_off"][l] <= lay["total"]
            assert (lay["wts_off"][l] - lay["ws_off"][l]) * 2 == (3 * lay["ws_plane"][l] if spec.gemm_split else 0)
        assert lay["w_off"][spec.n_layers] == -1 and lay["uf"][spec.n_layers] == 0
        rng = np.random.default_rng(1)
        params = rng.normal(0, 0.1, spec.n_params).astype(np.float32)
        scale = rng.uniform(0.5, 2.0, sum(spec.out_dim)).astype(np.float32)
        buf, regions = P.expected_packed(spec, lay, params, scale)
        assert buf.size == lay["total"] and P.first_difference(buf, buf.copy(), regions) is None
        (v0, _), o, i = P.layer_tensors(spec, params)[0], spec.out_dim[0], spec.in_dim[0]
        W = buf[lay["w_off"][0]:lay["w_off"][0] + o * lay["ldw"][0]].reshape(o, -1)
        WT = buf[lay["wt_off"][0]:lay["wt_off"][0] + i * lay["ldwt"][0]].reshape(i, -1)
        assert np.array_equal(W[:, :i], v0 * scale[:o, None]) and not W[:, i:].any()
        assert np.array_equal(WT[:, :o], W[:, :i].T) and not WT[:, o:].any()
        Wf = buf[lay["wf_off"][0]:lay["wtf_off"][0]]
        assert np.array_equal(np.sort(Wf[Wf != 0]), np.sort(W[W != 0]))
        other = buf.copy()
        other[lay["wtf_off"][1] + 5] += 1
        assert "WTf" in P.first_difference(other, buf, regions)
    assert _lib.lib().dsdf_debug_packed_layout(None, C.byref(_lib.DsdfPackedLayout())) == -1
    assert _lib.lib().dsdf_debug_packed_layout(C.byref(spec.c_struct()), None) == -1 and b"NULL" in _lib.lib().dsdf_last_error()
