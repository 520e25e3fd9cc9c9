"""What every byte of the packed-weight buffer must be (numpy), from the parameter arena, the layout the library states
(dsdf_debug_packed_layout) and the weight-norm scale vector -- the formulas of kernels.hpp wn_tiles_kernel and fused_bf16x8.hpp:

  W[r][c]   = fl32(v[r][c] * scale[r])                                   [out][ldw]
  W^T       = its transpose                                               [in][ldwt]        (every layer but the last)
  Wf / WTf  = fragment order of B = W (n = out, k = in) / B = W^T (n = in, k = out):
              Bf[((nt U + u) 2 + i) 256 + lane 4 + e] = B[32 nt + (lane & 31)][16 u + 8 (lane >> 5) + 4 i + e], zero out of range
  Wfb       = bf16(W) rounded to nearest even, element ((nt 32 + slot(u)) 64 + lane) 8 + 4 i + e, k-units phase-major:
              slot(u) = 16 ((u >> 1) & 1) + 2 (u >> 2) + (u & 1)
  Ws / WTs  = three bf16 planes h, m, l of B = W / W^T, each the top 16 bits of what is left (x = h + m + l exactly),
              element ((nt U + u) 64 + lane) 8 + 4 i + e of its plane

Everything else -- leading-dimension padding, rows and k-units past the matrix inside a written tile (the kernel writes zeros there),
n-tiles that only the rounding to 4 allocates, unused k-unit slots, every fragment copy of the last layer -- is ZERO: the caller zeroes the
buffer once and no kernel may write there."""
import ctypes as C

import numpy as np


def layout_of(spec):
    """dsdf_debug_packed_layout as a dict of Python ints / lists (one entry per layer)."""
    from deepsdf_amd import _lib
    lay = _lib.DsdfPackedLayout()
    net = spec.c_struct()
    _lib.check(_lib.lib().dsdf_debug_packed_layout(C.byref(net), C.byref(lay)))
    d = dict(total=int(lay.total), scale_off=int(lay.scale_off))
    for k in ("w_off", "wt_off", "wf_off", "wtf_off", "wfb_off", "ws_off", "wts_off", "ws_plane", "wts_plane", "ldw", "ldwt", "uf", "utf"):
        d[k] = [int(x) for x in getattr(lay, k)]
    return d


def bf16_rne_bits(x):
    """float32 array -> uint16 bf16 bit patterns, round to nearest, ties to even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_trunc_bits(x):
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def split3_bits(x):
    """The three bf16 planes of fused_kloop_split's operands: each the top 16 bits of what is left.  float32 array -> (h, m, l) uint16."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    top = lambda a: (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    h = top(x)
    r = x - h           # exact: the low 16 bits of the significand
    m = top(r)
    t = r - m           # exact
    return bf16_trunc_bits(h), bf16_trunc_bits(m), bf16_trunc_bits(t)


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def frag_index(n, k, U):
    """Element index of B[n][k] inside a fragment-ordered fp32 copy with U k-units per n-tile."""
    nt, ln = n // 32, n % 32
    u, rem = k // 16, k % 16
    h, i, e = rem // 8, (rem % 8) // 4, rem % 4
    return ((nt * U + u) * 2 + i) * 256 + (ln + 32 * h) * 4 + e


def frag_index_bf16(n, k, U, phase_major=False):
    """Element index (in bf16 elements) of B[n][k] inside a bf16 fragment copy: U k-units per n-tile in natural order (the split
    planes), or 32 phase-major slots (Wfb)."""
    nt, ln = n // 32, n % 32
    u, rem = k // 16, k % 16
    h, j = rem // 8, rem % 8
    if phase_major:
        u = 16 * ((u >> 1) & 1) + 2 * (u >> 2) + (u & 1)
        U = 32
    return ((nt * U + u) * 64 + (ln + 32 * h)) * 8 + j


def layer_tensors(spec, params):
    """[(v [out, in] float32, row0)] per layer from the flat parameter arena (numpy float32)."""
    out, r0 = [], 0
    for l in range(spec.n_layers):
        pv = [p for p in spec.params if p.layer == l and p.kind in ("v", "weight")][0]
        out.append((params[pv.offset:pv.offset + pv.numel].reshape(pv.shape), r0))
        r0 += spec.out_dim[l]
    return out


def expected_packed(spec, lay, params, scale):
    """The whole buffer as a float32 array of lay['total'] elements (compare its bytes).  params: the flat fp32 arena; scale: the
    fp32 scale vector [sum of out_dim] the other regions are derived from."""
    params = np.ascontiguousarray(params, dtype=np.float32)
    scale = np.ascontiguousarray(scale, dtype=np.float32)
    buf = np.zeros(lay["total"], dtype=np.float32)
    b16 = buf.view(np.uint16)
    buf[lay["scale_off"]:lay["scale_off"] + scale.size] = scale
    regions = {"scale": [(lay["scale_off"], lay["scale_off"] + scale.size)]}
    last = spec.n_layers - 1
    for l, (v, r0) in enumerate(layer_tensors(spec, params)):
        o, i = v.shape
        W = v * scale[r0:r0 + o, None]                       # float32 * float32: one rounding
        assert W.dtype == np.float32
        r, c = np.meshgrid(np.arange(o), np.arange(i), indexing="ij")
        buf[lay["w_off"][l] + r * lay["ldw"][l] + c] = W
        regions.setdefault("W", []).append((lay["w_off"][l], lay["w_off"][l] + o * lay["ldw"][l]))
        if l == last:
            continue
        buf[lay["wt_off"][l] + c * lay["ldwt"][l] + r] = W
        regions.setdefault("WT", []).append((lay["wt_off"][l], lay["wt_off"][l] + i * lay["ldwt"][l]))
        buf[lay["wf_off"][l] + frag_index(r, c, lay["uf"][l])] = W
        buf[lay["wtf_off"][l] + frag_index(c, r, lay["utf"][l])] = W
        regions.setdefault("Wf", []).append((lay["wf_off"][l], lay["wtf_off"][l]))
        regions.setdefault("WTf", []).append((lay["wtf_off"][l], lay["wfb_off"][l]))
        if spec.forward_bf16:
            b16[2 * lay["wfb_off"][l] + frag_index_bf16(r, c, 0, phase_major=True)] = bf16_rne_bits(W)
            regions.setdefault("Wfb", []).append((lay["wfb_off"][l], lay["wfb_off"][l] + ((o + 31) // 32 + 3) // 4 * 4 * 32 * 256))
        if spec.gemm_split:
            for name, off, plane, U, idx in (("Ws", lay["ws_off"][l], lay["ws_plane"][l], lay["uf"][l], frag_index_bf16(r, c, lay["uf"][l])),
                                             ("WTs", lay["wts_off"][l], lay["wts_plane"][l], lay["utf"][l],
                                              frag_index_bf16(c, r, lay["utf"][l]))):
                for q, bits in enumerate(split3_bits(W)):
                    b16[2 * off + q * plane + idx] = bits
                    regions.setdefault(f"{name}.{'hml'[q]}", []).append((off + q * plane // 2, off + (q + 1) * plane // 2))
    return buf, regions


def first_difference(got, want, regions):
    """None when the two float32 buffers are bit-equal; else a message naming the region and the first differing word."""
    a, b = got.view(np.uint32), want.view(np.uint32)
    if a.size != b.size:
        return f"size {a.size} != {b.size}"
    bad = np.flatnonzero(a != b)
    if bad.size == 0:
        return None
    w = int(bad[0])
    where = "padding"
    for name, spans in regions.items():
        if any(s <= w < e for s, e in spans):
            where = name
    return f"{bad.size} words differ, first at float {w} ({where}): got 0x{int(a[w]):08x}, want 0x{int(b[w]):08x}"
