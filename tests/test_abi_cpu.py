"""CPU (no GPU needed): the C-ABI library builds, loads, and exports every symbol include/dsdf.h declares;
host-side layout logic agrees with the library.  No compute call is made."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from deepsdf_amd.build import build_library
    build_library()
    from deepsdf_amd import _lib
    return _lib.lib()


def test_every_declared_symbol_is_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "dsdf.h")).read()
    names = set(re.findall(r"\b(dsdf_[a-z_0-9]+)\s*\(", hdr))
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/dsdf.h but not exported"
    from deepsdf_amd._lib import PROTOTYPES
    assert names == set(PROTOTYPES) | {"dsdf_last_error"}


def test_layout_and_sizes(lib):
    from deepsdf_amd import _lib
    from deepsdf_amd.net import NetSpec
    spec = NetSpec(256, [512] * 8, 3, dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)),
                   latent_in=[4], weight_norm=True)
    assert spec.n_params == 1843195 and spec.w_mac == 1835520
    assert spec.out_dim[3] == 253 and spec.in_dim[4] == 512
    net = spec.c_struct()
    lay = _lib.DsdfParamLayout()
    assert lib.dsdf_param_layout(C.byref(net), C.byref(lay)) == 0
    assert lay.total == spec.n_params
    for p in spec.params:
        off = {"bias": lay.bias_off, "g": lay.g_off, "v": lay.v_off, "weight": lay.v_off}[p.kind][p.layer]
        assert off == p.offset, p.name
    b = C.c_size_t()
    assert lib.dsdf_workspace_bytes(C.byref(net), 16384, 64, C.byref(b)) == 0
    assert 300e6 < b.value < 900e6
    assert lib.dsdf_decode_workspace_bytes(C.byref(net), 16384, C.byref(b)) == 0
    assert b.value < 200e6


def test_gradient_buckets(lib):
    """dsdf_grad_buckets: where the K-bucket data-parallel backward (DsdfLossCfg.dw_phase / dw_buckets) cuts the layers and the
    arena; dsdf_dw_phase_supported; dsdf_workspace_bytes_buckets."""
    from deepsdf_amd.net import NetSpec
    spec = NetSpec(256, [512] * 8, 3, dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)), latent_in=[4], weight_norm=True)
    net = spec.c_struct()
    first, off = (C.c_int32 * 2)(), (C.c_int64 * 3)()
    assert lib.dsdf_grad_buckets(C.byref(net), 2, first, off) == 0
    assert list(first) == [4, 0] and off[0] == spec.n_params and off[2] == 0
    assert off[1] == min(p.offset for p in spec.params if p.layer == 4) == sum(p.numel for p in spec.params if p.layer < 4)
    assert 0.35 < off[1] / spec.n_params < 0.65                                     # two buckets of comparable size
    first, off = (C.c_int32 * 4)(), (C.c_int64 * 5)()
    assert lib.dsdf_grad_buckets(C.byref(net), 4, first, off) == 0
    assert list(first) == [6, 4, 2, 0]
    assert list(off) == [spec.n_params] + [sum(p.numel for p in spec.params if p.layer < k) for k in (6, 4, 2, 0)]
    plain = NetSpec(5, [48] * 3, 3)                                                 # no weight norm: weight first, then bias
    first, off = (C.c_int32 * 2)(), (C.c_int64 * 3)()
    assert lib.dsdf_grad_buckets(C.byref(plain.c_struct()), 2, first, off) == 0
    assert first[0] == 2 and off[1] == min(p.offset for p in plain.params if p.layer == 2)
    first, off = (C.c_int32 * 8)(), (C.c_int64 * 9)()                               # 4 layers, 8 buckets: empty buckets repeat an offset
    assert lib.dsdf_grad_buckets(C.byref(plain.c_struct()), 8, first, off) == 0
    assert list(first) == [3, 3, 2, 2, 1, 1, 0, 0] and off[0] == plain.n_params and off[8] == 0
    assert all(off[b + 1] <= off[b] for b in range(8)) and off[1] == off[2]
    assert lib.dsdf_grad_buckets(C.byref(plain.c_struct()), 2, None, off) == -1
    assert lib.dsdf_grad_buckets(C.byref(plain.c_struct()), 1, first, off) == -1
    assert lib.dsdf_grad_buckets(C.byref(plain.c_struct()), 9, first, off) == -1
    assert lib.dsdf_dw_phase_supported(C.byref(net)) == 1
    wide = NetSpec(8, [640] * 3, 3)                                                 # wider than the fused kernels take
    assert lib.dsdf_dw_phase_supported(C.byref(wide.c_struct())) == 0
    b2, b8 = C.c_size_t(), C.c_size_t()
    assert lib.dsdf_workspace_bytes(C.byref(net), 16384, 64, C.byref(b2)) == 0
    assert lib.dsdf_workspace_bytes_buckets(C.byref(net), 16384, 64, 2, C.byref(b8)) == 0 and b8.value == b2.value
    assert lib.dsdf_workspace_bytes_buckets(C.byref(net), 16384, 64, 8, C.byref(b8)) == 0 and b8.value > b2.value
    assert lib.dsdf_workspace_bytes_buckets(C.byref(net), 16384, 64, 9, C.byref(b8)) == -1


def test_invalid_nets_rejected(lib):
    from deepsdf_amd.net import NetSpec
    with pytest.raises(NotImplementedError):
        NetSpec(4, [32] * 2, 3, xyz_in_all=True, forward_bf16=True)
    with pytest.raises(NotImplementedError, match="output layer"):      # config 5's kernels: the output layer sees activations only
        NetSpec(4, [32] * 2, 3, latent_in=[2], forward_bf16=True)
    last_skip = NetSpec(4, [32] * 2, 3, latent_in=[2]).c_struct()          # fine in fp32 ...
    bq = C.c_size_t()
    assert lib.dsdf_workspace_bytes(C.byref(last_skip), 8, 1, C.byref(bq)) == 0
    last_skip.fwd_bf16 = 1                                                  # ... refused by the library too
    assert lib.dsdf_workspace_bytes(C.byref(last_skip), 8, 1, C.byref(bq)) == -1 and b"output layer" in lib.dsdf_last_error()
    ln = NetSpec(4, [32] * 2, 3, norm_layers=[0, 2], weight_norm=False)    # LayerNorm variant: bn modules, also the unused last one
    assert [p.name for p in ln.params] == ["lin0.weight", "lin0.bias", "bn0.weight", "bn0.bias", "lin1.weight", "lin1.bias",
                                           "lin2.weight", "lin2.bias", "bn2.weight", "bn2.bias"]
    both = ln.c_struct()
    both.weight_norm_mask = 1
    b1 = C.c_size_t()
    assert lib.dsdf_workspace_bytes(C.byref(both), 8, 1, C.byref(b1)) == -1 and b"exclude" in lib.dsdf_last_error()
    x = NetSpec(4, [32] * 3, 3, xyz_in_all=True, latent_in=[2])           # deep_sdf_decoder.py:42-48 layer arithmetic
    assert x.out_dim == [29, 25, 29, 1] and x.in_dim == [7, 32, 32, 32]
    bad = x.c_struct()
    bad.xyz_in_all = 0                                                    # widths no longer add up without the xyz columns
    b0 = C.c_size_t()
    assert lib.dsdf_workspace_bytes(C.byref(bad), 8, 1, C.byref(b0)) == -1 and b"in_dim" in lib.dsdf_last_error()
    spec = NetSpec(4, [32, 32, 32], 3, latent_in=[1, 2])
    b = C.c_size_t()
    net = spec.c_struct()
    assert lib.dsdf_workspace_bytes(C.byref(net), 8, 1, C.byref(b)) == -1
    assert b"latent_in" in lib.dsdf_last_error()


def test_param_names_match_oracle():
    from deepsdf_amd.net import NetSpec
    from oracle import deepsdf_oracle as orc
    kw = dict(dims=[64] * 4, dropout=[0, 1, 2, 3], dropout_prob=0.2, norm_layers=[0, 1, 2, 3], latent_in=[2],
              weight_norm=True, geom_dimension=3)
    assert [p.name for p in NetSpec(4, **kw).params] == orc.param_names(orc.make_net(4, **kw))
    from deepsdf_amd.net import dropout_layer_key
    assert dropout_layer_key(1234, 5, 3) == orc.dropout_layer_key(1234, 5, 3)
    assert dropout_layer_key((1 << 40) + 7, (1 << 33) + 1, 0) == orc.dropout_layer_key((1 << 40) + 7, (1 << 33) + 1, 0)


def test_size_queries_survive_degenerate_batches(lib):
    from deepsdf_amd.net import NetSpec
    net = NetSpec(4, [32, 32], 3, norm_layers=[0, 1], weight_norm=True).c_struct()
    b = C.c_size_t()
    for n in (0, 1, 63, 64, 65):
        assert lib.dsdf_workspace_bytes(C.byref(net), n, 1 if n else 0, C.byref(b)) == 0 and b.value > 0
        assert lib.dsdf_decode_workspace_bytes(C.byref(net), n, C.byref(b)) == 0
    assert lib.dsdf_workspace_bytes(C.byref(net), -1, 0, C.byref(b)) == -1


def test_argument_errors_are_reported_before_any_launch(lib):
    """Entry points validate their arguments on the host and fail with a message (no GPU needed to see that)."""
    from deepsdf_amd import _lib
    from deepsdf_amd.net import NetSpec
    lib.dsdf_last_error.restype = C.c_char_p
    assert lib.dsdf_sample_batch(None, 3, None, None, None, None, None, 4, 64, 1, None, None, None) == -1
    assert b"NULL" in lib.dsdf_last_error()
    dummy = C.c_void_p(256)     # never dereferenced: the shape checks come first
    assert lib.dsdf_sample_batch(dummy, 0, dummy, dummy, dummy, dummy, dummy, 4, 64, 1, dummy, dummy, None) == -1
    assert b"geom_dim" in lib.dsdf_last_error()
    assert lib.dsdf_sample_batch(dummy, 3, dummy, dummy, dummy, dummy, dummy, 4, 1, 1, dummy, dummy, None) == -1   # 2*(1//2) == 0 rows
    # the bf16 forward exists for widths <= 512 only, and the single-code decode needs the fp32 fused forward
    wide = NetSpec(8, [640, 640], 3, forward_bf16=True).c_struct()
    n = C.c_int64()
    assert lib.dsdf_packed_floats(C.byref(wide), C.byref(n)) == -1 and b"fwd_bf16" in lib.dsdf_last_error()
    net = NetSpec(8, [64, 64], 3).c_struct()
    assert lib.dsdf_decode_latent(C.byref(net), None, None, None, None, 10, None, None, 0, None) == -1
    # dsdf_decode_latent_supported is the ONE definition of "the single-code decode takes this net" (decode_sdf asks it)
    big = NetSpec(256, [512] * 8, 3, dropout=list(range(8)), dropout_prob=0.2, norm_layers=list(range(8)), latent_in=[4], weight_norm=True)
    assert lib.dsdf_decode_latent_supported(C.byref(big.c_struct())) == 1
    assert lib.dsdf_decode_latent_supported(C.byref(net)) == 1
    for kw in (dict(norm_layers=[0, 1], weight_norm=False),             # LayerNorm
               dict(xyz_in_all=True), dict(latent_dropout=True)):       # the other two layer-by-layer variants
        assert lib.dsdf_decode_latent_supported(C.byref(NetSpec(8, [64, 64], 3, **kw).c_struct())) == 0, kw
    assert lib.dsdf_decode_latent_supported(C.byref(NetSpec(8, [640, 640], 3).c_struct())) == 0       # wider than the fused kernels
    assert lib.dsdf_decode_latent_supported(C.byref(NetSpec(8, [64], 3).c_struct())) == 0             # one hidden layer
    assert lib.dsdf_decode_latent_supported(C.byref(NetSpec(8, [64, 64], 5).c_struct())) == 0         # geom_dim > 4
    broken = NetSpec(8, [64, 64], 3).c_struct()
    broken.in_dim[1] = 63
    assert lib.dsdf_decode_latent_supported(C.byref(broken)) == -1 and b"in_dim" in lib.dsdf_last_error()
    # an xyz_in_all net's d/d(xyz) scratch rows hold 4 floats: more geometry columns are refused, on both sides of the ABI
    x5 = NetSpec(8, [64, 64], 4, xyz_in_all=True).c_struct()
    x5.geom_dim, x5.in_dim[0] = 5, 13
    x5.in_dim[1], x5.out_dim[0] = 64, 59
    assert lib.dsdf_packed_floats(C.byref(x5), C.byref(n)) == -1 and b"xyz_in_all needs geom_dim" in lib.dsdf_last_error()
    with pytest.raises(NotImplementedError, match="geom_dimension <= 4"):
        NetSpec(8, [64, 64], 5, xyz_in_all=True)
    # gemm_split: widths <= 512, not together with the bf16 forward or the layer-by-layer variants; its planes enlarge `packed`
    sp = NetSpec(8, [64, 64], 3, gemm_split=True).c_struct()
    plain = NetSpec(8, [64, 64], 3, gemm_split=False).c_struct()
    n2 = C.c_int64()
    assert lib.dsdf_packed_floats(C.byref(sp), C.byref(n)) == 0 and lib.dsdf_packed_floats(C.byref(plain), C.byref(n2)) == 0
    assert n.value > n2.value
    sp.fwd_bf16 = 1                      # together with the bf16 forward: allowed (the backward chain is the split one)
    assert lib.dsdf_packed_floats(C.byref(sp), C.byref(n)) == 0
    sp.fwd_bf16, sp.latent_dropout = 0, 1
    assert lib.dsdf_packed_floats(C.byref(sp), C.byref(n)) == -1 and b"gemm_split" in lib.dsdf_last_error()
    with pytest.raises(NotImplementedError):
        NetSpec(8, [640, 640], 3, gemm_split=True)
    with pytest.raises(NotImplementedError):
        NetSpec(8, [64, 64], 3, gemm_split=True, latent_dropout=True)


def test_warm_own_code_bound_is_inside_the_text_section(tmp_path):
    """common.hpp warm_own_code reads the kernel's own instructions as data, clamped to the address of
    dsdf_text_end_marker.  Pinned here on the gfx950 code object inside libdsdf_hip.so: the marker lies INSIDE .text (no read
    can leave the section) and BEHIND every kernel that warms itself (so each of them has room to cover its own code)."""
    import re
    import shutil
    import subprocess
    from deepsdf_amd.build import LIB
    llvm = "/opt/rocm/lib/llvm/bin"
    tools = {t: os.path.join(llvm, t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    if not all(os.path.exists(p) for p in tools.values()) or not os.path.exists(LIB):
        pytest.skip("ROCm LLVM tools or the built library are not available")
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "co.elf")
    subprocess.run([tools["llvm-objcopy"], "-O", "binary", "--only-section=.hip_fatbin", LIB, fat], check=True)
    subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    sec = subprocess.run([tools["llvm-readelf"], "-SW", co], capture_output=True, text=True, check=True).stdout
    m = re.search(r"\.text\s+PROGBITS\s+([0-9a-f]+)\s+[0-9a-f]+\s+([0-9a-f]+)", sec)
    text_lo, text_hi = int(m.group(1), 16), int(m.group(1), 16) + int(m.group(2), 16)
    syms = subprocess.run([tools["llvm-readelf"], "-sW", co], capture_output=True, text=True, check=True).stdout
    funcs = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            funcs[f[7]] = (int(f[1], 16), int(f[2]))
    marker = [v for k, v in funcs.items() if "dsdf_text_end_marker" in k]
    assert len(marker) == 1
    mk = marker[0][0]
    assert text_lo <= mk < text_hi
    warmers = [k for k in funcs if re.search(r"fused_(forward|backward|fwd_bwd)_kernel", k) and "bf16" not in k]
    assert len(warmers) == 3
    for k in warmers:
        addr, size = funcs[k]
        assert addr + size <= mk, (k, hex(addr + size), hex(mk))
    shutil.rmtree(str(tmp_path), ignore_errors=True)


def test_split_wait_window_of_the_dw_split_kernel_is_clean():
    """dwstream.hpp dw_block_split keeps all sixteen ds_read_b128 of a step in flight across compiler-scheduled code (asm statement
    1 ends without a wait, statement 2 is the lgkmcnt(0)).  Correct only if nothing in between touches their destination registers -- a
    register-allocation outcome, so it is checked on the gfx950 code object of the library that was just built (the build does the
    same and refuses a violating library), and the checker itself is checked on hand-made instruction streams."""
    from deepsdf_amd import asmcheck
    from deepsdf_amd.build import LIB
    reads = [("ds_read_b128", f"v[{16 + 4 * k}:{19 + 4 * k}], v1 offset:{1024 * k}") for k in range(16)]
    body = [("v_and_b32_e32", "v0, 0xffff0000, v16"), ("v_sub_f32_e32", "v1, v16, v0"), ("v_perm_b32", "v2, v20, v24, s5")]
    close = [("s_waitcnt", "lgkmcnt(0)")]
    ok = reads + [("s_waitcnt", "lgkmcnt(8)")] + body + close + [("v_mov_b32_e32", "v3, v48")]
    assert asmcheck.check_split_wait_windows(ok) == 1                     # reads of A registers (v16..v47) are fine; B = v48..v79
    for bad in (("v_mov_b32_e32", "v3, v50"), ("v_accvgpr_write_b32", "a7, v79"), ("v_pk_mul_f32", "v[4:5], v[78:79], v[8:9]"),
                ("scratch_store_dwordx4", "off, v[4:7], off offset:16"), ("v_mov_b32_e32", "v48, v3")):
        with pytest.raises(asmcheck.AsmHazard):
            asmcheck.check_split_wait_windows(reads + [("s_waitcnt", "lgkmcnt(8)")] + body + [bad] + close)
    with pytest.raises(asmcheck.AsmHazard):                                # a window that is never closed
        asmcheck.check_split_wait_windows(reads + [("s_waitcnt", "lgkmcnt(8)")] + body)
    # the woven block leaves all sixteen reads in flight: A registers (v16..v47) are protected too; MFMAs on other registers may run
    mf = ("v_mfma_f32_32x32x16_bf16", "a[0:15], v[100:103], v[104:107], a[0:15]")
    assert asmcheck.check_split_wait_windows(reads + [mf, ("v_sub_f32_e32", "v2, v3, v4")] + close) == 1
    with pytest.raises(asmcheck.AsmHazard):
        asmcheck.check_split_wait_windows(reads + [mf, ("v_and_b32_e32", "v0, 0xffff0000, v16")] + close)
    assert asmcheck.check_split_wait_windows(reads + close) == 0             # reads + wait in one statement: no window at all
    assert asmcheck.vgprs("a[0:15], v[4:7], v9, s[0:3], 0xff, v12 offset:16") == {4, 5, 6, 7, 9, 12}
    if not asmcheck.tools_available() or not os.path.exists(LIB):
        pytest.skip("ROCm LLVM tools or the built library are not available")
    assert asmcheck.check_library(LIB) >= 1


def test_bf16x8_kloop_never_reloads_the_sources_of_the_mfma_in_front():
    """fused_bf16x8.hpp runs two waves per SIMD; its first k-loop let the register allocator hand a ds_read / buffer_load the registers
    the MFMA straight in front of it reads as srcA / srcB, and 3 % of the rows differed from run to run (profiles/r02_lab_bf16x8_race.log;
    on the code object of that version, rebuilt from commit 5f67ff3: 24 + 22 such loads, profiles/r03_bf16x8_reuse_audit.log).  The
    rewritten loop keeps a full step of MFMAs between an MFMA and any load into its source registers -- a property of the EMITTED code,
    so it is measured there (the build does the same and refuses a library that violates it); the measure itself is checked on
    hand-made streams."""
    from deepsdf_amd import asmcheck
    from deepsdf_amd.build import LIB
    mk = lambda op, args, addr, target=None: dict(op=op, args=args, addr=addr, target=target)   # noqa: E731
    mf = lambda a, acc, sa, sb: mk("v_mfma_f32_32x32x16_bf16", f"v[{acc}:{acc + 15}], v[{sa}:{sa + 3}], v[{sb}:{sb + 3}], v[{acc}:{acc + 15}]", a)   # noqa: E731
    bad = [mf(0, 0, 100, 104), mk("ds_read_b128", "v[104:107], v9", 8)]                                     # reload right behind the reader
    assert asmcheck.mfma_src_reuse_distances(bad) == {1: 0}
    good = [mf(0, 0, 100, 104), mf(8, 16, 108, 112), mf(16, 32, 116, 120), mk("buffer_load_dwordx4", "v[100:103], v9, s[8:11], s2 offen", 24)]
    assert asmcheck.mfma_src_reuse_distances(good) == {3: 2}
    drained = [mf(0, 0, 100, 104), mk("v_readfirstlane_b32", "s3, v15", 8), mk("ds_read_b128", "v[104:107], v9", 16)]   # a VALU read of the result
    assert asmcheck.mfma_src_reuse_distances(drained) == {}
    loop = [mk("ds_read_b128", "v[104:107], v9", 0), mf(8, 0, 100, 104), mk("s_cbranch_scc1", "65533", 16, target=0)]  # across the back-edge
    assert asmcheck.mfma_src_reuse_distances(loop) == {0: 0} and asmcheck.mfma_src_reuse_distances(loop, fall_through_only=True) == {}
    assert asmcheck.mfma_src_reuse_distances(loop, edges="loops") == {0: 0}       # the build gate follows loop back-edges: the steady state
    # ... but not a FORWARD branch over a guarded step's MFMAs (the path only exists together with the guard that skips the load too)
    guarded = [mf(0, 0, 100, 104), mk("s_cbranch_vccnz", "2", 8, target=32), mf(16, 16, 108, 112), mf(24, 32, 116, 120),
               mk("ds_read_b128", "v[104:107], v9", 32)]
    assert asmcheck.mfma_src_reuse_distances(guarded, edges="loops") == {4: 2} and asmcheck.mfma_src_reuse_distances(guarded) == {4: 0}
    if not asmcheck.tools_available() or not os.path.exists(LIB):
        pytest.skip("ROCm LLVM tools or the built library are not available")
    worst, pairs = asmcheck.check_mfma_src_reuse(LIB, min_distance=2)
    assert worst is not None and worst >= 2 and pairs > 20


def test_same_code_tells_equal_instruction_streams_from_changed_ones():
    """asmcheck.same_code is how a refactor of the kernel sources is shown to leave the GPU's code alone: per function, mnemonic and
    operand text in order, with one mask -- the literal of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 (the PC-relative
    distance to data, which moves when code elsewhere changes size).  The comparison itself is checked on hand-made streams."""
    from deepsdf_amd import asmcheck
    from deepsdf_amd.build import LIB
    pc = lambda lo, hi: [("s_getpc_b64", "s[4:5]"), ("s_add_u32", f"s4, s4, {lo}"), ("s_addc_u32", f"s5, s5, {hi}")]   # noqa: E731
    body = [("s_load_dwordx2", "s[0:1], s[4:5], 0x0"), ("s_add_u32", "s6, s6, 0x1f38"), ("v_mov_b32_e32", "v3, v48"), ("s_endpgm", "")]
    a = {"k1": pc("0x1f38", "0") + body, "k2": body}
    assert asmcheck.same_streams(a, {n: list(x) for n, x in a.items()}) == ({"k1": (7, 7, None), "k2": (4, 4, None)}, [], [])
    moved = {"k1": pc("0x2a40", "1") + body, "k2": body}                         # only the masked literal differs
    assert asmcheck.same_streams(a, moved) == ({"k1": (7, 7, None), "k2": (4, 4, None)}, [], [])
    other_base = {"k1": [("s_getpc_b64", "s[4:5]"), ("s_add_u32", "s4, s6, 0x1f38"), ("s_addc_u32", "s5, s5, 0")] + body, "k2": body}
    assert asmcheck.same_streams(a, other_base)[0]["k1"] == (7, 7, 1)            # the mask covers the literal, not the registers
    bare = {"k1": pc("0x1f38", "0") + body, "k2": [body[0], ("s_add_u32", "s6, s6, 0x2a40")] + body[2:]}
    assert asmcheck.same_streams(a, bare)[0]["k2"] == (4, 4, 1)                  # ... and no s_add_u32 without the s_getpc_b64
    renamed = {"k1": pc("0x1f38", "0") + body[:2] + [("v_mov_b32_e32", "v3, v49")] + body[3:], "k2": body}
    assert asmcheck.same_streams(a, renamed) == ({"k1": (7, 7, 5), "k2": (4, 4, None)}, [], [])
    longer = {"k1": pc("0x1f38", "0") + body, "k2": body[:3] + [("s_nop", "0")] + body[3:]}
    assert asmcheck.same_streams(a, longer)[0]["k2"] == (4, 5, 3)
    assert asmcheck.same_streams(a, {"k1": a["k1"], "k2": body + [("s_nop", "0")]})[0]["k2"] == (4, 5, 4)   # a longer tail alone
    assert asmcheck.same_streams(a, {"k1": a["k1"], "k3": body}) == ({"k1": (7, 7, None)}, ["k2"], ["k3"])
    if asmcheck.tools_available() and os.path.exists(LIB):
        per, only_a, only_b = asmcheck.same_code(LIB, LIB)
        assert len(per) > 100 and not only_a and not only_b
        assert all(na == nb and na > 0 and diff is None for na, nb, diff in per.values())


# ---- workspace planners: red zones and the region table (dsdf_debug_ws_*; host code, no device) ------------------------------------
def _net_from_golden(kw):
    from deepsdf_amd.net import NetSpec
    return NetSpec(**kw).c_struct()


def _plan_table(lib, net, N, R, kind, seg, K, fr):
    from deepsdf_amd import _lib
    assert lib.dsdf_debug_ws_plan(C.byref(net), N, R, kind, seg, K, fr) == 0, lib.dsdf_last_error()
    return _lib.ws_regions()


@pytest.fixture()
def redzone(lib):
    """Sets a red zone for one test and ALWAYS puts 0 back (the setting is process-wide)."""
    def set_(g):
        assert lib.dsdf_debug_ws_redzone(g) == 0, lib.dsdf_last_error()
    yield set_
    assert lib.dsdf_debug_ws_redzone(0) == 0


def test_default_layout_equals_the_recorded_totals(lib, golden_dir):
    """Red zone 0: every size answer equals what the commit before the debug red zones answered (tests/golden/ws_totals.json,
    recorded by tests/golden/make_golden_ws_totals.py): the default layout did not move by a byte."""
    import json
    gold = json.load(open(os.path.join(golden_dir, "ws_totals.json")))
    assert lib.dsdf_debug_ws_redzone(0) == 0
    assert len(gold["cases"]) >= 150 and len(gold["mc"]) >= 5 and len(gold["msdf"]) >= 9
    nets = {name: _net_from_golden(kw) for name, kw in gold["nets"].items()}
    b, tri, ns = C.c_size_t(), C.c_size_t(), C.c_int32()
    for c in gold["cases"]:
        net = nets[c["net"]]
        assert lib.dsdf_workspace_bytes(C.byref(net), c["N"], c["R"], C.byref(b)) == 0 and b.value == c["train"], c
        assert lib.dsdf_workspace_bytes_buckets(C.byref(net), c["N"], c["R"], c["K"], C.byref(b)) == 0 and b.value == c["buckets"], c
        assert lib.dsdf_decode_workspace_bytes(C.byref(net), c["N"], C.byref(b)) == 0 and b.value == c["decode"], c
    for m in gold["mc"]:
        assert lib.dsdf_mc_workspace_bytes(*m["grid"], C.byref(b)) == 0 and b.value == m["bytes"], m
    for m in gold["msdf"]:
        assert lib.dsdf_msdf_plan(m["faces"], m["queries"], C.byref(tri), C.byref(b), C.byref(ns)) == 0
        assert (tri.value, b.value, ns.value) == (m["tri"], m["ws"], m["splits"]), m


def test_red_zones_add_one_guard_per_region_and_the_size_answers_cover_every_plan(lib, golden_dir, redzone):
    """Per plan: total(G) = total(0) + G x regions, offsets move by G x (regions in front).  dsdf_workspace_bytes / _buckets answer
    a maximum over the plans a launch can choose (segment mode on / off, 32- / 64-row workgroups): at least every one of them,
    with and without red zones -- that inequality is the contract the entry points' size checks rely on."""
    import json
    from deepsdf_amd import _lib
    gold = json.load(open(os.path.join(golden_dir, "ws_totals.json")))
    nets = {name: _net_from_golden(kw) for name, kw in gold["nets"].items()}
    b = C.c_size_t()
    for c in gold["cases"]:
        net, N, R, K = nets[c["net"]], c["N"], c["R"], c["K"]
        plans = [(_lib.WS_PLAN_TRAIN, seg, k, fr) for seg in (0, 1) for fr in (32, 64) for k in (2, K)]
        plans += [(_lib.WS_PLAN_DECODE, 0, 2, fr) for fr in (32, 64)] + [(_lib.WS_PLAN_DECODE_LATENT, 0, 2, 64)]
        base = {}
        for G in (0, 256, 1024):
            redzone(G)
            answers = {}
            for k in (2, K):
                assert lib.dsdf_workspace_bytes_buckets(C.byref(net), N, R, k, C.byref(b)) == 0
                answers[k] = b.value
            assert lib.dsdf_workspace_bytes(C.byref(net), N, R, C.byref(b)) == 0 and b.value == answers[2]
            assert lib.dsdf_decode_workspace_bytes(C.byref(net), N, C.byref(b)) == 0
            dec = b.value
            for p in plans:
                kind, seg, k, fr = p
                rows, total = _plan_table(lib, net, N, R, kind, seg, k, fr)
                if G == 0:
                    base[p] = (rows, total)
                    continue
                rows0, total0 = base[p]
                assert [(n, nb) for n, _, nb in rows] == [(n, nb) for n, _, nb in rows0], (c, p)
                assert [o for _, o, _ in rows] == [o + G * i for i, (_, o, _) in enumerate(rows0)], (c, p, G)
                if kind == _lib.WS_PLAN_DECODE_LATENT:      # (sized like dsdf_decode's buffer, with a floor of 16384 bytes)
                    own = rows[-1][1] + rows[-1][2] + G
                    assert len(rows) == 2 and total == max(_plan_table(lib, net, N, R, _lib.WS_PLAN_DECODE, 0, 2, fr)[1], 16384, own), (c, p, G)
                else:
                    assert total == total0 + G * len(rows), (c, p, G, total, total0, len(rows))
            for p in plans:                                   # the inequality, at this G (0 included)
                kind, seg, k, fr = p
                _, total = _plan_table(lib, net, N, R, kind, seg, k, fr)
                if kind == _lib.WS_PLAN_TRAIN:
                    assert answers[k] >= total, (c, p, G)
                elif kind == _lib.WS_PLAN_DECODE:
                    assert dec >= total, (c, p, G)
                else:
                    assert lib.dsdf_decode_workspace_bytes(C.byref(net), max(N, 64), C.byref(b)) == 0
                    assert max(b.value, 16384) >= total, (c, p, G)
            if G == 0:                                        # and the maximum is attained: the answer is not padded beyond its plans
                assert answers[2] == max(t for (kind, _, k, _), (_, t) in base.items() if kind == _lib.WS_PLAN_TRAIN and k == 2)
    for m in gold["mc"]:
        tot = {}
        for G in (0, 256):
            redzone(G)
            assert lib.dsdf_mc_workspace_bytes(*m["grid"], C.byref(b)) == 0
            rows, tot[G] = _lib.ws_regions()
            assert tot[G] == b.value and len(rows) == 7
        assert tot[256] == tot[0] + 256 * 7
    for m in gold["msdf"]:
        tot = {}
        for G in (0, 512):
            redzone(G)
            assert lib.dsdf_msdf_plan(m["faces"], m["queries"], None, C.byref(b), None) == 0
            rows, tot[G] = _lib.ws_regions()
            assert tot[G] == b.value and [r[0] for r in rows] == ["msdf_partials"] and rows[0][2] == m["ws"]
        assert tot[512] == tot[0] + 512


def test_region_tables_of_the_whole_gpu_sweep(lib, redzone):
    """Every plan a case of tests/test_gpu_workspace.py can launch with, laid out on the host by the SAME make_plan: offsets
    256-aligned and in layout order, regions disjoint with at least the red zone between them, last end + red zone <= total,
    names unique, and the size answer the GPU test allocates covers the plan."""
    from deepsdf_amd import _lib
    from tests import test_gpu_workspace as T
    from tests.ws_guard import table_problems
    n_plans = 0
    for G in (0, 256):
        redzone(G)
        sizes = {}
        for c in T.CASES:
            net = T.spec_of(c.net).c_struct()
            key = (c.net, c.entry if c.entry in ("decode", "decode_latent") else c.entry in T.MODULE, c.N, c.R, c.K)
            if key in sizes:
                continue
            sizes[key] = c.ws_query(lib, net)
            for kind, N, R, seg, K, fr in c.plans():
                rows, total = _plan_table(lib, net, N, R, kind, seg, K, fr)
                assert not table_problems(rows, total, G), (c.id, kind, seg, K, fr, table_problems(rows, total, G))
                assert total <= sizes[key], (c.id, kind, seg, K, fr)
                n_plans += 1
        for shape, _ in T.MC_GRIDS:
            b = C.c_size_t()
            assert lib.dsdf_mc_workspace_bytes(*shape, C.byref(b)) == 0
            rows, total = _lib.ws_regions()
            assert not table_problems(rows, total, G) and total == b.value
        for nf, nq in T.MSDF_CASES:
            b = C.c_size_t()
            assert lib.dsdf_msdf_plan(nf, nq, None, C.byref(b), None) == 0
            rows, total = _lib.ws_regions()
            assert not table_problems(rows, total, G) and total == b.value
    assert n_plans > 2000


def test_break_point_value_sweep_lists_what_it_must():
    """The conditions of tests/test_gpu_breakpoints.py's case list (not measurements): both product nets at v - 1, v, v + 1 of every
    threshold and at every BIG_N, every R of R_VALUES, many short segments, every entry point, every family of the workspace sweep
    (or a stated reason), every segment shape of the sweep; every group reaches the one test that runs it; the pinned table of restated bf16 bounds is well-formed."""
    import inspect
    from collections import Counter
    from tests import test_gpu_breakpoints as B
    from tests import test_gpu_workspace as T
    per = Counter(g.tier for g in B.GROUPS)
    n_launch = sum(len(g.launches) for g in B.GROUPS)
    print(f"\nbreak-point value sweep: {len(B.GROUPS)} oracle runs {dict(per)}, {n_launch} (net, entry) pairs")
    for net in B.PRODUCT_NETS:
        mine = [g for g in B.GROUPS if g.tier == 1 and g.onet == net]
        ns = {g.N for g in mine}
        for name, v in T.thresholds().items():
            assert {v - 1, v, v + 1} <= ns | {0}, (net, name)
        assert set(T.BIG_N) <= ns and set(T.n_values()) <= ns, net
        assert {g.R for g in mine} >= set(T.R_VALUES), net
        assert any(g.R >= 2000 and g.R > g.N / 32 for g in mine), net
        for g in mine:                                   # the full product: these entries at EVERY N
            assert {"fb", "step", "decode", "decode_latent"} <= {e for n, e in g.launches if n == net}, g.id
        for v in T.thresholds().values():                # ... and the rest exactly one above every threshold
            g = next(g for g in mine if g.N == v + 1)
            want = set(B.ENTRIES) - (set() if T._fused(net) else {"phase2", "phase4"})
            assert want <= {e for n, e in g.launches if n == net}, g.id
    nets = {n for g in B.GROUPS for n, _ in g.launches}
    assert set(B.EXCLUDED) == {"L0"} and all(B.EXCLUDED.values())
    assert nets | set(B.EXCLUDED) == set(T.NETS) and not nets & set(B.EXCLUDED)
    assert {e for g in B.GROUPS for _, e in g.launches} == set(B.ENTRIES)
    for net in B.SEGMENT_NETS:                           # section 3 of the sweep, shape by shape
        mine = {g.lens for g in B.GROUPS if g.onet == net and ("fb" in {e for n, e in g.launches if n == net})}
        for lens in [(sl,) * R for R, sl in T.SEG_RS] + [tuple(l) for l in T.SEG_GENERAL]:
            assert lens in mine or (net == "fused_8x512" and sum(lens) > T.thresholds()["last_blocks"]), (net, lens[:4])
    for g in B.GROUPS:
        assert sum(g.lens) == g.N and len(g.lens) == g.R and g.launches and g.onet not in B.EXCLUDED
    # every group belongs to exactly one parametrisation of the one test, whose body runs all of its groups and all of their launches
    assert sorted(B.TESTS) == sorted({(g.tier, g.onet) for g in B.GROUPS}) and len(set(B.TESTS)) == len(B.TESTS)
    # the restated bf16 bounds name groups and quantities that exist, on bf16 nets only, and no spread can widen one at run time
    gids = {g.id for g in B.GROUPS if B.NETS[g.onet][1].get("forward_bf16")}
    for (gid, q), d in B.BF16_RESTATED.items():
        assert gid in gids and q in B.QUANTITIES and 0 < d < 0.02, (gid, q, d)
    src = inspect.getsource(B)
    for word in ("skip", "xfail", "importorskip"):       # nothing in the module can skip or xfail a case
        assert "pytest." + word not in src and "mark." + word not in src


def test_safe_batch_takes_explicit_segment_lengths_and_draws_what_it_drew_before():
    """tests/safe_batch.py: (a) three calls of the builder's earlier form (equal segments; 2-D geometry; rows of a larger table) give
    the tensors they gave before it took `lens` (SHA-256 of idx | xyz | gt, pinned on the earlier code); (b) lens = [S] * B is that same
    batch; (c) ragged lengths sum to N, every segment reads the row `scenes` names, and the result is margin-safe by the oracle."""
    import hashlib
    import math
    import torch
    from oracle import deepsdf_oracle as orc
    from tests.safe_batch import big_batch, safe_batch
    from tests.test_gpu_parity import SEG_SHAPES

    def digest(*ts):
        m = hashlib.sha256()
        for t in ts:
            m.update(t.contiguous().numpy().tobytes())
        return m.hexdigest()

    def state(name):
        c = SEG_SHAPES[name]
        net = orc.make_net(c["L"], **c["net"])
        params = orc.init_params(net, 31)
        lat0 = torch.randn(c["B"], c["L"], generator=torch.Generator().manual_seed(32)) / math.sqrt(c["L"])
        lat0[-1] *= 1.7 / lat0[-1].norm()
        return net, orc.TrainState.create({k: v.double() for k, v in params.items()}, lat0.double()), c["B"], c["S"], c["net"]["geom_dimension"]

    net, st, B, S, G = state("skip2_w64")
    a = safe_batch(net, st, B, S, 500, 0.1, 1.0, 77, G=G)
    assert digest(*a) == "1ae796386144c98516ddc663ee36447eceaba3af0e6b083adce377eb0db47570"
    b = safe_batch(net, st, None, None, 500, 0.1, 1.0, 77, G=G, lens=[S] * B)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    net, st, B, S, G = state("geom2_plain")
    assert digest(*safe_batch(net, st, B, S, 500, 0.1, 1.0, 77, G=G)) == "774d94455d792cc98f5e4b338a57be027b254aa0c6e6b4bccdf0a32106edff51"
    net, st, B, S, G = state("noskip_w40_L6_drop")
    st.latents = torch.cat([st.latents, st.latents * 0.5, st.latents * 0.25])
    scenes = torch.tensor([4, 1])
    assert digest(*safe_batch(net, st, B, S, 950, 0.1, 1.0, 7, scenes=scenes)) == "4f63a4083fd6bfb0163ddb459c2f80afe44fa8be2234d4934f0ac8e880fc2d20"
    # ragged lengths through a permuted scenes vector into the 6-row table, one row in use above code_bound
    lens, scenes = [1, 63, 64, 65, 7], torch.tensor([5, 0, 3, 2, 4])
    st.latents[3] *= 1.7 / st.latents[3].norm()
    idx, xyz, gt = safe_batch(net, st, None, None, 11, 0.1, 1.0, 77, G=G, scenes=scenes, lens=lens)
    assert idx.numel() == xyz.shape[0] == gt.shape[0] == sum(lens) and xyz.shape[1] == G
    assert torch.equal(torch.unique_consecutive(idx, return_counts=True)[1], torch.tensor(lens))
    assert torch.equal(torch.unique_consecutive(idx), scenes)
    lat = st.latents.clone()
    orc.renorm_rows_(lat, idx, 1.0)
    y, sv = orc.decoder_forward(net, st.params, torch.cat([lat[idx], xyz.double()], 1), training=True, masks=orc.dropout_masks(net, 77, 0, sum(lens)),
                                track_margin=True)
    d = torch.clamp(y, -0.1, 0.1) - torch.clamp(gt.double(), -0.1, 0.1)
    assert float(sv.min_abs_pre.min()) >= 1e-6 and not bool((((y.abs() - 0.1).abs() < 2e-5) | ((d != 0) & (d.abs() < 2e-5))).any())
    assert big_batch(None, None, 3, lens=[2, 5])[0].tolist() == [0, 0, 1, 1, 1, 1, 1]
    with pytest.raises(RuntimeError, match="margin-safe"):     # a margin nothing can meet: it raises, it never returns an unsafe batch
        safe_batch(net, st, None, None, 11, 0.1, 1.0, 77, G=G, scenes=scenes, lens=lens, relu_margin=1e3)


def test_debug_entries_check_their_arguments(lib, redzone):
    from deepsdf_amd import _lib
    from deepsdf_amd.net import NetSpec
    for bad in (-256, 1, 100, 255, 257, _lib.WS_MAX_REDZONE + 256):
        assert lib.dsdf_debug_ws_redzone(bad) == -1 and b"multiple of 256" in lib.dsdf_last_error(), bad
    net = NetSpec(8, [32] * 4, 3, latent_in=[2]).c_struct()
    b0, b1 = C.c_size_t(), C.c_size_t()
    assert lib.dsdf_workspace_bytes(C.byref(net), 1000, 4, C.byref(b0)) == 0          # a refused setting changed nothing
    redzone(_lib.WS_MAX_REDZONE)
    assert lib.dsdf_workspace_bytes(C.byref(net), 1000, 4, C.byref(b1)) == 0 and b1.value > b0.value
    redzone(0)
    assert lib.dsdf_workspace_bytes(C.byref(net), 1000, 4, C.byref(b1)) == 0 and b1.value == b0.value
    for args in ((-1, 4, 0, 0, 2, 64), (1000, -1, 0, 0, 2, 64), (1000, 4, 3, 0, 2, 64), (1000, 4, 0, 0, 9, 64), (1000, 4, 0, 0, 2, 48),
                 (1000, 4, 0, 0, -1, 64)):
        assert lib.dsdf_debug_ws_plan(C.byref(net), *args) == -1, args
    assert lib.dsdf_debug_ws_plan(None, 1000, 4, 0, 0, 2, 64) == -1
    assert lib.dsdf_debug_ws_plan(C.byref(net), 1000, 4, _lib.WS_PLAN_TRAIN, 1, 2, 32) == 0
    n, total = C.c_int32(), C.c_size_t()
    assert lib.dsdf_debug_ws_regions(None, 0, None, None) == -1 and b"n_regions" in lib.dsdf_last_error()
    assert lib.dsdf_debug_ws_regions(None, 0, C.byref(n), C.byref(total)) == 0 and n.value > 20 and total.value > 0    # NULL table: the count
    assert lib.dsdf_debug_ws_regions(None, 0, C.byref(n), None) == 0
    small = (_lib.DsdfWsRegion * (n.value - 1))()
    for r in small:
        r.offset = 77
    n2 = C.c_int32()
    assert lib.dsdf_debug_ws_regions(small, n.value - 1, C.byref(n2), None) == -1 and n2.value == n.value     # too small: refused,
    assert all(r.offset == 77 for r in small) and b"regions" in lib.dsdf_last_error()                        # nothing written
    exact = (_lib.DsdfWsRegion * n.value)()
    assert lib.dsdf_debug_ws_regions(exact, n.value, C.byref(n2), C.byref(total)) == 0
    names = [r.name.decode() for r in exact]
    assert names[0] == "in0" and "part" in names and "hoistU" in names and "dwslab3" in names and exact[-1].offset + exact[-1].bytes <= total.value
    rows, tot = _lib.ws_regions()
    assert [r[0] for r in rows] == names and tot == total.value
    # dsdf_debug_packed_layout: NULL arguments and an invalid net are refused and write nothing; a valid net's total is dsdf_packed_floats'
    lay = _lib.DsdfPackedLayout()
    lay.total = 77
    assert lib.dsdf_debug_packed_layout(None, C.byref(lay)) == -1 and lib.dsdf_debug_packed_layout(C.byref(net), None) == -1
    bad = NetSpec(8, [32] * 4, 3, latent_in=[2]).c_struct()
    bad.in_dim[2] += 1
    assert lib.dsdf_debug_packed_layout(C.byref(bad), C.byref(lay)) == -1 and b"in_dim" in lib.dsdf_last_error() and lay.total == 77
    nf = C.c_int64()
    assert lib.dsdf_debug_packed_layout(C.byref(net), C.byref(lay)) == 0 and lib.dsdf_packed_floats(C.byref(net), C.byref(nf)) == 0
    assert lay.total == nf.value and lay.w_off[0] == 0 and lay.ldw[0] == 32 and lay.w_off[net.n_layers] == -1
    assert lay.scale_off + sum(net.out_dim[l] for l in range(net.n_layers)) <= lay.wf_off[0] < lay.total


def test_latent_size_zero_never_reaches_segment_mode(lib):
    """validate() accepts latent_size == 0 (the general inference path takes such a net).  The hoist kernel of segment mode clamps
    its loads to column latent_size - 1: every way into it must refuse L = 0 on the host, before anything is launched."""
    from deepsdf_amd import _lib
    from deepsdf_amd.net import NetSpec
    net = NetSpec(0, [32, 32, 32], 3).c_struct()
    b = C.c_size_t()
    assert lib.dsdf_workspace_bytes(C.byref(net), 256, 4, C.byref(b)) == 0 and b.value > 0        # sizes: fine
    assert lib.dsdf_decode_workspace_bytes(C.byref(net), 256, C.byref(b)) == 0
    assert lib.dsdf_decode_latent_supported(C.byref(net)) == 0
    dummy = C.c_void_p(4096)                                    # never dereferenced: the argument checks come first
    batch = _lib.DsdfBatch(4096, 4096, 4, 4096, 4096, 256, 256, 0, 64)                           # 4 equal segments of 64: segment-mode shaped
    cfg = _lib.DsdfLossCfg()
    cfg.clamp_dist, cfg.training = 0.1, 1
    rc = lib.dsdf_train_forward_backward(C.byref(net), dummy, dummy, dummy, 4, C.byref(batch), C.byref(cfg), dummy, dummy, dummy, None, 0,
                                         dummy, 1 << 30, None)
    assert rc == -1 and b"latent_size > 0" in lib.dsdf_last_error()
    adam = _lib.DsdfAdamCfg(1, 5e-4, 1e-3, 0.9, 0.999, 1e-8, None)
    rc = lib.dsdf_train_step(C.byref(net), dummy, dummy, dummy, dummy, dummy, dummy, 4, dummy, dummy, dummy, C.byref(batch), C.byref(cfg),
                             C.byref(adam), dummy, None, dummy, 1 << 30, None)
    assert rc == -1 and b"latent_size > 0" in lib.dsdf_last_error()
    rc = lib.dsdf_decode_latent(C.byref(net), dummy, dummy, dummy, dummy, 256, dummy, dummy, 1 << 30, None)
    assert rc == -1 and b"dsdf_decode_latent needs" in lib.dsdf_last_error()


# ---- the opening of the decoder entry points: which error an invalid call gets --------------------------------------------------
# One argument list per ABI name, valid but for what a row overrides.  Pointers are never dereferenced: every row fails on the host
# (or is the n == 0 no-op).
_OPEN_N, _OPEN_R = 128, 2
_OPEN_ARGS = {
    "dsdf_decode": "net packed params input ld_in n sdf_out ws ws_bytes stream",
    "dsdf_decode_latent": "net packed params latent xyz n sdf_out ws ws_bytes stream",
    "dsdf_module_forward": "net packed params input ld_in n training dropout_key sdf_out ws ws_bytes stream",
    "dsdf_module_backward": "net packed params d_sdf n training dropout_key grads accumulate d_input ld_din ws ws_bytes stream",
    "dsdf_module_input_grad": "net packed params d_sdf n d_input ld_din ws ws_bytes stream",
    "dsdf_module_jvp": "net packed params tangent ld_t n training dropout_key jvp_out ws ws_bytes stream",
    "dsdf_train_forward_backward": "net packed params latent_table n_scenes b cfg grads dlat loss_out sdf_out accumulate ws ws_bytes "
                                   "stream",
    "dsdf_train_step": "net packed params grads exp_avg exp_avg_sq latent_table n_scenes dlat lat_exp_avg lat_exp_avg_sq b cfg adam "
                       "loss_out sdf_out ws ws_bytes stream",
}
_OPEN_INTS = {"ld_in": 16, "ld_din": 16, "ld_t": 16, "n": _OPEN_N, "training": 0, "accumulate": 0, "n_scenes": 4, "ws_bytes": 1 << 30}
_WS = "workspace {got} < {need} bytes"      # a -2 row's message; the test says what `need` is compared with
_NULL3 = "NULL packed/params/workspace pointer"
_ALIGN = "packed/params must be 16-byte and workspace 256-byte aligned"
_PHASE = "dw_phase needs the fused kernels (dsdf_dw_phase_supported), a trainable decoder, accumulate = 0 and the two-call path"
_LATENT = "dsdf_decode_latent needs the fused forward (widths <= 512, geom_dim <= 4): use dsdf_decode"
_DECODERS = ("dsdf_decode", "dsdf_decode_latent", "dsdf_module_forward", "dsdf_module_backward", "dsdf_module_input_grad",
             "dsdf_module_jvp", "dsdf_train_forward_backward")
_OWN = {"dsdf_decode": "bad input/sdf_out/ld_in", "dsdf_decode_latent": "bad latent/xyz/sdf_out",
        "dsdf_module_forward": "bad input/sdf_out/ld_in", "dsdf_module_backward": "bad d_sdf/grads",
        "dsdf_module_input_grad": "input gradient: -1 rows", "dsdf_module_jvp": "bad tangent/jvp_out/ld_t",
        "dsdf_train_forward_backward": "empty batch (n_points -1, n_segments 2)"}
# the data pointer whose NULL is the entry's own fault, and its message
_OWN_NULL = {"dsdf_decode": ("input", "bad input/sdf_out/ld_in"), "dsdf_decode_latent": ("xyz", "bad latent/xyz/sdf_out"),
             "dsdf_module_forward": ("sdf_out", "bad input/sdf_out/ld_in"), "dsdf_module_backward": ("d_sdf", "bad d_sdf/grads"),
             "dsdf_module_input_grad": ("d_sdf", "input gradient: NULL d_sdf or d_input"),
             "dsdf_module_jvp": ("jvp_out", "bad tangent/jvp_out/ld_t"), "dsdf_train_forward_backward": ("dlat", "NULL argument")}
_SMALL_LD = {"dsdf_decode": ("ld_in", "bad input/sdf_out/ld_in"), "dsdf_module_forward": ("ld_in", "bad input/sdf_out/ld_in"),
             "dsdf_module_backward": ("ld_din", "ld_din too small"), "dsdf_module_input_grad": ("ld_din", "ld_din too small"),
             "dsdf_module_jvp": ("ld_t", "bad tangent/jvp_out/ld_t")}
# (kind, segment mode, buckets, rows per workgroup) of the plan each entry lays out for the default call: dsdf_debug_ws_plan's arguments
_OPEN_PLAN = {"dsdf_decode": (1, 0, 2, 32), "dsdf_decode_latent": (2, 0, 2, 32), "dsdf_module_forward": (0, 0, 2, 64),
              "dsdf_module_backward": (0, 0, 2, 64), "dsdf_module_input_grad": (0, 0, 2, 64), "dsdf_module_jvp": (0, 0, 2, 64),
              "dsdf_train_forward_backward": (0, 0, 0, 32), "dsdf_train_step": (0, 0, 0, 32)}


def _open_rows():
    """(id, ABI name, net keywords, environment, overrides, rc, message).  Overrides: argument name -> value; "b.<field>" /
    "cfg.<field>" / "adam.<field>" set a field of the training structs."""
    rows = []

    def row(name, what, over, rc, msg, net=None, env=None):
        rows.append((f"{name[5:]}-{what}", name, net or {}, env or {}, over, rc, msg))

    for e in _DECODERS:
        train = e == "dsdf_train_forward_backward"
        nkey = "b.n_points" if train else "n"
        row(e, "null-net", {"net": None}, -1, "net is NULL")
        for p in ("packed", "params", "ws"):
            row(e, f"null-{p}", {p: None}, -1, _NULL3)
        row(e, "misaligned-ws", {"ws": 256 + 64}, -1, _ALIGN)
        row(e, "misaligned-params", {"params": 256 + 8}, -1, _ALIGN)
        row(e, "negative-n", {nkey: -1}, -1, _OWN[e])
        if e in _SMALL_LD:
            row(e, "small-ld", {_SMALL_LD[e][0]: 10}, -1, _SMALL_LD[e][1])          # in_dim[0] = 11
        row(e, "small-ws", {"ws_bytes": 0}, -2, _WS)
        row(e, "ws-one-byte-short", {"ws_bytes": -1}, -2, _WS)                       # -1: the plan's size less one
        own_ptr, own_msg = _OWN_NULL[e]
        row(e, "null-data", {own_ptr: None}, -1, own_msg)
        # n == 0: nothing to do, whatever the data pointers -- but only behind the shared checks; an empty training batch is an error
        nulls = {k: None for k in _OPEN_ARGS[e].split() if k in ("input", "latent", "xyz", "sdf_out", "d_sdf", "grads", "d_input",
                                                                    "tangent", "jvp_out", "dropout_key")}
        if train:
            row(e, "empty", {nkey: 0}, -1, "empty batch (n_points 0, n_segments 2)")
        else:
            row(e, "n0-null-data", dict(nulls, n=0), 0, None)
            row(e, "n0-small-ws", dict(nulls, n=0, ws_bytes=0), 0, None)
            row(e, "n0-null-packed", dict(nulls, n=0, packed=None), -1, _NULL3)
        # two faults at once: the shared check before the entry's own, the entry's own before the size
        shared_first = "input gradient: -1 rows" if e == "dsdf_module_input_grad" else _NULL3   # (its wrapper looks at n first)
        row(e, "shared-vs-own", {"packed": None, nkey: -1}, -1, shared_first)
        row(e, "net-vs-own", {"net": None, own_ptr: None}, -1, own_msg if e == "dsdf_module_input_grad" else "net is NULL")
        row(e, "own-vs-size", {own_ptr: None, "ws_bytes": 0}, -1, own_msg)
    # dropout keys: the module entries want them when they will hash
    row("dsdf_module_forward", "null-key", {"training": 1, "dropout_key": None}, -1, "dropout_key is NULL",
        net=dict(dropout=[0, 1], dropout_prob=0.2))
    row("dsdf_module_forward", "null-key-vs-size", {"training": 1, "dropout_key": None, "ws_bytes": 0}, -1, "dropout_key is NULL",
        net=dict(dropout=[0, 1], dropout_prob=0.2))
    row("dsdf_module_backward", "null-key", {"training": 1, "dropout_key": None}, -1,
        "dropout_key is NULL (latent_dropout needs the forward's key for d/d(input))", net=dict(latent_dropout=True))
    row("dsdf_module_jvp", "null-key", {"training": 1, "dropout_key": None}, -1,
        "dropout_key is NULL (latent_dropout needs the forward's key)", net=dict(latent_dropout=True))
    row("dsdf_module_backward", "null-grads-vs-ld", {"grads": None, "ld_din": 10}, -1, "bad d_sdf/grads")
    # training
    t = "dsdf_train_forward_backward"
    row(t, "null-batch", {"b": None}, -1, "NULL argument")
    row(t, "null-cfg", {"cfg": None}, -1, "NULL argument")
    row(t, "null-batch-vs-packed", {"b": None, "packed": None}, -1, _NULL3)
    row(t, "no-segments", {"b.n_segments": 0}, -1, "empty batch (n_points 128, n_segments 0)")
    row(t, "no-scenes", {"n_scenes": 0}, -1, "empty batch (n_points 128, n_segments 2)")
    row(t, "null-batch-pointer", {"b.sdf_gt": None}, -1, "NULL batch pointer")
    row(t, "n-norm", {"b.n_norm": 0}, -1, "n_norm must be positive")
    row(t, "empty-vs-n-norm", {"b.n_points": 0, "b.n_norm": 0}, -1, "empty batch (n_points 0, n_segments 2)")
    row(t, "latent-size-0", {}, -1, "training needs latent_size > 0", net=dict(latent_size=0))
    row(t, "n-norm-vs-latent-size-0", {"b.n_norm": -3}, -1, "n_norm must be positive", net=dict(latent_size=0))
    for k in (-1, 9):
        row(t, f"buckets{k}", {"cfg.dw_buckets": k}, -1, f"dw_buckets {k} out of range [0, 8]")
    for k, p in ((0, 1), (1, 1), (2, 0), (2, 3), (2, -1), (8, 9)):
        row(t, f"buckets{k}-phase{p}", {"cfg.dw_buckets": k, "cfg.dw_phase": p}, -1,
            f"dw_phase {p} out of range for dw_buckets {k} (0 without buckets, 1..K with K >= 2)")
    row(t, "buckets-vs-phase", {"cfg.dw_buckets": 9, "cfg.dw_phase": -1}, -1, "dw_buckets 9 out of range [0, 8]")
    row(t, "phase-range-vs-size", {"cfg.dw_buckets": 2, "cfg.dw_phase": 3, "ws_bytes": 0}, -1,
        "dw_phase 3 out of range for dw_buckets 2 (0 without buckets, 1..K with K >= 2)")
    phased = {"cfg.dw_buckets": 2, "cfg.dw_phase": 1}
    row(t, "phase-accumulate", dict(phased, accumulate=1), -1, _PHASE)
    row(t, "phase2-accumulate", {"cfg.dw_buckets": 2, "cfg.dw_phase": 2, "accumulate": 1}, -1, _PHASE)
    row(t, "phase-frozen", dict(phased, **{"cfg.frozen_decoder": 1}), -1, _PHASE)
    row(t, "phase-accumulate-small-ws", dict(phased, accumulate=1, ws_bytes=0), -2, _WS)      # the size check comes first
    row(t, "phase-layered", phased, -1, _PHASE, env={"DSDF_NO_FUSED": "1"})
    row(t, "phase-layered-net", phased, -1, _PHASE, net=dict(xyz_in_all=True))
    s = "dsdf_train_step"
    row(s, "phase", phased, -1, _PHASE)
    row(s, "phase-small-ws", dict(phased, ws_bytes=0), -2, _WS)
    row(s, "null-adam", {"adam": None}, -1, "NULL argument")
    row(s, "null-adam-vs-net", {"adam": None, "net": None}, -1, "NULL argument")             # its wrapper's checks come first
    row(s, "adam-step-0", {"adam.step": 0}, -1, "Adam step must be >= 1")
    row(s, "null-net", {"net": None}, -1, "net is NULL")
    row(s, "null-batch", {"b": None}, -1, "NULL argument")
    row(s, "small-ws", {"ws_bytes": 0}, -2, _WS)
    # the single-code decode takes no layer-by-layer net; nets that exist in the fused kernels only, with those switched off
    row("dsdf_decode_latent", "layernorm", {}, -1, _LATENT, net=dict(norm_layers=[0, 1], weight_norm=False))
    row("dsdf_decode_latent", "layernorm-vs-size", {"ws_bytes": 0}, -1, _LATENT, net=dict(norm_layers=[0, 1], weight_norm=False))
    row("dsdf_decode_latent", "no-fused", {}, -1, _LATENT, env={"DSDF_NO_FUSED": "1"})
    for e in _DECODERS:
        for kw, flag in ((dict(gemm_split=True), "gemm_split"), (dict(forward_bf16=True), "fwd_bf16")):
            msg = f"{flag} exists only in the fused kernels (DSDF_NO_FUSED is set)"
            row(e, f"no-fused-{flag}", {}, -1, msg, net=kw, env={"DSDF_NO_FUSED": "1"})
            if e != "dsdf_module_input_grad":
                row(e, f"no-fused-{flag}-vs-null", {"packed": None}, -1, msg, net=kw, env={"DSDF_NO_FUSED": "1"})
    return rows


def _open_call(lib, name, net_kw, over):
    """Call `name` with the default arguments but `over`; returns (rc, message, the net)."""
    from deepsdf_amd import _lib
    from deepsdf_amd.net import NetSpec
    kw = dict(latent_size=8)
    kw.update(net_kw)
    net = NetSpec(kw.pop("latent_size"), [64, 64], 3, **kw).c_struct()
    dummy = 256
    batch = _lib.DsdfBatch(dummy, dummy, _OPEN_R, dummy, dummy, _OPEN_N, _OPEN_N, 0, 0)
    cfg = _lib.DsdfLossCfg()
    cfg.clamp_dist, cfg.training = 0.1, 1
    adam = _lib.DsdfAdamCfg(1, 5e-4, 1e-3, 0.9, 0.999, 1e-8, None)
    structs = {"net": net, "b": batch, "cfg": cfg, "adam": adam}
    for k, v in over.items():
        if "." in k:
            s, f = k.split(".")
            setattr(structs[s], f, v)
    args = []
    for a in _OPEN_ARGS[name].split():
        if a in over:
            v = over[a]
        elif a in structs:
            v = structs[a]
        elif a == "stream":
            v = None
        elif a == "dropout_key":
            v = (C.c_uint32 * 16)()
        else:
            v = _OPEN_INTS.get(a, dummy)
        args.append(C.byref(v) if isinstance(v, C.Structure) else v)
    rc = getattr(lib, name)(*args)
    return rc, (lib.dsdf_last_error().decode() if rc != 0 else None), net


@pytest.mark.parametrize("name,net_kw,env,over,rc,msg", [pytest.param(*r[1:], id=r[0]) for r in _open_rows()])
def test_invalid_calls_of_the_decoder_entries_get_the_same_answer(lib, monkeypatch, name, net_kw, env, over, rc, msg):
    """Return code AND message of the entry points that launch the decoder, for calls that never reach a launch: which check speaks
    first when two arguments are wrong is part of what a caller sees.  The literals were recorded from the library before the
    entry points got one shared opening.  Byte counts are not literals: the message's `need` must be the total of the plan the
    entry lays out for this call (dsdf_debug_ws_plan), which the size queries must cover (dsdf_decode_workspace_bytes: equal)."""
    from deepsdf_amd import _lib
    for k, v in env.items():
        monkeypatch.setenv(k, v)          # (the switches are read per call)
    if rc != -2:
        assert _open_call(lib, name, net_kw, over)[:2] == (rc, msg)
        return
    kind, seg, K, fr = _OPEN_PLAN[name]
    K = over.get("cfg.dw_buckets", K)
    R = _OPEN_R if "train" in name else 0
    net = _open_call(lib, name, net_kw, dict(over, net=None))[2]
    assert lib.dsdf_debug_ws_plan(C.byref(net), _OPEN_N, R, kind, seg, K, fr) == 0
    need = _lib.ws_regions()[1]
    cover = C.c_size_t()
    if kind == 0:
        assert lib.dsdf_workspace_bytes_buckets(C.byref(net), _OPEN_N, R, K, C.byref(cover)) == 0 and need <= cover.value
    else:
        assert lib.dsdf_decode_workspace_bytes(C.byref(net), _OPEN_N, C.byref(cover)) == 0
        assert need == (cover.value if kind == 1 else max(cover.value, 16384))
    got = need - 1 if over["ws_bytes"] == -1 else over["ws_bytes"]
    assert _open_call(lib, name, net_kw, dict(over, ws_bytes=got))[:2] == (-2, _WS.format(got=got, need=need))
