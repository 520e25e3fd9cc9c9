"""The build-time audit of the fp32 dW ring (deepsdf_amd/asmcheck.py check_dw_ring_waits), on hand-written listings: no GPU.

dw_item<4> (csrc/dwstream.hpp) prefetches DW_RING k-steps of two loads each into registers.  Its steady-state loop is only worth
anything if no wait inside it empties the ring: every s_waitcnt that names vmcnt must leave >= 2 (DW_RING - 2) loads in flight, and
none may be vmcnt(0) -- the shape the loop had for four rounds (one vmcnt(0) at the header, the loads under scalar branches).  The
results are the same either way, so only the code object can tell; the build refuses a library that fails."""
import os

import pytest

from deepsdf_amd import asmcheck

RING = 16
SYM = "_ZN4dsdf16dw_stream_kernelENS_6DwArgsENS_11PostBwdArgsEii"
BASE = 0x1000


def listing(groups, pre=(), post=()):
    """llvm-objdump -d text: `pre`, then one loop (header .. backward s_cbranch_scc1) whose body is `groups` -- per group a tuple of
    lines in front of its 16 MFMAs -- then `post`."""
    lines, addr = [f"{BASE:016x} <{SYM}>:"], BASE

    def emit(text, tail=""):
        nonlocal addr
        lines.append(f"\t{text} // {addr:012X}: BF800000{tail}")
        addr += 8

    for t in pre:
        emit(t)
    head = addr
    for g in groups:
        for t in g:
            emit(t)
        for k in range(16):
            emit(f"v_mfma_f32_32x32x2_f32 a[{16 * k}:{16 * k + 15}], v{128 + k // 4}, v{132 + k % 4}, a[{16 * k}:{16 * k + 15}]")
    emit("s_cbranch_scc1 64000", f" <{SYM}+0x{head - BASE:x}>")
    for t in post:
        emit(t)
    return "\n".join(lines) + "\n"


LOAD_A, LOAD_B = "buffer_load_dwordx4 v[0:3], v14, s[4:7], s11 offen", "buffer_load_dwordx4 v[4:7], v15, s[8:11], s29 offen"
PROLOGUE = tuple(LOAD_A if k % 2 == 0 else LOAD_B for k in range(2 * (RING - 1)))


def test_a_rolling_ring_passes():
    """Two loads and one counted wait in front of every group of 16 MFMAs, as the shipped loop has them (vmcnt 28 / 29)."""
    groups = [(LOAD_A, LOAD_B, f"s_waitcnt vmcnt({28 + q % 2})") for q in range(RING)]
    ins = asmcheck.parse_listing(listing(groups, pre=PROLOGUE, post=("s_waitcnt vmcnt(0)", "s_endpgm")))
    assert asmcheck.check_dw_ring_waits_ins(ins, RING) == [28 + q % 2 for q in range(RING)]     # (the drain BEHIND the loop is no finding)
    # a wait that names only another counter is not the audit's business
    groups[3] = groups[3] + ("s_waitcnt lgkmcnt(0)",)
    assert len(asmcheck.check_dw_ring_waits_ins(asmcheck.parse_listing(listing(groups)), RING)) == RING


def test_a_drained_ring_is_refused():
    """The loop of the four silent rounds: one vmcnt(0) at the header, behind the revolution's first two loads; and near misses."""
    drained = [(LOAD_A, LOAD_B, "s_waitcnt vmcnt(0)")] + [(LOAD_A, LOAD_B)] * (RING - 1)
    with pytest.raises(asmcheck.AsmHazard, match=r"vmcnt\(0\)"):
        asmcheck.check_dw_ring_waits_ins(asmcheck.parse_listing(listing(drained, pre=PROLOGUE)), RING)
    with pytest.raises(asmcheck.AsmHazard, match=r"vmcnt\(0\)"):       # combined with another counter it is still a drain
        combined = [(LOAD_A, LOAD_B, "s_waitcnt vmcnt(0) lgkmcnt(0)")] + [(LOAD_A, LOAD_B, "s_waitcnt vmcnt(28)")] * (RING - 1)
        asmcheck.check_dw_ring_waits_ins(asmcheck.parse_listing(listing(combined)), RING)
    shallow = [(LOAD_A, LOAD_B, f"s_waitcnt vmcnt({27 if q == 5 else 28})") for q in range(RING)]      # one step too few in flight
    with pytest.raises(asmcheck.AsmHazard, match="28"):
        asmcheck.check_dw_ring_waits_ins(asmcheck.parse_listing(listing(shallow)), RING)
    # no loop of one revolution (here: of another ring depth) -- the audit must not pass vacuously
    with pytest.raises(asmcheck.AsmHazard, match="vacuous"):
        asmcheck.check_dw_ring_waits_ins(asmcheck.parse_listing(listing([(LOAD_A, LOAD_B, "s_waitcnt vmcnt(12)")] * 8)), RING)
    assert asmcheck.check_dw_ring_waits_ins(asmcheck.parse_listing(listing([(LOAD_A, LOAD_B, "s_waitcnt vmcnt(12)")] * 8)), 8) == [12] * 8


def test_the_built_library_keeps_its_ring_rolling():
    from deepsdf_amd.build import LIB
    if not asmcheck.tools_available() or not os.path.exists(LIB):
        pytest.skip("ROCm LLVM tools or the built library are not available")
    waits = asmcheck.check_dw_ring_waits(LIB, ring=RING)
    assert len(waits) >= RING and min(waits) >= 2 * (RING - 2)
