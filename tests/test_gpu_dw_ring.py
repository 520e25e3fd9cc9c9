"""-m gpu: the register ring of dw_item (csrc/dwstream.hpp) at every step count at which it changes shape, against the float64 oracle.

The ring prefetches DW_RING k-steps of two points; every load is unconditional and its step index clamped to the item's last step,
so the edge cases are STEP COUNTS of an item, nsteps = (kend - kbeg) >> 1: no step at all (the ring is skipped, the odd-point tail
does the work), fewer steps than slots (prologue and tail only), exactly one / two revolutions and one step either side of each.
A clamped load re-requests a step whose data must never reach an accumulator: the workspace is poisoned with 0xFF bytes (NaN as
floats) and every planner region is followed by a red zone (tests/ws_guard.py), so a "never used" load that WAS used shows as a
NaN gradient, and a load or store outside the regions as a damaged gap.

Shapes: batches below 128 points are ONE K-split (dw_schedule: at most N / 64 splits), so nsteps = N >> 1; 129 / 130 points are two
splits (66 + 63 / 66 + 64) and 4225 points of the 128-wide net 64 splits of 66 and a last one of ONE point.  Segment mode needs
segments of whole 32-point workgroups: there the step counts come from the last split of 13 ... 97 segments of 32 points.  The split count is
asserted on the plan the launch recorded; the launch itself on the profile's per-kernel counts.  In every case the batch's last
item ends at the last row of dP / act: behind it lie the planner's 4096 bytes of slack (poisoned) and the red zone.
Comparisons and tolerances are tests/test_gpu_breakpoints.py's (Truth, Launcher: GRAD_TOL norm-wise, GRAD_ELEM_TOL entry-wise, ...)."""
import ctypes as C
import os
import re

import pytest
import torch

from deepsdf_amd import _lib
from tests import test_gpu_breakpoints as B
from tests import test_gpu_workspace as W
from tests import ws_guard as G
from tests.test_gpu_parity import BIG

pytestmark = pytest.mark.gpu

DW_RING = int(re.search(r"#define\s+DW_RING_STEPS\s+(\d+)", open(os.path.join(G.ROOT, "deepsdf_amd", "csrc", "dwstream.hpp")).read()).group(1))
STEP_COUNTS = (0, 1, DW_RING - 2, DW_RING - 1, DW_RING, DW_RING + 1, 2 * DW_RING - 1, 2 * DW_RING, 2 * DW_RING + 1)
FILL = 0xFF

# name -> W.NETS row (latent size, NetSpec arguments, environment); registered in W.NETS for the duration of a test only
RING_NETS = {
    "n128_6x128": W.NETS["n128_6x128"],
    # two 512-wide hidden layers, the input fed in again at layer 1 (the headline net's skip layout): out_dim[0] = 512 - 19 = 493,
    # so the skip layer has a short last row tile as well
    "ring_2x512_skip": (16, dict(BIG, dims=[512, 512], dropout=[0, 1], norm_layers=[0, 1], latent_in=[1]), {}),
}


def split_points(N, ns0):
    """Points per K-split as dw_schedule (csrc/dsdf_api.hip) cuts a batch of N points when it aims at ns0 splits."""
    kchunk = max(2, -(-N // ns0) + (-(-N // ns0) & 1))
    return [min(N, k + kchunk) - k for k in range(0, N, kchunk)]


# (N, the split count dw_schedule aims at, segment length): min(waves / tiles, N / 64) splits -- 1 below 128 points whatever the net
# and the chip.  One segment of N points is segment mode only where N is a multiple of 32; the step counts a multiple of 32 cannot
# give to a single split come from the LAST split of batches of 32-point segments: kchunk = 66 or 70, 66 / 34 / 32 / 30 / 28 / 2 points
# left (no batch of whole 32-point segments leaves an odd split or a split of one point: those run on the general path only)
SMALL = [(max(1, 2 * v), 1, 0) for v in STEP_COUNTS] + [(3, 1, 0), (2 * DW_RING - 1, 1, 0), (4 * DW_RING + 1, 1, 0)]   # + odd last points
TWO_SPLITS = [(8 * DW_RING + 1, 2, 0), (8 * DW_RING + 2, 2, 0)]
SEGMENTS = [(32 * m, 32 * m // 64, 32) for m in (13, 65, 67, 69, 71, 97)] if DW_RING == 16 else []
CASES = {"n128_6x128": SMALL + TWO_SPLITS + SEGMENTS + [(65 * 65, 66, 0)], "ring_2x512_skip": SMALL + TWO_SPLITS + SEGMENTS}
SEG_STEP_COUNTS = (1, DW_RING - 2, DW_RING - 1, DW_RING, DW_RING + 1, 2 * DW_RING, 2 * DW_RING + 1)      # reached in SEGMENT mode too


def steps_of(cases, segmode=False):
    return {p >> 1 for N, ns0, sl in cases for p in split_points(N, ns0) if not segmode or (sl or N) % 32 == 0}


class GuardedLauncher(B.Launcher):
    """B.Launcher on a poisoned, red-zoned workspace, with the launch and its plan asserted after every forward + backward."""

    def fresh(self):
        eng, lat, dlat = super().fresh()
        b = C.c_size_t()
        _lib.check(eng.lib.dsdf_workspace_bytes(C.byref(eng.cnet), self.g.N, self.g.R, C.byref(b)))
        self.ws = eng._ws = G.poisoned(b.value, FILL)
        eng._ws_sizes = {}
        return eng, lat, dlat

    def fb(self, seg_len, mode, **kw):
        lib = _lib.lib()
        lib.dsdf_profile_enable(1)
        try:
            super().fb(seg_len, mode, **kw)
            prof = _lib.DsdfProfile()
            _lib.check(lib.dsdf_profile_read(C.byref(prof)))
        finally:
            lib.dsdf_profile_enable(0)
        w = self.where("fb", mode)
        count = dict(zip(_lib.PROF_NAMES, prof.count))
        assert count["dw_stream_kernel"] == 1 and count["gemm_tn_kernel"] == 0, f"{w}: not the dW stream launch: {count}"
        rows, _ = G.assert_clean(self.ws, FILL, w)
        reg = {name: nb for name, _, nb in rows}
        ns = {}
        for l in range(self.spec.n_layers - 1):        # slabs of layer l: nsplit x rup(out_l x ld_in_l, 64) floats; in_l: N x ld_in_l floats + 4096
            ld = (reg[f"in{l}"] - 4096) // (4 * self.g.N)
            assert (reg[f"in{l}"] - 4096) % (4 * self.g.N) == 0 and ld >= self.spec.in_dim[l]
            slab = 4 * (-(-self.spec.out_dim[l] * ld // 64) * 64)
            assert reg[f"dwslab{l}"] % slab == 0, f"{w}: dwslab{l}"
            ns[l] = reg[f"dwslab{l}"] // slab
        # (segment mode: layer 0 has no items and no slabs -- its gradient is the riding roles' work)
        assert set(ns.values()) - {0} == {len(self.pts)} and ns[self.spec.n_layers - 2] > 0, \
            f"{w}: the plan has {ns} K-splits per layer, the case was chosen for {len(self.pts)}"


def run_case(net, N, ns0, sl, book):
    g = B.Group(0, net, [sl] * (N // sl) if sl else [N])     # equal segments: segment mode (where the kernels take it) AND the general path
    t = B.Truth(g)
    L = GuardedLauncher(t, net, book)
    L.pts = split_points(N, ns0)
    with G.redzone():
        book.launches += L.run("fb")
    book.groups += 1


def test_the_case_list_reaches_every_step_count():
    for net, cases in CASES.items():
        assert set(STEP_COUNTS) <= steps_of(cases), (net, sorted(steps_of(cases)))
        assert set(SEG_STEP_COUNTS) <= steps_of(cases, segmode=True), (net, sorted(steps_of(cases, segmode=True)))
        assert {1, 2} <= {N for N, _, _ in cases}
        assert any(p & 1 for N, ns0, _ in cases for p in split_points(N, ns0))
    assert split_points(65 * 65, 66) == [66] * 64 + [1] and split_points(8 * DW_RING + 1, 2) == [4 * DW_RING + 2, 4 * DW_RING - 1]


@pytest.mark.parametrize("net", sorted(CASES))
def test_dw_ring_step_counts_vs_oracle_on_a_poisoned_workspace(net, monkeypatch):
    monkeypatch.setitem(W.NETS, net, RING_NETS[net])
    book = B.Book()
    try:
        for N, ns0, sl in CASES[net]:
            run_case(net, N, ns0, sl, book)
    finally:
        torch.cuda.empty_cache()
    print("\n" + book.report(f"dW ring, {net}, DW_RING = {DW_RING}: N = {[N for N, _, _ in CASES[net]]}"))
    assert book.launches == 2 * len(CASES[net])
    assert not book.fails, f"{len(book.fails)} of {book.n} comparisons miss their bound:\n" + "\n".join(book.fails[:40])
