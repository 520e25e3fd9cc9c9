"""Byte-level memory-safety checks around calls into libdsdf_hip.so, with torch ops only (no check kernel, no sanitizer):

  redzone(G)          context: every planner region is followed by G unused bytes (dsdf_debug_ws_redzone); 0 again on exit
  poisoned(n, fill)   a workspace of n bytes + one red zone of tail, every byte = fill
  damage / assert_clean   after a call: every byte OUTSIDE the regions of the plan the call recorded (dsdf_debug_ws_regions:
                      red zones, the rounding padding behind a region, the tail) must still be `fill`; a damaged gap is reported
                      with the region in front of it and the offsets of its first and last changed byte
  Fences              caller-sized outputs as views into sentinel-filled tensors; check() compares the bytes around each view
  constants()         the planners' break points, parsed from the kernel sources (nothing is copied into the tests)
"""
import contextlib
import ctypes as C
import glob
import os
import re

import numpy as np
import torch

from deepsdf_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDZONE = 256          # bytes behind every region while a check runs
SENTINEL = 0xA5        # byte around caller-sized outputs
FENCE = 256            # bytes of sentinel in front of and behind an output (keeps the view 256-byte aligned)
SMALL_GAP = 1 << 16    # gaps up to this size are compared with ONE gather; larger ones (the tail of an over-sized buffer) as slices
CHUNK = 1 << 28


def constants():
    """{name: int} of every `constexpr int NAME = <integer>` in deepsdf_amd/csrc (also the `A = 1, B = 2` form)."""
    out = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "deepsdf_amd", "csrc", "*.h*"))):
        for decl in re.findall(r"constexpr\s+int\s+([^;]+);", open(path).read()):
            for name, val in re.findall(r"([A-Z][A-Z0-9_]*)\s*=\s*(\d+)\s*(?:,|$|/)", decl):
                out[name] = int(val)
    return out


def chip_cus():
    """Compute units the library plans for: the device's, or the MI355X's 256 without one (chip_waves() / 4 in dsdf_api.hip)."""
    if torch.cuda.is_available():
        return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    return 256


@contextlib.contextmanager
def redzone(g=REDZONE):
    lib = _lib.lib()
    _lib.check(lib.dsdf_debug_ws_redzone(g))
    try:
        yield g
    finally:
        _lib.check(lib.dsdf_debug_ws_redzone(0))


def poisoned(nbytes, fill, tail=REDZONE, device="cuda"):
    return torch.full((int(nbytes) + tail,), fill, dtype=torch.uint8, device=device)


def gaps(rows, size):
    """[(name of the region in front, start, end)] of every byte range of [0, size) that no region of `rows` covers."""
    out, cursor, prev = [], 0, "<start>"
    for name, off, nb in sorted(rows, key=lambda r: (r[1], r[2])):
        if off > cursor:
            out.append((prev, cursor, min(off, size)))
        if off + nb > cursor:
            cursor = off + nb
        prev = name
    if cursor < size:
        out.append((prev, cursor, size))
    return [g for g in out if g[2] > g[1]]


def damage(ws, fill, rows):
    """[(region in front of the gap, first changed byte, last changed byte)] over every gap of the uint8 tensor `ws`."""
    found = []
    gs = gaps(rows, ws.numel())
    small = [g for g in gs if g[2] - g[1] <= SMALL_GAP]
    if small:
        idx = np.concatenate([np.arange(a, b, dtype=np.int64) for _, a, b in small])
        owner = np.repeat(np.arange(len(small)), [b - a for _, a, b in small])
        bad = (ws[torch.from_numpy(idx).to(ws.device)] != fill).cpu().numpy()
        for k in np.unique(owner[bad]):
            pos = idx[bad & (owner == k)]
            found.append((small[k][0], int(pos.min()), int(pos.max())))
    for prev, a, b in gs:
        if b - a <= SMALL_GAP:
            continue
        first = last = None
        for c in range(a, b, CHUNK):
            nz = (ws[c:min(b, c + CHUNK)] != fill).nonzero()
            if nz.numel():
                first = c + int(nz.min()) if first is None else first
                last = c + int(nz.max())
        if first is not None:
            found.append((prev, first, last))
    return sorted(found, key=lambda f: f[1])


def table_problems(rows, total, g):
    """Violations of the layout contract of a recorded plan (empty list: fine)."""
    bad = []
    order = sorted(range(len(rows)), key=lambda i: rows[i][1])
    if [rows[i][1] for i in order] != [r[1] for r in rows]:
        bad.append("offsets are not in layout order")
    end = 0
    for k, (name, off, nb) in enumerate(rows):
        if off % 256:
            bad.append(f"{name}: offset {off} is not a multiple of 256")
        if k and off < end + g:
            bad.append(f"{name}: starts at {off}, less than {g} bytes behind the end {end} of {rows[k - 1][0]}")
        end = off + nb
    if rows and end + g > total:
        bad.append(f"last region ends at {end}: + {g} exceeds the total {total}")
    if len({r[0] for r in rows}) != len(rows):
        bad.append("region names repeat")
    return bad


def assert_clean(ws, fill, case, g=REDZONE):
    """Property A for the plan the LAST call on this thread recorded.  Returns (rows, total)."""
    torch.cuda.synchronize()
    rows, total = _lib.ws_regions()
    assert rows, f"{case}: the call recorded no plan"
    assert total <= ws.numel(), f"{case}: the plan needs {total} bytes, the ABI's size answer gave {ws.numel()}"
    assert not table_problems(rows, total, g), f"{case}: {table_problems(rows, total, g)}"
    hits = damage(ws, fill, rows)
    assert not hits, (f"{case}: bytes outside every workspace region changed (fill 0x{fill:02X}): " +
                      "; ".join(f"behind '{p}': first {a}, last {b}" for p, a, b in hits))
    return rows, total


class Fences:
    """Caller-sized buffers as views into larger sentinel-filled tensors."""

    def __init__(self, device="cuda"):
        self.device, self.items = device, []

    def new(self, name, shape, dtype=torch.float32, zero=False):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty(0, dtype=dtype).element_size()
        big = torch.full((FENCE + nbytes + FENCE,), SENTINEL, dtype=torch.uint8, device=self.device)
        view = big[FENCE:FENCE + nbytes].view(dtype).view(shape)
        if zero:
            view.zero_()
        self.items.append((name, big, nbytes))
        return view

    def problems(self):
        out = []
        for name, big, nbytes in self.items:
            for side, part, base in (("in front of", big[:FENCE], -FENCE), ("behind", big[FENCE + nbytes:], nbytes)):
                nz = (part != SENTINEL).nonzero()
                if nz.numel():
                    out.append(f"{name} ({nbytes} bytes): bytes {base + int(nz.min())} .. {base + int(nz.max())} {side} it changed")
        return out

    def check(self, case):
        torch.cuda.synchronize()
        assert not self.problems(), f"{case}: a caller-sized buffer was overrun: " + "; ".join(self.problems())


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
