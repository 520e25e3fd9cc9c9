"""Mesh SDF throughput (csrc/meshsdf.hpp through dsdf_msdf_query), one JSON line per case, written to --out and stdout.

    python tools/meshsdf_bench.py [--out profiles/meshsdf_bench.log] [--reps 5]

Cases: 1e5 uniform queries in [-1, 1]^3 (the fork's SDFSampler call) against icospheres of 20 480, 81 920 and 327 680 faces
and one lattice-like mesh (this package's marching_cubes of an analytic strut field), each in sdf mode (distance + winding)
and distance-only mode; then one SDFSampler.sample_sdfs file end to end (1e5 samples of the 81 920-face icosphere, mesh upload
included) with the share of its time spent outside the query kernel.

ms: HIP events around one dsdf_msdf_query call (outputs and workspace allocated beforehand), best of --reps after 2 warm-up
calls.  issue_bound_ms: the least time the query kernel could take at the VALU issue rate: the VALU instructions of its face
loop, counted in this build's code object (2 cycles per wave64 instruction on a SIMD, 4 for a transcendental), times
waves x faces, over 256 CUs x 4 SIMDs at 2.4 GHz.  issue_fraction = issue_bound_ms / ms.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepsdf_amd import _lib, asmcheck  # noqa: E402
from deepsdf_amd.build import LIB  # noqa: E402
from deepsdf_amd.mesh import marching_cubes  # noqa: E402
from deepsdf_amd._lib import ptr as _ptr, stream as _stream  # noqa: E402
from deepsdf_amd.meshsdf import TriangleMesh  # noqa: E402
from deepsdf_amd.sdf_sampler import SDFfromMesh, SDFSampler  # noqa: E402
from tests.meshsdf_numpy import icosphere  # noqa: E402

CUS, SIMDS, CLOCK = 256, 4, 2.4e9
TRANS = re.compile(r"^v_(rcp|rsq|sqrt|exp|log|sin|cos)_")


def loop_counts(kernel_part):
    """(VALU, transcendental) instruction counts of the largest backward-branch loop of the kernel whose symbol contains
    kernel_part, in the library's gfx950 code object."""
    with tempfile.TemporaryDirectory() as d:
        co = asmcheck.extract_code_object(LIB, d)
        syms = subprocess.run([os.path.join(asmcheck.LLVM, "llvm-readelf"), "-sW", co], capture_output=True, text=True,
                              check=True).stdout
        names = sorted({f.split()[7] for f in syms.splitlines()
                        if len(f.split()) >= 8 and f.split()[3] == "FUNC" and kernel_part in f.split()[7]})
        assert len(names) == 1, names
        out = subprocess.run([os.path.join(asmcheck.LLVM, "llvm-objdump"), "-d", f"--disassemble-symbols={names[0]}", co],
                             capture_output=True, text=True, check=True).stdout
    ins = []
    for line in out.splitlines():
        m = re.match(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):[^<]*(?:<[^+>]*\+0x([0-9a-f]+)>)?", line)
        if m:
            ins.append((int(m.group(3), 16), m.group(1), int(m.group(4), 16) if m.group(4) else None))
    start = ins[0][0]
    best = (0, 0)
    for addr, op, off in ins:
        if op.startswith("s_cbranch") and off is not None and start + off < addr:
            body = [o for a, o, _ in ins if start + off <= a <= addr]
            valu = [o for o in body if o.startswith("v_")]
            best = max(best, (len(valu), sum(1 for o in valu if TRANS.match(o))))
    return best


def lattice_mesh(n=128, cell=0.5, radius=0.06):
    """Cubic strut lattice (struts along x, y, z every `cell`) cut by the box |x| <= 0.9, meshed by marching_cubes."""
    ax = torch.linspace(-1, 1, n, device="cuda", dtype=torch.float64)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    g = [u - cell * torch.round(u / cell) for u in (x, y, z)]
    strut = torch.minimum(torch.minimum(torch.hypot(g[1], g[2]), torch.hypot(g[0], g[2])), torch.hypot(g[0], g[1])) - radius
    f = torch.maximum(strut, torch.maximum(torch.maximum(x.abs(), y.abs()), z.abs()) - 0.9)
    h = 2.0 / (n - 1)
    v, fc = marching_cubes(f.float(), 0.0, (h, h, h), (-1, -1, -1))
    return v, fc


def time_query(m, Q, mode, reps):
    nq = Q.shape[0]
    lib = _lib.lib()
    wb, ns = m.plan(nq)
    ws = torch.empty(wb, dtype=torch.uint8, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    sdf = torch.empty(nq, **f32) if mode == "sdf" else None
    d2 = torch.empty(nq, **f32) if mode == "distance" else None
    face = torch.empty(nq, dtype=torch.int32, device="cuda") if mode == "distance" else None
    cl = torch.empty(nq, 3, **f32) if mode == "distance" else None

    def call():
        _lib.check(lib.dsdf_msdf_query(_ptr(m.tri), m.n_faces, _ptr(Q), nq, _ptr(sdf), _ptr(d2), _ptr(face), _ptr(cl), None, 0,
                                       _ptr(ws), ws.numel(), _stream()))
    for _ in range(2):
        call()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return min(times), ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meshsdf_bench.log"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.cuda.get_device_name(0)
    Q = (torch.rand(100000, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64) * 2 - 1).float().cuda()
    counts = {"sdf": loop_counts("msdf_query_kernelILb1ELb1E"), "distance": loop_counts("msdf_query_kernelILb1ELb0E")}
    meshes = [(f"icosphere{s}", *icosphere(s)) for s in (5, 6, 7)]
    lv, lf = lattice_mesh()
    meshes.append(("lattice", lv, lf))
    lines = []
    kernel_ms = {}
    for name, V, F in meshes:
        m = TriangleMesh(V, F)
        waves = -(-Q.shape[0] // 256) * 4
        for mode in ("sdf", "distance"):
            ms, ns = time_query(m, Q, mode, a.reps)
            valu, trans = counts[mode]
            bound = waves * m.n_faces * (2 * (valu - trans) + 4 * trans) / (CUS * SIMDS * CLOCK) * 1e3
            kernel_ms[(name, mode)] = ms
            lines.append(dict(case=name, faces=m.n_faces, queries=Q.shape[0], mode=mode, splits=ns, ms=round(ms, 3),
                              gpairs_s=round(Q.shape[0] * m.n_faces / ms / 1e6, 2), loop_valu=valu, loop_transcendental=trans,
                              issue_bound_ms=round(bound, 3), issue_fraction=round(bound / ms, 3), device=dev))
            print(json.dumps(lines[-1]), flush=True)
        del m
    # one sample_sdfs file end to end: warm-up file first (process start-up), then a fresh SDFfromMesh (upload + prepare)
    V, F = meshes[1][1], meshes[1][2]
    with tempfile.TemporaryDirectory() as d:
        s = SDFSampler(os.path.join(d, "SdfSamples"), d)
        info = {"dataset_name": "bench", "class_name": "warm"}
        np.random.seed(0)
        s.sample_sdfs([SDFfromMesh((V, F))], info, n_samples=1e5)
        info = {"dataset_name": "bench", "class_name": "timed"}
        t0 = time.perf_counter()
        s.sample_sdfs([SDFfromMesh((V, F))], info, n_samples=1e5)
        total = (time.perf_counter() - t0) * 1e3
        t = s.timings[0]
    k = kernel_ms[(meshes[1][0], "sdf")]
    lines.append(dict(case="sample_sdfs_file", mesh=meshes[1][0], faces=len(F), n_samples=100000, total_ms=round(total, 2),
                      sample_ms=round(t["sample_s"] * 1e3, 2), sdf_call_ms=round(t["sdf_s"] * 1e3, 2),
                      write_ms=round(t["write_s"] * 1e3, 2), query_kernel_ms=round(k, 3),
                      host_share=round(1 - k / total, 4), device=dev))
    print(json.dumps(lines[-1]), flush=True)
    with open(a.out, "w") as fh:
        fh.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
