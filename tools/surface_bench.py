"""Time of the surface stage (deepsdf_amd/surface.py, csrc/meshtopo.hpp) split into its steps, on the meshes an optimisation
iteration produces.  One JSON line per mesh.

    python tools/surface_bench.py [--nets 4x64 8x512] [--L 16] [--N 256] [--tiling 4 4 4] [--reps 5] [--cpu first]

Meshes       microstructure: microstructure_mesh_diff of ms_bench.py's seeded net and field at --N, --tiling (with its derivative);
             mesh_bench: mesh_bench.py's single-code mesh of the first net at --N (no derivative).
Steps        HIP events around each step, on a fresh workspace per repetition, median of --reps after one warm-up (min and max of
             the whole chain beside it):
               edge_keys_ms, edge_sort_ms (torch.sort, stable, of 3 F int64 keys), adjacency_ms, components_ms (host clock as
               well: the entry reads its change flags on the host every four rounds), rounds, degenerate_ms, corner_sort_ms
               (torch.sort of the 3 F corners + searchsorted), vertex_geometry_ms, volume_ms; with a derivative:
               volume_gradient_ms (the adjoint) and dtheta_ms with its store rate (V * 3 * R * 4 bytes over the median).
CPU          cpu_components_s: the numpy oracle (tests/meshtopo_numpy.py: mates by sorting, labels by union-find) on the same
             faces, host clock, once.  --cpu first: only the first microstructure mesh and the mesh_bench one; all; none.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from deepsdf_amd import _lib  # noqa: E402
from deepsdf_amd.mesh import marching_cubes, microstructure_mesh_diff, sdf_grid  # noqa: E402
from deepsdf_amd._lib import ptr as _ptr, stream as _stream  # noqa: E402
from deepsdf_amd.surface import SurfaceMesh  # noqa: E402
from tools import mesh_bench, ms_bench  # noqa: E402

STEPS = ("edge_keys", "edge_sort", "adjacency", "components", "degenerate", "corner_sort", "vertex_geometry", "volume")


def ev():
    return torch.cuda.Event(enable_timing=True)


def chain(m):
    """The steps of a SurfaceMesh through the C ABI with an event between each: ({step: ms}, components host ms, rounds, stats)."""
    lib = _lib.lib()
    nv, nf = m.n_verts, m.n_faces
    dev = m.device
    ws = m._ws()
    keys = torch.empty(3 * nf, dtype=torch.int64, device=dev)
    mate = torch.empty(3 * nf, dtype=torch.int32, device=dev)
    stats = torch.empty(6, dtype=torch.int64, device=dev)
    label, size = torch.empty(nf, dtype=torch.int32, device=dev), torch.empty(nf, dtype=torch.int32, device=dev)
    deg = torch.empty(nf, dtype=torch.uint8, device=dev)
    normals, grad = torch.empty(nv, 3, device=dev), torch.empty(nv, 3, device=dev)
    vol = torch.empty(1, dtype=torch.float64, device=dev)
    rounds = C.c_int32()
    marks = [ev() for _ in range(len(STEPS) + 1)]
    torch.cuda.synchronize()
    marks[0].record()
    _lib.check(lib.dsdf_mt_edge_keys(_ptr(m.F), nf, nv, _ptr(keys), _stream()))
    marks[1].record()
    skeys, order = torch.sort(keys, stable=True)
    marks[2].record()
    _lib.check(lib.dsdf_mt_adjacency(_ptr(m.F), nf, _ptr(skeys), _ptr(order), _ptr(mate), _ptr(stats), _ptr(ws), ws.numel(), _stream()))
    marks[3].record()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check(lib.dsdf_mt_components(_ptr(mate), nf, _ptr(label), _ptr(size), C.byref(rounds), _ptr(ws), ws.numel(), _stream()))
    marks[4].record()
    torch.cuda.synchronize()
    host_ms = (time.perf_counter() - t0) * 1e3
    _lib.check(lib.dsdf_mt_face_degenerate(_ptr(m.V), nv, _ptr(m.F), nf, _ptr(deg), _stream()))
    marks[5].record()
    corners, corder = torch.sort(m.F.reshape(-1).to(torch.int64), stable=True)
    vstart = torch.searchsorted(corners, torch.arange(nv + 1, dtype=torch.int64, device=dev))
    marks[6].record()
    _lib.check(lib.dsdf_mt_vertex_geometry(_ptr(m.V), nv, _ptr(m.F), nf, _ptr(corder), _ptr(vstart), _ptr(normals), _ptr(grad), _stream()))
    marks[7].record()
    _lib.check(lib.dsdf_mt_volume(_ptr(m.V), nv, _ptr(m.F), nf, _ptr(vol), _ptr(ws), ws.numel(), _stream()))
    marks[8].record()
    torch.cuda.synchronize()
    ms = {s: marks[i].elapsed_time(marks[i + 1]) for i, s in enumerate(STEPS)}
    return ms, host_ms, rounds.value, stats.tolist(), int((size > 0).sum()), float(vol)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        e0, e1 = ev(), ev()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
        del out
    return [round(x, 3) for x in (statistics.median(ts), min(ts), max(ts))]


def report(what, m, args, cpu, extra):
    chain(m)
    runs = [chain(m) for _ in range(args.reps)]
    med = {s + "_ms": round(statistics.median(r[0][s] for r in runs), 3) for s in STEPS}
    tot = [sum(r[0].values()) for r in runs]
    line = dict(what=what, V=m.n_verts, F=m.n_faces, **extra, **med,
                components_host_ms=round(statistics.median(r[1] for r in runs), 3), rounds=runs[-1][2],
                chain_ms=[round(x, 3) for x in (statistics.median(tot), min(tot), max(tot))],
                stats=dict(zip(("edges", "boundary", "nonmanifold", "paired", "same_direction", "degenerate_halfedges"), runs[-1][3])),
                components=runs[-1][4], volume=runs[-1][5])
    if m.diff is not None:
        R = m.diff.n_control_points * m.diff.latent_size
        line["volume_gradient_ms"] = timed(lambda: SurfaceMesh.volume_gradient(m), args.reps)
        try:
            line["dtheta_ms"] = timed(lambda: m.dtheta(), args.reps)
            line["dtheta_store_gbs"] = round(m.n_verts * 3 * R * 4 / 1e9 / line["dtheta_ms"][0] * 1e3, 1)
            jac, axis = m.diff.jacobian()
            out = torch.empty(m.n_verts, 3, R, device=m.device)
            st = (C.c_float * 3)(*m.stretch)
            n = m.vertex_normals()
            line["project_kernel_ms"] = timed(lambda: _lib.check(_lib.lib().dsdf_mt_project(_ptr(jac), _ptr(axis), _ptr(n), m.n_verts, R, st, 1.0,
                                                                                           _ptr(out), _stream())), args.reps)
            line["project_store_gbs"] = round(m.n_verts * 3 * R * 4 / 1e9 / line["project_kernel_ms"][0] * 1e3, 1)
            del jac, axis, out
        except MemoryError as e:
            line["dtheta_ms"] = f"skipped: {e}"
    if cpu:
        from tests import meshtopo_numpy
        faces = m.F.cpu().numpy()
        t0 = time.perf_counter()
        mate, _ = meshtopo_numpy.adjacency(faces)
        t1 = time.perf_counter()
        label, _ = meshtopo_numpy.components(mate, len(faces))
        t2 = time.perf_counter()
        line["cpu_adjacency_s"], line["cpu_components_s"] = round(t1 - t0, 3), round(t2 - t1, 3)
        line["cpu_labels_equal"] = bool((torch.from_numpy(label).to(m.device) == m.face_labels()).all())
        gpu = (med["edge_keys_ms"] + med["edge_sort_ms"] + med["adjacency_ms"] + line["components_host_ms"]) / 1e3
        line["cpu_over_gpu_adjacency_and_components"] = round((t2 - t0) / gpu, 1)
    line["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["4x64", "8x512"], choices=sorted(bench.NETWORKS))
    ap.add_argument("--L", type=int, default=16)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--tiling", nargs=3, type=int, default=[4, 4, 4])
    ap.add_argument("--max-batch", type=int, default=32 ** 3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", choices=("first", "all", "none"), default="first")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench.py needs an AMD GPU: nothing here can be timed on a CPU")
    field = ms_bench.make_field(args.L)
    for k, name in enumerate(args.nets):
        dec = ms_bench.make_decoder(name, args.L, field, args.tiling)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = microstructure_mesh_diff(args.tiling, dec, field, args.N, args.max_batch)
        torch.cuda.synchronize()
        build_ms = (time.perf_counter() - t0) * 1e3
        m = SurfaceMesh.from_diff(d, (2, 1, 1))
        report("microstructure", m, args, args.cpu == "all" or (args.cpu == "first" and k == 0),
               dict(net=name, L=args.L, N=args.N, tiling=args.tiling, band=d.band.numel(), mesh_diff_first_call_ms=round(build_ms, 1)))
        del d, m, dec
        torch.cuda.empty_cache()
    dec, z = mesh_bench.make_decoder(args.nets[0])
    h = 2.0 / (args.N - 1)
    with torch.no_grad():
        v, f = marching_cubes(sdf_grid(dec, z, args.N, args.max_batch), 0.0, (h, h, h), (-1, -1, -1))
    report("mesh_bench", SurfaceMesh(v, f), args, args.cpu != "none", dict(net=args.nets[0], N=args.N))


if __name__ == "__main__":
    main()
