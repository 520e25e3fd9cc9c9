"""The volume mesh derivative (deepsdf_amd.mesh.VolumeMeshDiff) beside the surface derivative on the tiled structure
tools/fem_bench.py solves, one JSON line per size.

    python tools/voldiff_bench.py [--net 4x64] [--n-base 16] [--tiling 4 4 4] [--reps 9] [--log profiles/voldiff_bench.log]

The structure of tools/ms_bench.py (degree-1 field, 2 x 2 x 2 seeded codes, L = 16) at N = n_base * tiling + 1 per axis:
microstructure_mesh_diff gives the surface and its band, tetrahedralize (t_clamp = 0.05, largest component, vertex edges) the volume
mesh of the same grid, MicrostructureMeshDiff.for_tetmesh the volume band.  Timed with HIP events after one warm-up, [median, min,
max] of --reps: the volume band build (rows, decode and input gradient at the band points, mask), the volume adjoint and tangent,
and the surface adjoint and tangent on the same structure in the same process, the two adjoints alternating.  The last figure is
the ratio of the two adjoints' time per listed vertex (volume: the class >= 1 vertices; surface: all of its vertices)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))          # mesh_bench / ms_bench: the decoders and the timers
import torch  # noqa: E402

from deepsdf_amd.mesh import microstructure_mesh_diff, tetrahedralize  # noqa: E402


def med(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="4x64")
    ap.add_argument("--n-base", nargs="*", type=int, default=[16], help="grid points per tile of the tiled structure")
    ap.add_argument("--tiling", nargs=3, type=int, default=[4, 4, 4])
    ap.add_argument("--max-batch", type=int, default=32 ** 3)
    ap.add_argument("--t-clamp", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--log", default=None, help="append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voldiff_bench.py needs an AMD GPU: nothing here can be timed on a CPU")
    import ms_bench
    from mesh_bench import events_ms
    dev = torch.cuda.get_device_name(0)
    L, tiling = 16, args.tiling
    field = ms_bench.make_field(L)
    dec = ms_bench.make_decoder(args.net, L, field, tiling)
    lines = []
    for n_base in sorted(args.n_base):
        n = [n_base * t + 1 for t in tiling]
        d = microstructure_mesh_diff(tiling, dec, field, n, args.max_batch)
        tet = tetrahedralize(d.grid, 0.0, d.voxel_size, t_clamp=args.t_clamp, keep_largest=True, return_edges=True)
        v = d.for_tetmesh(tet, args.t_clamp)                                   # warm-up of the band build
        band_ms = [events_ms(lambda: d.for_tetmesh(tet, args.t_clamp))[0] for _ in range(args.reps)]
        gen = torch.Generator().manual_seed(1)
        gs = torch.randn(d.verts.shape[0], 3, generator=gen).cuda()
        gv = torch.randn(v.n_verts, 3, generator=gen).cuda()
        dcp = torch.randn(d.n_control_points, L, generator=gen).cuda()
        d.vjp(gs), v.vjp(gv), d.jvp(dcp), v.jvp(dcp)
        s_vjp, v_vjp, s_jvp, v_jvp = [], [], [], []
        for _ in range(args.reps):                                             # alternating: the same clocks and caches for both
            s_vjp.append(events_ms(lambda: d.vjp(gs))[0])
            v_vjp.append(events_ms(lambda: v.vjp(gv))[0])
            s_jvp.append(events_ms(lambda: d.jvp(dcp))[0])
            v_jvp.append(events_ms(lambda: v.jvp(dcp))[0])
        Vs, Vm = int(d.verts.shape[0]), int(v.moving.numel())
        per_s, per_v = statistics.median(s_vjp) / Vs, statistics.median(v_vjp) / Vm
        cls = torch.bincount(v.vert_class.long(), minlength=8).tolist()
        line = dict(what="tiled structure", dims=n, surface_verts=Vs, volume_verts=v.n_verts, volume_listed=Vm, class_counts=cls,
                    surface_band=int(d.band.numel()), volume_band=int(v.band.numel()), reps=args.reps, t_clamp=args.t_clamp,
                    volume_band_build_ms=med(band_ms), volume_vjp_ms=med(v_vjp), volume_jvp_ms=med(v_jvp), surface_vjp_ms=med(s_vjp),
                    surface_jvp_ms=med(s_jvp), vjp_parts=[d.vjp_plan()[1], v.vjp_plan()[1]],
                    vjp_ns_per_vertex=[round(per_s * 1e6, 2), round(per_v * 1e6, 2)], vjp_per_vertex_ratio=round(per_v / per_s, 3),
                    device=dev, net=args.net, L=L, n_control_points=d.n_control_points, tiling=tiling, N_base=n_base)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if args.log:
        with open(args.log, "a") as fh:
            fh.write("# python tools/voldiff_bench.py " + " ".join(sys.argv[1:]) + f"   ({dev}; [median, min, max] of {args.reps} after one "
                     "warm-up, HIP events; the two adjoints alternate)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
