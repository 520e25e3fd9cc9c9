"""Marching cubes against the tetrahedral mesher (deepsdf_amd/tetmesh.py) on the same grids in one process, one JSON
line per grid.

    python tools/tet_bench.py [--net 4x64] [--N 64 128] [--n-base 16] [--tiling 4 4 4] [--reps 7] [--log profiles/tet_bench.log]

Grids: the single-code grid of a seeded decoder of bench.py's NetworkSpecs (tools/mesh_bench.py make_decoder) at every --N, and the
tiled, capped structure of tools/ms_bench.py (degree-1 field, 2 x 2 x 2 seeded codes, L = 16) at N = n_base * tiling + 1 per axis.
The grid is decoded once; then, after one warm-up of each, --reps rounds of (marching_cubes, tetrahedralize, tetrahedralize with
return_edges, solid_components), alternating, HIP events around each call as the library runs it (the totals' host read included).
Medians with min and max; V / F of the surface, V / T / M of the volume mesh, its bytes, and the share of the elements that have
all four corners on grid points.  The lines are printed and, with --log, appended to that file behind a header naming the command.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))          # mesh_bench / ms_bench: the decoders and the timers
import torch  # noqa: E402

from deepsdf_amd.mesh import marching_cubes, microstructure_sdf_grid, sdf_grid, solid_components, tetrahedralize  # noqa: E402


def stats(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def compare(what, grid, spacing, origin, reps, dev, **extra):
    from mesh_bench import events_ms
    calls = dict(mc=lambda: marching_cubes(grid, 0.0, spacing, origin),
                 tet=lambda: tetrahedralize(grid, 0.0, spacing, origin),
                 tet_edges=lambda: tetrahedralize(grid, 0.0, spacing, origin, return_edges=True),
                 components=lambda: solid_components(grid))
    for fn in calls.values():
        fn()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t, out = events_ms(fn)
            ms[k].append(t)
            if k == "mc":
                v, f = out
            elif k == "tet":
                m = out
            elif k == "components":
                rounds, n_comp = out[2], int((out[1] > 0).sum())
    me = tetrahedralize(grid, 0.0, spacing, origin, return_edges=True)
    full = int((me.vert_class[me.tets.long()] == 0).all(1).sum())
    out_bytes = m.n_verts * 12 + m.n_tets * 16 + m.n_bfaces * 13
    line = dict(what=what, dims=list(grid.shape), reps=reps, mc_ms=stats(ms["mc"]), tet_ms=stats(ms["tet"]),
                tet_edges_ms=stats(ms["tet_edges"]), components_ms=stats(ms["components"]), component_rounds=rounds,
                components=n_comp, tet_over_mc=round(statistics.median(ms["tet"]) / statistics.median(ms["mc"]), 2),
                surface_V=v.shape[0], surface_F=f.shape[0], V=m.n_verts, T=m.n_tets, M=m.n_bfaces, output_mb=round(out_bytes / 1e6, 2),
                grid_only_elements=round(full / max(m.n_tets, 1), 4), volume=m.volume(), device=dev, **extra)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="4x64")
    ap.add_argument("--N", nargs="*", type=int, default=[64, 128])
    ap.add_argument("--n-base", type=int, default=16, help="grid points per tile of the tiled structure (0: skip it)")
    ap.add_argument("--tiling", nargs=3, type=int, default=[4, 4, 4])
    ap.add_argument("--max-batch", type=int, default=32 ** 3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log", default=None, help="append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tet_bench.py needs an AMD GPU: nothing here can be timed on a CPU")
    import mesh_bench
    import ms_bench
    dev = torch.cuda.get_device_name(0)
    lines = []

    def emit(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    dec, z = mesh_bench.make_decoder(args.net)
    for N in args.N:
        h = 2.0 / (N - 1)
        with torch.no_grad():
            grid = sdf_grid(dec, z, N, args.max_batch)
        emit(compare("single code", grid, (h, h, h), (-1, -1, -1), args.reps, dev, net=args.net, N=N))
        del grid
    if args.n_base > 0:
        L, tiling = 16, args.tiling
        field = ms_bench.make_field(L)
        dec = ms_bench.make_decoder(args.net, L, field, tiling)
        n = [args.n_base * t + 1 for t in tiling]
        with torch.no_grad():
            grid = microstructure_sdf_grid(tiling, dec, field, n, args.max_batch)
        vs = [2.0 / (k - 1) for k in n]
        emit(compare("tiled structure", grid, vs, [-1 - v for v in vs], args.reps, dev, net=args.net, L=L, tiling=tiling,
                     N_base=args.n_base))
    if args.log:
        with open(args.log, "a") as fh:
            fh.write("# python tools/tet_bench.py " + " ".join(sys.argv[1:]) + f"   ({dev}; medians [median, min, max] of {args.reps} "
                     "alternating rounds after one warm-up, HIP events around each library call)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
