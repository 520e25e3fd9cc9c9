"""The elasticity solver (deepsdf_amd/fem.py) on the volume mesh of the tiled structure tools/tet_bench.py meshes, one
JSON line per size.

    python tools/fem_bench.py [--net 4x64] [--n-base 8 16] [--tiling 4 4 4] [--reps 5] [--host-iters 20] [--log profiles/fem_bench.log]

The structure of tools/ms_bench.py (degree-1 field, 2 x 2 x 2 seeded codes, L = 16) at N = n_base * tiling + 1 per axis is meshed with
t_clamp = 0.05, its largest component kept, and shifted so that its lowest corner is the origin; then the reference's problem
(CantileverBeam.set_up): the reference's boundary attributes, attribute 1 (the low-x face) clamped, the traction (0, 0, -0.01) on
attribute 2 (the top), lam = 0, mu = 105.  Timed with HIP events after one warm-up, medians of --reps: one operator application
(dsdf_fem_apply through LinearElasticity.apply), the two terms of the exact discrete gradient the same way (stiffness_gradient: two
passes and two allocations; load_gradient: the boundary pass of the one traction and the sum), one CG iteration (the difference of two solves of 50 and 250 iterations at rel_tol = 0,
one host read each), and the whole solve to 1e-10 with its iteration count.  Bytes per iteration are DESIGN 4.21.4's two counts: what
the kernels request (612 T + 353 V) and what has to cross HBM at least once (304 T + 378 V); the rates divide them by the iteration
time.  On the smallest mesh the oracle's scipy PCG (tests/fem_numpy.py) runs --host-iters iterations on the host, for scale."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))          # mesh_bench / ms_bench: the decoders and the timers
import torch  # noqa: E402

from deepsdf_amd.fem import LinearElasticity  # noqa: E402
from deepsdf_amd.mesh import microstructure_sdf_grid, tetrahedralize  # noqa: E402

LAM, MU, TRACTION = 0.0, 105.0, (0.0, 0.0, -0.01)


def requested_bytes(V, T):
    return 612 * T + 353 * V


def compulsory_bytes(V, T):
    return 304 * T + 378 * V


def med(ts):
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def problem(mesh):
    s = LinearElasticity(mesh, LAM, MU)
    s.fix_faces(1)
    s.add_traction(2, TRACTION)
    return s


def host_pcg_ms(mesh, iters):
    """Wall milliseconds per iteration of the oracle's PCG on the host (assembly excluded, reported beside it)."""
    from tests import fem_numpy as F
    v, t, bf = mesh.verts.cpu().numpy(), mesh.tets.cpu().numpy(), mesh.bfaces.cpu().numpy()
    kind = mesh.boundary_attributes().cpu().numpy()
    t0 = time.perf_counter()
    mask = F.fixed_vertices(bf, kind == 1, len(v)) | F.held_vertices(t, F.geometry(v, t)[1], len(v))
    A = F.masked(F.assemble(v, t, LAM, MU), mask)
    f = F.load(v, bf, kind == 2, TRACTION, mask)
    Dinv = F.block_inverse(F.diag_blocks(A))
    t1 = time.perf_counter()
    _, it, _, _ = F.pcg(A, Dinv, f, rel_tol=0.0, max_iter=iters)
    return (time.perf_counter() - t1) * 1e3 / max(it, 1), (t1 - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", default="4x64")
    ap.add_argument("--n-base", nargs="*", type=int, default=[8, 16], help="grid points per tile of the tiled structure")
    ap.add_argument("--tiling", nargs=3, type=int, default=[4, 4, 4])
    ap.add_argument("--max-batch", type=int, default=32 ** 3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=20, help="iterations of the oracle's PCG on the smallest mesh (0: skip)")
    ap.add_argument("--log", default=None, help="append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fem_bench.py needs an AMD GPU: nothing here can be timed on a CPU")
    import ms_bench
    from mesh_bench import events_ms
    dev = torch.cuda.get_device_name(0)
    L, tiling = 16, args.tiling
    field = ms_bench.make_field(L)
    dec = ms_bench.make_decoder(args.net, L, field, tiling)
    lines = []
    for k, n_base in enumerate(sorted(args.n_base)):
        n = [n_base * t + 1 for t in tiling]
        with torch.no_grad():
            grid = microstructure_sdf_grid(tiling, dec, field, n, args.max_batch)
        vs = [2.0 / (q - 1) for q in n]
        mesh = tetrahedralize(grid, 0.0, vs, [-1 - q for q in vs], t_clamp=0.05, keep_largest=True)
        del grid
        mesh = mesh.transformed(1.0, (-mesh.verts.min(0).values).tolist())
        V, T = mesh.n_verts, mesh.n_tets
        attr = mesh.boundary_attributes()
        if int((attr == 1).sum()) == 0 or int((attr == 2).sum()) == 0:
            raise SystemExit("no boundary triangle carries attribute 1 or 2: nothing to clamp or to load")
        t_setup, s = events_ms(lambda: problem(mesh))
        x = torch.randn(V, 3, dtype=torch.float64, device="cuda")
        s.apply(x)
        apply_ms = [events_ms(lambda: [s.apply(x) for _ in range(20)])[0] / 20 for _ in range(args.reps)]
        s.stiffness_gradient(x)
        s.load_gradient(x)
        stiffness_gradient_ms = [events_ms(lambda: [s.stiffness_gradient(x) for _ in range(20)])[0] / 20 for _ in range(args.reps)]
        load_gradient_ms = [events_ms(lambda: [s.load_gradient(x) for _ in range(20)])[0] / 20 for _ in range(args.reps)]
        s.solve(rel_tol=0.0, max_iter=50, check_every=10 ** 6)
        iter_ms = []
        for _ in range(args.reps):
            a = events_ms(lambda: s.solve(rel_tol=0.0, max_iter=50, check_every=10 ** 6))[0]
            b = events_ms(lambda: s.solve(rel_tol=0.0, max_iter=250, check_every=10 ** 6))[0]
            iter_ms.append((b - a) / 200)
        solve_ms, res = [], None
        for _ in range(args.reps):
            t, res = events_ms(lambda: s.solve())
            solve_ms.append(t)
        it_s = statistics.median(iter_ms) * 1e-3
        line = dict(what="tiled structure", dims=n, V=V, T=T, M=mesh.n_bfaces, skipped=s.n_skipped_elements, held=s.n_held_vertices,
                    reps=args.reps, setup_ms=round(t_setup, 3), apply_ms=med(apply_ms), stiffness_gradient_ms=med(stiffness_gradient_ms),
                    load_gradient_ms=med(load_gradient_ms), cg_iteration_ms=med(iter_ms), solve_ms=med(solve_ms),
                    iterations=res[0], converged=res[1], ratio=res[2], compliance=s.compliance(), work=s.work(), volume=s.volume(),
                    requested_mb_per_iteration=round(requested_bytes(V, T) / 1e6, 2),
                    compulsory_mb_per_iteration=round(compulsory_bytes(V, T) / 1e6, 2),
                    requested_tb_s=round(requested_bytes(V, T) / it_s / 1e12, 3), compulsory_tb_s=round(compulsory_bytes(V, T) / it_s / 1e12, 3),
                    device=dev, net=args.net, L=L, tiling=tiling, N_base=n_base)
        if k == 0 and args.host_iters > 0:
            per_it, assembly = host_pcg_ms(mesh, args.host_iters)
            line.update(host_pcg_ms_per_iteration=round(per_it, 2), host_assembly_ms=round(assembly, 1), host_iters=args.host_iters)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
        del s, mesh
    if args.log:
        with open(args.log, "a") as fh:
            fh.write("# python tools/fem_bench.py " + " ".join(sys.argv[1:]) + f"   ({dev}; [median, min, max] of {args.reps} after one warm-up, "
                     "HIP events; a CG iteration = (solve of 250 - solve of 50 iterations) / 200)\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
