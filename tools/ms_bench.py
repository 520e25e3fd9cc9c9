"""Time of one microstructure mesh (deepsdf_amd/mesh.py create_mesh_microstructure) split into its steps, and the row kernel
against the same rows composed from torch ops.  One JSON line per (net, L) and one per L for the row kernel.

    python tools/ms_bench.py [--nets 8x512 4x64] [--L 16 256] [--N 256] [--tiling 4 4 4] [--max-batch 32768] [--reps 5]
    python tools/ms_bench.py --diff [--nets 8x512 4x64] [--L 16] [--diff-N 64 256]
    python tools/ms_bench.py --block 4 [--lipschitz 1 0] [--nets 8x512 4x64] [--L 16]

mesh lines   rows_ms / decode_ms / caps_ms: HIP events around each step of every chunk, summed over the grid (the loop of
             microstructure_sdf_grid restated with events between the steps); mc_ms: events around marching_cubes; total_ms: host
             clock around microstructure_sdf_grid + marching_cubes as the library runs them, ending in a synchronise.  Median of
             --reps after one warm-up, with min and max of the total.
row lines    dsdf_ms_rows on one range of --row-points grid points, 20 launches after 3 warm-ups: median, min, max; the bytes it
             must write ((L + 3) * 4 per point) over the median as GB/s, beside the measured HBM copy rate of MI355X (6.29 TB/s
             for reading and writing, MI355X_MICROARCH.md); and the same rows from torch ops on the device (index arithmetic, the
             fold, a degree-1 basis and a matmul for the spline, a concatenation), checked against the kernel's before timing.

--diff       the derivative with respect to the control points (deepsdf_amd/mesh.py microstructure_mesh_diff) instead: one line per
             (net, L, N) with the band size and the time of its steps -- rows at the band indices, forward + input gradient,
             the dense assembly (with its store rate: V * ncp * L * 4 bytes over the median), the adjoint -- and, for comparison,
             the reference's recipe on the same build: ncp * L calls of Decoder.jvp over the same band, chunk by chunk
             (deep_sdf/mesh.py:405-422 runs that many double-backward passes, over the whole grid).  HIP events, median of --reps
             after one warm-up, with min and max.  --diff-N gives the grid sizes.

--block B    dense against sparse (microstructure_sdf_grid(block=B): surface following on blocks) in one process, one
             line per (net, L, lipschitz): a warm-up of both, then --reps alternating pairs; device events around grid + marching
             cubes; medians; the sparse path's steps from follow_surface's own events (coarse decode, the rounds' decode -- rows,
             decode and caps at listed points, one figure per round --, index kernels, fill), both marching cubes, its count reads, the
             fraction decoded and the rounds.

Nets: seeded (nn.Linear init) decoders of bench.py's NetworkSpecs with CodeLength L; the output bias is shifted so that the zero
level set crosses the structure.  A (net, L) pair for which no net exists (4x64 with L = 256) is reported as skipped.  The field: degree 1, 2 x 2 x 2 seeded codes.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))          # mesh_bench's timers (--block)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from deepsdf_amd.decoder import Decoder  # noqa: E402
from deepsdf_amd.mesh import (marching_cubes, microstructure_mesh_diff, microstructure_sdf_grid, ms_apply_caps, ms_grid_rows,  # noqa: E402
                              ms_rows_at)
from deepsdf_amd.spline import BSplineField  # noqa: E402

HBM_COPY_TBS = 6.29


def make_field(L):
    cp = torch.randn(8, L, generator=torch.Generator().manual_seed(2)) * (0.5 / math.sqrt(L))
    return BSplineField([1, 1, 1], [[-1, -1, 1, 1]] * 3, cp.numpy())


def make_decoder(name, L, field, tiling):
    torch.manual_seed(0)
    dec = Decoder(L, **bench.NETWORKS[name]["net"]).cuda().eval()
    with torch.no_grad():
        y = microstructure_sdf_grid(tiling, dec, field, 32, apply_caps=False)
        last = getattr(dec, f"lin{dec.spec.n_layers - 1}")
        last.bias -= torch.atanh(y[1:-1, 1:-1, 1:-1].median())
    return dec


def ev():
    return torch.cuda.Event(enable_timing=True)


def staged(dec, field, tiling, N, max_batch):
    """The chunk loop of microstructure_sdf_grid with events between its steps: (rows_ms, decode_ms, caps_ms)."""
    n = (N + 2) ** 3
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    eng = dec.engine()
    eng.materialize()
    marks = []
    with torch.no_grad():
        for b in range(0, n, max_batch):
            e = min(n, b + max_batch)
            m = [ev() for _ in range(4)]
            m[0].record()
            rows = ms_grid_rows(field, tiling, N, b, e)
            m[1].record()
            out[b:e] = eng.decode(rows).reshape(-1)
            m[2].record()
            ms_apply_caps(out[b:e], N, b, e)
            m[3].record()
            marks.append(m)
    torch.cuda.synchronize()
    return tuple(sum(m[i].elapsed_time(m[i + 1]) for m in marks) for i in range(3))


def whole(dec, field, tiling, N, max_batch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    grid = microstructure_sdf_grid(tiling, dec, field, N, max_batch)
    e0, e1 = ev(), ev()
    e0.record()
    h = 2.0 / (N - 1)
    v, f = marching_cubes(grid, 0.0, (h, h, h))
    e1.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), v.shape[0], f.shape[0]


def torch_rows(cp, tiling, N, start, end):
    """The rows of dsdf_ms_rows for a degree-1, 2 x 2 x 2 field from torch ops on the device."""
    n = N + 2
    vs = 2.0 / (n - 1 - 2)
    idx = torch.arange(start, end, dtype=torch.int64, device=cp.device)
    xo = torch.stack([(idx // n) // n, (idx // n) % n, idx % n], 1).to(torch.float32) * vs + (-1 - vs)
    inside = ((xo >= -1) & (xo <= 1)).all(1, keepdim=True)
    u = ((xo + 1) * 0.5).clamp(0, 1)
    B = torch.stack([1 - u, u], 2)                                           # [n, axis, 2]
    w = torch.einsum("pi,pj,pk->pkji", B[:, 0], B[:, 1], B[:, 2]).reshape(-1, 8)
    lat = (w @ cp) * inside
    cols = []
    for a, t in enumerate(tiling):
        p = 2.0 / t
        cols.append((2 / p) * torch.abs((xo[:, a] - t % 2) % (p * 2) - p) - 1)
    return torch.cat([lat, torch.stack(cols, 1)], 1)


def timed(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = ev(), ev()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)


ROWS_KERNEL_TBS = 3.0            # what the row kernel reaches at L = 256 (profiles/ms_bench.log)


def diff_bench(args, dev):
    """--diff: the steps of microstructure_mesh_diff and the reference's recipe, per (net, L, N)."""
    tiling = args.tiling
    for L in args.L:
        field = make_field(L)
        ncp = field.control_points.shape[0]
        for name in args.nets:
            spec = bench.NETWORKS[name]["net"]
            if any(spec["dims"][l - 1] <= L + 3 for l in spec["latent_in"]):
                print(json.dumps(dict(what="diff", net=name, L=L, skipped=f"no {name} net exists for L = {L}")), flush=True)
                continue
            dec = make_decoder(name, L, field, tiling)
            eng = dec.engine()
            for N in args.diff_N:
                d = microstructure_mesh_diff(tiling, dec, field, N, args.max_batch)
                nb, V = d.band.numel(), d.verts.shape[0]
                ones = torch.ones(min(nb, args.max_batch), device="cuda")

                def band_steps():
                    marks = []
                    with torch.no_grad():
                        for b in range(0, nb, args.max_batch):
                            e = min(nb, b + args.max_batch)
                            m = [ev() for _ in range(3)]
                            m[0].record()
                            rows, _, _ = ms_rows_at(field, tiling, N, d.band[b:e])
                            m[1].record()
                            eng.module_forward(rows, False)
                            eng.module_input_grad(ones[:e - b], e - b)
                            m[2].record()
                            marks.append(m)
                    torch.cuda.synchronize()
                    return tuple(sum(m[i].elapsed_time(m[i + 1]) for m in marks) for i in range(2))

                def reference_recipe():
                    with torch.no_grad():
                        for b in range(0, nb, args.max_batch):
                            e = min(nb, b + args.max_batch)
                            rows, w, base = ms_rows_at(field, tiling, N, d.band[b:e])
                            tangent = torch.zeros_like(rows)
                            for c in range(ncp):           # degree 1, 2 x 2 x 2: slot (k * 4 + j) * 4 + i of control point c
                                wc = w[:, ((c >> 2) * 4 + ((c >> 1) & 1)) * 4 + (c & 1)]
                                for l in range(L):
                                    tangent.zero_()
                                    tangent[:, l] = wc
                                    dec.jvp(rows, tangent)

                band_steps()
                st = [band_steps() for _ in range(args.reps)]
                gw = torch.randn(V, 3, device="cuda")
                dense = timed(lambda: d.jacobian(), args.reps, 1)
                vjp = timed(lambda: d.vjp(gw), args.reps, 1)
                jvp = timed(lambda: d.jvp(d.G.new_ones(ncp, L)), args.reps, 1)
                ref = timed(reference_recipe, args.reps, 1)
                rows_ms, grad_ms = (statistics.median(s[i] for s in st) for i in range(2))
                gb = V * ncp * L * 4 / 1e9
                ours = rows_ms + grad_ms + dense[0]
                print(json.dumps(dict(what="diff", net=name, L=L, N=N, tiling=tiling, max_batch=args.max_batch, V=V, band=nb,
                                      grid_points=(N + 2) ** 3, n_control_points=ncp, rows_ms=round(rows_ms, 3),
                                      forward_input_grad_ms=round(grad_ms, 3), dense_ms=[round(x, 3) for x in dense],
                                      dense_store_gbs=round(gb / dense[0] * 1e3, 1),
                                      dense_share_of_row_kernel_rate=round(gb / dense[0] / ROWS_KERNEL_TBS, 3),
                                      vjp_ms=[round(x, 3) for x in vjp], jvp_ms=[round(x, 3) for x in jvp],
                                      reference_recipe_ms=[round(x, 1) for x in ref], reference_jvp_calls=ncp * L,
                                      reference_over_ours=round(ref[0] / ours, 1), device=dev)), flush=True)
                del d


def sparse_bench(args, dev):
    from mesh_bench import StepTimer, events_ms, sparse_summary
    N, tiling = args.N, args.tiling
    h = 2.0 / (N - 1)
    mc = lambda g: marching_cubes(g, 0.0, (h, h, h))                                   # noqa: E731
    for L in args.L:
        field = make_field(L)
        for name in args.nets:
            spec = bench.NETWORKS[name]["net"]
            if any(spec["dims"][l - 1] <= L + 3 for l in spec["latent_in"]):
                print(json.dumps(dict(what="sparse", net=name, L=L, skipped=f"no {name} net exists for L = {L}")), flush=True)
                continue
            dec = make_decoder(name, L, field, tiling)

            def pair(lip):
                d_ms, grid = events_ms(lambda: microstructure_sdf_grid(tiling, dec, field, N, args.max_batch))
                mc_ms, (vd, fd) = events_ms(lambda: mc(grid))
                del grid
                stats, timer = {}, StepTimer()
                s_ms, grid = events_ms(lambda: microstructure_sdf_grid(tiling, dec, field, N, args.max_batch, block=args.block, lipschitz=lip,
                                                                       stats=stats, on_step=timer))
                mc2_ms, (vs, fs) = events_ms(lambda: mc(grid))
                same = vd.shape == vs.shape and fd.shape == fs.shape and bool(torch.equal(vd, vs)) and bool(torch.equal(fd, fs))
                return dict(dense=d_ms + mc_ms, mc=mc_ms, sparse=s_ms + mc2_ms, mc_sparse=mc2_ms, steps=timer.steps(), waits=timer.waits(),
                            stats=stats, same=same, F=(fd.shape[0], fs.shape[0]))

            for lip in args.lipschitz:
                pair(lip)
                runs = [pair(lip) for _ in range(args.reps)]
                print(json.dumps(dict(what="sparse", net=name, L=L, N=N, tiling=tiling, block=args.block, lipschitz=lip, max_batch=args.max_batch,
                                      reps=args.reps, **sparse_summary(runs), device=dev)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["8x512", "4x64"], choices=sorted(bench.NETWORKS))
    ap.add_argument("--L", nargs="+", type=int, default=[16, 256])
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--tiling", nargs=3, type=int, default=[4, 4, 4])
    ap.add_argument("--max-batch", type=int, default=32 ** 3, help="chunk (create_mesh_microstructure's max_batch)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--row-points", type=int, default=1 << 21, help="points of the row-kernel measurement")
    ap.add_argument("--diff", action="store_true", help="time the derivative with respect to the control points instead")
    ap.add_argument("--diff-N", nargs="+", type=int, default=[64, 256], help="grid sizes of --diff")
    ap.add_argument("--block", type=int, default=None, help="compare the dense path with surface following on blocks of this edge")
    ap.add_argument("--lipschitz", nargs="+", type=float, default=[1.0, 0.0], help="with --block: the seeding slopes to run")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ms_bench.py needs an AMD GPU: nothing here can be timed on a CPU")
    dev = torch.cuda.get_device_name(0)
    if args.diff:
        return diff_bench(args, dev)
    if args.block:
        return sparse_bench(args, dev)
    N, tiling = args.N, args.tiling
    for L in args.L:
        field = make_field(L)
        cp = torch.from_numpy(np.ascontiguousarray(field.control_points, dtype=np.float32)).cuda()
        n = min(args.row_points, (N + 2) ** 3)
        start = ((N + 2) ** 3 - n) // 2
        k = ms_grid_rows(field, tiling, N, start, start + n)
        t = torch_rows(cp, tiling, N, start, start + n)
        diff = float((k - t).abs().max())
        assert diff < 1e-5, diff                                  # the same rows up to fp32 rounding of the composed ops
        del k, t
        km = timed(lambda: ms_grid_rows(field, tiling, N, start, start + n), 20, 3)
        tm = timed(lambda: torch_rows(cp, tiling, N, start, start + n), 20, 3)
        gb = n * (L + 3) * 4 / 1e9
        print(json.dumps(dict(what="rows", L=L, points=n, kernel_ms=[round(x, 4) for x in km], torch_ops_ms=[round(x, 4) for x in tm],
                              kernel_write_gbs=round(gb / km[0] * 1e3, 1), share_of_hbm_copy_rate=round(gb / km[0] / HBM_COPY_TBS, 3),
                              torch_over_kernel=round(tm[0] / km[0], 2), max_abs_diff=diff, device=dev)), flush=True)
        for name in args.nets:
            spec = bench.NETWORKS[name]["net"]
            if any(spec["dims"][l - 1] <= L + 3 for l in spec["latent_in"]):
                # the layer in front of a latent_in layer has dims - (L + 3) outputs: no such net exists
                print(json.dumps(dict(what="mesh", net=name, L=L, skipped=f"no {name} net with latent_in {spec['latent_in']} "
                                      f"exists for L = {L}: the layer before it would have {spec['dims'][0]} - {L + 3} outputs")), flush=True)
                continue
            dec = make_decoder(name, L, field, tiling)
            staged(dec, field, tiling, N, args.max_batch)
            st = [staged(dec, field, tiling, N, args.max_batch) for _ in range(args.reps)]
            wh = [whole(dec, field, tiling, N, args.max_batch) for _ in range(args.reps)]
            rows, decode, caps = (statistics.median(s[i] for s in st) for i in range(3))
            tot = [w[0] for w in wh]
            print(json.dumps(dict(what="mesh", net=name, L=L, N=N, tiling=tiling, max_batch=args.max_batch, rows_ms=round(rows, 3),
                                  decode_ms=round(decode, 3), caps_ms=round(caps, 3),
                                  mc_ms=round(statistics.median(w[1] for w in wh), 3), total_ms=round(statistics.median(tot), 3),
                                  total_min_max_ms=[round(min(tot), 3), round(max(tot), 3)],
                                  rows_share_of_chunk=round(rows / (rows + decode + caps), 4), V=wh[-1][2], F=wh[-1][3],
                                  device=dev)), flush=True)


if __name__ == "__main__":
    main()
