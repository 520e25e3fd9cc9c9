"""Time of one mesh (deepsdf_amd/mesh.py create_mesh) split into its three steps, one JSON line per (net, N):
decode (sdf_grid: the N^3 grid through Engine.decode_latent in max_batch chunks), marching cubes (HIP events around
dsdf_mc_count + the totals read + dsdf_mc_emit) and PLY write, with V and F.

    python tools/mesh_bench.py [--nets 8x512 4x64] [--N 128 256] [--max-batch 32768] [--reps 3]
    python tools/mesh_bench.py --block 4 [--lipschitz 1 0] [--reps 5]

--block B    dense against sparse (sdf_grid(block=B): surface following on blocks) in one process, one JSON line per
             (net, N, lipschitz): after a warm-up of both paths, --reps pairs of (dense, sparse), alternating; device events
             around the grid and around marching cubes of each; medians.  The sparse path's steps from device events at
             follow_surface's step boundaries: coarse decode, every round's decode, the index kernels, fill; the host's count
             reads (number and wall time); the fraction of grid points decoded, rounds, and whether the two meshes are identical.

Nets: `g6_trained` is the trained 4x64 net of tests/golden/g6_real_weights with a zero code; the others are seeded (nn.Linear
init) decoders of bench.py's NetworkSpecs with that spec's CodeLength, the output bias shifted so that the zero level set crosses
the grid.  Without --block, times are the best of --reps after one warm-up mesh.
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from deepsdf_amd.decoder import Decoder  # noqa: E402
from deepsdf_amd.mesh import marching_cubes, sdf_grid, write_ply  # noqa: E402


TRAINED = "g6_trained"          # the trained 4x64 net of tests/golden/g6_real_weights (the reference's shipped weights), zero code


def make_decoder(name):
    if name == TRAINED:
        from tests.golden_io import Golden
        g = Golden("g6_real_weights")
        dec = Decoder(g.meta["L"], **g.meta["net_specs"]).cuda().eval()
        dec.load_state_dict({k: v for k, v in g.group("params").items()})
        return dec, torch.zeros(g.meta["L"]).cuda()
    nw = bench.NETWORKS[name]
    L = nw["defaults"]["code_length"]
    torch.manual_seed(0)
    dec = Decoder(L, **nw["net"]).cuda().eval()
    z = (torch.randn(L, generator=torch.Generator().manual_seed(1)) / math.sqrt(L)).cuda()
    with torch.no_grad():
        y = sdf_grid(dec, z, 32, 32 ** 3)
        last = getattr(dec, f"lin{dec.spec.n_layers - 1}")
        last.bias -= torch.atanh(y.median())
    return dec, z


def one(dec, z, N, max_batch, path):
    h = 2.0 / (N - 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    grid = sdf_grid(dec, z, N, max_batch)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    v, f = marching_cubes(grid, 0.0, (h, h, h), (-1, -1, -1))
    e1.record()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    write_ply(path, v, f)
    t3 = time.perf_counter()
    return dict(decode_ms=(t1 - t0) * 1e3, mc_ms=e0.elapsed_time(e1), ply_ms=(t3 - t2) * 1e3, V=v.shape[0], F=f.shape[0])


def events_ms(fn):
    """(device-event milliseconds around fn(), its result)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


class StepTimer:
    """follow_surface's on_step: a device event and the host clock at every step boundary.  After a synchronise, steps() gives
    {coarse_decode, index, fill: ms summed over the run, decode_per_round: [ms]} (a step's time is what lies between the boundary
    before it and its own) and waits() the wall time of every count read."""
    INDEX = ("coarse", "seed", "emit", "grow")

    def __init__(self):
        self.marks = []

    def __call__(self, name, ws, plan, indices):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e, time.perf_counter()))

    def steps(self):
        out = dict(coarse_decode=0.0, index=0.0, fill=0.0, decode_per_round=[])
        for (_, e0, _), (name, e1, _) in zip(self.marks, self.marks[1:]):
            ms = e0.elapsed_time(e1)
            if name == "decode":
                out["decode_per_round"].append(ms)
            elif name in self.INDEX:
                out["index"] += ms
            elif name in ("coarse_decode", "fill"):
                out[name] += ms
        return out

    def waits(self):
        return [(t1 - t0) * 1e3 for (_, _, t0), (name, _, t1) in zip(self.marks, self.marks[1:]) if name == "wait"]


def sparse_summary(runs):
    """The JSON fields both benchmarks share, from runs = [dict(dense, sparse, mc, mc_sparse, steps, waits, stats, same, F)]."""
    med = statistics.median
    st = runs[-1]["stats"]
    d, s = med(r["dense"] for r in runs), med(r["sparse"] for r in runs)
    rounds = len(runs[-1]["steps"]["decode_per_round"])
    return dict(dense_ms=round(d, 3), sparse_ms=round(s, 3),
                sparse_min_max_ms=[round(min(r["sparse"] for r in runs), 3), round(max(r["sparse"] for r in runs), 3)],
                dense_over_sparse=round(d / s, 3), fraction_decoded=round(st["points"] / st["total"], 4), rounds=st["rounds"],
                blocks=st["blocks"], seeds=st["seeds"], active=st["active"],
                coarse_decode_ms=round(med(r["steps"]["coarse_decode"] for r in runs), 3),
                decode_ms_per_round=[round(med(r["steps"]["decode_per_round"][k] for r in runs), 3) for k in range(rounds)],
                index_ms=round(med(r["steps"]["index"] for r in runs), 3), fill_ms=round(med(r["steps"]["fill"] for r in runs), 3),
                mc_ms=round(med(r["mc"] for r in runs), 3), mc_sparse_ms=round(med(r["mc_sparse"] for r in runs), 3),
                host_waits=len(runs[-1]["waits"]), host_wait_ms=round(med(sum(r["waits"]) for r in runs), 3),
                meshes_identical=all(r["same"] for r in runs), F_dense=runs[-1]["F"][0], F_sparse=runs[-1]["F"][1])


def sparse_pair(dec, z, N, max_batch, block, lipschitz):
    """One dense and one sparse mesh, each timed as grid + marching cubes."""
    h = 2.0 / (N - 1)
    mc = lambda g: marching_cubes(g, 0.0, (h, h, h), (-1, -1, -1))                     # noqa: E731
    dense_ms, grid = events_ms(lambda: sdf_grid(dec, z, N, max_batch))
    mc_ms, (vd, fd) = events_ms(lambda: mc(grid))
    del grid
    stats, timer = {}, StepTimer()
    sparse_ms, grid = events_ms(lambda: sdf_grid(dec, z, N, max_batch, block=block, lipschitz=lipschitz, stats=stats, on_step=timer))
    mc2_ms, (vs, fs) = events_ms(lambda: mc(grid))
    same = vd.shape == vs.shape and fd.shape == fs.shape and bool(torch.equal(vd, vs)) and bool(torch.equal(fd, fs))
    return dict(dense=dense_ms + mc_ms, dense_decode=dense_ms, mc=mc_ms, sparse=sparse_ms + mc2_ms, mc_sparse=mc2_ms,
                steps=timer.steps(), waits=timer.waits(), stats=stats, same=same, F=(fd.shape[0], fs.shape[0]))


def sparse_bench(args):
    for name in args.nets:
        dec, z = make_decoder(name)
        for N in args.N:
            for lip in args.lipschitz:
                sparse_pair(dec, z, N, args.max_batch, args.block, lip)                # warms both paths
                runs = [sparse_pair(dec, z, N, args.max_batch, args.block, lip) for _ in range(args.reps)]
                dd = statistics.median(r["dense_decode"] for r in runs)
                frac = runs[-1]["stats"]["points"] / runs[-1]["stats"]["total"]
                print(json.dumps(dict(what="sparse", net=name, N=N, block=args.block, lipschitz=lip, max_batch=args.max_batch, reps=args.reps,
                                      dense_decode_ms=round(dd, 3), expected_ms_fraction_x_dense=round(frac * dd, 3),
                                      **sparse_summary(runs), device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["8x512", "4x64"], choices=sorted(bench.NETWORKS) + [TRAINED])
    ap.add_argument("--N", nargs="+", type=int, default=[128, 256])
    ap.add_argument("--max-batch", type=int, default=32 ** 3, help="decode chunk (create_mesh's max_batch)")
    ap.add_argument("--reps", type=int, default=None, help="default 3; 5 with --block")
    ap.add_argument("--block", type=int, default=None, help="compare the dense path with surface following on blocks of this edge")
    ap.add_argument("--lipschitz", nargs="+", type=float, default=[1.0, 0.0], help="with --block: the seeding slopes to run")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 5 if args.block else 3
    if args.block:
        return sparse_bench(args)
    with tempfile.TemporaryDirectory() as d:
        for name in args.nets:
            dec, z = make_decoder(name)
            for N in args.N:
                path = os.path.join(d, "m.ply")
                one(dec, z, N, args.max_batch, path)
                runs = [one(dec, z, N, args.max_batch, path) for _ in range(args.reps)]
                best = {k: min(r[k] for r in runs) for k in ("decode_ms", "mc_ms", "ply_ms")}
                tot = sum(best.values())
                print(json.dumps(dict(net=name, N=N, max_batch=args.max_batch, **{k: round(v, 3) for k, v in best.items()},
                                      decode_share=round(best["decode_ms"] / tot, 4), V=runs[-1]["V"], F=runs[-1]["F"],
                                      decode_mpts_s=round(N ** 3 / best["decode_ms"] / 1e3, 1),
                                      device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
