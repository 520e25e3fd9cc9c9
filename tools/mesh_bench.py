"""Time of one mesh (deepsdf_amd/mesh.py create_mesh) split into its three steps, one JSON line per (net, N):
decode (sdf_grid: the N^3 grid through Engine.decode_latent in max_batch chunks), marching cubes (HIP events around
dsdf_mc_count + the totals read + dsdf_mc_emit) and PLY write, with V and F.

    python tools/mesh_bench.py [--nets 8x512 4x64] [--N 128 256] [--max-batch 32768] [--reps 3]

Nets: seeded (nn.Linear init) decoders of bench.py's NetworkSpecs with that spec's CodeLength; the output bias is shifted
so that the zero level set crosses the grid.  Times are the best of --reps after one warm-up mesh.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from deepsdf_amd.decoder import Decoder  # noqa: E402
from deepsdf_amd.mesh import marching_cubes, sdf_grid, write_ply  # noqa: E402


def make_decoder(name):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nets", nargs="+", default=["8x512", "4x64"], choices=sorted(bench.NETWORKS))
    ap.add_argument("--N", nargs="+", type=int, default=[128, 256])
    ap.add_argument("--max-batch", type=int, default=32 ** 3, help="decode chunk (create_mesh's max_batch)")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
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
