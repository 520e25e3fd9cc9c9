#!/usr/bin/env python3
"""Mesh a tiled microstructure whose unit cells blend between trained latent codes (the reference's
evaluation_scripts/05_create_microstructure.py, as a command line).

A B-spline over the design domain [-1, 1]^3 carries the named trained codes as its control points (first axis fastest), the
domain is tiled with mirrored unit cells, the borders are capped and the zero level set is written as a binary PLY -- all through
deep_sdf.mesh.create_mesh_microstructure: rows, decode, caps and marching cubes on the GPU.

    python create_microstructure.py -e <experiment_dir> -c latest --tiling 4 4 2 --codes 0 3 1 2 5 5 7 8 \\
        [--degrees 1 1 1] [--resolution 256] [--cap x1=1:0.1 z0=-1:0] [-b 32] [--jacobian out.npz] \\
        [--tetmesh out.mesh [--t-clamp 0.05]] -o out.ply

With degrees p the number of codes must be a product nx * ny * nz of control points per axis, each > p; the split is taken
from --control-points, or for 8 codes 2 x 2 x 2.  Knot vectors are uniform and clamped.

--jacobian FILE.npz also writes the mesh with its derivative with respect to the control points: verts [V, 3], faces [F, 3],
jac [V, ncp, L] = d verts[v, axis[v]] / d control points, axis [V] (the other two coordinates of a vertex do not depend on them).

--tetmesh FILE.mesh also writes the solid as a tetrahedral mesh in MFEM mesh v1.0 format, in the PLY's coordinates
(deep_sdf.mesh.tetrahedralize of the same capped grid, which is decoded once for both files); --t-clamp bounds how thin a cut
element can get.  --jacobian decodes the structure once more (microstructure_mesh_diff keeps the raw and the capped grid).
"""
import argparse

import numpy as np
import torch

import deep_sdf.mesh
import deep_sdf.workspace as ws
from deepsdf_amd.spline import BSplineField


def uniform_clamped_knots(n, p):
    inner = np.linspace(-1.0, 1.0, n - p + 1)[1:-1]
    return [-1.0] * (p + 1) + [float(u) for u in inner] + [1.0] * (p + 1)


def parse_caps(items):
    """["x1=1:0.1", ...] -> {"x1": {"cap": 1, "measure": 0.1}, ...} in the order given; None without --cap (the defaults)."""
    if not items:
        return None
    caps = {}
    for it in items:
        try:
            loc, rest = it.split("=")
            cap, measure = rest.split(":")
            caps[loc] = {"cap": int(cap), "measure": float(measure)}
        except ValueError:
            raise SystemExit(f"--cap {it!r}: expected <face>=<cap>:<measure>, e.g. x1=1:0.1")
        if loc not in deep_sdf.mesh.location_lookup:
            raise SystemExit(f"--cap {it!r}: face must be one of {list(deep_sdf.mesh.location_lookup)}")
    return caps


def main(experiment_directory, checkpoint, tiling, codes, out, degrees=(1, 1, 1), control_points=None, resolution=256,
         caps=None, max_batch=32, jacobian=None, block=None, lipschitz=1.0, tetmesh=None, t_clamp=0.0):
    if not torch.cuda.is_available():
        raise RuntimeError("create_microstructure.py (deepsdf_amd) needs an AMD GPU: the HIP path has no CPU fallback")
    decoder = ws.load_trained_model(experiment_directory, checkpoint)
    decoder.eval()
    latent = ws.load_latent_vectors(experiment_directory, checkpoint)
    if control_points is None:
        if len(codes) != 8:
            raise SystemExit(f"{len(codes)} codes: say how they split over the axes with --control-points nx ny nz")
        control_points = [2, 2, 2]
    if int(np.prod(control_points)) != len(codes):
        raise SystemExit(f"--control-points {control_points} needs {int(np.prod(control_points))} codes, got {len(codes)}")
    bad = [c for c in codes if not 0 <= c < len(latent)]
    if bad:
        raise SystemExit(f"codes {bad} outside the experiment's {len(latent)} latent codes")
    cp = torch.stack([latent[c].detach().reshape(-1).cpu() for c in codes]).numpy()
    field = BSplineField(degrees, [uniform_clamped_knots(n, p) for n, p in zip(control_points, degrees)], cp)
    name = out[:-4] if out.endswith(".ply") else out
    if tetmesh:                                   # one decode of the structure for the surface and the volume mesh
        m = deep_sdf.mesh.microstructure_tetmesh(list(tiling), decoder, field, resolution, int(max_batch ** 3), caps, t_clamp=t_clamp,
                                                 block=block, lipschitz=lipschitz, ply_filename=name + ".ply")
        m.write_mfem(tetmesh)
        print(f"wrote {tetmesh}: {m.n_verts} vertices, {m.n_tets} elements, {m.n_bfaces} boundary triangles")
    else:
        with deep_sdf.mesh.sparse_grid(block, lipschitz):
            deep_sdf.mesh.create_mesh_microstructure(list(tiling), decoder, field, name, N=resolution, max_batch=int(max_batch ** 3),
                                                     cap_border_dict=caps, save_ply_file=True)
    print(f"wrote {name}.ply")
    if jacobian:
        d = deep_sdf.mesh.microstructure_mesh_diff(list(tiling), decoder, field, resolution, int(max_batch ** 3), caps, block=block,
                                                   lipschitz=lipschitz)
        jac, axis = d.jacobian()
        np.savez(jacobian, verts=d.verts.cpu().numpy(), faces=d.faces.cpu().numpy(), jac=jac.cpu().numpy(), axis=axis.cpu().numpy())
        print(f"wrote {jacobian}")


def build_parser():
    parser = argparse.ArgumentParser(description="Write the PLY mesh of a tiled microstructure over trained latent codes.")
    parser.add_argument("--experiment_directory", "-e", type=str, required=True)
    parser.add_argument("--checkpoint", "-c", type=str, default="latest")
    parser.add_argument("--tiling", type=int, nargs=3, required=True, metavar=("TX", "TY", "TZ"))
    parser.add_argument("--codes", type=int, nargs="+", required=True, help="indices of trained codes, first axis fastest")
    parser.add_argument("--degrees", type=int, nargs=3, default=[1, 1, 1])
    parser.add_argument("--control-points", type=int, nargs=3, default=None, metavar=("NX", "NY", "NZ"))
    parser.add_argument("--resolution", type=int, default=256, help="grid points per axis (N of create_mesh_microstructure)")
    parser.add_argument("--cap", type=str, nargs="*", default=None, help="<face>=<cap>:<measure>, e.g. x1=1:0.1; in order")
    parser.add_argument("--max_batch", "-b", type=int, default=32, help="decode chunk = max_batch^3 grid points")
    parser.add_argument("--jacobian", type=str, default=None, metavar="FILE.npz",
                        help="also write verts, faces, jac [V, ncp, L] (d vertex / d control points along axis) and axis; decodes the "
                             "structure a second time")
    parser.add_argument("--tetmesh", type=str, default=None, metavar="FILE.mesh",
                        help="also write the solid as a tetrahedral MFEM mesh v1.0 file, in the PLY's coordinates (from the PLY's grid: no "
                             "second decode)")
    parser.add_argument("--t-clamp", type=float, default=0.0, help="clamp of the edge parameter in [0, 0.5) (--tetmesh)")
    parser.add_argument("--output", "-o", type=str, required=True)
    deep_sdf.mesh.add_sparse_args(parser)
    return parser


if __name__ == "__main__":
    args = build_parser().parse_args()
    main(args.experiment_directory, args.checkpoint, args.tiling, args.codes, args.output, args.degrees, args.control_points,
         args.resolution, parse_caps(args.cap), args.max_batch, args.jacobian, args.block, args.lipschitz, args.tetmesh, args.t_clamp)
