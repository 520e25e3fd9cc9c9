#!/usr/bin/env python3
"""Mesh every trained latent code of an experiment, and the interpolation sequence between codes 1..8 (the reference's
create_ply_files_from_latent.py, same flags -e / -c / -b, plus --resolution).

Every mesh goes through deep_sdf.mesh.create_mesh: grid decode on the GPU, HIP marching cubes, binary PLY.  Files:
``<experiment>/Reconstructions/<checkpoint>/Meshes/latent_recon/all/<i>.ply`` and
``.../latent_recon/interpolation/interpolate_<a>_<b>_<step>.ply``.

Deviation from the reference: the reference passed the file name with its suffix stripped to create_mesh, which wrote a
file WITHOUT ``.ply`` -- so its own "file exists, skip" check never fired.  Here the file is ``<instance>.ply``, and an
existing file is skipped.  With fewer than 9 codes the interpolation sequence (codes 1..8) is skipped with a message
instead of an IndexError.

    python create_ply_files_from_latent.py -e <experiment_dir> -c latest [-b 32] [--resolution 256]
"""
import datetime
import os
import pathlib
import time

import torch

import deep_sdf.mesh
import deep_sdf.workspace as ws

INTERP_INDICES = [1, 2, 3, 4, 5, 6, 7, 8]
INTERP_STEPS = 11


def _mesh(decoder, latent_in, fname, N, max_batch):
    fname = pathlib.Path(fname)
    os.makedirs(fname.parent, exist_ok=True)
    if fname.exists():
        print(f"Skipping {fname}")
        return False
    deep_sdf.mesh.create_mesh(decoder, latent_in, str(fname), N=N, max_batch=int(max_batch ** 3))
    return True


def main(experiment_directory, checkpoint, max_batch=32, resolution=256, block=None, lipschitz=1.0):
    if not torch.cuda.is_available():
        raise RuntimeError("create_ply_files_from_latent.py (deepsdf_amd) needs an AMD GPU: the HIP path has no CPU fallback")
    with deep_sdf.mesh.sparse_grid(block, lipschitz):
        _main(experiment_directory, checkpoint, max_batch, resolution)


def _main(experiment_directory, checkpoint, max_batch, resolution):
    decoder = ws.load_trained_model(experiment_directory, checkpoint)
    decoder.eval()
    latent = ws.load_latent_vectors(experiment_directory, checkpoint)

    for i, latent_in in enumerate(latent):
        fname = ws.get_reconstructed_mesh_filename(experiment_directory, checkpoint, "latent_recon", "all", f"{i}")
        print(f"Reconstructing {fname} ({i}/{len(latent)})")
        _mesh(decoder, latent_in, fname, resolution, max_batch)

    if len(latent) <= max(INTERP_INDICES):
        print(f"{len(latent)} latent codes: the interpolation sequence needs codes {INTERP_INDICES[0]}..{INTERP_INDICES[-1]}, skipped")
        return
    start = time.time()
    num_samples = (len(INTERP_INDICES) - 1) * INTERP_STEPS
    i_sample = 1
    for index1, index2 in zip(INTERP_INDICES[:-1], INTERP_INDICES[1:]):
        latent1, latent2 = latent[index1], latent[index2]
        for i in range(INTERP_STEPS):
            latent_in = latent1 + (latent2 - latent1) * i / (INTERP_STEPS - 1)
            fname = ws.get_reconstructed_mesh_filename(experiment_directory, checkpoint, "latent_recon", "interpolation",
                                                       f"interpolate_{index1}_{index2}_{i}")
            if not _mesh(decoder, latent_in, fname, resolution, max_batch):
                continue
            tot_time = time.time() - start
            avg = tot_time / i_sample
            remaining = str(datetime.timedelta(seconds=round(avg * (num_samples - i_sample))))
            print(f"Finished {i_sample} ({i_sample}/{num_samples}) [{i_sample / num_samples * 100:.2f}%] in {remaining} "
                  f"({avg:.2f}s/epoch)")
            i_sample += 1


def build_parser():
    import argparse

    parser = argparse.ArgumentParser(description="Write a PLY mesh for every latent code of a trained experiment.")
    parser.add_argument("--experiment_directory", "-e", type=str, required=True)
    parser.add_argument("--checkpoint", "-c", type=str, default="latest")
    parser.add_argument("--max_batch", "-b", type=int, default=32, help="decode chunk = max_batch^3 grid points")
    parser.add_argument("--resolution", type=int, default=256, help="grid points per axis (N of create_mesh)")
    deep_sdf.mesh.add_sparse_args(parser)
    return parser


if __name__ == "__main__":
    args = build_parser().parse_args()
    main(args.experiment_directory, args.checkpoint, args.max_batch, args.resolution, args.block, args.lipschitz)
