#!/usr/bin/env python3
"""Score reconstructions: the Chamfer distance of every reconstructed mesh of a split to its ground-truth surface samples.

The fork deleted upstream's evaluate.py and kept the metric (deep_sdf/metrics/chamfer.py) and the workspace layout it wrote
to; this script restores the step on the GPU (deepsdf_amd/metrics.py: HIP surface sampling and nearest neighbours, no trimesh,
no scipy).  For every instance ``<dataset>/<class>/<instance>`` of the split it reads

    <experiment>/Reconstructions/<checkpoint>/Meshes/<dataset>/<class>/<instance>.ply     (reconstruct.py --mesh)
    <data>/SurfaceSamples/<dataset>/<class>/<instance>.ply                               (vertex-only PLY)
    <data>/NormalizationParameters/<dataset>/<class>/<instance>.npz                       (offset, scale; identity if absent)

and writes ``<experiment>/Evaluation/<checkpoint>/chamfer.csv``: a first line ``shape, chamfer_dist``, then one line
``<dataset>/<class>/<instance>, <value>`` per instance.  A missing reconstruction is logged and skipped.

    python evaluate.py -e <experiment_dir> -c latest -d <data_dir> -s <split.json> [--samples 30000] [--seed 0] [--exact]
"""
import argparse
import json
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def reconstruction_epoch(experiment_directory, checkpoint):
    """The directory name under Reconstructions/: the checkpoint's name as upstream used it, or -- reconstruct.py's choice --
    the epoch stored in that checkpoint when only that directory exists."""
    import torch
    import deep_sdf.workspace as ws
    base = os.path.join(experiment_directory, ws.reconstructions_subdir)
    params = os.path.join(experiment_directory, ws.model_params_subdir, checkpoint + ".pth")
    if not os.path.isdir(os.path.join(base, str(checkpoint))) and os.path.isfile(params):
        epoch = torch.load(params, map_location="cpu", weights_only=True)["epoch"]
        if os.path.isdir(os.path.join(base, str(epoch))):
            return str(epoch)
    return str(checkpoint)


def evaluate(experiment_directory, checkpoint, data_dir, split_filename, samples=30000, seed=0, exact=False):
    """Writes chamfer.csv and returns [(shape, chamfer)] of the instances that could be scored."""
    import deep_sdf.workspace as ws
    from deepsdf_amd.meshsdf import read_mesh, read_points
    from deepsdf_amd.metrics import compute_trimesh_chamfer

    with open(split_filename) as f:
        split = json.load(f)
    epoch = reconstruction_epoch(experiment_directory, checkpoint)
    results, told_identity = [], False
    for dataset in split:
        for class_name in split[dataset]:
            for instance in split[dataset][class_name]:
                shape = f"{dataset}/{class_name}/{instance}"
                mesh_file = ws.get_reconstructed_mesh_filename(experiment_directory, epoch, dataset, class_name, instance)
                gt_file = os.path.join(data_dir, ws.surface_samples_subdir, dataset, class_name, instance + ".ply")
                if not os.path.isfile(mesh_file):
                    logging.warning("%s: no reconstruction at %s, skipped", shape, mesh_file)
                    continue
                if not os.path.isfile(gt_file):
                    logging.warning("%s: no surface samples at %s, skipped", shape, gt_file)
                    continue
                norm_file = ws.get_normalization_params_filename(data_dir, dataset, class_name, instance)
                offset, scale = np.zeros(3), 1.0
                if os.path.isfile(norm_file):
                    with np.load(norm_file) as norm:
                        offset, scale = np.asarray(norm["offset"], dtype=np.float64).reshape(3), float(np.asarray(norm["scale"]))
                elif not told_identity:
                    logging.info("no normalization parameters under %s: using offset 0, scale 1",
                                 os.path.join(data_dir, ws.normalization_param_subdir))
                    told_identity = True
                V, F = read_mesh(mesh_file)
                if len(F) == 0:
                    logging.warning("%s: the reconstruction has no faces, skipped", shape)
                    continue
                value = compute_trimesh_chamfer(read_points(gt_file), (V, F), offset, scale, num_mesh_samples=samples, seed=seed,
                                                exact=exact)
                logging.debug("%s: %.9g", shape, value)
                results.append((shape, value))
    out = os.path.join(ws.get_evaluation_dir(experiment_directory, str(checkpoint), True), "chamfer.csv")
    with open(out, "w") as f:
        f.write("shape, chamfer_dist\n")
        for shape, value in results:
            f.write(f"{shape}, {value!r}\n")
    return results, out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate reconstructed meshes: Chamfer distance to the ground-truth surface samples.")
    ap.add_argument("--experiment", "-e", dest="experiment_directory", required=True)
    ap.add_argument("--checkpoint", "-c", dest="checkpoint", default="latest")
    ap.add_argument("--data", "-d", dest="data_source", required=True)
    ap.add_argument("--split", "-s", dest="split_filename", required=True)
    ap.add_argument("--samples", type=int, default=30000, help="points drawn from every reconstructed mesh")
    ap.add_argument("--seed", type=int, default=0, help="seed of the surface samples")
    ap.add_argument("--exact", action="store_true",
                    help="ground truth -> reconstruction by the exact point-to-surface distance instead of sampled points")
    ap.add_argument("--debug", action="store_true", help="log every shape's value")
    ap.add_argument("--quiet", "-q", action="store_true", help="log warnings only")
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if a.debug else (logging.WARNING if a.quiet else logging.INFO),
                        format="evaluate - %(levelname)s - %(message)s")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate.py (deepsdf_amd) needs an AMD GPU: the HIP path has no CPU fallback")
    results, out = evaluate(a.experiment_directory, a.checkpoint, a.data_source, a.split_filename, a.samples, a.seed, a.exact)
    if results:
        values = np.array([v for _, v in results])
        print(f"{len(values)} shapes: mean chamfer {values.mean():.9g}, median {np.median(values):.9g}")
    else:
        print("0 shapes scored")
    print(f"-> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
