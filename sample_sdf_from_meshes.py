"""Mesh files -> DeepSDF training samples, on the GPU.

    python sample_sdf_from_meshes.py --data-dir data --dataset microstructure --class double_lattice \\
        --split double_lattice_3D.json [--samples 100000] [--strategy uniform] [--seed 0] [--force] MESH [MESH ...]

Writes <data-dir>/SdfSamples/<dataset>/<class>/<class>_<10000 + i>.npz for the i-th mesh (in the order given) and the split
<data-dir>/splits/<split>, as the reference's data scripts do with SDFSampler(data/SdfSamples, data/splits) and one
SDFfromMesh per mesh.  An existing sample file is kept unless --force.  Prints one line per mesh: name, faces, and the time
spent drawing points, in the SDF kernel (upload and read-back included) and writing the file.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--class", dest="class_name", required=True)
    ap.add_argument("--split", required=True, help="split file name, written under <data-dir>/splits")
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--strategy", default="uniform", choices=["uniform", "plane", "spherical_gaussian"])
    ap.add_argument("--seed", type=int, default=None, help="np.random.seed before sampling (default: not seeded)")
    ap.add_argument("--force", action="store_true", help="overwrite existing sample files")
    ap.add_argument("meshes", nargs="+", metavar="MESH", help=".ply or .obj files")
    a = ap.parse_args(argv)

    from deepsdf_amd.meshsdf import read_mesh
    from deepsdf_amd.sdf_sampler import SDFfromMesh, SDFSampler

    outdir, splitdir = os.path.join(a.data_dir, "SdfSamples"), os.path.join(a.data_dir, "splits")
    os.makedirs(splitdir, exist_ok=True)
    info = {"dataset_name": a.dataset, "class_name": a.class_name}
    meshes = [read_mesh(m) for m in a.meshes]
    if a.force:
        for i in range(len(meshes)):
            f = os.path.join(outdir, a.dataset, a.class_name, f"{a.class_name}_{10000 + i}.npz")
            if os.path.isfile(f):
                os.remove(f)
    if a.seed is not None:
        np.random.seed(a.seed)
    sampler = SDFSampler(outdir, splitdir)
    split = sampler.sample_sdfs([SDFfromMesh(m) for m in meshes], info, n_samples=a.samples, sampling_strategy=a.strategy)
    sampler.write_json(a.split, info, split)
    done = {t["index"]: t for t in sampler.timings}
    for i, (path, (V, F)) in enumerate(zip(a.meshes, meshes)):
        t = done.get(i)
        if t is None:
            print(f"{os.path.basename(path)}: {len(F)} faces -> {split[i]}.npz (exists, kept)")
        else:
            print(f"{os.path.basename(path)}: {len(F)} faces -> {t['name']}: sampling {t['sample_s'] * 1e3:.1f} ms, "
                  f"kernel {t['sdf_s'] * 1e3:.1f} ms, write {t['write_s'] * 1e3:.1f} ms")
    print(f"split -> {os.path.join(splitdir, a.split)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
