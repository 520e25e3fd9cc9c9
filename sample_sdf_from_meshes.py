"""Mesh files -> DeepSDF training samples, on the GPU.

    python sample_sdf_from_meshes.py --data-dir data --dataset microstructure --class double_lattice \\
        --split double_lattice_3D.json [--samples 100000] [--strategy uniform] [--seed 0] [--force] [--surface-samples N] \\
        MESH [MESH ...]

Writes <data-dir>/SdfSamples/<dataset>/<class>/<class>_<10000 + i>.npz for the i-th mesh (in the order given) and the split
<data-dir>/splits/<split>, as the reference's data scripts do with SDFSampler(data/SdfSamples, data/splits) and one
SDFfromMesh per mesh.  An existing sample file is kept unless --force.  Prints one line per mesh: name, faces, and the time
spent drawing points, in the SDF kernel (upload and read-back included) and writing the file.

With --surface-samples N it also writes what evaluate.py reads: <data-dir>/SurfaceSamples/<dataset>/<class>/<instance>.ply, N
points drawn from the mesh's surface on the GPU (a vertex-only PLY; seeded by --seed, 0 if not given), and
<data-dir>/NormalizationParameters/<dataset>/<class>/<instance>.npz with the offset and scale this script applied to the mesh
(none: offset 0, scale 1).  Without the flag nothing changes.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def write_surface_samples(a, meshes, split):
    """The ground truth evaluate.py compares against: surface points and the (identity) normalization of every mesh."""
    from deepsdf_amd.mesh import write_points_ply
    from deepsdf_amd.meshsdf import TriangleMesh
    from deepsdf_amd.workspace import get_normalization_params_filename, surface_samples_subdir
    for (V, F), stem in zip(meshes, split):
        ply = os.path.join(a.data_dir, surface_samples_subdir, a.dataset, a.class_name, stem + ".ply")
        npz = get_normalization_params_filename(a.data_dir, a.dataset, a.class_name, stem)
        for path in (ply, npz):
            os.makedirs(os.path.dirname(path), exist_ok=True)
        if os.path.isfile(ply) and os.path.isfile(npz) and not a.force:
            print(f"{stem}: surface samples exist, kept")
            continue
        pts, _ = TriangleMesh(V, F).sample_surface(a.surface_samples, seed=a.seed or 0)
        write_points_ply(ply, pts)
        np.savez(npz, offset=np.zeros(3), scale=np.float64(1.0))
        print(f"{stem}: {a.surface_samples} surface samples -> {ply}")


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
    ap.add_argument("--surface-samples", type=int, default=0, metavar="N",
                    help="also write N surface points per mesh (SurfaceSamples) and its NormalizationParameters")
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
    if a.surface_samples > 0:
        write_surface_samples(a, meshes, split)
    print(f"split -> {os.path.join(splitdir, a.split)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
