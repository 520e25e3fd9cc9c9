"""Training data from SDFs: the API of the reference's ``sdf_sampler/sdf_sampler.py`` with the mesh distance on the GPU.

Same names, signatures and semantics as the reference module (analytic helpers :21-69, ``RandomSampleSDF`` :81-107,
``SDFSampler.sample_sdfs`` / ``write_json`` :109-157, ``noisy_sample`` :164-167, ``random_sample_sdf`` :187-199, ``SDFfromMesh`` :201-242).
``random_sample_sdf`` makes the same ``np.random`` calls in the same order, so a seeded run draws the reference's points bit
for bit, and ``sample_sdfs`` writes the same files (``<class>_<10000 + i>.npz`` with float64 ``pos`` / ``neg`` rows).

``SDFfromMesh`` needs neither igl nor trimesh: distance and sign come from ``deepsdf_amd.meshsdf.TriangleMesh`` (HIP, brute
force; the sign is the parity of the generalized winding number, the ray-parity answer of the reference's embree test on
closed meshes).  Plotting (``show=True``, ``create_gus_plottable``) needs gustaf, which this package does not require.
"""
import datetime
import json
import logging
import os
import pathlib
import time
import typing
from abc import ABC, abstractmethod

import numpy as np
import numpy.typing as npt

logger = logging.getLogger(__name__)


def _gustaf():
    try:
        import gustaf
    except ImportError:
        raise ImportError("plotting samples needs gustaf, which is not installed") from None
    return gustaf


class SDFBase(ABC):
    @abstractmethod
    def __call__(self, queries: npt.ArrayLike) -> npt.ArrayLike:
        """Signed distances [n, 1] of queries [n, 3]."""

    def __add__(self, other):
        return SummedSDF(self, other)

    def __neg__(self):
        return NegatedCallable(self)


class SummedSDF(ABC):
    """Union of two SDFs: the pointwise minimum (written -max(-a, -b), as the reference)."""

    def __init__(self, obj1, obj2):
        self.obj1 = obj1
        self.obj2 = obj2

    def __call__(self, input_param):
        a, b = self.obj1(input_param), self.obj2(input_param)
        return -np.maximum(-a, -b)             # the reference's expression, so results match it bit for bit


class NegatedCallable(SDFBase):
    def __init__(self, obj):
        self.obj = obj

    def __call__(self, input_param):
        return -self.obj(input_param)


class BoxSDF(SDFBase):
    """Chebyshev distance to `center` minus `box_size` (the reference's box, exact on the axes only)."""

    def __init__(self, box_size: float = 1, center: npt.ArrayLike = np.array([0, 0, 0])):
        self.box_size = box_size
        self.center = center

    def __call__(self, queries: npt.ArrayLike) -> npt.ArrayLike:
        chebyshev = np.abs(np.asarray(queries) - self.center).max(axis=1)
        return (chebyshev - self.box_size).reshape(-1, 1)


class DataSetInfo(typing.TypedDict):
    dataset_name: str
    class_name: str


class SphereParameters(typing.TypedDict):
    cx: float
    cy: float
    cz: float
    r: float


class RandomSampleSDF:
    samples: npt.ArrayLike
    distances: npt.ArrayLike

    def __init__(self, samples, distances):
        self.samples = samples
        self.distances = distances

    def split_pos_neg(self):
        """(pos, neg): distances >= 0 go to pos, < 0 to neg (NaN to neither)."""
        d = self.distances
        rows = (np.where(d >= 0.0)[0], np.where(d < 0.0)[0])
        return tuple(RandomSampleSDF(samples=self.samples[r], distances=d[r]) for r in rows)

    def create_gus_plottable(self):
        gus = _gustaf()
        vp = gus.Vertices(vertices=self.samples)
        vp.vertex_data["distance"] = self.distances
        return vp

    @property
    def stacked(self):
        return np.hstack((self.samples, self.distances))

    def __add__(self, other):
        return RandomSampleSDF(samples=np.vstack((self.samples, other.samples)),
                               distances=np.vstack((self.distances, other.distances)))


class _TimedSDF:
    """Wraps an SDF and accumulates the wall time of its calls (SDFSampler.timings)."""

    def __init__(self, sdf):
        self.sdf, self.seconds = sdf, 0.0

    def __call__(self, queries):
        t = time.perf_counter()
        out = self.sdf(queries)
        self.seconds += time.perf_counter() - t
        return out


class SDFSampler:
    def __init__(self, outdir, splitdir) -> None:
        self.outdir = outdir
        self.splitdir = splitdir
        self.timings = []     # one dict per file written by the last sample_sdfs: index, name, sample_s, sdf_s, write_s

    def sample_sdfs(self, sdfs, data_set_info: DataSetInfo, show=False, n_samples: int = 1e5, sampling_strategy="uniform",
                    clamp_distance=0.1, box_size=None, stds=[0.0025, 0.00025]) -> list:
        """Writes <outdir>/<dataset>/<class>/<class>_<10000 + i>.npz for every SDF (an existing file is kept unless show) and
        returns the split list of their stems.  clamp_distance, box_size and stds are accepted and unused, as in the
        reference."""
        cls = data_set_info["class_name"]
        folder = pathlib.Path(f"{self.outdir}/{data_set_info['dataset_name']}/{cls}")
        begin = time.time()
        self.timings = []
        stems = []
        for i, sdf in enumerate(sdfs):
            path = folder / f"{cls}_{10000 + i}.npz"
            stems.append(path.stem)
            os.makedirs(folder, exist_ok=True)
            if path.is_file() and not show:
                continue
            t0 = time.perf_counter()
            timed = _TimedSDF(sdf)
            drawn = random_sample_sdf(timed, bounds=(-1, 1), n_samples=int(n_samples), type=sampling_strategy)
            t1 = time.perf_counter()
            pos, neg = drawn.split_pos_neg()
            if show:
                self._show(pos, neg)
            np.savez(path, neg=neg.stacked, pos=pos.stacked)
            t2 = time.perf_counter()
            self.timings.append(dict(index=i, name=str(path), sample_s=t1 - t0 - timed.seconds, sdf_s=timed.seconds,
                                     write_s=t2 - t1))
            n_done = i + 1
            per_file = (time.time() - begin) / n_done
            eta = datetime.timedelta(seconds=round(per_file * (len(sdfs) - n_done)))
            print(f"Sampling {path} ({n_done}/{len(sdfs)}) [{n_done / len(sdfs) * 100:.2f}%] in {eta} ({per_file:.2f}s/file)")
        return stems

    @staticmethod
    def _show(pos, neg):
        try:
            gus = _gustaf()
        except ImportError as e:
            logger.warning("show=True: %s; the samples are written without a plot", e)
            return
        vp_pos = pos.create_gus_plottable()
        vp_neg = neg.create_gus_plottable()
        for vp in (vp_pos, vp_neg):
            vp.show_options["cmap"] = "coolwarm"
            vp.show_options["vmin"] = -0.1
            vp.show_options["vmax"] = 0.1
        gus.show(vp_neg, vp_pos)

    def write_json(self, json_fname, data_info, split_files):
        """<splitdir>/<json_fname>: {dataset: {class: split_files}}, indented by 4 (the split file train_deep_sdf.py reads)."""
        with open(pathlib.Path(f"{self.splitdir}/{json_fname}"), "w") as fh:
            json.dump({data_info["dataset_name"]: {data_info["class_name"]: split_files}}, fh, indent=4)


def random_points_cube(count, box_size):
    """count points drawn uniformly (one np.random.uniform call) from the axis-aligned cube of edge box_size around the
    origin."""
    half = box_size / 2
    return np.random.uniform(-half, half, (int(count), 3))


def random_sample_sdf(sdf, bounds, n_samples, type="uniform"):
    """n_samples points drawn with np.random ("uniform" in the bounds cube, "plane": z = 0, "spherical_gaussian": unit-sphere
    directions plus N(0, 0.01) noise) and their distances sdf(points)."""
    lo, hi, n = bounds[0], bounds[1], n_samples
    if type == "uniform":
        pts = np.random.uniform(lo, hi, (n, 3))
    elif type == "plane":
        pts = np.hstack((np.random.uniform(lo, hi, (n, 2)), np.zeros((n, 1))))
    elif type == "spherical_gaussian":
        dirs = np.random.randn(n, 3)
        dirs /= np.linalg.norm(dirs, axis=1).reshape(-1, 1)
        pts = dirs + np.random.normal(0, 0.01, (n, 3))
    else:
        raise ValueError(f"unknown sampling type {type!r} (uniform, plane, spherical_gaussian)")
    return RandomSampleSDF(samples=pts, distances=sdf(pts))


def _mesh_arrays(mesh):
    if isinstance(mesh, (str, os.PathLike)):
        from .meshsdf import read_mesh
        return read_mesh(mesh)
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        return np.asarray(mesh.vertices), np.asarray(mesh.faces)
    if isinstance(mesh, (tuple, list)) and len(mesh) == 2:
        return mesh
    raise TypeError("SDFfromMesh needs an object with .vertices / .faces, a (V, F) pair or a .ply / .obj path")


def noisy_sample(mesh, std, count, seed=0):
    """count points of the mesh's surface plus N(0, std^2) noise per coordinate, float64 [count, 3] -- the reference's helper of
    this name (:164-167: trimesh's ``mesh.sample`` plus ``np.random.normal``), drawn on the GPU from `seed` instead of numpy's
    global state.  mesh: what SDFfromMesh takes, or a deepsdf_amd.meshsdf.TriangleMesh."""
    from .meshsdf import TriangleMesh
    tm = mesh if isinstance(mesh, TriangleMesh) else TriangleMesh(*_mesh_arrays(mesh))
    return tm.sample_surface(int(count), seed=seed, std=float(std))[0].cpu().numpy().astype(np.float64)


class SDFfromMesh(SDFBase):
    def __init__(self, mesh, dtype=np.float32, flip_sign=False):
        """Signed distance to a triangle mesh, negative inside.

        mesh: an object with .vertices / .faces (trimesh, gustaf), a (V, F) pair or a .ply / .obj path.  The mesh is uploaded
        and prepared once, on first use.  flip_sign is stored and, unlike the reference (which stores it and never applies
        it), negates the result when set."""
        self.mesh = mesh
        self.dtype = dtype
        self.flip_sign = flip_sign
        self._tm = None

    def triangle_mesh(self):
        if self._tm is None:
            from .meshsdf import TriangleMesh
            V, F = _mesh_arrays(self.mesh)
            self._tm = TriangleMesh(V, F)
        return self._tm

    def __call__(self, queries):
        d = self.triangle_mesh().sdf(np.asarray(queries), flip_sign=self.flip_sign)
        return d.astype(self.dtype, copy=False).reshape(-1, 1)
