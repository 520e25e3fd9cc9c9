#!/usr/bin/env python3
"""Generate golden g13 (tests/golden/g13_sdf_sampler.npz) from the REFERENCE's sdf_sampler/sdf_sampler.py.

Runs ONLY where the reference tree is available (REF below).  The reference module is imported by file path; the third-party
modules it imports at the top and never calls on these paths (igl, trimesh, gustaf, skimage) are registered as empty stub
modules first, as for the decoder goldens.  Recorded, all as data:
  - random_sample_sdf(BoxSDF(0.5), (-1, 1), 257, type) for uniform / plane / spherical_gaussian after np.random.seed(SEED),
    and random_points_cube(100, 1.5) after the same seed;
  - BoxSDF, SummedSDF (also through +), NegatedCallable (also through unary -) on 64 fixed queries, and the pos / neg / summed
    stacks of RandomSampleSDF.split_pos_neg;
  - the pos / neg arrays of the two files SDFSampler.sample_sdfs writes for two analytic SDFs (seeded, 2000 uniform samples) and
    the split JSON write_json writes, with the split list.
tests/test_meshsdf_cpu.py requires the port (deepsdf_amd/sdf_sampler.py) to reproduce every array bit for bit, dtypes included.

Usage:  python tests/golden/make_golden_sdf_sampler.py
"""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SEED = 13


def reference_module():
    for name in ("igl", "trimesh", "gustaf", "skimage", "skimage.measure"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["skimage"].measure = sys.modules["skimage.measure"]
    spec = importlib.util.spec_from_file_location("ref_sdf_sampler", os.path.join(REF, "sdf_sampler", "sdf_sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = reference_module()
    out = {"seed": np.array(SEED)}
    for kind in ("uniform", "plane", "spherical_gaussian"):
        np.random.seed(SEED)
        r = ref.random_sample_sdf(ref.BoxSDF(0.5), (-1, 1), 257, type=kind)
        out[f"draw_{kind}_samples"], out[f"draw_{kind}_distances"] = r.samples, r.distances
    np.random.seed(SEED)
    out["cube_points"] = ref.random_points_cube(100, 1.5)

    q = np.random.default_rng(SEED).uniform(-1, 1, (64, 3))
    out["queries"] = q
    a, b = ref.BoxSDF(0.5), ref.BoxSDF(0.25, np.array([0.3, -0.2, 0.1]))
    for name, f in (("box", a), ("box2", b), ("sum", a + b), ("sum_cls", ref.SummedSDF(a, b)), ("neg", -a),
                    ("neg_cls", ref.NegatedCallable(b))):
        out[f"sdf_{name}"] = f(q)
    pos, neg = ref.RandomSampleSDF(q, a(q)).split_pos_neg()
    out["split_pos"], out["split_neg"], out["split_sum"] = pos.stacked, neg.stacked, (pos + neg).stacked

    meta = {"dataset": "analytic", "class": "boxes", "n_samples": 2000, "split_name": "boxes.json"}
    with tempfile.TemporaryDirectory() as d:
        sampler = ref.SDFSampler(os.path.join(d, "SdfSamples"), os.path.join(d, "splits"))
        os.makedirs(os.path.join(d, "splits"))
        info = {"dataset_name": meta["dataset"], "class_name": meta["class"]}
        np.random.seed(SEED)
        sdfs = [ref.BoxSDF(0.5), ref.BoxSDF(0.3, np.array([0.1, 0.2, -0.1])) + ref.BoxSDF(0.2)]
        split = sampler.sample_sdfs(sdfs, info, n_samples=float(meta["n_samples"]), sampling_strategy="uniform")
        sampler.write_json(meta["split_name"], info, split)
        meta["split"] = split
        with open(os.path.join(d, "splits", meta["split_name"])) as fh:
            meta["split_json"] = fh.read()
        for i, stem in enumerate(split):
            with np.load(os.path.join(d, "SdfSamples", meta["dataset"], meta["class"], stem + ".npz")) as z:
                out[f"file{i}_pos"], out[f"file{i}_neg"] = z["pos"], z["neg"]
    out["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(os.path.join(HERE, "g13_sdf_sampler.npz"), **out)
    print("wrote g13_sdf_sampler")


if __name__ == "__main__":
    main()
