#!/usr/bin/env python3
"""Record golden ws_totals.json: the workspace totals the library's planners answer with red zone 0.

Run ONCE at the commit whose layout is to be pinned (the one before the debug red zones existed), with the library built
from that commit.  Only the host-side size queries are called: no GPU is needed.  tests/test_abi_cpu.py requires the
current library to answer every recorded total byte for byte while the red zone is 0 -- "the default layout did not move".

Recorded per case: the NetSpec constructor arguments, N, R, K and
  train    dsdf_workspace_bytes(net, N, R)
  buckets  dsdf_workspace_bytes_buckets(net, N, R, K)
  decode   dsdf_decode_workspace_bytes(net, N)
and, net-free, dsdf_mc_workspace_bytes per grid and dsdf_msdf_plan (tri, ws, splits) per (faces, queries).

Usage:  python tests/golden/make_golden_ws_totals.py
"""
import ctypes as C
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

_WN = dict(dropout_prob=0.2, weight_norm=True)
NETS = {
    "8x512": dict(latent_size=256, dims=[512] * 8, geom_dimension=3, dropout=list(range(8)), norm_layers=list(range(8)),
                  latent_in=[4], **_WN),
    "8x512_bf16": dict(latent_size=256, dims=[512] * 8, geom_dimension=3, dropout=list(range(8)), norm_layers=list(range(8)),
                       latent_in=[4], forward_bf16=True, **_WN),
    "6x128": dict(latent_size=16, dims=[128] * 6, geom_dimension=3, dropout=list(range(6)), norm_layers=list(range(6)),
                  latent_in=[3], **_WN),
    "4x64": dict(latent_size=16, dims=[64] * 4, geom_dimension=3, dropout=list(range(4)), norm_layers=list(range(4)),
                 latent_in=[2], **_WN),
    "4x32": dict(latent_size=8, dims=[32] * 4, geom_dimension=3, latent_in=[2]),
    "3x640": dict(latent_size=8, dims=[640] * 3, geom_dimension=3),
    "ln": dict(latent_size=4, dims=[32] * 3, geom_dimension=3, norm_layers=[0, 1, 3], weight_norm=False),
    "xyz_in_all": dict(latent_size=4, dims=[32] * 3, geom_dimension=3, xyz_in_all=True, latent_in=[2]),
    "L1_g2": dict(latent_size=1, dims=[48] * 3, geom_dimension=2),
    "L512_g4": dict(latent_size=508, dims=[256] * 4, geom_dimension=4),
    "L256_skip": dict(latent_size=256, dims=[512, 512, 128], geom_dimension=3, latent_in=[2]),
    "L0": dict(latent_size=0, dims=[32] * 3, geom_dimension=3),
}
SHAPES = [(0, 0, 2), (1, 1, 2), (31, 1, 2), (64, 2, 4), (257, 3, 8), (4096, 64, 2), (8191, 3, 4), (8192, 64, 8), (8193, 512, 2),
          (16384, 64, 2), (16384, 64, 8), (65472, 2000, 2), (65536, 64, 4), (65600, 1, 2), (160000, 10, 2)]
MC_GRIDS = [(2, 2, 2), (3, 5, 7), (33, 33, 33), (64, 65, 66), (128, 128, 128)]
MSDF = [(1, 0), (1, 1), (12, 100000), (4096, 1), (4096, 255), (100000, 256), (100000, 257), (1000000, 64), (300, 5000)]


def record(lib, NetSpec):
    sz = C.c_size_t()
    out = {"nets": NETS, "cases": [], "mc": [], "msdf": []}
    for name, kw in NETS.items():
        net = NetSpec(**kw).c_struct()
        for N, R, K in SHAPES:
            rec = {"net": name, "N": N, "R": R, "K": K}
            assert lib.dsdf_workspace_bytes(C.byref(net), N, R, C.byref(sz)) == 0, lib.dsdf_last_error()
            rec["train"] = sz.value
            assert lib.dsdf_workspace_bytes_buckets(C.byref(net), N, R, K, C.byref(sz)) == 0, lib.dsdf_last_error()
            rec["buckets"] = sz.value
            assert lib.dsdf_decode_workspace_bytes(C.byref(net), N, C.byref(sz)) == 0, lib.dsdf_last_error()
            rec["decode"] = sz.value
            out["cases"].append(rec)
    for g in MC_GRIDS:
        assert lib.dsdf_mc_workspace_bytes(*g, C.byref(sz)) == 0, lib.dsdf_last_error()
        out["mc"].append({"grid": list(g), "bytes": sz.value})
    tri, ns = C.c_size_t(), C.c_int32()
    for nf, nq in MSDF:
        assert lib.dsdf_msdf_plan(nf, nq, C.byref(tri), C.byref(sz), C.byref(ns)) == 0, lib.dsdf_last_error()
        out["msdf"].append({"faces": nf, "queries": nq, "tri": tri.value, "ws": sz.value, "splits": ns.value})
    return out


def main():
    from deepsdf_amd import _lib
    from deepsdf_amd.net import NetSpec
    out = record(_lib.lib(), NetSpec)
    with open(os.path.join(HERE, "ws_totals.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote ws_totals.json:", len(out["cases"]), "net cases,", len(out["mc"]), "grids,", len(out["msdf"]), "mesh-sdf plans")


if __name__ == "__main__":
    main()
