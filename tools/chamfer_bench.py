"""Nearest-neighbour and Chamfer throughput (csrc/pointset.hpp through dsdf_nn_query), one JSON line per case, written to --out
and stdout.

    python tools/chamfer_bench.py [--out profiles/chamfer_bench.log] [--reps 5]

Cases: the 1e6 x 1e5 nearest-neighbour query and the 30000 x 30000 one (one direction of the Chamfer case), each next to the
yardstick -- dsdf_msdf_query in distance-only mode with the same number of queries against a triangle soup of as many faces
as there are reference points (its pair test contains the nearest-neighbour one) -- then one 30000 x 30000 chamfer_distance
call end to end (two queries, two means, the read-back) and, where scipy imports, the same work through
scipy.spatial.cKDTree on the host (build + query, up to 16 worker threads).

ms: HIP events around one call (outputs and workspace allocated beforehand), best of --reps after 2 warm-up calls; the
end-to-end and host cases by the host clock around a call that ends in a device synchronise / on the host.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from deepsdf_amd import _lib, metrics  # noqa: E402
from deepsdf_amd._lib import ptr as _ptr, stream as _stream  # noqa: E402
from deepsdf_amd.meshsdf import TriangleMesh  # noqa: E402


def best_ms(call, reps):
    for _ in range(2):
        call()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return min(times)


def time_nn(Q, R, reps):
    lib = _lib.lib()
    nq, nr = Q.shape[0], R.shape[0]
    wb, ns = metrics.plan(nq, nr)
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    d2 = torch.empty(nq, dtype=torch.float32, device="cuda")
    idx = torch.empty(nq, dtype=torch.int32, device="cuda")
    return best_ms(lambda: _lib.check(lib.dsdf_nn_query(_ptr(Q), nq, _ptr(R), nr, _ptr(d2), _ptr(idx), _ptr(ws), ws.numel(),
                                                        _stream())), reps), ns


def time_msdf_distance(Q, n_faces, reps, gen):
    """The yardstick: distance-only mesh SDF against a soup of n_faces small triangles in the unit cube."""
    lib = _lib.lib()
    a = torch.rand(n_faces, 1, 3, generator=gen) * 2 - 1
    V = (a + (torch.rand(n_faces, 3, 3, generator=gen) - 0.5) * 0.05).reshape(-1, 3)
    m = TriangleMesh(V, torch.arange(3 * n_faces).reshape(-1, 3))
    nq = Q.shape[0]
    wb, ns = m.plan(nq)
    ws = torch.empty(max(wb, 1), dtype=torch.uint8, device="cuda")
    d2 = torch.empty(nq, dtype=torch.float32, device="cuda")
    face = torch.empty(nq, dtype=torch.int32, device="cuda")
    return best_ms(lambda: _lib.check(lib.dsdf_msdf_query(_ptr(m.tri), m.n_faces, _ptr(Q), nq, None, _ptr(d2), _ptr(face), None,
                                                          None, 0, _ptr(ws), ws.numel(), _stream())), reps), ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chamfer_bench.log"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.cuda.get_device_name(0)
    gen = torch.Generator().manual_seed(0)
    lines = []

    def emit(**kw):
        lines.append(dict(kw, device=dev))
        print(json.dumps(lines[-1]), flush=True)

    for nq, nr in ((1000000, 100000), (30000, 30000)):
        Q = (torch.rand(nq, 3, generator=gen) * 2 - 1).cuda()
        R = (torch.rand(nr, 3, generator=gen) * 2 - 1).cuda()
        ms, ns = time_nn(Q, R, a.reps)
        emit(case="nearest_neighbour", queries=nq, refs=nr, splits=ns, ms=round(ms, 3), gpairs_s=round(nq * nr / ms / 1e6, 2))
        ms, ns = time_msdf_distance(Q, nr, a.reps, gen)
        emit(case="msdf_distance_only", queries=nq, faces=nr, splits=ns, ms=round(ms, 3), gpairs_s=round(nq * nr / ms / 1e6, 2))
    A = (torch.rand(30000, 3, generator=gen) * 2 - 1).cuda()
    B = (torch.rand(30000, 3, generator=gen) * 2 - 1).cuda()
    for _ in range(2):
        value = metrics.chamfer_distance(A, B)
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value = metrics.chamfer_distance(A, B)             # float(): ends in a read-back
        times.append((time.perf_counter() - t0) * 1e3)
    emit(case="chamfer_30000x30000_end_to_end", ms=round(min(times), 3), gpairs_s=round(2 * 30000 * 30000 / min(times) / 1e6, 2),
         value=value)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        emit(case="ckdtree_host", note="scipy does not import: not measured")
    else:
        An, Bn = A.cpu().numpy(), B.cpu().numpy()
        cpus = min(16, len(os.sched_getaffinity(0)))
        t0 = time.perf_counter()
        host = float(np.mean(cKDTree(Bn).query(An, workers=cpus)[0] ** 2) + np.mean(cKDTree(An).query(Bn, workers=cpus)[0] ** 2))
        ms = (time.perf_counter() - t0) * 1e3
        emit(case="ckdtree_host_chamfer_30000x30000", ms=round(ms, 3), value=host, rel_diff_to_gpu=abs(host - value) / host,
             cpus=cpus)
        Qn = (torch.rand(1000000, 3, generator=gen) * 2 - 1).numpy()
        Rn = (torch.rand(100000, 3, generator=gen) * 2 - 1).numpy()
        t0 = time.perf_counter()
        cKDTree(Rn).query(Qn, workers=cpus)
        ms = (time.perf_counter() - t0) * 1e3
        emit(case="ckdtree_host_nearest_neighbour", queries=1000000, refs=100000, ms=round(ms, 3), cpus=cpus)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.writelines(json.dumps(x) + "\n" for x in lines)


if __name__ == "__main__":
    main()
