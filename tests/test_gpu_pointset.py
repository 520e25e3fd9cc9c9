"""-m gpu: the point-set kernels (dsdf_nn_*, dsdf_mean_f64, dsdf_surf_*; deepsdf_amd/metrics.py, TriangleMesh.sample_surface)
against the numpy oracle of tests/pointset_numpy.py; split and call determinism; the Chamfer distance end to end; the
sampling and evaluation command lines."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mc_numpy
from tests import meshsdf_numpy as mn
from tests import pointset_numpy as pn
from tests import ws_guard

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = ws_guard.constants()                         # the planners' break points, read from the kernel sources
NN_TILE = K["NN_BLOCK"] * K["NN_QPL"]            # queries per workgroup
SURF_TILE = K["SURF_BLOCK"] * K["SURF_PER_LANE"]  # faces per workgroup of the scan
SOUP_SEED = 13                                   # tests/test_pointset_cpu.py checks this seed's margins and shares on the CPU


def _mc_sphere(n, radius):
    """Marching-cubes mesh of |x| - radius on an n^3 grid over [-1, 1]^3."""
    from deepsdf_amd.mesh import marching_cubes
    ax = torch.linspace(-1, 1, n, dtype=torch.float64)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    f = (torch.sqrt(x * x + y * y + z * z) - radius).to(torch.float32).cuda()
    h = 2.0 / (n - 1)
    v, fc = marching_cubes(f, 0.0, (h, h, h), (-1, -1, -1))
    return v.cpu().numpy().astype(np.float64), fc.cpu().numpy().astype(np.int64)


def _first_nr_with_splits(nq, want):
    """The smallest reference count for which dsdf_nn_plan answers `want` splits (the split count is monotone in it)."""
    from deepsdf_amd.metrics import plan
    lo, hi = 1, 1 << 20
    assert plan(nq, hi)[1] >= want
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if plan(nq, mid)[1] >= want else (mid + 1, hi)
    assert plan(nq, lo)[1] == want and (lo == 1 or plan(nq, lo - 1)[1] == want - 1)
    return lo


# ---- nearest neighbour ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 255, 256, 257, 1000])
def test_nearest_neighbour_matches_the_oracle(nq):
    from deepsdf_amd.metrics import nearest_neighbor, plan
    b2, b3 = _first_nr_with_splits(256, 2), _first_nr_with_splits(256, 3)
    g = np.random.default_rng(100 + nq)
    Q = g.uniform(-1, 1, (nq, 3))
    Rall = g.uniform(-1, 1, (b3 + 1, 3))
    seen = set()
    for nr in (1, 2, b2 - 1, b2, b2 + 1, b3 - 1, b3, b3 + 1):
        R = Rall[:nr]
        d2, idx = nearest_neighbor(Q, R)
        assert d2.dtype == np.float32 and idx.dtype == np.int32 and d2.shape == (nq,) and idx.shape == (nq,)
        ref, _ = pn.nn_bruteforce(Q, R)
        err = np.abs(d2 - ref) / ref
        back = pn.pair_d2(Q, R, idx) / ref
        print(f"nq {nq} nr {nr} splits {plan(nq, nr)[1]}: max rel err {err.max():.2e}, returned pair / min {back.max():.9f}")
        assert idx.min() >= 0 and idx.max() < nr
        assert np.all(np.abs(d2 - ref) <= 1e-6 * ref), (nr, err.max())
        assert np.all(pn.pair_d2(Q, R, idx) <= ref * (1 + 1e-6)), (nr, back.max())
        seen.add(plan(nq, nr)[1])
    assert seen == {1, 2, 3}


def test_nearest_neighbour_is_exact_on_dyadic_points():
    """Coordinates k / 64 in [-2, 2]: every d2 is exact in fp32, so values are bit-equal to the oracle and the index is the
    oracle's lowest -- also across splits, where a duplicate in split 1 must lose against its original in split 0."""
    from deepsdf_amd.metrics import nearest_neighbor, plan
    g = np.random.default_rng(7)
    for want in (1, 2, 3):
        nr = _first_nr_with_splits(256, want) + (77 if want > 1 else 900)
        assert plan(1000, nr)[1] == want
        R = g.integers(-128, 129, (nr, 3)) / 64.0
        Q = g.integers(-128, 129, (1000, 3)) / 64.0
        chunk = -(-nr // want)
        if want > 1:
            R[chunk + 5] = R[3]                  # split 1 repeats a point of split 0 ...
            R[nr - 1] = R[chunk - 1]             # ... and the last split the last point of split 0
            Q[0], Q[1] = R[3], R[chunk - 1]      # queries AT the duplicated points: distance 0 on both sides of the cut
        Q[2:200] = R[g.integers(0, nr, 198)] + g.integers(-1, 2, (198, 3)) / 64.0       # many near ties
        d2, idx = nearest_neighbor(Q, R)
        ref, ridx = pn.nn_bruteforce(Q, R)
        assert np.array_equal(d2.astype(np.float64), ref), want
        assert np.array_equal(idx, ridx), want
        if want > 1:
            assert idx[0] <= 3 and idx[1] <= chunk - 1 and d2[0] == 0 and d2[1] == 0
        ties = int(((((Q[:200, None, :] - R[None]) ** 2).sum(2) == ref[:200, None]).sum(1) > 1).sum())
        assert ties >= (2 if want > 1 else 0), ties               # the case really holds queries with several nearest points


def test_nearest_neighbour_determinism_outputs_and_errors():
    from deepsdf_amd.metrics import nearest_neighbor, plan
    nr = _first_nr_with_splits(256, 3) + 28
    g = torch.Generator().manual_seed(5)
    big = 2047 * 1024 + 1                                                  # one split: the query tiles alone fill the launch
    assert plan(1000, nr)[1] == 3 and plan(big, nr)[1] == 1
    Q = (torch.rand(big, 3, generator=g) * 2 - 1).cuda()
    R = (torch.rand(nr, 3, generator=g) * 2 - 1).cuda()
    a = nearest_neighbor(Q[:1000], R)
    b = nearest_neighbor(Q, R)
    assert a[0].is_cuda and a[1].dtype == torch.int32
    assert torch.equal(a[0], b[0][:1000]) and torch.equal(a[1], b[1][:1000])          # the split does not show
    a2 = nearest_neighbor(Q[:1000], R)
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])                      # nor does the call
    d_only, none = nearest_neighbor(Q[:1000], R, index=False)
    none2, i_only = nearest_neighbor(Q[:1000], R, sqr_dist=False)
    assert none is None and none2 is None and torch.equal(d_only, a[0]) and torch.equal(i_only, a[1])
    d1, i1 = nearest_neighbor(Q[:300], R[:50], index=False)[0], nearest_neighbor(Q[:300], R[:50], sqr_dist=False)[1]
    both = nearest_neighbor(Q[:300], R[:50])
    assert torch.equal(d1, both[0]) and torch.equal(i1, both[1])                      # one split: the query kernel writes them
    # numpy in, numpy out; cpu tensor in, cpu tensor out; no queries
    qn, rn = Q[:300].cpu().numpy(), R.cpu().numpy()
    dn, idn = nearest_neighbor(qn, rn)
    assert isinstance(dn, np.ndarray) and np.array_equal(dn, a[0][:300].cpu().numpy()) and np.array_equal(idn, a[1][:300].cpu().numpy())
    dc, _ = nearest_neighbor(Q[:300].cpu(), R.cpu())
    assert dc.device.type == "cpu"
    d0, i0 = nearest_neighbor(np.zeros((0, 3)), rn)
    assert d0.shape == (0,) and i0.shape == (0,)
    # a NaN reference point is never chosen
    rn2 = rn.copy()
    rn2[0] = np.nan
    dn2, idn2 = nearest_neighbor(qn, rn2)
    ref, ridx = pn.nn_bruteforce(qn, rn[1:])
    assert np.array_equal(idn2, ridx + 1) and np.all(np.abs(dn2 - ref) <= 1e-6 * ref)
    with pytest.raises(ValueError):
        nearest_neighbor(qn, np.zeros((0, 3)))
    with pytest.raises(ValueError):
        nearest_neighbor(qn, rn, sqr_dist=False, index=False)
    with pytest.raises(ValueError):
        nearest_neighbor(np.zeros((5, 2)), rn)
    with pytest.raises(ValueError):
        nearest_neighbor(qn, np.zeros((5, 4)))



def _check_nn(Q, R, d2, idx, what):
    """Every query against the fp64 brute force, under the tolerances of test_nearest_neighbour_matches_the_oracle."""
    ref, _ = pn.nn_bruteforce(Q, R, block=64)
    err = np.abs(d2 - ref) / ref
    back = pn.pair_d2(Q, R, idx) / ref
    print(f"{what}: max rel err {err.max():.2e}, returned pair / min {back.max():.9f}")
    assert idx.min() >= 0 and idx.max() < len(R)
    assert np.all(np.abs(d2 - ref) <= 1e-6 * ref), (what, err.max())
    assert np.all(pn.pair_d2(Q, R, idx) <= ref * (1 + 1e-6)), (what, back.max())


@pytest.mark.parametrize("nq", [1023, 1024, 1025, 2049])
def test_nearest_neighbour_query_tile_tails(nq):
    """One query short of a tile, a full tile, one into the second, one into the third: every query against the oracle, with one
    split (the query kernel writes the outputs) and with three (partials and the combine pass)."""
    from deepsdf_amd.metrics import nearest_neighbor, plan
    assert NN_TILE == 1024
    g = np.random.default_rng(300 + nq)
    Q = g.uniform(-1, 1, (nq, 3))
    for want, nr in ((1, 900), (3, 3 * K["NN_MIN_SPLIT_REFS"] + 77)):
        assert plan(nq, nr)[1] == want
        R = g.uniform(-1, 1, (nr, 3))
        d2, idx = nearest_neighbor(Q, R)
        assert d2.shape == (nq,) and idx.shape == (nq,)
        _check_nn(Q, R, d2, idx, f"nq {nq} nr {nr} splits {want}")


@pytest.mark.parametrize("nq,nr,want", [(300, 65535, 63), (300, 65536, 64), (300, 65536 + 77, 64), (300, 131072 + 5, 64),
                                        (1025, 65536 + 77, 64)])
def test_nearest_neighbour_at_the_split_cap_is_exact_on_dyadic_points(nq, nr, want):
    """Up to and beyond NN_MAX_SPLITS splits, on coordinates k / 64 (every d2 exact in fp32): values and indices are the oracle's
    bit for bit.  The LAST split repeats points of split 0 and queries sit AT them, so the lowest index has to win through every
    partial of the combine pass."""
    from deepsdf_amd.metrics import nearest_neighbor, plan
    assert K["NN_MAX_SPLITS"] == 64 and plan(nq, nr)[1] == want
    g = np.random.default_rng(nr + nq)
    R = g.integers(-128, 129, (nr, 3)) / 64.0
    Q = g.integers(-128, 129, (nq, 3)) / 64.0
    chunk = -(-nr // want)
    last = (want - 1) * chunk
    assert last + 5 < nr - 1
    R[last + 5] = R[3]                       # the last split repeats a point of split 0 ...
    R[nr - 1] = R[chunk - 1]                 # ... and, as its last point, the last point of split 0
    Q[0], Q[1] = R[3], R[chunk - 1]
    Q[2:200] = R[g.integers(0, nr, 198)] + g.integers(-1, 2, (198, 3)) / 64.0       # many near ties
    d2, idx = nearest_neighbor(Q, R)
    ref, ridx = pn.nn_bruteforce(Q, R, block=32)
    print(f"nq {nq} nr {nr} splits {want}: {int((idx != ridx).sum())} indices and {int((d2.astype(np.float64) != ref).sum())} values differ")
    assert np.array_equal(d2.astype(np.float64), ref)
    assert np.array_equal(idx, ridx)
    assert idx[0] <= 3 and idx[1] <= chunk - 1 and d2[0] == 0 and d2[1] == 0


def test_nearest_neighbour_split_count_bound_by_the_query_tiles():
    """513 query tiles leave room for ceil(2048 / 513) = 4 splits although the reference set would allow 8: the tile-bound branch
    of the planner.  A sample of the queries against the oracle; all of them against a second call and against a one-split call."""
    from deepsdf_amd.metrics import nearest_neighbor, plan
    nq, nr = 512 * NN_TILE + 3, 8 * K["NN_MIN_SPLIT_REFS"] + 1
    tiles = -(-nq // NN_TILE)
    assert (nq, nr, tiles) == (524291, 8193, 513)
    assert plan(nq, nr)[1] == -(-K["NN_TARGET_WG"] // tiles) == 4 < nr // K["NN_MIN_SPLIT_REFS"]
    big = (K["NN_TARGET_WG"] - 1) * NN_TILE + 1
    assert plan(big, nr)[1] == 1
    gen = torch.Generator().manual_seed(17)
    Q = (torch.rand(big, 3, generator=gen) * 2 - 1).cuda()
    R = (torch.rand(nr, 3, generator=gen) * 2 - 1).cuda()
    a = nearest_neighbor(Q[:nq], R)
    a2 = nearest_neighbor(Q[:nq], R)
    one = nearest_neighbor(Q, R)
    assert torch.equal(a[0], a2[0]) and torch.equal(a[1], a2[1])
    assert torch.equal(a[0], one[0][:nq]) and torch.equal(a[1], one[1][:nq])
    others = np.random.default_rng(17).choice(np.arange(NN_TILE, nq - 1027), 1000, replace=False)
    sel = np.concatenate([np.arange(NN_TILE), np.sort(others), np.arange(nq - 1027, nq)])
    st = torch.from_numpy(sel).cuda()
    _check_nn(Q[st].cpu().numpy(), R.cpu().numpy(), a[0][st].cpu().numpy(), a[1][st].cpu().numpy(), f"{len(sel)} of {nq} queries")


def test_nearest_neighbour_without_a_comparable_pair():
    """include/dsdf.h: a query with no comparable reference point (every d2 NaN or +inf) reports (+inf, 0) -- index 0, not the
    first index of some split.  Three splits, both outputs."""
    from deepsdf_amd.metrics import nearest_neighbor, plan
    nq, nr = 300, 3 * K["NN_MIN_SPLIT_REFS"] + 5
    assert plan(nq, nr)[1] == 3
    chunk = -(-nr // 3)
    g = np.random.default_rng(23)
    Q, R = g.uniform(-1, 1, (nq, 3)), g.uniform(-1, 1, (nr, 3))
    inf = np.float32(np.inf)

    def nothing(d2, idx, rows):
        assert d2.dtype == np.float32 and np.array_equal(d2[rows], np.full(len(d2[rows]), inf)), d2[rows][:8]
        assert np.array_equal(idx[rows], np.zeros(len(idx[rows]), np.int32)), idx[rows][:8]

    Qn = Q.copy()
    Qn[7, 1] = np.nan                                    # a NaN query: one coordinate, and all three
    Qn[299] = np.nan
    d2, idx = nearest_neighbor(Qn, R)
    nothing(d2, idx, [7, 299])
    keep = np.setdiff1d(np.arange(nq), [7, 299])
    _check_nn(Qn[keep], R, d2[keep], idx[keep], "the other queries")
    d2, idx = nearest_neighbor(Q, np.full((nr, 3), np.nan))      # every reference point NaN
    nothing(d2, idx, np.arange(nq))
    Ri = np.full((nr, 3), np.nan)                        # the only points that are not NaN sit at +inf, none of them in split 0
    Ri[chunk + 3] = [np.inf, 0.25, -0.5]
    Ri[2 * chunk + 1] = np.inf
    Ri[nr - 1] = [0.0, np.inf, np.inf]
    d2, idx = nearest_neighbor(Q, Ri)
    nothing(d2, idx, np.arange(nq))
    for dead in range(3):                                # one split all NaN: the answer comes from the two others
        Rd = R.copy()
        Rd[dead * chunk:min(nr, (dead + 1) * chunk)] = np.nan
        alive = np.nonzero(~np.isnan(Rd[:, 0]))[0]
        d2, idx = nearest_neighbor(Q, Rd)
        ref, ridx = pn.nn_bruteforce(Q, Rd[alive])
        assert np.array_equal(idx, alive[ridx]), dead
        assert np.all(np.abs(d2 - ref) <= 1e-6 * ref), dead


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_mean_f64(n):
    from deepsdf_amd.metrics import mean_f64
    x = (torch.rand(n, generator=torch.Generator().manual_seed(n)) * 3 + 0.01).cuda()
    m1, m2 = mean_f64(x), mean_f64(x)
    assert m1.dtype == torch.float64 and m1.is_cuda
    ref = x.cpu().numpy().astype(np.float64).mean()
    print(f"n {n}: mean {m1.item()!r} numpy {ref!r} rel diff {abs(m1.item() - ref) / ref:.2e}")
    assert abs(m1.item() - ref) <= n * 2.0 ** -53 * ref
    assert m1.item() == m2.item()
    with pytest.raises(ValueError):
        mean_f64(x[:0])


def _mean_plan(n):
    """(workgroups, values per workgroup) of dsdf_mean_f64, as include/dsdf.h states them."""
    blocks = min(-(-n // K["MEAN_MIN_SLICE"]), K["MEAN_MAX_BLOCKS"])
    return blocks, -(-n // blocks)


# n, workgroups, slice: one workgroup up to 4096 values; two from 4097; 257 partials send the final pass's loop round a second
# time; all 1024 workgroups at the smallest slice; a slice above it, with a short last one
@pytest.mark.parametrize("n,blocks,slice_", [(4095, 1, 4095), (4096, 1, 4096), (4097, 2, 2049), (256 * 4096 + 1, 257, 4081),
                                             (1024 * 4096, 1024, 4096), (1024 * 4096 + 1025, 1024, 4098)])
def test_mean_f64_at_the_planner_break_points(n, blocks, slice_):
    from deepsdf_amd.metrics import mean_f64
    assert (K["MEAN_MIN_SLICE"], K["MEAN_MAX_BLOCKS"], K["MEAN_BLOCK"]) == (4096, 1024, 256) and _mean_plan(n) == (blocks, slice_)
    assert (blocks - 1) * slice_ < n <= blocks * slice_            # every workgroup has values; the last may be short
    x = torch.rand(n, generator=torch.Generator().manual_seed(n)) * 3 + 0.01
    ref = math.fsum(x.tolist()) / n
    xd = x.cuda()
    m1, m2 = mean_f64(xd).item(), mean_f64(xd).item()
    print(f"n {n} ({blocks} x {slice_}): mean {m1!r} exact {ref!r} rel diff {abs(m1 - ref) / ref:.2e}")
    assert abs(m1 - ref) <= n * 2.0 ** -53 * ref
    assert m1 == m2


def test_mean_f64_never_accumulates_in_fp32():
    """2^22 + 1025 values, all 1 + 2^-23: every partial sum k (1 + 2^-23), k < 2^23, is exact in fp64 (47 bits), so the mean is
    1 + 2^-23 exactly; an fp32 accumulation anywhere loses the low bit."""
    from deepsdf_amd.metrics import mean_f64
    n = 2 ** 22 + 1025
    assert _mean_plan(n) == (1024, 4098)
    one = 1.0 + 2.0 ** -23
    x = torch.full((n,), one, dtype=torch.float32).cuda()
    assert x[0].item() == one
    assert mean_f64(x).item() == one


# ---- surface sampler --------------------------------------------------------------------------------------------------------
def _areas_are_the_specification(name, V, F, area32, power=True):
    """The prepare pass's fp32 areas equal pn.face_areas_f32 bit for bit; the count of differing areas and their distance are
    printed first.  power: a contracted cross product would give at least a tenth of the faces another area."""
    want = pn.face_areas_f32(V, F)
    if power:
        d = int((want.view(np.uint32) != pn.face_areas_f32(V, F, contracted=True).view(np.uint32)).sum())
        print(f"{name}: a contracted cross product would change {d} of {len(F)} areas")
        assert d >= 0.1 * len(F), (name, d)
    d, n = mc_numpy.differing(area32, want)
    print(f"{name}: {d} of {n} areas differ from the single-rounded specification, by at most {mc_numpy.ulp_distance(area32, want)} ulp")
    assert d == 0, (name, d, n)


def _six_face_mesh():
    """Four triangles of different areas with two zero-area faces between them (a repeated vertex; three collinear vertices)."""
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5], [2, 0, 0], [0, 0, 2], [0.25, 3, 1], [-1, -1, 0.75]], dtype=np.float64)
    F = np.array([[0, 1, 2], [3, 3, 5], [1, 3, 2], [1, 4, 3], [0, 1, 4], [5, 6, 7]])
    return V, F


@pytest.mark.parametrize("name,seed", [("mc_sphere", 11), ("six_faces", 12)])
def test_sampler_matches_the_oracle(name, seed):
    from deepsdf_amd.meshsdf import TriangleMesh
    V, F = _mc_sphere(24, 0.6) if name == "mc_sphere" else _six_face_mesh()
    n = 4096
    m = TriangleMesh(V, F)
    area32, cdf = (t.cpu().numpy() for t in m.face_areas())
    exact = pn.face_areas(V, F)
    assert np.abs(area32 - exact).max() <= 1e-5 * exact.max()
    _areas_are_the_specification(name, V, F, area32, power=name == "mc_sphere")      # six_faces is dyadic: its products are exact
    # the scan: deterministic and within n_faces * 2^-53 * total of the exact prefix sums
    want, ext = pn.exact_cdf(area32)
    total = want[-1]
    scan_err = np.abs(cdf.astype(np.longdouble) - ext).max()
    print(f"{name}: {len(F)} faces, total {total!r}, scan error / total {float(scan_err) / total:.2e}")
    assert scan_err <= len(F) * 2.0 ** -53 * total
    assert np.all(np.diff(cdf) >= 0)
    assert abs(m.area() - total) <= len(F) * 2.0 ** -53 * total
    assert np.array_equal(TriangleMesh(V, F).face_areas()[1].cpu().numpy(), cdf)
    pts, face, bary = (t.cpu().numpy() for t in m.sample_surface(n, seed=seed, return_bary=True))
    assert pts.dtype == np.float32 and face.dtype == np.int32 and pts.shape == (n, 3) and bary.shape == (n, 2)
    o = pn.surface_samples(V, F, area32, n, seed)
    assert o["margin"].min() > 1e-12, o["margin"].min()        # the oracle alone: no sample sits in the undecided band
    assert np.array_equal(face, o["face"])
    assert np.array_equal(bary[:, 0], o["u"]) and np.array_equal(bary[:, 1], o["v"])
    extent = np.abs(V).max()
    perr = np.abs(pts - o["point"]).max()
    print(f"{name}: max point error {perr:.2e} (extent {extent})")
    assert perr <= 1e-6 * extent
    assert np.all(area32[face] > 0)
    if name == "six_faces":
        assert area32.tolist()[1] == 0 and area32.tolist()[4] == 0 and set(np.unique(face)) == {0, 2, 3, 5}
    pts2, face2 = m.sample_surface(n, seed=seed)
    assert np.array_equal(pts2.cpu().numpy(), pts) and np.array_equal(face2.cpu().numpy(), face)
    other = m.sample_surface(n, seed=seed + 1)[0].cpu().numpy()
    assert not np.array_equal(other, pts)


def test_face_without_area_between_two_real_faces_is_never_drawn():
    """The face (0, d, 2 d) with a non-dyadic d: its two products per normal component round alike, so the specification's area is
    exactly 0 and the face is never chosen; a contracted cross product leaves it a rounding error of area and a place in the CDF."""
    from deepsdf_amd.meshsdf import TriangleMesh
    V, F = pn.sliver_between_faces()
    assert pn.face_areas_f32(V, F)[1] == 0.0 and pn.face_areas_f32(V, F, contracted=True)[1] > 0.0
    m = TriangleMesh(V, F)
    area32, cdf = (t.cpu().numpy() for t in m.face_areas())
    print(f"area of the face without area: {area32[1]!r}")
    _areas_are_the_specification("sliver", V, F, area32)
    assert area32[1] == 0.0 and cdf[1] == cdf[0] and np.all(np.diff(cdf) >= 0)
    face = m.sample_surface(65536, seed=3)[1].cpu().numpy()
    assert set(np.unique(face)) == {0, 2}


def _surf_tiles(nf):
    from deepsdf_amd import _lib
    nt = C.c_int32()
    _lib.check(_lib.lib().dsdf_surf_plan(nf, None, None, C.byref(nt)))
    return nt.value


@pytest.mark.parametrize("nf", [1023, 1024, 1025, pn.SOUP_SPLIT, pn.SOUP_SPLIT + 1, pn.SOUP_SPLIT + 1025])
def test_scan_and_sampler_at_the_tile_break_points(nf):
    """A seeded triangle soup cut around one scan tile (1024 faces) and around 256 of them, where the scan of the tile sums goes
    round its carry loop a second time; there the faces behind the first 256 tiles carry half of the area, so that carry decides
    half of the samples."""
    from deepsdf_amd.meshsdf import TriangleMesh
    assert SURF_TILE == 1024 and pn.SOUP_SPLIT == K["SURF_BLOCK"] * SURF_TILE
    tiles = _surf_tiles(nf)
    assert tiles == -(-nf // SURF_TILE) and (tiles > K["SURF_BLOCK"]) == (nf > pn.SOUP_SPLIT)
    V, F = pn.triangle_soup(nf, SOUP_SEED, heavy_tail=True)
    m = TriangleMesh(V, F)
    area32, cdf = (t.cpu().numpy() for t in m.face_areas())
    _areas_are_the_specification(f"soup {nf}", V, F, area32)
    want, ext = pn.exact_cdf(area32)
    total = want[-1]
    scan_err = np.abs(cdf.astype(np.longdouble) - ext).max()
    print(f"soup {nf}: {tiles} tiles, total {total!r}, scan error / total {float(scan_err) / total:.2e}")
    assert scan_err <= nf * 2.0 ** -53 * total
    assert np.all(np.diff(cdf) >= 0)
    assert m.area() == cdf[-1]
    n = 4096
    pts, face, bary = (t.cpu().numpy() for t in m.sample_surface(n, seed=SOUP_SEED, return_bary=True))
    o = pn.surface_samples(V, F, area32, n, SOUP_SEED)
    assert o["margin"].min() > 1e-12, o["margin"].min()        # the oracle alone: no sample sits in the undecided band
    behind = float((o["face"] >= pn.SOUP_SPLIT).mean())
    print(f"soup {nf}: share of the samples behind the first 256 tiles {behind:.3f}, smallest margin {o['margin'].min():.2e}")
    if nf > pn.SOUP_SPLIT:
        assert behind >= 0.25
    assert np.array_equal(face, o["face"])
    assert np.array_equal(bary[:, 0], o["u"]) and np.array_equal(bary[:, 1], o["v"])
    extent = np.abs(V).max()
    perr = np.abs(pts - o["point"]).max()
    print(f"soup {nf}: max point error {perr:.2e} (extent {extent})")
    assert perr <= 1e-6 * extent


def test_sampler_statistics():
    from deepsdf_amd.meshsdf import TriangleMesh
    V = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 1], [3, 0, 1], [0, 2, 1]], dtype=np.float64)      # areas 1 and 3
    F = np.array([[0, 1, 2], [3, 4, 5]])
    m = TriangleMesh(V, F)
    assert m.area() == 4.0
    n = 65536
    _, face, bary = (t.cpu().numpy() for t in m.sample_surface(n, seed=2024, return_bary=True))
    share = (face == 1).mean()
    mu = bary.astype(np.float64).mean(axis=0)
    print(f"share of the large face {share:.5f}, mean barycentrics {mu}")
    assert abs(share - 0.75) <= 0.0085                        # 5 sigma, sigma = sqrt(0.75 * 0.25 / n)
    assert np.all(np.abs(mu - 1 / 3) <= 0.0046)              # 5 sigma, sigma = sqrt(1 / 18 / n)
    assert (bary >= 0).all() and (bary.sum(axis=1) <= 1 + 2.0 ** -23).all()


def test_sampler_offset_noise_and_errors():
    from deepsdf_amd.meshsdf import TriangleMesh
    from deepsdf_amd.sdf_sampler import noisy_sample
    V, F = mn.icosphere(2, 0.8)
    m = TriangleMesh(V, F)
    n = 65536
    one = [t.cpu().numpy() for t in m.sample_surface(2 * n, seed=9, return_bary=True)]
    lo = [t.cpu().numpy() for t in m.sample_surface(n, seed=9, return_bary=True)]
    hi = [t.cpu().numpy() for t in m.sample_surface(n, seed=9, return_bary=True, offset=n)]
    for a, b, c in zip(one, lo, hi):
        assert np.array_equal(a[:n], b) and np.array_equal(a[n:], c)
    far = (1 << 32) - 1000                                    # the counter's second index word
    x = m.sample_surface(2000, seed=9, offset=far)[0].cpu().numpy()
    y = m.sample_surface(1000, seed=9, offset=far + 1000)[0].cpu().numpy()
    assert np.array_equal(x[1000:], y)
    clean = m.sample_surface(n, seed=9, std=0.0)[0].cpu().numpy()
    assert np.array_equal(clean, lo[0])                       # std = 0: no bit changes
    noisy = m.sample_surface(n, seed=9, std=0.01)[0].cpu().numpy()
    d = noisy.astype(np.float64) - clean
    print("noise mean", d.mean(axis=0), "std", d.std(axis=0))
    assert np.all(np.abs(d.mean(axis=0)) <= 5 * 0.01 / math.sqrt(n))
    assert np.all(np.abs(d.std(axis=0) - 0.01) <= 5 * 0.01 / math.sqrt(2 * n))
    assert abs(np.corrcoef(d[:, 0], d[:, 1])[0, 1]) <= 5 / math.sqrt(n)
    ns = noisy_sample((V, F), 0.01, 3000, seed=9)
    assert ns.dtype == np.float64 and np.array_equal(ns, noisy[:3000].astype(np.float64))
    assert m.sample_surface(0)[0].shape == (0, 3)
    flat = TriangleMesh(np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=np.float64), np.array([[0, 1, 2]]))
    with pytest.raises(ValueError):
        flat.sample_surface(10)
    with pytest.raises(ValueError):
        m.sample_surface(10, std=-1.0)


# ---- Chamfer distance -------------------------------------------------------------------------------------------------------
def test_chamfer_end_to_end():
    from deepsdf_amd.meshsdf import TriangleMesh
    from deepsdf_amd.metrics import chamfer_distance, compute_trimesh_chamfer, mean_f64, nearest_neighbor
    n, delta2 = 20000, 0.0025
    Va, Fa = _mc_sphere(48, 0.50)
    Vb, Fb = _mc_sphere(48, 0.55)
    ma, mb = TriangleMesh(Va, Fa), TriangleMesh(Vb, Fb)
    for m in (ma, mb):                                        # the sampling floor of one direction: inputs fit for the bounds below
        assert m.area() / (math.pi * n) < 0.03 * delta2
    gt = ma.sample_surface(n, seed=1)[0]
    zero, one = np.zeros(3), 1.0
    exact_dir = float(mean_f64(mb.squared_distance(gt)[0]))
    print(f"gt -> gen exact {exact_dir:.6e} (delta^2 {delta2})")
    assert abs(exact_dir - delta2) <= 0.05 * delta2
    sampled = compute_trimesh_chamfer(gt, (Vb, Fb), zero, one, num_mesh_samples=n, seed=2)
    exact = compute_trimesh_chamfer(gt, (Vb, Fb), zero, one, num_mesh_samples=n, seed=2, exact=True)
    print(f"chamfer sampled {sampled:.6e} exact {exact:.6e} (2 delta^2 {2 * delta2})")
    assert 2 * delta2 <= sampled <= 2 * delta2 * 1.10
    gen = mb.sample_surface(n, seed=2)[0]
    assert sampled == chamfer_distance(gt, gen)
    gen_to_gt = float(mean_f64(nearest_neighbor(gen, gt, index=False)[0]))
    assert exact == exact_dir + gen_to_gt and exact < sampled      # exact=True swaps one direction and nothing else

    class Cloud:
        vertices = gt.cpu().numpy()
    assert compute_trimesh_chamfer(Cloud(), (Vb, Fb), zero, one, num_mesh_samples=n, seed=2) == sampled
    assert chamfer_distance(gt, gt) == 0.0
    # p / scale - offset: the mesh scaled by 2 with scale = 2 is the same mesh; a shifted one comes back by its offset
    scaled = compute_trimesh_chamfer(gt, (Vb * 2, Fb), zero, 2.0, num_mesh_samples=n, seed=2)
    assert abs(scaled - sampled) <= 1e-6 * sampled
    off = np.array([0.25, -0.5, 0.125])
    moved = compute_trimesh_chamfer(gt, ((Vb + off) * 2, Fb), off, 2.0, num_mesh_samples=n, seed=2)
    assert abs(moved - sampled) <= 1e-4 * sampled


def test_sampling_and_evaluation_cli(tmp_path):
    import deep_sdf.workspace as ws
    from deepsdf_amd.mesh import write_ply
    from deepsdf_amd.meshsdf import read_points
    V, F = mn.icosphere(2, 0.5)
    write_ply(str(tmp_path / "ball.ply"), V.astype(np.float32), F.astype(np.int32))
    data, exp = tmp_path / "data", tmp_path / "exp"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sample_sdf_from_meshes.py"), "--data-dir", str(data), "--dataset", "ds",
                        "--class", "shapes", "--split", "shapes.json", "--samples", "2000", "--seed", "0", "--surface-samples", "2000",
                        str(tmp_path / "ball.ply")], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    gt = read_points(str(data / "SurfaceSamples" / "ds" / "shapes" / "shapes_10000.ply"))
    assert gt.shape == (2000, 3) and np.abs(np.linalg.norm(gt, axis=1) - 0.5).max() < 0.02
    with np.load(ws.get_normalization_params_filename(str(data), "ds", "shapes", "shapes_10000")) as z:
        assert np.array_equal(z["offset"], np.zeros(3)) and float(z["scale"]) == 1.0
    rec = ws.get_reconstructed_mesh_filename(str(exp), "latest", "ds", "shapes", "shapes_10000")
    os.makedirs(os.path.dirname(rec))
    write_ply(rec, V.astype(np.float32), F.astype(np.int32))
    split = {"ds": {"shapes": ["shapes_10000", "shapes_missing"]}}                     # the second has no reconstruction: skipped
    json.dump(split, open(tmp_path / "eval.json", "w"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "-e", str(exp), "-c", "latest", "-d", str(data), "-s",
                        str(tmp_path / "eval.json"), "--samples", "2000", "--seed", "1"], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mean chamfer" in r.stdout and "median" in r.stdout and "shapes_missing" in r.stderr
    lines = open(exp / "Evaluation" / "latest" / "chamfer.csv").read().splitlines()
    assert lines[0] == "shape, chamfer_dist" and len(lines) == 2
    shape, value = lines[1].split(", ")
    area = pn.face_areas(V, F).sum()
    print(f"chamfer {value} bound {4 * area / (math.pi * 2000):.3e}")
    assert shape == "ds/shapes/shapes_10000" and 0 < float(value) < 4 * area / (math.pi * 2000)
