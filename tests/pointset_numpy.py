"""numpy restatement of csrc/pointset.hpp's specification (include/dsdf.h, dsdf_nn_* / dsdf_surf_*): the oracle of
tests/test_pointset_cpu.py and tests/test_gpu_pointset.py.  No torch, no device.

    nn_bruteforce       fp64 brute-force nearest neighbour on the fp32-rounded inputs, lowest index on ties
    philox4x32_10       Philox4x32-10 (Salmon et al., SC'11), vectorised over counters
    surface_samples     the sampler's face / barycentric / point rule in fp64, taking the fp32 face areas as input
    face_areas_f32      the prepare pass's fp32 face areas, operation for operation (bit-exact by construction)
    triangle_soup, sliver_between_faces      inputs shared by the CPU and the GPU tests
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def nn_bruteforce(Q, R, block=512):
    """(d2 fp64 [nq], index int64 [nq]) of the fp32-rounded points; np.argmin returns the lowest index of the minimum."""
    Q, R = f32(Q).reshape(-1, 3), f32(R).reshape(-1, 3)
    d2, idx = np.empty(len(Q)), np.empty(len(Q), dtype=np.int64)
    for s in range(0, len(Q), block):
        d = Q[s:s + block, None, :] - R[None, :, :]
        dd = (d * d).sum(axis=2)
        idx[s:s + block] = dd.argmin(axis=1)
        d2[s:s + block] = dd[np.arange(dd.shape[0]), idx[s:s + block]]
    return d2, idx


def pair_d2(Q, R, idx):
    """fp64 squared distance from Q[i] to R[idx[i]] (fp32-rounded inputs)."""
    d = f32(Q).reshape(-1, 3) - f32(R).reshape(-1, 3)[np.asarray(idx, dtype=np.int64)]
    return (d * d).sum(axis=1)


def philox4x32_10(counter, key):
    """counter: uint32 [n, 4] (or [4]), key: two uint32 -> uint32 [n, 4]."""
    c = np.atleast_2d(np.asarray(counter, dtype=np.uint64)).copy()
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[:, 0], M1 * c[:, 2]                        # 32 x 32 -> 64 bits: no overflow in uint64
        n0 = (p1 >> S32) ^ c[:, 1] ^ np.uint64(k0)
        n2 = (p0 >> S32) ^ c[:, 3] ^ np.uint64(k1)
        c = np.stack([n0, p1 & MASK, n2, p0 & MASK], axis=1)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c.astype(np.uint32)


def sample_words(n, seed, offset=0, stream=0):
    i = np.arange(n, dtype=np.uint64) + np.uint64(offset)
    ctr = np.stack([i & MASK, np.full(n, stream, np.uint64), i >> S32, np.zeros(n, np.uint64)], axis=1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def exact_cdf(area32):
    """Inclusive prefix sums of the fp32 areas in extended precision, rounded to fp64 (and the extended values)."""
    ext = np.cumsum(np.asarray(area32, dtype=np.float32).astype(np.longdouble))
    return ext.astype(np.float64), ext


def surface_samples(V, F, area32, n, seed, offset=0):
    """The rule of dsdf_surf_sample with the exact CDF of the given fp32 areas.  Returns a dict: face int64 [n], u, v fp32 [n]
    (bit-exact by construction), point fp64 [n, 3] (from the fp32-rounded vertices), x = r * total fp64 [n], and margin [n]: the
    distance of x to the nearest CDF boundary relative to the total (a face is only decided where this is not tiny)."""
    V, F = f32(V), np.asarray(F, dtype=np.int64)
    w = sample_words(n, seed, offset)
    cdf, _ = exact_cdf(area32)
    total = cdf[-1]
    k = (w[:, 0].astype(np.uint64) << S32) | w[:, 3].astype(np.uint64)
    r = k.astype(np.float64) * 2.0 ** -64                           # uint64 -> fp64 rounds to nearest, as the device does
    x = r * total
    face = np.searchsorted(cdf, x, side="right")                     # the first f with cdf[f] > x
    last = int(np.searchsorted(cdf, total, side="left"))             # the first f with cdf[f] == total
    face = np.where(face >= len(cdf), last, face)
    j = np.searchsorted(cdf, x)
    lo, hi = cdf[np.clip(j - 1, 0, len(cdf) - 1)], cdf[np.clip(j, 0, len(cdf) - 1)]
    margin = np.minimum(np.abs(lo - x), np.abs(hi - x)) / total
    one = np.float32(1)
    u = (w[:, 1] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    v = (w[:, 2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    flip = (u + v) > one                                             # the fp32 sum, rounded
    u, v = np.where(flip, one - u, u), np.where(flip, one - v, v)
    a = V[F[face, 0]]
    ab32 = (V[F[face, 1]].astype(np.float32) - a.astype(np.float32)).astype(np.float64)   # the device's fp32 edge vectors
    ac32 = (V[F[face, 2]].astype(np.float32) - a.astype(np.float32)).astype(np.float64)
    p = a + u.astype(np.float64)[:, None] * ab32 + v.astype(np.float64)[:, None] * ac32
    return dict(face=face, u=u, v=v, point=p, x=x, margin=margin, total=total)


def face_areas(V, F):
    """fp64 areas of the fp32-rounded mesh."""
    V, F = f32(V), np.asarray(F, dtype=np.int64)
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    return 0.5 * np.linalg.norm(n, axis=1)


def face_areas_f32(V, F, contracted=False):
    """The fp32 areas of dsdf_surf_prepare, operation for operation (include/dsdf.h): ab = b - a, ac = c - a, n = ab x ac,
    area = 0.5 * sqrt((nx nx + ny ny) + nz nz), every difference, product and sum rounded to fp32 on its own, the square root
    correctly rounded (np.sqrt on float32 is), the factor 0.5 exact.

    contracted=True is what a compiler makes of the same expressions when it may contract: every normal component is
    fma(p, q, -(r * s)) with r * s rounded, and n.n is fma(nz, nz, fma(ny, ny, nx * nx)); the fused operations are formed in fp64
    from the fp32 operands (products exact) and rounded to fp32 once.  It is NOT the specification: it exists so that a test can
    prove that its inputs tell the two apart."""
    V, F = np.asarray(V, dtype=np.float32), np.asarray(F, dtype=np.int64)
    a = V[F[:, 0]]
    ab, ac = V[F[:, 1]] - a, V[F[:, 2]] - a
    x, y, z = 0, 1, 2
    if not contracted:
        n = [ab[:, i] * ac[:, j] - ab[:, j] * ac[:, i] for i, j in ((y, z), (z, x), (x, y))]
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    else:
        d = np.float64
        n = [(ab[:, i].astype(d) * ac[:, j].astype(d) - (ab[:, j] * ac[:, i]).astype(d)).astype(np.float32)
             for i, j in ((y, z), (z, x), (x, y))]
        s = (n[1].astype(d) * n[1].astype(d) + (n[0] * n[0]).astype(d)).astype(np.float32)
        nn = (n[2].astype(d) * n[2].astype(d) + s.astype(d)).astype(np.float32)
    assert nn.dtype == np.float32
    return np.float32(0.5) * np.sqrt(nn)


SOUP_SPLIT = 262144          # 256 scan tiles of 1024 faces: the faces from here on lie behind the tile scan's first round


def triangle_soup(nf, seed, heavy_tail=False):
    """(V float32 [3 nf, 3], F int64 [nf, 3]): nf seeded triangles with three fresh vertices each, centres in [-1, 1]^3, edges of
    about 0.05; no coordinate is dyadic.  The first nf faces of a larger soup of the same seed are this soup.  heavy_tail: the
    faces from SOUP_SPLIT on are scaled about their first vertex so that together they carry about half of the total area."""
    big = max(nf, SOUP_SPLIT + 1025)
    g = np.random.default_rng(seed)
    c = g.uniform(-1, 1, (big, 1, 3))
    V = (c + g.uniform(-0.03, 0.03, (big, 3, 3))).astype(np.float32)[:nf]
    if heavy_tail and nf > SOUP_SPLIT:
        area = face_areas(V.reshape(-1, 3), np.arange(3 * nf).reshape(nf, 3))
        k = np.sqrt(area[:SOUP_SPLIT].sum() / area[SOUP_SPLIT:].sum())
        a = V[SOUP_SPLIT:, :1].astype(np.float64)
        V[SOUP_SPLIT:] = (a + k * (V[SOUP_SPLIT:].astype(np.float64) - a)).astype(np.float32)
    return V.reshape(-1, 3), np.arange(3 * nf, dtype=np.int64).reshape(nf, 3)


def sliver_between_faces():
    """(V float32, F): the degenerate face (0, d, 2 d) with a non-dyadic d between two real faces.  ab = d and ac = 2 d exactly, so
    both products of every normal component round to the same number and the specification's area is exactly 0; a contracted
    cross product keeps the rounding error of one product instead."""
    d = np.array([0.3, 0.7, 1.1], dtype=np.float32)
    V = np.array([[0, 0, 0], d, 2 * d, [1.1, 0.2, 0.3], [0.1, 1.3, 0.2], [0.3, 0.1, 0.9], [-0.7, 0.6, -1.3]], dtype=np.float32)
    return V, np.array([[0, 3, 4], [0, 1, 2], [3, 5, 6]], dtype=np.int64)
