"""Numpy oracle of surface following on blocks of a dense grid (csrc/sparsegrid.hpp, include/dsdf.h dsdf_sg_*): a
restatement of the six steps on a field that is known everywhere (a table look-up stands in for the decoder).

    grid     dims (nx, ny, nz), linear index z fastest; block edge b >= 2 cells; coarse coordinates of axis a:
             {0, b, 2b, ... < n_a - 1} + {n_a - 1}; block (I, J, K) owns the closed point box between consecutive coarse coordinates
    inside   v < level, strictly
    states   0 inactive, 1 new (active, its points not yet decoded), 2 valued

Also the analytic fields the tests share."""
import numpy as np

INACTIVE, NEW, VALUED = 0, 1, 2


def coarse_coords(n, b):
    return np.array(list(range(0, n - 1, b)) + [n - 1], dtype=np.int64)


def threshold(b, spacing, lipschitz):
    """thr in double, rounded to fp32 once: lipschitz * half the diagonal of a full block in decoder coordinates."""
    s = [float(x) for x in (spacing if np.ndim(spacing) else [spacing] * 3)]
    return np.float32(float(lipschitz) * 0.5 * np.sqrt(sum((b * x) ** 2 for x in s)))


def _closed(A, axis, c, ufunc):
    """ufunc over the closed index ranges [c[J], c[J + 1]] of `axis`."""
    return ufunc(ufunc.reduceat(A, c[:-1], axis=axis), np.take(A, c[1:], axis=axis))


def _member(n, c):
    """M [n, blocks] bool: point i lies in block I's closed range; low [n]: the coarse coordinate of the lowest such block."""
    i = np.arange(n)[:, None]
    M = (c[None, :-1] <= i) & (i <= c[None, 1:])
    return M, c[np.argmax(M, axis=1)]


class Result:
    pass


def follow_surface(field, b, thr, level=0.0, capped=None):
    """field [nx, ny, nz] fp32: the values a decoder would give; capped: the values after the caps (the grid that is meshed), or
    None.  Returns a Result: seeds / states (uint8 [blocks] after seeding and after every round), indices (the coarse list, then
    one int64 list per round), have (uint8 [points]), grid / capped (filled, fp32), stats."""
    raw = np.ascontiguousarray(field, dtype=np.float32)
    dims = raw.shape
    g = raw if capped is None else np.ascontiguousarray(capped, dtype=np.float32)
    lvl, thr = np.float32(level), np.float32(thr)
    c = [coarse_coords(n, b) for n in dims]
    nb = [len(x) - 1 for x in c]
    mem = [_member(dims[a], c[a]) for a in range(3)]
    inside = g < lvl

    # steps 1 and 2
    corner = g[np.ix_(*c)]
    cin = corner < lvl
    dist = np.abs(corner - lvl)                                    # fp32 subtraction
    any_in = np.zeros(nb, dtype=bool)
    all_in = np.ones(nb, dtype=bool)
    near = np.full(nb, np.inf, dtype=np.float32)
    for d in range(8):
        sl = tuple(slice(o, o + nb[a]) for a, o in enumerate(((d >> 2) & 1, (d >> 1) & 1, d & 1)))
        any_in |= cin[sl]
        all_in &= cin[sl]
        near = np.fmin(near, dist[sl])                             # a NaN never seeds
    state = np.where((any_in & ~all_in) | (near <= thr), NEW, INACTIVE).astype(np.uint8)

    have = np.zeros(dims, dtype=bool)
    have[np.ix_(*c)] = True
    r = Result()
    r.coarse = np.flatnonzero(have.reshape(-1)).astype(np.int64)
    r.seeds = state.reshape(-1).copy()
    r.indices, r.states = [], []

    # mixed[a][m, J, K]: the face in the plane of coarse coordinate m of axis a, over the closed ranges of the two other axes
    mixed = []
    for a in range(3):
        P = np.take(inside, c[a], axis=a)
        others = [x for x in range(3) if x != a]
        hi, lo = P, P
        for x in others:
            hi, lo = _closed(hi, x, c[x], np.maximum), _closed(lo, x, c[x], np.minimum)
        mixed.append(np.moveaxis(hi & ~lo, a, 0))

    n_seeds = int((state == NEW).sum())
    while (state == NEW).any():
        # step 3: the points of new blocks without a value, ascending
        S = (state == NEW).astype(np.int64)
        T = np.tensordot(mem[0][0].astype(np.int64), S, (1, 0))
        T = np.tensordot(mem[1][0].astype(np.int64), T, (1, 1))    # [ny, nx, nbz]
        T = np.tensordot(mem[2][0].astype(np.int64), T, (1, 2))    # [nz, ny, nx]
        want = (T.transpose(2, 1, 0) > 0) & ~have
        r.indices.append(np.flatnonzero(want.reshape(-1)).astype(np.int64))
        have |= want
        # step 4: gather-form growth from the blocks valued in this round
        new = state == NEW
        pend = np.zeros(nb, dtype=bool)
        for a in range(3):
            nw, mxa = np.moveaxis(new, a, 0), mixed[a]             # mxa: [coarse coordinate of a, the two other axes' blocks]
            p = np.zeros(nw.shape, dtype=bool)
            p[1:] |= nw[:-1] & mxa[1:-1]                           # the neighbour below shares the plane of c[I]
            p[:-1] |= nw[1:] & mxa[1:-1]                           # the neighbour above shares the plane of c[I + 1]
            pend |= np.moveaxis(p, 0, a)
        state = np.where(new, VALUED, np.where(pend & (state == INACTIVE), NEW, state)).astype(np.uint8)
        r.states.append(state.reshape(-1).copy())

    # step 5
    low = np.ix_(mem[0][1], mem[1][1], mem[2][1])
    r.have = have.reshape(-1).astype(np.uint8)
    r.grid = np.where(have, raw, raw[low])
    r.capped = None if capped is None else np.where(have, g, g[low])
    r.active = (state == VALUED).reshape(nb)
    r.blocks, r.coords = nb, c
    r.stats = dict(blocks=int(np.prod(nb)), seeds=n_seeds, active=int((state == VALUED).sum()), rounds=len(r.indices),
                   points=int(r.have.sum()), total=int(have.size))
    return r


def cell_active(r, dims):
    """bool [nx - 1, ny - 1, nz - 1]: the cell lies in an active block (a cell lies in exactly one block)."""
    out = r.active
    for a in range(3):
        cell_block = np.searchsorted(r.coords[a], np.arange(dims[a] - 1), side="right") - 1
        out = np.take(out, cell_block, axis=a)
    return out


# ---- fields (fp32 on the grid over [-1, 1]^3; the spacing of axis a is 2 / (n_a - 1)) --------------------------------------------
def _axes(dims):
    return np.meshgrid(*[np.linspace(-1, 1, n, dtype=np.float64) for n in dims], indexing="ij")


def spacing(dims):
    return [2.0 / (n - 1) for n in dims]


def sphere(dims, r=0.5):
    X, Y, Z = _axes(dims)
    return (np.sqrt(X * X + Y * Y + Z * Z) - r).astype(np.float32)


def torus(dims, R=0.6, r=0.11):
    X, Y, Z = _axes(dims)
    return (np.sqrt((np.sqrt(X * X + Y * Y) - R) ** 2 + Z * Z) - r).astype(np.float32)


def gyroid(dims, t=0.3):
    X, Y, Z = (np.pi * 2 * A for A in _axes(dims))
    return (np.sin(X) * np.cos(Y) + np.sin(Y) * np.cos(Z) + np.sin(Z) * np.cos(X) - t).astype(np.float32)


# the rods run between the coarse planes of a 33^3 grid with b = 4 (multiples of 0.25), so no block corner lies inside one
ROD_AT = (0.125, -0.375)


def rods(dims, r=0.07):
    """Three axis-parallel rods of radius r: the distance to the nearest one (a true distance field)."""
    X, Y, Z = _axes(dims)
    u, w = ROD_AT
    d = np.minimum(np.sqrt((Y - u) ** 2 + (Z - w) ** 2), np.sqrt((X - w) ** 2 + (Z - u) ** 2))
    return (np.minimum(d, np.sqrt((X - u) ** 2 + (Y - w) ** 2)) - r).astype(np.float32)


def sphere_bubble(dims, r=0.5, rb=0.04, at=(0.8125, 0.8125, 0.8125)):
    """A sphere and a bubble that holds one grid point of the 33^3 grid, (29, 29, 29), which is no block corner at b = 4: eight
    crossing cells that no corner sign shows (the union: a true distance field outside both)."""
    X, Y, Z = _axes(dims)
    s = np.sqrt(X * X + Y * Y + Z * Z) - r
    q = np.sqrt((X - at[0]) ** 2 + (Y - at[1]) ** 2 + (Z - at[2]) ** 2) - rb
    return np.minimum(s, q).astype(np.float32)


DISTANCE_FIELDS = {"sphere": sphere, "torus": torus, "rods": rods, "sphere_bubble": sphere_bubble}
FIELDS = dict(DISTANCE_FIELDS, gyroid=gyroid)


def blobs(dims, seed):
    """A seeded sum of Gaussian blobs minus a level: smooth, several components, not a distance field."""
    g = np.random.default_rng(seed)
    X, Y, Z = _axes(dims)
    out = np.zeros(dims)
    for _ in range(int(g.integers(3, 9))):
        c, w, a = g.uniform(-0.9, 0.9, 3), g.uniform(0.08, 0.4), g.uniform(0.5, 1.5)
        out += a * np.exp(-((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) / (2 * w * w))
    return (0.5 - out).astype(np.float32)
