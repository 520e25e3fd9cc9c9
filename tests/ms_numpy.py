"""Numpy references for microstructure meshing, written from the specification in include/dsdf.h (dsdf_ms_*): the grid's
unfolded and folded coordinates in fp32 with every operation rounded on its own, a tensor-product B-spline in fp64 by the
Cox-de Boor recursion, and the caps in fp32.  The tests compare the HIP kernels against these."""
import numpy as np

LOCATION = {"x0": (0, -1), "x1": (0, 1), "y0": (1, -1), "y1": (1, 1), "z0": (2, -1), "z1": (2, 1)}
F = np.float32


def fold(xo, t):
    """(2/p) * |((xo - t%2) mod 2p) - p| - 1 in fp32, p = 2/t, mod the floored remainder; constants rounded from double once."""
    xo = np.asarray(xo, dtype=F)
    p = 2.0 / t
    sub, mod, pf, scale = F(t % 2), F(p * 2.0), F(p), F(2.0 / p)
    r = np.fmod(xo - sub, mod)
    r = np.where((r != 0) & (r < 0), r + mod, r).astype(F)
    return (scale * np.abs(r - pf) - F(1)).astype(F)


def grid_axes(N, tiling):
    """Per axis a of the padded grid (N[a] + 2 points): (xo [n] fp32, folded [n] fp32, inside [n] bool)."""
    out = []
    for n, t in zip(N, tiling):
        n = int(n) + 2
        vs = 2.0 / (n - 1 - 2)
        xo = (np.arange(n).astype(F) * F(vs)).astype(F) + F(-1 - vs)
        assert xo.dtype == F
        out.append((xo, fold(xo, int(t)), (xo >= -1) & (xo <= 1)))
    return out


def grid_points(axes, which=0):
    """[n, 3] array of the grid in linear order (z fastest) from the per-axis arrays grid_axes returns (which: 0 xo, 1 folded)."""
    g = np.meshgrid(*[a[which] for a in axes], indexing="ij")
    return np.stack([x.reshape(-1) for x in g], 1)


def grid_inside(axes):
    g = np.meshgrid(*[a[2] for a in axes], indexing="ij")
    return (g[0] & g[1] & g[2]).reshape(-1)


def basis_matrix(p, U, u):
    """B [len(u), n]: the n = len(U) - p - 1 B-spline basis functions of degree p at u (clamped to the knot range), fp64, by the
    Cox-de Boor recursion with 0/0 = 0.  The degree-0 functions are half-open except that the right end of the range belongs to
    the last non-empty span."""
    U = np.asarray(U, dtype=np.float64)
    n = U.size - p - 1
    u = np.clip(np.asarray(u, dtype=np.float64), U[p], U[n])
    m = U.size - 1
    B = np.zeros((u.size, m))
    for i in range(m):
        B[:, i] = (U[i] <= u) & (u < U[i + 1])
    last = max(i for i in range(p, n) if U[i] < U[i + 1])
    B[u == U[n]] = 0.0
    B[u == U[n], last] = 1.0
    for d in range(1, p + 1):
        nxt = np.zeros((u.size, m - d))
        for i in range(m - d):
            a = U[i + d] - U[i]
            b = U[i + d + 1] - U[i + 1]
            if a > 0:
                nxt[:, i] += (u - U[i]) / a * B[:, i]
            if b > 0:
                nxt[:, i] += (U[i + d + 1] - u) / b * B[:, i + 1]
        B = nxt
    return B


def bspline_eval(degrees, knots, cp, pts):
    """Values [n, L] (fp64) of the trivariate spline at pts [n, 3]; cp [ncp, L], first parametric axis fastest."""
    pts = np.asarray(pts, dtype=np.float64)
    cp = np.asarray(cp, dtype=np.float64)
    Bs = [basis_matrix(int(degrees[a]), knots[a], pts[:, a]) for a in range(3)]
    nx, ny, nz = (B.shape[1] for B in Bs)
    P = cp.reshape(nz, ny, nx, -1)
    out = np.empty((pts.shape[0], P.shape[-1]))
    for s in range(0, pts.shape[0], 4096):
        e = min(pts.shape[0], s + 4096)
        out[s:e] = np.einsum("pi,pj,pk,kjil->pl", Bs[0][s:e], Bs[1][s:e], Bs[2][s:e], P, optimize=True)
    return out


def _max(a, b):
    """max(a, b) as compare-and-select: on a tie (+0 against -0 included) the first stays, a NaN in a stays.  np.maximum leaves
    the sign of a zero to the platform's vector instruction, so a bit-for-bit specification cannot be written with it."""
    return np.where(b > a, b, a).astype(F)


def _min(a, b):
    return np.where(b < a, b, a).astype(F)


def caps(sdf, xo, cap_border_dict, vmax=_max, vmin=_min):
    """The capped field, fp32: sdf [nx, ny, nz], xo the three per-axis coordinate arrays.  First the dictionary's entries in its
    own order (cap -1: max(sdf, -border), cap 1: min(sdf, border), border = (xo - m * (1 - measure)) * -m), then the six planes
    of the unit cube with max.  vmax / vmin: the compare-and-select above, or np.maximum / np.minimum (equal as values)."""
    v = np.array(sdf, dtype=F)
    shape = [(-1, 1, 1), (1, -1, 1), (1, 1, -1)]
    for loc, d in cap_border_dict.items():
        dim, m = LOCATION[loc]
        x = np.asarray(xo[dim], dtype=F).reshape(shape[dim])
        border = ((x - F(m * (1 - d["measure"]))) * F(-m)).astype(F)
        if d["cap"] == -1:
            v = vmax(v, -border)
        elif d["cap"] == 1:
            v = vmin(v, border)
        else:
            raise ValueError("Cap must be -1 or 1")
    for dim in range(3):
        for m in (-1, 1):
            x = np.asarray(xo[dim], dtype=F).reshape(shape[dim])
            v = vmax(v, -((x - F(m)) * F(-m)).astype(F))
    assert v.dtype == F
    return v
