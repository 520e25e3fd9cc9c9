"""The optimiser tail's spec in float64 (numpy), and beside every quantity the bound an fp32 kernel that evaluates the SAME
expressions must meet, built from the count of fp32 roundings in those expressions -- never from an observed error.

Adam exactly as torch/optim/adam.py (single-tensor form) and oracle.adam_update_ define it:

    m' = m + (1 - b1) (g - m)
    v' = b2 v + (1 - b2) g^2
    p' = p - lr / (1 - b1^t) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

with the four variants of the step's tail: `grad_scale` multiplies g first; the sched form uses g + l2 p; the clip coefficient is
min(1, max_norm / (norm + 1e-6)); the weight-norm row scale is g' / ||v'_row||.

The constants are the ones the C ABI carries: DsdfAdamCfg holds lr, beta1, beta2 and eps as FLOATS, so the spec is evaluated at
float(0.9), float(0.999), float(1e-8) (`f32(x)` below), not at the decimal values: 1 - float(0.9) differs from 0.1 by 4 units of
fp32 roundoff, which is an input of the kernels, not an error of theirs.

Bounds.  U = 2^-24 is the unit roundoff of fp32 (round to nearest: one operation's relative error is at most U; divisions and square
roots are correctly rounded in the library's build).  k roundings in a row give gamma(k) = k U / (1 - k U) (Higham, Accuracy and
Stability of Numerical Algorithms, Lemma 3.1).  A compiler that contracts a * b + c into one fused multiply-add removes roundings,
it never adds one: every count is the UN-contracted expression's.  Every input regime of the tests keeps every intermediate a
normal fp32 number (or an exact zero), so no absolute (denormal) term appears.
"""
import math

import numpy as np

U = 2.0 ** -24


def gamma(k):
    return k * U / (1.0 - k * U)


def f32(x):
    """The double that equals float(x): how a Python constant reaches the kernels through the C ABI."""
    return float(np.float32(x))


B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)


def step_scalars(lr, b1, b2, t):
    """(lr / (1 - b1^t), sqrt(1 - b2^t)) in double: the host side of every Adam launch."""
    return lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)


def adam_ref(p, g, m, v, *, lr, t, b1=B1, b2=B2, eps=EPS, grad_scale=1.0, l2=0.0, step_size=None, bc2_sqrt=None):
    """One Adam step in float64.  Returns dict(p, m, v, g_eff, upd_scale): the new state, the gradient the variant feeds
    (grad_scale * g, or g + l2 p), and the natural scale of the update (see p_bound).  step_size / bc2_sqrt given: the two step
    scalars as a device schedule holds them (dsdf_adam_latent_sched) instead of lr and t."""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    ge = g * float(grad_scale) + float(l2) * p
    if step_size is None:
        step_size, bc2_sqrt = step_scalars(lr, b1, b2, t)
    m2 = m + (1.0 - b1) * (ge - m)
    v2 = b2 * v + (1.0 - b2) * ge * ge
    den = np.sqrt(v2) / bc2_sqrt + eps
    p2 = p - step_size * (m2 / den)
    # the update the kernel's m' can produce: its error is relative to max(|m|, |g|), not to a cancelled |m'|
    upd_scale = step_size * np.maximum(np.maximum(np.abs(m), np.abs(ge)), np.abs(m2)) / den
    return dict(p=p2, m=m2, v=v2, g_eff=ge, upd_scale=upd_scale)


def _kg(scaled):
    """Roundings that enter the effective gradient: g * grad_scale, or fma(l2, p, g): ONE (relative to the result either way: a
    product, or a single-rounded fused multiply-add); none for the plain forms."""
    return 1 if scaled else 0


def m_bound(m, g_eff, scaled=False):
    """|m'_kernel - m'| <= gamma(k) max(|m|, |g|), k = 2 + kg.  mi = fma(omb1, gi - m, m): the difference (1 rounding, <= U |gi - m|
    <= 2 U max, times omb1 <= 1/2: <= U max) and the fused multiply-add (1 rounding, <= U |m'| <= U max); the effective gradient's
    rounding reaches m' times omb1 (<= 1 more).  Valid for 1 - b1 <= 1/2."""
    return gamma(2 + _kg(scaled)) * np.maximum(np.abs(m), np.abs(g_eff))


def v_bound(v_new, scaled=False):
    """|v'_kernel - v'| <= gamma(k) v', k = 4 + 2 kg.  vi = b2 * v + ((omb2 * gi) * gi): three products and one sum of two
    non-negative terms = 4 roundings, every one relative to a term of v'; the effective gradient's rounding enters squared (2 more)."""
    return gamma(4 + 2 * _kg(scaled)) * np.abs(v_new)


def p_bound(p_new, upd_scale, scaled=False):
    """|p'_kernel - p'| <= gamma(k) upd_scale + U |p'|, upd_scale = step_size max(|m|, |g|, |m'|) / (sqrt(v') / bc2_sqrt + eps).
    p - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps)), k = 7 + ceil(kv / 2) + km:
      7: the host's two roundings to float (step_size, bc2_sqrt), sqrtf, the division by bc2_sqrt, the sum with eps (both terms
         non-negative), the division mi / (...), the product with step_size;
      ceil(kv / 2) = 2 + kg: v' enters through a square root, which halves its relative error (kv = 4 + 2 kg, v_bound);
      km = 2 + kg: m' enters linearly with an error relative to max(|m|, |g|) (m_bound) -- hence upd_scale in place of the update;
    and the final subtraction rounds once, relative to |p'|."""
    kg = _kg(scaled)
    k = 7 + (2 + kg) + (2 + kg)
    return gamma(k) * upd_scale + U * np.abs(p_new)


def sum_bound(total, chain, depth, per_term=1):
    """A sum of n non-negative terms, each carrying `per_term` roundings of its own (1: a square), accumulated along chains of at
    most `chain` additions and then through a tree of `depth` levels: |s_kernel - s| <= gamma(per_term + chain + depth) s."""
    return gamma(per_term + chain + depth) * np.abs(total)


# ---- weight-norm row scale ----------------------------------------------------------------------------------------------------

def row_scale_ref(g_new, v_new_rows):
    """g' / ||v'_row|| in float64: g_new [out], v_new_rows [out, in]."""
    v = np.asarray(v_new_rows, dtype=np.float64)
    return np.asarray(g_new, dtype=np.float64).reshape(-1) / np.sqrt((v * v).sum(axis=1))


def row_scale_k(n_in, lanes=64, tree=6):
    """Roundings of scale = g / sqrtf(ss), ss summed by one wave: every lane squares and adds its columns c = lane, lane + 64, ...
    (the lane-strided sum: 1 rounding per square, a chain of ceil(in / 64) additions), six shuffle additions, ONE square root
    (which halves what came before) and ONE division.  k = ceil((1 + ceil(in / 64) + 6) / 2) + 2."""
    kss = 1 + -(-n_in // lanes) + tree
    return -(-kss // 2) + 2


def row_scale_bound(scale_ref, n_in, lanes=64, tree=6):
    return gamma(row_scale_k(n_in, lanes, tree)) * np.abs(scale_ref)


# ---- gradient norm and clip coefficient ----------------------------------------------------------------------------------------

def clip_coef_ref(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_: min(1, max_norm / (norm + 1e-6))."""
    return min(1.0, float(max_norm) / (float(norm) + 1e-6))


def grad_norm_counts(n):
    """(blocks, kss) of dsdf_grad_norm for n floats.  Stage 1: blocks = min(1024, ceil(n / 4096)) blocks of 256 threads, a thread
    squares (1 rounding) and adds its elements i = tid, tid + 256 blocks, ... (chain ceil(n / (256 blocks))), then the block sum:
    six shuffle additions and a two-level tree over the four waves (8).  Stage 2: one block, a thread adds ceil(blocks / 256)
    partials, then the same block sum (8).  kss = 1 + chain1 + 8 + chain2 + 8."""
    blocks = min(1024, -(-n // 4096))
    chain1 = -(-n // (256 * blocks))
    chain2 = -(-blocks // 256)
    return blocks, 1 + chain1 + 8 + chain2 + 8


def grad_norm_bound(norm_ref, n):
    """|norm_kernel - norm| <= gamma(ceil(kss / 2) + 1) norm: the sum of squares (grad_norm_counts), halved by the square root,
    plus the square root's own rounding."""
    _, kss = grad_norm_counts(n)
    return gamma(-(-kss // 2) + 1) * abs(norm_ref)


def clip_coef_bound(coef_ref, n):
    """coef = fminf(1, max_norm / (nrm + 1e-6f)) below 1: the norm's own roundings (grad_norm_bound), the constant 1e-6f (1, relative
    to 1e-6 <= nrm + 1e-6), the sum (1) and the division (1).  A coefficient that the spec puts at 1 with a margin wider than this
    bound must be EXACTLY 1.0f."""
    _, kss = grad_norm_counts(n)
    return gamma(-(-kss // 2) + 1 + 3) * abs(coef_ref)


# ---- the tests' input generator ------------------------------------------------------------------------------------------------

G_DECADES = tuple(range(-12, -1))       # |g| in [10^d, 10^(d+1)), d = -12 .. -2: 1e-12 .. 1e-1
FLT_MIN = 2.0 ** -126


def make_state(n, seed, row=16, aged=True):
    """The fixed generator of the tail tests: (p, g, m, v) as float32 arrays of n elements.
      p ~ N(0, 0.05);  aged: v = 10^U(-16, -2), m = +-sqrt(v) U(0, 1.5);  not aged: m = v = 0
      |g| log-uniform over the decades 1e-12 .. 1e-1 (a band around eps = 1e-8 included), random sign; the lower limit 1e-12 keeps
      g^2 >= 1e-24 and (1 - b2) g^2 >= 1e-27 NORMAL fp32 numbers (FLT_MIN = 1.2e-38), so every bound stays purely relative
      one twentieth of the g entries are exact zeros; every fifth row of `row` elements (a latent row absent from the batch) is
      zero in g.
    Small n (< 220): the first entries walk the decades in order, so every decade is present at every size that can hold them."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0.0, 0.05, n)
    e = rng.uniform(-12.0, -1.0, n)
    k = min(n, 11 * 20)
    e[:k] = (np.arange(k) % 11) - 12 + rng.uniform(0.0, 1.0, k)
    g = 10.0 ** e * rng.choice([-1.0, 1.0], n)
    g[rng.permutation(n)[: n // 20]] = 0.0
    rows = np.arange(n) // row
    g[(rows % 5) == 3] = 0.0
    if aged:
        v = 10.0 ** rng.uniform(-16.0, -2.0, n)
        m = np.sqrt(v) * rng.uniform(0.0, 1.5, n) * rng.choice([-1.0, 1.0], n)
    else:
        v, m = np.zeros(n), np.zeros(n)
    return tuple(x.astype(np.float32) for x in (p, g, m, v))


def check_state(p, g, m, v, row=16, aged=True):
    """The generator's properties, asserted on the CPU before a GPU sees the inputs."""
    n = g.size
    a = np.abs(g.astype(np.float64))
    nz = a[a > 0]
    assert nz.size == 0 or (nz.min() >= 1e-12 * (1 - 1e-6) and nz.max() < 0.1 * (1 + 1e-6))
    g2 = (g.astype(np.float32) * g.astype(np.float32))[a > 0]
    assert g2.size == 0 or float(g2.min()) >= FLT_MIN, "g^2 must stay a normal fp32 number"
    assert g2.size == 0 or float(g2.min()) * (1.0 - B2) >= FLT_MIN
    if n >= 11 * 20 + 64:      # room for every decade next to the zeros
        dec = np.floor(np.log10(nz)).astype(int)
        for d in G_DECADES:
            assert (dec == d).any(), f"no |g| in decade 1e{d}"
        assert ((nz > 1e-10) & (nz < 1e-6)).sum() >= 4, "the band around eps must be populated"
        assert (a == 0).sum() >= n // 20, "one twentieth of g are exact zeros"
        rows = a[: n // row * row].reshape(-1, row)
        assert n < 5 * row or (rows == 0).all(axis=1).any(), "whole zero rows"
    if aged:
        vv = v.astype(np.float64)
        assert vv.min() >= 1e-16 * (1 - 1e-6) and vv.max() <= 1e-2 * (1 + 1e-6)
        assert (np.abs(m.astype(np.float64)) <= 1.5 * np.sqrt(vv) * (1 + 1e-6)).all()
        if n >= 1000:
            assert vv.min() < 1e-13 and vv.max() > 1e-5 and (m > 0).any() and (m < 0).any()
    else:
        assert not m.any() and not v.any()
    assert abs(float(np.std(p.astype(np.float64))) - 0.05) < 0.02 or n < 200
