"""Seeded training batches for the oracle comparisons (torch on the CPU only): the plain batch of B x S points and the margin-safe
batch built from it, for equal segments (tests/test_gpu_parity.py's callers) or explicit segment lengths (tests/test_gpu_breakpoints.py)."""
import torch

from oracle import deepsdf_oracle as orc


def big_batch(B, S, seed, G=3, lens=None):
    """B scenes of S points (or one scene per entry of `lens`): idx [N], xyz [N, G] in the cube, gt [N, 1] = the distance to a sphere
    per scene.  lens = [S] * B draws exactly what (B, S) draws."""
    gen = torch.Generator().manual_seed(seed)
    if lens is None:
        idx = torch.arange(B).repeat_interleave(S)
    else:
        B = len(lens)
        idx = torch.arange(B).repeat_interleave(torch.tensor(lens, dtype=torch.int64))
    xyz = torch.rand(idx.numel(), G, generator=gen) * 2 - 1
    c = (torch.rand(B, G, generator=gen) - 0.5) * 0.6
    r = 0.3 + 0.3 * torch.rand(B, 1, generator=gen)
    gt = (xyz - c[idx]).norm(dim=1, keepdim=True) - r[idx]
    return idx, xyz, gt


def safe_batch(net, st64, B, S, seed, delta, code_bound, drop_seed, margin=2e-5, relu_margin=1e-6, G=3, masks=None, scenes=None, lens=None):
    """Seeded batch whose clamp / sign / ReLU decisions are robust: points with | |y|-delta | or |clamp(y)-clamp(t)|
    within `margin`, or any hidden pre-activation within `relu_margin` of 0 (decided by the float64 oracle), are
    re-drawn.  A clamp/sign flip of one point moves 1/N of the gradient (6e-5 at N=16384); ~10 ReLU flips out of 67 M
    pre-activations put BOTH fp32 implementations (HIP and the CPU oracle) 1.5e-4 from the fp64 truth.  That is
    discontinuity noise, not kernel error, so the comparison is made on a margin-safe batch.

    Segments: B equal ones of S points, or `lens` (one length per segment, ragged or not; B and S are then ignored).  `scenes` [R]
    names the latent-table row of every segment (any order, a table larger than R); without it segment i reads row i.  Raises if
    12 rounds of re-drawing leave a risky point: there is no unsafe fall-back."""
    idx, xyz, gt = big_batch(B, S, seed, G, lens)
    if scenes is not None:                                   # rows of a larger latent table instead of 0 .. B-1
        idx = scenes.repeat_interleave(S) if lens is None else scenes.repeat_interleave(torch.tensor(lens, dtype=torch.int64))
    gen = torch.Generator().manual_seed(seed + 999)
    lat = st64.latents.clone()
    orc.renorm_rows_(lat, idx, code_bound)
    if masks is None:
        masks = orc.dropout_masks(net, drop_seed, st64.step, xyz.shape[0])
    lmask = orc.latent_dropout_mask(net, drop_seed, st64.step, xyz.shape[0]) if net.latent_dropout else None
    for _ in range(12):
        x0 = torch.cat([lat[idx], xyz.double()], 1)
        y, sv = orc.decoder_forward(net, st64.params, x0, training=True, masks=masks, track_margin=True, latent_mask=lmask)
        d = torch.clamp(y, -delta, delta) - torch.clamp(gt.double(), -delta, delta)
        risky = (((y.abs() - delta).abs() < margin) | ((d != 0) & (d.abs() < margin))).reshape(-1)
        risky |= sv.min_abs_pre < relu_margin
        if not bool(risky.any()):
            return idx, xyz, gt
        k = int(risky.sum())
        xyz[risky] = torch.rand(k, G, generator=gen) * 2 - 1
        gt[risky] = (torch.rand(k, 1, generator=gen) - 0.5) * 0.4
    raise RuntimeError("could not build a margin-safe batch")
