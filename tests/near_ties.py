"""Training batches with ties and near-ties planted ON the step's decision sites, and the analysis of what a kernel decided there
(torch on the CPU only).  tests/safe_batch.py keeps every oracle comparison a margin away from the places where the
step decides (ReLU, dropout-then-ReLU, the loss's sign and clamp mask); this module goes there on purpose:

  plant_relu_ties      one pre-activation per hidden unit moved to within a rounding of zero (through the unit's bias)
  plant_head_ties      targets on the network's output (and one ulp either side), the clamp edge on one point's |y|
  analyse              what a kernel stored -> its own decisions, checked against a counted rounding band around the fp64 values
                       computed from the kernel's OWN layer inputs; the decisions then force the fp64 oracle onto the kernel's branches
  decisions_from_workspace   the kernel's stored activations, read through the last plan's region table

The band: a K-term fp32 dot product in any order, of operands rounded once (the materialised weight) plus the bias add, is within
  tau = (K + 4) * 2^-24 * (sum_k |W_jk| |in_ik| + |b_j|)
of the exact value (a term passes through at most K roundings, its product and at most K - 1 additions; one more for the weight
rounding, one for the bias add, two spare for the second-order terms).  The bf16 forward rounds both operands of every product to 8 significant bits first; its weight is the bf16
rounding of an fp32 weight that may itself be a few ulp from the fp64 one, which can move that rounding by one bf16 ulp: 2^-7 of
the product, added to the band for those nets."""
import torch

from oracle import deepsdf_oracle as orc

U32 = 2.0 ** -24
BF16_ULP = 2.0 ** -7


def nets():
    """The three decoders of the near-tie tests, one per width class of the kernels (<= 32, <= 64, one layer above 128): four
    hidden layers (segment mode needs the skip layer away from the deepest hidden one), a skip layer, dropout on some layers,
    weight norm on some or all, odd widths where the class allows them."""
    return {
        "w32": (5, dict(dims=[32, 32, 28, 32], dropout=[0, 1, 3], dropout_prob=0.2, norm_layers=[0, 1, 2, 3, 4], latent_in=[2],
                        weight_norm=True, use_tanh=False, geom_dimension=3)),
        "w64": (8, dict(dims=[64, 64, 56, 64], dropout=[1, 2], dropout_prob=0.2, norm_layers=[0, 1, 2, 3, 4], latent_in=[2],
                        weight_norm=True, use_tanh=True, geom_dimension=3)),
        "w136": (8, dict(dims=[136, 72, 136, 72], dropout=[0, 2, 3], dropout_prob=0.2, norm_layers=[0, 1, 3, 4], latent_in=[2],
                         weight_norm=True, use_tanh=False, geom_dimension=3)),
    }


def rb(t):
    """bf16 round to nearest even of an fp32 / fp64 tensor, kept in its dtype (the oracle's config-5 emulation)."""
    return t.float().bfloat16().to(t.dtype)


def dbl(params):
    return {k: v.double() for k, v in params.items()}


def _lin(net, l, W, b, inp):
    """(z, sum of magnitudes) of hidden Linear l in the dtype of its operands (bf16-rounded operands for a forward_bf16 net)."""
    if net.forward_bf16:
        W, inp = rb(W), rb(inp)
    return inp @ W.t() + b, inp.abs() @ W.abs().t() + b.abs()


def pre_activations(net, p64, x0, masks, relu_keep=None):
    """fp64 training-mode forward: (y, Saved, [z_l], [magnitude sums]) with z_l the pre-activation of hidden layer l."""
    y, sv = orc.decoder_forward(net, p64, x0, training=True, masks=masks, relu_keep=relu_keep)
    Wb = orc.effective_weights(net, p64)
    zm = [_lin(net, l, Wb[l][0], Wb[l][1], sv.inputs[l]) for l in range(net.n_lin - 1)]
    return y, sv, [z for z, _ in zm], [m for _, m in zm]


def plant_relu_ties(net, params, lat, idx, xyz, masks):
    """One near-tie per hidden unit, layer by layer from the fp64 forward (deeper layers after shallower ones: a layer's planting
    moves every deeper pre-activation).  Unit j of hidden layer l gets a point i(j) its dropout mask keeps; the fp64
    pre-activation z[i, j] is subtracted from lin{l}.bias[j] and the bias rounded to fp32, which leaves |z[i, j]| <= half an ulp
    of the new bias.  `params` (fp32) is changed in place; lat: the table the kernels will look up (rows inside the max-norm
    bound).  Returns [(layer, row, column)]."""
    planted = []
    x0 = torch.cat([lat.double()[idx], xyz.double()], 1)
    N = x0.shape[0]
    for l in range(net.n_lin - 1):
        _, _, zs, _ = pre_activations(net, dbl(params), x0, masks)
        bias = params[f"lin{l}.bias"]
        for j in range(net.layers[l].out_dim):
            kept = torch.arange(N) if masks is None or masks[l] is None else masks[l][:, j].nonzero().reshape(-1)
            i = int(kept[(37 * j + 11 * l + 5) % kept.numel()])
            bias[j] = (bias[j].double() - zs[l][i, j]).float()
            planted.append((l, i, j))
    return planted


def plant_head_ties(net, params, lat, idx, xyz, masks, gt):
    """Targets and clamp distance on the output's own values (fp64 forward of the planted net): every third point's target is
    fp32(y), eight more sit one fp32 ulp above it and eight one below, and delta = fp32(|y_k|) for the point k in the middle of the
    batch's |y| range, so y_k is on a clamp edge to within rounding and about half of the batch is inside.  Returns (gt [N, 1] fp32,
    delta, dict(tied, above, below, edge))."""
    x0 = torch.cat([lat.double()[idx], xyz.double()], 1)
    y64 = pre_activations(net, dbl(params), x0, masks)[0]
    yf = y64.float()
    N = yf.shape[0]
    gt = gt.clone().float().reshape(N, 1)
    tied, above, below = torch.arange(0, N, 3), torch.arange(1, N, 3)[:8], torch.arange(2, N, 3)[:8]
    gt[tied] = yf[tied]
    gt[above] = torch.nextafter(yf[above], torch.full_like(yf[above], float("inf")))
    gt[below] = torch.nextafter(yf[below], torch.full_like(yf[below], float("-inf")))
    k = int(torch.argsort(y64.abs().reshape(-1))[N // 2])
    delta = float(y64[k, 0].abs().float())
    return gt, delta, dict(tied=tied, above=above, below=below, edge=k)


def head_decisions(y, gt, delta):
    """(sign [N, 1], inside [N, 1]) of clamped_l1 from y and gt as given (exact comparisons in their own precision)."""
    y, gt = y.reshape(-1, 1), gt.reshape(-1, 1)
    return torch.sign(torch.clamp(y, -delta, delta) - torch.clamp(gt, -delta, delta)), (y >= -delta) & (y <= delta)


def analyse(net, params, x0, acts, y, gt, delta, masks, dp_last=None, fwd_tol=1e-5):
    """What a kernel (or the fp32 oracle standing in for one) decided, and whether it was allowed to.

    params: the fp32 parameters; x0 [N, L+G]: the layer-0 input the kernel saw (its renormed rows); acts[l]: the activation it
    stored for hidden layer l ([N, out_l], after ReLU and dropout), or None where it keeps none -- then dp_last [N, out_l], the
    gradient it stored in front of that layer's ReLU, tells the branch on every row whose head gradient is not zero (on the other
    rows the branch cannot reach any gradient; fp64's is taken).  y [N]: its output; masks: the dropout specification.

    Every hidden layer is recomputed in fp64 from the input the KERNEL stored for it, so no error is carried in from earlier layers:
      (b) a stored activation > 0 where z~ < -tau, or == 0 on a kept entry where z~ > tau, is a wrong branch;
      (c) a kept entry must be max(z~, 0) * scale within tau * scale, a dropped one exactly 0.
    The head: sign and inside from the kernel's y may differ from those of y~ (fp64, from the kernel's last hidden activation) only
    where the two compared quantities are within fwd_tol * max|y|.
    Returns dict(relu_keep, head, z, tau, problems: [text], band: [entries inside the band per layer], y64)."""
    p64 = dbl(params)
    Wb = orc.effective_weights(net, p64)
    x0 = x0.double()
    N = x0.shape[0]
    nh = net.n_lin - 1
    scale = 1.0 / (1.0 - net.dropout_prob) if net.dropout_prob < 1.0 else 0.0
    yk = y.reshape(N, 1)
    sign_k, inside_k = head_decisions(yk.float(), gt.float(), delta)
    informative = ((sign_k != 0) & inside_k).reshape(N, 1)
    out = dict(relu_keep=[], z=[], tau=[], problems=[], band=[], head=(sign_k.double(), inside_k))
    a_prev = None
    for l in range(nh + 1):
        ly = net.layers[l]
        inp = x0 if l == 0 else a_prev
        if ly.skip_in:
            inp = torch.cat([inp, x0], 1)
        W, b = Wb[l]
        if l == nh:
            u = inp @ W.t() + b
            break
        z, mag = _lin(net, l, W, b, inp)
        tau = (ly.in_dim + 4) * U32 * mag
        if net.forward_bf16:
            tau = tau + BF16_ULP * (mag - b.abs())
        on = masks is not None and masks[l] is not None and ly.dropout and net.dropout_prob > 0.0
        drop = masks[l].to(torch.bool) if on else torch.ones(N, ly.out_dim, dtype=torch.bool)
        s = scale if on else 1.0
        if acts[l] is not None:
            a = acts[l].double()
            k = a > 0
            known = drop
            if bool(((~drop) & (a != 0)).any()):
                out["problems"].append(f"layer {l}: {int(((~drop) & (a != 0)).sum())} dropped entries are not exactly 0")
            off = drop & ((a - torch.clamp_min(z, 0.0) * s).abs() > tau * s)
            if bool(off.any()):
                i, j = (int(v) for v in off.nonzero()[0])
                out["problems"].append(f"layer {l}: {int(off.sum())} stored activations are not max(z~, 0) * scale within tau * scale, "
                                       f"first [{i}, {j}]: stored {float(a[i, j]):.9e}, z~ {float(z[i, j]):.9e}, tau {float(tau[i, j]):.2e}")
            a_prev = a
        else:
            if dp_last is None or l != nh - 1:
                raise ValueError(f"no stored activation of hidden layer {l} and nothing else that tells its branches")
            known = drop & informative
            k = dp_last.double() != 0
            a_prev = torch.where(torch.where(known, k, z > 0) & drop, z, torch.zeros_like(z)) * s
        wrong_on = known & k & (z < -tau)
        wrong_off = known & (~k) & (z > tau)
        for name, w in (("> 0 where z~ < -tau", wrong_on), ("== 0 on a kept entry where z~ > tau", wrong_off)):
            if bool(w.any()):
                i, j = (int(v) for v in w.nonzero()[0])
                out["problems"].append(f"layer {l}: {int(w.sum())} entries {name}, first [{i}, {j}]: z~ {float(z[i, j]):.9e}, tau {float(tau[i, j]):.2e}")
        out["relu_keep"].append(torch.where(known, k, z > 0))
        out["z"].append(z)
        out["tau"].append(tau)
        out["band"].append(int((drop & (z.abs() <= tau)).sum()))
    t = torch.tanh(u) if net.use_tanh else u
    y64 = torch.tanh(t)
    sign64, inside64 = head_decisions(y64, gt.double(), delta)
    bound = fwd_tol * float(y64.abs().max())
    d64 = (torch.clamp(y64, -delta, delta) - torch.clamp(gt.double().reshape(N, 1), -delta, delta)).abs()
    bad_sign = (sign64 != sign_k.double()) & (d64 > bound)
    bad_inside = (inside64 != inside_k) & ((y64.abs() - delta).abs() > bound)
    if bool(bad_sign.any()):
        out["problems"].append(f"head: {int(bad_sign.sum())} signs differ from fp64's with |clamp(y~) - clamp(gt)| > {bound:.2e}")
    if bool(bad_inside.any()):
        out["problems"].append(f"head: {int(bad_inside.sum())} clamp masks differ from fp64's with ||y~| - delta| > {bound:.2e}")
    out["y64"] = y64
    return out


def flips(planted, relu_keep, z_ref):
    """How many planted entries were decided differently from the fp64 forward z_ref (its own inputs, no forcing)."""
    return sum(int(bool(relu_keep[l][i, j]) != bool(z_ref[l][i, j] > 0)) for l, i, j in planted)


def decisions_from_workspace(ws, rows, spec_in_dims, out_dims, N, merged):
    """The activations the last training call left in its workspace `ws` (uint8 device tensor), through that call's region table
    rows = [(name, offset, bytes)]: acts[l] = in{l+1}[:, :out_l] for every hidden layer (row stride: the layer input width rounded
    up to 4), on the CPU.  merged (forward and backward in one launch): the deepest hidden activation goes from the forward's LDS slab
    straight into the backward head and has no global copy -- acts[-1] is None and dp_last = dpl{nh-1}[:, :out] (row stride: the
    widest layer input rounded up to 4, at least 4) is returned in its place.  Returns (acts, dp_last); ReLU decisions are acts[l] > 0
    (analyse)."""
    table = {name: (off, nb) for name, off, nb in rows}
    nh = len(out_dims)
    ld_in = [(d + 3) // 4 * 4 for d in spec_in_dims]

    def region(name, ld):
        off, nb = table[name]
        assert nb >= N * ld * 4, (name, nb, N, ld)
        return ws[off:off + N * ld * 4].view(torch.float32).view(N, ld).cpu()

    acts, dp_last = [], None
    for l in range(nh):
        if merged and l == nh - 1:
            acts.append(None)
            dp_last = region(f"dpl{l}", max([4] + ld_in))[:, :out_dims[l]].clone()
        else:
            acts.append(region(f"in{l + 1}", ld_in[l + 1])[:, :out_dims[l]].clone())
    return acts, dp_last


# ---- the shared cases -------------------------------------------------------------------------------------------------------------
B_SEG, S_SEG = 4, 64                 # four segments of 64 points: N = 256
DROP_SEED, CODE_BOUND, EPOCH, LAM = 81, 1.0, 130, 1e-4
_CASES = {}


def build_case(name, bf16=False):
    """The planted batch of net `name` (nets()), built once: dict(net, L, kw, params [planted, fp32], lat0, idx, xyz, gt, delta,
    masks, planted, head, z_ref [fp64 pre-activations of the planted net], y_ref)."""
    key = (name, bool(bf16))
    if key in _CASES:
        return _CASES[key]
    import math
    from tests.safe_batch import big_batch
    L, kw = nets()[name]
    net = orc.make_net(L, forward_bf16=bf16, **kw)
    seed = 8100 + 10 * sorted(nets()).index(name)
    params = orc.init_params(net, seed)
    lat0 = torch.randn(B_SEG, L, generator=torch.Generator().manual_seed(seed + 1)) / math.sqrt(L)
    lat0 *= torch.clamp(0.9 / lat0.norm(dim=1, keepdim=True), max=1.0)      # inside the bound: the renorm has its own exact-tie test
    idx, xyz, gt = big_batch(B_SEG, S_SEG, seed + 2, kw["geom_dimension"])
    masks = orc.dropout_masks(net, DROP_SEED, 0, xyz.shape[0])
    planted = plant_relu_ties(net, params, lat0, idx, xyz, masks)
    gt, delta, head = plant_head_ties(net, params, lat0, idx, xyz, masks, gt)
    x0 = torch.cat([lat0.double()[idx], xyz.double()], 1)
    y_ref, _, z_ref, mag = pre_activations(net, dbl(params), x0, masks)
    _CASES[key] = dict(net=net, L=L, kw=dict(kw, forward_bf16=True) if bf16 else dict(kw), params=params, lat0=lat0, idx=idx, xyz=xyz,
                       gt=gt, delta=delta, masks=masks, planted=planted, head=head, z_ref=z_ref, mag_ref=mag, y_ref=y_ref)
    return _CASES[key]


def oracle_step(c, decisions=None, dtype=torch.float64):
    """One step_gradients of case c in `dtype` (fresh copies of the table), forced onto `decisions` or not."""
    cast = (lambda t: t.double()) if dtype == torch.float64 else (lambda t: t.float())
    return orc.step_gradients(c["net"], {k: cast(v) for k, v in c["params"].items()}, cast(c["lat0"]).clone(), c["idx"], cast(c["xyz"]),
                              cast(c["gt"]), delta=c["delta"], code_bound=CODE_BOUND, code_reg=True, code_reg_lambda=LAM, epoch=EPOCH,
                              training=True, masks=c["masks"], decisions=decisions)
