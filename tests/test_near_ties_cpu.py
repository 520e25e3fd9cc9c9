"""The near-tie batches do what they claim, with the fp32 oracle standing in for a kernel: the planted entries are
ties to within a rounding, fp32 and fp64 take different branches on many of them, that alone puts the plain fp64 comparison
far outside the gradient tolerance -- and the fp64 oracle forced onto the fp32 run's own decisions agrees with it again.  Also the
oracle's own contract: forcing a run onto ITS decisions changes nothing, bit for bit."""
import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests import near_ties as NT
from tests.golden_io import rel_err, worst_elem

GRAD_TOL, GRAD_ELEM_TOL = 1e-4, 1e-4          # tests/test_gpu_parity.py's
NETS = sorted(NT.nets())


def _own_decisions(r, c):
    sv = r["saved"]
    keep = []
    for l, a in enumerate(sv.acts):
        k = a > 0
        if sv.drop_keep[l] is not None:          # a dropped entry's branch: from nothing it stored -- any value must do
            k = k | ~sv.drop_keep[l]
        keep.append(k)
    return dict(relu_keep=keep, head=NT.head_decisions(r["y"], c["gt"].to(r["y"].dtype), c["delta"]))


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_forcing_a_run_onto_its_own_decisions_changes_nothing(name, dtype):
    c = NT.build_case(name)
    r = NT.oracle_step(c, dtype=dtype)
    f = NT.oracle_step(c, decisions=_own_decisions(r, c), dtype=dtype)
    assert torch.equal(r["loss"], f["loss"]) and torch.equal(r["y"], f["y"])
    assert torch.equal(r["dlat"], f["dlat"]) and torch.equal(r["dx0"], f["dx0"])
    for k in r["grads"]:
        assert torch.equal(r["grads"][k], f["grads"][k]), k
    # ... and through train_step, which hands them on
    st = [orc.TrainState.create({k: v.to(dtype).clone() for k, v in c["params"].items()}, c["lat0"].to(dtype).clone()) for _ in range(2)]
    kw = dict(delta=c["delta"], code_bound=NT.CODE_BOUND, epoch=NT.EPOCH, seed=NT.DROP_SEED)
    a = orc.train_step(c["net"], st[0], c["idx"], c["xyz"].to(dtype), c["gt"].to(dtype), **kw)
    b = orc.train_step(c["net"], st[1], c["idx"], c["xyz"].to(dtype), c["gt"].to(dtype), decisions=_own_decisions(r, c), **kw)
    assert a["loss"] == b["loss"] and all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])
    assert all(torch.equal(st[0].params[k], st[1].params[k]) for k in st[0].params) and torch.equal(st[0].latents, st[1].latents)


def _hidden(net, k):
    return int(k.split(".")[0][3:]) < net.n_lin - 1


@pytest.mark.parametrize("name", NETS)
def test_planted_batches_tell_a_flipped_tie_from_a_wrong_gradient(name):
    c = NT.build_case(name)
    net, N = c["net"], c["xyz"].shape[0]
    # every planted entry is a tie to within the rounding of its own bias
    for l, i, j in c["planted"]:
        assert abs(float(c["z_ref"][l][i, j])) <= NT.U32 * float(c["mag_ref"][l][i, j]), (l, i, j)
        assert c["masks"][l] is None or bool(c["masks"][l][i, j])
    r32 = NT.oracle_step(c, dtype=torch.float32)
    an = NT.analyse(net, c["params"], r32["saved"].x0, r32["saved"].acts, r32["y"], c["gt"], c["delta"], c["masks"])
    assert not an["problems"], an["problems"]
    n_flip = NT.flips(c["planted"], an["relu_keep"], c["z_ref"])
    print(f"\n{name}: {len(c['planted'])} planted entries, fp32 decides {n_flip} of them differently from fp64; entries inside the band per layer {an['band']}")
    assert 4 * n_flip >= len(c["planted"])
    for l in range(net.n_lin - 1):       # the forced oracle IS the fp64 oracle everywhere else
        assert an["band"][l] * N <= 2 * N * net.layers[l].out_dim, (l, an["band"])
        diff = an["relu_keep"][l] != (an["z"][l] > 0)
        assert not bool((diff & (an["z"][l].abs() > an["tau"][l])).any()), l
    # the head: some of the planted targets fall on the other side in fp32
    s64, i64 = NT.head_decisions(c["y_ref"], c["gt"].double(), c["delta"])
    tied = c["head"]["tied"]
    n_sign = int((an["head"][0][tied] != s64[tied]).sum())
    print(f"{name}: {n_sign} of {tied.numel()} tied targets get another sign in fp32; clamp mask differs on {int((an['head'][1] != i64).sum())} points")
    assert n_sign > 0
    plain, forced = NT.oracle_step(c), NT.oracle_step(c, decisions=dict(relu_keep=an["relu_keep"], head=an["head"]))
    worst_plain = max(rel_err(r32["grads"][k], plain["grads"][k]) for k in plain["grads"] if _hidden(net, k))
    print(f"{name}: worst hidden-layer tensor against the plain fp64 oracle {worst_plain:.2e}")
    assert worst_plain >= 100 * GRAD_TOL
    assert abs(float(r32["loss"]) - float(forced["loss"])) <= 1e-5 * abs(float(forced["loss"]))
    for k in forced["grads"]:
        e, w = rel_err(r32["grads"][k], forced["grads"][k]), worst_elem(r32["grads"][k], forced["grads"][k])
        assert e <= GRAD_TOL and w <= GRAD_ELEM_TOL, (k, e, w)
    assert rel_err(r32["dlat"], forced["dlat"]) <= GRAD_TOL and rel_err(r32["dx0"], forced["dx0"]) <= GRAD_TOL


def test_bf16_emulation_forced_onto_the_fp32_runs_decisions():
    """The config-5 form of the widest net: the fp32 run of the bf16 emulation against the fp64 run of it, forced (the tolerances of
    tests/test_gpu_parity.py's bf16 test: its weights are bf16 roundings of values that differ in the last fp32 place)."""
    c = NT.build_case("w136", bf16=True)
    r32 = NT.oracle_step(c, dtype=torch.float32)
    an = NT.analyse(c["net"], c["params"], r32["saved"].x0, r32["saved"].acts, r32["y"], c["gt"], c["delta"], c["masks"])
    assert not an["problems"], an["problems"]
    forced = NT.oracle_step(c, decisions=dict(relu_keep=an["relu_keep"], head=an["head"]))
    assert abs(float(r32["loss"]) - float(forced["loss"])) <= 1e-4 * abs(float(forced["loss"]))
    for k in forced["grads"]:
        assert rel_err(r32["grads"][k], forced["grads"][k]) <= 1e-2, k
    assert rel_err(r32["dlat"], forced["dlat"]) <= 1e-2
