"""CPU: the oracle (oracle/deepsdf_oracle.py) against every golden vector generated from the reference.

Tolerances (written here, per north_star): forward SDF <= 1e-5 rel, gradients <= 1e-4 rel (norm-wise),
post-Adam parameters <= 1e-5 rel.  Observed oracle-vs-reference errors are ~1e-7."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import deepsdf_oracle as orc
from tests.golden_io import GOLDEN, Golden, rel_err

FWD_TOL, GRAD_TOL, PARAM_TOL = 1e-5, 1e-4, 1e-5

TRAIN_CASES = ["g1a_tiny_full", "g1b_lastnorm_tanh", "g1c_plain_clip", "g2_8x512_slice", "g3a_dropout_tiny",
               "g3b_dropout_8x512", "g4_batch_split2",
               # the Decoder variants no shipped spec uses: xyz_in_all, latent_dropout (+ batch_split 2), LayerNorm (incl. the
               # bn module of the last Linear, which forward never calls: zero gradient, no Adam movement)
               "g11a_xyz_in_all", "g11b_latent_dropout", "g11c_layer_norm",
               # away from CodeBound 1.0 / ClampingDistance 0.1 / lambda 1e-4 / torch's Adam defaults
               "g14a_off_point_tight", "g14b_off_point_loose"]


def run_case(name):
    g = Golden(name)
    m = g.meta
    net = orc.make_net(m["L"], **m["net_specs"])
    params = g.group("params0") if m["store"] == "full" else orc.init_params(net, m["seed"])
    st = orc.TrainState.create({k: v.clone() for k, v in params.items()}, g.get("lat0/w").clone())
    res = []
    for si in range(m["n_steps"]):
        i = g.group(f"step{si}/in")
        r = orc.train_step(net, st, i["idx"], i["xyz"], i["gt"], delta=m["delta"], code_bound=m["code_bound"],
                           code_reg=m["code_reg"], code_reg_lambda=m["lam"], epoch=m["epoch"],
                           lr_decoder=m["lr"][0], lr_latent=m["lr"][1], batch_split=m["batch_split"],
                           grad_clip=m["grad_clip"], training=True, seed=m["drop_seed"],
                           betas=tuple(m.get("betas", (0.9, 0.999))), eps=m.get("eps", 1e-8))     # (older goldens: torch's defaults)
        res.append(r)
        o = g.group(f"step{si}/out")
        assert abs(r["loss"] - float(o["loss"])) <= 1e-5 * abs(float(o["loss"])) + 1e-9, (name, si)
        assert rel_err(r["dlat"], g.get(f"step{si}/dlat/w")) <= GRAD_TOL, (name, si)
        assert rel_err(st.latents, g.get(f"step{si}/lat_after/w")) <= PARAM_TOL, (name, si)
        gg = g.group(f"step{si}/grads")
        if m["grad_clip"] is None:
            for k, ref in gg.items():
                assert rel_err(r["grads"][k], ref) <= GRAD_TOL, (name, si, k)
        else:
            assert abs(float(r["grad_norm"]) - float(o["grad_norm"])) <= 1e-4 * float(o["grad_norm"])
        for k, ref in g.group(f"step{si}/grads_fro").items():
            assert abs(float(r["grads"][k].double().norm()) - float(ref)) <= GRAD_TOL * float(ref), (name, si, k)
        for k, ref in g.group(f"step{si}/grads_corner").items():
            scale = float(r["grads"][k].abs().max())
            assert float((r["grads"][k][:8, :8] - ref).abs().max()) <= GRAD_TOL * scale, (name, si, k)
        for k, ref in g.group(f"step{si}/params_after").items():
            assert rel_err(st.params[k], ref) <= PARAM_TOL, (name, si, k)
        for k, ref in g.group(f"step{si}/params_after_fro").items():
            assert abs(float(st.params[k].double().norm()) - float(ref)) <= PARAM_TOL * float(ref), (name, si, k)
        for k, ref in g.group(f"step{si}/adam_m").items():
            mine = st.m_lat if k == "latent" else st.m[k]
            assert rel_err(mine, ref) <= GRAD_TOL, (name, si, "m", k)
        for k, ref in g.group(f"step{si}/adam_v").items():
            mine = st.v_lat if k == "latent" else st.v[k]
            assert rel_err(mine, ref) <= 2 * GRAD_TOL, (name, si, "v", k)
    return g, st, res


@pytest.mark.parametrize("name", TRAIN_CASES)
def test_train_cases(name):
    run_case(name)


def test_forward_y_matches():
    for name in ["g1a_tiny_full", "g3a_dropout_tiny"]:
        g = Golden(name)
        m = g.meta
        net = orc.make_net(m["L"], **m["net_specs"])
        params = g.group("params0")
        lat = g.get("lat0/w").clone()
        i = g.group("step0/in")
        orc.renorm_rows_(lat, i["idx"], m["code_bound"])
        x0 = torch.cat([lat[i["idx"]], i["xyz"]], 1)
        masks = orc.dropout_masks(net, m["drop_seed"], 0, x0.shape[0]) if m["dropout_train"] else None
        y, _ = orc.decoder_forward(net, params, x0, training=True, masks=masks)
        assert rel_err(y, g.get("step0/out/y")) <= FWD_TOL


def test_renorm_fired_and_absent_row_moves():
    g, st, res = run_case("g1a_tiny_full")
    lat0 = g.get("lat0/w")
    assert float(lat0[1].norm()) > 2.9                      # started above CodeBound
    # step 1 omits scene 2: zero gradient, yet the row keeps moving through Adam momentum (dense Adam)
    assert float(res[1]["dlat"][2].abs().max()) == 0.0
    after0, after1 = g.get("step0/lat_after/w"), g.get("step1/lat_after/w")
    assert float((after1[2] - after0[2]).abs().max()) > 1e-5


def test_batch_split_equals_unsplit():
    g = Golden("g4_batch_split2")
    m = g.meta
    net = orc.make_net(m["L"], **m["net_specs"])
    outs = []
    for bs in (1, 2):
        st = orc.TrainState.create({k: v.clone() for k, v in g.group("params0").items()}, g.get("lat0/w").clone())
        i = g.group("step0/in")
        r = orc.train_step(net, st, i["idx"], i["xyz"], i["gt"], delta=m["delta"], code_bound=m["code_bound"],
                           epoch=m["epoch"], batch_split=bs, seed=m["drop_seed"])
        outs.append((r, st))
    for k in outs[0][0]["grads"]:
        assert rel_err(outs[0][0]["grads"][k], outs[1][0]["grads"][k]) <= 1e-5
    assert abs(outs[0][0]["loss"] - outs[1][0]["loss"]) < 1e-7


def test_lr_schedules():
    d = json.load(open(os.path.join(GOLDEN, "g5_lr_schedules.json")))
    for spec, row in zip(d["specs"], d["values"]):
        for e, v in zip(d["epochs"], row):
            assert orc.learning_rate(spec, e) == v
    with pytest.raises(Exception, match="no known learning rate schedule"):
        orc.learning_rate({"Type": "Cosine"}, 1)


def test_real_weights_known_answer():
    """G6: weights of experiments/corner_spheres_only_small_network (shipped by the reference);
    f(0) = -0.1340 is the value the reference's own TorchScript export returns."""
    g = Golden("g6_real_weights")
    net = orc.make_net(g.meta["L"], **g.meta["net_specs"])
    params = g.group("params")
    for k, logged in g.meta["logged_norms"].items():       # assignment check vs the reference's Logs.pth
        assert abs(float(params[k].norm()) - logged) <= 1e-6 * logged
    y, _ = orc.decoder_forward(net, params, torch.zeros(1, g.meta["L"] + 3), training=False)
    assert abs(float(y) - g.meta["f0_survey"]) < 5e-5


def test_latent_only():
    g = Golden("g7_latent_only")
    m = g.meta
    net = orc.make_net(m["L"], **m["net_specs"])
    params = g.group("params0")
    z = g.get("z0/z").clone()
    mm, vv = torch.zeros_like(z), torch.zeros_like(z)
    for it in range(m["iters"]):
        d = g.group(f"it{it}")
        loss, dz = orc.latent_step(net, params, z, mm, vv, it + 1, d["xyz"], d["gt"], delta=m["delta"], lr=m["lr"],
                                   l2reg=m["l2reg"])
        assert abs(loss - float(d["loss"])) <= 1e-5 * abs(float(d["loss"]))
        assert rel_err(dz, d["dz"]) <= GRAD_TOL
        assert rel_err(z, d["z_after"]) <= PARAM_TOL


@pytest.mark.parametrize("name", ["g8_eval_8x512", "g8_eval_6x128"])
def test_eval_forward(name):
    g = Golden(name)
    net = orc.make_net(g.meta["L"], **g.meta["net_specs"])
    params = orc.init_params(net, g.meta["seed"])
    y, _ = orc.decoder_forward(net, params, g.get("in/x"), training=False)
    assert rel_err(y, g.get("out/y")) <= FWD_TOL


def test_dropout_hash_properties():
    key = orc.dropout_layer_key(1234, 5, 3)
    keep = orc.dropout_keep(key, 4096, 512, 0.2)
    frac = keep.mean()
    assert abs(frac - 0.8) < 2e-3
    # row_offset consistency: a chunk starting at row r sees the same bits as the full batch
    part = orc.dropout_keep(key, 100, 512, 0.2, row_offset=37)
    assert (part == keep[37:137]).all()
    # different layers / steps decorrelate
    other = orc.dropout_keep(orc.dropout_layer_key(1234, 6, 3), 4096, 512, 0.2)
    assert abs((keep == other).mean() - (0.8 * 0.8 + 0.2 * 0.2)) < 5e-3
    assert orc.dropout_threshold16(0.2) == 13107


def test_torch_native_restatement_agrees_with_oracle_and_golden():
    """oracle/torch_native.py (stock torch ops + autograd + torch.optim.Adam: the op sequence bench.py times as the CPU baseline)
    reproduces the reference-generated golden g3a (dropout-injected training, 2 steps incl. renorm + dense Adam) and the
    explicit-algebra oracle."""
    from oracle.torch_native import NativeStep
    g = Golden("g3a_dropout_tiny")
    m = g.meta
    net = orc.make_net(m["L"], **m["net_specs"])
    params = g.group("params0")
    st = orc.TrainState.create({k: v.clone() for k, v in params.items()}, g.get("lat0/w").clone())
    nat = NativeStep(net, params, g.get("lat0/w"), code_bound=m["code_bound"], lr_decoder=m["lr"][0], lr_latent=m["lr"][1])
    for si in range(m["n_steps"]):
        i = g.group(f"step{si}/in")
        loss = nat.step(i["idx"], i["xyz"], i["gt"], delta=m["delta"], code_reg=m["code_reg"], code_reg_lambda=m["lam"],
                        epoch=m["epoch"], seed=m["drop_seed"])
        ro = orc.train_step(net, st, i["idx"], i["xyz"], i["gt"], delta=m["delta"], code_bound=m["code_bound"],
                            code_reg=m["code_reg"], code_reg_lambda=m["lam"], epoch=m["epoch"], lr_decoder=m["lr"][0],
                            lr_latent=m["lr"][1], seed=m["drop_seed"])
        assert abs(loss - float(g.group(f"step{si}/out")["loss"])) <= 1e-6 * abs(loss)
        assert abs(loss - ro["loss"]) <= 1e-6 * abs(loss)
        for k, ref in g.group(f"step{si}/params_after").items():
            assert rel_err(nat.params[k].detach(), ref) <= 1e-6, (si, k)
            assert rel_err(nat.params[k].detach(), st.params[k]) <= 1e-6, (si, k)
        assert rel_err(nat.lat.weight.detach(), g.get(f"step{si}/lat_after/w")) <= 1e-6
