"""GPU parity tests of the whole training step over the SE-ResNet-18/34 encoders.

The oracle is the unchanged OracleTrainer with oracle.nets._resnet_encoder replaced, for the duration of a test, by the encoder of
tests/_se_reference.py (the gate on the residual branch of every basic unit) and the SE tensors added to its parameters; it is called with
backbone 'resnet18' / 'resnet34'.  The arithmetic of the gate is fixed by this repository (include/stp_hip.h, stp_se_*), not pinned by the
reference.  fp32 bars are those of tests/test_model_gpu.py::test_fp32_step_matches_oracle for its ResNet-18/34 rows, unchanged.
"""
import numpy as np
import pytest
import torch

import _se_reference as R

pytestmark = pytest.mark.gpu

from oracle import nets as onets  # noqa: E402
from oracle import step as ostep  # noqa: E402

LOSS = "binary_crossentropy+1.0*dice_loss"
# oracle tap -> plan tensor, in forward order (localises a mismatch)
TAP_MAP = [("bn_data", "bn_data"), ("conv0", "conv0"), ("relu0", "bn0"), ("pooling0", "pooling0"), ("stage1_unit1_relu1", "stage1_unit1_bn1"),
           ("stage1_unit1_out", "stage1_unit1_se"), ("stage1_unit2_out", "stage1_unit2_se"), ("stage2_unit1_out", "stage2_unit1_se"),
           ("stage3_unit1_out", "stage3_unit1_se"), ("stage4_unit1_out", "stage4_unit1_se"), ("stage4_unit2_out", "stage4_unit2_se"),
           ("relu1", "bn1")]


def make(arch, backbone, size, n, dtype, use_graph=False, **kw):
    from segmentation_training_pipeline_amd.backend import HipSegModel
    return HipSegModel(arch, backbone, (size, size, 3), 1, "sigmoid", batch=n, dtype=dtype, loss=kw.pop("loss", LOSS),
                       optimizer=kw.pop("optimizer", "Adam"), lr=kw.pop("lr", 1e-3), use_graph=use_graph, **kw)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


def first_bad_tap(model, taps, atol):
    for oname, pname in TAP_MAP:
        if oname not in taps or pname not in model.plan.tensors:
            continue
        ref = taps[oname].detach().numpy()
        got = model.activation(pname)[..., :ref.shape[-1]]
        err = np.abs(got - ref).max()
        if not err <= atol * max(1.0, np.abs(ref).max()):
            return "%s: max err %.3g (ref max %.3g)" % (pname, err, np.abs(ref).max())
    return None


@pytest.mark.parametrize("b2_range", [0.0, 2.0], ids=["own_init", "b2_pm2"])
@pytest.mark.parametrize("arch,backbone,size", [("Unet", "seresnet18", 64), ("Unet", "seresnet34", 64), ("Linknet", "seresnet18", 64),
                                                ("FPN", "seresnet18", 64), ("PSPNet", "seresnet18", 96)])
def test_fp32_step_matches_oracle(arch, backbone, size, b2_range, monkeypatch):
    R.install(monkeypatch)
    n = 2
    P = R.init(arch, backbone, seed=42, b2_range=b2_range)
    x, y = ostep.synthetic_batch(n, size, size, seed=1234)
    kw = dict(optimizer="sgd", lr=0.05, opt_kwargs={"momentum": 0.9})
    tr = ostep.OracleTrainer(P, backbone=R.BASE[backbone], loss=LOSS, architecture=arch, **kw)
    m = make(arch, backbone, size, n, "fp32", optimizer="SGD", lr=0.05, opt_kwargs={"momentum": 0.9})
    assert sorted(m.get_weights()) == sorted(P)            # same parameter names as the oracle's Keras layout
    own = m.get_weights()
    for k in R.se_names(P):
        assert own[k].shape == P[k].shape, k
        if k.endswith("bias"):
            assert not own[k].any(), k                     # the model's own initialisation: zero biases, he_uniform kernels
        else:
            lim = np.sqrt(6.0 / own[k].shape[2])
            assert 0.5 * lim < np.abs(own[k]).max() <= lim, k
    m.set_weights(P)
    taps = {}
    o = tr.step(x.astype(np.float32), y.astype(np.float32), taps=taps)
    m.load_batch(x, y)
    m.forward_backward()
    bad = first_bad_tap(m, taps, 2e-4)
    m.apply_gradients()
    met = m.metrics()
    assert bad is None, bad
    np.testing.assert_allclose(m.logits(), o["logits"], atol=1e-3)
    assert abs(met["dice_loss"] - o["dice_loss"]) < 1e-5
    assert abs(met["loss"] - o["loss"]) < 1e-5 * max(1.0, abs(o["loss"]))
    g = m.get_gradients()
    worst = {}
    for k, ref in o["grads"].items():
        e = rel_l2(g[k], ref)
        if "_se_fc" in k:
            kind = k.split("_se_")[1]
            worst[kind] = max(worst.get(kind, 0.0), e)
        assert e <= (1e-4 if k.startswith("final_conv") else 3e-2), "grad %s: rel L2 %.3g" % (k, e)
    print("SE gradients, worst relative L2 by tensor kind:", {k: "%.2g" % v for k, v in worst.items()})
    w = m.get_weights()
    for k in tr.P:
        np.testing.assert_allclose(w[k], tr.P[k], atol=2e-4, err_msg=k)
    # second step after re-synchronising the weights: the forward agrees again, the momentum update carries over
    m.set_weights(tr.P)
    o2 = tr.step(x.astype(np.float32), y.astype(np.float32))
    met2 = m.train_on_batch(x, y)
    np.testing.assert_allclose(m.logits(), o2["logits"], atol=1e-3)
    assert abs(met2["dice_loss"] - o2["dice_loss"]) < 1e-5
    w = m.get_weights()
    for k in tr.P:
        np.testing.assert_allclose(w[k], tr.P[k], atol=2e-4, err_msg=k)


# Measured on MI355X (U-Net / seresnet34, 2 x 128 x 128, b2 in +-2; also in DESIGN.md 3.19), device vs the storage-quantised oracle | that
# oracle vs its float64-accumulation twin (the same rounding points evaluated a second, equally valid way = the noise floor of the step):
#   bf16: logits max 17.6 / mean 1.92 storage ulp, gradient cosine min 0.731 / median 0.876   |  15.5 / 1.90, 0.436 / 0.886
#   fp16: logits max 17.1 / mean 2.18 storage ulp, gradient cosine min 0.933 / median 0.984   |  16.0 / 2.20, 0.942 / 0.981
# i.e. the device sits at the floor; the test holds it to 1.5 x the floor it measures itself and fixes no absolute ulp bar.
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_step_matches_the_storage_quantised_oracle(dtype, monkeypatch):
    """U-Net / seresnet34 at its 16-bit precisions (fp16: loss scale 2^14, which every SE gradient carries like any other gradient of
    the arena) against the oracle that rounds where the kernels round: u, x and du are stored tensors, z / h / s and the parameter
    gradients stay fp32.  Held to the yardstick test_16bit_step_of_the_other_graphs_matches_the_storage_quantised_oracle measures
    itself: mean logit error <= 1.5 x the distance between the oracle and its accum64 twin + 0.25 storage ulp, median gradient cosine
    within 1.5 x the twin's + 0.01."""
    R.install(monkeypatch)
    # (the decoder's class-collapsed weight copies - sums of taps rounded once more - are a rounding point the oracle does not have)
    monkeypatch.setenv("STP_UPCOLLAPSE", "0")
    n, size, backbone = 2, 128, "seresnet34"
    P = R.init("Unet", backbone, seed=42, b2_range=2.0)
    x, y = ostep.synthetic_batch(n, size, size, seed=1234)
    m = make("Unet", backbone, size, n, dtype)
    gs = m.loss_scale
    assert gs == (16384.0 if dtype == "fp16" else 1.0)
    kw = dict(backbone=R.BASE[backbone], loss=LOSS, optimizer="adam", lr=1e-3, storage=dtype, grad_scale=gs)
    o = ostep.OracleTrainer(P, **kw).step(x.astype(np.float32), y.astype(np.float32), apply=False)
    o64 = ostep.OracleTrainer(P, accum64=True, **kw).step(x.astype(np.float32), y.astype(np.float32), apply=False)
    m.set_weights(P)
    m.load_batch(x, y)
    m.forward_backward()
    met = m.metrics()
    ref, got = o["logits"], m.logits()
    rng_ = float(np.abs(ref).max())
    ulp = 2.0 ** (np.floor(np.log2(rng_)) - (7 if dtype == "bf16" else 10))
    err, floor = np.abs(got - ref), np.abs(o64["logits"] - ref)
    got_g = m.get_gradients()

    def cosines(ga):
        out = {}
        for k, r in o["grads"].items():
            if r.size > 64:
                a, b = ga[k].ravel().astype(np.float64), r.ravel().astype(np.float64)
                out[k] = a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30)
        return out
    cos, cos_floor = cosines(got_g), cosines(o64["grads"])
    srt, srt_f = sorted(cos.values()), sorted(cos_floor.values())
    se = sorted(v for k, v in cos.items() if "_se_fc" in k)
    se_f = sorted(v for k, v in cos_floor.items() if "_se_fc" in k)
    print("[%s] logit range %.3f ulp %.4g: device max %.2f ulp mean %.3f ulp | floor max %.2f ulp mean %.3f ulp; loss %.5f (oracle %.5f)"
          % (dtype, rng_, ulp, err.max() / ulp, err.mean() / ulp, floor.max() / ulp, floor.mean() / ulp, met["loss"], o["loss"]))
    print("[%s] gradient cosine: device min %.5f median %.5f | floor min %.5f median %.5f; SE tensors: device min %.5f median %.5f | floor min "
          "%.5f median %.5f" % (dtype, srt[0], srt[len(srt) // 2], srt_f[0], srt_f[len(srt_f) // 2], se[0], se[len(se) // 2], se_f[0],
                                se_f[len(se_f) // 2]))
    assert np.isfinite(got).all() and all(np.isfinite(v).all() for v in got_g.values())
    assert err.mean() <= 1.5 * floor.mean() + 0.25 * ulp, (err.mean() / ulp, floor.mean() / ulp)
    assert 1.0 - srt[len(srt) // 2] <= 1.5 * (1.0 - srt_f[len(srt_f) // 2]) + 0.01, (srt[len(srt) // 2], srt_f[len(srt_f) // 2])
    # every SE tensor received a gradient at the oracle's scale: the fp16 loss scale (2^14) is divided out like everywhere else in the
    # arena - a missed or doubled scale would show as a factor of 16384, rounding noise stays far inside a factor of 16
    for k in R.se_names(P):
        a, b = np.linalg.norm(got_g[k]), np.linalg.norm(o["grads"][k])
        assert a > 0 and 1.0 / 16 < a / (b + 1e-30) < 16.0, (k, a, b)


@pytest.mark.parametrize("arch", ["Unet", "Linknet"])
def test_hipgraph_replay_equals_eager(arch):
    P = R.init(arch, "seresnet18", seed=7, b2_range=2.0)
    x, y = ostep.synthetic_batch(2, 64, 64, seed=5)
    outs = []
    for use_graph in (False, True):
        m = make(arch, "seresnet18", 64, 2, "bf16", use_graph=use_graph)
        m.set_weights(P)
        r = [m.train_on_batch(x, y) for _ in range(3)]
        outs.append((r, m.logits(), m.get_weights()))
    assert outs[0][0] == outs[1][0]                        # bitwise: every reduction has a fixed order
    np.testing.assert_array_equal(outs[0][1], outs[1][1])
    for k in outs[0][2]:
        np.testing.assert_array_equal(outs[0][2][k], outs[1][2][k], err_msg=k)


def test_predict_and_checkpoint_round_trip(tmp_path, monkeypatch):
    R.install(monkeypatch)
    n, size = 2, 64
    P = R.init("Unet", "seresnet18", seed=3, b2_range=2.0)
    x, y = ostep.synthetic_batch(n, size, size, seed=9)
    m = make("Unet", "seresnet18", size, n, "fp32")
    m.set_weights(P)
    for _ in range(2):
        m.train_on_batch(x, y)
    w = m.get_weights()
    # inference plan (moving statistics; squeeze, excite, scale-add without the table) vs the oracle's training=False forward, 3 images
    tr = ostep.OracleTrainer(P, backbone="resnet18", loss=LOSS)
    tr.P.update({k: w[k] for k in w})
    x3 = np.concatenate([x, x[:1]], axis=0)
    ref = torch.sigmoid(torch.from_numpy(tr.forward(x3.astype(np.float32), training=False))).numpy()
    np.testing.assert_allclose(m.predict(x3), ref, atol=2e-4)
    path = str(tmp_path / "best-0.0.weights")
    m.save_weights(path)
    m2 = make("Unet", "seresnet18", size, n, "fp32")
    m2.load_weights(path)
    w2 = m2.get_weights()
    assert len(R.se_names(w2)) == 32
    for k in w:
        np.testing.assert_array_equal(w[k], w2[k], err_msg=k)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_ten_adam_steps_lower_the_loss_and_move_every_se_tensor(dtype):
    x, y = ostep.synthetic_batch(2, 64, 64, seed=11)
    m = make("Unet", "seresnet34", 64, 2, dtype, use_graph=True)
    w0 = m.get_weights()
    losses = [m.train_on_batch(x, y)["loss"] for _ in range(10)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    w1 = m.get_weights()
    se = R.se_names(w0)
    assert len(se) == 64
    for k in se:
        assert np.isfinite(w1[k]).all() and np.abs(w1[k] - w0[k]).max() > 0, k


def test_frozen_encoder_keeps_the_se_tensors_and_unfreeze_releases_them():
    x, y = ostep.synthetic_batch(2, 64, 64, seed=11)
    m = make("Unet", "seresnet18", 64, 2, "bf16", freeze_encoder=True)
    w0 = m.get_weights()
    for _ in range(2):
        m.train_on_batch(x, y)
    w1 = m.get_weights()
    for k in R.se_names(w0):
        np.testing.assert_array_equal(w1[k], w0[k], err_msg=k)
    assert np.abs(w1["decoder_stage0_conv1/kernel"] - w0["decoder_stage0_conv1/kernel"]).max() > 0


def test_warm_start_from_a_resnet34_checkpoint(tmp_path):
    """No SE-ResNet ImageNet file exists offline: users start these encoders from a ResNet checkpoint given as `encoder_weights: <path>`.
    Every tensor the file has lands in the plan; the SE tensors, which it lacks, keep their initialisation."""
    from segmentation_training_pipeline_amd import models
    src = make("Unet", "resnet34", 64, 2, "fp32", seed=5)
    x, y = ostep.synthetic_batch(2, 64, 64, seed=2)
    src.train_on_batch(x, y)                                # (moving statistics and weights away from their initial values)
    path = str(tmp_path / "resnet34_unet.weights")
    src.save_weights(path)
    saved = src.get_weights()
    fresh = make("Unet", "seresnet34", 64, 2, "fp32").get_weights()          # the initialisation of the default seed
    mdl = models.Unet(backbone_name="seresnet34", input_shape=(64, 64, 3), classes=1, activation="sigmoid", encoder_weights=path)
    mdl.compile(batch=2, dtype="fp32")
    w = mdl.impl.get_weights()
    se = R.se_names(w)
    assert len(se) == 64 and not set(se) & set(saved)
    for k in saved:
        np.testing.assert_array_equal(w[k], saved[k], err_msg=k)
    for k in se:
        np.testing.assert_array_equal(w[k], fresh[k], err_msg=k)
    assert np.isfinite(mdl.train_on_batch(x, y)["loss"])


def test_the_plain_encoder_is_untouched():
    m = make("Unet", "resnet34", 64, 2, "bf16")
    plan = m.plan
    names = [r[2] for r in plan.fwd + plan.bwd + plan.prep + plan.opt]
    assert not [k for k in names if k and k.startswith("stp_se_")]
    assert not [k for k in plan.params if "_se_" in k]
    # conv2 of every unit still carries the residual operand and the fused statistics
    by_layer = {(rec[3] or {}).get("layer"): rec for rec in plan.fwd if rec[2] == "stp_conv2d"}
    units = [k for k in by_layer if k and k.startswith("stage") and k.endswith("_conv2")]
    assert len(units) == 16
    for k in units:
        p = by_layer[k][1][0]._obj
        assert p.residual and p.stats_partial, k
    # ... and in the SE plan it carries neither
    s = make("Unet", "seresnet34", 64, 2, "bf16").plan
    by_layer = {(rec[3] or {}).get("layer"): rec for rec in s.fwd if rec[2] == "stp_conv2d"}
    for k in units:
        p = by_layer[k][1][0]._obj
        assert not p.residual and not p.stats_partial, k
    assert [r[2] for r in s.fwd].count("stp_se_scale_add") == 16
