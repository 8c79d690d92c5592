"""lovasz_softmax on the multi-class softmax head, on the GPU, at model level: one training step of each segmentation_models graph with the
term evaluated by tests/_lovasz_softmax_reference.py on the model's own logits, graph replay, the 16-bit builds with their loss scales, a
short validation batch, and a YAML experiment end to end.  Bars: the term within 2e-5 * max(1, |ref|) (tests/test_lovasz_softmax_ops_gpu.py)."""
import csv
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lovasz_softmax_reference as R  # noqa: E402
from oracle import nets as onets  # noqa: E402
from test_softmax_losses_gpu import LabelSet, label_discs  # noqa: E402

SPEC = "categorical_crossentropy+0.5*lovasz_softmax"


def model(arch="Unet", backbone="resnet18", size=64, classes=3, n=2, dtype="fp32", loss=SPEC, **kw):
    from segmentation_training_pipeline_amd.backend import HipSegModel
    kw.setdefault("use_graph", False)
    kw.setdefault("optimizer", "Adam")
    kw.setdefault("lr", 1e-3)
    return HipSegModel(arch, backbone, (size, size, 3), classes, "softmax", batch=n, dtype=dtype, loss=loss, **kw)


def fwd_names(m):
    return [name for _fn, _a, name, _m in m.plan.fwd if name]


def check_step(m, x, y, classes, ignore_label=None):
    met = m.train_on_batch(x, y)
    ref = R.reference(m.logits().reshape(-1, classes), y.reshape(-1), ignore_label)
    print("lovasz_softmax %.9g ref %.9g loss %.9g cce %.9g" % (met["lovasz_softmax"], ref["value"], met["loss"], met["categorical_crossentropy"]))
    assert abs(met["lovasz_softmax"] - ref["value"]) <= 2e-5 * max(1.0, abs(ref["value"]))
    assert abs(met["loss"] - (met["categorical_crossentropy"] + 0.5 * met["lovasz_softmax"])) <= 2e-5
    assert "lovasz_loss" not in met and 0.0 < met["lovasz_softmax"] <= 1.0
    for k, v in m.get_gradients().items():
        assert np.isfinite(v).all(), k
    return met, ref


def test_fp32_step_logs_the_term_of_its_own_logits():
    n, size, classes = 2, 64, 3
    m = model(n=n)
    assert m.loss_w == (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5) and m.evaluated_terms == ("lovasz_softmax",)
    names = fwd_names(m)
    assert names[names.index("stp_softmax_loss_ex") + 1] == "stp_lovasz_softmax" and names.count("stp_lovasz_softmax") == 1
    m.set_weights(onets.init_unet_resnet("resnet18", classes=classes, seed=42))
    x, y = label_discs(n, size, classes, seed=5)
    check_step(m, x, y, classes)
    # the gradient of the class convolution moves with the term's weight: the launch adds to what the loss launch wrote
    g1 = m.get_gradients()["final_conv/kernel"]
    plain = model(n=n, loss="categorical_crossentropy")
    plain.set_weights(onets.init_unet_resnet("resnet18", classes=classes, seed=42))
    plain.train_on_batch(x, y)
    assert np.abs(g1 - plain.get_gradients()["final_conv/kernel"]).max() > 1e-6


@pytest.mark.parametrize("arch", ["FPN", "PSPNet"])
def test_fp32_step_on_resized_logits(arch):
    n, size, classes = 2, 96, 3
    m = model(arch, n=n, size=size)
    names = [name for _fn, _a, name, _m in m.plan.fwd + m.plan.bwd if name]
    assert "stp_resize_bilinear" in names and "stp_resize_bilinear_bwd" in names and names.count("stp_lovasz_softmax") == 1
    x, y = label_discs(n, size, classes, seed=6)
    check_step(m, x, y, classes)


def test_fp32_step_with_a_void_border():
    n, size, classes = 2, 64, 3
    m = model(n=n, ignore_label=255)
    names = fwd_names(m)
    assert names[names.index("stp_softmax_loss_masked") + 1] == "stp_lovasz_softmax"
    m.set_weights(onets.init_unet_resnet("resnet18", classes=classes, seed=42))
    x, y = label_discs(n, size, classes, seed=7)
    y[:, :3], y[:, -3:], y[:, :, :3], y[:, :, -3:] = 255, 255, 255, 255
    met, ref = check_step(m, x, y, classes, ignore_label=255)
    assert met["counted_pixels"] == float(ref["on"].sum()) == n * (size - 6) ** 2


def test_graph_replay_gives_the_eager_losses():
    n, size, classes = 2, 64, 3
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = label_discs(n, size, classes, seed=8)
    losses = []
    for use_graph in (False, True):
        m = model(n=n, dtype="bf16", use_graph=use_graph)
        m.set_weights(P)
        losses.append([m.train_on_batch(x, y)["loss"] for _ in range(5)])
    assert losses[0] == losses[1], losses


def test_bf16_the_term_alone_trains():
    n, size, classes = 2, 64, 3
    m = model(n=n, dtype="bf16", loss="lovasz_softmax", use_graph=True)
    assert list(m.plan._loss_weights) == [0.0] * 5
    m.set_weights(onets.init_unet_resnet("resnet18", classes=classes, seed=42))
    x, y = label_discs(n, size, classes, seed=9)
    losses = [m.train_on_batch(x, y)["loss"] for _ in range(12)]
    print(losses)
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]


@pytest.mark.parametrize("scale", ["static", "dynamic"])
def test_fp16_step_under_a_loss_scale(scale, monkeypatch):
    n, size, classes = 2, 64, 3
    if scale == "static":
        monkeypatch.setenv("STP_DYNAMIC_LOSS_SCALE", "0")
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = label_discs(n, size, classes, seed=10)
    m = model(n=n, dtype="fp16", loss_scale=4096.0 if scale == "static" else None, use_graph=True)
    names = fwd_names(m)
    i = names.index("stp_softmax_loss_ex")
    assert names[i + 1] == "stp_lovasz_softmax" and m.loss_scale == (4096.0 if scale == "static" else 16384.0)
    if scale == "dynamic":      # the dynamic multiplier scales what both launches wrote
        assert m.plan.dls is not None and names[i + 2] == "stp_scale_by_device"
    else:
        assert m.plan.dls is None and "stp_scale_by_device" not in names
    m.set_weights(P)
    met = m.train_on_batch(x, y)
    assert all(np.isfinite(v) for v in met.values()), met
    assert m.skipped_steps == 0
    for k, v in m.get_gradients().items():
        assert np.isfinite(v).all(), k
    ref = model(n=n, dtype="fp32")
    ref.set_weights(P)
    want = ref.train_on_batch(x, y)
    # 16-bit tolerance: the bars of the 16-bit steps of tests/test_softmax_losses_gpu.py (loss 1e-2, a term 5e-3)
    print(scale, met["loss"], want["loss"], met["lovasz_softmax"], want["lovasz_softmax"])
    assert abs(met["loss"] - want["loss"]) < 1e-2 and abs(met["lovasz_softmax"] - want["lovasz_softmax"]) < 5e-3
    # the scaled gradient, unscaled by the optimizer's factor, is the fp32 model's to 16-bit accuracy
    a, b = m.get_gradients()["final_conv/kernel"].ravel().astype(np.float64), ref.get_gradients()["final_conv/kernel"].ravel().astype(np.float64)
    assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30) > 0.99


@pytest.mark.parametrize("ignore_label", [None, 255])
def test_short_validation_batch_reruns_the_launch(ignore_label):
    """A padded batch of four re-run over its first two samples gives the scalars of a batch-2 model on those two samples
    (the form of tests/test_model_gpu.py::test_short_validation_batch_reruns_every_loss_family)."""
    size, classes = 64, 3
    x, y = label_discs(4, size, classes, seed=21)
    if ignore_label is not None:
        y[:, :4] = ignore_label
    x[2:], y[2:] = x[:2], y[:2]                      # the wrapped tail
    kw = {} if ignore_label is None else {"ignore_label": ignore_label}
    m4, m2 = model(n=4, **kw), model(n=2, **kw)
    m4.init_weights(seed=3)
    m2.set_weights(m4.get_weights())
    out = []
    for m, xs, ys, n_real in ((m4, x, y, 2), (m2, x[:2], y[:2], 2)):
        ep = m.eval_plan()
        assert [name for _f, _a, name, _m in ep.fwd].count("stp_lovasz_softmax") == 1
        ep.inputs["image"].buf.copy_(torch.from_numpy(xs).reshape(ep.inputs["image"].buf.shape))
        ep.inputs["mask"].buf.copy_(torch.from_numpy(ys).to(torch.uint8).reshape(ep.inputs["mask"].buf.shape))
        ep.run(ep.prep); ep.run(ep.fwd)
        if n_real < m.batch:
            full = ep.loss_scalars.cpu().numpy().copy()
            ep.rerun_loss(n_real)
        out.append(ep.loss_scalars.cpu().numpy().copy())
    np.testing.assert_allclose(out[0][:15], out[1][:15], rtol=2e-5, atol=2e-6)
    assert out[0][14] > 0 and abs(out[0][0] - (out[0][1] + 0.5 * out[0][14])) <= 2e-5
    assert np.isfinite(full).all()


YAML = """
backbone: resnet18
architecture: Unet
classes: 3
activation: softmax
encoder_weights:
shape: [64, 64, 3]
batch: 4
lr: 0.005
optimizer: Adam
loss: categorical_crossentropy+0.5*lovasz_softmax
metrics: [mean_iou]
primary_metric: val_lovasz_softmax
folds_count: 2
random_state: 7
dtype: fp32
draw_examples: false
stages:
  - epochs: 1
"""


def test_yaml_experiment_end_to_end(tmp_path):
    from segmentation_pipeline import segmentation
    cfgp = tmp_path / "lovasz.yaml"
    cfgp.write_text(YAML)
    cfg = segmentation.parse(str(cfgp))
    out = cfg.fit(LabelSet(8, seed=1), foldsToExecute=[0])
    assert len(out) == 1 and np.isfinite(out[0]["val_lovasz_softmax"])
    with open(cfg.metricsPath(0, 0)) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1
    for col in ("lovasz_softmax", "val_lovasz_softmax", "categorical_crossentropy", "val_categorical_crossentropy", "mean_iou", "val_mean_iou"):
        assert col in rows[0] and np.isfinite(float(rows[0][col])), col
    assert "lovasz_loss" not in rows[0] and "val_lovasz_loss" not in rows[0]
    assert 0.0 < float(rows[0]["lovasz_softmax"]) <= 1.0 and 0.0 < float(rows[0]["val_lovasz_softmax"]) <= 1.0
    assert os.path.getsize(cfg.weightsPath(0, 0)) > 0          # the best-weights file, chosen on val_lovasz_softmax (the smallest)
