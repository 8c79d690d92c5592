"""border_weights on the GPU, whole steps: one fp32 training step against the oracle whose cross-entropy is weighted with the reference
map (tests/_border_weight_reference.py; bars of tests/test_model_gpu.py::test_fp32_step_matches_oracle), the bf16 step under a captured
graph, a short last validation batch, a YAML experiment end to end and the inspection helper PipelineConfig.border_weight_map."""
import csv

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _border_weight_reference as R  # noqa: E402
from oracle import nets as onets  # noqa: E402
from oracle import step as ostep  # noqa: E402
from test_model_gpu import LOSS, make, rel_l2  # noqa: E402

KEY = {"w0": 10, "sigma": 3, "radius": 12}
BORDER = {"w0": 10.0, "sigma": 3.0, "radius": 12, "class_balance": (1.0, 1.0)}


def launch_names(plan):
    return [name for _fn, _a, name, _m in plan.prep + plan.fwd + plan.bwd if name]


@pytest.mark.parametrize("balance", [None, (0.5, 2.0)])
def test_fp32_step_matches_the_weighted_oracle(balance):
    """``balance`` None: the key as an experiment would write it.  (0.5, 2.0): class balances that move every pixel's weight, so that a
    step which ignored the map would miss the bars by far (with w0 alone the discs of this batch move the mean weight by 4e-4)."""
    KEY, BORDER = dict(globals()["KEY"]), dict(globals()["BORDER"])
    if balance is not None:
        KEY["class_balance"], BORDER["class_balance"] = list(balance), balance
    n, size = 2, 64
    x, y = ostep.synthetic_batch(n, size, size, seed=1234)
    L = np.stack([R.label(m[..., 0]) for m in y])
    frac = R.term_fraction(L, BORDER["radius"])
    print("background pixels with a border term: %.3f" % frac)
    assert frac >= 0.05
    P = onets.init_unet_resnet("resnet18", seed=42)
    tr = R.weighted_oracle(P, backbone="resnet18", loss=LOSS, optimizer="sgd", lr=0.05, opt_kwargs={"momentum": 0.9}, border=BORDER)
    m = make("resnet18", size, n, "fp32", optimizer="SGD", lr=0.05, opt_kwargs={"momentum": 0.9}, border_weights=KEY)
    assert m.border_weights == BORDER
    names = launch_names(m.plan)
    assert names.count("stp_mask_label") == n and names.count("stp_border_weight") == 1 and names.count("stp_sigmoid_bce_dice_weighted") == 1
    assert "stp_sigmoid_bce_dice" not in names and "stp_sigmoid_loss_bias_grad" not in names
    m.set_weights(P)
    o = tr.step(x.astype(np.float32), y.astype(np.float32))
    met = m.train_on_batch(x, y)
    # the map the step computed from its own target
    got = m.plan.border_map.cpu().numpy().astype(np.float64)
    assert np.abs(got - o["omega"]).max() <= 2e-6 * (10.0 + max(BORDER["class_balance"]))
    assert np.array_equal(m.plan.border_labels.cpu().numpy(), L)
    print("logits max err %.3g" % np.abs(m.logits() - o["logits"]).max(), "loss", met["loss"], o["loss"], "weighted bce", met["weighted_binary_crossentropy"],
          o["weighted_bce"], "bce", met["binary_crossentropy"], o["bce"], "mean weight", met["border_weight_mean"], o["weight_mean"])
    np.testing.assert_allclose(m.logits(), o["logits"], atol=1e-3)
    assert abs(met["dice_loss"] - o["dice_loss"]) < 1e-5
    flips = 2 * 2.0 / (2.0 * float(y.sum()) + 1.0)
    assert abs(met["dice"] - o["dice"]) < 1e-5 + flips
    assert abs(met["loss"] - o["loss"]) < 1e-5 * max(1.0, abs(o["loss"]))
    assert abs(met["weighted_binary_crossentropy"] - o["weighted_bce"]) < 1e-5 * max(1.0, abs(o["weighted_bce"]))
    assert abs(met["binary_crossentropy"] - o["bce"]) < 1e-5                      # the logged term stays unweighted
    assert o["weighted_bce"] > o["bce"] if balance is None else abs(o["weighted_bce"] - o["bce"]) > 0.05      # ... and is another number
    assert abs(met["border_weight_mean"] - o["weight_mean"]) < 1e-5 * o["weight_mean"]
    assert abs(met["binary_accuracy"] - o["binary_accuracy"]) < 1e-6 + 2.0 / y.size
    g = m.get_gradients()
    for k, ref in o["grads"].items():
        e = rel_l2(g[k], ref)
        assert e <= (1e-4 if k.startswith("final_conv") else 3e-2), "grad %s: rel L2 %.3g" % (k, e)
    w = m.get_weights()
    for k in tr.P:
        np.testing.assert_allclose(w[k], tr.P[k], atol=2e-4, err_msg=k)


def test_bf16_graph_steps_learn_and_repeat_bit_for_bit():
    n, size = 2, 64
    x, y = ostep.synthetic_batch(n, size, size, seed=1234)
    P = onets.init_unet_resnet("resnet18", seed=42)
    out = []
    for _ in range(2):
        m = make("resnet18", size, n, "bf16", use_graph=True, border_weights=KEY)
        m.set_weights(P)
        mets = [m.train_on_batch(x, y) for _ in range(30)]
        assert all(np.isfinite(v) for d in mets for v in d.values())
        assert mets[-1]["loss"] < mets[0]["loss"] and mets[-1]["weighted_binary_crossentropy"] < mets[0]["weighted_binary_crossentropy"]
        assert mets[0]["border_weight_mean"] == mets[-1]["border_weight_mean"] > 1.0          # the same target every step
        out.append((mets, m.get_weights()))
    assert out[0][0] == out[1][0]
    for k, v in out[0][1].items():
        assert np.array_equal(v, out[1][1][k]), k


@pytest.mark.parametrize("arch,size", [("FPN", 64), ("PSPNet", 96)])
def test_low_resolution_heads_and_fp16_train_under_the_key(arch, size):
    x, y = ostep.synthetic_batch(2, size, size, seed=7)
    m = make("resnet18", size, 2, "fp16", use_graph=True, architecture=arch, border_weights=True)
    fwd = [name for _fn, _a, name, _m in m.plan.fwd if name]
    assert m.plan.dls is not None and fwd[fwd.index("stp_sigmoid_bce_dice_weighted") + 1] == "stp_scale_by_device"
    mets = [m.train_on_batch(x, y) for _ in range(8)]
    assert all(np.isfinite(v) for d in mets for v in d.values())
    assert mets[-1]["loss"] < mets[0]["loss"]


def test_short_validation_batch_is_the_loss_of_the_real_samples():
    """Plan.rerun_loss knows the weighted launch: the scalars of the first two samples of a padded batch of four equal those of a batch-2
    model evaluating those two samples (the map of a sample does not depend on its neighbours in the batch)."""
    x, y = ostep.synthetic_batch(4, 64, 64, seed=23)
    assert R.term_fraction(np.stack([R.label(v[..., 0]) for v in y[:2]]), 12) >= 0.10
    x[2:], y[2:] = x[:2], y[:2]                      # the wrapped tail
    y[3] = 0                                         # ... whose content must not matter
    m4 = make("resnet18", 64, 4, "fp32", border_weights=KEY)
    m2 = make("resnet18", 64, 2, "fp32", border_weights=KEY)
    m4.init_weights(seed=3)
    m2.set_weights(m4.get_weights())
    out = []
    for m, xs, ys, n_real in ((m4, x, y, 2), (m2, x[:2], y[:2], 2)):
        ep = m.eval_plan()
        assert [k for k in launch_names(ep) if k.startswith("stp_sigmoid_bce")] == ["stp_sigmoid_bce_dice_weighted"]
        ep.inputs["image"].buf.copy_(torch.from_numpy(xs).reshape(ep.inputs["image"].buf.shape))
        ep.inputs["mask"].buf.copy_(torch.from_numpy(ys).to(torch.uint8).reshape(ep.inputs["mask"].buf.shape))
        ep.run(ep.prep); ep.run(ep.fwd)
        if n_real < m.batch:
            full = ep.loss_scalars.cpu().numpy().copy()
            ep.rerun_loss(n_real)
        out.append(ep.loss_scalars.cpu().numpy().copy())
    np.testing.assert_allclose(out[0], out[1], rtol=2e-5, atol=2e-6)
    assert out[0][15] > 1.005 and out[0][13] > out[0][1] and abs(full[15] - out[0][15]) > 1e-4      # the padded batch had another mean weight


YAML = """
backbone: resnet18
architecture: Unet
classes: 1
activation: sigmoid
encoder_weights:
shape: [64, 64, 3]
batch: 4
lr: 0.005
optimizer: Adam
loss: binary_crossentropy+dice_loss
border_weights: {w0: 10, sigma: 3, radius: 12}
primary_metric: val_weighted_binary_crossentropy
folds_count: 2
random_state: 7
dtype: bf16
draw_examples: false
stages:
  - epochs: 2
"""


class DiscSet(object):
    """Ad-hoc dataset: the oracle's synthetic discs, H x W x 1 masks of 0 / 255."""

    def __init__(self, n, size=64, seed=0):
        self.x, y = ostep.synthetic_batch(n, size, size, seed=seed)
        self.y = y * 255

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        from segmentation_pipeline.impl.datasets import PredictionItem
        return PredictionItem("disc%03d.png" % i, self.x[i], self.y[i])


def test_yaml_experiment_logs_and_selects_on_the_weighted_term(tmp_path):
    from segmentation_pipeline import segmentation
    from segmentation_training_pipeline_amd import pipeline
    cfgp = tmp_path / "border.yaml"
    cfgp.write_text(YAML)
    cfg = segmentation.parse(str(cfgp))
    assert pipeline.metric_mode(cfg.primary_metric, cfg.primary_metric_mode) == "min"
    out = cfg.fit(DiscSet(14, seed=1), foldsToExecute=[0])          # 7 validation samples: a short last batch
    assert len(out) == 1 and np.isfinite(out[0]["val_weighted_binary_crossentropy"])
    with open(cfg.metricsPath(0, 0)) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    for col in ("loss", "val_loss", "binary_crossentropy", "val_binary_crossentropy", "weighted_binary_crossentropy",
                "val_weighted_binary_crossentropy", "border_weight_mean", "val_border_weight_mean", "dice_loss"):
        assert all(col in r and np.isfinite(float(r[col])) for r in rows), col
    for r in rows:
        assert float(r["val_weighted_binary_crossentropy"]) >= float(r["val_binary_crossentropy"]) and float(r["val_border_weight_mean"]) >= 1.0
    # the checkpoint kept is the epoch with the smallest value of the primary metric
    vals = [float(r["val_weighted_binary_crossentropy"]) for r in rows]
    assert out[0]["best_epoch"] == int(np.argmin(vals)) and abs(out[0]["val_weighted_binary_crossentropy"] - min(vals)) <= 1e-4 * max(1.0, min(vals))


def test_border_weight_map_of_a_numpy_mask():
    from segmentation_pipeline.segmentation import PipelineConfig
    mask = R.blobs(48, 70, 3) * 255
    L = R.label(mask)
    got = PipelineConfig.border_weight_map(mask, w0=10, sigma=3, radius=12, class_balance=(0.5, 2.0))
    assert got.dtype == np.float32 and got.shape == (48, 70)
    want = R.weight_map(L, 10.0, 3.0, 12, 0.5, 2.0)
    assert np.abs(got - want).max() <= 2e-6 * 12.0 and R.term_fraction(L, 12) >= 0.10
    # the op's own map, bit for bit
    from test_border_weight_ops_gpu import run_border
    assert np.array_equal(got, run_border(L[None], 10.0, 3.0, 12, 0.5, 2.0)[0][0])
    # the default radius is ceil(4 sigma)
    assert np.array_equal(PipelineConfig.border_weight_map(mask, sigma=3), PipelineConfig.border_weight_map(mask, sigma=3, radius=12))
    # an instance label image: touching instances with different labels get a border between them, the binary mask sees one object
    inst = np.zeros((20, 40), np.int64)
    inst[5:15, 5:20], inst[5:15, 21:35] = 4, 9
    inst[5:15, 20] = 0                                         # a one-pixel gap
    inst[12:15, 20] = 9                                        # ... closed at the bottom: one component, two instances
    lab = PipelineConfig.border_weight_map(inst, sigma=2, radius=8, labelled=True)
    binary = PipelineConfig.border_weight_map(inst, sigma=2, radius=8)
    assert np.array_equal(lab, run_border(inst[None].astype(np.int32), 10.0, 2.0, 8)[0][0])
    assert (binary == 1.0).all() and lab[8, 20] > 1.0 + 10.0 * np.exp(-4.0 / 8.0) - 1e-4 and (lab[inst > 0] == 1.0).all()
    with pytest.raises(ValueError):
        PipelineConfig.border_weight_map(inst, sigma=9)       # the default radius 36 exceeds 32: name one
    with pytest.raises(ValueError):
        PipelineConfig.border_weight_map(inst - 1, labelled=True)
