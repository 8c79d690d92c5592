"""border_weights on the one-class sigmoid head, host side (no GPU): the YAML key with its defaults and refusals, the keywords an
experiment passes on, the names the epoch log carries, the C-ABI signatures, the plan's launch records, and the arithmetic of
include/stp_hip.h restated twice in tests/_border_weight_reference.py - the window search and the separable algorithm agree exactly, and
both stay within the stated truncation bound of the untruncated scipy form."""
import inspect

import numpy as np
import pytest
import torch

import _border_weight_reference as R
from segmentation_training_pipeline_amd import _lib, backend, graph, models, nets, pipeline

KEY = {"w0": 10.0, "sigma": 5.0, "radius": 20, "class_balance": (1.0, 1.0)}

YAML = """
backbone: resnet18
architecture: Unet
classes: 1
activation: sigmoid
encoder_weights:
shape: [64, 64, 3]
batch: 4
loss: binary_crossentropy+dice_loss
dtype: bf16
stages:
  - epochs: 1
"""


# ------------------------------------------------------------------------------------------------ the key
def test_defaults_and_true():
    assert backend.check_border_weights(None) is None and backend.check_border_weights(False) is None
    assert backend.check_border_weights(True) == KEY
    assert backend.check_border_weights({}) == KEY
    assert backend.check_border_weights({"sigma": 3}) == {"w0": 10.0, "sigma": 3.0, "radius": 12, "class_balance": (1.0, 1.0)}
    assert backend.check_border_weights({"sigma": 2.6})["radius"] == 11                       # ceil(4 sigma)
    got = backend.check_border_weights({"w0": 0, "sigma": 20, "radius": 32, "class_balance": [0.5, 2]}, 1, "FPN", "sigmoid", False, "dice_loss")
    assert got == {"w0": 0.0, "sigma": 20.0, "radius": 32, "class_balance": (0.5, 2.0)}
    for arch in ("Unet", "Linknet", "FPN", "PSPNet"):
        assert backend.check_border_weights(True, 1, arch, "sigmoid", False, "binary_crossentropy+0.5*dice_loss") == KEY
    assert backend.border_weight_params() == KEY


@pytest.mark.parametrize("spec,match", [
    ({"sigma": 9}, "name a radius"),                                     # the default ceil(4 sigma) = 36 exceeds 32
    ({"radius": 0}, "radius must be an integer 1..32"),
    ({"radius": 33}, "radius must be an integer 1..32"),
    ({"radius": 2.5}, "radius must be an integer 1..32"),
    ({"radius": True}, "radius must be an integer 1..32"),
    ({"w0": -1}, "w0"), ({"w0": float("nan")}, "w0"), ({"w0": float("inf")}, "w0"), ({"w0": "ten"}, "w0"),
    ({"sigma": 0}, "sigma"), ({"sigma": -2}, "sigma"), ({"sigma": float("inf")}, "sigma"),
    ({"class_balance": [1.0]}, "class_balance"), ({"class_balance": [0, 1]}, "class_balance"), ({"class_balance": [1, float("nan")]}, "class_balance"),
    ({"class_balance": 2}, "class_balance"),
    ({"w_0": 10}, "unknown key"),
    ("yes", "`true` or a mapping"),
])
def test_bad_parameters_are_refused(spec, match):
    with pytest.raises(ValueError, match=match):
        backend.check_border_weights(spec)


def test_heads_and_losses_that_cannot_take_the_key():
    with pytest.raises(ValueError, match="multi-label sigmoid head"):
        backend.check_border_weights(True, 3, "Unet", "sigmoid", True, "binary_crossentropy")
    with pytest.raises(ValueError, match="softmax head"):
        backend.check_border_weights(True, 3, "Unet", "softmax", False, "categorical_crossentropy")
    with pytest.raises(ValueError, match="DeepLabV3 .*use Unet, Linknet, FPN or PSPNet"):
        backend.check_border_weights(True, 1, "DeepLabV3", "sigmoid", False, "binary_crossentropy")
    for spec in ("binary_crossentropy+0.5*iou_loss", "focal_loss", "binary_crossentropy+dice_loss+0*jaccard_loss", "binary_crossentropy+lovasz_loss"):
        with pytest.raises(ValueError, match="may name binary_crossentropy and dice_loss"):
            backend.check_border_weights(True, 1, "Unet", "sigmoid", False, spec)
    # the models refuse before any device work (the plan would need a GPU: a ValueError comes first)
    with pytest.raises(ValueError, match="multi-label sigmoid head"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 3, "sigmoid", border_weights=True, device="cpu")
    with pytest.raises(ValueError, match="softmax head"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 3, "softmax", loss="categorical_crossentropy", border_weights=True, device="cpu")
    with pytest.raises(ValueError, match="not available for DeepLabV3"):
        backend.HipSegModel("DeepLabV3", "mobilenetv2", (64, 64, 3), 1, "sigmoid", border_weights=True, device="cpu")
    with pytest.raises(ValueError, match="may name binary_crossentropy and dice_loss"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 1, "sigmoid", loss="binary_crossentropy+focal_loss", border_weights=True, device="cpu")
    with pytest.raises(ValueError, match="name a radius"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 1, "sigmoid", border_weights={"sigma": 10}, device="cpu")


# ------------------------------------------------------------------------------------------------ YAML -> compile()
class _Recorder(object):
    classes, activation = 1, "sigmoid"

    def compile(self, **kw):
        self.kw = kw


def compiled_keywords(tmp_path, extra):
    from segmentation_pipeline import segmentation
    p = tmp_path / "e.yaml"
    p.write_text(YAML + extra)
    cfg = segmentation.parse(str(p))
    rec = _Recorder()
    cfg.createNet = lambda: rec
    cfg._compiled(cfg.stages[0])
    return cfg, rec.kw


def test_the_yaml_key_reaches_compile(tmp_path):
    _, kw = compiled_keywords(tmp_path, "border_weights: {w0: 10, sigma: 5, radius: 20, class_balance: [1.0, 1.0]}\n")
    assert kw["border_weights"] == {"w0": 10, "sigma": 5, "radius": 20, "class_balance": [1.0, 1.0]}
    assert backend.check_border_weights(kw["border_weights"]) == KEY
    _, kw = compiled_keywords(tmp_path, "border_weights: true\n")
    assert kw["border_weights"] is True
    _, kw = compiled_keywords(tmp_path, "border_weights: {sigma: 3}\n")
    assert backend.check_border_weights(kw["border_weights"])["radius"] == 12


def test_an_experiment_without_the_key_passes_what_it_passed(tmp_path):
    cfg, kw = compiled_keywords(tmp_path, "")
    assert cfg.border_weights is None
    assert sorted(kw) == sorted(["optimizer", "loss", "lr", "batch", "dtype", "clipnorm", "clipvalue", "metrics", "device", "use_graph", "loss_scale"])
    _, kw = compiled_keywords(tmp_path, "border_weights: false\n")
    assert "border_weights" not in kw


def test_the_constructors_take_the_keyword():
    assert inspect.signature(models.SegModel.compile).parameters["border_weights"].default is None
    assert inspect.signature(backend.HipSegModel.__init__).parameters["border_weights"].default is None
    sig = inspect.signature(graph.Plan.sigmoid_loss)
    assert list(sig.parameters)[1:] == ["logits", "target", "w_bce", "w_dice", "w_iou", "w_jaccard", "w_focal", "w_lovasz"]
    assert graph.Plan(2, "bf16", "cpu").border_weights is None


def test_log_names_follow_the_key():
    plain = pipeline.epoch_log_names(1, False, "sigmoid")
    assert not set(backend.BORDER_WEIGHT_TERMS) & set(plain)
    names = pipeline.epoch_log_names(1, False, "sigmoid", (), False, backend.BORDER_WEIGHT_TERMS)
    assert sorted(set(names) - set(plain)) == ["border_weight_mean", "weighted_binary_crossentropy"] and set(plain) <= set(names)
    scal = np.arange(16, dtype=np.float32)
    d = pipeline.derived_metrics(scal, 1, False, "sigmoid", (), backend.BORDER_WEIGHT_TERMS)
    assert d["weighted_binary_crossentropy"] == 13.0 and d["border_weight_mean"] == 15.0 and d["binary_crossentropy"] == 1.0
    assert "weighted_binary_crossentropy" not in pipeline.derived_metrics(scal, 1, False, "sigmoid")
    assert pipeline.metric_mode("weighted_binary_crossentropy") == "min" and pipeline.metric_mode("val_weighted_binary_crossentropy") == "min"
    assert pipeline.metric_mode("val_dice") == "max" and pipeline.metric_mode("border_weight_mean") == "max"

    class Keyed(object):
        loss_w, head_activation, classes = (1.0, 1.0), "sigmoid", 1
        unevaluated_terms, evaluated_terms = (), backend.BORDER_WEIGHT_TERMS
    assert pipeline._logged(Keyed()) == backend.BORDER_WEIGHT_TERMS and not pipeline._extended(Keyed())


# ------------------------------------------------------------------------------------------------ ABI
def test_ctypes_signatures():
    vp, i32, f32, sz = _lib.vp, _lib.i32, _lib.f32, _lib.sz
    S = _lib.SIGNATURES
    # the sibling's list with one more pointer in front of the stream
    assert S["stp_sigmoid_bce_dice_weighted"] == (i32, S["stp_sigmoid_bce_dice"][1][:-1] + [vp, vp])
    assert S["stp_sigmoid_bce_dice_weighted"][1][2] is _lib.i64 and "stp_sigmoid_bce_dice_weighted" in graph.Plan.LOSS_LAUNCHES
    assert S["stp_border_weight"] == (i32, [vp, i32, i32, i32, f32, f32, i32, f32, f32, vp, vp, vp, vp, sz, vp])
    assert S["stp_border_weight_workspace_bytes"] == (sz, [i32, i32, i32])
    for storage in ("bf16", "fp16"):
        lib = _lib.load(storage)
        assert hasattr(lib, "stp_border_weight") and hasattr(lib, "stp_sigmoid_bce_dice_weighted")
        # the query is host arithmetic: 8 bytes per pixel, 0 for the sizes the entry refuses
        assert lib.stp_border_weight_workspace_bytes(2, 64, 64) == 2 * 64 * 64 * 8
        assert lib.stp_border_weight_workspace_bytes(1, 1, 1) == 16
        assert lib.stp_border_weight_workspace_bytes(0, 64, 64) == 0 and lib.stp_border_weight_workspace_bytes(1 << 15, 1 << 8, 1 << 8) == 0


# ------------------------------------------------------------------------------------------------ planning
def plan_for(net, border, training=True, dtype="bf16", dls=False, loss=(1.0, 1.0), size=96):
    p = graph.Plan(2, dtype, "cpu", training=training)
    if dtype == "fp16":
        p.loss_scale = 16384.0
    if dls:
        p.dls = torch.zeros(8, dtype=torch.float32)
    p.border_weights = border
    p.define(lambda q_: net(q_, "resnet18", size, size, classes=1, loss=loss))
    return p


def names(pl):
    return [x[2] for x in pl.prep + pl.fwd + pl.bwd]


NEW = ("stp_mask_label", "stp_border_weight", "stp_sigmoid_bce_dice_weighted")


@pytest.mark.parametrize("net", [nets.unet_resnet, nets.fpn_resnet, nets.linknet_resnet, nets.pspnet_resnet])
def test_the_launches_of_a_keyed_plan(net):
    key = dict(KEY, w0=7.0, sigma=3.0, radius=12, class_balance=(0.5, 2.0))
    p = plan_for(net, key)
    n = [x[2] for x in p.fwd]
    assert n.count("stp_mask_label") == 2 and n.count("stp_border_weight") == 1 and n.count("stp_sigmoid_bce_dice_weighted") == 1
    assert "stp_sigmoid_bce_dice" not in names(p) and "stp_sigmoid_loss_ex" not in names(p) and "stp_scale_by_device" not in names(p)
    assert "stp_sigmoid_loss_bias_grad" not in names(p)             # the weighted gradient pass leaves no per-workgroup sums
    i = n.index("stp_mask_label")
    assert n[i:i + 4] == ["stp_mask_label", "stp_mask_label", "stp_border_weight", "stp_sigmoid_bce_dice_weighted"]
    a0, a1, bw, ls = (p.fwd[i + k][1] for k in range(4))
    mask = p.inputs["mask"].buf
    # one call per sample into one [N][H][W] buffer, the 8-neighbourhood, one workspace and one count word
    assert a0[0] == mask.data_ptr() and a1[0] == mask.data_ptr() + 96 * 96 and a0[1:5] == (96, 96, 2, 0) == a1[1:5]
    assert a0[5] == p.border_labels.data_ptr() and a1[5] == a0[5] + 4 * 96 * 96 and a0[6:] == a1[6:]
    assert a0[8] >= _lib.load().stp_mask_label_workspace_bytes(96, 96) > 0
    assert bw[:9] == (p.border_labels.data_ptr(), 2, 96, 96, 7.0, 3.0, 12, 0.5, 2.0) and bw[9] == p.border_map.data_ptr()
    assert bw[10] is None and bw[11] is None and bw[13] >= 2 * 96 * 96 * 8
    assert p.border_labels.dtype == torch.int32 and p.border_map.dtype == torch.float32 and p.border_map.numel() == 2 * 96 * 96
    # the loss launch: the sibling's arguments, the map behind the workspace
    assert ls[2] == 2 * 96 * 96 and ls[4:6] == (1.0, 1.0) and ls[6] == p.loss_scalars.data_ptr() and ls[7] is not None
    assert ls[9] == 1.0 and ls[10] == p.ws_loss.data_ptr() and ls[12] == p.border_map.data_ptr() and len(ls) == 13
    assert p.loss_scalars.numel() == 16
    # an evaluation plan: the same launches, a NULL gradient
    e = plan_for(net, key, training=False)
    en = [x[2] for x in e.fwd]
    assert [k for k in en if k in NEW] == ["stp_mask_label", "stp_mask_label", "stp_border_weight", "stp_sigmoid_bce_dice_weighted"]
    assert e.fwd[en.index("stp_sigmoid_bce_dice_weighted")][1][7] is None and "stp_sigmoid_bce_dice" not in en
    # without the key: none of the new records, and the launch that was always there
    plain = plan_for(net, None)
    assert not set(NEW) & set(names(plain)) and names(plain).count("stp_sigmoid_bce_dice") == 1
    assert getattr(plain, "border_map", None) is None


@pytest.mark.parametrize("net", [nets.unet_resnet, nets.fpn_resnet])
def test_the_dynamic_loss_scale_follows_the_weighted_launch(net):
    p = plan_for(net, KEY, dtype="fp16", dls=True)
    n = [x[2] for x in p.fwd]
    i = n.index("stp_sigmoid_bce_dice_weighted")
    assert n[i + 1] == "stp_scale_by_device" and n.count("stp_scale_by_device") == 1
    assert p.fwd[i][1][9] == 16384.0 and p.fwd[i + 1][1][0] == p.fwd[i][1][7]


def test_the_plan_refuses_the_other_terms():
    with pytest.raises(graph.StpShapeError, match="binary_crossentropy only"):
        plan_for(nets.unet_resnet, KEY, loss=(1.0, 1.0, 0.5, 0.0, 0.0, 0.0))
    with pytest.raises(graph.StpShapeError, match="binary_crossentropy only"):
        plan_for(nets.unet_resnet, KEY, loss=(1.0, 0.0, 0.0, 0.0, 0.0, 0.5))


# ------------------------------------------------------------------------------------------------ arithmetic
CASES = [(24, 40, 1, 5), (33, 29, 2, 8), (40, 70, 3, 20), (48, 48, 5, 12)]


@pytest.mark.parametrize("h,w,seed,radius", CASES)
def test_the_separable_algorithm_is_the_window_search(h, w, seed, radius):
    L = R.label(R.blobs(h, w, seed))
    assert L.max() >= 2
    assert R.term_fraction(L, radius) >= 0.10            # an all-zero term cannot pass: the window search alone says so
    a, b = R.distances_window(L, radius), R.distances_separable(L, radius)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert (a[0][L > 0] == 0).all() and (a[1][a[0] < 0] == -1).all() and ((a[1] < 0) | (a[1] >= a[0])).all()


@pytest.mark.parametrize("h,w,seed,radius", CASES)
def test_the_window_truncates_the_scipy_form_within_the_bound(h, w, seed, radius):
    L = R.label(R.blobs(h, w, seed))
    assert R.term_fraction(L, radius) >= 0.10
    for sigma in (radius / 4.0, radius / 2.5):
        full = R.untruncated(L, 10.0, sigma, 0.5, 2.0)
        bound = R.truncation_bound(10.0, sigma, radius)
        for fn in (R.distances_window, R.distances_separable):
            got = R.weight_map(L, 10.0, sigma, radius, 0.5, 2.0, fn=fn)
            err = np.abs(got - full).max()
            print(h, w, radius, sigma, fn.__name__, "max |truncated - untruncated| %.3g, bound %.3g" % (err, bound))
            assert err < bound
            assert (got[L > 0] == 2.0).all() and (got[L == 0] >= 0.5).all() and got.max() > 0.5 + 10.0 * 1e-3


def test_ties_one_pixel_objects_and_touching_labels():
    salt = R.label(R.salt(30, 37, 7))
    assert salt.max() == 83
    a, b = R.distances_window(salt, 6), R.distances_separable(salt, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # any label image, not only a labeller's: touching pixels with different values are different objects, equal values one object
    rng = np.random.RandomState(3)
    L = (rng.randint(1, 5, (20, 31)) * (rng.rand(20, 31) < 0.4)).astype(np.int32)
    a, b = R.distances_window(L, 4), R.distances_separable(L, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    two = np.zeros((5, 8), np.int32)
    two[:, :4], two[:, 4:] = 7, 3                        # two touching objects, no background: no term anywhere
    d1, d2 = R.distances_window(two, 2)
    assert (d1 == 0).all() and d2[0, 3] == 1 and d2[0, 0] == -1
    assert (R.weight_map(two, 10.0, 2.0, 2, 1.0, 3.0) == 3.0).all()
    # a one-pixel gap between them carries the largest term: d1 = d2 = 1
    gap = np.zeros((5, 9), np.int32)
    gap[:, :4], gap[:, 5:] = 7, 3
    w = R.weight_map(gap, 10.0, 2.0, 2)
    assert np.allclose(w[:, 4], 1.0 + 10.0 * np.exp(-4.0 / 8.0)) and (np.delete(w, 4, axis=1) == 1.0).all()
    # the same label on both sides is one object
    gap[:, 5:] = 7
    assert (R.weight_map(gap, 10.0, 2.0, 2) == 1.0).all()


def test_the_weighted_loss_reference():
    rng = np.random.RandomState(0)
    z, t = rng.randn(500) * 3.0, (rng.rand(500) < 0.3).astype(np.uint8)
    z[:4] = (40.0, -40.0, 40.0, -40.0)                   # beyond the probability clip: no cross-entropy gradient
    pw = rng.uniform(0.5, 11.0, 500)
    s, g, p = R.weighted_loss(z, t, pw, 1.0, 0.5)
    s1, g1, _ = R.weighted_loss(z, t, np.ones(500), 1.0, 0.5)
    assert abs(s1[13] - s1[1]) < 1e-15 and s1[15] == 1.0 and np.array_equal(s[1:10], s1[1:10])      # the weights enter [0], [13], [15] only
    assert abs(s[0] - (s[13] + 0.5 * s[2])) < 1e-15 and abs(s[15] - pw.mean()) < 1e-12
    # the gradient is the derivative of [0]
    zt = torch.from_numpy(z.copy()).requires_grad_(True)
    pt = torch.sigmoid(zt)
    y = torch.from_numpy(t.astype(np.float64))
    pc = torch.clamp(pt, R.EPS, R.HI)
    zc = torch.log(pc / (1.0 - pc))
    ce = torch.clamp(zc, min=0) - zc * y + torch.log1p(torch.exp(-torch.abs(zc)))
    loss = (torch.from_numpy(pw) * ce).mean() + 0.5 * (1.0 - (2.0 * (pt * y).sum() + 1.0) / (y.sum() + pt.sum() + 1.0))
    loss.backward()
    assert abs(float(loss.detach()) - s[0]) < 1e-12 and np.abs(zt.grad.numpy() - g).max() < 1e-12
