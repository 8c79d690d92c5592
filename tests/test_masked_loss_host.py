"""ignore_label / class_weights of the softmax heads, host side (no GPU): the refusals, the label images prepare_item makes, the YAML keys'
way to compile(), the plan's routing to stp_softmax_loss_masked / stp_class_confusion_ignore, the ctypes signatures, and the float64
reference of tests/_masked_loss_reference.py held to oracle/losses.py where the two must agree."""
import numpy as np
import pytest
import torch

import _masked_loss_reference as R
from oracle import losses as olosses
from segmentation_training_pipeline_amd import _lib, backend, graph, nets, pipeline

YAML = """
backbone: resnet18
architecture: Unet
classes: 3
activation: softmax
encoder_weights:
shape: [64, 64, 3]
batch: 2
loss: categorical_crossentropy+dice_loss
metrics: [dice]
dtype: fp32
draw_examples: false
stages:
  - epochs: 1
"""


# ------------------------------------------------------------------------------------------ refusals
def model(classes=3, activation="softmax", arch="Unet", backbone="resnet18", **kw):
    return backend.HipSegModel(arch, backbone, (64, 64, 3), classes, activation, batch=2, device="cpu", **kw)


@pytest.mark.parametrize("kw", [{"ignore_label": 255}, {"class_weights": [1.0]}])
def test_sigmoid_heads_refuse_the_keys(kw):
    with pytest.raises(ValueError, match="one-class sigmoid head"):
        model(1, "sigmoid", **kw)
    with pytest.raises(ValueError, match="multi-label sigmoid head"):
        model(3, "sigmoid", **({"class_weights": [1.0, 1.0, 1.0]} if "class_weights" in kw else kw))


@pytest.mark.parametrize("kw", [{"ignore_label": 255}, {"class_weights": [1.0, 2.0, 3.0]}])
def test_deeplab_refuses_the_keys(kw):
    with pytest.raises(ValueError, match="DeepLabV3"):
        model(3, "softmax", "DeepLabV3", "mobilenetv2", **kw)


def test_bad_weights_and_labels_are_refused():
    for cw in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], []):
        with pytest.raises(ValueError, match="entries"):
            model(class_weights=cw)
    for cw in ([1.0, 0.0, 1.0], [1.0, -2.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0]):
        with pytest.raises(ValueError, match="finite and > 0"):
            model(class_weights=cw)
    with pytest.raises(ValueError, match="list of one float per class"):
        model(class_weights=2.0)
    for ign in (-1, 256, 1000, 2.5, "255", True):
        with pytest.raises(ValueError, match="ignore_label must be an integer 0..255"):
            model(ignore_label=ign)
    assert backend.check_masked_loss(None, None, 1, "Unet", "sigmoid") == (None, None)       # no key: nothing to refuse
    assert backend.check_masked_loss(np.uint8(255), (1, 2, 3), 3, "FPN", "softmax") == (255, (1.0, 2.0, 3.0))


# ------------------------------------------------------------------------------------------ prepare_item
class _Item(object):
    def __init__(self, y, x=None):
        self.id, self.y = "item", y
        self.x = np.zeros(y.shape[:2] + (3,), np.uint8) if x is None else x


def test_prepare_item_keeps_the_void_label_with_the_key_and_clamps_without_it():
    y = np.array([[0, 1, 2, 3], [7, 254, 255, 2]], np.uint8)[:, :, None]
    plain = pipeline.prepare_item(_Item(y), 3, False, activation="softmax").y.numpy()
    assert np.array_equal(plain, [[0, 1, 2, 2], [2, 2, 2, 2]])
    kept = pipeline.prepare_item(_Item(y), 3, False, activation="softmax", ignore_label=255).y.numpy()
    assert np.array_equal(kept, [[0, 1, 2, 2], [2, 2, 255, 2]]) and kept.dtype == np.uint8
    # an ignore label inside the class range is kept as it is too
    zero = pipeline.prepare_item(_Item(y), 3, False, activation="softmax", ignore_label=0).y.numpy()
    assert np.array_equal(zero, [[0, 1, 2, 2], [2, 2, 2, 2]])
    # a one-hot mask cannot carry a void label
    onehot = np.eye(3, dtype=np.uint8)[np.array([[0, 1], [2, 1]])]
    assert np.array_equal(pipeline.prepare_item(_Item(onehot), 3, False, activation="softmax").y.numpy(), [[0, 1], [2, 1]])
    with pytest.raises(ValueError, match="one-hot .* cannot carry a void label"):
        pipeline.prepare_item(_Item(onehot), 3, False, activation="softmax", ignore_label=255)


def test_feeder_and_prefetcher_hand_the_label_on():
    f = pipeline.DeviceFeeder("cpu", (4, 4), [], seed=1, classes=3, activation="softmax", ignore_label=255)
    assert f.ignore_label == 255 and pipeline.DeviceFeeder("cpu", (4, 4), [], seed=1, classes=3).ignore_label is None
    y = np.full((4, 4, 1), 255, np.uint8)
    ds = [_Item(y), _Item(y)]
    got = [b for b in pipeline.HostPrefetcher(ds, [0, 1], 2, 3, False, activation="softmax", ignore_label=255)]
    assert all((it.y.numpy() == 255).all() for it in got[0])
    got = [b for b in pipeline.HostPrefetcher(ds, [0, 1], 2, 3, False, activation="softmax")]
    assert all((it.y.numpy() == 2).all() for it in got[0])


# ------------------------------------------------------------------------------------------ YAML -> compile()
class _Recorder(object):
    classes, activation = 3, "softmax"

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


def test_yaml_keys_reach_compile(tmp_path):
    cfg, kw = compiled_keywords(tmp_path, "ignore_label: 255\nclass_weights: [0.5, 2.0, 1.0]\n")
    assert cfg.ignore_label == 255 and cfg.class_weights == [0.5, 2.0, 1.0]
    assert kw["ignore_label"] == 255 and kw["class_weights"] == [0.5, 2.0, 1.0]
    _, kw = compiled_keywords(tmp_path, "ignore_label: 0\n")
    assert kw["ignore_label"] == 0 and "class_weights" not in kw
    _, kw = compiled_keywords(tmp_path, "class_weights: [1, 1, 3]\n")
    assert kw["class_weights"] == [1, 1, 3] and "ignore_label" not in kw


def test_an_experiment_without_the_keys_passes_no_new_keyword(tmp_path):
    cfg, kw = compiled_keywords(tmp_path, "")
    assert cfg.ignore_label is None and cfg.class_weights is None
    assert "ignore_label" not in kw and "class_weights" not in kw and "class_metrics" not in kw
    assert sorted(kw) == sorted(["optimizer", "loss", "lr", "batch", "dtype", "clipnorm", "clipvalue", "metrics", "device", "use_graph", "loss_scale"])


def test_seg_model_compile_takes_the_keywords():
    import inspect
    from segmentation_training_pipeline_amd import models
    sig = inspect.signature(models.SegModel.compile).parameters
    assert sig["ignore_label"].default is None and sig["class_weights"].default is None
    sig = inspect.signature(backend.HipSegModel.__init__).parameters
    assert sig["ignore_label"].default is None and sig["class_weights"].default is None


# ------------------------------------------------------------------------------------------ signatures and the plan
def test_ctypes_signatures():
    vp, i32, i64, f32, sz = _lib.vp, _lib.i32, _lib.i64, _lib.f32, _lib.sz
    S = _lib.SIGNATURES
    # the sibling's arguments, then ignore_label and the device pointer of the class weights in front of the stream
    assert S["stp_softmax_loss_masked"] == (i32, S["stp_softmax_loss_ex"][1][:-1] + [i32, vp, vp])
    assert S["stp_class_confusion_ignore"] == (i32, S["stp_class_confusion"][1][:-1] + [i32, vp])
    for storage in ("bf16", "fp16"):
        lib = _lib.load(storage)
        assert hasattr(lib, "stp_softmax_loss_masked") and hasattr(lib, "stp_class_confusion_ignore")
    assert "stp_softmax_loss_masked" in graph.Plan.LOSS_LAUNCHES


def plan_for(net, classes=4, training=True, dtype="bf16", size=96, loss=(1.0, 1.0), masked=None, dls=False, **kw):
    p = graph.Plan(2, dtype, "cpu", training=training, **kw)
    p.masked_loss = masked
    if dls:
        p.loss_scale = 16384.0
        p.dls = torch.zeros(8, dtype=torch.float32)
    p.define(lambda q_: net(q_, "resnet18", size, size, classes=classes, loss=loss))
    return p


def names(pl, lst=None):
    return [x[2] for x in (pl.prep + pl.fwd + pl.bwd if lst is None else lst)]


BOTH = {"ignore_label": 255, "class_weights": [0.5, 1.0, 2.0, 4.0]}


@pytest.mark.parametrize("net", [nets.unet_resnet, nets.linknet_resnet, nets.fpn_resnet, nets.pspnet_resnet])
@pytest.mark.parametrize("training", [True, False])
def test_plan_routes_to_the_masked_launch(net, training):
    p = plan_for(net, training=training, masked=BOTH, class_metrics=True)
    n = names(p)
    assert n.count("stp_softmax_loss_masked") == 1 and n.count("stp_class_confusion_ignore") == 1
    for other in ("stp_softmax_cce_dice", "stp_softmax_cce_dice_up", "stp_softmax_loss_ex", "stp_class_confusion", "stp_class_confusion_up",
                  "fused:resize->loss"):
        assert other not in n, other
    fwd = names(p, p.fwd)
    assert fwd[fwd.index("stp_class_confusion_ignore") - 1] == "stp_softmax_loss_masked"
    if net in (nets.fpn_resnet, nets.pspnet_resnet):      # no low-resolution form: the resize of the logits and its gradient launch stay
        base = names(plan_for(net, training=training, loss=(1.0, 1.0, 0.5, 0.0, 0.0)))          # an extended spec
        assert [n.count(k) for k in ("stp_resize_bilinear", "stp_resize_bilinear_bwd")] == \
            [base.count(k) for k in ("stp_resize_bilinear", "stp_resize_bilinear_bwd")]
        assert "stp_resize_bilinear" in n and (not training or "stp_resize_bilinear_bwd" in n)
    a = [x for x in p.fwd if x[2] == "stp_softmax_loss_masked"][0][1]
    c = [x for x in p.fwd if x[2] == "stp_class_confusion_ignore"][0][1]
    assert a[2:5] == (2 * 96 * 96, 4, 4) and c[:6] == a[:6]
    assert a[-2] == 255 and a[-1] == p.class_weights.data_ptr() and c[-1] == 255
    assert p.class_weights.dtype == torch.float32 and p.class_weights.tolist() == [0.5, 1.0, 2.0, 4.0]
    assert p.loss_scalars.numel() == 16 and a[7] == p.loss_scalars.data_ptr()
    assert (a[8] is not None) == training                      # the gradient buffer


def test_either_key_alone():
    p = plan_for(nets.unet_resnet, masked={"ignore_label": 0, "class_weights": None}, class_metrics=True)
    a = [x for x in p.fwd if x[2] == "stp_softmax_loss_masked"][0][1]
    assert a[-2] == 0 and a[-1] is None and p.class_weights is None
    assert [x for x in p.fwd if x[2] == "stp_class_confusion_ignore"][0][1][-1] == 0
    p = plan_for(nets.unet_resnet, masked={"ignore_label": None, "class_weights": [1, 2, 3, 4]}, class_metrics=True)
    a = [x for x in p.fwd if x[2] == "stp_softmax_loss_masked"][0][1]
    assert a[-2] == -1 and a[-1] == p.class_weights.data_ptr()
    assert [x for x in p.fwd if x[2] == "stp_class_confusion_ignore"][0][1][-1] == -1
    with pytest.raises(graph.StpShapeError):
        plan_for(nets.unet_resnet, masked={"ignore_label": None, "class_weights": [1, 2, 3]})


def test_fp16_plan_keeps_the_loss_scale_launch_behind_the_masked_loss():
    p = plan_for(nets.unet_resnet, dtype="fp16", masked=BOTH, dls=True)
    fwd = names(p, p.fwd)
    assert fwd[fwd.index("stp_softmax_loss_masked") + 1] == "stp_scale_by_device"
    a = [x for x in p.fwd if x[2] == "stp_softmax_loss_masked"][0][1]
    assert a[10] == 16384.0                                     # grad_scale


@pytest.mark.parametrize("net", [nets.unet_resnet, nets.fpn_resnet, nets.pspnet_resnet])
@pytest.mark.parametrize("loss", [(1.0, 1.0), (1.0, 0.5, 0.25, 0.125, 0.0625)])
def test_without_the_keys_the_plan_is_what_it_was(net, loss):
    base = graph.Plan(2, "bf16", "cpu", training=True, class_metrics=True)
    base.define(lambda q_: net(q_, "resnet18", 96, 96, classes=4, loss=loss))
    off = plan_for(net, loss=loss, masked=None, class_metrics=True)
    assert names(off) == names(base) and off.class_weights is None
    assert "stp_softmax_loss_masked" not in names(off) and "stp_class_confusion_ignore" not in names(off)
    m = model(loss="categorical_crossentropy+dice_loss")
    assert m.plan.masked_loss is None and not m.masked and m.ignore_label is None and m.class_weights is None
    assert "stp_softmax_loss_masked" not in names(m.plan) and m.plan.loss_scalars.numel() == 12


def test_model_hands_the_keys_to_both_plans():
    m = model(loss="categorical_crossentropy+dice_loss", ignore_label=255, class_weights=[1.0, 2.0, 0.5], class_metrics=True)
    assert m.masked and m.ignore_label == 255 and m.class_weights == (1.0, 2.0, 0.5)
    for p in (m.plan, m.eval_plan()):
        a = [x for x in p.fwd if x[2] == "stp_softmax_loss_masked"][0][1]
        assert a[-2] == 255 and p.class_weights.tolist() == [1.0, 2.0, 0.5]
        assert names(p, p.fwd).count("stp_class_confusion_ignore") == 1
    # the log keeps its names
    assert pipeline.epoch_log_names(3, False, "softmax", (), True) == sorted(
        ["loss", "categorical_crossentropy", "dice_loss", "dice", "binary_accuracy", "iou", "iot"] + backend.class_metric_names(3))


# ------------------------------------------------------------------------------------------ the reference against the oracle
def _case(P, C, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(P, C) * 2.0, rng.randint(0, C, P).astype(np.uint8)


@pytest.mark.parametrize("C", [2, 3, 20])
def test_reference_is_the_oracle_on_the_counted_rows(C):
    z, t = _case(500, C, C)
    t[::3] = 255
    on = t != 255
    w5 = (1.0, 0.5, 0.3, 0.2, 2.0)
    sc, g, pd, v = R.reference(z, t, w5, 255, [1.0] * C)
    assert np.array_equal(v, on) and sc[12] == on.sum() == sc[13] == sc[6]
    p = torch.softmax(torch.from_numpy(z[on]), dim=-1)
    y = torch.from_numpy(np.eye(C)[t[on]])
    want = [float(f(y, p)) for f in (olosses.categorical_crossentropy, olosses.dice_loss, olosses.iou_loss, olosses.jaccard_loss, olosses.focal_loss)]
    for got, ref in zip((sc[1], sc[2], 1 - sc[8], sc[10], sc[11]), want):
        assert abs(got - ref) <= 1e-12 * max(1.0, abs(ref)), (got, ref)
    assert abs(sc[0] - sum(w * x for w, x in zip(w5, want))) <= 1e-12 * sc[0]
    assert (g[~on] == 0).all() and np.abs(g[on]).max() > 0
    # the gradient of the counted rows is the oracle's on those rows alone
    zz = torch.from_numpy(z[on]).requires_grad_(True)
    olosses_sum = sum(w * f(y, torch.softmax(zz, dim=-1)) for w, f in zip(w5, (olosses.categorical_crossentropy, olosses.dice_loss,
                                                                                olosses.iou_loss, olosses.jaccard_loss, olosses.focal_loss)))
    olosses_sum.backward()
    np.testing.assert_allclose(g[on], zz.grad.numpy(), rtol=1e-10, atol=1e-15)


def test_reference_weights_and_the_empty_batch():
    z, t = _case(200, 3, 1)
    w = [0.25, 1.0, 4.0]
    one = (1.0, 0, 0, 0, 0)
    sc, g, pd, v = R.reference(z, t, one, None, w)
    ce = -np.log(pd[np.arange(200), t])
    assert abs(sc[1] - (np.asarray(w)[t] * ce).sum() / 200) < 1e-12 and abs(sc[13] - np.asarray(w)[t].sum()) < 1e-12 and sc[12] == 200
    # class weights do not enter the region terms
    plain = R.reference(z, t, one, None, None)[0]
    assert np.array_equal(sc[2:10], plain[2:10])
    # a label past the classes counts as the last class (the clamp of the other kernels) unless it is the ignore label
    t2 = t.copy(); t2[:10] = 200
    t3 = t.copy(); t3[:10] = 2
    assert np.array_equal(R.reference(z, t2, one)[0], R.reference(z, t3, one)[0])
    assert R.reference(z, t2, one, 200)[0][12] == 190
    # nothing counted: zeros, the smooth-term values, no NaN
    sc, g, _, v = R.reference(z, np.full(200, 255, np.uint8), (1.0, 0.5, 0.3, 0.2, 2.0), 255, w)
    assert not v.any() and np.isfinite(sc).all() and (g == 0).all()
    assert sc[0] == 0 and sc[1] == 0 and sc[2] == 0 and sc[8] == 1 and sc[10] == 0 and sc[11] == 0 and sc[12] == 0 and sc[4] == 0


def test_reference_has_no_clip_edge_element_on_the_gpu_tests_seeds():
    """The GPU test exempts gradient elements whose probability lies within rounding of a 1e-7 clip bound, under a cap; with logits
    of scale 2 the float64 reference has none at the seeds that test uses."""
    import test_masked_loss_gpu as G
    for C, P, seed in G.reference_cases():
        z, t = G.make_case(P, C, C, seed)
        pd = torch.softmax(torch.from_numpy(z[:, :C].astype(np.float64)), dim=-1).numpy()
        assert int(G.edge_elements(pd).sum()) == 0, (C, P, seed)
