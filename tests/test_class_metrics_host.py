"""categorical_accuracy, mean_iou and iou_class_k of the softmax heads, host side (no GPU): the C-ABI signatures of the confusion
kernel, where the plan puts its launch, the switch left off, the refusal on sigmoid heads, the log names, the metric values of a
hand-written matrix and the epoch aggregation."""
import ctypes as C

import numpy as np
import pytest

from segmentation_training_pipeline_amd import _lib, backend, graph, nets, pipeline


def test_class_confusion_ctypes_signatures():
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    S = _lib.SIGNATURES
    assert S["stp_class_confusion_workspace_bytes"] == (sz, [i32])
    assert S["stp_class_confusion"] == (i32, [vp, vp, i64, i32, i32, i32, vp, vp, sz, vp])
    assert S["stp_class_confusion_up_ok"] == (i32, [i32, i32, i32])
    assert S["stp_class_confusion_up"] == (i32, [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, sz, vp])
    # argument 2 is the pixel count, as in every loss launch (Plan.rerun_loss shortens it); the first six arguments are those of the
    # loss on the same rows
    assert S["stp_class_confusion"][1][:6] == S["stp_softmax_cce_dice"][1][:6]
    # the low-resolution form takes the geometry arguments of the low-resolution loss
    assert S["stp_class_confusion_up"][1][:9] == S["stp_softmax_cce_dice_up"][1][:9]
    lib = _lib.load()
    for name in ("stp_class_confusion_workspace_bytes", "stp_class_confusion", "stp_class_confusion_up_ok", "stp_class_confusion_up"):
        assert hasattr(lib, name) and hasattr(_lib.load("fp16"), name)


def test_workspace_query_and_up_ok_are_host_functions():
    lib = _lib.load()
    assert lib.stp_class_confusion_workspace_bytes(1) == 0 and lib.stp_class_confusion_workspace_bytes(33) == 0
    for c in (2, 3, 20, 32):
        n = lib.stp_class_confusion_workspace_bytes(c)
        assert n > 0 and n % (4 * c * c) == 0                       # whole int32 tables
    for f in (2, 4, 8, 16):
        assert lib.stp_class_confusion_up_ok(f, 3, _lib.BF16) == 1 and lib.stp_class_confusion_up_ok(f, 20, _lib.F32) == 1
    assert lib.stp_class_confusion_up_ok(3, 3, _lib.BF16) == 0 and lib.stp_class_confusion_up_ok(32, 3, _lib.BF16) == 0
    assert lib.stp_class_confusion_up_ok(8, 1, _lib.BF16) == 0 and lib.stp_class_confusion_up_ok(8, 33, _lib.BF16) == 0
    assert lib.stp_class_confusion_up_ok(8, 3, _lib.F16) == 0       # the other build's 16-bit code
    assert _lib.load("fp16").stp_class_confusion_up_ok(8, 3, _lib.F16) == 1


def plan_for(net, classes=4, training=True, dtype="bf16", size=96, loss=(1.0, 1.0), **kw):
    p = graph.Plan(2, dtype, "cpu", training=training, **kw)
    p.define(lambda q_: net(q_, "resnet18", size, size, classes=classes, loss=loss))
    return p


def names(pl, lst=None):
    return [x[2] for x in (pl.prep + pl.fwd + pl.bwd if lst is None else lst)]


@pytest.mark.parametrize("net", [nets.unet_resnet, nets.linknet_resnet])
@pytest.mark.parametrize("training", [True, False])
def test_full_resolution_heads_get_one_launch_behind_the_loss(net, training):
    p = plan_for(net, training=training, class_metrics=True)
    n = names(p, p.fwd)
    assert n.count("stp_class_confusion") == 1 and "stp_class_confusion_up" not in n
    assert n[n.index("stp_class_confusion") - 1] == "stp_softmax_cce_dice"
    loss = [x for x in p.fwd if x[2] == "stp_softmax_cce_dice"][0][1]
    a = [x for x in p.fwd if x[2] == "stp_class_confusion"][0][1]
    assert a[:6] == loss[:6]                                          # the same rows, target, pixel count, classes, stride, dtype
    assert a[2:5] == (2 * 96 * 96, 4, 4)
    assert p.class_counts.dtype.is_floating_point is False and p.class_counts.numel() == 16 and a[6] == p.class_counts.data_ptr()
    assert a[8] == p.lib.stp_class_confusion_workspace_bytes(4)
    # the extended spec: behind stp_softmax_loss_ex
    ext = backend.parse_loss("categorical_crossentropy+focal_loss", 4, "Unet", "softmax")
    n = names(plan_for(net, training=training, loss=ext, class_metrics=True))
    assert n[n.index("stp_class_confusion") - 1] == "stp_softmax_loss_ex"


@pytest.mark.parametrize("net,factor", [(nets.pspnet_resnet, 8), (nets.fpn_resnet, 4)])
def test_low_resolution_heads_keep_the_fused_loss_in_training(net, factor):
    p = plan_for(net, class_metrics=True)
    off = plan_for(net)
    n = names(p)
    assert n.count("stp_class_confusion_up") == 1 and "stp_class_confusion" not in n
    assert n.count("stp_softmax_cce_dice_up") == 1 and "fused:resize->loss" in n
    # the resize of the logits stays out of the step (PSPNet's pyramid levels keep theirs): exactly the switch-off plan's launches
    assert [n.count(k) for k in ("stp_resize_bilinear", "stp_resize_bilinear_bwd")] == [names(off).count(k) for k in ("stp_resize_bilinear", "stp_resize_bilinear_bwd")]
    lo = p.tensors["final_conv"]
    assert not any(x[2] == "stp_resize_bilinear" and x[1][0] == lo.buf.data_ptr() for x in p.fwd)
    fwd = names(p, p.fwd)
    assert fwd[fwd.index("stp_class_confusion_up") - 1] == "stp_softmax_cce_dice_up"
    loss = [x for x in p.fwd if x[2] == "stp_softmax_cce_dice_up"][0][1]
    a = [x for x in p.fwd if x[2] == "stp_class_confusion_up"][0][1]
    assert a[:9] == loss[:9] and a[5] == factor and a[2:5] == (2, 96 // factor, 96 // factor)
    # the fused loss launch is what it is without the switch (scalars aside: pointers differ, the values do not)
    loss_off = [x for x in off.fwd if x[2] == "stp_softmax_cce_dice_up"][0][1]
    assert loss[2:11] == loss_off[2:11] and loss[13:15] == loss_off[13:15]
    # evaluation plans have no resize to fuse: the full-resolution form behind the plain loss
    e = plan_for(net, training=False, class_metrics=True)
    n = names(e, e.fwd)
    assert n.count("stp_class_confusion") == 1 and "stp_class_confusion_up" not in n
    assert any(x[2] == "stp_resize_bilinear" and x[1][0] == e.tensors["final_conv"].buf.data_ptr() for x in e.fwd)
    assert n[n.index("stp_class_confusion") - 1] == "stp_softmax_cce_dice"


def test_deeplab_counts_on_its_probabilities():
    for training in (True, False):
        p = graph.Plan(2, "fp32", "cpu", training=training, class_metrics=True)
        p.define(lambda q_: nets.deeplab_mobilenetv2(q_, "mobilenetv2", 64, 64, 3, 3, (), (1.0, 1.0)))
        n = names(p, p.fwd)
        assert n.count("stp_class_confusion") == 1 and n[n.index("stp_class_confusion") - 1] == "stp_prob_cce_dice"
        a = [x for x in p.fwd if x[2] == "stp_class_confusion"][0][1]
        assert a[0] == p.tensors["logits"].buf.data_ptr() and a[2:5] == (2 * 64 * 64, 3, 3)


@pytest.mark.parametrize("net", [nets.unet_resnet, nets.linknet_resnet, nets.pspnet_resnet, nets.fpn_resnet])
@pytest.mark.parametrize("training", [True, False])
def test_switch_off_leaves_every_plan_as_it_was(net, training):
    base = plan_for(net, training=training)
    off = plan_for(net, training=training, class_metrics=False)
    assert names(off, off.prep) == names(base, base.prep) and names(off, off.fwd) == names(base, base.fwd) and names(off, off.bwd) == names(base, base.bwd)
    assert not any(x.startswith("stp_class_confusion") for x in names(off)) and off.class_counts is None and not off.class_metrics
    # on: nothing but the one launch is added
    on = plan_for(net, training=training, class_metrics=True)
    assert [x for x in names(on) if not x.startswith("stp_class_confusion")] == names(base)
    # the binary head ignores nothing silently: it has no multi-class loss, so no launch either way
    b = plan_for(net, classes=1, training=training)
    assert not any(x.startswith("stp_class_confusion") for x in names(b))


def test_sigmoid_heads_refuse_the_switch():
    with pytest.raises(ValueError, match="one-class sigmoid head"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 1, "sigmoid", device="cpu", class_metrics=True)
    with pytest.raises(ValueError, match="multi-label sigmoid head"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 3, "sigmoid", device="cpu", class_metrics=True)


def test_log_names_on_and_off():
    seven = sorted(["loss", "categorical_crossentropy", "dice_loss", "dice", "binary_accuracy", "iou", "iot"])
    assert pipeline.epoch_log_names(3, False, "softmax") == seven
    assert pipeline.epoch_log_names(3, False, "softmax", (), False) == seven
    on = pipeline.epoch_log_names(3, False, "softmax", (), True)
    assert on == sorted(seven + ["categorical_accuracy", "mean_iou", "iou_class_0", "iou_class_1", "iou_class_2"])
    assert backend.class_metric_names(2) == ["categorical_accuracy", "mean_iou", "iou_class_0", "iou_class_1"]
    for name in ("categorical_accuracy", "val_categorical_accuracy", "mean_iou", "val_mean_iou", "iou_class_0", "val_iou_class_19"):
        assert backend.is_class_metric(name) and pipeline.metric_mode(name) == "max"
    for name in ("iou", "val_iou", "binary_accuracy", "iou_class_", "iou_class_x", "val_loss", "top_k_categorical_accuracy"):
        assert not backend.is_class_metric(name)


class _Cfg(object):
    """What GenericTaskConfig._wants_class_metrics reads."""

    def __init__(self, metrics=(), primary="val_loss", callbacks=None):
        self.metrics, self.primary_metric, self.all = list(metrics), primary, {"callbacks": callbacks}

    _wants_class_metrics = pipeline.GenericTaskConfig._wants_class_metrics


class _Model(object):
    def __init__(self, classes, activation):
        self.classes, self.activation = classes, activation


def test_the_pipeline_turns_the_switch_on_only_when_a_name_asks_for_it():
    soft, sig, ml = _Model(3, "softmax"), _Model(1, "sigmoid"), _Model(3, "sigmoid")
    assert not _Cfg(["dice"], "val_loss")._wants_class_metrics(soft)
    assert _Cfg(["categorical_accuracy"])._wants_class_metrics(soft)
    assert _Cfg([], "val_categorical_accuracy")._wants_class_metrics(soft)
    assert _Cfg([], "mean_iou")._wants_class_metrics(soft)
    assert _Cfg([], "val_loss", {"EarlyStopping": {"monitor": "val_iou_class_2", "patience": 3}})._wants_class_metrics(soft)
    assert not _Cfg([], "val_loss", {"EarlyStopping": {"monitor": "val_iou", "patience": 3}})._wants_class_metrics(soft)
    # a sigmoid head never gets it: the name is then refused with the other unknown names, before the first epoch
    assert not _Cfg(["categorical_accuracy"], "val_mean_iou")._wants_class_metrics(sig)
    assert not _Cfg(["categorical_accuracy"], "val_mean_iou")._wants_class_metrics(ml)
    # a stage's own callbacks
    stage = pipeline.Stage({"callbacks": {"ReduceLROnPlateau": {"monitor": "val_mean_iou", "patience": 2}}}, None)
    assert _Cfg()._wants_class_metrics(soft, stage)


def test_metric_values_of_a_hand_written_matrix():
    #            predicted 0  1  2
    m = np.array([[5, 1, 0],         # target 0
                  [2, 3, 0],         # target 1
                  [0, 0, 0]])        # target 2: never a target, never predicted - its union is empty
    d = backend.confusion_metrics(m)
    assert d["categorical_accuracy"] == 8 / 11
    assert d["iou_class_0"] == 5 / (6 + 7 - 5) and d["iou_class_1"] == 3 / (5 + 4 - 3) and d["iou_class_2"] == 0.0
    assert d["mean_iou"] == (5 / 8 + 3 / 6) / 2                      # over the two classes with a non-empty union (tf.metrics.mean_iou)
    assert sorted(d) == sorted(backend.class_metric_names(3))
    # a class that is predicted but never a target has a union: it counts, with IoU 0
    m2 = np.array([[4, 0, 1], [0, 4, 0], [0, 0, 0]])
    d2 = backend.confusion_metrics(m2.reshape(-1))                  # (flat, as the kernel writes it)
    assert d2["iou_class_2"] == 0.0 and d2["mean_iou"] == (4 / 5 + 1.0 + 0.0) / 3 and d2["categorical_accuracy"] == 8 / 9
    z = backend.confusion_metrics(np.zeros((3, 3), np.int64))
    assert z["categorical_accuracy"] == 0.0 and z["mean_iou"] == 0.0
    # counts beyond 2^31 (an epoch of many batches) stay exact
    big = np.array([[3 << 40, 1], [0, 1 << 40]], np.int64)
    assert backend.confusion_metrics(big)["categorical_accuracy"] == float(4 << 40) / float((4 << 40) + 1)


def test_epoch_values_come_from_the_summed_matrix():
    m1 = np.array([[10, 0, 0], [0, 0, 0], [0, 0, 0]], np.int64)      # a batch of class 0 alone, all right
    m2 = np.array([[0, 2, 0], [1, 1, 0], [0, 2, 4]], np.int64)
    names7 = pipeline.epoch_log_names(3, False, "softmax")
    sums = {k: 3.0 * 6 for k in names7}
    sums[pipeline.CONFUSION_KEY] = (m1 + m2).reshape(-1)
    logs = pipeline.reduce_epoch_sums(sums, 6, 3, False, "softmax", (), True)
    want = backend.confusion_metrics(m1 + m2)
    for k, v in want.items():
        assert logs[k] == v, k
    assert all(logs[k] == 3.0 for k in names7)
    assert sorted(logs) == pipeline.epoch_log_names(3, False, "softmax", (), True)
    # not the mean of the two batches' values
    a, b = backend.confusion_metrics(m1), backend.confusion_metrics(m2)
    assert abs(logs["mean_iou"] - 0.5 * (a["mean_iou"] + b["mean_iou"])) > 0.05
    # a rank that saw nothing contributes zeros in the same layout; nobody saw anything: no logs
    assert pipeline.reduce_epoch_sums({}, 0, 3, False, "softmax", (), True) == {}
    # switch off: the call and its result are what they were
    off = pipeline.reduce_epoch_sums({k: 3.0 * 6 for k in names7}, 6, 3, False, "softmax")
    assert sorted(off) == names7
