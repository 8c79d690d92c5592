"""lovasz_softmax on the multi-class softmax head, host side (no GPU): the float64 restatement of include/stp_hip.h against an independent
torch-autograd restatement of Berman et al.'s published formula, the properties of the rank weights, the loss grammar and its refusals,
the names the epoch log carries, the C-ABI signatures and the plan's launch records."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _lovasz_softmax_reference as R
from segmentation_training_pipeline_amd import _lib, backend, graph, nets, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ arithmetic
def berman(z, t, ignore_label=None):
    """Lovasz-Softmax as published (Berman, Triki, Blaschko, CVPR 2018, algorithm 1 with the Jaccard increments of their lovasz_grad;
    per_image=False, classes='present'), on float64 torch tensors with autograd -> (value, d value / d z)."""
    z = torch.from_numpy(np.asarray(z, np.float64)).requires_grad_(True)
    labels = torch.from_numpy(np.asarray(t).astype(np.int64))
    probas = torch.softmax(z, dim=1)
    if ignore_label is not None:
        keep = labels != ignore_label
        probas, labels = probas[keep], labels[keep]
    losses = []
    for c in range(z.shape[1]):
        fg = (labels == c).to(torch.float64)
        if fg.numel() == 0 or fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        fg_sorted = fg[perm]
        gts = fg_sorted.sum()
        intersection = gts - fg_sorted.cumsum(0)
        union = gts + (1.0 - fg_sorted).cumsum(0)
        jaccard = 1.0 - intersection / union
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
        losses.append(torch.dot(errors_sorted, jaccard.detach()))
    if not losses:
        return 0.0, np.zeros(tuple(z.shape))
    value = torch.stack(losses).mean()
    value.backward()
    return float(value.detach()), z.grad.numpy()


def case(shape, classes, seed, absent=None, ignore=False):
    rng = np.random.RandomState(seed)
    pixels = int(np.prod(shape))
    z = rng.randn(pixels, classes) * 2.0
    t = rng.randint(0, classes, pixels).astype(np.uint8)
    if absent is not None:
        t[t == absent] = (absent + 1) % classes
    if ignore:
        t[rng.rand(pixels) < 0.25] = 255
    return z, t


@pytest.mark.parametrize("shape,classes", [((2, 12, 10), 3), ((1, 9, 7), 5)])
@pytest.mark.parametrize("ignore", [False, True])
def test_reference_equals_the_published_formula(shape, classes, ignore):
    z, t = case(shape, classes, seed=classes + 10 * ignore, absent=1, ignore=ignore)
    ign = 255 if ignore else None
    ref = R.reference(z, t, ign)
    value, grad = berman(z, t, ign)
    assert ref["present"] == classes - 1 and ref["positives"][1] == 0
    assert abs(ref["value"] - value) <= 1e-10, (ref["value"], value)
    assert np.abs(ref["dz"] - grad).max() <= 1e-10
    assert (ref["dz"][~ref["on"]] == 0).all()


def test_rank_weights_sum_to_one_and_bound_the_term():
    rng = np.random.RandomState(3)
    for n, k in ((1, 1), (7, 1), (7, 7), (100, 13), (4097, 500)):
        ys = np.zeros(n)
        ys[rng.permutation(n)[:k]] = 1.0
        g = R.rank_weights(ys)
        assert (g >= 0).all() and abs(g.sum() - 1.0) <= 1e-12
    for seed in range(4):
        z, t = case((1, 16, 16), 4, seed, ignore=bool(seed % 2))
        v = R.reference(z, t, 255 if seed % 2 else None)["value"]
        assert 0.0 <= v <= 1.0
    # a perfect one-hot prediction: every error is 0
    t = rng.randint(0, 3, 50).astype(np.uint8)
    z = np.where(np.eye(3)[t] > 0, 800.0, -800.0)
    ref = R.reference(z, t)
    assert ref["value"] == 0.0 and np.abs(ref["dz"]).max() == 0.0
    # nothing counted: the term and the gradient are 0, nothing is NaN
    ref = R.reference(rng.randn(20, 3), np.full(20, 255, np.uint8), 255)
    assert ref["value"] == 0.0 and ref["present"] == 0 and (ref["dz"] == 0).all()


def test_reference_tie_rule_is_the_stable_order():
    """All logits equal: every error is one of two values per class, the order inside a value is the pixel order."""
    t = np.array([0, 1, 2, 0, 1, 2, 2, 2], np.uint8)
    ref = R.reference(np.zeros((8, 3)), t)
    d = np.zeros((8, 3))
    value = 0.0
    for c in range(3):
        pos, neg = np.nonzero(t == c)[0], np.nonzero(t != c)[0]          # e = 2/3 for the positives, 1/3 for the negatives
        g = R.rank_weights(np.concatenate([np.ones(pos.size), np.zeros(neg.size)]))
        d[pos, c], d[neg, c] = -g[:pos.size] / 3.0, g[pos.size:] / 3.0
        value += ((2.0 / 3.0) * g[:pos.size].sum() + (1.0 / 3.0) * g[pos.size:].sum()) / 3.0
    assert abs(ref["value"] - value) <= 1e-15
    assert np.abs(ref["dz"] - (d - d.sum(axis=1, keepdims=True) / 3.0) / 3.0).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ grammar, names, ABI
def test_parse_loss_carries_the_weight():
    assert backend.parse_loss("categorical_crossentropy+0.5*lovasz_softmax", 3, "Unet", "softmax") == (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5)
    assert backend.parse_loss("lovasz_softmax", 20, "PSPNet", "softmax") == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    w = backend.parse_loss("categorical_crossentropy+dice_loss+0.3*iou_loss+0.2*jaccard_loss+2*focal_loss+0.25*lovasz_softmax", 4, "FPN", "softmax")
    assert w == (1.0, 1.0, 0.3, 0.2, 2.0, 0.0, 0.25) and backend.lovasz_softmax_weight(w) == 0.25
    assert backend.lovasz_softmax_weight((1.0, 1.0)) == 0.0 and backend.lovasz_softmax_weight((1.0, 0.0, 0.5, 0.0, 0.0, 0.0)) == 0.0
    # a zero weight names nothing: the spec returns what it returned
    assert backend.parse_loss("categorical_crossentropy+0*lovasz_softmax", 3, "Unet", "softmax") == (1.0, 0.0)


def test_parse_loss_refusals_say_what_to_use():
    with pytest.raises(ValueError, match="use lovasz_loss"):
        backend.parse_loss("binary_crossentropy+lovasz_softmax", 1)
    with pytest.raises(ValueError, match="use lovasz_loss"):
        backend.parse_loss("lovasz_softmax")
    with pytest.raises(ValueError, match="multi-label sigmoid head"):
        backend.parse_loss("binary_crossentropy+lovasz_softmax", 3, "Unet", "sigmoid")
    with pytest.raises(ValueError, match="DeepLabV3 .*use Unet, Linknet, FPN or PSPNet"):
        backend.parse_loss("categorical_crossentropy+lovasz_softmax", 3, "DeepLabV3", "softmax")
    # the models refuse before any device work
    with pytest.raises(ValueError, match="use lovasz_loss"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 1, "sigmoid", loss="lovasz_softmax", device="cpu")
    with pytest.raises(ValueError, match="multi-label sigmoid head"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 3, "sigmoid", loss="binary_crossentropy+lovasz_softmax", device="cpu")
    with pytest.raises(ValueError, match="lovasz_softmax is not available for DeepLabV3"):
        backend.HipSegModel("DeepLabV3", "mobilenetv2", (64, 64, 3), 3, "softmax", loss="categorical_crossentropy+lovasz_softmax", device="cpu")


def test_existing_specs_return_what_they_returned():
    parse_loss = backend.parse_loss
    assert parse_loss("binary_crossentropy+0.1*dice_loss") == (1.0, 0.1)
    assert parse_loss("dice_loss") == (0.0, 1.0)
    assert parse_loss("lovasz_loss") == (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
    assert parse_loss("binary_crossentropy+0.5*iou_loss") == (1.0, 0.0, 0.5, 0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        parse_loss("hinge_loss")
    with pytest.raises(ValueError):
        parse_loss("lovasz_loss", classes=3)
    with pytest.raises(ValueError, match="lovasz_loss is not available for a multi-label head"):
        parse_loss("categorical_crossentropy+lovasz_loss", 3, "Unet", "softmax")
    assert parse_loss("categorical_crossentropy+0.5*focal_loss+jaccard_loss", 4, "FPN", "softmax") == (1.0, 0.0, 0.0, 1.0, 0.5, 0.0)
    assert parse_loss("categorical_crossentropy+dice_loss", 4, "Unet", "softmax") == (1.0, 1.0)


def test_log_names_follow_the_spec():
    assert "lovasz_softmax" not in pipeline.epoch_log_names(3, True, "softmax")
    assert "lovasz_softmax" not in pipeline.epoch_log_names(3, False, "softmax")
    names = pipeline.epoch_log_names(3, True, "softmax", ("focal_loss",), False, ("lovasz_softmax",))
    assert "lovasz_softmax" in names and "lovasz_loss" not in names and "focal_loss" not in names
    assert sorted(set(names) - {"lovasz_softmax"}) == pipeline.epoch_log_names(3, True, "softmax", ("focal_loss",))
    scal = np.arange(16, dtype=np.float32)
    assert "lovasz_softmax" not in pipeline.derived_metrics(scal, 3, True, "softmax")
    d = pipeline.derived_metrics(scal, 3, True, "softmax", (), ("lovasz_softmax",))
    assert d["lovasz_softmax"] == 14.0 and d["jaccard_loss"] == 10.0 and "lovasz_loss" not in d

    class Named(object):
        loss_w, head_activation, classes = (1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5), "softmax", 3
        unevaluated_terms, evaluated_terms = ("focal_loss",), ("lovasz_softmax",)
    assert pipeline._logged(Named()) == ("lovasz_softmax",) and pipeline._logged(object()) == ()
    assert pipeline._extended(Named())
    # a loss without the word "loss": the best checkpoint is the smallest value
    assert pipeline.metric_mode("val_lovasz_softmax") == "min" and pipeline.metric_mode("val_mean_iou") == "max"


def test_ctypes_signatures_and_the_exported_chunk():
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
    assert _lib.SIGNATURES["stp_lovasz_softmax_workspace_bytes"] == (sz, [i64, i32])
    sig = _lib.SIGNATURES["stp_lovasz_softmax"]
    assert sig == (i32, [vp, vp, i64, i32, i32, i32, f32, vp, vp, i32, f32, i32, vp, sz, vp])
    # argument 2 is the pixel count, as for every name of Plan.LOSS_LAUNCHES: Plan.rerun_loss rewrites it the same way
    for name in graph.Plan.LOSS_LAUNCHES:
        assert _lib.SIGNATURES[name][1][2] is i64
    assert sig[1][2] is i64
    with open(os.path.join(ROOT, "include", "stp_hip.h")) as f:
        chunk = int(re.search(r"#define STP_LOVASZ_SOFTMAX_CHUNK (\d+)", f.read()).group(1))
    assert chunk == _lib.LOVASZ_SOFTMAX_CHUNK and chunk % 1024 == 0


# ------------------------------------------------------------------------------------------------ planning
class _HostSize(object):
    """The library with the sort-workspace query answered on the host (tests/_plan_dump.py wraps lovasz_loss's the same way: the
    library sizes the sort on a device; the launch records hold the number, nothing else depends on it)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def stp_lovasz_softmax_workspace_bytes(self, pixels, classes):
        return 24 * int(pixels) * int(classes) + 65536


def plan_for(net, loss, weight, training=True, dtype="bf16", dls=False, masked=None):
    p = graph.Plan(2, dtype, "cpu", training=training)
    p.lib = _HostSize(p.lib)
    if dtype == "fp16":
        p.loss_scale = 16384.0
    if dls:
        p.dls = torch.zeros(8, dtype=torch.float32)
    p.lovasz_softmax = weight
    p.masked_loss = masked
    p.define(lambda q_: net(q_, "resnet18", 96, 96, classes=4, loss=loss))
    return p


def names(pl):
    return [x[2] for x in pl.prep + pl.fwd + pl.bwd]


NETS = [nets.unet_resnet, nets.linknet_resnet, nets.fpn_resnet, nets.pspnet_resnet]


@pytest.mark.parametrize("net", NETS)
def test_the_launch_sits_behind_the_extended_loss_launch(net):
    loss = backend.parse_loss("categorical_crossentropy+0.5*lovasz_softmax", 4, "Unet", "softmax")
    assert loss[:5] == (1.0, 0.0, 0.0, 0.0, 0.0)
    p = plan_for(net, loss, backend.lovasz_softmax_weight(loss))
    n = [x[2] for x in p.fwd]
    assert n.count("stp_lovasz_softmax") == 1 and n.count("stp_softmax_loss_ex") == 1
    assert "stp_softmax_cce_dice" not in names(p) and "stp_softmax_cce_dice_up" not in names(p) and "stp_scale_by_device" not in names(p)
    i = n.index("stp_softmax_loss_ex")
    assert n[i + 1] == "stp_lovasz_softmax"
    first, a = p.fwd[i][1], p.fwd[i + 1][1]
    assert a[2] == 2 * 96 * 96 and a[3:5] == (4, 4) and a[6] == 0.5
    assert a[0] == first[0] and a[1] == first[1] and a[7] == first[7] and a[8] == first[8] and a[8] is not None      # logits, target, scalars, gradient
    assert a[9] == 8 and a[10] == 1.0 and a[11] == -1 and a[12] == p.ws_lovasz.data_ptr() and a[13] == p.ws_lovasz.numel()
    assert p.loss_scalars.numel() == 16 and list(p._loss_weights) == [1.0, 0.0, 0.0, 0.0, 0.0]
    if net in (nets.pspnet_resnet, nets.fpn_resnet):      # the extended branch: the logits are resized, the resize has its gradient launch
        assert "stp_resize_bilinear" in names(p) and "stp_resize_bilinear_bwd" in names(p) and "fused:resize->loss" not in names(p)
    # the term alone: the weights of the first launch are all zero
    alone = plan_for(net, backend.parse_loss("lovasz_softmax", 4, "Unet", "softmax"), 1.0)
    assert list(alone._loss_weights) == [0.0] * 5 and [x[2] for x in alone.fwd].count("stp_lovasz_softmax") == 1
    # an evaluation plan: the same launch without a gradient buffer
    e = plan_for(net, loss, 0.5, training=False)
    ea = [x for x in e.fwd if x[2] == "stp_lovasz_softmax"]
    assert len(ea) == 1 and ea[0][1][8] is None and ea[0][1][2] == 2 * 96 * 96
    # the same spec without the term: no such record, and the plan that was always built
    plain = plan_for(net, loss[:6], 0.0)
    assert "stp_lovasz_softmax" not in names(plain) and getattr(plain, "ws_lovasz", None) is None


@pytest.mark.parametrize("net", NETS)
def test_the_dynamic_loss_scale_covers_the_launch(net):
    loss = backend.parse_loss("categorical_crossentropy+0.5*lovasz_softmax", 4, "Unet", "softmax")
    p = plan_for(net, loss, 0.5, dtype="fp16", dls=True)
    n = [x[2] for x in p.fwd]
    i = n.index("stp_softmax_loss_ex")
    assert n[i + 1] == "stp_lovasz_softmax" and n[i + 2] == "stp_scale_by_device" and n.count("stp_scale_by_device") == 1
    assert p.fwd[i + 1][1][10] == 16384.0                       # the static loss scale goes in as grad_scale
    assert p.fwd[i + 2][1][0] == p.fwd[i + 1][1][8]             # and the device multiplier scales the gradient both launches wrote


def test_the_launch_honours_the_ignore_label():
    loss = backend.parse_loss("categorical_crossentropy+0.5*lovasz_softmax", 4, "Unet", "softmax")
    p = plan_for(nets.unet_resnet, loss, 0.5, masked={"ignore_label": 255, "class_weights": (1.0, 2.0, 3.0, 4.0)})
    n = [x[2] for x in p.fwd]
    i = n.index("stp_softmax_loss_masked")
    assert n[i + 1] == "stp_lovasz_softmax" and p.fwd[i + 1][1][11] == 255 and "stp_softmax_loss_ex" not in n


def test_plan_interface_stays():
    sig = inspect.signature(graph.Plan.softmax_loss)
    assert list(sig.parameters)[1:] == ["logits", "target", "w_cce", "w_dice", "w_iou", "w_jaccard", "w_focal"]
    assert graph.Plan(2, "bf16", "cpu").lovasz_softmax == 0.0
    assert "stp_lovasz_softmax" not in graph.Plan.LOSS_LAUNCHES          # it adds to what a loss launch wrote: rerun_loss runs it second
