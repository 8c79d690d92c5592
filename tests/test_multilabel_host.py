"""Multi-label sigmoid heads (``classes: C > 1`` with ``activation: sigmoid``), host side (no GPU): mask bit-packing,
the refusals, loss parsing and metric names by activation, the C-ABI signatures of the new entry points, and the
augmentation oracle carrying packed class bits through its mask resampling."""
import ctypes as C

import numpy as np
import pytest

from oracle import augment as oaug
from segmentation_training_pipeline_amd import _lib, backend, pipeline


class Item(object):
    def __init__(self, x, y, ident="a.png"):
        self.x, self.y, self.id = x, y, ident


def packed(it, classes):
    return pipeline.prepare_item(it, classes, False, 3, "sigmoid").y.numpy()


def test_prepare_item_packs_class_bits():
    rng = np.random.RandomState(0)
    for classes in (2, 3, 5, 8):
        y = (rng.rand(12, 9, classes) < 0.5).astype(np.uint8)
        out = packed(Item(np.zeros((12, 9, 3), np.uint8), y), classes)
        assert out.dtype == np.uint8 and out.shape == (12, 9)
        for c in range(classes):
            assert np.array_equal((out >> c) & 1, y[:, :, c]), c
        if classes < 8:
            assert (out >> classes == 0).all()
    # 0 / 255 masks (PNG maps) and overlapping classes
    y = np.zeros((4, 4, 3), np.uint8)
    y[0, 0] = (255, 255, 0)
    y[1, 1] = (0, 0, 255)
    y[2, 2] = (255, 255, 255)
    out = packed(Item(np.zeros((4, 4, 3), np.uint8), y), 3)
    assert out[0, 0] == 0b011 and out[1, 1] == 0b100 and out[2, 2] == 0b111 and out[3, 3] == 0
    # all eight classes at once: every bit of the byte
    out = packed(Item(np.zeros((2, 2, 3), np.uint8), np.ones((2, 2, 8), np.uint8) * 255), 8)
    assert (out == 255).all()


def test_prepare_item_keeps_one_class_and_softmax_labels():
    y = np.zeros((4, 4, 3), np.uint8)
    y[..., 2] = 1
    y[0, 0] = (1, 0, 0)
    it = Item(np.zeros((4, 4, 3), np.uint8), y)
    soft = pipeline.prepare_item(it, 3, False, 3).y.numpy()               # no activation: softmax, as before
    assert soft[0, 0] == 0 and soft[1, 1] == 2
    assert np.array_equal(pipeline.prepare_item(it, 3, False, 3, "softmax").y.numpy(), soft)
    one = pipeline.prepare_item(Item(np.zeros((4, 4, 3), np.uint8), np.full((4, 4, 1), 255, np.uint8)), 1, False, 3, "sigmoid").y.numpy()
    assert (one == 1).all()


def test_prepare_item_refuses_single_channel_mask_for_multilabel_head():
    it = Item(np.zeros((4, 4, 3), np.uint8), np.ones((4, 4, 1), np.uint8))
    with pytest.raises(ValueError, match="cannot say which classes overlap"):
        pipeline.prepare_item(it, 3, False, 3, "sigmoid")
    with pytest.raises(ValueError, match="2..8 classes"):
        pipeline.pack_multilabel(np.ones((4, 4, 9), np.uint8), 9)


def test_model_refusals():
    # (the checks run before any device work: no GPU needed)
    with pytest.raises(ValueError, match="2..8 classes, not 9"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 9, "sigmoid", device="cpu")
    with pytest.raises(ValueError, match="DeepLabV3 has no multi-label"):
        backend.HipSegModel("DeepLabV3", "mobilenetv2", (64, 64, 3), 3, "sigmoid", device="cpu")
    with pytest.raises(ValueError, match="lovasz_loss is not available for a multi-label head"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 3, "sigmoid", loss="binary_crossentropy+lovasz_loss", device="cpu")
    with pytest.raises(ValueError, match="1-class sigmoid heads"):
        backend.HipSegModel("Unet", "resnet18", (64, 64, 3), 40, "softmax", device="cpu")


def test_parse_loss_by_activation():
    assert backend.parse_loss("binary_crossentropy+dice_loss", 1) == (1.0, 1.0)
    assert backend.parse_loss("binary_crossentropy+dice_loss", 4, "Unet", "sigmoid") == (1.0, 1.0)
    assert backend.parse_loss("binary_crossentropy+0.5*focal_loss+jaccard_loss", 4, "FPN", "sigmoid") == (1.0, 0.0, 0.0, 1.0, 0.5, 0.0)
    assert backend.parse_loss("categorical_crossentropy+dice_loss", 4, "Unet", "softmax") == (1.0, 1.0)
    assert backend.parse_loss("categorical_crossentropy+dice_loss", 4) == (1.0, 1.0)        # (no activation: softmax, as before)
    with pytest.raises(ValueError):
        backend.parse_loss("categorical_crossentropy", 4, "Unet", "sigmoid")
    with pytest.raises(ValueError):
        backend.parse_loss("binary_crossentropy", 4, "Unet", "softmax")
    with pytest.raises(ValueError):
        backend.parse_loss("binary_crossentropy+focal_loss", 4, "Unet", "softmax")
    with pytest.raises(ValueError, match="lovasz_loss"):
        backend.parse_loss("binary_crossentropy+lovasz_loss", 3, "Unet", "sigmoid")
    assert backend.is_multilabel(3, "sigmoid") and not backend.is_multilabel(1, "sigmoid") and not backend.is_multilabel(3, "softmax")


def test_metric_names_follow_the_activation():
    soft = pipeline.epoch_log_names(3, False)
    assert "categorical_crossentropy" in soft and "binary_crossentropy" not in soft
    assert pipeline.epoch_log_names(3, False, "softmax") == soft
    ml = pipeline.epoch_log_names(3, False, "sigmoid")
    assert "binary_crossentropy" in ml and "categorical_crossentropy" not in ml
    assert ml == pipeline.epoch_log_names(1, False)
    mlx = pipeline.epoch_log_names(3, True, "sigmoid")
    assert {"iou_loss", "jaccard_loss", "focal_loss"} <= set(mlx) and "lovasz_loss" not in mlx
    assert "lovasz_loss" in pipeline.epoch_log_names(1, True)
    scal = np.arange(16, dtype=np.float32)
    d = pipeline.derived_metrics(scal, 4, True, "sigmoid")
    assert d["binary_crossentropy"] == 1.0 and d["jaccard_loss"] == 10.0 and d["focal_loss"] == 11.0


def test_new_entry_points_ctypes_signatures():
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
    assert _lib.SIGNATURES["stp_sigmoid_multilabel_loss"] == (i32, [vp, vp, i64, i32, i32, i32, vp, vp, vp, i32, f32, vp, sz, vp])
    assert _lib.SIGNATURES["stp_sigmoid_multilabel_bias_grad"] == (i32, [vp, i64, i32, vp, i32, vp])


def test_graph_routes_multilabel_heads_to_the_new_loss():
    from segmentation_training_pipeline_amd import graph
    assert "stp_sigmoid_multilabel_loss" in graph.Plan.LOSS_LAUNCHES
    assert hasattr(graph.Plan, "sigmoid_multilabel_loss")


@pytest.mark.parametrize("steps", [[("fliplr",)], [("flipud",), ("affine", 1.2, (0.05, -0.1), 17.0, 5.0)],
                                   [("crop", 3, 5, 30, 40), ("resize", 48, 64), ("fliplr",)],
                                   [("affine", 0.8, (0.0, 0.0), -30.0, 0.0)]])
def test_augmentation_oracle_keeps_packed_class_bits(steps):
    """Nearest-neighbour mask resampling with a constant-0 border: warping the packed byte equals packing the C warped
    class maps, for every one of the eight bits."""
    rng = np.random.RandomState(len(steps))
    n, h, w, classes = 2, 48, 64, 8
    y = (rng.rand(n, h, w, classes) < 0.5).astype(np.uint8)
    bits = np.zeros((n, h, w), np.uint8)
    for c in range(classes):
        bits |= (y[..., c] << c).astype(np.uint8)
    img = rng.randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    M = oaug.compose(h, w, steps, (40, 56))
    params = np.zeros((n, oaug.AUG_RECORD), np.float32)
    params[:, :6] = M[:2].reshape(-1)
    params[:, 9:12] = 1.0                                                   # identity point operations
    _, out = oaug.warp_u8(img, bits, params, (40, 56))
    for c in range(classes):
        _, oc = oaug.warp_u8(img, y[..., c].copy(), params, (40, 56))
        assert np.array_equal((out >> c) & 1, oc), c
    assert set(np.unique(out)) <= set(np.unique(bits)) | {0}
