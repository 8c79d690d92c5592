"""CPU tests of the device prediction path's host side: the numpy restatements the GPU tests compare with (tests/_predict_reference.py)
agree with the host chain they restate, ``labelMap`` refuses what it cannot write before anything is loaded, and the new entry points
are bound."""
import inspect

import numpy as np
import pytest

import _predict_reference as R

SIZES = [((8, 8), (8, 8)), ((8, 8), (1, 1)), ((8, 8), (5, 13)), ((6, 10), (19, 7)), ((6, 10), (16, 16)), ((64, 64), (50, 70)),
         ((64, 64), (64, 64)), ((64, 64), (100, 90))]


def config(**kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "batch": 4}
    return segmentation.PipelineConfig(**dict(base, **kw))


@pytest.mark.parametrize("src,dst", SIZES)
def test_gather_restates_scale_back(src, dst):
    from segmentation_pipeline.segmentation import PipelineConfig
    p = np.random.RandomState(1).uniform(0, 1, size=src + (3,)).astype(np.float32)
    assert np.array_equal(R.gather(p, *dst), PipelineConfig._scale_back(p, *dst))
    if src == dst:
        assert np.array_equal(R.gather(p, *dst), p)


def test_finish_restates_the_host_chain():
    """mean, then _scale_back, then the bytes of predict_to_directory / numpy's argmax - in the host's order of operations."""
    from segmentation_pipeline.segmentation import PipelineConfig
    rng = np.random.RandomState(2)
    maps = [rng.uniform(0, 1, size=(6, 10, 3)).astype(np.float32) for _ in range(6)]
    acc = np.zeros((6, 10, 3), np.float32)
    for m in maps:
        acc += m
    host = PipelineConfig._scale_back(acc / 6, 19, 7)
    assert np.array_equal(R.finish(acc, 6, 0, 19, 7), host)
    assert np.array_equal(R.finish(acc, 6, 1, 19, 7), (host * 255).astype(np.uint8))
    assert np.array_equal(R.finish(acc, 6, 2, 19, 7), np.argmax(host, axis=2))
    one = acc[:, :, :1]
    assert np.array_equal(R.finish(one, 6, 2, 19, 7), PipelineConfig._scale_back(one / 6, 19, 7)[:, :, 0] > 0.5)


def test_flips_restate_the_host_loop():
    x = np.arange(2 * 3 * 4 * 2).reshape(2, 3, 4, 2)
    assert np.array_equal(R.flip(x, 0), x) and np.array_equal(R.flip(x, 1), x[:, :, ::-1]) and np.array_equal(R.flip(x, 2), x[:, ::-1])
    for f in R.FLIPS:
        assert np.array_equal(R.flip(R.flip(x, f), f), x)          # the un-flip of a map is the same flip


@pytest.mark.parametrize("size", [(100, 90), (50, 70), (7, 5), (64, 64)])
@pytest.mark.parametrize("crops", [2, 3])
def test_cell_rectangles_restate_crop_bounds(size, crops):
    from segmentation_training_pipeline_amd.pipeline import crop_bounds
    h, w = size
    ys, xs = crop_bounds(h, crops), crop_bounds(w, crops)
    want = [(ys[r], ys[r + 1], xs[q], xs[q + 1]) for r in range(crops) for q in range(crops)]
    assert R.cell_rectangles(h, w, crops) == want
    cover = np.zeros((h, w), np.int32)
    for y0, y1, x0, x1 in want:
        cover[y0:y1, x0:x1] += 1
    assert (cover == 1).all()                                       # the cells tile the image: every pixel of the map is written once


def test_label_map_refusals(tmp_path):
    """A multi-label head has no single label per pixel, and a label map is a PNG: both are refused before a model is loaded or a
    directory is made."""
    target = tmp_path / "out"
    multilabel = config(classes=3, activation="sigmoid")
    with pytest.raises(ValueError, match="labelMap"):
        multilabel.predict_to_directory(str(tmp_path), str(target), labelMap=True)
    for cfg in (config(), config(classes=3, activation="softmax")):
        with pytest.raises(ValueError, match="labelMap"):
            cfg.predict_to_directory(str(tmp_path), str(target), labelMap=True, binaryArray=True)
    assert not target.exists()
    from segmentation_pipeline.segmentation import PipelineConfig
    sig = inspect.signature(PipelineConfig.predict_to_directory)
    assert sig.parameters["labelMap"].default is False
    assert list(sig.parameters)[:9] == ["self", "spath", "tpath", "fold", "stage", "limit", "batchSize", "binaryArray", "ttflips"]


def test_entry_points_are_bound():
    from segmentation_pipeline.segmentation import PipelineConfig
    from segmentation_training_pipeline_amd import _lib, backend, ops
    i32, vp = _lib.i32, _lib.vp
    assert _lib.SIGNATURES["stp_flip_u8"] == (i32, [vp, vp, i32, i32, i32, i32, i32, vp])
    assert _lib.SIGNATURES["stp_predict_accumulate"] == (i32, [vp, vp, i32, i32, i32, i32, i32, vp])
    assert _lib.SIGNATURES["stp_predict_finish"] == (i32, [vp, i32, i32, i32, i32, i32, vp, i32, i32, i32, vp])
    for name in ("flip_u8", "predict_accumulate", "predict_finish"):
        assert callable(getattr(ops, name))
    assert list(inspect.signature(backend.HipSegModel.predict_device).parameters) == ["self", "x_dev", "n", "flip"]
    assert list(inspect.signature(PipelineConfig.predict_on_batch_device).parameters) == ["self", "models", "ttflips", "xs_dev", "n"]
    assert list(inspect.signature(PipelineConfig.predict_on_batch).parameters) == ["self", "models", "ttflips", "xs"]


def test_wrappers_have_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    with pytest.raises(_lib.StpError):
        ops.flip_u8(torch.zeros(48, dtype=torch.uint8), torch.zeros(48, dtype=torch.uint8), 1, 4, 4, 3, 1)
    with pytest.raises(_lib.StpError):
        ops.predict_accumulate(torch.zeros(48), torch.zeros(48), 1, 4, 4, 3, 1)
    with pytest.raises(_lib.StpError):
        ops.predict_finish(torch.zeros(48), 4, 4, 3, 1, 0, torch.zeros(48), 4, 4)
