"""CPU tests of the device mask path's host side (segmentation_pipeline/segmentation.py over csrc/mask.hip): the host statements the GPU
tests compare with (tests/_mask_reference.py) agree with the reference's golden run-length vectors, with ``impl.rle.rle_encode`` and with
scipy; every refusal of ``predict_masks`` / ``predict_to_csv`` / ``find_threshold`` fires before a model file is opened; the new entry
points are bound and their wrappers have no CPU fallback."""
import inspect
import json
import os

import numpy as np
import pytest

import _mask_reference as R


def config(**kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "batch": 4}
    return segmentation.PipelineConfig(**dict(base, **kw))


def test_rle_runs_format_to_the_golden_vectors(golden_dir):
    with open(os.path.join(golden_dir, "rle_golden.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) >= 3
    for c in cases:
        mask = np.asarray(c["mask"], np.uint8)
        runs = R.rle_runs(mask)
        assert runs.dtype == np.int32 and runs.shape == (len(c["rle"].split()) // 2, 2)
        assert R.format_runs(runs) == c["rle"] == R.rle_encode(mask)


def test_rle_runs_follow_the_flat_column_major_array():
    m = np.zeros((4, 3), np.uint8)
    m[2:, 0] = 1
    m[:2, 1] = 1                                    # bottom of column 0 goes on at the top of column 1: ONE run
    assert R.rle_runs(m).tolist() == [[3, 4]] and R.column_crossings(m) == 1
    assert R.format_runs(R.rle_runs(np.zeros((5, 4), np.uint8))) == "" == R.rle_encode(np.zeros((5, 4)))
    assert R.rle_runs(np.ones((5, 4), np.uint8)).tolist() == [[1, 20]]
    rng = np.random.RandomState(3)
    for shape in ((1, 1), (7, 5), (64, 3), (65, 2)):
        m = (rng.uniform(size=shape) > 0.5).astype(np.uint8)
        assert R.format_runs(R.rle_runs(m)) == R.rle_encode(m)


def test_disk_and_scipy_defaults():
    d2 = R.disk(2)
    assert d2.shape == (5, 5) and int(d2.sum()) == 13
    assert d2.tolist() == [[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [1, 1, 1, 1, 1], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]]
    assert [int(R.disk(r).sum()) for r in (1, 3, 7)] == [5, 29, 149]
    ones = np.ones((9, 11), np.uint8)
    assert int(R.opening(ones, 2).sum()) == 87 and int(R.closing(ones, 2).sum()) == 35      # scipy's closing clears the border band
    m = (np.random.RandomState(4).uniform(size=(20, 30)) > 0.3).astype(np.uint8)
    for r in (1, 2, 3):
        assert np.array_equal(R.opening(m, r), R.dilate(R.erode(m, r), r))
        assert np.array_equal(R.closing(m, r), R.erode(R.dilate(m, r), r))


def test_threshold_mask_and_counts_restate_numpy():
    rng = np.random.RandomState(5)
    arr = rng.uniform(size=(6, 7, 3)).astype(np.float32)
    arr[0, 0, 2] = np.nan
    arr[1, 1] = 0.5                                  # an exact three-way tie: the first index wins
    arr[2, 2, 1:] = arr[2, 2].max() + 1              # a two-way tie of channels 1 and 2
    assert np.array_equal(R.threshold_mask(arr, 2, 0, 0.25), arr[:, :, 2] > 0.25) and R.threshold_mask(arr, 2, 0, 0.25)[0, 0] == 0
    labels = R.threshold_mask(arr, 1, 1)
    ok = ~np.isnan(arr).any(axis=2)
    assert np.array_equal(labels[ok], (np.argmax(arr, axis=2) == 1)[ok]) and labels[1, 1] == 0 and labels[2, 2] == 1
    assert R.threshold_mask(arr, 0, 1)[1, 1] == 1
    target = rng.uniform(size=(6, 7)) > 0.5
    thr = [0.1, 0.5, 0.9]
    counts, totals = R.threshold_counts(arr, target, thr, channel=0)
    for t, v in enumerate(thr):
        m = arr[:, :, 0] > v
        assert counts[t].tolist() == [int(m.sum()), int((m & target).sum())]
    assert totals.tolist() == [int(target.sum()), 42] and counts.dtype == np.int64


def test_score_on_hand_made_counters():
    from segmentation_pipeline.segmentation import PipelineConfig
    for score in (R.score, PipelineConfig.sweep_score):
        assert float(score("dice", 6, 3, 4)) == 2 * 3 / 10
        assert float(score("iou", 6, 3, 4)) == 3 / 7
        assert float(score("f2", 6, 3, 4)) == 15 / 22
        for metric in R.METRICS:
            assert float(score(metric, 0, 0, 0)) == 1.0          # nothing predicted, nothing there
            assert float(score(metric, 5, 0, 0)) == 0.0
            assert float(score(metric, 0, 0, 5)) == 0.0
            assert float(score(metric, 5, 5, 5)) == 1.0
        got = score("dice", np.array([[6, 0], [0, 2]]), np.array([[3, 0], [0, 2]]), np.array([[4], [2]]))
        assert got.dtype == np.float64 and got.tolist() == [[0.6, 0.0], [0.0, 1.0]]
    per_image = [(np.array([[6, 3], [0, 0]]), np.array([4, 100])), (np.array([[0, 0], [0, 0]]), np.array([0, 100]))]
    assert R.sweep_table(per_image, "dice", "image").tolist() == [(0.6 + 1.0) / 2, (0.0 + 1.0) / 2]
    assert R.sweep_table(per_image, "dice", "pixels").tolist() == [0.6, 0.0]


@pytest.fixture
def no_model_files(monkeypatch):
    """Any attempt to load a model fails the test: the refusals must come first."""
    from segmentation_pipeline.segmentation import PipelineConfig

    def load_model(self, fold=0, stage=-1):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(PipelineConfig, "load_model", load_model)


def test_predict_masks_refusals(tmp_path, no_model_files):
    softmax = config(classes=3, activation="softmax")
    with pytest.raises(ValueError, match="threshold"):
        softmax.predict_masks(str(tmp_path), threshold=0.25)           # (raised by the call, not by the first next())
    with pytest.raises(ValueError, match="threshold"):
        softmax.predict_to_csv(str(tmp_path), str(tmp_path / "out.csv"), threshold=0.3)
    assert not (tmp_path / "out.csv").exists()
    for kw in ({"channel": 1}, {"channel": -1}, {"opening": 8}, {"closing": -1}, {"opening": 1.5}):
        with pytest.raises(ValueError):
            config().predict_masks(str(tmp_path), **kw)
    with pytest.raises(ValueError):
        softmax.predict_masks(str(tmp_path), channel=3)
    with pytest.raises(ValueError):
        config().predict_to_csv(str(tmp_path), str(tmp_path / "out.csv"), columns=("image",))
    # what passes the checks is a generator that has not touched a model yet
    assert inspect.isgenerator(softmax.predict_masks(str(tmp_path), channel=2))
    assert inspect.isgenerator(config(classes=3).predict_masks(str(tmp_path), channel=2, threshold=0.25, opening=2, closing=7))


def test_find_threshold_refusals(no_model_files):
    ds = object()                                                      # never looked at: every refusal comes before the dataset is
    with pytest.raises(ValueError, match="softmax"):
        config(classes=3, activation="softmax").find_threshold(ds, 0)
    cfg = config()
    with pytest.raises(ValueError, match="metric"):
        cfg.find_threshold(ds, 0, metric="accuracy")
    with pytest.raises(ValueError, match="average"):
        cfg.find_threshold(ds, 0, average="batch")
    for bad in ([0.5, 0.25], [0.25, 0.25], [0.5, 0.5 + 1e-12], [0.1, float("nan")], [0.1, float("inf")], []):
        with pytest.raises(ValueError, match="thresholds"):
            cfg.find_threshold(ds, 0, thresholds=bad)                 # (0.5 + 1e-12 is 0.5 as float32)
    with pytest.raises(ValueError, match="64"):
        cfg.find_threshold(ds, 0, thresholds=[i / 100 for i in range(65)])
    with pytest.raises(ValueError, match="channel"):
        cfg.find_threshold(ds, 0, channel=1)


def test_public_signatures():
    from segmentation_pipeline.segmentation import PipelineConfig
    p = inspect.signature(PipelineConfig.predict_masks).parameters
    assert list(p) == ["self", "spath", "fold", "stage", "limit", "ttflips", "threshold", "opening", "closing", "channel", "rle"]
    assert [p[k].default for k in list(p)[2:]] == [0, 0, -1, False, 0.5, 0, 0, 0, True]
    p = inspect.signature(PipelineConfig.predict_to_csv).parameters
    assert list(p)[:3] == ["self", "spath", "csv_path"] and p["columns"].default == ("image", "rle_mask")
    p = inspect.signature(PipelineConfig.find_threshold).parameters
    assert list(p) == ["self", "ds", "fold", "stage", "negatives", "ttflips", "thresholds", "metric", "average", "channel"]
    assert [p[k].default for k in list(p)[3:]] == [-1, "real", None, None, "dice", "image", 0]


def test_entry_points_are_bound():
    from segmentation_training_pipeline_amd import _lib, ops
    i32, i64, f32, vp, sz = _lib.i32, _lib.i64, _lib.f32, _lib.vp, _lib.sz
    assert _lib.SIGNATURES["stp_mask_threshold"] == (i32, [vp, i32, i32, i32, i32, i32, f32, vp, i32, vp])
    assert _lib.SIGNATURES["stp_mask_morph"] == (i32, [vp, vp, i32, i32, i32, i32, vp])
    assert _lib.SIGNATURES["stp_mask_rle_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_mask_rle"] == (i32, [vp, i32, i32, vp, vp, i64, vp, sz, vp])
    assert _lib.SIGNATURES["stp_threshold_counts_workspace_bytes"] == (sz, [i32])
    res, args = _lib.SIGNATURES["stp_threshold_counts"]
    assert res == i32 and args[:6] == [vp, vp, i32, i32, i32, i32] and args[7:] == [i32, vp, vp, vp, sz, vp]
    for name in ("mask_threshold", "mask_morph", "mask_rle", "threshold_counts"):
        assert callable(getattr(ops, name))
    for storage in ("bf16", "fp16"):                                   # both builds export the same code; the queries run without a GPU
        lib = _lib.load(storage)
        assert lib.stp_mask_rle_workspace_bytes(64, 64) == 64 * 8 + 16
        assert lib.stp_mask_rle_workspace_bytes(65, 300) == 600 * 8 + 3 * 16
        assert lib.stp_mask_rle_workspace_bytes(0, 5) == 0 and lib.stp_mask_rle_workspace_bytes(1 << 16, 1 << 15) == 0
        assert lib.stp_threshold_counts_workspace_bytes(19) == 256 * 20 * 2 * 4
        assert lib.stp_threshold_counts_workspace_bytes(0) == 0 and lib.stp_threshold_counts_workspace_bytes(65) == 0


def test_argument_checks_come_before_any_launch():
    """STP_E_BADARG needs no device: NULL pointers and bad sizes are refused on a machine without one."""
    import ctypes as C
    from segmentation_training_pipeline_amd import _lib
    lib = _lib.load()
    assert lib.stp_mask_threshold(None, 4, 4, 1, 0, 0, 0.5, None, 4, None) == -1
    assert lib.stp_mask_morph(None, None, 4, 4, 2, 0, None) == -1
    assert lib.stp_mask_rle(None, 4, 4, None, None, 8, None, 0, None) == -1
    thr = (C.c_float * 2)(0.5, 0.25)
    assert lib.stp_threshold_counts(None, None, 4, 4, 1, 0, thr, 2, None, None, None, 0, None) == -1


def test_wrappers_have_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)                  # noqa: E731
    with pytest.raises(_lib.StpError):
        ops.mask_threshold(torch.zeros(4, 4, 1), 4, 4, 1, 0, 0, 0.5, u8(4, 4))
    with pytest.raises(_lib.StpError):
        ops.mask_morph(u8(4, 4), u8(4, 4), 4, 4, 2, 0)
    with pytest.raises(_lib.StpError):
        ops.mask_rle(u8(4, 4), 4, 4, torch.zeros(8, 2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), u8(64))
    with pytest.raises(_lib.StpError):
        ops.threshold_counts(torch.zeros(4, 4, 1), u8(4, 4), 4, 4, 1, 0, [0.5], torch.zeros(1, 2, dtype=torch.int64),
                             torch.zeros(2, dtype=torch.int64), u8(8192))
