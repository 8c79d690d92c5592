"""CPU tests of the connected-component path's host side (segmentation_pipeline/segmentation.py over csrc/components.hip): the host
statements the GPU tests compare with (tests/_components_reference.py) on hand-checked cases; grouping the run triples by label
reproduces ``impl.rle.multi_rle_encode``; every new refusal of ``predict_masks_ex`` / ``predict_to_csv`` fires before a model file is
opened; ``predict_masks`` keeps its call shape and ``predict_masks_ex`` extends it; the new entry points are bound and their wrappers have no CPU fallback."""
import inspect

import numpy as np
import pytest

import _components_reference as R


def config(**kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "batch": 4}
    return segmentation.PipelineConfig(**dict(base, **kw))


def test_label_on_hand_checked_cases():
    eye = np.eye(3, dtype=np.uint8)
    labels, n = R.label(eye, 1)
    assert n == 3 and labels.tolist() == [[1, 0, 0], [0, 2, 0], [0, 0, 3]] and labels.dtype == np.int32
    labels, n = R.label(eye, 2)
    assert n == 1 and np.array_equal(labels, eye)
    labels, n = R.label(eye, 1, invert=1)                                   # the zeros of eye(3): two corners of three pixels
    assert n == 2 and labels.tolist() == [[0, 1, 1], [2, 0, 1], [2, 2, 0]]
    # components are numbered by their first pixel in row-major order, whatever their shape
    m = np.array([[0, 0, 1, 0, 1], [1, 0, 1, 0, 1], [1, 1, 1, 0, 0]], np.uint8)
    assert R.label(m, 1)[0].tolist() == [[0, 0, 1, 0, 2], [1, 0, 1, 0, 2], [1, 1, 1, 0, 0]]


def test_remove_small_objects_is_strict():
    m = np.array([[1, 1, 0, 1], [0, 0, 0, 0], [1, 0, 1, 1]], np.uint8)      # sizes 2, 1, 1, 2
    assert np.array_equal(R.remove_small_objects(m, 0), m) and np.array_equal(R.remove_small_objects(m, 1), m)
    assert R.remove_small_objects(m, 2).tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1]]      # exactly 2 pixels: stays
    assert R.remove_small_objects(m, 3).sum() == 0
    diag = np.eye(3, dtype=np.uint8)
    assert R.remove_small_objects(diag, 2, connectivity=1).sum() == 0 and np.array_equal(R.remove_small_objects(diag, 2, connectivity=2), diag)


def test_remove_small_holes_on_a_ring_and_at_the_border():
    ring = np.ones((3, 3), np.uint8)
    ring[1, 1] = 0
    assert R.remove_small_holes(ring, 2).all()                               # the one-pixel hole is smaller than 2
    assert np.array_equal(R.remove_small_holes(ring, 1), ring)               # and not smaller than 1
    border = np.ones((4, 5), np.uint8)
    border[0, 0] = border[3, 2] = border[3, 3] = 0                           # zeros that touch the image border
    assert R.remove_small_holes(border, 2)[0, 0] == 1 and R.remove_small_holes(border, 2)[3, 2] == 0
    assert R.remove_small_holes(border, 3).all()
    s = R.serpentine(67, 71)
    assert int(s.sum()) == 2447 and R.label(s, 1)[1] == 1
    assert np.array_equal(R.remove_small_holes(s, 70), s) and R.remove_small_holes(s, 71).all()


def test_label_runs_follow_the_flat_column_major_array():
    assert R.label_runs(np.array([[0, 2], [1, 1]])).tolist() == [[1, 2, 1], [2, 3, 1], [1, 4, 1]]
    wrap = np.array([[0, 3], [3, 0]])                                        # bottom of column 0, top of column 1, the same label
    assert R.label_runs(wrap).tolist() == [[3, 2, 2]] and R.column_wraps(wrap) == (1, 0)
    other = np.array([[0, 4], [3, 0]])                                       # another label: two runs
    assert R.label_runs(other).tolist() == [[3, 2, 1], [4, 3, 1]] and R.column_wraps(other) == (0, 1)
    assert R.label_runs(np.zeros((3, 4), np.int32)).shape == (0, 3) and R.label_runs(np.zeros((3, 4), np.int32)).dtype == np.int32
    assert R.label_runs(np.full((3, 4), 7)).tolist() == [[7, 1, 12]]


def test_grouped_runs_are_multi_rle_encode():
    from segmentation_pipeline.segmentation import PipelineConfig
    rng = np.random.default_rng(12)
    for shape, p in (((37, 53), 0.5), ((20, 9), 0.3), ((1, 40), 0.6), ((40, 1), 0.6), ((5, 5), 0.0)):
        m = (rng.random(shape) < p).astype(np.uint8)
        labels, n = R.label(m, 2)
        runs = R.label_runs(labels)
        want = R.multi_rle(m)
        assert len(want) == n
        assert R.group_runs(runs, n) == want and PipelineConfig._group_runs(runs, n) == want
    assert PipelineConfig._group_runs(np.zeros((0, 3), np.int32), 0) == []


@pytest.fixture
def no_model_files(monkeypatch):
    """Any attempt to load a model fails the test: the refusals must come first."""
    from segmentation_pipeline.segmentation import PipelineConfig

    def load_model(self, fold=0, stage=-1):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(PipelineConfig, "load_model", load_model)


def test_new_refusals(tmp_path, no_model_files):
    cfg = config()
    for kw in ({"min_size": -1}, {"area_threshold": -1}, {"min_size": 1.5}, {"area_threshold": 64.0}, {"min_size": "64"}, {"min_size": None},
               {"area_threshold": True}):
        with pytest.raises(ValueError, match="min_size|area_threshold"):
            cfg.predict_masks_ex(str(tmp_path), **kw)                          # (raised by the call, not by the first next())
        with pytest.raises(ValueError, match="min_size|area_threshold"):
            cfg.predict_to_csv(str(tmp_path), str(tmp_path / "out.csv"), **kw)
    assert not (tmp_path / "out.csv").exists()
    # what passes the checks is a generator that has not touched a model yet
    assert inspect.isgenerator(cfg.predict_masks_ex(str(tmp_path), min_size=64, area_threshold=np.int64(64), components=True))
    assert inspect.isgenerator(config(classes=3, activation="softmax").predict_masks_ex(str(tmp_path), channel=2, min_size=9, rle=False))


def test_predict_masks_keeps_its_call_shape_and_the_new_keywords_follow_it():
    from segmentation_pipeline.segmentation import PipelineConfig
    old = inspect.signature(PipelineConfig.predict_masks)
    b = old.bind(None, "dir", 1, 0, 5, True, 0.25, 1, 2, 0, False)           # the positional call predict_to_csv used to make
    assert b.arguments["channel"] == 0 and b.arguments["rle"] is False and b.arguments["closing"] == 2
    assert list(old.parameters)[-1] == "rle"                                 # predict_masks itself takes none of the new keywords
    new = inspect.signature(PipelineConfig.predict_masks_ex)
    p = new.parameters
    assert list(p) == list(old.parameters) + ["min_size", "area_threshold", "components"]
    assert [p[k].default for k in old.parameters] == [v.default for v in old.parameters.values()]
    assert [p[k].default for k in ("min_size", "area_threshold", "components")] == [0, 0, False]
    b = new.bind(None, "dir", 1, 0, 5, True, 0.25, 1, 2, 0, False)
    assert b.arguments["channel"] == 0 and b.arguments["rle"] is False
    p = inspect.signature(PipelineConfig.predict_to_csv).parameters
    assert list(p)[-4:] == ["columns", "min_size", "area_threshold", "components"]
    assert [p[k].default for k in list(p)[-3:]] == [0, 0, False]


def test_entry_points_are_bound():
    from segmentation_training_pipeline_amd import _lib, ops
    i32, i64, vp, sz = _lib.i32, _lib.i64, _lib.vp, _lib.sz
    assert _lib.SIGNATURES["stp_mask_label_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_mask_label"] == (i32, [vp, i32, i32, i32, i32, vp, vp, vp, sz, vp])
    assert _lib.SIGNATURES["stp_mask_area_filter_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_mask_area_filter"] == (i32, [vp, vp, i32, i32, i32, i32, i64, vp, sz, vp])
    assert _lib.SIGNATURES["stp_label_rle_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_label_rle"] == (i32, [vp, i32, i32, vp, vp, i64, vp, sz, vp])
    for storage in ("bf16", "fp16"):                                         # both builds export the same code; the queries run without a GPU
        lib = _lib.load(storage)
        assert lib.stp_mask_label_workspace_bytes(64, 64) == 4096 * 4 + 16 * 2 * 4          # parents + 2 ints per workgroup of 256 pixels
        assert lib.stp_mask_label_workspace_bytes(3, 5) == 15 * 4 + 16
        assert lib.stp_mask_area_filter_workspace_bytes(37, 53) == 37 * 53 * 8              # parents + areas
        assert lib.stp_label_rle_workspace_bytes(70, 133) == 9310 * 4 + 10 * 4 * 4          # the flat array + 4 ints per 1024 pixels
        for query in (lib.stp_mask_label_workspace_bytes, lib.stp_mask_area_filter_workspace_bytes, lib.stp_label_rle_workspace_bytes):
            assert query(0, 5) == 0 and query(5, -1) == 0 and query(1 << 16, 1 << 15) == 0
    assert ops.mask_label_workspace_bytes(64, 64) > 0 and ops.mask_area_filter_workspace_bytes(64, 64) > 0
    assert ops.label_rle_workspace_bytes(64, 64) > 0


def test_argument_checks_come_before_any_launch():
    """STP_E_BADARG needs no device: NULL pointers and bad sizes are refused on a machine without one."""
    from segmentation_training_pipeline_amd import _lib
    lib = _lib.load()
    assert lib.stp_mask_label(None, 4, 4, 1, 0, None, None, None, 0, None) == -1
    assert lib.stp_mask_area_filter(None, None, 4, 4, 1, 0, 9, None, 0, None) == -1
    assert lib.stp_label_rle(None, 4, 4, None, None, 16, None, 0, None) == -1


def test_wrappers_have_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)                        # noqa: E731
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)                       # noqa: E731
    with pytest.raises(_lib.StpError):
        ops.mask_label(u8(4, 4), 4, 4, 1, 0, i32(4, 4), i32(1), u8(256))
    with pytest.raises(_lib.StpError):
        ops.mask_area_filter(u8(4, 4), u8(4, 4), 4, 4, 1, 0, 9, u8(256))
    with pytest.raises(_lib.StpError):
        ops.label_rle(i32(4, 4), 4, 4, i32(16, 3), i32(1), u8(256))
