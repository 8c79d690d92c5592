"""CPU tests of the object-score path's host side (segmentation_pipeline/segmentation.py over csrc/object_match.hip): the two host
statements of the true positives (tests/_object_match_reference.py: the kernel's integer arithmetic and the competitions' dense IoU
matrix) agree; ``object_score`` on hand-made counters; every refusal of ``score_objects`` / ``find_object_threshold`` /
``object_overlaps`` fires before a model file is opened; the conversion of ``iou_thresholds``; the new entry points are bound, refuse bad
arguments without a device and have no CPU fallback."""
import inspect

import numpy as np
import pytest

import _object_match_reference as R

TS = [n / 20 for n in R.DEFAULT_NUM]


def config(**kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "batch": 4}
    return segmentation.PipelineConfig(**dict(base, **kw))


def cases():
    """(pred mask, truth mask): discs against the same discs shifted and flipped, and salt-and-pepper against salt-and-pepper."""
    out = []
    for k, (h, w) in enumerate([(1, 1), (5, 9), (23, 31), (40, 64), (64, 70), (90, 120)]):
        for j, (shift, flip) in enumerate([((0, 0), 0.0), ((1, 0), 0.002), ((1, 2), 0.02)]):
            out.append((R.discs(h, w, 10 * k + j, shift, flip, 1), R.discs(h, w, 10 * k + j, (0, 0), flip, 2)))
        out.append((R.salt(h, w, 100 + k), R.salt(h, w, 200 + k)))
    return out


def test_the_two_reference_statements_agree():
    sums = np.zeros(len(TS), np.int64)
    for pm, gm in cases():
        (p, n_p), (g, n_g) = R.label8(pm), R.label8(gm)
        got = R.label_match(p, g, (p.size + 1) // 2)
        want, partners = R.kaggle_true_positives(p, g, TS)
        assert got[:len(TS)].tolist() == want and got[len(TS):].tolist() == [n_p, n_g, 0]
        assert partners <= 1                                           # t >= 1/2: no label has two partners, so no assignment step
        sums += got[:len(TS)]
    print("TP sums per threshold:", sums.tolist())
    assert sums[0] > sums[-1] > 0 and len(set(sums.tolist())) >= 5     # the inputs discriminate between the thresholds


def test_reference_edge_cases():
    full = np.ones((4, 5), np.int32)
    zero = np.zeros((4, 5), np.int32)
    assert R.label_match(full, full, 10, [1, 2], 2).tolist() == [1, 0, 1, 1, 0]          # IoU 1: above 1/2, not above 1
    assert R.label_match(zero, full, 10).tolist() == [0] * 10 + [0, 1, 0]
    assert R.label_match(full, zero, 10).tolist() == [0] * 10 + [1, 0, 0]
    a = np.array([[1, 1, 1, 0], [7, 7, 0, 0]], np.int32)                                 # 7 is above the cap of 5
    b = np.array([[2, 2, 0, 0], [2, -1, 0, 9]], np.int32)
    triples, area_p, area_g, outside = R.overlaps(a, b, 5)
    assert triples.tolist() == [[1, 2, 2]] and area_p.tolist() == [0, 3, 0, 0, 0, 0] and area_g.tolist() == [0, 0, 3, 0, 0, 0]
    assert outside == 3                                                                  # (1, 0), (1, 1) - counted once - and (1, 3)
    # I = 2, U = 3 + 3 - 2 = 4: IoU exactly 1/2 does not exceed 1/2
    assert R.label_match(a, b, 5, [1], 2).tolist() == [0, 1, 1, 3]


def test_object_score_on_hand_made_counters():
    from segmentation_pipeline.segmentation import PipelineConfig
    for score in (R.object_score, PipelineConfig.object_score):
        for metric in ("f2", "ap"):
            assert float(score(metric, 0, 0, 0)) == 1.0                # nothing predicted, nothing there
            assert float(score(metric, 0, 3, 0)) == 0.0                # no truth, with predictions
            assert float(score(metric, 0, 0, 3)) == 0.0
            assert float(score(metric, 4, 4, 4)) == 1.0
        assert float(score("f2", 2, 3, 4)) == 10 / (10 + 8 + 1)        # TP 2, FP 1, FN 2
        assert float(score("ap", 2, 3, 4)) == 2 / 5
        got = score("f2", np.array([[2, 0], [0, 0]]), np.array([[3], [0]]), np.array([[4], [0]]))
        assert got.dtype == np.float64 and got.tolist() == [[10 / 19, 0.0], [1.0, 1.0]]
    with pytest.raises(ValueError, match="metric"):
        PipelineConfig.object_score("dice", 1, 1, 1)


def test_iou_thresholds_conversion():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    nums, ts = P._iou_fractions(None)
    assert nums == list(range(500, 1000, 50)) and ts == [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]
    assert P._iou_fractions(np.arange(0.5, 1.0, 0.05)) == (nums, ts)                      # the notebooks' float steps, exactly
    assert P._iou_fractions([0.5, 0.725, 1])[0] == [500, 725, 1000]
    assert P._iou_fractions([i / 1000 for i in range(500, 564)])[0] == list(range(500, 564))
    for bad, what in (([0.45], "0.5"), ([0.5005], "three places"), ([0.7, 0.6], "ascending"), ([0.6, 0.6], "ascending"), ([1.001], "0.5"),
                      ([float("nan")], "three places"), ([], "64"), ([i / 1000 for i in range(500, 565)], "64")):
        with pytest.raises(ValueError, match=what):
            P._iou_fractions(bad)


@pytest.fixture
def no_model_files(monkeypatch):
    """Any attempt to load a model fails the test: the refusals must come first."""
    from segmentation_pipeline.segmentation import PipelineConfig

    def load_model(self, fold=0, stage=-1):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(PipelineConfig, "load_model", load_model)


def test_score_objects_refusals(no_model_files):
    ds = object()                                                      # never looked at: every refusal comes before the dataset is
    cfg, softmax = config(), config(classes=3, activation="softmax")
    with pytest.raises(ValueError, match="threshold"):
        softmax.score_objects(ds, 0, threshold=0.25)
    for kw, what in (({"metric": "dice"}, "metric"), ({"truth": "rle"}, "truth"), ({"channel": 1}, "channel"), ({"opening": 8}, "opening"),
                     ({"closing": 1.5}, "closing"), ({"min_size": -1}, "min_size"), ({"min_size": 2.0}, "min_size"),
                     ({"area_threshold": True}, "area_threshold"), ({"iou_thresholds": [0.45]}, "0.5"),
                     ({"iou_thresholds": [0.5005]}, "three places"), ({"iou_thresholds": [0.9, 0.8]}, "ascending"),
                     ({"iou_thresholds": [i / 1000 for i in range(500, 565)]}, "64")):
        with pytest.raises(ValueError, match=what):
            cfg.score_objects(ds, 0, **kw)
    with pytest.raises(ValueError, match="channel"):
        softmax.score_objects(ds, 0, channel=3)


def test_find_object_threshold_refusals(no_model_files):
    ds = object()
    cfg, softmax = config(), config(classes=3, activation="softmax")
    with pytest.raises(ValueError, match="softmax"):
        softmax.find_object_threshold(ds, 0, thresholds=[0.5])
    for bad in ([0.5, 0.25], [0.25, 0.25], [0.1, float("nan")], [], [i / 100 for i in range(65)]):
        with pytest.raises(ValueError, match="thresholds"):
            cfg.find_object_threshold(ds, 0, thresholds=bad)
    for bad in ((), (-1,), (2.5,), (4, 4), (9, 4)):
        with pytest.raises(ValueError, match="min_size"):
            cfg.find_object_threshold(ds, 0, min_sizes=bad)
    for kw, what in (({"metric": "iou"}, "metric"), ({"truth": None}, "truth"), ({"channel": -1}, "channel"), ({"opening": -1}, "opening"),
                     ({"iou_thresholds": [0.3]}, "0.5")):
        with pytest.raises(ValueError, match=what):
            cfg.find_object_threshold(ds, 0, **kw)


def test_object_overlaps_refusals():
    from segmentation_pipeline.segmentation import PipelineConfig
    ok = np.ones((4, 5), np.int32)
    for p, g in ((ok, np.ones((5, 4), np.int32)), (ok.astype(np.float32), ok), (ok[0], ok[0]), (ok[:0], ok[:0]), (ok * -1, ok), (ok, ok * 21)):
        with pytest.raises(ValueError):
            PipelineConfig.object_overlaps(p, g)


def test_public_signatures():
    from segmentation_pipeline.segmentation import PipelineConfig
    p = inspect.signature(PipelineConfig.score_objects).parameters
    assert list(p) == ["self", "ds", "fold", "stage", "negatives", "ttflips", "threshold", "opening", "closing", "channel", "min_size",
                       "area_threshold", "metric", "iou_thresholds", "truth"]
    assert [p[k].default for k in list(p)[3:]] == [-1, "real", None, 0.5, 0, 0, 0, 0, 0, "f2", None, "mask"]
    p = inspect.signature(PipelineConfig.find_object_threshold).parameters
    assert list(p)[:8] == ["self", "ds", "fold", "stage", "negatives", "ttflips", "thresholds", "min_sizes"]
    assert p["thresholds"].default is None and p["min_sizes"].default == (0,) and p["metric"].default == "f2"
    assert list(inspect.signature(PipelineConfig.object_overlaps).parameters) == ["pred_labels", "truth_labels"]


def test_entry_points_are_bound():
    import ctypes as C
    from segmentation_training_pipeline_amd import _lib, ops
    i32, i64, vp, sz = _lib.i32, _lib.i64, _lib.vp, _lib.sz
    assert _lib.SIGNATURES["stp_label_match_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_label_overlaps_workspace_bytes"] == (sz, [i32, i32])
    res, args = _lib.SIGNATURES["stp_label_match"]
    assert res == i32 and args[:5] == [vp, vp, i32, i32, i32] and args[5] == C.POINTER(i32) and args[6:] == [i32, i32, vp, vp, sz, vp]
    assert _lib.SIGNATURES["stp_label_overlaps"] == (i32, [vp, vp, i32, i32, i32, vp, vp, i64, vp, vp, vp, vp, sz, vp])
    for name in ("label_match", "label_overlaps", "label_match_workspace_bytes", "label_overlaps_workspace_bytes"):
        assert callable(getattr(ops, name))
    for storage in ("bf16", "fp16"):                                   # both builds export the same code; the queries run without a GPU
        lib = _lib.load(storage)
        for query in (lib.stp_label_match_workspace_bytes, lib.stp_label_overlaps_workspace_bytes):
            assert query(1, 1) == 16 + 2 * 12                          # two areas of 2 entries, 2 slots of 12 bytes
            assert query(64, 64) == 2 * 4097 * 4 + 8 + 8192 * 12       # 2 h w = 8192 slots
            assert query(37, 53) == 2 * 1962 * 4 + 4096 * 12           # 2 h w = 3922 -> 4096 slots
            assert query(0, 5) == 0 and query(5, -1) == 0 and query(1 << 16, 1 << 15) == 0


def test_argument_checks_come_before_any_launch():
    """STP_E_BADARG needs no device: NULL pointers and bad thresholds are refused on a machine without one."""
    import ctypes as C
    from segmentation_training_pipeline_amd import _lib
    lib = _lib.load()
    num = (C.c_int32 * 2)(10, 15)
    assert lib.stp_label_match(None, None, 4, 4, 8, num, 2, 20, None, None, 0, None) == -1
    assert lib.stp_label_overlaps(None, None, 4, 4, 8, None, None, 16, None, None, None, None, 0, None) == -1
    fake = 4096                                                        # a non-NULL, aligned address that is never dereferenced
    args = lambda n, T, den, h=4, w=4, cap=8: (fake, fake, h, w, cap, n, T, den, fake, fake, 1 << 20, None)      # noqa: E731
    assert lib.stp_label_match(*args((C.c_int32 * 1)(9), 1, 20)) == -1                     # 2 * num < den
    assert lib.stp_label_match(*args((C.c_int32 * 1)(21), 1, 20)) == -1                    # num > den
    assert lib.stp_label_match(*args((C.c_int32 * 2)(15, 15), 2, 20)) == -1                # not ascending
    assert lib.stp_label_match(*args(num, 0, 20)) == -1 and lib.stp_label_match(*args((C.c_int32 * 65)(*range(500, 565)), 65, 1000)) == -1
    assert lib.stp_label_match(*args(num, 2, 0)) == -1 and lib.stp_label_match(*args((C.c_int32 * 1)(1001), 1, 1001)) == -1
    assert lib.stp_label_match(*args(num, 2, 20, h=0)) == -1 and lib.stp_label_match(*args(num, 2, 20, w=-3)) == -1
    assert lib.stp_label_match(*args(num, 2, 20, cap=-1)) == -1 and lib.stp_label_match(*args(num, 2, 20, cap=17)) == -1
    assert lib.stp_label_match(fake, fake, 4, 4, 8, num, 2, 20, fake, fake, lib.stp_label_match_workspace_bytes(4, 4) - 1, None) == -3
    assert lib.stp_label_overlaps(fake, fake, 4, 4, 8, fake, fake, 15, fake, fake, fake, fake, 1 << 20, None) == -1      # capacity < h w
    assert lib.stp_label_overlaps(fake, fake, 4, 4, 8, fake, fake, 16, fake, fake, fake, fake,
                                  lib.stp_label_overlaps_workspace_bytes(4, 4) - 1, None) == -3


def test_wrappers_have_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    lab = torch.zeros((4, 4), dtype=torch.int32)
    ws = torch.zeros(ops.label_match_workspace_bytes(4, 4), dtype=torch.uint8)
    with pytest.raises(_lib.StpError):
        ops.label_match(lab, lab, 4, 4, 8, [10, 15], 20, torch.zeros(5, dtype=torch.int64), ws)
    with pytest.raises(_lib.StpError):
        ops.label_overlaps(lab, lab, 4, 4, 8, torch.zeros((16, 3), dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                           torch.zeros(9, dtype=torch.int32), torch.zeros(9, dtype=torch.int32), torch.zeros(1, dtype=torch.int64), ws)
    with pytest.raises(ValueError):
        ops.label_match(lab.to(torch.int64), lab, 4, 4, 8, [10], 20, torch.zeros(4, dtype=torch.int64), ws)
