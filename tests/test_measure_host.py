"""CPU tests of the per-object measurement path's host side (segmentation_pipeline/segmentation.py over csrc/measure.hip): the host
statement (tests/_measure_reference.py) agrees with numpy's and scipy's own per-object functions; the selection is the identity with
neutral arguments, keeps the order and keeps an object that meets the bound exactly; the new entry points are bound, refuse bad arguments
without a device and have no CPU fallback; the public methods have their signatures, and every refusal of theirs fires before a model
file is opened."""
import inspect

import numpy as np
import pytest
from scipy import ndimage

import _measure_reference as M


def the_reference_states_the_library():
    """The reference's constants are the public ones and the entry points it restates exist: a test of the reference alone starts here."""
    from segmentation_pipeline.segmentation import PipelineConfig
    from segmentation_training_pipeline_amd import _lib
    assert (M.CONF_ONE, M.CONF_DEN) == (PipelineConfig.CONF_ONE, PipelineConfig.CONF_DEN)
    assert "stp_label_measure" in _lib.SIGNATURES and "stp_label_select" in _lib.SIGNATURES


def config(**kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "batch": 4}
    return segmentation.PipelineConfig(**dict(base, **kw))


def seeded_inputs():
    """(labels, probs) pairs: smoothed random fields, labelled with the 8-neighbourhood, and salt images with the 4-neighbourhood."""
    out = []
    for k in range(8):
        rng = np.random.default_rng(100 + k)
        h, w = (int(v) for v in rng.integers(5, 60, 2))
        f = ndimage.gaussian_filter(rng.random((h, w)), 1.5)
        f = ((f - f.min()) / (f.max() - f.min())).astype(np.float32)
        out.append((ndimage.label(f > 0.5, np.ones((3, 3)))[0].astype(np.int32), f))
        out.append((ndimage.label(rng.random((h, w)) < 0.5)[0].astype(np.int32), rng.random((h, w)).astype(np.float32)))
    return out


def test_quantisation():
    the_reference_states_the_library()
    p = np.array([0.0, 1.0, 0.5, -0.25, 1.5, np.nan, np.inf, -np.inf, 1e-9, 0.99999994, 2.0 / 65535], np.float32)
    q = M.quantise(p)
    assert q.dtype == np.int64 and q.tolist() == [0, 65535, 32767, 0, 65535, 0, 65535, 0, 0, 65534, 2]
    rng = np.random.default_rng(3)
    q = M.quantise(rng.random(100000).astype(np.float32))
    assert q.min() >= 0 and q.max() <= 65535 and len(np.unique(q)) > 50000


def test_the_reference_agrees_with_numpy_and_scipy():
    the_reference_states_the_library()
    objects = 0
    for labels, probs in seeded_inputs():
        cap = int(labels.max())
        sums, boxes, outside = M.measure(labels, cap, probs)
        assert outside == 0 and sums.dtype == np.int64 and boxes.dtype == np.int32 and sums.shape == boxes.shape == (cap + 1, 4)
        assert np.array_equal(sums[1:, 0], np.bincount(labels.ravel(), minlength=cap + 1)[1:])
        assert sums[0].tolist() == [0, 0, 0, 0] and boxes[0].tolist() == [labels.shape[0], labels.shape[1], -1, -1]
        t = M.table(sums, boxes, cap)
        for k, sl in enumerate(ndimage.find_objects(labels)):
            assert (t["y0"][k], t["y1"][k], t["x0"][k], t["x1"][k]) == (sl[0].start, sl[0].stop, sl[1].start, sl[1].stop)
        index = np.arange(1, cap + 1)
        com = np.array(ndimage.center_of_mass(np.ones_like(labels), labels, index)).reshape(-1, 2)
        assert np.abs(t["cy"] - com[:, 0]).max() <= 1e-12 and np.abs(t["cx"] - com[:, 1]).max() <= 1e-12
        mean = ndimage.mean(M.quantise(probs), labels, index)
        assert np.abs(t["confidence"] * 65535 - mean).max() <= 1e-9
        assert t["label"].tolist() == index.tolist() and all(t[c].dtype == np.int64 for c in ("label", "area", "y0", "x0", "y1", "x1"))
        assert all(t[c].dtype == np.float64 for c in ("cy", "cx", "confidence")) and tuple(t) == M.COLUMNS
        objects += cap
    assert objects > 300


def test_out_of_range_labels_are_background():
    the_reference_states_the_library()
    labels = np.array([[1, 1, 0, 7], [-3, 2, 2, 9], [5, 5, 5, 2]], np.int32)
    sums, boxes, outside = M.measure(labels, 5)
    assert outside == 3 and sums[:, 0].tolist() == [0, 2, 3, 0, 0, 3]
    assert boxes.tolist() == [[3, 4, -1, -1], [0, 0, 0, 1], [1, 1, 2, 3], [3, 4, -1, -1], [3, 4, -1, -1], [2, 0, 2, 2]]
    assert sums[2].tolist() == [3, 1 + 1 + 2, 1 + 2 + 3, 0]
    out, count, s2, b2 = M.select(labels, 5, sums, boxes, 3, 0)
    assert count == 2 and out.tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [2, 2, 2, 1]]
    assert s2.tolist() == [[0, 0, 0, 0], sums[2].tolist(), sums[5].tolist()] and b2.tolist() == [[3, 4, -1, -1], [1, 1, 2, 3], [2, 0, 2, 2]]


def test_selection_properties():
    the_reference_states_the_library()
    dropped = 0
    for labels, probs in seeded_inputs():
        cap = int(labels.max())
        sums, boxes, _ = M.measure(labels, cap, probs)
        out, count, s2, b2 = M.select(labels, cap, sums, boxes, 0, 0)      # neutral: the identity on a contiguous labelling
        assert count == cap and np.array_equal(out, labels) and np.array_equal(s2, sums) and np.array_equal(b2, boxes)
        for min_area, conf in ((8, 0.5), (0, 0.6), (20, 0.55), (3, 0.4999)):
            out, count, s2, b2 = M.measure_select(labels, probs, 0, min_area, conf)
            keep = M.keep_flags(sums, min_area, M.conf_num(conf))
            assert count == int(keep.sum()) and np.array_equal(out != 0, keep[labels])
            old = np.flatnonzero(keep)                                   # the survivors keep their order
            for new, k in enumerate(old, start=1):
                assert np.array_equal(out == new, labels == k)
            assert np.array_equal(s2[1:], sums[old]) and np.array_equal(b2[1:], boxes[old])
            again = M.measure(out, count, probs)                         # the compacted rows are the measurement of the new image
            assert np.array_equal(again[0], s2) and np.array_equal(again[1], b2)
            dropped += cap - count
    assert dropped > 100


def test_an_object_on_the_bound_is_kept():
    the_reference_states_the_library()
    one = np.ones((1, 1), np.int32)
    sums, boxes, _ = M.measure(one, 1, np.ones((1, 1), np.float32))
    assert sums[1].tolist() == [1, 0, 0, 65535] and sums[1, 3] * 10000 == 10000 * 65535 * sums[1, 0]
    assert M.select(one, 1, sums, boxes, 1, M.conf_num(1.0))[1] == 1
    sums, boxes, _ = M.measure(one, 1, np.full((1, 1), 0.99999, np.float32))
    assert M.select(one, 1, sums, boxes, 1, M.conf_num(1.0))[1] == 0 and M.select(one, 1, sums, boxes, 1, 9999)[1] == 1
    assert M.select(one, 1, sums, boxes, 2, 0)[1] == 0
    two = np.ones((1, 2), np.int32)                                      # q = 32767 and 32768: the mean is 65535 / 2 exactly
    p = np.array([[32767.5 / 65535, 32768.5 / 65535]], np.float32)
    sums, boxes, _ = M.measure(two, 1, p)
    assert sums[1, 3] == 65535 and M.select(two, 1, sums, boxes, 0, 5000)[1] == 1 and M.select(two, 1, sums, boxes, 0, 5001)[1] == 0


# ------------------------------------------------------------------------------------------------ the entry points
def test_entry_points_are_bound():
    from segmentation_training_pipeline_amd import _lib, ops
    i32, i64, vp, sz = _lib.i32, _lib.i64, _lib.vp, _lib.sz
    assert _lib.SIGNATURES["stp_label_measure"] == (i32, [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp])
    assert _lib.SIGNATURES["stp_label_select_workspace_bytes"] == (sz, [i32])
    assert _lib.SIGNATURES["stp_label_select"] == (i32, [vp, i32, i32, i32, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, sz, vp])
    for name in ("label_measure", "label_select_workspace_bytes", "label_select"):
        assert callable(getattr(ops, name))
    for storage in ("bf16", "fp16"):                                     # both builds export the same code; the query runs without a GPU
        query = _lib.load(storage).stp_label_select_workspace_bytes
        assert query(-1) == 0 and query(0) == 16                         # the map (8-byte multiples) and one int32 per block of 256 labels
        assert query(255) == 1024 + 8 and query(256) == 1032 + 8 and query(1961) == 7848 + 32
        assert query(255) == ops.label_select_workspace_bytes(255)


def test_argument_checks_come_before_any_launch():
    """STP_E_BADARG and STP_E_WORKSPACE need no device: they are returned on a machine without one."""
    from segmentation_training_pipeline_amd import _lib
    lib = _lib.load()
    fake = 4096                                                          # a non-NULL, aligned address that is never dereferenced
    measure, select = lib.stp_label_measure, lib.stp_label_select
    assert measure(None, None, 4, 4, 1, 0, 4, fake, fake, fake, None) == -1
    assert measure(fake, None, 4, 4, 1, 0, 4, None, fake, fake, None) == -1 and measure(fake, None, 4, 4, 1, 0, 4, fake, None, fake, None) == -1
    assert measure(fake, None, 4, 4, 1, 0, 4, fake, fake, None, None) == -1
    for h, w in ((0, 4), (4, 0), (-1, 4), (32768, 1), (1, 32768)):
        assert measure(fake, None, h, w, 1, 0, 0, fake, fake, fake, None) == -1
    assert measure(fake, None, 4, 4, 1, 0, -1, fake, fake, fake, None) == -1 and measure(fake, None, 4, 4, 1, 0, 17, fake, fake, fake, None) == -1
    assert measure(fake, fake, 4, 4, 0, 0, 4, fake, fake, fake, None) == -1      # with probs: C >= 1 and 0 <= channel < C
    assert measure(fake, fake, 4, 4, 3, 3, 4, fake, fake, fake, None) == -1 and measure(fake, fake, 4, 4, 3, -1, 4, fake, fake, fake, None) == -1
    assert measure(fake, None, 4, 4, 1, 0, 4, fake + 4, fake, fake, None) == -1  # sums not 8-byte aligned
    big = 1 << 20
    ok = dict(labels=fake, h=4, w=4, cap=4, sums=fake, boxes=fake, min_area=0, num=0, den=10000, out=fake, count=fake, out_sums=fake + 512,
              out_boxes=fake + 1024, ws=fake + 2048, bytes=big)

    def sel(**kw):
        a = dict(ok, **kw)
        return select(a["labels"], a["h"], a["w"], a["cap"], a["sums"], a["boxes"], a["min_area"], a["num"], a["den"], a["out"], a["count"],
                      a["out_sums"], a["out_boxes"], a["ws"], a["bytes"], None)
    for name in ("labels", "sums", "boxes", "out", "count", "out_sums", "out_boxes", "ws"):
        assert sel(**{name: None}) == -1, name
    for kw in ({"h": 0}, {"w": -1}, {"h": 32768, "w": 1}, {"cap": -1}, {"cap": 17}, {"min_area": -1}, {"den": 0}, {"den": 10001},
               {"num": -1}, {"num": 10001}, {"num": 5, "den": 4}, {"out_sums": fake}, {"out_boxes": fake}, {"ws": fake + 2052}):
        assert sel(**kw) == -1, kw
    assert sel(bytes=lib.stp_label_select_workspace_bytes(4) - 1) == -3


def test_wrappers_have_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    lab = torch.zeros((4, 4), dtype=torch.int32)
    sums, boxes = torch.zeros((5, 4), dtype=torch.int64), torch.zeros((5, 4), dtype=torch.int32)
    word, count = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    ws = torch.zeros(ops.label_select_workspace_bytes(4), dtype=torch.uint8)
    with pytest.raises(_lib.StpError):
        ops.label_measure(lab, None, 4, 4, 1, 0, 4, sums, boxes, word)
    with pytest.raises(_lib.StpError):
        ops.label_measure(lab, torch.zeros((4, 4, 2)), 4, 4, 2, 1, 4, sums, boxes, word)
    with pytest.raises(_lib.StpError):
        ops.label_select(lab, 4, 4, 4, sums, boxes, 0, 0, 10000, lab.clone(), count, sums.clone(), boxes.clone(), ws)
    for bad in (dict(labels=lab.to(torch.int64)), dict(probs=torch.zeros((4, 4), dtype=torch.float64)), dict(sums=sums.to(torch.int32)),
                dict(boxes=boxes[:4]), dict(word=count), dict(probs=torch.zeros((4, 3)))):
        a = dict(dict(labels=lab, probs=None, sums=sums, boxes=boxes, word=word), **bad)
        with pytest.raises(ValueError):
            ops.label_measure(a["labels"], a["probs"], 4, 4, 1, 0, 4, a["sums"], a["boxes"], a["word"])
    with pytest.raises(ValueError):
        ops.label_select(lab, 4, 4, 4, sums, boxes, 0, 0, 10000, lab.to(torch.int64), count, sums.clone(), boxes.clone(), ws)
    with pytest.raises(ValueError):
        ops.label_select(lab, 4, 4, 4, sums, boxes, 0, 0, 10000, lab.clone(), count, sums[:4].clone(), boxes.clone(), ws)
    with pytest.raises(ValueError):
        ops.label_select(lab, 4, 4, 4, sums, boxes, 0, 0, 10000, lab.clone(), word, sums.clone(), boxes.clone(), ws)


# ------------------------------------------------------------------------------------------------ the public methods
def test_public_signatures():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    assert P.CONF_ONE == 65535 == M.CONF_ONE and P.CONF_DEN == 10000 == M.CONF_DEN
    assert list(inspect.signature(P.object_table).parameters) == ["sums", "boxes", "count"]
    assert list(inspect.signature(P.measure_labels).parameters) == ["labels", "probs", "channel"]
    assert [v.default for v in inspect.signature(P.measure_labels).parameters.values()][1:] == [None, 0]
    for name in ("object_table", "measure_labels"):
        assert isinstance(inspect.getattr_static(P, name), staticmethod)
    p, base = inspect.signature(P.predict_instances_ex).parameters, inspect.signature(P.predict_instances).parameters
    assert list(p) == list(base) + ["min_area", "min_confidence", "measure"]
    assert [p[k].default for k in list(base)[1:]] == [base[k].default for k in list(base)[1:]]
    assert [p[k].default for k in ("min_area", "min_confidence", "measure")] == [0, 0.0, False]
    p, base = inspect.signature(P.predict_instances_to_csv_ex).parameters, inspect.signature(P.predict_instances_to_csv).parameters
    assert list(p) == list(base) + ["min_area", "min_confidence", "measures"]
    assert [p[k].default for k in list(base)[1:]] == [base[k].default for k in list(base)[1:]]
    assert [p[k].default for k in ("min_area", "min_confidence", "measures")] == [0, 0.0, ()]
    p, base = inspect.signature(P.score_instances_ex).parameters, inspect.signature(P.score_instances).parameters
    assert list(p) == list(base) + ["min_area", "min_confidence"]
    assert [p[k].default for k in list(base)[1:]] == [base[k].default for k in list(base)[1:]]
    assert [p[k].default for k in ("min_area", "min_confidence")] == [0, 0.0]
    p = inspect.signature(P.find_confidence).parameters
    assert list(p) == ["self", "ds", "fold", "stage", "negatives", "ttflips", "thresholds", "confidences", "split", "min_size", "min_area", "opening",
                       "closing", "channel", "area_threshold", "metric", "iou_thresholds", "truth"]
    assert [p[k].default for k in list(p)[3:]] == [-1, "real", None, None, (0.0, 0.5, 0.6, 0.7, 0.8), 0.0, 0, 0, 0, 0, 0, 0, "f2", None, "mask"]


def test_object_table_is_the_reference_expression():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    for labels, probs in seeded_inputs()[:4]:
        cap = int(labels.max())
        sums, boxes, _ = M.measure(labels, cap, probs)
        got, want = P.object_table(sums, boxes, cap), M.table(sums, boxes, cap)
        assert tuple(got) == M.COLUMNS
        for c in M.COLUMNS:
            assert got[c].dtype == want[c].dtype and np.array_equal(got[c], want[c]), c
        few = P.object_table(sums, boxes, min(cap, 2))
        assert all(len(few[c]) == min(cap, 2) for c in M.COLUMNS)
    empty = P.object_table(np.zeros((1, 4), np.int64), np.array([[3, 4, -1, -1]], np.int32), 0)
    assert all(len(empty[c]) == 0 for c in M.COLUMNS)
    gap = P.object_table(np.array([[0] * 4, [0] * 4, [2, 3, 5, 65535]], np.int64), np.array([[3, 4, -1, -1]] * 2 + [[1, 2, 2, 3]], np.int32), 2)
    assert gap["area"].tolist() == [0, 2] and np.isnan(gap["cy"][0]) and np.isnan(gap["confidence"][0])
    assert (gap["cy"][1], gap["cx"][1], gap["confidence"][1]) == (1.5, 2.5, 0.5)
    assert (gap["y0"][1], gap["x0"][1], gap["y1"][1], gap["x1"][1]) == (1, 2, 3, 4)


def test_confidence_and_area_conversion():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    assert [P._conf_num(v) for v in (0, 0.0, 1, 1.0, 0.5, 0.55, 0.0001, 0.3333, np.float64(0.7), np.float32(0.25))] == \
        [0, 0, 10000, 10000, 5000, 5500, 1, 3333, 7000, 2500]
    for bad in (True, False, -0.1, 1.0001, 0.55555, float("nan"), float("inf"), "0.5", None, [0.5], 2):
        with pytest.raises(ValueError, match="min_confidence"):
            P._conf_num(bad)
    assert [P._min_area(v) for v in (0, 8, np.int64(3))] == [0, 8, 3]
    for bad in (True, -1, 2.0, "2", None):
        with pytest.raises(ValueError, match="min_area"):
            P._min_area(bad)


BAD_AREAS = (True, -1, 2.0, "2", None)
BAD_CONFIDENCES = (True, -0.1, 1.5, 0.55555, float("nan"), "0.5", None)


@pytest.fixture
def no_model_files(monkeypatch):
    """Any attempt to load a model fails the test: the refusals must come first."""
    from segmentation_pipeline.segmentation import PipelineConfig

    def load_model(self, fold=0, stage=-1):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(PipelineConfig, "load_model", load_model)


def test_predict_instances_ex_refusals(no_model_files, tmp_path):
    cfg, softmax = config(), config(classes=3, activation="softmax")
    nowhere = str(tmp_path / "no_such_directory")                         # never listed: every refusal comes at the call, not at next()
    csv = str(tmp_path / "x.csv")
    for bad in BAD_AREAS:
        with pytest.raises(ValueError, match="min_area"):
            cfg.predict_instances_ex(nowhere, min_area=bad)
        with pytest.raises(ValueError, match="min_area"):
            cfg.predict_instances_to_csv_ex(nowhere, csv, min_area=bad)
    for bad in BAD_CONFIDENCES:
        with pytest.raises(ValueError, match="min_confidence"):
            cfg.predict_instances_ex(nowhere, min_confidence=bad)
        with pytest.raises(ValueError, match="min_confidence"):
            cfg.predict_instances_to_csv_ex(nowhere, csv, min_confidence=bad)
    for kw, what in (({"channel": 1}, "channel"), ({"opening": 8}, "opening"), ({"closing": 1.5}, "closing"), ({"min_size": -1}, "min_size"),
                     ({"area_threshold": True}, "area_threshold"), ({"split": -1}, "split"), ({"split": True}, "split")):
        with pytest.raises(ValueError, match=what):
            cfg.predict_instances_ex(nowhere, min_confidence=0.5, **kw)
        with pytest.raises(ValueError, match=what):
            cfg.predict_instances_to_csv_ex(nowhere, csv, measures=("area",), **kw)
    with pytest.raises(ValueError, match="threshold"):
        softmax.predict_instances_ex(nowhere, threshold=0.25, measure=True)
    with pytest.raises(ValueError, match="columns"):
        cfg.predict_instances_to_csv_ex(nowhere, csv, columns=("image",))
    with pytest.raises(ValueError, match="columns"):
        cfg.predict_instances_to_csv_ex(nowhere, csv, columns=("image", "rle", "area"))
    for bad in (("area", "perimeter"), ("label",), "area", (0,)):
        with pytest.raises(ValueError, match="measures"):
            cfg.predict_instances_to_csv_ex(nowhere, csv, measures=bad)
    assert not (tmp_path / "x.csv").exists()


def test_score_instances_ex_refusals(no_model_files):
    ds = object()                                                        # never looked at: every refusal comes before the dataset is
    cfg, softmax = config(), config(classes=3, activation="softmax")
    for bad in BAD_AREAS:
        with pytest.raises(ValueError, match="min_area"):
            cfg.score_instances_ex(ds, 0, min_area=bad)
    for bad in BAD_CONFIDENCES:
        with pytest.raises(ValueError, match="min_confidence"):
            cfg.score_instances_ex(ds, 0, min_confidence=bad)
    with pytest.raises(ValueError, match="threshold"):
        softmax.score_instances_ex(ds, 0, threshold=0.25, min_confidence=0.5)
    for kw, what in (({"metric": "dice"}, "metric"), ({"truth": "rle"}, "truth"), ({"channel": 1}, "channel"), ({"opening": 8}, "opening"),
                     ({"min_size": 2.0}, "min_size"), ({"area_threshold": True}, "area_threshold"), ({"split": 1025}, "split"),
                     ({"iou_thresholds": [0.45]}, "0.5"), ({"iou_thresholds": [0.9, 0.8]}, "ascending")):
        with pytest.raises(ValueError, match=what):
            cfg.score_instances_ex(ds, 0, min_confidence=0.5, **kw)


def test_find_confidence_refusals(no_model_files):
    ds = object()
    cfg, softmax = config(), config(classes=3, activation="softmax")
    with pytest.raises(ValueError, match="softmax"):
        softmax.find_confidence(ds, 0, thresholds=[0.5])
    for bad in ([0.5, 0.25], [0.25, 0.25], [0.1, float("nan")], [], [i / 100 for i in range(65)]):
        with pytest.raises(ValueError, match="thresholds"):
            cfg.find_confidence(ds, 0, thresholds=bad)
    for bad in ((), tuple(i / 100 for i in range(65)), (0.5, 0.5), (0.6, 0.5), (0.5, True), (-0.1, 0.5), (0.5, 1.5), (0.5, float("nan")),
                (0.5, "0.6"), (None,), (0.55555,)):
        with pytest.raises(ValueError, match="confidences"):
            cfg.find_confidence(ds, 0, confidences=bad)
    for kw, what in (({"metric": "iou"}, "metric"), ({"truth": None}, "truth"), ({"channel": -1}, "channel"), ({"opening": -1}, "opening"),
                     ({"min_size": -1}, "min_size"), ({"min_area": 1.5}, "min_area"), ({"min_area": True}, "min_area"),
                     ({"split": -1}, "split"), ({"area_threshold": -2}, "area_threshold"), ({"iou_thresholds": [0.3]}, "0.5")):
        with pytest.raises(ValueError, match=what):
            cfg.find_confidence(ds, 0, **kw)


def test_measure_labels_refusals():
    from segmentation_pipeline.segmentation import PipelineConfig
    ok = np.ones((4, 5), np.int32)
    for labels in (ok[0], ok[:0], ok[:, :, None], ok.astype(np.float32), ok.astype(object), np.array([["a"]])):
        with pytest.raises(ValueError, match="label image"):
            PipelineConfig.measure_labels(labels)
    for labels in (ok - 2, ok * 21):
        with pytest.raises(ValueError, match="object numbers"):
            PipelineConfig.measure_labels(labels)
    for probs in (np.ones((4, 4), np.float32), np.ones((4, 5, 2, 1), np.float32), np.ones(20, np.float32), np.array([["a"] * 5] * 4),
                  np.ones((4, 5, 0), np.float32)):
        with pytest.raises(ValueError, match="probs"):
            PipelineConfig.measure_labels(ok, probs)
    for channel in (2, -1, True, 0.0):
        with pytest.raises(ValueError, match="channel"):
            PipelineConfig.measure_labels(ok, np.ones((4, 5, 2), np.float32), channel)
