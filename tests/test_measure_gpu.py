"""GPU tests of the per-object measurement methods of ``PipelineConfig`` (segmentation_pipeline/segmentation.py over csrc/measure.hip):
``predict_instances_ex``, ``predict_instances_to_csv_ex``, ``score_instances_ex``, ``find_confidence`` and ``measure_labels`` against the
host chain they replace - the ``rle=False`` label images of ``predict_instances`` and the maps of ``predict_in_directory``, then
tests/_measure_reference.py, ``impl.rle.rle_encode`` and the pair-histogram score of tests/_object_match_reference.py - by string and
array equality, and scores by ``==``.

The experiment of test_split_gpu.py: an untrained U-Net/resnet18 at 64 x 64, batch 2, saved as the models of two folds, and a directory
of four images of differing sizes.  ``min_confidence`` is chosen on the reference side: the first of a few quantiles of the reference
objects' confidences, rounded to four places, that drops an object and keeps one."""
import csv
import os
import types

import numpy as np
import pytest
import torch
import yaml

import _components_reference as CR
import _measure_reference as M
import _object_match_reference as OM

pytestmark = pytest.mark.gpu

SIZES = {"a.x.png": (50, 70), "b.png": (64, 64), "c.png": (37, 53), "d.png": (70, 133)}      # (h, w); "a.x.png" -> image column "a"
MASK_QUANTILE = 0.3                                                  # the threshold: most pixels are foreground, in blobs joined by necks
CONF_QUANTILES = (0.5, 0.3, 0.7, 0.15, 0.85)                         # candidates for min_confidence, in order of preference
SPLIT = 1.5
MIN_AREA = 3
NUMS, DEN = list(range(500, 1000, 50)), 1000
TS = [n / DEN for n in NUMS]
MEASURES = ("area", "confidence", "y0", "x0", "y1", "x1", "cy", "cx")


def _memo(fn):
    cache = {}

    def load(fold=0, stage=-1):
        if stage < 0:
            stage = 0                                        # (one stage: -1 is stage 0)
        if (fold, stage) not in cache:
            cache[(fold, stage)] = fn(fold, stage)
        return cache[(fold, stage)]
    return load


class ListDataSet(object):
    """The images of a directory with masks held in memory: ``y`` [h, w, 1]."""

    def __init__(self, path, ys):
        from segmentation_pipeline.impl.datasets import DirectoryDataSet
        self.src, self.ys = DirectoryDataSet(path), ys

    def __len__(self):
        return len(self.src)

    def __getitem__(self, i):
        from segmentation_pipeline.impl.datasets import PredictionItem
        it = self.src[i]
        return PredictionItem(it.id, it.x, self.ys[it.id][:, :, None])

    def isPositive(self, i):
        return bool(self.ys[self.src[i].id].any())


def experiment(root, classes, activation, loss):
    from PIL import Image
    from segmentation_pipeline import segmentation
    conf = {"architecture": "Unet", "backbone": "resnet18", "classes": classes, "activation": activation, "encoder_weights": None,
            "shape": [64, 64, 3], "batch": 2, "dtype": "fp32", "loss": loss, "folds_count": 2, "stages": [{"epochs": 1}]}
    with open(str(root / "config.yaml"), "w") as f:
        yaml.safe_dump(conf, f)
    cfg = segmentation.parse(str(root / "config.yaml"))
    net = cfg.createNet1(True)
    net.compile(loss=loss, batch=2, dtype="fp32")
    for fold, seed in ((0, 11), (1, 23)):
        net.impl.init_weights(seed)
        w = net.impl.get_weights()
        net.impl.set_weights({k: np.full_like(v, 0.7) for k, v in w.items() if k.endswith("/gamma")})     # (keeps the logits of a deep random net small)
        net.impl.save_weights(cfg.weightsPath(fold, 0))
    del net
    cfg.load_model = _memo(cfg.load_model)
    rng = np.random.RandomState(5)
    os.makedirs(str(root / "images"))
    for name, (h, w) in SIZES.items():
        Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(str(root / "images" / name))
    return types.SimpleNamespace(cfg=cfg, images=str(root / "images"), root=root)


def maps_of(e, channel=0, **kw):
    """The finished maps [h, w, C] of ``predict_in_directory`` by file name."""
    maps = {}
    e.cfg.predict_in_directory(e.images, kw.get("fold", 0), kw.get("stage", 0), lambda name, mp, data: data.__setitem__(name, mp.arr), maps,
                               ttflips=kw.get("ttflips", False))
    assert sorted(maps) == sorted(SIZES)
    return maps


def host_objects(labels, probs, channel, min_area, min_confidence):
    """The host chain of one image -> (selected labels, codes, table)."""
    out, n, sums, boxes = M.measure_select(labels, probs, channel, min_area, min_confidence)
    from segmentation_pipeline.impl.rle import rle_encode
    return out, [rle_encode(out == k) for k in range(1, n + 1)], M.table(sums, boxes, n)


def pick_confidence(labels, maps, channel=0):
    """The first candidate that drops an object in some image and keeps one."""
    conf = np.concatenate([M.table(*M.measure(labels[k], int(labels[k].max()), maps[k], channel)[:2], int(labels[k].max()))["confidence"]
                           for k in sorted(labels)])
    assert len(conf) >= 2
    for q in CONF_QUANTILES:
        c = round(float(np.quantile(conf, q)), 4)
        kept = [M.measure_select(labels[k], maps[k], channel, 0, c)[1] for k in sorted(labels)]
        total = [int(labels[k].max()) for k in sorted(labels)]
        print("quantile %g, min_confidence %.4f: kept %s of %s objects" % (q, c, kept, total))
        if 0 <= c <= 1 and sum(kept) >= 1 and any(a < b for a, b in zip(kept, total)):
            return c
    raise AssertionError("no candidate min_confidence drops an object and keeps one")


def same_table(got, want):
    assert tuple(got) == M.COLUMNS
    for c in M.COLUMNS:
        assert got[c].dtype == want[c].dtype and np.array_equal(got[c], want[c]), c
    return True


@pytest.fixture(scope="module")
def exp(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("measure_sigmoid"), 1, "sigmoid", "binary_crossentropy")
    e.kw = {"fold": [0, 1], "stage": 0, "ttflips": True}
    e.maps = maps_of(e, **e.kw)
    e.thr = float(np.quantile(np.concatenate([m.reshape(-1) for m in e.maps.values()]), MASK_QUANTILE))
    e.labels = {s: dict(e.cfg.predict_instances(e.images, threshold=e.thr, rle=False, split=s, **e.kw)) for s in (0, SPLIT)}
    e.conf = pick_confidence(e.labels[SPLIT], e.maps)
    # the scored side: fold 0 alone, no flips - what score_instances runs; the items' masks come from the model's own maps
    e.maps0 = maps_of(e, fold=0)
    values = np.concatenate([m.reshape(-1) for m in e.maps0.values()])
    e.q0 = lambda q: float(np.quantile(values, q))                   # noqa: E731
    e.thr0 = e.q0(MASK_QUANTILE)
    e.truth = {k: CR.remove_small_objects(m[:, :, 0] > e.q0(0.5), 6) for k, m in e.maps0.items()}
    e.truth_labels = {k: OM.label8(m)[0] for k, m in e.truth.items()}
    e.ds = ListDataSet(e.images, e.truth)
    e.ids = [e.ds[int(i)].id for i in e.cfg.kfold(e.ds, range(0, len(e.ds))).sampledIndexes(0, False, "real")]
    assert len(e.ids) >= 2
    e.labels0 = {s: dict(e.cfg.predict_instances(e.images, fold=0, stage=0, threshold=e.thr0, rle=False, split=s)) for s in (0, SPLIT)}
    e.conf0 = pick_confidence({k: e.labels0[SPLIT][k] for k in e.ids}, e.maps0)
    yield e
    torch.cuda.synchronize()


def host_counts(e, split, min_area, min_confidence):
    """int64 [images, T + 3]: the selected reference objects of fold 0's label images against the truth's labels."""
    return np.stack([OM.label_match(M.measure_select(e.labels0[split][i], e.maps0[i], 0, min_area, min_confidence)[0], e.truth_labels[i],
                                    e.truth_labels[i].size, NUMS, DEN) for i in e.ids])


def test_defaults_are_predict_instances(exp):
    for kw in ({}, {"split": SPLIT, "min_size": 4}):
        want = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, **kw, **exp.kw))
        assert dict(exp.cfg.predict_instances_ex(exp.images, threshold=exp.thr, **kw, **exp.kw)) == want
        want = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, rle=False, **kw, **exp.kw))
        got = dict(exp.cfg.predict_instances_ex(exp.images, threshold=exp.thr, rle=False, **kw, **exp.kw))
        assert sorted(got) == sorted(SIZES) and all(got[k].dtype == np.int32 and got[k].tobytes() == want[k].tobytes() for k in SIZES)


def test_the_table_equals_the_reference(exp):
    objects = 0
    for split in (0, SPLIT):
        rows = list(exp.cfg.predict_instances_ex(exp.images, threshold=exp.thr, rle=False, split=split, measure=True, **exp.kw))
        assert sorted(r[0] for r in rows) == sorted(SIZES) and all(len(r) == 3 for r in rows)
        for name, labels, table in rows:
            assert np.array_equal(labels, exp.labels[split][name])
            _, _, want = host_objects(exp.labels[split][name], exp.maps[name], 0, 0, 0.0)
            assert same_table(table, want), (name, split)
            objects += len(table["label"])
        codes = {name: (c, t) for name, c, t in exp.cfg.predict_instances_ex(exp.images, threshold=exp.thr, split=split, measure=True, **exp.kw)}
        plain = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, split=split, **exp.kw))
        assert {k: v[0] for k, v in codes.items()} == plain and all(len(v[0]) == len(v[1]["area"]) for v in codes.values())
    assert objects > 2 * len(SIZES)
    again = list(exp.cfg.predict_instances_ex(exp.images, threshold=exp.thr, rle=False, split=SPLIT, measure=True, **exp.kw))
    assert all(a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and all(a[2][c].tobytes() == b[2][c].tobytes() for c in M.COLUMNS)
               for a, b in zip(rows, again))


def test_the_selection_equals_the_reference(exp):
    dropped = kept = 0
    for split in (0, SPLIT):
        for min_area, conf in ((MIN_AREA, 0.0), (0, exp.conf), (MIN_AREA, exp.conf)):
            kw = dict(threshold=exp.thr, split=split, min_area=min_area, min_confidence=conf, **exp.kw)
            labels = {n: (l, t) for n, l, t in exp.cfg.predict_instances_ex(exp.images, rle=False, measure=True, **kw)}
            codes = dict(exp.cfg.predict_instances_ex(exp.images, **kw))
            assert sorted(labels) == sorted(codes) == sorted(SIZES)
            for name in SIZES:
                want = host_objects(exp.labels[split][name], exp.maps[name], 0, min_area, conf)
                assert labels[name][0].dtype == np.int32 and np.array_equal(labels[name][0], want[0]), (name, split, min_area, conf)
                assert codes[name] == want[1] and same_table(labels[name][1], want[2]), (name, split, min_area, conf)
                dropped += int(exp.labels[split][name].max()) - len(want[1])
                kept += len(want[1])
    assert dropped >= 2 and kept >= 2


def test_the_csv_has_the_measures(exp):
    kw = dict(threshold=exp.thr, split=SPLIT, min_area=MIN_AREA, min_confidence=exp.conf, **exp.kw)
    path = str(exp.root / "measured.csv")
    n = exp.cfg.predict_instances_to_csv_ex(exp.images, path, measures=MEASURES, **kw)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    want = [["image", "rle_mask"] + list(MEASURES)]
    for name in sorted(SIZES):
        _, codes, t = host_objects(exp.labels[SPLIT][name], exp.maps[name], 0, MIN_AREA, exp.conf)
        for k, code in enumerate(codes):
            want.append([name[:name.index(".")], code] + [repr(float(t[m][k])) if t[m].dtype == np.float64 else str(int(t[m][k])) for m in MEASURES])
        if not codes:
            want.append([name[:name.index(".")]] + [""] * (1 + len(MEASURES)))
    assert rows == want and n == len(want) - 1 and n >= len(SIZES)
    assert any("." in r[3] for r in rows[1:] if r[1]) and all("." not in r[2] for r in rows[1:])      # floats with repr, integers as integers
    path = str(exp.root / "plain.csv")                                    # no measures: predict_instances_to_csv's file
    n = exp.cfg.predict_instances_to_csv_ex(exp.images, path, threshold=exp.thr, split=SPLIT, **exp.kw)
    other = str(exp.root / "plain_want.csv")
    assert n == exp.cfg.predict_instances_to_csv(exp.images, other, threshold=exp.thr, split=SPLIT, **exp.kw)
    with open(path) as a, open(other) as b:
        assert a.read() == b.read()
    path = str(exp.root / "empty.csv")
    n = exp.cfg.predict_instances_to_csv_ex(exp.images, path, threshold=1.0, limit=2, columns=("id", "code"), measures=("area", "cy"), **exp.kw)
    with open(path, newline="") as f:
        assert list(csv.reader(f)) == [["id", "code", "area", "cy"], ["a", "", "", ""], ["b", "", "", ""]] and n == 2


def test_score_instances_ex_equals_the_host_chain(exp):
    thr = exp.thr0
    plain = exp.cfg.score_instances(exp.ds, 0, threshold=thr, min_size=4, split=SPLIT)
    same = exp.cfg.score_instances_ex(exp.ds, 0, threshold=thr, min_size=4, split=SPLIT)      # neutral: score_instances' counters
    assert np.array_equal(same["counts"], plain["counts"]) and same["score"] == plain["score"] and same["images"] == plain["images"]
    differs = False
    for split in (0, SPLIT):
        neutral = host_counts(exp, split, 0, 0.0)
        assert np.array_equal(exp.cfg.score_instances_ex(exp.ds, 0, threshold=thr, split=split)["counts"], neutral)
        for min_area, conf in ((MIN_AREA, 0.0), (0, exp.conf0), (MIN_AREA, exp.conf0)):
            want = host_counts(exp, split, min_area, conf)
            print(split, min_area, conf, "reference counters (TP per t, n_pred, n_truth, outside):", want.tolist())
            differs |= not np.array_equal(want, neutral)
            for metric in ("f2", "ap"):
                got = exp.cfg.score_instances_ex(exp.ds, 0, threshold=thr, metric=metric, split=split, min_area=min_area, min_confidence=conf)
                per = OM.object_score(metric, want[:, :10], want[:, 10:11], want[:, 11:12])
                assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want)
                assert got["score"] == float(per.mean(axis=1).mean())
                assert list(got["by_iou"]) == TS and [got["by_iou"][t] for t in TS] == per.mean(axis=0).tolist()
                assert got["images"] == [(i, float(v)) for i, v in zip(exp.ids, per.mean(axis=1))]
    assert differs                                           # the selection changes the counters


def test_find_confidence_equals_per_cell_score_instances_ex(exp):
    thresholds = sorted([exp.thr0, exp.q0(0.2)])
    confidences = sorted({0.0, exp.conf0, round(min(exp.conf0 + 0.01, 1.0), 4)})
    assert len(confidences) == 3
    for metric in ("f2", "ap"):
        best, table = exp.cfg.find_confidence(exp.ds, 0, thresholds=thresholds, confidences=confidences, split=SPLIT, min_area=MIN_AREA,
                                              metric=metric)
        cells = [(t, c) for t in thresholds for c in confidences]
        assert list(table) == cells
        want = [exp.cfg.score_instances_ex(exp.ds, 0, threshold=t, metric=metric, split=SPLIT, min_area=MIN_AREA, min_confidence=c)["score"]
                for t, c in cells]
        assert [table[c] for c in cells] == want
        assert best == cells[int(np.argmax(want))]           # the first argmax
    again = exp.cfg.find_confidence(exp.ds, 0, thresholds=thresholds, confidences=confidences, split=SPLIT, min_area=MIN_AREA, metric="ap")
    assert again == (best, table)
    best, table = exp.cfg.find_confidence(exp.ds, 0, thresholds=[thresholds[1]], confidences=(exp.conf0,), opening=1, closing=1, area_threshold=6)
    got = exp.cfg.score_instances_ex(exp.ds, 0, threshold=thresholds[1], opening=1, closing=1, area_threshold=6, min_confidence=exp.conf0)["score"]
    assert table == {(thresholds[1], exp.conf0): got} and best == (thresholds[1], exp.conf0)


def test_a_fold_list_and_flips_each_work_once(exp):
    for kw in ({"fold": [0, 1], "stage": 0}, {"fold": 1, "stage": 0, "ttflips": True}):
        maps = maps_of(exp, **kw)
        plain = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, rle=False, split=SPLIT, **kw))
        for name, labels, table in exp.cfg.predict_instances_ex(exp.images, threshold=exp.thr, rle=False, split=SPLIT, min_area=MIN_AREA,
                                                                 min_confidence=exp.conf, measure=True, **kw):
            want = host_objects(plain[name], maps[name], 0, MIN_AREA, exp.conf)
            assert np.array_equal(labels, want[0]) and same_table(table, want[2]), (name, kw)


def test_measure_labels_equals_the_reference():
    from scipy import ndimage
    from segmentation_pipeline.segmentation import PipelineConfig
    f = ndimage.gaussian_filter(np.random.default_rng(70133).random((70, 133)), 2.0)
    f = ((f - f.min()) / (f.max() - f.min())).astype(np.float32)
    labels, n = OM.label8(f > 0.5)
    labels[labels == 2] = 0                                  # a value that does not occur: area 0, NaN centroid
    probs3 = np.stack([1 - f, f, f * f], axis=2)
    for lab in (labels, labels.astype(np.int64), labels.astype(np.uint16)):
        for probs, channel in ((None, 0), (f, 0), (probs3, 1), (probs3.astype(np.float64), 2)):
            got = PipelineConfig.measure_labels(lab, probs, channel)
            sums, boxes, outside = M.measure(labels, n, None if probs is None else np.asarray(probs, np.float32), channel)
            want = M.table(sums, boxes, n)
            assert got.pop("out_of_range") == outside == 0 and tuple(got) == M.COLUMNS
            for c in M.COLUMNS:
                assert got[c].dtype == want[c].dtype and np.array_equal(got[c], want[c], equal_nan=True), c
            assert got["area"][1] == 0 and np.isnan(got["cy"][1]) and (got["y0"][1], got["y1"][1]) == (70, 0)
    assert n >= 4 and PipelineConfig.measure_labels(np.zeros((3, 4), np.uint8))["label"].tolist() == []
    torch.cuda.synchronize()


def test_softmax_head_measures_a_channel(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("measure_softmax"), 3, "softmax", "categorical_crossentropy")
    kw = {"fold": [0, 1], "stage": 0, "ttflips": True}
    maps = maps_of(e, **kw)
    plain = dict(e.cfg.predict_instances(e.images, channel=1, rle=False, split=SPLIT, **kw))
    conf = pick_confidence(plain, maps, 1)
    for name, labels, table in e.cfg.predict_instances_ex(e.images, channel=1, rle=False, split=SPLIT, min_area=2, min_confidence=conf,
                                                           measure=True, **kw):
        want = host_objects(plain[name], maps[name], 1, 2, conf)
        assert np.array_equal(labels, want[0]) and same_table(table, want[2]), name
    masks = dict(e.cfg.predict_masks(e.images, fold=0, stage=0, channel=1, rle=False))
    truth = {k: CR.remove_small_objects(m, 4) for k, m in masks.items()}
    ds = ListDataSet(e.images, truth)
    e.ids = [ds[int(i)].id for i in e.cfg.kfold(ds, range(0, len(ds))).sampledIndexes(0, False, "real")]
    e.maps0 = maps_of(e, fold=0)
    e.labels0 = {SPLIT: dict(e.cfg.predict_instances(e.images, fold=0, stage=0, channel=1, rle=False, split=SPLIT))}
    e.truth_labels = {k: OM.label8(m)[0] for k, m in truth.items()}
    conf0 = pick_confidence({k: e.labels0[SPLIT][k] for k in e.ids}, e.maps0, 1)
    want = np.stack([OM.label_match(M.measure_select(e.labels0[SPLIT][i], e.maps0[i], 1, 2, conf0)[0], e.truth_labels[i],
                                    e.truth_labels[i].size, NUMS, DEN) for i in e.ids])
    got = e.cfg.score_instances_ex(ds, 0, channel=1, split=SPLIT, min_area=2, min_confidence=conf0)
    assert np.array_equal(got["counts"], want)
    best, table = e.cfg.find_confidence(ds, 0, channel=1, split=SPLIT, min_area=2, confidences=(0.0, conf0))
    assert list(table) == [(0.5, 0.0), (0.5, conf0)] and table[(0.5, conf0)] == got["score"] and best[0] == 0.5
    with pytest.raises(ValueError):
        e.cfg.find_confidence(ds, 0, channel=1, thresholds=[0.4])
    torch.cuda.synchronize()
