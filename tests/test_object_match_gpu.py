"""GPU tests of the object-score methods of ``PipelineConfig`` (segmentation_pipeline/segmentation.py over csrc/object_match.hip):
``score_objects`` and ``find_object_threshold`` against the host chain they replace - the ``rle=False`` masks of ``predict_masks_ex``,
``scipy.ndimage.label`` with the 8-neighbourhood and the integer statement of tests/_object_match_reference.py - by array equality, and
their scores against ``object_score`` of those counters by ``==``.

An untrained U-Net/resnet18 at 64 x 64, batch 2, saved as the models of two folds, and six images of differing sizes with masks: fold 0
validates on three of them (two batches).  An untrained model's masks are salt and pepper, so each item's mask is derived from the
model's own map - ``remove_small_objects(map > quantile, 6)`` - and the scored masks, at lower quantiles, overlap it without equalling
it: that the reference's own counters hold an image and a t with 0 < TP < n_truth is asserted."""
import os
import types

import numpy as np
import pytest
import torch
import yaml

import _components_reference as CR
import _object_match_reference as R

pytestmark = pytest.mark.gpu

SIZES = {"a.png": (50, 70), "b.png": (64, 64), "c.png": (37, 53), "d.png": (70, 133), "e.png": (64, 64), "f.png": (45, 45)}
Q_TRUTH, Q_SCORED, Q_SWEEP = 0.8, 0.7, (0.6, 0.7, 0.78)            # quantiles of the maps: the items' masks, the scored masks, the sweep
MIN_SIZES = (0, 4, 9)
NUMS, DEN = list(range(500, 1000, 50)), 1000
TS = [n / DEN for n in NUMS]


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
    """The images of a directory with masks (or label images) held in memory: ``y`` [h, w, 1]."""

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


def validation_ids(e, ds):
    return [ds[int(i)].id for i in e.cfg.kfold(ds, range(0, len(ds))).sampledIndexes(0, False, "real")]


def host_counts(e, truth_labels, ids, channel=0, **mask_kw):
    """The host chain: predict_masks_ex(rle=False) masks -> scipy.ndimage.label (8-neighbourhood) -> the reference; int64 [images, T + 3]."""
    masks = dict(e.cfg.predict_masks_ex(e.images, fold=0, stage=0, rle=False, channel=channel, **mask_kw))
    return np.stack([R.label_match(R.label8(masks[i])[0], truth_labels[i], masks[i].size, NUMS, DEN) for i in ids])


def check_scores(result, counts, ids, metric):
    per = R.object_score(metric, counts[:, :10], counts[:, 10:11], counts[:, 11:12])
    assert np.array_equal(result["counts"], counts) and result["counts"].dtype == np.int64
    assert result["score"] == float(per.mean(axis=1).mean())
    assert list(result["by_iou"]) == TS and [result["by_iou"][t] for t in TS] == per.mean(axis=0).tolist()
    assert result["images"] == [(i, float(v)) for i, v in zip(ids, per.mean(axis=1))]


@pytest.fixture(scope="module")
def exp(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("objects_sigmoid"), 1, "sigmoid", "binary_crossentropy")
    maps = {}
    e.cfg.predict_in_directory(e.images, 0, 0, lambda name, mp, data: data.__setitem__(name, mp.arr[:, :, 0]), maps)
    assert sorted(maps) == sorted(SIZES)
    values = np.concatenate([m.reshape(-1) for m in maps.values()])
    e.q = lambda q: float(np.quantile(values, q))                    # noqa: E731
    e.truth = {k: CR.remove_small_objects(m > e.q(Q_TRUTH), 6) for k, m in maps.items()}
    e.truth_labels = {k: R.label8(m)[0] for k, m in e.truth.items()}
    e.ds = ListDataSet(e.images, e.truth)
    e.ids = validation_ids(e, e.ds)
    assert len(e.ids) == 3
    yield e
    torch.cuda.synchronize()


def test_score_objects_equals_the_host_chain(exp):
    thr = exp.q(Q_SCORED)
    partial = False
    for kw in ({"min_size": 0}, {"min_size": 9}, {"min_size": 4, "opening": 1, "closing": 1}, {"min_size": 0, "area_threshold": 6}):
        want = host_counts(exp, exp.truth_labels, exp.ids, threshold=thr, **kw)
        print(kw, "reference counters (TP per t, n_pred, n_truth, outside):", want.tolist())
        partial |= bool(((want[:, :10] > 0) & (want[:, :10] < want[:, 11:12])).any())
        for metric in ("f2", "ap"):
            got = exp.cfg.score_objects(exp.ds, 0, threshold=thr, metric=metric, **kw)
            check_scores(got, want, exp.ids, metric)
    assert partial                                           # an image and a t with 0 < TP < n_truth: no run of only zeros or ones
    f2 = exp.cfg.score_objects(exp.ds, 0, threshold=thr)["score"]
    ap = exp.cfg.score_objects(exp.ds, 0, threshold=thr, metric="ap")["score"]
    assert f2 != ap
    few = exp.cfg.score_objects(exp.ds, 0, threshold=thr, iou_thresholds=[0.5, 0.725, 1])
    assert list(few["by_iou"]) == [0.5, 0.725, 1.0] and few["counts"].shape == (3, 6) and (few["counts"][:, 2] == 0).all()
    assert np.array_equal(few["counts"][:, 0], host_counts(exp, exp.truth_labels, exp.ids, threshold=thr)[:, 0])


def test_truth_labels_keep_touching_objects_apart(exp):
    """``truth="labels"``: the items carry a label image - here the 4-connected components, more of them than the 8-connected ones the
    mask form finds."""
    labels4 = {k: CR.label(m, 1)[0] for k, m in exp.truth.items()}
    assert sum(int(v.max()) for v in labels4.values()) > sum(int(v.max()) for v in exp.truth_labels.values())
    ds = ListDataSet(exp.images, labels4)
    thr = exp.q(Q_SCORED)
    want = host_counts(exp, labels4, exp.ids, threshold=thr, min_size=4)
    assert not np.array_equal(want, host_counts(exp, exp.truth_labels, exp.ids, threshold=thr, min_size=4))
    check_scores(exp.cfg.score_objects(ds, 0, threshold=thr, min_size=4, truth="labels"), want, exp.ids, "f2")
    with pytest.raises(ValueError, match="labels"):
        exp.cfg.score_objects(ListDataSet(exp.images, {k: v.astype(np.float32) for k, v in labels4.items()}), 0, truth="labels")


def test_find_object_threshold_equals_nine_score_objects_calls(exp):
    thresholds = [exp.q(q) for q in Q_SWEEP]
    for metric in ("f2", "ap"):
        best, table = exp.cfg.find_object_threshold(exp.ds, 0, thresholds=thresholds, min_sizes=MIN_SIZES, metric=metric)
        cells = [(t, m) for t in thresholds for m in MIN_SIZES]
        assert list(table) == cells
        want = [exp.cfg.score_objects(exp.ds, 0, threshold=t, min_size=m, metric=metric)["score"] for t, m in cells]
        assert [table[c] for c in cells] == want
        assert best == cells[int(np.argmax(want))] and len(set(want)) > 1      # the first argmax; the grid moves the score
    best, table = exp.cfg.find_object_threshold(exp.ds, 0, thresholds=[thresholds[1]], opening=1, closing=1, area_threshold=6)
    got = exp.cfg.score_objects(exp.ds, 0, threshold=thresholds[1], opening=1, closing=1, area_threshold=6)["score"]
    assert table == {(thresholds[1], 0): got} and best == (thresholds[1], 0)


def test_softmax_head_scores_a_channel(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("objects_softmax"), 3, "softmax", "categorical_crossentropy")
    plain = dict(e.cfg.predict_masks(e.images, fold=0, stage=0, channel=1, rle=False))
    truth = {k: CR.remove_small_objects(m, 4) for k, m in plain.items()}
    assert any(0 < int(t.sum()) < int(plain[k].sum()) for k, t in truth.items())
    labels = {k: R.label8(m)[0] for k, m in truth.items()}
    ds = ListDataSet(e.images, truth)
    ids = validation_ids(e, ds)
    for m in (0, 3):
        want = host_counts(e, labels, ids, channel=1, min_size=m)
        print("softmax channel 1, min_size %d:" % m, want.tolist())
        check_scores(e.cfg.score_objects(ds, 0, channel=1, min_size=m), want, ids, "f2")
    best, table = e.cfg.find_object_threshold(ds, 0, channel=1, min_sizes=(0, 3, 4))
    assert list(table) == [(0.5, 0), (0.5, 3), (0.5, 4)] and best[0] == 0.5
    assert [table[c] for c in table] == [e.cfg.score_objects(ds, 0, channel=1, min_size=m)["score"] for m in (0, 3, 4)]
    with pytest.raises(ValueError):
        e.cfg.find_object_threshold(ds, 0, channel=1, thresholds=[0.4])
    torch.cuda.synchronize()
