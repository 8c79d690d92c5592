"""GPU tests of the object-splitting methods of ``PipelineConfig`` (segmentation_pipeline/segmentation.py over csrc/split.hip):
``predict_instances``, ``predict_instances_to_csv``, ``score_instances``, ``find_split`` and ``split_labels`` against the host chain they
replace - the ``rle=False`` masks of ``predict_masks_ex``, the restated split of tests/_split_reference.py, ``impl.rle.rle_encode`` and
the pair-histogram statement of tests/_object_match_reference.py - by string and array equality, and scores by ``==``.

The experiment of test_components_gpu.py: an untrained U-Net/resnet18 at 64 x 64, batch 2, saved as the models of two folds, and a
directory of four images of differing sizes.  An untrained model's masks are salt and pepper, so the threshold is a low quantile of the
maps - most pixels are foreground, in blobs joined by necks - chosen on the reference side as the first of a few quantiles at which the
reference's own split gains an object in some image and keeps an object without a core."""
import csv
import os
import types

import numpy as np
import pytest
import torch
import yaml

import _components_reference as CR
import _object_match_reference as OM
import _split_reference as R

pytestmark = pytest.mark.gpu

SIZES = {"a.x.png": (50, 70), "b.png": (64, 64), "c.png": (37, 53), "d.png": (70, 133)}      # (h, w); "a.x.png" -> image column "a"
QUANTILES = (0.3, 0.2, 0.4, 0.1)                                    # candidates for the threshold, in order of preference
SPLIT = 1.5                                                          # c2 = 2: a core pixel has its whole 3 x 3 neighbourhood in the mask
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


def gains_and_coreless(masks, c2):
    """-> (images whose split has more objects than their plain labelling, objects without a core) on the reference side."""
    gains = coreless = 0
    for m in masks:
        nc = R.cores(m, c2)[2]
        n = R.split(m, c2)[1]
        gains += n > CR.label(m, 2)[1]
        coreless += n - nc
    return gains, coreless


def pick_threshold(maps, c2):
    values = np.concatenate([m.reshape(-1) for m in maps.values()])
    for q in QUANTILES:
        thr = float(np.quantile(values, q))
        gains, coreless = gains_and_coreless([m > thr for m in maps.values()], c2)
        print("quantile %g, threshold %.6g: %d image(s) gain an object, %d object(s) without a core" % (q, thr, gains, coreless))
        if gains >= 1 and coreless >= 1:
            return thr
    raise AssertionError("no candidate threshold makes the reference split non-trivial")


@pytest.fixture(scope="module")
def exp(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("split_sigmoid"), 1, "sigmoid", "binary_crossentropy")
    e.c2 = R.c2_of(SPLIT)
    maps = {}
    e.cfg.predict_in_directory(e.images, [0, 1], 0, lambda name, mp, data: data.__setitem__(name, mp.arr[:, :, 0]), maps, ttflips=True)
    assert sorted(maps) == sorted(SIZES)
    e.kw = {"fold": [0, 1], "stage": 0, "ttflips": True}
    e.thr = pick_threshold(maps, e.c2)
    # the scored side: fold 0 alone, no flips - what score_objects runs; the items' masks come from the model's own maps
    maps0 = {}
    e.cfg.predict_in_directory(e.images, 0, 0, lambda name, mp, data: data.__setitem__(name, mp.arr[:, :, 0]), maps0)
    e.thr0 = pick_threshold(maps0, e.c2)
    values = np.concatenate([m.reshape(-1) for m in maps0.values()])
    e.q0 = lambda q: float(np.quantile(values, q))                   # noqa: E731
    e.truth = {k: CR.remove_small_objects(m > e.q0(0.5), 6) for k, m in maps0.items()}
    e.truth_labels = {k: OM.label8(m)[0] for k, m in e.truth.items()}
    e.ds = ListDataSet(e.images, e.truth)
    e.ids = [e.ds[int(i)].id for i in e.cfg.kfold(e.ds, range(0, len(e.ds))).sampledIndexes(0, False, "real")]
    assert len(e.ids) >= 2
    yield e
    torch.cuda.synchronize()


def host_counts(e, ids, truth_labels, c2, channel=0, **mask_kw):
    """The host chain: predict_masks_ex(rle=False) masks -> the reference split -> the pair-histogram statement; int64 [images, T + 3]."""
    masks = dict(e.cfg.predict_masks_ex(e.images, fold=0, stage=0, rle=False, channel=channel, **mask_kw))
    return np.stack([OM.label_match(R.split(masks[i], c2)[0], truth_labels[i], masks[i].size, NUMS, DEN) for i in ids])


def test_split_zero_is_components(exp):
    for kw in ({}, {"min_size": 4, "area_threshold": 4}):
        lists = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, **kw, **exp.kw))
        want = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, components=True, **kw, **exp.kw))
        assert sorted(lists) == sorted(SIZES) and lists == want
        labels = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, rle=False, **kw, **exp.kw))
        want = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, components=True, rle=False, **kw, **exp.kw))
        for name in SIZES:
            assert labels[name].dtype == np.int32 and labels[name].tobytes() == want[name].tobytes(), name
    empty = list(exp.cfg.predict_instances(exp.images, threshold=1.0, limit=2, split=SPLIT, **exp.kw))
    assert [c for _, c in empty] == [[], []]                 # an empty mask has no objects


def test_predict_instances_equals_the_reference_split(exp):
    gained = coreless = 0
    for kw in ({}, {"min_size": 4, "opening": 1}):
        masks = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, rle=False, **kw, **exp.kw))
        labels = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, rle=False, split=SPLIT, **kw, **exp.kw))
        lists = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, split=SPLIT, **kw, **exp.kw))
        assert sorted(labels) == sorted(lists) == sorted(SIZES)
        for name, m in masks.items():
            want, n = R.split(m, exp.c2)
            assert labels[name].dtype == np.int32 and np.array_equal(labels[name], want), (name, kw)
            assert isinstance(lists[name], list) and lists[name] == [CR.rle_encode(want == k) for k in range(1, n + 1)], (name, kw)
        if not kw:
            gained, coreless = gains_and_coreless(masks.values(), exp.c2)
    assert gained >= 1 and coreless >= 1                     # the reference cuts a neck and keeps a thin object
    wide = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, rle=False, split=4, limit=2, **exp.kw))
    masks = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, rle=False, limit=2, **exp.kw))
    for name in wide:
        assert np.array_equal(wide[name], R.split(masks[name], 16)[0]), name


def test_predict_instances_to_csv_writes_one_row_per_object(exp):
    lists = dict(exp.cfg.predict_instances(exp.images, threshold=exp.thr, min_size=4, split=SPLIT, **exp.kw))
    path = str(exp.root / "instances.csv")
    n = exp.cfg.predict_instances_to_csv(exp.images, path, threshold=exp.thr, min_size=4, split=SPLIT, **exp.kw)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    want = [["image", "rle_mask"]] + [[name[:name.index(".")], code] for name in sorted(lists) for code in (lists[name] or [""])]
    assert rows == want and n == len(want) - 1 and n > len(SIZES)
    path = str(exp.root / "empty.csv")
    n = exp.cfg.predict_instances_to_csv(exp.images, path, threshold=1.0, limit=2, columns=("id", "code"), split=SPLIT, **exp.kw)
    with open(path, newline="") as f:
        assert list(csv.reader(f)) == [["id", "code"], ["a", ""], ["b", ""]] and n == 2      # one empty row per image without objects


def test_score_instances_equals_the_host_chain(exp):
    thr = exp.thr0
    plain = exp.cfg.score_objects(exp.ds, 0, threshold=thr, min_size=4)
    same = exp.cfg.score_instances(exp.ds, 0, threshold=thr, min_size=4)                      # split = 0
    assert np.array_equal(same["counts"], plain["counts"]) and same["score"] == plain["score"] and same["images"] == plain["images"]
    differs = False
    for split, kw in ((SPLIT, {}), (SPLIT, {"min_size": 4, "closing": 1}), (2.5, {})):
        want = host_counts(exp, exp.ids, exp.truth_labels, R.c2_of(split), threshold=thr, **kw)
        print(split, kw, "reference counters (TP per t, n_pred, n_truth, outside):", want.tolist())
        for metric in ("f2", "ap"):
            got = exp.cfg.score_instances(exp.ds, 0, threshold=thr, metric=metric, split=split, **kw)
            per = OM.object_score(metric, want[:, :10], want[:, 10:11], want[:, 11:12])
            assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want)
            assert got["score"] == float(per.mean(axis=1).mean())
            assert list(got["by_iou"]) == TS and [got["by_iou"][t] for t in TS] == per.mean(axis=0).tolist()
            assert got["images"] == [(i, float(v)) for i, v in zip(exp.ids, per.mean(axis=1))]
        if not kw:
            differs |= not np.array_equal(want, host_counts(exp, exp.ids, exp.truth_labels, 0, threshold=thr))
    assert differs                                           # the split changes the counters the plain labelling gives
    labels4 = {k: CR.label(m, 1)[0] for k, m in exp.truth.items()}                            # truth="labels": never split, as given
    want = host_counts(exp, exp.ids, labels4, exp.c2, threshold=thr)
    got = exp.cfg.score_instances(ListDataSet(exp.images, labels4), 0, threshold=thr, truth="labels", split=SPLIT)
    assert np.array_equal(got["counts"], want)


def test_find_split_equals_per_cell_score_instances(exp):
    thresholds, splits = [exp.q0(0.25), exp.thr0 if exp.thr0 > exp.q0(0.25) else exp.q0(0.35)], (0, SPLIT, 2.5)
    for metric in ("f2", "ap"):
        best, table = exp.cfg.find_split(exp.ds, 0, thresholds=thresholds, splits=splits, min_size=4, metric=metric)
        cells = [(t, r) for t in thresholds for r in splits]
        assert list(table) == cells
        want = [exp.cfg.score_instances(exp.ds, 0, threshold=t, min_size=4, metric=metric, split=r)["score"] for t, r in cells]
        assert [table[c] for c in cells] == want
        assert best == cells[int(np.argmax(want))] and len(set(want)) > 1      # the first argmax; the grid moves the score
    best, table = exp.cfg.find_split(exp.ds, 0, thresholds=[thresholds[1]], splits=(SPLIT,), opening=1, closing=1, area_threshold=6)
    got = exp.cfg.score_instances(exp.ds, 0, threshold=thresholds[1], opening=1, closing=1, area_threshold=6, split=SPLIT)["score"]
    assert table == {(thresholds[1], SPLIT): got} and best == (thresholds[1], SPLIT)


def test_split_labels_equals_the_reference():
    from segmentation_pipeline.segmentation import PipelineConfig
    f = np.random.default_rng(70133).random((70, 133))
    from scipy import ndimage
    m = ndimage.gaussian_filter(f, 2.0) > 0.5
    for split in (0, 1.5, 2.5, 4):
        want, n = R.split(m, R.c2_of(split))
        for mask in (m, m.astype(np.uint8) * 255, m.astype(np.float32)):
            got, count = PipelineConfig.split_labels(mask, split)
            assert got.dtype == np.int32 and count == n and np.array_equal(got, want), split
    assert len({R.split(m, R.c2_of(s))[1] for s in (0, 1.5, 2.5, 4)}) >= 3
    got, count = PipelineConfig.split_labels(R.two_discs(), 8)
    assert count == 2 and np.bincount(got.ravel())[1:].tolist() == [440, 431]
    torch.cuda.synchronize()


def test_softmax_head_splits_a_channel(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("split_softmax"), 3, "softmax", "categorical_crossentropy")
    kw = {"fold": [0, 1], "stage": 0, "ttflips": True}
    objects = 0
    for c in (0, 1, 2):
        plain = dict(e.cfg.predict_masks(e.images, channel=c, rle=False, **kw))
        labels = dict(e.cfg.predict_instances(e.images, channel=c, rle=False, split=SPLIT, **kw))
        lists = dict(e.cfg.predict_instances(e.images, channel=c, split=SPLIT, closing=1, **kw))
        closed = dict(e.cfg.predict_masks_ex(e.images, channel=c, rle=False, closing=1, **kw))
        for name in SIZES:
            want, n = R.split(plain[name], R.c2_of(SPLIT))
            objects += n
            assert np.array_equal(labels[name], want), (name, c)
            want, n = R.split(closed[name], R.c2_of(SPLIT))
            assert lists[name] == [CR.rle_encode(want == k) for k in range(1, n + 1)], (name, c)
    assert objects >= 3
    plain = dict(e.cfg.predict_masks(e.images, fold=0, stage=0, channel=1, rle=False))
    truth = {k: CR.remove_small_objects(m, 4) for k, m in plain.items()}
    labels = {k: OM.label8(m)[0] for k, m in truth.items()}
    ds = ListDataSet(e.images, truth)
    ids = [ds[int(i)].id for i in e.cfg.kfold(ds, range(0, len(ds))).sampledIndexes(0, False, "real")]
    want = host_counts(e, ids, labels, R.c2_of(SPLIT), channel=1, min_size=3)
    got = e.cfg.score_instances(ds, 0, channel=1, min_size=3, split=SPLIT)
    assert np.array_equal(got["counts"], want)
    best, table = e.cfg.find_split(ds, 0, channel=1, min_size=3, splits=(0, SPLIT))
    assert list(table) == [(0.5, 0), (0.5, SPLIT)] and table[(0.5, SPLIT)] == got["score"] and best[0] == 0.5
    with pytest.raises(ValueError):
        e.cfg.find_split(ds, 0, channel=1, thresholds=[0.4])
    torch.cuda.synchronize()
