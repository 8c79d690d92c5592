"""GPU tests of the connected-component steps of ``PipelineConfig.predict_masks_ex`` / ``predict_to_csv``
(segmentation_pipeline/segmentation.py over csrc/components.hip): ``min_size``, ``area_threshold`` and ``components`` against the host
chain they replace - the ``rle=False`` masks of the same call without the new keywords, skimage's ``remove_small_objects`` /
``remove_small_holes`` restated on scipy (tests/_components_reference.py), ``impl.rle.rle_encode`` / ``multi_rle_encode`` and
``scipy.ndimage.label`` - by string and array equality.

An untrained U-Net/resnet18 at 64 x 64, batch 2, saved as the models of two folds, and a directory of four images of differing sizes.
An untrained model's masks are salt and pepper: the threshold is a quantile of the maps, ``min_size`` and ``area_threshold`` come from
the reference's own component sizes, and that the reference removes an object and fills a hole is asserted."""
import csv
import os
import types

import numpy as np
import pytest
import torch
import yaml

import _components_reference as R

pytestmark = pytest.mark.gpu

SIZES = {"a.x.png": (50, 70), "b.png": (64, 64), "c.png": (37, 53), "d.png": (70, 133)}      # (h, w); "a.x.png" -> image column "a"


def _memo(fn):
    cache = {}

    def load(fold=0, stage=-1):
        if stage < 0:
            stage = 0                                        # (one stage: -1 is stage 0)
        if (fold, stage) not in cache:
            cache[(fold, stage)] = fn(fold, stage)
        return cache[(fold, stage)]
    return load


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


@pytest.fixture(scope="module")
def exp(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("components_sigmoid"), 1, "sigmoid", "binary_crossentropy")
    maps = {}
    e.cfg.predict_in_directory(e.images, [0, 1], 0, lambda name, mp, data: data.__setitem__(name, mp.arr), maps, ttflips=True)
    e.kw = {"fold": [0, 1], "stage": 0, "ttflips": True}
    e.thr = float(np.quantile(np.concatenate([m.reshape(-1) for m in maps.values()]), 0.45))
    e.plain = dict(e.cfg.predict_masks(e.images, threshold=e.thr, rle=False, **e.kw))         # the masks of the call without the new keywords
    assert sorted(e.plain) == sorted(SIZES)
    for name, m in e.plain.items():
        assert np.array_equal(m, maps[name][:, :, 0] > e.thr)
    yield e
    torch.cuda.synchronize()


def sizes_of(masks, invert):
    return np.concatenate([np.bincount(R.label(m, 1, invert)[0].ravel())[1:] for m in masks])


def test_min_size_and_area_threshold_equal_the_host_chain(exp):
    objects, holes = sizes_of(exp.plain.values(), 0), sizes_of(exp.plain.values(), 1)
    m, a = int(np.median(objects)) + 1, int(np.median(holes)) + 1
    print("threshold %.6g: %d objects, %d zero components; min_size %d, area_threshold %d" % (exp.thr, len(objects), len(holes), m, a))
    removed = filled = 0
    for ms, at in ((m, a), (m, 0), (0, a), (64, 64)):
        codes = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, min_size=ms, area_threshold=at, **exp.kw))
        masks = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, rle=False, min_size=ms, area_threshold=at, **exp.kw))
        assert sorted(codes) == sorted(masks) == sorted(SIZES)
        for name, plain in exp.plain.items():
            kept = R.remove_small_objects(plain, ms) if ms else plain
            want = R.remove_small_holes(kept, at) if at else kept
            if (ms, at) == (m, a):
                removed += int(plain.sum()) > int(kept.sum())
                filled += int(want.sum()) > int(kept.sum())
            assert masks[name].dtype == np.uint8 and np.array_equal(masks[name], want), (name, ms, at)
            assert codes[name] == R.rle_encode(want), (name, ms, at)
    assert removed >= 1 and filled >= 1                      # the reference removes an object and fills a hole


def test_cleanup_after_an_opening_and_a_closing(exp):
    name = "d.png"
    got = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, opening=1, closing=1, rle=False, min_size=9, area_threshold=9, **exp.kw))
    from scipy import ndimage
    disk = ndimage.generate_binary_structure(2, 1)           # skimage's disk(1)
    opened = ndimage.binary_closing(ndimage.binary_opening(exp.plain[name] != 0, disk), disk)
    assert np.array_equal(got[name], R.remove_small_holes(R.remove_small_objects(opened, 9), 9))


def test_components_equal_multi_rle_encode_and_scipys_labels(exp):
    lists = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, components=True, **exp.kw))
    labels = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, components=True, rle=False, **exp.kw))
    several = 0
    for name, plain in exp.plain.items():
        want = R.multi_rle(plain)
        several += len(want) >= 2
        assert isinstance(lists[name], list) and lists[name] == want, name
        assert labels[name].dtype == np.int32 and np.array_equal(labels[name], R.label(plain, 2)[0]), name
    assert several >= 1
    cleaned = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, min_size=9, area_threshold=9, components=True, limit=2, **exp.kw))
    for name in sorted(SIZES)[:2]:                           # the objects of the FINAL mask
        assert cleaned[name] == R.multi_rle(R.remove_small_holes(R.remove_small_objects(exp.plain[name], 9), 9)), name
    empty = list(exp.cfg.predict_masks_ex(exp.images, threshold=1.0, components=True, limit=2, **exp.kw))
    assert [c for _, c in empty] == [[], []]                 # an empty mask has no objects


def test_predict_to_csv_writes_one_row_per_component(exp):
    lists = dict(exp.cfg.predict_masks_ex(exp.images, threshold=exp.thr, min_size=4, components=True, **exp.kw))
    path = str(exp.root / "objects.csv")
    n = exp.cfg.predict_to_csv(exp.images, path, threshold=exp.thr, min_size=4, components=True, **exp.kw)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    want = [["image", "rle_mask"]] + [[name[:name.index(".")], code] for name in sorted(lists) for code in (lists[name] or [""])]
    assert rows == want and n == len(want) - 1 and n > len(SIZES)
    path = str(exp.root / "empty.csv")
    n = exp.cfg.predict_to_csv(exp.images, path, threshold=1.0, components=True, limit=2, columns=("id", "code"), **exp.kw)
    with open(path, newline="") as f:
        assert list(csv.reader(f)) == [["id", "code"], ["a", ""], ["b", ""]] and n == 2      # one empty row per image without objects
    path = str(exp.root / "whole.csv")                       # without `components` the rows are the whole-mask codes, as before
    n = exp.cfg.predict_to_csv(exp.images, path, threshold=exp.thr, min_size=4, **exp.kw)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert n == 4 and [r[1] for r in rows[1:]] == [R.rle_encode(R.remove_small_objects(exp.plain[k], 4)) for k in sorted(SIZES)]


def test_softmax_head_cleans_the_argmax_mask(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("components_softmax"), 3, "softmax", "categorical_crossentropy")
    kw = {"fold": [0, 1], "stage": 0, "ttflips": True}
    changed = 0
    for c in (0, 1, 2):
        plain = dict(e.cfg.predict_masks(e.images, channel=c, rle=False, **kw))
        sizes = sizes_of(plain.values(), 0)
        m = int(np.median(sizes)) + 1 if len(sizes) else 2
        masks = dict(e.cfg.predict_masks_ex(e.images, channel=c, rle=False, min_size=m, **kw))
        lists = dict(e.cfg.predict_masks_ex(e.images, channel=c, min_size=m, components=True, **kw))
        for name in SIZES:
            want = R.remove_small_objects(plain[name], m)
            changed += int(want.sum()) < int(plain[name].sum())
            assert np.array_equal(masks[name], want), (name, c)
            assert lists[name] == R.multi_rle(want), (name, c)
    assert changed >= 1
    torch.cuda.synchronize()
