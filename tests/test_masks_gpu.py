"""GPU tests of the mask methods of ``PipelineConfig`` (segmentation_pipeline/segmentation.py over csrc/mask.hip): ``predict_masks``,
``predict_to_csv`` and ``find_threshold`` against the host chains they replace - ``predict_in_directory`` / ``evaluateAll`` maps, numpy's
``>``, scipy's ``binary_opening``, ``impl.rle.rle_encode`` and the float64 scores of tests/_mask_reference.py - by string and array
equality.

An untrained U-Net/resnet18 at 64 x 64, batch 2, saved as the models of two folds; a directory of four images of differing sizes (two
batches), a ``crops: 2`` directory and a six-item dataset with masks.  An untrained model's probabilities sit close together, so the
thresholds are taken from the host maps themselves (their median, their quantiles): the masks have both values, and that is asserted."""
import csv
import os
import types

import numpy as np
import pytest
import torch
import yaml

import _mask_reference as R

pytestmark = pytest.mark.gpu

SIZES = {"a.x.png": (50, 70), "b.png": (64, 64), "c.png": (37, 53), "d.png": (70, 133)}      # (h, w); "a.x.png" -> image column "a"
BIG = {"e.png": (100, 90), "f.png": (77, 120)}
DATASET = [(50, 70), (64, 64), (37, 53), (70, 133), (64, 64), (45, 45)]


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
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": classes, "activation": activation, "encoder_weights": None,
            "shape": [64, 64, 3], "batch": 2, "dtype": "fp32", "loss": loss, "folds_count": 2, "stages": [{"epochs": 1}]}
    cfgs = {}
    for name, extra in (("config", {}), ("crops", {"crops": 2, "shape": [128, 128, 3]})):      # crops: 2 -> the same 64 x 64 network
        with open(str(root / (name + ".yaml")), "w") as f:
            yaml.safe_dump(dict(base, **extra), f)
        cfgs[name] = segmentation.parse(str(root / (name + ".yaml")))
    cfg = cfgs["config"]
    net = cfg.createNet1(True)
    net.compile(loss=loss, batch=2, dtype="fp32")
    for fold, seed in ((0, 11), (1, 23)):
        net.impl.init_weights(seed)
        w = net.impl.get_weights()
        net.impl.set_weights({k: np.full_like(v, 0.7) for k, v in w.items() if k.endswith("/gamma")})     # (keeps the logits of a deep random net small)
        net.impl.save_weights(cfg.weightsPath(fold, 0))
    del net
    cfg.load_model = _memo(cfg.load_model)
    cfgs["crops"].load_model = cfg.load_model
    rng = np.random.RandomState(5)
    dirs = {}
    for d, sizes in (("images", SIZES), ("big", BIG)):
        os.makedirs(str(root / d))
        for name, (h, w) in sizes.items():
            Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(str(root / d / name))
        dirs[d] = str(root / d)
    return types.SimpleNamespace(cfg=cfg, crops=cfgs["crops"], dirs=dirs, root=root)


@pytest.fixture(scope="module")
def exp(tmp_path_factory):
    e = experiment(tmp_path_factory.mktemp("masks_sigmoid"), 1, "sigmoid", "binary_crossentropy")
    yield e
    torch.cuda.synchronize()


def host_maps(cfg, path, fold, ttflips):
    seen = {}
    cfg.predict_in_directory(path, fold, 0, lambda name, mp, data: data.__setitem__(name, mp.arr), seen, ttflips=ttflips)
    return seen


def host_chain(arr, thr, r):
    """README.md:498-525 with a disk opening as its clean-up: numpy's `>` on the float32 map, scipy's opening, rle_encode."""
    from scipy.ndimage import binary_opening
    mask = arr[:, :, 0] > thr
    if r:
        mask = binary_opening(mask, R.disk(r))
    return mask, R.rle_encode(mask)


CASES = {"plain": ("cfg", "images", 0, False), "ttflips": ("cfg", "images", 0, True), "folds": ("cfg", "images", [0, 1], False),
         "crops": ("crops", "big", [0, 1], True)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_predict_masks_equals_the_host_chain(exp, case):
    which, d, fold, ttflips = CASES[case]
    cfg, path = getattr(exp, which), exp.dirs[d]
    maps = host_maps(cfg, path, fold, ttflips)
    assert sorted(maps) == sorted(SIZES if d == "images" else BIG)
    thr = float(np.median(np.concatenate([m.reshape(-1) for m in maps.values()])))
    codes = dict(cfg.predict_masks(path, fold=fold, stage=0, ttflips=ttflips, threshold=thr, opening=1))
    masks = dict(cfg.predict_masks(path, fold=fold, stage=0, ttflips=ttflips, threshold=thr, opening=1, rle=False))
    assert sorted(codes) == sorted(masks) == sorted(maps)
    both = 0
    for name, arr in maps.items():
        want_mask, want_code = host_chain(arr, thr, 1)
        both += 0 < want_mask.sum() < want_mask.size
        assert masks[name].dtype == np.uint8 and masks[name].shape == arr.shape[:2]
        assert np.array_equal(masks[name], want_mask), name
        assert codes[name] == want_code, name
    print("%s: threshold %.6g, %d of %d opened masks have both values" % (case, thr, both, len(maps)))
    assert both >= 1                                         # an untrained model, a median threshold: two-valued masks
    # no clean-up, and a closing after the opening: the plain threshold and scipy's two defaults
    name = sorted(maps)[-1]
    plain = dict(cfg.predict_masks(path, fold=fold, stage=0, ttflips=ttflips, threshold=thr, limit=len(maps)))
    assert plain[name] == host_chain(maps[name], thr, 0)[1]
    closed = dict(cfg.predict_masks(path, fold=fold, stage=0, ttflips=ttflips, threshold=thr, opening=2, closing=3, rle=False))
    assert np.array_equal(closed[name], R.closing(R.opening(maps[name][:, :, 0] > thr, 2), 3))


def test_predict_masks_limit_and_order(exp):
    got = list(exp.cfg.predict_masks(exp.dirs["images"], limit=3, threshold=0.0))
    assert [n for n, _ in got] == sorted(SIZES)[:3]
    for name, code in got:                                   # every probability of a sigmoid is above 0: one run over the whole image
        h, w = SIZES[name]
        assert code == "1 %d" % (h * w)
    assert [c for _, c in exp.cfg.predict_masks(exp.dirs["images"], limit=2, threshold=1.0)] == ["", ""]


def test_predict_to_csv_equals_the_rows_of_predict_masks(exp):
    maps = host_maps(exp.cfg, exp.dirs["images"], [0, 1], True)
    thr = float(np.median(np.concatenate([m.reshape(-1) for m in maps.values()])))
    path = str(exp.root / "submission.csv")
    n = exp.cfg.predict_to_csv(exp.dirs["images"], path, fold=[0, 1], stage=0, ttflips=True, threshold=thr, opening=1)
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    want = [["image", "rle_mask"]] + [[name[:name.index(".")], host_chain(maps[name], thr, 1)[1]] for name in sorted(maps)]
    assert n == 4 and rows == want and rows[1][0] == "a"
    other = str(exp.root / "other.csv")
    exp.cfg.predict_to_csv(exp.dirs["images"], other, limit=1, threshold=thr, columns=("id", "code"))
    with open(other, newline="") as f:
        assert list(csv.reader(f)) == [["id", "code"], ["a", host_chain(host_maps(exp.cfg, exp.dirs["images"], 0, False)["a.x.png"], thr, 0)[1]]]


@pytest.fixture(scope="module")
def dataset(exp):
    """Six image / mask pairs of differing sizes (one mask empty): fold 0 validates on three of them, two batches."""
    from PIL import Image
    from segmentation_pipeline.impl.datasets import SimplePNGMaskDataSet
    img_dir, msk_dir = str(exp.root / "train"), str(exp.root / "train_mask")
    os.makedirs(img_dir); os.makedirs(msk_dir)
    rng = np.random.RandomState(6)
    for i, (h, w) in enumerate(DATASET):
        yy, xx = np.mgrid[0:h, 0:w]
        m = ((yy - h * rng.uniform(0.3, 0.7)) / (h * 0.3)) ** 2 + ((xx - w * rng.uniform(0.3, 0.7)) / (w * 0.25)) ** 2 <= 1
        if i == 1:
            m[:] = False
        Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(img_dir, "s%02d.png" % i))
        Image.fromarray((m * 255).astype(np.uint8)).save(os.path.join(msk_dir, "s%02d.png" % i))
    return SimplePNGMaskDataSet(img_dir, msk_dir)


@pytest.mark.parametrize("ttflips", [None, True])
def test_find_threshold_equals_the_evaluate_all_loop(exp, dataset, ttflips):
    pairs = []                                               # (float32 h x w x 1 map, h x w x 1 mask) of the fold's validation items
    for b in exp.cfg.evaluateAll(dataset, 0, ttflips=ttflips):
        pairs += [(p.arr, g.arr) for p, g in zip(b.predicted_maps_aug, b.segmentation_maps)]
    assert len(pairs) == 3
    values = np.concatenate([p.reshape(-1) for p, _ in pairs])
    sweeps = {"quantiles": [float(v) for v in np.unique(np.quantile(values, np.linspace(0.05, 0.95, 19)).astype(np.float32))],
              "default": None, "one": [float(np.float32(np.median(values)))]}
    assert len(sweeps["quantiles"]) >= 10
    for name, thresholds in sweeps.items():
        thr = [d / 20 for d in range(1, 20)] if thresholds is None else thresholds
        per_image = [R.threshold_counts(p, g[:, :, 0], thr) for p, g in pairs]
        if name == "quantiles":                              # the sweep moves the counters: no vacuous table
            assert any(c[0, 0] > c[-1, 0] > 0 for c, _ in per_image)
        for metric in R.METRICS:
            for average in ("image", "pixels"):
                want = R.sweep_table(per_image, metric, average)
                best, table = exp.cfg.find_threshold(dataset, 0, ttflips=ttflips, thresholds=thresholds, metric=metric, average=average)
                assert list(table) == thr and [table[t] for t in thr] == want.tolist(), (name, metric, average)
                assert best == thr[int(np.argmax(want))]     # the first threshold wins a tie


def experiment_softmax(root):
    return experiment(root, 3, "softmax", "categorical_crossentropy")


def test_softmax_head_masks_are_the_label_map(tmp_path_factory):
    from PIL import Image
    e = experiment_softmax(tmp_path_factory.mktemp("masks_softmax"))
    dst = str(e.root / "labels")
    e.cfg.predict_to_directory(e.dirs["images"], dst, fold=[0, 1], stage=0, ttflips=True, labelMap=True)
    seen = set()
    for c in (0, 1, 2):
        masks = dict(e.cfg.predict_masks(e.dirs["images"], fold=[0, 1], stage=0, ttflips=True, channel=c, rle=False))
        codes = dict(e.cfg.predict_masks(e.dirs["images"], fold=[0, 1], stage=0, ttflips=True, channel=c))
        for name in SIZES:
            labels = np.asarray(Image.open(os.path.join(dst, name[:name.index(".")] + ".png")))
            assert np.array_equal(masks[name], labels == c), (name, c)
            assert codes[name] == R.rle_encode(labels == c), (name, c)
            seen.update(np.unique(labels).tolist())
    print("labels that occur:", sorted(seen))
    with pytest.raises(ValueError):
        e.cfg.find_threshold(None, 0)
    torch.cuda.synchronize()
