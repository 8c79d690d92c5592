"""GPU tests of sliding-window prediction (``windows: <overlap>``: segmentation_pipeline/segmentation.py over csrc/window.hip): the
finished maps of ``_predict_windows`` and of the public methods routed through it, compared by ``np.array_equal`` with the host
statement of tests/_window_reference.py - numpy windows, sums and cross-fade around the same models' ``predict``.

One experiment per head (1 class sigmoid, 3 classes softmax) and storage dtype (fp32, bf16): U-Net/resnet18 at 64 x 64, batch 4, two
checkpoints from different seeds, loaded once and shared by the tests.  Images of 150 x 100 (12 windows at overlap 32: three batches,
up to nine windows on a pixel), 64 x 64 (one window) and 40 x 90 (smaller than the window along one axis: edge-replicated).  The
statement's map of every (image, overlap, folds, flips) is computed once and shared."""
import os
import types

import numpy as np
import pytest
import torch
import yaml

import _components_reference as CR
import _window_reference as R

pytestmark = pytest.mark.gpu

HEADS = {"sigmoid1": (1, "sigmoid", "binary_crossentropy"), "softmax3": (3, "softmax", "categorical_crossentropy")}
SIZES = {"a.png": (150, 100), "b.png": (64, 64), "c.png": (40, 90)}
DATASET = [(70, 100), (64, 64), (90, 66), (100, 70), (64, 80), (50, 70)]


def _memo(fn):
    cache = {}

    def load(fold=0, stage=-1):
        if stage < 0:
            stage = 0                                        # (one stage: -1 is stage 0)
        if (fold, stage) not in cache:
            cache[(fold, stage)] = fn(fold, stage)
        return cache[(fold, stage)]
    return load


@pytest.fixture(scope="module", params=[(h, d) for h in HEADS for d in ("fp32", "bf16")], ids=lambda p: "%s-%s" % p)
def exp(request, tmp_path_factory):
    from PIL import Image
    from segmentation_pipeline import segmentation
    head, dtype = request.param
    classes, activation, loss = HEADS[head]
    root = tmp_path_factory.mktemp("window_%s_%s" % (head, dtype))
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": classes, "activation": activation, "encoder_weights": None,
            "shape": [64, 64, 3], "batch": 4, "dtype": dtype, "loss": loss, "folds_count": 2, "stages": [{"epochs": 1}]}
    cfgs = {}
    for name, extra in (("config", {}), ("yaml16", {"windows": 16}), ("crops", {"crops": 2, "shape": [128, 128, 3]})):
        with open(str(root / (name + ".yaml")), "w") as f:
            yaml.safe_dump(dict(base, **extra), f)
        cfgs[name] = segmentation.parse(str(root / (name + ".yaml")))
    cfg = cfgs["config"]
    net = cfg.createNet1(True)
    net.compile(loss=loss, batch=4, dtype=dtype)
    for fold, seed in ((0, 11), (1, 23)):                  # two checkpoints with different seeds
        net.impl.init_weights(seed)
        w = net.impl.get_weights()
        net.impl.set_weights({k: np.full_like(v, 0.7) for k, v in w.items() if k.endswith("/gamma")})     # (keeps the logits of a deep random net small)
        net.impl.save_weights(cfg.weightsPath(fold, 0))
    del net
    load = _memo(cfg.load_model)
    for c in cfgs.values():                                # same directory, same checkpoints, same network shape
        c.load_model = load
    os.makedirs(str(root / "images"))
    rng = np.random.RandomState(5)
    for name, (h, w) in SIZES.items():
        Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(str(root / "images" / name))
    models = [load(0, 0), load(1, 0)]
    e = types.SimpleNamespace(cfg=cfg, yaml16=cfgs["yaml16"], crops=cfgs["crops"], models=models, images=str(root / "images"), root=root,
                              classes=classes, head=head, dtype=dtype, statements={})
    yield e
    cfg.windows = None
    torch.cuda.synchronize()


def images_of(path):
    from segmentation_pipeline.impl.datasets import DirectoryDataSet
    ds = DirectoryDataSet(path)
    return [ds[i] for i in range(len(ds))]


def statement(e, name, img, overlap, folds, ttflips):
    """The host statement's float32 map of one image, computed once per (image, overlap, folds, flips)."""
    key = (name, overlap, folds, bool(ttflips))
    if key not in e.statements:
        e.statements[key] = R.predict_windows(e.models[:folds], ttflips, img, 64, 64, 3, overlap, 4)
    return e.statements[key]


class windows(object):
    """``with windows(cfg, 16):`` - the key set on a parsed config, as ``cfg.gpus`` is, and unset again."""

    def __init__(self, cfg, overlap):
        self.cfg, self.overlap = cfg, overlap

    def __enter__(self):
        self.cfg.windows = self.overlap
        return self.cfg

    def __exit__(self, *exc):
        self.cfg.windows = None
        return False


@pytest.mark.parametrize("ttflips", [False, True])
@pytest.mark.parametrize("folds", [1, 2])
@pytest.mark.parametrize("overlap", [0, 16, 32])
def test_predict_windows_equals_the_statement(exp, overlap, folds, ttflips):
    with windows(exp.cfg, overlap) as cfg:
        for it in images_of(exp.images):
            want = statement(exp, it.id, it.x, overlap, folds, ttflips)
            assert want.shape == SIZES[it.id] + (exp.classes,) and want.dtype == np.float32
            for mode in (cfg.PROBS, cfg.BYTES, cfg.LABELS):
                got = cfg._predict_windows(exp.models[:folds], ttflips, it.x, mode)
                assert np.array_equal(got, R.quantise(want, mode)), (it.id, mode)
            dev = cfg._predict_windows_device(exp.models[:folds], ttflips, it.x)
            assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == want.shape
    a = exp.statements[("a.png", overlap, folds, ttflips)]
    print("statement a.png: min %.3g max %.3g std %.3g" % (a.min(), a.max(), a.std()))
    assert a.std() > 0


def test_one_window_is_the_plain_path(exp):
    """A 64 x 64 image is one window: at overlap 0 every weight is 1 and the map IS the plain path's; at overlap 16 the ramp weight
    is multiplied in and divided out again - one more rounding than the plain path's division: within 2 ulp."""
    it = [i for i in images_of(exp.images) if i.id == "b.png"][0]
    plain = exp.cfg._predict_maps(exp.models, True, [it])[0]
    with windows(exp.cfg, 0) as cfg:
        assert np.array_equal(cfg._predict_maps(exp.models, True, [it])[0], plain)
    with windows(exp.cfg, 16) as cfg:
        got = cfg._predict_maps(exp.models, True, [it])[0]
    ulp = np.spacing(np.maximum(np.abs(plain), np.float32(2.0 ** -126)))
    err = float((np.abs(got.astype(np.float64) - plain.astype(np.float64)) / ulp).max())
    print("one window at overlap 16 against the plain path: max error %.3g ulp" % err)
    assert got.shape == plain.shape and err <= 2.0


def test_directory_methods_equal_the_statement(exp):
    """predict_in_directory's maps, predict_to_directory's PNGs, .npy files and label maps, predict_on_directory's list - with the key
    from the YAML (``windows: 16``), two folds and flips."""
    from PIL import Image
    cfg = exp.yaml16
    assert cfg.windows == 16
    want = {it.id: statement(exp, it.id, it.x, 16, 2, True) for it in images_of(exp.images)}
    seen = {}
    cfg.predict_in_directory(exp.images, [0, 1], 0, lambda name, mp, data: data.__setitem__(name, mp.arr), seen, ttflips=True)
    assert sorted(seen) == sorted(SIZES)
    for name in SIZES:
        assert seen[name].dtype == np.float32 and np.array_equal(seen[name], want[name]), name
    png, npy, lab = str(exp.root / "png"), str(exp.root / "npy"), str(exp.root / "labels")
    cfg.predict_to_directory(exp.images, png, fold=[0, 1], stage=0, ttflips=True)
    cfg.predict_to_directory(exp.images, npy, fold=[0, 1], stage=0, ttflips=True, binaryArray=True)
    cfg.predict_to_directory(exp.images, lab, fold=[0, 1], stage=0, ttflips=True, labelMap=True)
    for name in SIZES:
        assert np.array_equal(np.asarray(Image.open(os.path.join(png, name))), (want[name] * 255).astype(np.uint8)[:, :, 0]), name
        assert np.array_equal(np.load(os.path.join(npy, name[:-4] + ".npy")), want[name]), name
        labels = np.argmax(want[name], axis=2) if exp.classes > 1 else want[name][:, :, 0] > 0.5
        assert np.array_equal(np.asarray(Image.open(os.path.join(lab, name))), labels), name
    batches = list(cfg.predict_on_directory(exp.images, fold=[0, 1], stage=0, ttflips=True))
    assert len(batches) == 1 and isinstance(batches[0][1], list)                      # as under `crops`: the maps at their own sizes
    for it, m in zip(*batches[0]):
        assert np.array_equal(m, want[it.id]), it.id


def test_predict_masks_ex_goes_on_from_the_blended_map(exp):
    """threshold (a softmax head: argmax == channel), remove_small_objects(4), per-object run-length codes - the host chain applied to
    the statement's map."""
    want = {it.id: statement(exp, it.id, it.x, 16, 2, True) for it in images_of(exp.images)}
    if exp.classes > 1:
        t, counts = 0.5, np.bincount(np.argmax(want["a.png"], axis=2).ravel(), minlength=exp.classes)
        channel = int(np.argmin(np.abs(counts - counts.sum() / 2)))
        host = {n: (np.argmax(m, axis=2) == channel) for n, m in want.items()}
    else:
        t, channel = float(np.median(want["a.png"])), 0
        host = {n: m[:, :, 0] > np.float32(t) for n, m in want.items()}
    assert 0 < host["a.png"].sum() < host["a.png"].size                               # the mask has both values
    with windows(exp.cfg, 16) as cfg:
        codes = dict(cfg.predict_masks_ex(exp.images, fold=[0, 1], stage=0, ttflips=True, threshold=t, channel=channel, min_size=4,
                                          components=True))
        masks = dict(cfg.predict_masks_ex(exp.images, fold=[0, 1], stage=0, ttflips=True, threshold=t, channel=channel, min_size=4,
                                          rle=False))
    assert sorted(codes) == sorted(SIZES)
    removed = 0
    for name in SIZES:
        kept = CR.remove_small_objects(host[name], 4)
        removed += int(host[name].sum()) - int(kept.sum())
        assert np.array_equal(masks[name], kept), name
        assert codes[name] == CR.multi_rle(kept), name
    print("threshold %.6g channel %d: %d pixels of small objects removed, %d objects in a.png" % (t, channel, removed, len(codes["a.png"])))


def test_evaluate_all_gives_the_same_maps(exp):
    from PIL import Image
    from segmentation_pipeline.impl.datasets import SimplePNGMaskDataSet
    img_dir, msk_dir = str(exp.root / "train"), str(exp.root / "train_mask")
    os.makedirs(img_dir); os.makedirs(msk_dir)
    rng = np.random.RandomState(6)
    for i, (h, w) in enumerate(DATASET):
        Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(img_dir, "s%02d.png" % i))
        Image.fromarray((rng.randint(0, 2, size=(h, w)) * 255).astype(np.uint8)).save(os.path.join(msk_dir, "s%02d.png" % i))
    ds = SimplePNGMaskDataSet(img_dir, msk_dir)
    n = 0
    with windows(exp.cfg, 16) as cfg:
        for b in cfg.evaluateAll(ds, 0, ttflips=True):
            for img, name, p in zip(b.images, b.data, b.predicted_maps_aug):
                want = R.predict_windows(exp.models[:1], True, img, 64, 64, 3, 16, 4)
                assert p.arr.dtype == np.float32 and np.array_equal(p.arr, want), name
                n += 1
    assert n == 3


def test_windows_together_with_crops_is_refused(exp):
    with windows(exp.crops, 16) as cfg:
        with pytest.raises(ValueError, match="crops"):
            cfg.predict_in_directory(exp.images, [0, 1], 0, lambda *a: None, None)
        with pytest.raises(ValueError, match="crops"):
            cfg._predict_maps(exp.models, False, images_of(exp.images)[:1])
    with windows(exp.cfg, 33) as cfg:
        with pytest.raises(ValueError, match="windows"):
            cfg._predict_maps(exp.models, False, images_of(exp.images)[:1])
