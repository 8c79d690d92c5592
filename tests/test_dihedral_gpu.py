"""GPU tests of dihedral (D4) test-time augmentation on the device path (``ttflips="d4"``: segmentation_pipeline/segmentation.py over
csrc/dihedral.hip): ``predict_device`` with the five new members, ``predict_on_batch_device`` with all eight, the public methods
routed through it (directory prediction, PNG bytes and label maps, component masks, ``crops``, ``windows``) and ``find_tta`` - each
compared by ``np.array_equal`` with the host chain it replaces: numpy transforms and sums around ``model.predict``
(tests/_dihedral_reference.py), ``_scale_back``, ``(x * 255).astype(uint8)``, ``np.argmax``, tests/_window_reference.py.

The experiments are those of tests/test_predict_gpu.py: U-Net/resnet18 at 64 x 64, batch 4, two checkpoints, per head and storage
dtype."""
import os

import numpy as np
import pytest
import torch

import _dihedral_reference as D
import _predict_reference as R
import _window_reference as WR
from test_predict_gpu import CROPS_SIZE, SIZES, exp, images_of  # noqa: F401  (exp: the module's fixture)

pytestmark = pytest.mark.gpu


def d4_maps(e, cfg, path):
    """{file name: float32 h x w x classes}: the host chain, two folds with all eight members."""
    items = images_of(path)
    xs = cfg._resize_to_net(e.models[0].impl, [it.x for it in items])
    probs = cfg.predict_on_batch(e.models, "d4", xs)
    return {it.id: cfg._scale_back(p, *it.x.shape[:2]) for it, p in zip(items, probs)}


@pytest.fixture(scope="module")
def host(exp):
    return d4_maps(exp, exp.cfg, exp.dirs["images"])


def test_predict_device_is_predict_of_the_transformed_batch(exp):
    impl = exp.models[0].impl
    xs = np.random.RandomState(9).randint(0, 256, size=(4, 64, 64, 3)).astype(np.uint8)
    xd = torch.from_numpy(xs).to("cuda")
    for f in (3, 4, 5, 6, 7):
        want = impl.predict(D.apply(xs, f))
        got = impl.predict_device(xd, 4, flip=f)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want), f
    for f in (-1, 8):
        with pytest.raises(ValueError):
            impl.predict_device(xd, 4, flip=f)


@pytest.mark.parametrize("n", [1, 3, 4])
def test_predict_on_batch_device_equals_the_host_loop(exp, n):
    xs = np.random.RandomState(n).randint(0, 256, size=(4, 64, 64, 3)).astype(np.uint8)
    xd = torch.from_numpy(xs).to("cuda")
    host = exp.cfg.predict_on_batch(exp.models, "d4", xs[:n])
    acc, k = exp.cfg.predict_on_batch_device(exp.models, "d4", xd, n)
    assert k == 16 and tuple(acc.shape) == (4, 64, 64, exp.classes) and acc.dtype == torch.float32
    assert host.dtype == np.float32 and np.array_equal(acc[:n].cpu().numpy() / k, host)
    # the loop written out: per model the eight members in ascending order, each map un-transformed, one float32 add each
    want = np.zeros((n, 64, 64, exp.classes), np.float32)
    for m in exp.models:
        for op in D.OPS:
            want += D.invert(m.predict(np.ascontiguousarray(D.apply(xs[:n], op))), op)
    assert np.array_equal(host, want / 16)
    # one model, not in a list
    acc1, k1 = exp.cfg.predict_on_batch_device(exp.models[1], "d4", xd, n)
    assert k1 == 8 and np.array_equal(acc1[:n].cpu().numpy() / k1, exp.cfg.predict_on_batch(exp.models[1], "d4", xs[:n]))
    if n == 3:      # ttflips=True is what it was: six maps, the flips' host loop
        acc3, k3 = exp.cfg.predict_on_batch_device(exp.models, True, xd, n)
        flips = np.zeros((n, 64, 64, exp.classes), np.float32)
        for m in exp.models:
            for f in R.FLIPS:
                flips += R.flip(m.predict(np.ascontiguousarray(R.flip(xs[:n], f))), f)
        assert k3 == 6 and np.array_equal(acc3[:n].cpu().numpy() / k3, flips / 6)
        assert not np.array_equal(flips / 6, host)


def test_predict_in_directory_equals_the_host_chain(exp, host):
    seen = {}
    exp.cfg.predict_in_directory(exp.dirs["images"], [0, 1], 0, lambda name, mp, data: data.__setitem__(name, mp.arr), seen, ttflips="d4")
    assert sorted(seen) == sorted(SIZES)
    for name, (h, w) in SIZES.items():
        assert seen[name].shape == (h, w, exp.classes) and seen[name].dtype == np.float32
        assert np.array_equal(seen[name], host[name]), name


def test_predict_to_directory_writes_the_host_bytes_and_labels(exp, host):
    from PIL import Image
    dst = str(exp.root / "png_d4")
    exp.cfg.predict_to_directory(exp.dirs["images"], dst, fold=[0, 1], stage=0, ttflips="d4")
    multilabel = exp.head == "multilabel3"
    for name in SIZES:
        b = (host[name] * 255).astype(np.uint8)
        for c in (range(3) if multilabel else [0]):
            png = np.asarray(Image.open(os.path.join(dst, "%s_%d.png" % (name[:-4], c) if multilabel else name)))
            assert png.dtype == np.uint8 and np.array_equal(png, b[:, :, c]), (name, c)
    if multilabel:
        return
    labels = str(exp.root / "labels_d4")
    exp.cfg.predict_to_directory(exp.dirs["images"], labels, fold=[0, 1], stage=0, ttflips="d4", labelMap=True)
    for name, (h, w) in SIZES.items():
        png = np.asarray(Image.open(os.path.join(labels, name)))
        want = np.argmax(host[name], axis=2) if exp.classes > 1 else (host[name][:, :, 0] > 0.5)
        assert png.shape == (h, w) and png.dtype == np.uint8 and np.array_equal(png, want), name


def test_component_masks_equal_the_host_chain(exp, host):
    from segmentation_pipeline.impl import rle
    softmax = exp.head == "softmax3"
    thr = 0.5 if softmax else float(np.median(np.concatenate([m[:, :, 0].reshape(-1) for m in host.values()])))
    got = dict(exp.cfg.predict_masks_ex(exp.dirs["images"], fold=[0, 1], stage=0, ttflips="d4", threshold=thr, components=True))
    assert sorted(got) == sorted(SIZES)
    for name, arr in host.items():
        mask = (np.argmax(arr, axis=2) == 0) if softmax else (arr[:, :, 0] > np.float32(thr))
        assert got[name] == rle.multi_rle_encode(mask[:, :, None]), name


def test_crops_cells_equal_the_host_chain(exp):
    seen = {}
    exp.crops.predict_in_directory(exp.dirs["big"], [0, 1], 0, lambda name, mp, data: data.__setitem__(name, mp.arr), seen, ttflips="d4")
    img = images_of(exp.dirs["big"])[0].x
    h, w = img.shape[:2]
    rects = R.cell_rectangles(h, w, 2)
    xs = exp.crops._resize_to_net(exp.models[0].impl, [img[y0:y1, x0:x1] for y0, y1, x0, x1 in rects])
    probs = exp.crops.predict_on_batch(exp.models, "d4", xs)
    want = np.zeros((h, w, exp.classes), np.float32)
    for (y0, y1, x0, x1), p in zip(rects, probs):
        want[y0:y1, x0:x1] = exp.crops._scale_back(p, y1 - y0, x1 - x0)
    assert seen["c.png"].shape == CROPS_SIZE + (exp.classes,) and np.array_equal(seen["c.png"], want)


def test_windows_equal_the_window_statement(exp, monkeypatch):
    """``windows: 16`` on the 100 x 90 image: the statement of tests/_window_reference.py with its per-batch sum replaced by the
    ``"d4"`` host loop (sixteen maps per window)."""
    monkeypatch.setattr(WR, "batch_sum", lambda models, ttflips, xs: D.batch_sum(models, xs))
    img = images_of(exp.dirs["big"])[0].x
    assert exp.cfg.windows is None
    exp.cfg.windows = 16
    try:
        for mode in (WR.PROBS, WR.LABELS):
            want = WR.predict_windows(exp.models, "d4", img, 64, 64, 3, 16, 4, mode)
            got = exp.cfg._predict_windows(exp.models, "d4", img, mode)
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), mode
        seen = {}
        exp.cfg.predict_in_directory(exp.dirs["big"], [0, 1], 0, lambda name, mp, data: data.__setitem__(name, mp.arr), seen, ttflips="d4")
        assert np.array_equal(seen["c.png"], WR.predict_windows(exp.models, "d4", img, 64, 64, 3, 16, 4))
    finally:
        exp.cfg.windows = None


@pytest.fixture(scope="module")
def dataset(exp):
    """Five image / mask pairs of differing sizes (one mask empty)."""
    from PIL import Image
    from segmentation_pipeline.impl.datasets import SimplePNGMaskDataSet
    img_dir, msk_dir = str(exp.root / "train"), str(exp.root / "train_mask")
    os.makedirs(img_dir); os.makedirs(msk_dir)
    rng = np.random.RandomState(6)
    for i, (h, w) in enumerate([(50, 70), (64, 64), (37, 53), (64, 64), (45, 45)]):
        yy, xx = np.mgrid[0:h, 0:w]
        m = ((yy - h * rng.uniform(0.3, 0.7)) / (h * 0.3)) ** 2 + ((xx - w * rng.uniform(0.3, 0.7)) / (w * 0.25)) ** 2 <= 1
        if i == 1:
            m[:] = False
        Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(img_dir, "s%02d.png" % i))
        Image.fromarray((m * 255).astype(np.uint8)).save(os.path.join(msk_dir, "s%02d.png" % i))
    return SimplePNGMaskDataSet(img_dir, msk_dir)


def test_find_tta_equals_three_find_threshold_calls(exp, dataset):
    if exp.head == "softmax3":
        with pytest.raises(ValueError, match="softmax"):
            exp.cfg.find_tta(dataset, 0, stage=0)
        return
    values = np.concatenate([p.arr[:, :, 0].reshape(-1) for b in exp.cfg.evaluateAll(dataset, 0, stage=0, ttflips="d4")
                             for p in b.predicted_maps_aug])
    thr = float(np.float32(np.median(values)))          # an untrained model's maps sit close together: a threshold inside them
    for metric, average in (("dice", "image"), ("iou", "pixels"), ("f2", "image")):
        best, table = exp.cfg.find_tta(dataset, 0, stage=0, threshold=thr, metric=metric, average=average)
        assert list(table) == [False, True, "d4"]
        want = [exp.cfg.find_threshold(dataset, 0, stage=0, ttflips=v, thresholds=[thr], metric=metric, average=average)[1][thr]
                for v in (False, True, "d4")]
        print("%s / %s at %.6g: %r" % (metric, average, thr, want))
        assert [table[v] for v in (False, True, "d4")] == want, (metric, average)
        first = (False, True, "d4")[int(np.argmax(want))]          # the first maximum wins a tie
        assert best == first and type(best) is type(first)
