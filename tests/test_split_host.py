"""CPU tests of the object-splitting path's host side (segmentation_pipeline/segmentation.py over csrc/split.hip): the two host
statements of the squared distance transform and the two of the growth (tests/_split_reference.py) agree; a hand case pins the
definition; ties go to the smaller label; every object is 8-connected; the new entry points are bound, refuse bad arguments without a
device and have no CPU fallback; the five public methods have their signatures, and every refusal of theirs fires before a model file
is opened."""
import inspect

import numpy as np
import pytest
from scipy import ndimage

import _split_reference as R


def config(**kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "batch": 4}
    return segmentation.PipelineConfig(**dict(base, **kw))


def small_masks():
    rng = np.random.default_rng(21)
    out = [np.zeros((4, 5), np.uint8), np.ones((4, 5), np.uint8), np.ones((1, 1), np.uint8), R.two_discs()]
    for k in range(40):
        h, w = (int(v) for v in rng.integers(1, 24, 2))
        out.append((rng.random((h, w)) < rng.uniform(0.3, 0.95)).astype(np.uint8))
    for k in range(6):
        f = ndimage.gaussian_filter(np.random.default_rng(k).random((30, 41)), 2.0)
        out.append((f > np.quantile(f, 0.4)).astype(np.uint8))
    return out


def test_the_two_distance_statements_agree():
    seen = 0
    for m in small_masks():
        d2 = R.edt2(m)
        assert d2.dtype == np.int32 and np.array_equal(d2, R.edt2_brute(m))
        if not m.all():                                                  # scipy's float distances round to the same integers
            assert np.array_equal(np.rint(ndimage.distance_transform_edt(m) ** 2).astype(np.int32), d2)
        else:
            assert (d2 == R.NO_BACKGROUND).all() and R.NO_BACKGROUND == 2 ** 31 - 1
        assert (d2[m == 0] == 0).all() and (d2[m != 0] >= 1).all()
        seen = max(seen, int(d2[d2 != R.NO_BACKGROUND].max(initial=0)))
    assert seen >= 100                                                   # distances of 10 pixels and more were compared


def test_the_two_growth_statements_agree():
    rng = np.random.default_rng(22)
    ties = 0
    for m in small_masks():
        seeds = np.where(rng.random(m.shape) < 0.08, rng.integers(1, m.size + 1, m.shape), 0).astype(np.int32)
        got, rounds = R.grow(m, seeds, return_rounds=True)
        assert np.array_equal(got, R.grow_lexicographic(m, seeds))
        assert (got[m == 0] == 0).all() and np.array_equal(got[(seeds != 0) & (m != 0)], seeds[(seeds != 0) & (m != 0)])
        assert np.array_equal(R.grow(m, seeds, max_rounds=rounds), got) and np.array_equal(R.grow(m, got), got)
        ties += rounds >= 2
    assert ties >= 10


def test_the_hand_case_pins_the_definition():
    m = R.two_discs()
    assert m.shape == (40, 64) and int(m.sum()) == 871 and R.label(m, 2)[1] == 1
    labels, n = R.split(m, 64)
    assert n == 2 and np.bincount(labels.ravel())[1:].tolist() == [440, 431]
    assert R.cores(m, 64)[2] == 2 and (labels[:, :31][m[:, :31] != 0] == 1).all() and (labels[:, 32:][m[:, 32:] != 0] == 2).all()
    labels, n = R.split(m, 16)
    assert n == 1 and R.cores(m, 16)[2] == 1 and np.array_equal(labels, m.astype(np.int32))      # the neck is wider than 2 * 4
    labels, n = R.split(m, 169)
    assert n == 1 and R.cores(m, 169)[2] == 0 and np.array_equal(labels, m.astype(np.int32))     # no core: one object all the same
    labels, n = R.split(m, 0)
    want, k = ndimage.label(m, np.ones((3, 3)))
    assert n == k and np.array_equal(labels, want)
    assert [R.c2_of(r) for r in (0, 1.5, 2.5, 4, 8, 13, 1024)] == [0, 2, 6, 16, 64, 169, 1048576]


def test_c2_zero_is_the_plain_labelling():
    for m in small_masks():
        labels, n = R.split(m, 0)
        want, k = ndimage.label(m, np.ones((3, 3)))
        assert n == k and np.array_equal(labels, want)


def test_a_tie_goes_to_the_smaller_label():
    m = np.ones((7, 11), np.uint8)
    seeds = np.zeros((7, 11), np.int32)
    seeds[3, 0], seeds[3, 10] = 77, 5                                    # column 5 is 5 steps from either seed
    for grow in (R.grow, R.grow_lexicographic):
        got = grow(m, seeds)
        assert (got[:, :5] == 77).all() and (got[:, 5:] == 5).all()
    seeds[3, 0], seeds[3, 10] = 5, 77
    for grow in (R.grow, R.grow_lexicographic):
        got = grow(m, seeds)
        assert (got[:, :6] == 5).all() and (got[:, 6:] == 77).all()
    m[:, 5] = 0                                                          # a wall: neither crosses it
    m[6, 5] = 1
    got = R.grow(m, seeds)
    assert got[6, 5] == 5 and (got[:, 6:] == 77).all() and np.array_equal(got, R.grow_lexicographic(m, seeds))


def test_every_object_is_8_connected():
    objects = split_more = 0
    for m in small_masks():
        for c2 in (0, 2, 6, 16):
            labels, n = R.split(m, c2)
            assert labels.dtype == np.int32 and np.array_equal(labels != 0, m != 0)              # the objects partition the mask
            assert sorted(np.unique(labels[labels != 0]).tolist()) == list(range(1, n + 1))
            for k in range(1, n + 1):
                assert R.is_8_connected(labels == k), (c2, k)
            objects += n
            split_more += n > R.label(m, 2)[1]
    assert objects > 500 and split_more >= 10


# ------------------------------------------------------------------------------------------------ the entry points
def test_entry_points_are_bound():
    from segmentation_training_pipeline_amd import _lib, ops
    i32, vp, sz = _lib.i32, _lib.vp, _lib.sz
    assert _lib.SIGNATURES["stp_mask_edt_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_label_grow_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_label_grow_rounds"] == (i32, [])
    assert _lib.SIGNATURES["stp_mask_edt"] == (i32, [vp, i32, i32, vp, vp, sz, vp])
    assert _lib.SIGNATURES["stp_edt_threshold"] == (i32, [vp, i32, i32, i32, vp, vp])
    assert _lib.SIGNATURES["stp_label_grow"] == (i32, [vp, vp, i32, i32, vp, vp, vp, sz, vp])
    assert _lib.SIGNATURES["stp_label_unclaimed"] == (i32, [vp, vp, i32, i32, vp, vp])
    assert _lib.SIGNATURES["stp_label_merge"] == (i32, [vp, vp, vp, i32, i32, vp, vp, vp])
    for name in ("mask_edt", "edt_threshold", "label_grow", "label_unclaimed", "label_merge", "mask_edt_workspace_bytes",
                 "label_grow_workspace_bytes"):
        assert callable(getattr(ops, name))
    for storage in ("bf16", "fp16"):                                     # both builds export the same code; the queries run without a GPU
        lib = _lib.load(storage)
        assert lib.stp_label_grow_rounds() == 32
        edt, grow = lib.stp_mask_edt_workspace_bytes, lib.stp_label_grow_workspace_bytes
        assert edt(1, 1) == 16 and grow(1, 1) == 16 + 128                # uint16 distances; one int32 image and 32 flag words
        assert edt(64, 64) == 8192 and grow(64, 64) == 16384 + 128
        assert edt(37, 53) == 3936 and grow(37, 53) == 7856 + 128        # 1961 pixels, rounded up to 16 bytes
        assert edt(32767, 1) == 65536 and grow(1, 32767) == 131072 + 128
        for query in (edt, grow):
            assert query(0, 5) == 0 and query(5, -1) == 0 and query(32768, 1) == 0 and query(1, 32768) == 0


def test_argument_checks_come_before_any_launch():
    """STP_E_BADARG and STP_E_WORKSPACE need no device: they are returned on a machine without one."""
    from segmentation_training_pipeline_amd import _lib
    lib = _lib.load()
    fake = 4096                                                          # a non-NULL, aligned address that is never dereferenced
    assert lib.stp_mask_edt(None, 4, 4, None, None, 0, None) == -1
    assert lib.stp_mask_edt(fake, 0, 4, fake, fake, 1 << 20, None) == -1 and lib.stp_mask_edt(fake, 4, 32768, fake, fake, 1 << 30, None) == -1
    assert lib.stp_mask_edt(fake, 4, 4, fake, fake + 4, 1 << 20, None) == -1                     # workspace not 8-byte aligned
    assert lib.stp_mask_edt(fake, 4, 4, fake, fake, lib.stp_mask_edt_workspace_bytes(4, 4) - 1, None) == -3
    assert lib.stp_edt_threshold(fake, 4, 4, -1, fake, None) == -1 and lib.stp_edt_threshold(None, 4, 4, 1, fake, None) == -1
    assert lib.stp_edt_threshold(fake, 4, -4, 1, fake, None) == -1
    assert lib.stp_label_grow(fake, fake, 4, 4, fake, None, fake, 1 << 20, None) == -1
    assert lib.stp_label_grow(fake, fake, 32768, 4, fake, fake, fake, 1 << 30, None) == -1
    assert lib.stp_label_grow(fake, fake, 4, 4, fake, fake, fake, lib.stp_label_grow_workspace_bytes(4, 4) - 1, None) == -3
    assert lib.stp_label_unclaimed(fake, None, 4, 4, fake, None) == -1 and lib.stp_label_unclaimed(fake, fake, 0, 4, fake, None) == -1
    assert lib.stp_label_merge(fake, fake, fake + 4, 4, 4, fake + 64, fake, None) == -1          # total is nc
    assert lib.stp_label_merge(fake, fake, fake + 4, 4, 4, fake + 64, fake + 4, None) == -1      # total is nr
    assert lib.stp_label_merge(fake, fake + 4, fake + 8, 4, 4, fake, fake + 12, None) == -1      # rest is labels
    assert lib.stp_label_merge(fake, fake + 4, fake + 8, 0, 4, fake + 64, fake + 12, None) == -1


def test_wrappers_have_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    m = torch.ones((4, 4), dtype=torch.uint8)
    lab = torch.zeros((4, 4), dtype=torch.int32)
    word = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.StpError):
        ops.mask_edt(m, 4, 4, lab, torch.zeros(ops.mask_edt_workspace_bytes(4, 4), dtype=torch.uint8))
    with pytest.raises(_lib.StpError):
        ops.edt_threshold(lab, 4, 4, 2, torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(_lib.StpError):
        ops.label_grow(m, lab, 4, 4, lab, word, torch.zeros(ops.label_grow_workspace_bytes(4, 4), dtype=torch.uint8))
    with pytest.raises(_lib.StpError):
        ops.label_unclaimed(m, lab, 4, 4, torch.zeros((4, 4), dtype=torch.uint8))
    with pytest.raises(_lib.StpError):
        ops.label_merge(lab, word, word.clone(), 4, 4, lab.clone(), word.clone())
    with pytest.raises(ValueError):
        ops.mask_edt(m, 4, 4, lab.to(torch.int64), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(ValueError):
        ops.label_grow(m, lab, 4, 4, lab[:3], word, torch.zeros(256, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the public methods
def test_public_signatures():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    assert list(inspect.signature(P.split_labels).parameters) == ["mask", "split"]
    assert isinstance(inspect.getattr_static(P, "split_labels"), staticmethod)
    p = inspect.signature(P.predict_instances).parameters
    assert list(p) == ["self", "spath", "fold", "stage", "limit", "ttflips", "threshold", "opening", "closing", "channel", "rle", "min_size",
                       "area_threshold", "split"]
    assert [p[k].default for k in list(p)[2:]] == [0, 0, -1, False, 0.5, 0, 0, 0, True, 0, 0, 0.0]
    ex = inspect.signature(P.predict_masks_ex).parameters                # predict_masks_ex's own, `components` replaced by `split`
    assert list(p)[:-1] == list(ex)[:-1] and [p[k].default for k in list(p)[2:-1]] == [ex[k].default for k in list(ex)[2:-1]]
    p = inspect.signature(P.predict_instances_to_csv).parameters
    assert list(p) == ["self", "spath", "csv_path", "fold", "stage", "limit", "ttflips", "threshold", "opening", "closing", "channel", "columns",
                       "min_size", "area_threshold", "split"]
    assert [p[k].default for k in list(p)[3:]] == [0, 0, -1, False, 0.5, 0, 0, 0, ("image", "rle_mask"), 0, 0, 0.0]
    p, so = inspect.signature(P.score_instances).parameters, inspect.signature(P.score_objects).parameters
    assert list(p) == list(so) + ["split"] and [p[k].default for k in so] == [so[k].default for k in so] and p["split"].default == 0.0
    p = inspect.signature(P.find_split).parameters
    assert list(p) == ["self", "ds", "fold", "stage", "negatives", "ttflips", "thresholds", "splits", "min_size", "opening", "closing", "channel",
                       "area_threshold", "metric", "iou_thresholds", "truth"]
    assert [p[k].default for k in list(p)[3:]] == [-1, "real", None, None, (0, 2, 4, 6), 0, 0, 0, 0, 0, "f2", None, "mask"]


def test_split_radius_conversion():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    assert [P._split_c2(r) for r in (0, 0.0, 1, 1.5, 2.5, 4, np.float32(2.0), np.int64(8), 1024)] == [0, 0, 1, 2, 6, 16, 4, 64, 1048576]
    for bad in (True, False, np.True_, -1, -0.5, 1024.5, 2000, float("nan"), float("inf"), "2", None, [2], (2,), 2 + 0j):
        with pytest.raises(ValueError, match="split"):
            P._split_c2(bad)


BAD_SPLITS = (True, -1, 1025, float("nan"), float("inf"), "2", None)


@pytest.fixture
def no_model_files(monkeypatch):
    """Any attempt to load a model fails the test: the refusals must come first."""
    from segmentation_pipeline.segmentation import PipelineConfig

    def load_model(self, fold=0, stage=-1):
        raise AssertionError("a model was loaded before the arguments were checked")
    monkeypatch.setattr(PipelineConfig, "load_model", load_model)


def test_predict_instances_refusals(no_model_files, tmp_path):
    cfg, softmax = config(), config(classes=3, activation="softmax")
    nowhere = str(tmp_path / "no_such_directory")                         # never listed: every refusal comes at the call, not at next()
    for bad in BAD_SPLITS:
        with pytest.raises(ValueError, match="split"):
            cfg.predict_instances(nowhere, split=bad)
        with pytest.raises(ValueError, match="split"):
            cfg.predict_instances_to_csv(nowhere, str(tmp_path / "x.csv"), split=bad)
    for kw, what in (({"channel": 1}, "channel"), ({"opening": 8}, "opening"), ({"closing": 1.5}, "closing"), ({"min_size": -1}, "min_size"),
                     ({"min_size": 2.0}, "min_size"), ({"area_threshold": True}, "area_threshold")):
        with pytest.raises(ValueError, match=what):
            cfg.predict_instances(nowhere, split=2, **kw)
        with pytest.raises(ValueError, match=what):
            cfg.predict_instances_to_csv(nowhere, str(tmp_path / "x.csv"), split=2, **kw)
    with pytest.raises(ValueError, match="threshold"):
        softmax.predict_instances(nowhere, threshold=0.25, split=2)
    with pytest.raises(ValueError, match="columns"):
        cfg.predict_instances_to_csv(nowhere, str(tmp_path / "x.csv"), columns=("image",), split=2)
    assert not (tmp_path / "x.csv").exists()


def test_score_instances_refusals(no_model_files):
    ds = object()                                                        # never looked at: every refusal comes before the dataset is
    cfg, softmax = config(), config(classes=3, activation="softmax")
    for bad in BAD_SPLITS:
        with pytest.raises(ValueError, match="split"):
            cfg.score_instances(ds, 0, split=bad)
    with pytest.raises(ValueError, match="threshold"):
        softmax.score_instances(ds, 0, threshold=0.25, split=2)
    for kw, what in (({"metric": "dice"}, "metric"), ({"truth": "rle"}, "truth"), ({"channel": 1}, "channel"), ({"opening": 8}, "opening"),
                     ({"closing": 1.5}, "closing"), ({"min_size": -1}, "min_size"), ({"min_size": 2.0}, "min_size"),
                     ({"area_threshold": True}, "area_threshold"), ({"iou_thresholds": [0.45]}, "0.5"),
                     ({"iou_thresholds": [0.5005]}, "three places"), ({"iou_thresholds": [0.9, 0.8]}, "ascending"),
                     ({"iou_thresholds": [i / 1000 for i in range(500, 565)]}, "64")):
        with pytest.raises(ValueError, match=what):
            cfg.score_instances(ds, 0, split=2, **kw)
    with pytest.raises(ValueError, match="channel"):
        softmax.score_instances(ds, 0, channel=3, split=2)


def test_find_split_refusals(no_model_files):
    ds = object()
    cfg, softmax = config(), config(classes=3, activation="softmax")
    with pytest.raises(ValueError, match="softmax"):
        softmax.find_split(ds, 0, thresholds=[0.5])
    for bad in ([0.5, 0.25], [0.25, 0.25], [0.1, float("nan")], [], [i / 100 for i in range(65)]):
        with pytest.raises(ValueError, match="thresholds"):
            cfg.find_split(ds, 0, thresholds=bad)
    for bad in ((), tuple(range(65)), (4, 4), (6, 2), (0, True), (-1, 2), (2, 1025), (2, float("nan")), (2, "4"), (None,)):
        with pytest.raises(ValueError, match="split"):
            cfg.find_split(ds, 0, splits=bad)
    for kw, what in (({"metric": "iou"}, "metric"), ({"truth": None}, "truth"), ({"channel": -1}, "channel"), ({"opening": -1}, "opening"),
                     ({"min_size": -1}, "min_size"), ({"min_size": 1.5}, "min_size"), ({"area_threshold": -2}, "area_threshold"),
                     ({"iou_thresholds": [0.3]}, "0.5")):
        with pytest.raises(ValueError, match=what):
            cfg.find_split(ds, 0, **kw)


def test_split_labels_refusals():
    from segmentation_pipeline.segmentation import PipelineConfig
    ok = np.ones((4, 5), np.uint8)
    for bad in BAD_SPLITS:
        with pytest.raises(ValueError, match="split"):
            PipelineConfig.split_labels(ok, bad)
    for mask in (ok[0], ok[:0], ok[:, :, None], ok.astype(object), np.array([["a"]])):
        with pytest.raises(ValueError, match="mask"):
            PipelineConfig.split_labels(mask, 2)
