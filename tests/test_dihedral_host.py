"""CPU tests of dihedral (D4) test-time augmentation's host side: the numpy statement of the group (tests/_dihedral_reference.py) is a
group and agrees with the flips it extends, ``PipelineConfig._tta_ops`` maps the ``ttflips`` values to their members, a non-square
network shape refuses ``"d4"`` before a model is loaded, the sliding-window weight bound counts eight maps per model, and the new
entry points are bound."""
import inspect
import types

import numpy as np
import pytest
import yaml

import _dihedral_reference as D
import _predict_reference as R


def distinct(shape):
    return np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)


def parsed(tmp_path, **kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "encoder_weights": None,
            "shape": [64, 64, 3], "batch": 4, "loss": "binary_crossentropy", "folds_count": 2, "stages": [{"epochs": 1}]}
    path = str(tmp_path / "config.yaml")
    with open(path, "w") as f:
        yaml.safe_dump(dict(base, **kw), f)
    return segmentation.parse(path)


def test_reference_is_the_dihedral_group():
    x = distinct((2, 5, 7, 3))
    images = [D.apply(x, op) for op in D.OPS]
    assert D.OPS == (0, 1, 2, 3, 4, 5, 6, 7)
    for op, g in zip(D.OPS, images):
        assert g.shape == ((2, 7, 5, 3) if op & 4 else (2, 5, 7, 3)), op
        assert np.array_equal(D.invert(g, op), x), op
        assert np.array_equal(g[..., 0] // 3, g[..., 2] // 3) and (g[..., 1] - g[..., 0] == 1).all()      # whole pixels, channels in order
    for a in D.OPS:
        for b in D.OPS:
            if a < b:
                assert images[a].shape != images[b].shape or not np.array_equal(images[a], images[b]), (a, b)
    for f in R.FLIPS:
        assert np.array_equal(images[f], R.flip(x, f)), f
    # the group table: 3 = 1 o 2 (half turn), 5 = 1 o 4 and 6 = 2 o 4 (quarter turns), 7 = 3 o 4 (anti-transpose)
    assert np.array_equal(images[3], D.apply(D.apply(x, 2), 1)) and np.array_equal(images[3], x[:, ::-1, ::-1])
    assert np.array_equal(images[5], D.apply(D.apply(x, 4), 1))
    assert np.array_equal(images[6], D.apply(D.apply(x, 4), 2))
    assert np.array_equal(images[7], D.apply(D.apply(x, 4), 3))
    assert np.array_equal(images[4], x.transpose(0, 2, 1, 3))
    assert np.array_equal(images[5], np.rot90(x, -1, axes=(1, 2))) and np.array_equal(images[6], np.rot90(x, 1, axes=(1, 2)))
    # closed under composition, and every member has its inverse among the eight
    for a in D.OPS:
        for b in D.OPS:
            c = D.apply(images[b], a)
            assert sum(c.shape == g.shape and np.array_equal(c, g) for g in images) == 1, (a, b)


def test_accumulate_adds_the_untransformed_map():
    rng = np.random.RandomState(1)
    for op in D.OPS:
        acc = rng.uniform(0, 1, size=(2, 5, 7, 3)).astype(np.float32)
        p = rng.uniform(0, 1, size=D.apply(acc, op).shape).astype(np.float32)
        want = acc + D.invert(p, op)
        if op < 3:
            assert np.array_equal(R.accumulate(acc.copy(), p, op), want)      # (the un-flip of a map is the same flip)
        got = D.accumulate(acc, p, op)
        assert got is acc and got.dtype == np.float32 and np.array_equal(got, want)


def test_the_package_states_the_same_group():
    from segmentation_pipeline.segmentation import PipelineConfig
    x = distinct((2, 5, 7, 3))
    for op in D.OPS:
        assert np.array_equal(PipelineConfig._d4_apply(x, op), D.apply(x, op)), op
        assert np.array_equal(PipelineConfig._d4_invert(D.apply(x, op), op), x), op


def test_tta_ops():
    from segmentation_pipeline.segmentation import PipelineConfig
    ops = PipelineConfig._tta_ops
    assert ops(None) == (0,) and ops(False) == (0,)
    assert ops(True) == (0, 1, 2) and ops(1) == (0, 1, 2) and ops(np.bool_(True)) == (0, 1, 2)
    assert ops("d4") == (0, 1, 2, 3, 4, 5, 6, 7)
    for bad in ("D4", "d8", ""):
        with pytest.raises(ValueError, match="d4"):
            ops(bad)


def test_host_loop_order_and_count():
    """``predict_on_batch``: per model the members in ascending order - the first three additions of ``"d4"`` are those of ``True`` -
    and k = 8 per model."""
    from segmentation_pipeline.segmentation import PipelineConfig
    cfg = PipelineConfig(architecture="Unet", backbone="resnet18", classes=2, activation="sigmoid", shape=[6, 6, 3], batch=4)
    xs = np.random.RandomState(3).randint(0, 256, size=(3, 6, 6, 3)).astype(np.uint8)
    seen = []

    class Model(object):
        def __init__(self, scale):
            self.scale = np.float32(scale)

        def predict(self, x):
            x = np.ascontiguousarray(x)
            seen.append(x)
            return (x[..., :2].astype(np.float32) / np.float32(255) * self.scale + x[..., 2:3].astype(np.float32) / np.float32(1024))

    models = [Model(1.0), Model(0.5)]
    got = cfg.predict_on_batch(models, "d4", xs)
    assert len(seen) == 16
    for i, x in enumerate(seen):
        assert np.array_equal(x, D.apply(xs, i % 8)), i
    acc, k = D.batch_sum(models, xs)
    assert k == 16 and got.dtype == np.float32 and np.array_equal(got, acc / k)
    del seen[:]
    three = cfg.predict_on_batch(models[0], True, xs)
    assert len(seen) == 3 and all(np.array_equal(x, R.flip(xs, f)) for f, x in zip(R.FLIPS, seen))
    want = np.zeros(three.shape, np.float32)
    for f in R.FLIPS:
        want += R.flip(models[0].predict(R.flip(xs, f)), f)
    assert np.array_equal(three, want / 3)


def test_non_square_shape_refuses_d4_before_a_model_is_loaded(tmp_path, monkeypatch):
    cfg = parsed(tmp_path, shape=[64, 96, 3])
    monkeypatch.setattr(cfg, "load_model", lambda *a, **k: pytest.fail("load_model was reached"))
    with pytest.raises(ValueError, match="H == W.*ttflips=True"):
        cfg.predict_in_directory(str(tmp_path), 0, 0, lambda *a: None, None, ttflips="d4")
    with pytest.raises(ValueError, match="H == W.*ttflips=True"):
        cfg.find_tta(None, 0)
    with pytest.raises(ValueError, match="H == W"):
        cfg.predict_to_directory(str(tmp_path), str(tmp_path / "out"), ttflips="d4")
    with pytest.raises(ValueError, match="H == W"):
        cfg.predict_masks(str(tmp_path), ttflips="d4")
    with pytest.raises(ValueError, match="H == W"):
        cfg.predict_instances(str(tmp_path), ttflips="d4")
    with pytest.raises(ValueError, match="H == W"):
        cfg.find_threshold(None, 0, ttflips="d4")
    with pytest.raises(ValueError, match="H == W"):
        cfg.score_objects(None, 0, ttflips="d4")
    with pytest.raises(ValueError, match="H == W"):
        cfg.score_instances_ex(None, 0, ttflips="d4")
    with pytest.raises(ValueError, match="H == W"):
        next(cfg.evaluateAll(range(4), 0, ttflips="d4"))
    with pytest.raises(ValueError, match="accepted values"):
        cfg.predict_in_directory(str(tmp_path), 0, 0, lambda *a: None, None, ttflips="d8")
    assert not (tmp_path / "out").exists()
    # the network shape after the `crops` division is what counts
    crops = parsed(tmp_path, shape=[128, 192, 3], crops=2)
    monkeypatch.setattr(crops, "load_model", lambda *a, **k: pytest.fail("load_model was reached"))
    with pytest.raises(ValueError, match="64 x 96"):
        crops.predict_in_directory(str(tmp_path), 0, 0, lambda *a: None, None, ttflips="d4")
    assert parsed(tmp_path, shape=[128, 128, 3], crops=2)._check_tta("d4") == D.OPS
    assert parsed(tmp_path, shape=[64, 96, 3])._check_tta(True) == (0, 1, 2)


def test_find_tta_refusals(tmp_path, monkeypatch):
    for kw in ({"windows": 16}, {"crops": 2, "shape": [128, 128, 3]}):
        cfg = parsed(tmp_path, **kw)
        monkeypatch.setattr(cfg, "load_model", lambda *a, **k: pytest.fail("load_model was reached"))
        with pytest.raises(ValueError, match="windows.*crops"):
            cfg.find_tta(None, 0)
    cfg = parsed(tmp_path)
    monkeypatch.setattr(cfg, "load_model", lambda *a, **k: pytest.fail("load_model was reached"))
    with pytest.raises(ValueError, match="one fold"):
        cfg.find_tta(None, [0, 1])
    with pytest.raises(ValueError, match="metric"):
        cfg.find_tta(None, 0, metric="f1")
    from segmentation_pipeline.segmentation import PipelineConfig
    assert list(inspect.signature(PipelineConfig.find_tta).parameters) == ["self", "ds", "fold", "stage", "negatives", "threshold", "metric",
                                                                            "average", "channel"]


class Reached(Exception):
    pass


def test_window_weight_check_counts_eight_maps_per_model(tmp_path):
    """``_predict_windows_device`` hands ``_check_windows`` 8 maps per model for ``"d4"`` (3 for True, 1 for False), and the 2^24 bound
    holds for them: 1024-pixel windows overlapping by 512 have weight sums of 513 per axis, so 8 x 8 = 64 maps exceed it (64 * 513^2 >
    2^24) where 8 x 3 = 24 do not."""
    cfg = parsed(tmp_path, shape=[1024, 1024, 3], windows=512)
    calls = []
    real = cfg._check_windows

    def check(k=None, size=None):
        calls.append((k, size))
        real(k, size)
        if k is not None:
            raise Reached()
    cfg._check_windows = check
    img = np.zeros((1536, 1536, 3), np.uint8)
    models = [types.SimpleNamespace(H=1024, W=1024, in_ch=3, batch=1, device="cpu") for _ in range(8)]
    for ttflips, per_model in ((False, 1), (True, 3), ("d4", 8)):
        for count in (1, 2):
            del calls[:]
            with pytest.raises(Reached):
                cfg._predict_windows_device(models[:count], ttflips, img)
            assert calls[-1] == (per_model * count, (1536, 1536)), (ttflips, count)
    assert int(cfg.window_sums(1536, 1024, 512).max()) == 513 and 63 * 513 * 513 <= 2 ** 24 < 64 * 513 * 513
    with pytest.raises(Reached):
        cfg._predict_windows_device(models, True, img)
    with pytest.raises(ValueError, match="64 maps per window"):
        cfg._predict_windows_device(models, "d4", img)


def test_entry_points_are_bound():
    from segmentation_training_pipeline_amd import _lib, ops
    i32, vp = _lib.i32, _lib.vp
    assert _lib.SIGNATURES["stp_dihedral_u8"] == (i32, [vp, vp, i32, i32, i32, i32, i32, vp])
    assert _lib.SIGNATURES["stp_predict_accumulate_dihedral"] == (i32, [vp, vp, i32, i32, i32, i32, i32, vp])
    for storage in ("bf16", "fp16"):
        lib = _lib.load(storage)
        assert lib.stp_dihedral_u8 and lib.stp_predict_accumulate_dihedral
    assert callable(ops.dihedral_u8) and callable(ops.predict_accumulate_dihedral)


def test_wrappers_check_sizes_and_have_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    with pytest.raises(ValueError, match="smaller"):
        ops.dihedral_u8(torch.zeros(47, dtype=torch.uint8), torch.zeros(48, dtype=torch.uint8), 1, 4, 4, 3, 4)
    with pytest.raises(ValueError, match="smaller"):
        ops.predict_accumulate_dihedral(torch.zeros(48), torch.zeros(47), 1, 4, 4, 3, 4)
    with pytest.raises(_lib.StpError):
        ops.dihedral_u8(torch.zeros(48, dtype=torch.uint8), torch.zeros(48, dtype=torch.uint8), 1, 4, 4, 3, 4)
    with pytest.raises(_lib.StpError):
        ops.predict_accumulate_dihedral(torch.zeros(48), torch.zeros(48), 1, 4, 4, 3, 4)
