"""CPU tests of sliding-window prediction's host side (``windows: <overlap>``): the exact-integer geometry of
``PipelineConfig.window_origins`` / ``window_ramp`` / ``window_sums`` against the brute-force restatement of
tests/_window_reference.py, the checks of the key, what the three entry points of csrc/window.hip refuse before any launch, the host
statement on a pointwise model, and that nothing reaches the new path while the key is unset."""
import ctypes
import inspect

import numpy as np
import pytest

import _window_reference as R

AXES = [(150, 64, 0), (150, 64, 16), (150, 64, 32), (100, 64, 16), (64, 64, 16), (40, 64, 16), (65, 64, 32), (5000, 512, 64),
        (128, 64, 0), (160, 64, 16), (160, 64, 32)]          # (the last three: a regular stride up to the image's edge)
BADARG = -1


def config(**kw):
    from segmentation_pipeline import segmentation
    base = {"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "batch": 4}
    return segmentation.PipelineConfig(**dict(base, **kw))


# ---------------------------------------------------------------- geometry
@pytest.mark.parametrize("size,L,overlap", AXES)
def test_axis_geometry(size, L, overlap):
    from segmentation_pipeline.segmentation import PipelineConfig as P
    org = P.window_origins(size, L, overlap)
    assert org == R.origins(size, L, overlap) and all(isinstance(o, int) for o in org)
    assert org[0] == 0 and all(a < b for a, b in zip(org, org[1:]))                   # strictly increasing
    assert org[-1] + L == max(size, L)                                                  # the last window ends at the image's edge
    if size > L:
        assert all(b - a <= L - overlap for a, b in zip(org, org[1:]))                # neighbours overlap by at least `overlap`
    cover = np.zeros(size, np.int64)
    for o in org:
        cover[o:o + L] += 1
    assert cover.min() >= 1 and cover.max() <= 3, (cover.min(), cover.max())           # every pixel is covered
    ramp = P.window_ramp(L, overlap)
    assert ramp.dtype == np.int64 and np.array_equal(ramp, R.ramp(L, overlap))
    assert ramp[0] == 1 and ramp[-1] == 1 and ramp.max() == min(overlap + 1, (L + 1) // 2) and np.array_equal(ramp, ramp[::-1])
    sums = P.window_sums(size, L, overlap)
    assert sums.dtype == np.int64 and sums.shape == (size,) and np.array_equal(sums, R.sums(size, L, overlap))
    assert sums.min() >= 1
    if size > L and (size - L) % (L - overlap) == 0:      # a regular stride throughout: two neighbours' ramps sum to overlap + 1
        assert (sums[overlap:size - overlap] == overlap + 1).all()


@pytest.mark.parametrize("ya,xa", [((150, 64, 16), (100, 64, 16)), ((150, 64, 32), (65, 64, 32)), ((40, 64, 16), (150, 64, 16)),
                                   ((64, 64, 0), (150, 64, 0))])
def test_weight_sum_is_separable(ya, xa):
    """The 2-D sum of ramp_y * ramp_x over the product grid of windows is outer(sy, sx): no weight canvas is needed."""
    from segmentation_pipeline.segmentation import PipelineConfig as P
    (h, H, ov), (w, W, _) = ya, xa
    total = np.zeros((h, w), np.int64)
    wgt = R.ramp(H, ov)[:, None] * R.ramp(W, ov)[None, :]
    for y0, x0 in R.raster(h, w, H, W, ov):
        nh, nw = min(H, h - y0), min(W, w - x0)
        total[y0:y0 + nh, x0:x0 + nw] += wgt[:nh, :nw]
    assert np.array_equal(total, np.outer(P.window_sums(h, H, ov), P.window_sums(w, W, ov)))


# ---------------------------------------------------------------- the key
def test_the_key_is_read_and_checked(tmp_path):
    assert config().windows is None and config(windows=32).windows == 32 and config(windows=0).windows == 0
    for bad in (True, False, 1.5, "16", [16]):
        with pytest.raises(ValueError, match="windows"):
            config(windows=bad)._check_windows()
    for bad in (-1, 33, 1000):
        with pytest.raises(ValueError, match="windows"):
            config(windows=bad)._check_windows()
    with pytest.raises(ValueError, match="windows"):
        config(windows=17, shape=[64, 32, 3])._check_windows()          # half the SMALLER side
    for ok in (0, 1, 32, np.int64(16)):
        config(windows=ok)._check_windows()
    with pytest.raises(ValueError, match="crops"):
        config(windows=16, crops=2)._check_windows()
    # refused before a model is loaded or a directory is read: load_model and every directory method start with the check
    for cfg in (config(windows=16, crops=2), config(windows=40), config(windows=True)):
        with pytest.raises(ValueError, match="windows"):
            cfg.load_model(0, 0)
        with pytest.raises(ValueError, match="windows"):
            cfg.predict_in_directory(str(tmp_path / "absent"), 0, 0, lambda *a: None, None)
        with pytest.raises(ValueError, match="windows"):
            cfg.predict_to_directory(str(tmp_path / "absent"), str(tmp_path / "out"))
        with pytest.raises(ValueError, match="windows"):
            cfg.predict_masks(str(tmp_path / "absent"))
    assert not (tmp_path / "out").exists()
    # set on a parsed config, as cfg.gpus is
    cfg = config()
    cfg.windows = 16
    cfg._check_windows()


def test_weight_sums_must_be_exact_float32_integers():
    """k * max(sy) * max(sx) <= 2**24: checked per image with the number of maps predict_on_batch_device sums."""
    from segmentation_pipeline.segmentation import PipelineConfig as P
    big = config(shape=[8192, 8192, 3], windows=4095)          # 20483 = 8192 + 3 * 4097: a regular stride
    assert int(P.window_sums(20483, 8192, 4095).max()) == 4096
    big._check_windows(1, (20483, 20483))                                 # 4096 * 4096 = 2**24 exactly
    with pytest.raises(ValueError, match="windows"):
        big._check_windows(2, (20483, 20483))
    cfg = config(windows=32)
    top = int(P.window_sums(150, 64, 32).max()) * int(P.window_sums(100, 64, 32).max())
    cfg._check_windows(2 ** 24 // top, (150, 100))
    with pytest.raises(ValueError, match="windows"):
        cfg._check_windows(2 ** 24 // top + 1, (150, 100))


def test_nothing_reaches_the_windows_while_the_key_is_unset(monkeypatch):
    """``windows`` unset: the prediction methods take their old branches (the ``crops`` one raises here instead of computing)."""
    from segmentation_pipeline.segmentation import PipelineConfig as P

    def never(*a, **k):
        raise AssertionError("the windows path was reached with the key unset")

    class Reached(Exception):
        pass

    def cells(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "_predict_windows_device", never)
    monkeypatch.setattr(P, "_predict_windows", never)
    monkeypatch.setattr(P, "_check_windows", never)
    monkeypatch.setattr(P, "_predict_cells_device", cells)
    monkeypatch.setattr(P, "_predict_cells", cells)
    item = type("Item", (), {"x": np.zeros((20, 20, 3), np.uint8), "id": "a.png"})()
    cfg = config(crops=2, shape=[128, 128, 3])
    assert cfg.windows is None
    with pytest.raises(Reached):
        cfg._predict_maps_device([None], False, [item])
    with pytest.raises(Reached):
        cfg._predict_maps([None], False, [item])
    # and with the key set they take the new one
    monkeypatch.setattr(P, "_predict_windows_device", cells)
    monkeypatch.setattr(P, "_predict_windows", cells)
    cfg = config(windows=0)
    with pytest.raises(Reached):
        cfg._predict_maps_device([None], False, [item])
    with pytest.raises(Reached):
        cfg._predict_maps([None], False, [item])


def test_no_existing_method_gained_a_keyword():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    assert list(inspect.signature(P._predict_windows_device).parameters) == ["self", "models", "ttflips", "img", "mode"]
    assert list(inspect.signature(P._predict_windows).parameters) == ["self", "models", "ttflips", "img", "mode"]
    assert list(inspect.signature(P._predict_maps_device).parameters) == ["self", "models", "ttflips", "items", "mode", "original_size"]
    assert list(inspect.signature(P.predict_on_batch_device).parameters) == ["self", "models", "ttflips", "xs_dev", "n"]
    for name in ("predict_in_directory", "predict_to_directory", "predict_on_directory", "evaluateAll", "predict_masks", "find_threshold"):
        assert "windows" not in inspect.signature(getattr(P, name)).parameters


# ---------------------------------------------------------------- the entry points
def test_entry_points_are_bound():
    from segmentation_training_pipeline_amd import _lib, ops
    i32, vp, ip = _lib.i32, _lib.vp, ctypes.POINTER(_lib.i32)
    assert _lib.SIGNATURES["stp_window_gather_u8"] == (i32, [vp, i32, i32, i32, ip, i32, vp, i32, i32, vp])
    assert _lib.SIGNATURES["stp_window_accumulate"] == (i32, [vp, i32, i32, i32, ip, i32, i32, vp, i32, i32, vp])
    assert _lib.SIGNATURES["stp_window_finish"] == (i32, [vp, i32, i32, i32, i32, vp, vp, i32, vp, i32, vp])
    for name in ("window_gather_u8", "window_accumulate", "window_finish"):
        assert callable(getattr(ops, name))


def test_wrappers_have_no_cpu_fallback_and_check_their_buffers():
    import torch
    from segmentation_training_pipeline_amd import _lib, ops
    u8, f32 = torch.uint8, torch.float32
    with pytest.raises(_lib.StpError):
        ops.window_gather_u8(torch.zeros(48, dtype=u8), 4, 4, 3, [(0, 0)], torch.zeros(48, dtype=u8), 4, 4)
    with pytest.raises(_lib.StpError):
        ops.window_accumulate(torch.zeros(48), 4, 4, 3, [(0, 0)], 1, torch.zeros(48), 4, 4)
    with pytest.raises(_lib.StpError):
        ops.window_finish(torch.zeros(48), 4, 4, 3, 1, torch.ones(4), torch.ones(4), 0, torch.zeros(48))
    with pytest.raises(ValueError):
        ops.window_gather_u8(torch.zeros(48, dtype=u8), 4, 4, 3, [(0, 0), (1, 1)], torch.zeros(48, dtype=u8), 4, 4)      # room for one window
    with pytest.raises(ValueError):
        ops.window_gather_u8(torch.zeros(48, dtype=u8), 4, 4, 3, [(0, 0)], torch.zeros(48, dtype=f32), 4, 4)
    with pytest.raises(ValueError):
        ops.window_gather_u8(torch.zeros(48, dtype=u8), 4, 4, 3, [], torch.zeros(48, dtype=u8), 4, 4)
    with pytest.raises(ValueError):
        ops.window_accumulate(torch.zeros(48), 4, 4, 3, [(0, 0)], 1, torch.zeros(47), 4, 4)
    with pytest.raises(ValueError):
        ops.window_accumulate(torch.zeros(48), 4, 4, 3, [(0, 0), (0, 0)], 1, torch.zeros(48), 4, 4)
    with pytest.raises(ValueError):
        ops.window_finish(torch.zeros(48), 4, 4, 3, 1, torch.ones(3), torch.ones(4), 0, torch.zeros(48))
    with pytest.raises(ValueError):
        ops.window_finish(torch.zeros(48), 4, 4, 3, 1, torch.ones(4), torch.ones(4), 1, torch.zeros(48))                 # mode 1 writes uint8
    with pytest.raises(ValueError):
        ops.window_finish(torch.zeros(48), 4, 4, 3, 1, torch.ones(4), torch.ones(4), 0, torch.zeros(48), out_ld=5)       # no room for the pitch


def test_badarg_before_any_launch():
    """Everything the header lists for the three entry points is refused before a launch - so it is refused without a GPU.  The
    pointers are never followed: they only have to be non-NULL and distinct (``origins`` is a real host array)."""
    from segmentation_training_pipeline_amd import _lib
    a, b, c, d = 0x10000, 0x20483, 0x30000, 0x40000

    def org(*pairs):
        return (ctypes.c_int32 * (2 * len(pairs)))(*[v for p in pairs for v in p])
    one = org((0, 0))
    for build in ("bf16", "fp16"):
        lib = _lib.load(build)
        gather = lambda img=a, h=13, w=17, C=3, o=one, n=1, dst=b, H=8, W=8: lib.stp_window_gather_u8(img, h, w, C, o, n, dst, H, W, None)
        accum = lambda acc=a, H=8, W=8, C=3, o=one, n=1, ov=2, cv=b, h=13, w=17: lib.stp_window_accumulate(acc, H, W, C, o, n, ov, cv, h, w, None)
        finish = lambda cv=a, h=13, w=17, C=3, k=1, sy=b, sx=c, mode=0, out=d, ld=17: lib.stp_window_finish(cv, h, w, C, k, sy, sx, mode, out, ld, None)
        # a NULL pointer
        assert gather(img=None) == BADARG and gather(dst=None) == BADARG and gather(o=None) == BADARG
        assert accum(acc=None) == BADARG and accum(cv=None) == BADARG and accum(o=None) == BADARG
        assert finish(cv=None) == BADARG and finish(sy=None) == BADARG and finish(sx=None) == BADARG and finish(out=None) == BADARG
        # a size <= 0
        for bad in (0, -1):
            for name in ("h", "w", "C", "H", "W"):
                assert gather(**{name: bad}) == BADARG, name
                assert accum(**{name: bad}) == BADARG, name
            for name in ("h", "w", "C", "k"):
                assert finish(**{name: bad}) == BADARG, name
        # n outside 1..64
        many = org(*[(0, 0)] * 65)
        for n in (0, -1, 65):
            assert gather(o=many, n=n) == BADARG and accum(o=many, n=n) == BADARG
        # an origin outside the image
        for y0, x0 in ((-1, 0), (0, -1), (13, 0), (0, 17)):
            assert gather(o=org((0, 0), (y0, x0)), n=2) == BADARG and accum(o=org((0, 0), (y0, x0)), n=2) == BADARG
        # overlap < 0 or 2 * overlap > min(H, W)
        assert accum(ov=-1) == BADARG and accum(ov=5) == BADARG and accum(ov=3, W=5) == BADARG
        # source equal to destination
        assert gather(dst=a) == BADARG and accum(cv=a) == BADARG and finish(out=a) == BADARG
        # out_ld < w, a mode outside 0..2, mode 2 with C > 32
        assert finish(ld=16) == BADARG and finish(mode=-1) == BADARG and finish(mode=3) == BADARG and finish(mode=2, C=33) == BADARG


# ---------------------------------------------------------------- the host statement
class Pointwise(object):
    """predict(x) = x.mean(-1, keepdims=True) / 255: the same value for a pixel in whichever window it is predicted."""

    def predict(self, xs):
        return (xs.astype(np.float32).mean(-1, keepdims=True) / np.float32(255)).astype(np.float32)


@pytest.mark.parametrize("overlap", [0, 16, 32])
def test_the_statement_blends_a_pointwise_model_to_itself(overlap):
    """Every window predicts the same value v for a pixel, so the blended map is sum(w_i * v) / sum(w_i) = v up to the roundings: one
    per multiplication, one per addition, one in the division.  With m windows on a pixel the relative error is at most
    (1 + (m - 1) + 1) * 2^-24 to first order, and one ulp of the result is at least 2^-24 of it: at most m + 1 ulp, asserted per pixel
    for every overlap.  The bound of 2 ulp over the whole 150 x 100 map is asserted at overlap 0 and 16 (up to 4 windows on a
    pixel; measured: 0 and 2 ulp).  At overlap 32 up to 9 windows meet on a pixel and the measured maximum is 3 ulp - inside the
    per-pixel bound, outside a flat 2 ulp, which nine rounded additions cannot promise."""
    img = np.random.RandomState(3).randint(0, 256, size=(150, 100, 3)).astype(np.uint8)
    model = Pointwise()
    whole = model.predict(img[None])[0]
    got = R.predict_windows([model], False, img, 64, 64, 3, overlap, 4)
    assert got.shape == (150, 100, 1) and got.dtype == np.float32
    ulp = np.spacing(np.maximum(np.abs(whole), np.float32(2.0 ** -126)))
    err = (np.abs(got.astype(np.float64) - whole.astype(np.float64)) / ulp)[:, :, 0]
    cover = np.zeros((150, 100), np.int64)
    for y0, x0 in R.raster(150, 100, 64, 64, overlap):
        cover[y0:y0 + 64, x0:x0 + 64] += 1
    print("overlap %d: max error %.3g ulp, up to %d windows on a pixel" % (overlap, err.max(), cover.max()))
    assert cover.min() >= 1 and (err <= cover + 1).all()
    if overlap <= 16:
        assert err.max() <= 2.0
    # and its bytes and labels are predict_to_directory's
    assert np.array_equal(R.predict_windows([model], False, img, 64, 64, 3, overlap, 4, R.BYTES), (got * 255).astype(np.uint8))
    assert np.array_equal(R.predict_windows([model], False, img, 64, 64, 3, overlap, 4, R.LABELS), got[:, :, 0] > 0.5)


def test_the_statement_pads_a_small_image_by_its_edge():
    img = np.random.RandomState(4).randint(0, 256, size=(5, 6, 3)).astype(np.uint8)
    assert np.array_equal(R.cut(img, 0, 0, 8, 8), np.pad(img, ((0, 3), (0, 2), (0, 0)), mode="edge"))
    assert np.array_equal(R.cut(img, 2, 3, 8, 8), np.pad(img, ((0, 5), (0, 5), (0, 0)), mode="edge")[2:10, 3:11])
    grey = R.prepare(img[:, :, 0], 3)
    assert grey.shape == (5, 6, 3) and (grey == img[:, :, :1]).all()
    assert np.array_equal(R.prepare(np.concatenate([img, img], axis=2), 3), img)
