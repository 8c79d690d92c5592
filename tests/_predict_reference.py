"""Numpy restatements of the prediction kernels (csrc/predict.hip) and of the host chain they replace (helper of
tests/test_predict_*.py; not collected).  Everything is the float32 arithmetic numpy performs in
``PipelineConfig.predict_on_batch`` / ``_scale_back`` / ``predict_to_directory``: one add per map, one division by the count, one
multiplication by 255 and a truncation, so the device results are compared with ``np.array_equal``."""
import numpy as np

FLIPS = (0, 1, 2)


def flip(x, f):
    """[N, H, W, C]: 0 as it is, 1 columns reversed, 2 rows reversed (whole pixels move; the channels keep their order)."""
    return x if f == 0 else (x[:, :, ::-1] if f == 1 else x[:, ::-1])


def accumulate(acc, probs, f):
    acc += flip(probs, f)          # (in place, as the host loop adds)
    return acc


def source_rows(H, h):
    return np.arange(h) * H // h


def gather(p, h, w):
    """[H, W, C] -> [h, w, C]: pixel (y, x) takes (y * H // h, x * W // w)."""
    return p[source_rows(p.shape[0], h)[:, None], source_rows(p.shape[1], w)[None, :]]


def finish(acc, k, mode, h, w):
    """One image's sums [H, W, C] -> the finished map: 0 float32 [h, w, C], 1 its bytes, 2 the uint8 label map [h, w]."""
    v = gather(acc, h, w) / k
    assert v.dtype == np.float32
    if mode == 0:
        return v
    if mode == 1:
        return (v * 255).astype(np.uint8)
    if acc.shape[2] == 1:
        return (v[:, :, 0] > 0.5).astype(np.uint8)
    return np.argmax(v, axis=2).astype(np.uint8)


def cell_rectangles(h, w, crops):
    """[(y0, y1, x0, x1)] of the crops x crops cells in row-major order: bounds floor(k * size / crops)."""
    ys = [(k * h) // crops for k in range(crops + 1)]
    xs = [(k * w) // crops for k in range(crops + 1)]
    return [(ys[r], ys[r + 1], xs[q], xs[q + 1]) for r in range(crops) for q in range(crops)]
