"""The host statement of sliding-window prediction (``windows: <overlap>``; helper of tests/test_window_*.py and of
tests/_window_time.py; numpy only, not collected, not imported by the package): what a user of the pipeline would write around
``model.predict`` today, and what the device path (csrc/window.hip under ``PipelineConfig._predict_windows_device``) must equal bit
for bit.

The geometry is restated here from its definition, not imported: along one axis the windows of length L start every ``L - overlap``
pixels, the last one shifted back to end at the image's edge; a window weights its pixel i with ``min(i + 1, L - i, overlap + 1)``.
Every float32 value comes from one numpy operation: one add per model and flip (``predict_on_batch``'s order, without its division),
one multiplication by the integer weight and one add per window in raster order, one division by ``k * sy[y] * sx[x]``."""
import numpy as np

PROBS, BYTES, LABELS = 0, 1, 2


def origins(size, L, overlap):
    if size <= L:
        return [0]
    out, o = [], 0
    while o < size - L:
        out.append(o)
        o += L - overlap
    return out + [size - L]


def ramp(L, overlap):
    return np.array([min(i + 1, L - i, overlap + 1) for i in range(L)], np.int64)


def sums(size, L, overlap):
    """Brute force: per pixel of the axis, the ramps of the windows that hold it."""
    r = ramp(L, overlap)
    return np.array([sum(int(r[p - o]) for o in origins(size, L, overlap) if o <= p < o + L) for p in range(size)], np.int64)


def raster(h, w, H, W, overlap):
    """The (y0, x0) of an h x w image's windows in raster order."""
    return [(y0, x0) for y0 in origins(h, H, overlap) for x0 in origins(w, W, overlap)]


def prepare(img, ch):
    """The channels as ``_resize_to_net`` prepares them: grey repeated, extra bands cut."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[:, :, None]
    if img.shape[2] < ch:
        assert img.shape[2] == 1
        img = np.repeat(img, ch, axis=2)
    return np.ascontiguousarray(img[:, :, :ch], dtype=np.uint8)


def cut(img, y0, x0, H, W):
    """The H x W window at (y0, x0), indices clipped to the image (np.pad(mode="edge") of an image smaller than the window)."""
    h, w = img.shape[:2]
    yy = np.minimum(y0 + np.arange(H), h - 1)[:, None]
    xx = np.minimum(x0 + np.arange(W), w - 1)[None, :]
    return img[yy, xx]


def batch_sum(models, ttflips, xs):
    """``predict_on_batch`` without its division: (float32 sums [n, H, W, classes], k)."""
    acc, k = None, 0
    for m in models:
        p = m.predict(xs)
        acc = np.zeros(p.shape, np.float32) if acc is None else acc
        acc += p; k += 1
        if ttflips:
            acc += m.predict(xs[:, :, ::-1])[:, :, ::-1]; k += 1
            acc += m.predict(xs[:, ::-1])[:, ::-1]; k += 1
    return acc, k


def accumulate(canvas, acc, chunk, overlap):
    """canvas[win] += (ry * rx) * acc, window by window in the chunk's order; the part of a window beyond the image is dropped."""
    h, w = canvas.shape[:2]
    H, W = acc.shape[1:3]
    ry, rx = ramp(H, overlap), ramp(W, overlap)
    wgt = (ry[:, None] * rx[None, :]).astype(np.float32)[..., None]
    for a, (y0, x0) in zip(acc, chunk):
        nh, nw = min(H, h - y0), min(W, w - x0)
        canvas[y0:y0 + nh, x0:x0 + nw] += (wgt * a)[:nh, :nw]
    return canvas


def quantise(v, mode):
    """A finished float32 map as it is, its bytes or its labels, as ``predict_to_directory`` makes them."""
    assert v.dtype == np.float32
    if mode == PROBS:
        return v
    if mode == BYTES:
        return (v * 255).astype(np.uint8)
    if v.shape[2] == 1:
        return (v[:, :, 0] > 0.5).astype(np.uint8)
    return np.argmax(v, axis=2).astype(np.uint8)


def finish(canvas, k, sy, sx, mode):
    """canvas / (k * sy[y] * sx[x]): the weight sums are exact float32 integers, and so is their product with k."""
    den = (np.float32(k) * sy.astype(np.float32)[:, None] * sx.astype(np.float32)[None, :])[..., None]
    return quantise(canvas / den, mode)


def predict_windows(models, ttflips, img, H, W, ch, overlap, batch, mode=PROBS):
    """The finished map of one image: ``models`` have ``predict(uint8 [n, H, W, ch]) -> float32 [n, H, W, classes]``, n <= batch."""
    img = prepare(img, ch)
    h, w = img.shape[:2]
    org = raster(h, w, H, W, overlap)
    canvas, k = None, 0
    for s in range(0, len(org), batch):
        chunk = org[s:s + batch]
        acc, k = batch_sum(models, ttflips, np.stack([cut(img, y0, x0, H, W) for y0, x0 in chunk]))
        if canvas is None:
            canvas = np.zeros((h, w, acc.shape[-1]), np.float32)
        accumulate(canvas, acc, chunk, overlap)
    return finish(canvas, k, sums(h, H, overlap), sums(w, W, overlap), mode)
