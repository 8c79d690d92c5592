"""Host statements of the mask kernels (csrc/mask.hip) on numpy, scipy.ndimage and segmentation_pipeline/impl/rle.py (helper of
tests/test_masks_*.py; not collected).  Everything is exact: comparisons of float32 values and integer work, so the device results
are compared with ``np.array_equal`` and string equality."""
import numpy as np
from scipy import ndimage

from segmentation_pipeline.impl.rle import rle_encode  # noqa: F401  (the string the device runs are formatted to)

METRICS = ("dice", "iou", "f2")


def disk(r):
    """skimage.morphology.disk(r): the (2r + 1)^2 element with dx*dx + dy*dy <= r*r."""
    d = np.arange(-r, r + 1)
    return (d[:, None] ** 2 + d[None, :] ** 2 <= r * r).astype(np.uint8)


def threshold_mask(arr, channel=0, mode=0, threshold=0.5):
    """arr float32 [h, w, C] -> uint8 [h, w].  mode 0: ``arr[..., channel] > float32(threshold)`` (what numpy does with a Python float
    against a float32 array; a NaN is never larger).  mode 1: the first index of the largest of the C values, found by the running
    ``v > best`` of stp_predict_finish mode 2, equals ``channel``."""
    arr = np.asarray(arr)
    assert arr.dtype == np.float32 and arr.ndim == 3
    if mode == 0:
        return (arr[:, :, channel] > np.float32(threshold)).astype(np.uint8)
    best = arr[:, :, 0].copy()
    arg = np.zeros(arr.shape[:2], np.int32)
    for c in range(1, arr.shape[2]):
        up = arr[:, :, c] > best
        best = np.where(up, arr[:, :, c], best)
        arg = np.where(up, c, arg)
    return (arg == channel).astype(np.uint8)


def erode(mask, r):
    return ndimage.binary_erosion(np.asarray(mask) != 0, disk(r)).astype(np.uint8)


def dilate(mask, r):
    return ndimage.binary_dilation(np.asarray(mask) != 0, disk(r)).astype(np.uint8)


def opening(mask, r):
    """scipy.ndimage.binary_opening with its defaults."""
    return ndimage.binary_opening(np.asarray(mask) != 0, disk(r)).astype(np.uint8)


def closing(mask, r):
    """scipy.ndimage.binary_closing with its defaults: the erosion reads zeros outside the image, so a band at the border is cleared."""
    return ndimage.binary_closing(np.asarray(mask) != 0, disk(r)).astype(np.uint8)


def rle_runs(mask):
    """int32 [count, 2] = (start, length): 1-based column-major pixel numbers; the flat array decides what a run is."""
    flat = (np.asarray(mask).T.reshape(-1) != 0).astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate(([0], flat, [0])))) + 1
    starts, stops = edges[0::2], edges[1::2]
    return np.stack([starts, stops - starts], axis=1).astype(np.int32).reshape(-1, 2)


def format_runs(runs):
    return " ".join("%d %d" % (s, n) for s, n in np.asarray(runs).reshape(-1, 2))


def column_crossings(mask):
    """How many runs go on from the bottom of a column to the top of the next."""
    m = np.asarray(mask) != 0
    return int(np.count_nonzero(m[-1, :-1] & m[0, 1:]))


def threshold_counts(arr, target, thresholds, channel=0):
    """-> (counts int64 [T, 2], totals int64 [2]): pixels above each float32 threshold and those of them on the target; target positives
    and the pixel count."""
    v = np.asarray(arr)[:, :, channel]
    assert v.dtype == np.float32
    g = np.asarray(target) != 0
    counts = np.zeros((len(thresholds), 2), np.int64)
    for t, thr in enumerate(thresholds):
        above = v > np.float32(thr)
        counts[t] = (np.count_nonzero(above), np.count_nonzero(above & g))
    return counts, np.array([np.count_nonzero(g), g.size], np.int64)


def score(metric, P, TP, G):
    """float64 from integer counters: P predicted, TP true positive, G positives of the target; 1 where P = G = 0."""
    P, TP, G = (np.asarray(a, np.float64) for a in (P, TP, G))
    num, den = {"dice": (2 * TP, P + G), "iou": (TP, P + G - TP), "f2": (5 * TP, 4 * G + P)}[metric]
    empty = (P == 0) & (G == 0)
    return np.where(empty, 1.0, num / np.where(empty, 1.0, den))


def sweep_table(per_image, metric, average):
    """per_image: [(counts [T, 2], totals [2])] -> float64 [T]: the mean of the images' scores ("image") or the score of the summed
    counters ("pixels")."""
    counts = np.stack([c for c, _ in per_image]).astype(np.int64)          # [n, T, 2]
    G = np.array([t[0] for _, t in per_image], np.int64)                   # [n]
    if average == "pixels":
        return score(metric, counts[:, :, 0].sum(0), counts[:, :, 1].sum(0), G.sum())
    return score(metric, counts[:, :, 0], counts[:, :, 1], G[:, None]).mean(axis=0)

