"""Host statement of the per-object measurements (csrc/measure.hip) on numpy (helper of tests/test_measure_*.py; not collected).
Everything after the quantisation is integer work: the device results are compared with ``np.array_equal``.

The arithmetic (include/stp_hip.h has the same text):
  * ``labels`` is an integer label image [h, w], 0 = background, values 0..label_cap; a value outside that range (a negative one too) is
    background, never an index, and its pixel is counted in ``out_of_range``.
  * ``quantise``: q = (int) (clamp(p, 0, 1) * 65535.0f) - one float32 multiply, one truncation; a NaN gives 0; 0..65535.
  * ``measure``: per label k in 0..label_cap  sums[k] = (area, sum of y, sum of x, sum of q) in int64 and boxes[k] = (min y, min x, max y,
    max x) in int32, closed, (h, w, -1, -1) for a label without a pixel.  Row 0 is all zero with the empty box.  The sums come from a stable
    sort by label and ``np.add.reduceat`` in int64: no float takes part.
  * ``table``: the float64 columns derived from the integers: cy = sum y / area, cx = sum x / area, confidence = sum q / (65535 * area), and
    the half-open box (y0, x0, y1, x1) = (min y, min x, max y + 1, max x + 1) - scipy.ndimage.find_objects' slices.
  * ``select``: label k is kept iff area > 0, area >= min_area and sum q * conf_den >= conf_num * 65535 * area, in Python integers; the kept
    labels keep their order and are renumbered 1..count through the cumulative sum of the keep flags; every other pixel becomes 0."""
import numpy as np

CONF_ONE = 65535
CONF_DEN = 10000
COLUMNS = ("label", "area", "y0", "x0", "y1", "x1", "cy", "cx", "confidence")


def quantise(p):
    """float32 array -> int64 array of q."""
    p = np.asarray(p, np.float32)
    p = np.where(np.isnan(p), np.float32(0), p)
    return (np.clip(p, 0, 1).astype(np.float32) * np.float32(CONF_ONE)).astype(np.int64)


def measure(labels, label_cap, probs=None, channel=0):
    """-> (sums int64 [label_cap + 1, 4], boxes int32 [label_cap + 1, 4], out_of_range)."""
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    outside = (lab < 0) | (lab > label_cap)
    lab = np.where(outside, 0, lab)
    q = np.zeros((h, w), np.int64)
    if probs is not None:
        probs = np.asarray(probs)
        q = quantise(probs if probs.ndim == 2 else probs[:, :, channel])
    sums = np.zeros((label_cap + 1, 4), np.int64)
    boxes = np.empty((label_cap + 1, 4), np.int32)
    boxes[:] = (h, w, -1, -1)
    yy, xx = (a.ravel() for a in np.indices((h, w)))
    flat = lab.ravel()
    on = flat > 0
    if on.any():
        order = np.argsort(flat[on], kind="stable")
        keys = flat[on][order]
        starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
        ks = keys[starts]
        ones = np.ones(len(keys), np.int64)
        for c, v in enumerate((ones, yy[on][order].astype(np.int64), xx[on][order].astype(np.int64), q.ravel()[on][order])):
            sums[ks, c] = np.add.reduceat(v, starts)
        boxes[ks, 0] = np.minimum.reduceat(yy[on][order], starts)
        boxes[ks, 1] = np.minimum.reduceat(xx[on][order], starts)
        boxes[ks, 2] = np.maximum.reduceat(yy[on][order], starts)
        boxes[ks, 3] = np.maximum.reduceat(xx[on][order], starts)
    return sums, boxes, int(outside.sum())


def conf_num(min_confidence):
    """The numerator n of the public ``min_confidence`` = n / 10000."""
    n = int(round(float(min_confidence) * CONF_DEN))
    assert abs(float(min_confidence) * CONF_DEN - n) < 1e-6 and 0 <= n <= CONF_DEN
    return n


def keep_flags(sums, min_area, num, den=CONF_DEN):
    """-> bool [rows]: Python integers, so that no product can wrap."""
    out = np.zeros(len(sums), bool)
    for k in range(1, len(sums)):
        area, sq = int(sums[k, 0]), int(sums[k, 3])
        out[k] = area > 0 and area >= int(min_area) and sq * int(den) >= int(num) * CONF_ONE * area
    return out


def select(labels, label_cap, sums, boxes, min_area, num, den=CONF_DEN):
    """-> (int32 [h, w] renumbered labels, count, sums [count + 1, 4], boxes [count + 1, 4]) - the rows 0..count in the new numbering."""
    lab = np.asarray(labels).astype(np.int64)
    h, w = lab.shape
    lab = np.where((lab < 0) | (lab > label_cap), 0, lab)
    keep = keep_flags(sums, min_area, num, den)
    new = np.where(keep, np.cumsum(keep), 0)
    count = int(keep.sum())
    out_sums = np.zeros((count + 1, 4), np.int64)
    out_boxes = np.empty((count + 1, 4), np.int32)
    out_boxes[0] = (h, w, -1, -1)
    out_sums[new[keep]] = sums[keep]
    out_boxes[new[keep]] = boxes[keep]
    return new[lab].astype(np.int32), count, out_sums, out_boxes


def table(sums, boxes, count):
    """The public columns over the objects 1..count, from the integers alone."""
    s, b = np.asarray(sums, np.int64)[1:count + 1], np.asarray(boxes, np.int64)[1:count + 1]
    area = s[:, 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"label": np.arange(1, count + 1, dtype=np.int64), "area": s[:, 0].copy(), "y0": b[:, 0].copy(), "x0": b[:, 1].copy(),
                "y1": b[:, 2] + 1, "x1": b[:, 3] + 1, "cy": s[:, 1] / area, "cx": s[:, 2] / area,
                "confidence": s[:, 3] / (np.float64(CONF_ONE) * area)}


def measure_select(labels, probs, channel, min_area, min_confidence, label_cap=None):
    """measure, then select -> (labels, count, sums, boxes) of the selected objects."""
    cap = int(np.asarray(labels).max(initial=0)) if label_cap is None else label_cap
    sums, boxes, _ = measure(labels, cap, probs, channel)
    return select(labels, cap, sums, boxes, min_area, conf_num(min_confidence))
