"""Host statements of the object-matching kernels (csrc/object_match.hip) on numpy and scipy.ndimage (helper of
tests/test_object_match_*.py; not collected).  Everything is integer work: the device results are compared with ``np.array_equal``.

Two statements of the true positives, which the CPU tests check against each other:
  * ``label_match``: the kernel's arithmetic - ``np.bincount`` areas, the pair histogram by ``np.unique((p << 32) | g)`` over the pixels
    with both labels > 0, a pair matches at t = num / den iff ``I * den > num * U`` in int64;
  * ``kaggle_true_positives``: the form of the competitions' notebooks - ``np.histogram2d`` intersections, the dense [n_truth, n_pred]
    float64 IoU matrix, "a truth object is hit if any prediction exceeds t"."""
import numpy as np
from scipy import ndimage

DEFAULT_NUM, DEFAULT_DEN = list(range(10, 20)), 20          # 0.5, 0.55, ..., 0.95


def label8(mask):
    """-> (int32 [h, w] labels, count): scipy.ndimage.label of ``mask != 0`` with the 8-neighbourhood."""
    labels, n = ndimage.label(np.asarray(mask) != 0, ndimage.generate_binary_structure(2, 2))
    return labels.astype(np.int32), int(n)


def clip_labels(labels, label_cap):
    """-> (int64 labels with every value outside 0..label_cap made background, the boolean image of those pixels)."""
    a = np.asarray(labels).astype(np.int64)
    outside = (a < 0) | (a > label_cap)
    return np.where(outside, 0, a), outside


def overlaps(pred, truth, label_cap):
    """-> (int32 [k, 3] triples (a, b, I) of the non-empty pairs sorted by (a, b), int32 areas [label_cap + 1] of pred and of truth, the
    number of pixels with a value outside 0..label_cap in either image)."""
    p, po = clip_labels(pred, label_cap)
    g, go = clip_labels(truth, label_cap)
    area_p = np.bincount(p.ravel(), minlength=label_cap + 1)
    area_g = np.bincount(g.ravel(), minlength=label_cap + 1)
    area_p[0] = area_g[0] = 0                         # the background is no object
    both = (p > 0) & (g > 0)
    keys, counts = np.unique((p[both] << 32) | g[both], return_counts=True)
    triples = np.stack([keys >> 32, keys & 0xffffffff, counts], axis=1).astype(np.int32).reshape(-1, 3)
    return triples, area_p.astype(np.int32), area_g.astype(np.int32), int(np.count_nonzero(po | go))


def label_match(pred, truth, label_cap, num=DEFAULT_NUM, den=DEFAULT_DEN):
    """-> int64 [T + 3]: TP per threshold num[k] / den, the pred labels with pixels, the truth labels with pixels, out-of-range pixels."""
    triples, area_p, area_g, outside = overlaps(pred, truth, label_cap)
    a, b, I = (triples[:, k].astype(np.int64) for k in range(3))
    U = area_p[a].astype(np.int64) + area_g[b].astype(np.int64) - I
    tp = [int(np.count_nonzero(I * int(den) > int(n) * U)) for n in num]
    return np.asarray(tp + [int(np.count_nonzero(area_p)), int(np.count_nonzero(area_g)), outside], np.int64)


def kaggle_true_positives(pred, truth, ts):
    """The notebooks' statement: per float threshold t the number of truth objects whose IoU with some predicted object is > t; also
    returns the largest number of partners any label has at the smallest t."""
    p, g = np.asarray(pred).ravel(), np.asarray(truth).ravel()
    n_p, n_g = int(p.max(initial=0)), int(g.max(initial=0))          # (labels 1..n, as scipy numbers them)
    inter = np.histogram2d(g, p, bins=(np.arange(n_g + 2) - 0.5, np.arange(n_p + 2) - 0.5))[0]
    area_g, area_p = inter.sum(axis=1, keepdims=True), inter.sum(axis=0, keepdims=True)
    union = area_g + area_p - inter
    iou = (inter[1:, 1:] / np.where(union[1:, 1:] > 0, union[1:, 1:], 1.0))          # without the background's row and column
    tp = [int((iou > t).any(axis=1).sum()) if iou.size else 0 for t in ts]
    hits = iou > min(ts)
    partners = int(max(hits.sum(axis=0).max(), hits.sum(axis=1).max())) if iou.size else 0
    return tp, partners


def object_score(metric, TP, n_pred, n_truth):
    """float64: f2 = 5TP / (5TP + 4FN + FP), ap = TP / (TP + FP + FN) with FP = n_pred - TP, FN = n_truth - TP; 1 where both are 0."""
    TP, P, G = (np.asarray(a, np.float64) for a in (TP, n_pred, n_truth))
    FP, FN = P - TP, G - TP
    num, den = (5 * TP, 5 * TP + 4 * FN + FP) if metric == "f2" else (TP, TP + FP + FN)
    empty = (P == 0) & (G == 0)
    return np.where(empty, 1.0, num / np.where(empty, 1.0, den))


# ------------------------------------------------------------------------------------------------ inputs
def discs(h, w, seed, shift=(0, 0), flip=0.0, flip_seed=0):
    """A mask of a few discs (one per 300 pixels, radii 1.5..7), moved by ``shift`` = (dy, dx), with a fraction ``flip`` of the pixels
    inverted (drawn from ``flip_seed``)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    for _ in range(max(1, h * w // 300)):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1.5, 7)
        m |= (yy - cy - shift[0]) ** 2 + (xx - cx - shift[1]) ** 2 <= r * r
    if flip:
        m ^= np.random.default_rng(seed + 7919 + flip_seed).random((h, w)) < flip
    return m.astype(np.uint8)


def salt(h, w, seed, p=0.5):
    return (np.random.default_rng(seed).random((h, w)) < p).astype(np.uint8)
