"""Host statements of the connected-component kernels (csrc/components.hip) on numpy, scipy.ndimage and
segmentation_pipeline/impl/rle.py (helper of tests/test_components_*.py; not collected).  skimage's ``remove_small_objects`` /
``remove_small_holes`` are restated from their code - ``ndi.label``, ``np.bincount``, ``sizes < min_size`` with a strict ``<``; the holes
as ``~remove_small_objects(~mask)`` - so that the tests need no skimage.  Everything is integer work: the device results are compared
with ``np.array_equal`` and string equality."""
import numpy as np
from scipy import ndimage

from segmentation_pipeline.impl.rle import multi_rle_encode, rle_encode  # noqa: F401


def label(mask, connectivity, invert=0):
    """-> (int32 [h, w] labels, count): scipy's numbering of the components of ``(mask != 0) != invert``; connectivity 1 is the 4-, 2 the
    8-neighbourhood."""
    fg = (np.asarray(mask) != 0) != bool(invert)
    labels, n = ndimage.label(fg, ndimage.generate_binary_structure(2, connectivity))
    return labels.astype(np.int32), int(n)


def remove_small_objects(mask, min_size, connectivity=1):
    """skimage.morphology.remove_small_objects on a boolean mask -> uint8 {0, 1}."""
    out = np.asarray(mask) != 0
    labels, n = label(out, connectivity)
    sizes = np.bincount(labels.ravel())
    too_small = sizes < min_size                      # (strict: a component of exactly min_size pixels stays)
    too_small[0] = False                              # the background's count is no object
    out = out.copy()
    out[too_small[labels]] = False
    return out.astype(np.uint8)


def remove_small_holes(mask, area_threshold, connectivity=1):
    """skimage.morphology.remove_small_holes = ~remove_small_objects(~mask, area_threshold, connectivity) -> uint8 {0, 1}: every component
    of zeros with fewer than ``area_threshold`` pixels is filled, one that touches the image border too."""
    m = np.asarray(mask) != 0
    return (1 - remove_small_objects(~m, area_threshold, connectivity)).astype(np.uint8)


def label_runs(labels):
    """int32 [count, 3] = (value, start, length): the maximal stretches of equal non-zero values of the flat column-major array
    ``labels.T.reshape(-1)``, 1-based starts, ascending."""
    flat = np.asarray(labels).T.reshape(-1).astype(np.int64)
    if flat.size == 0:
        return np.zeros((0, 3), np.int32)
    change = np.flatnonzero(np.diff(flat)) + 1
    starts = np.concatenate(([0], change))
    stops = np.concatenate((change, [flat.size]))
    keep = flat[starts] != 0
    return np.stack([flat[starts], starts + 1, stops - starts], axis=1)[keep].astype(np.int32).reshape(-1, 3)


def group_runs(runs, count=None):
    """The triples grouped by value (a stable sort: each value's runs stay in ascending start) and formatted: one ``"start length ..."``
    string per value 1..count, as ``PipelineConfig._group_runs`` does."""
    runs = np.asarray(runs).reshape(-1, 3)
    n = int(runs[:, 0].max()) if count is None and len(runs) else int(count or 0)
    order = np.argsort(runs[:, 0], kind="stable")
    runs = runs[order]
    cuts = np.searchsorted(runs[:, 0], np.arange(1, n + 2))
    return [" ".join("%d %d" % (s, c) for _, s, c in runs[cuts[k]:cuts[k + 1]]) for k in range(n)]


def multi_rle(mask):
    """impl.rle.multi_rle_encode of a 2-D mask: one run-length string per 8-connected component, in label order."""
    return multi_rle_encode(np.asarray(mask)[:, :, None])


def column_wraps(labels):
    """-> (same, different): column boundaries where a non-zero value at the bottom of a column meets the same / another non-zero value at
    the top of the next."""
    a, b = np.asarray(labels)[-1, :-1], np.asarray(labels)[0, 1:]
    both = (a != 0) & (b != 0)
    return int(np.count_nonzero(both & (a == b))), int(np.count_nonzero(both & (a != b)))


def serpentine(h, w):
    """Even rows all ones; odd row y has a single one, at the right end if (y // 2) is even and at the left end otherwise."""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = 1
    for y in range(1, h, 2):
        m[y, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m
