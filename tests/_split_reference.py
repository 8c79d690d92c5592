"""Host statements of the object-splitting kernels (csrc/split.hip) on numpy and scipy.ndimage (helper of tests/test_split_*.py; not
collected).  Everything is integer work: the device results are compared with ``np.array_equal``.

The arithmetic (include/stp_hip.h has the same text):
  1. ``edt2``: D2[p] = 0 off the foreground (``mask != 0``), else the smallest |p - q|^2 over the background pixels q of the image (what lies
     outside the image is no background, as in scipy) - the integer behind ``scipy.ndimage.distance_transform_edt``, taken from its
     ``return_indices``; a mask without a zero has D2 = NO_BACKGROUND everywhere (scipy defines nothing useful there).  ``edt2_brute`` is
     the definition itself.
  2. cores = ``D2 > c2``, numbered by ``scipy.ndimage.label`` with the 8-neighbourhood: 1..nc.
  3. ``grow``: the synchronous iteration "every unlabelled foreground pixel with a labelled 8-neighbour takes the smallest neighbouring
     label", until nothing changes.  ``grow_lexicographic`` is the second statement: every pixel takes the label of the lexicographically
     smallest (length of a shortest 8-path inside the mask, label) over all seeds.
  4. the foreground pixels still at 0 (components without a core) are labelled with the 8-neighbourhood, 1..nr, and take nc + that number."""
import heapq

import numpy as np
from scipy import ndimage

from _components_reference import label, serpentine  # noqa: F401

NO_BACKGROUND = 2147483647
EIGHT = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def edt2(mask):
    """-> int32 [h, w]: the exact squared Euclidean distance of every foreground pixel to the nearest zero pixel, 0 off the foreground,
    NO_BACKGROUND everywhere when the mask has no zero."""
    fg = np.asarray(mask) != 0
    if fg.all():
        return np.full(fg.shape, NO_BACKGROUND, np.int32)
    idx = ndimage.distance_transform_edt(fg, return_distances=False, return_indices=True)
    yy, xx = np.indices(fg.shape)
    return ((idx[0] - yy).astype(np.int64) ** 2 + (idx[1] - xx).astype(np.int64) ** 2).astype(np.int32)


def edt2_brute(mask):
    """The definition: per foreground pixel the minimum over all zero pixels (small inputs only)."""
    fg = np.asarray(mask) != 0
    out = np.zeros(fg.shape, np.int32)
    zy, zx = np.nonzero(~fg)
    if len(zy) == 0:
        out[:] = NO_BACKGROUND
        return out
    for y, x in zip(*np.nonzero(fg)):
        out[y, x] = int(((zy - y).astype(np.int64) ** 2 + (zx - x).astype(np.int64) ** 2).min())
    return out


def grow(mask, seeds, return_rounds=False, max_rounds=None):
    """The synchronous iteration -> int32 [h, w] (and, ``return_rounds``, the number of rounds that changed something).  Seeds off the
    foreground are dropped; labels are integers >= 1.  ``max_rounds``: stop after that many rounds."""
    fg = np.asarray(mask) != 0
    cur = np.where(fg, np.asarray(seeds), 0).astype(np.int64)
    h, w = fg.shape
    big = np.iinfo(np.int64).max
    rounds = 0
    while True:
        p = np.full((h + 2, w + 2), big, np.int64)
        p[1:-1, 1:-1] = np.where(cur != 0, cur, big)
        best = np.minimum.reduce([p[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy, dx in EIGHT])
        take = fg & (cur == 0) & (best != big)
        if not take.any() or rounds == max_rounds:
            break
        cur = np.where(take, best, cur)
        rounds += 1
    cur = cur.astype(np.int32)
    return (cur, rounds) if return_rounds else cur


def grow_lexicographic(mask, seeds):
    """The second statement: a search in ascending (path length, label) order - the first pair to reach a pixel is its smallest."""
    fg = np.asarray(mask) != 0
    seeds = np.asarray(seeds)
    h, w = fg.shape
    out = np.zeros((h, w), np.int32)
    heap = [(0, int(seeds[y, x]), int(y), int(x)) for y, x in zip(*np.nonzero(fg & (seeds != 0)))]
    heapq.heapify(heap)
    while heap:
        d, k, y, x = heapq.heappop(heap)
        if out[y, x]:
            continue
        out[y, x] = k
        for dy, dx in EIGHT:
            yy, xx = y + dy, x + dx
            if 0 <= yy < h and 0 <= xx < w and fg[yy, xx] and not out[yy, xx]:
                heapq.heappush(heap, (d + 1, k, yy, xx))
    return out


def cores(mask, c2):
    """-> (uint8 core mask, its int32 labels, nc)."""
    core = (edt2(mask) > int(c2)).astype(np.uint8)
    labels, nc = label(core, 2)
    return core, labels, nc


def split(mask, c2):
    """-> (int32 [h, w] labels, count): steps 1 to 4 of the module text."""
    fg = np.asarray(mask) != 0
    _, seeds, nc = cores(fg, c2)
    out = grow(fg, seeds)
    rest, nr = label(fg & (out == 0), 2)
    out = np.where(rest != 0, rest + nc, out).astype(np.int32)
    return out, nc + nr


def c2_of(radius):
    """The squared core distance of the public radius: floor(r * r)."""
    return int(np.floor(float(radius) * float(radius)))


def two_discs():
    """The hand case: a 40 x 64 image with the discs (cy, cx, r) = (20, 20, 12) and (20, 42, 12), one 8-component of 871 pixels."""
    yy, xx = np.mgrid[0:40, 0:64]
    m = np.zeros((40, 64), bool)
    for cy, cx, r in ((20, 20, 12), (20, 42, 12)):
        m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return m.astype(np.uint8)


def is_8_connected(obj):
    return label(obj, 2)[1] == 1
