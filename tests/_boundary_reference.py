"""The host statement of the boundary scores (include/stp_hip.h, csrc/boundary.hip): surfaces by scipy's binary erosion, the two scipy
distance transforms as exact integers, the counters, ``math.isqrt`` for q, (lo, hi, rem) from the sorted values, and the dict that
``PipelineConfig.surface_distances`` returns.  Restated here once; not the code under test."""
import math

import numpy as np
from scipy import ndimage

SCORES = ("boundary_precision", "boundary_recall", "boundary_f", "surface_dice")


def field(h, w):
    """The seeded Gaussian field of tests/test_measure_ops_gpu.py."""
    rng = np.random.default_rng(1000 * h + w)
    f = ndimage.gaussian_filter(rng.random((h, w)), 2.0)
    return ((f - f.min()) / (f.max() - f.min())).astype(np.float32)


def squared_distances(pred, truth):
    """-> (D2 of S(pred) to S(truth), D2 of S(truth) to S(pred), n0, n1): int64 arrays, both None when a surface is empty."""
    sp, st = (m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(2, 1), border_value=0) for m in (pred != 0, truth != 0))
    if not sp.any() or not st.any():
        return None, None, int(sp.sum()), int(st.sum())
    to_t = np.rint(ndimage.distance_transform_edt(~st) ** 2).astype(np.int64)
    to_p = np.rint(ndimage.distance_transform_edt(~sp) ** 2).astype(np.int64)
    return to_t[sp], to_p[st], int(sp.sum()), int(st.sum())


def counters(pred, truth, c2, pct_num, pct_den):
    """stp_surface_distances' ``out``: int64 [2 * (3 + T) + 3]."""
    d0, d1, n0, n1 = squared_distances(pred, truth)
    if d0 is None:
        return np.array([n0, -1, 0] + [0] * len(c2) + [n1, -1, 0] + [0] * len(c2) + [-1, -1, 0], np.int64)
    out = []
    for n, d in ((n0, d0), (n1, d1)):
        out += [n, int(d.max()), sum(math.isqrt(int(v) << 16) for v in d)] + [int((d <= c).sum()) for c in c2]
    both = np.sort(np.concatenate([d0, d1]))
    pos = pct_num * (len(both) - 1)
    j = pos // pct_den
    return np.array(out + [int(both[j]), int(both[min(j + 1, len(both) - 1)]), pos % pct_den], np.int64)


def scores(out, tolerances, pct_den):
    """The dict of ``PipelineConfig.surface_distances`` from the counters (``tolerances``: the public pixel tolerances, in c2's order)."""
    T = len(tolerances)
    a, b = [int(v) for v in out[:3 + T]], [int(v) for v in out[3 + T:2 * (3 + T)]]
    lo, hi, rem = (int(v) for v in out[2 * (3 + T):])
    if a[0] == 0 or b[0] == 0:                      # both empty: distances 0, scores 1; one empty: inf and 0
        res = dict.fromkeys(("hd", "hd_percentile", "assd"), 0.0 if a[0] == b[0] else math.inf)
        res.update({name: {tau: 1.0 if a[0] == b[0] else 0.0 for tau in tolerances} for name in SCORES})
        return dict(res, counts=np.asarray(out, np.int64))
    res = {"hd": math.sqrt(max(a[1], b[1])), "hd_percentile": math.sqrt(lo) + rem / pct_den * (math.sqrt(hi) - math.sqrt(lo)),
           "assd": (a[2] + b[2]) / (256 * (a[0] + b[0])), "counts": np.asarray(out, np.int64)}
    p, r = [a[3 + k] / a[0] for k in range(T)], [b[3 + k] / b[0] for k in range(T)]
    res["boundary_precision"], res["boundary_recall"] = dict(zip(tolerances, p)), dict(zip(tolerances, r))
    res["boundary_f"] = {tau: 2 * x * y / (x + y) if x + y > 0 else 0.0 for tau, x, y in zip(tolerances, p, r)}
    res["surface_dice"] = {tau: (a[3 + k] + b[3 + k]) / (a[0] + b[0]) for k, tau in enumerate(tolerances)}
    return res
