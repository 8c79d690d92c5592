"""GPU tests of the boundary-score methods of ``PipelineConfig`` (segmentation_pipeline/segmentation.py over csrc/boundary.hip):
``surface_distances`` against the reference dict, ``score_boundaries`` and ``find_boundary_threshold`` against the host chain they replace
- the ``rle=False`` masks of ``predict_masks_ex``, then tests/_boundary_reference.py - on the untrained model and the six images of
tests/test_object_match_gpu.py.  Integer counters by array equality, floats to 1e-12."""
import math

import numpy as np
import pytest

import _boundary_reference as R
from test_object_match_gpu import Q_SCORED, Q_SWEEP, exp  # noqa: F401  (exp: the module's fixture)

pytestmark = pytest.mark.gpu


def close(got, want):
    if isinstance(want, dict):
        return set(got) == set(want) and all(close(got[k], want[k]) for k in want)
    if isinstance(want, np.ndarray):
        return np.array_equal(got, want)                    # the integer counters
    return got == want or abs(got - want) <= 1e-12          # (== : inf)


def host_rows(e, taus, c2, **mask_kw):
    masks = dict(e.cfg.predict_masks_ex(e.images, fold=0, stage=0, rle=False, **mask_kw))
    return [R.scores(R.counters(masks[i], e.truth[i], c2, 950, 1000), taus, 1000) for i in e.ids]


def mean_of(rows, key, tau=None):
    return float(np.mean([r[key] if tau is None else r[key][tau] for r in rows])) if rows else math.nan


@pytest.mark.parametrize("size", [(37, 53), (70, 133)])
def test_surface_distances_equals_the_reference(size):
    from segmentation_pipeline.segmentation import PipelineConfig as P
    f = R.field(*size)
    for pred, truth, taus, c2, pct in ((f > 0.5, f > 0.6, (1, 2, 3), [1, 4, 9], 95), (f > 0.5, f > 2, (1,), [1], 95),
                                       (f > 2, f > 0.5, (), [], 0), (f > 2, f > 2, (1, 2), [1, 4], 100), (f > 0.5, f > 0.6, (2.5,), [6], 12.5)):
        got = P.surface_distances(pred.astype(np.float32), truth.astype(np.uint8) * 7, tolerances=taus, percentile=pct)
        assert close(got, R.scores(R.counters(pred, truth, c2, int(pct * 10), 1000), taus, 1000))


def test_score_boundaries_equals_the_host_chain(exp):  # noqa: F811
    for kw in ({}, {"min_size": 9}, {"opening": 1, "closing": 1, "area_threshold": 6}):
        kw = dict(kw, threshold=exp.q(Q_SCORED))
        want = host_rows(exp, (1, 2, 3), [1, 4, 9], **kw)
        got = exp.cfg.score_boundaries(exp.ds, 0, **kw)
        assert [i for i, _ in got["images"]] == exp.ids and all(close(g, w) for (_, g), w in zip(got["images"], want))
        assert np.array_equal(got["counts"], np.stack([w["counts"] for w in want])) and got["counts"].dtype == np.int64
        finite = [w for w in want if math.isfinite(w["hd"])]
        assert got["undefined"] == len(want) - len(finite) and finite and max(w["hd"] for w in finite) > 1
        assert all(close(got[k], mean_of(finite, k)) for k in ("hd", "hd_percentile", "assd"))
        assert all(close(got[k][t], mean_of(finite, k, t)) for k in R.SCORES for t in (1, 2, 3))


def test_find_boundary_threshold_equals_the_host_chain(exp):  # noqa: F811
    thresholds = [exp.q(q) for q in Q_SWEEP]
    rows = [host_rows(exp, (2,), [4], threshold=t) for t in thresholds]                       # [threshold][image]
    keep = [all(math.isfinite(cell[i]["hd"]) for cell in rows) for i in range(len(exp.ids))]
    kept = [[r for r, k in zip(cell, keep) if k] for cell in rows]
    for metric in exp.cfg.BOUNDARY_METRICS:
        best, table = exp.cfg.find_boundary_threshold(exp.ds, 0, thresholds=thresholds, metric=metric)
        want = [mean_of(cell, metric, 2 if metric in R.SCORES else None) for cell in kept]
        assert list(table) == thresholds and all(close(table[t], v) for t, v in zip(thresholds, want)) and len(set(want)) > 1
        assert best == thresholds[int((np.argmax if metric in R.SCORES else np.argmin)(want))]
