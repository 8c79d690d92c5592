"""CPU tests of the boundary-score path's host side (segmentation_pipeline/segmentation.py over csrc/boundary.hip): the reference's
integer percentile and fixed-point mean against numpy's float statements, the refusals of the three public methods, the signatures."""
import ctypes as C
import inspect

import numpy as np
import pytest

import _boundary_reference as R
from test_object_match_host import config, no_model_files  # noqa: F401  (no_model_files: a fixture)


@pytest.mark.parametrize("size", [(37, 53), (64, 64), (70, 133), (129, 67), (65, 257)])
def test_reference_percentile_and_assd_against_numpy(size):
    f = R.field(*size)
    d0, d1, n0, n1 = R.squared_distances(f > 0.5, f > 0.6)
    both = np.sqrt(np.concatenate([d0, d1]).astype(np.float64))
    assert min(n0, n1) >= 300 and len(np.unique(both)) >= 30      # neither surface is small, and the distances are many
    for num, p in ((950, 95), (0, 0), (1000, 100), (500, 50), (125, 12.5)):
        res = R.scores(R.counters(f > 0.5, f > 0.6, [1, 4, 9], num, 1000), (1, 2, 3), 1000)
        assert abs(res["hd_percentile"] - np.percentile(both, p)) <= 1e-12
        assert 0 <= both.mean() - res["assd"] < 1 / 256 and res["hd"] == both.max()
        assert res["surface_dice"][2] == ((d0 <= 4).sum() + (d1 <= 4).sum()) / (n0 + n1)


def test_refusals_come_before_a_model_is_loaded(no_model_files):  # noqa: F811
    ds, m = object(), np.ones((4, 5), np.uint8)
    cfg, softmax = config(), config(classes=3, activation="softmax")
    for kw, what in (({"tolerances": (2, 1)}, "ascend"), ({"tolerances": (1, 1.2)}, "ascend"), ({"tolerances": (-1,)}, "tolerances"),
                     ({"tolerances": (True,)}, "tolerances"), ({"tolerances": range(17)}, "16"), ({"percentile": 101}, "percentile"),
                     ({"percentile": 94.55}, "percentile"), ({"percentile": None}, "percentile")):
        for call in (lambda: cfg.surface_distances(m, m, **kw), lambda: cfg.score_boundaries(ds, 0, **kw)):
            with pytest.raises(ValueError, match=what):
                call()
    for kw, what in (({"channel": 1}, "channel"), ({"opening": 8}, "opening"), ({"min_size": -1}, "min_size"), ({"metric": "dice"}, "metric"),
                     ({"thresholds": [0.5, 0.25]}, "thresholds"), ({"tolerance": -2}, "tolerances"), ({"percentile": -1}, "percentile")):
        with pytest.raises(ValueError, match=what):
            cfg.find_boundary_threshold(ds, 0, **kw)
    for call in (lambda: cfg.score_boundaries(ds, 0, closing=1.5), lambda: softmax.score_boundaries(ds, 0, threshold=0.25),
                 lambda: softmax.find_boundary_threshold(ds, 0, thresholds=[0.5]), lambda: cfg.surface_distances(m, m[:3]),
                 lambda: cfg.surface_distances(m[0], m[0]), lambda: cfg.surface_distances(m[:0], m[:0])):
        with pytest.raises(ValueError):
            call()


def test_signatures():
    from segmentation_pipeline.segmentation import PipelineConfig as P
    from segmentation_training_pipeline_amd import _lib, ops
    i32, vp, sz = _lib.i32, _lib.vp, _lib.sz
    assert _lib.SIGNATURES["stp_surface_distances_workspace_bytes"] == (sz, [i32, i32])
    assert _lib.SIGNATURES["stp_surface_distances"] == (i32, [vp, vp, i32, i32, C.POINTER(i32), i32, i32, i32, vp, vp, sz, vp])
    assert list(inspect.signature(P.surface_distances).parameters) == ["pred_mask", "truth_mask", "tolerances", "percentile"]
    p = inspect.signature(P.score_boundaries).parameters
    assert list(p)[1:] == ["ds", "fold", "stage", "negatives", "ttflips", "threshold", "opening", "closing", "channel", "min_size",
                           "area_threshold", "tolerances", "percentile"]
    assert [p[k].default for k in list(p)[3:]] == [-1, "real", None, 0.5, 0, 0, 0, 0, 0, (1, 2, 3), 95]
    assert "tolerance" in inspect.signature(P.find_boundary_threshold).parameters
    assert ops.surface_distances_workspace_bytes(64, 64) >= 20 * 4096 and ops.surface_distances_workspace_bytes(5, 32768) == 0
