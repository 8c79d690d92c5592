"""GPU tests of the object-matching kernels (csrc/object_match.hip) at op level: stp_label_match and stp_label_overlaps (with
stp_label_match_workspace_bytes, stp_label_overlaps_workspace_bytes) against their host statement (tests/_object_match_reference.py).
Everything is exact integer work: every comparison is ``np.array_equal`` or ``==``.

Outputs and the workspace carry guard elements around them, pre-filled with a poison value, that must stay untouched; the triples past
``count`` too.  Sizes: 1 x 1, one row and one column past a 64-lane wave, 37 x 53, 64 x 64, 65 x 257 (one past a 64-row and a 256-column
edge), 101 x 101, 130 x 300.  The label images are scipy's 8-connected labels of seeded masks unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest
import torch
from scipy import ndimage

import _object_match_reference as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 70), (70, 1), (37, 53), (64, 64), (65, 257), (101, 101), (130, 300)]
POISON = -5
GUARD = 4
T64_NUM = [500 + 7 * k for k in range(63)] + [1000]                    # T = 64 over den = 1000: 0.5, 0.507, ..., 0.934, 1
THRESHOLDS = {"default": (R.DEFAULT_NUM, R.DEFAULT_DEN), "one": ([7], 7), "half": ([1], 2), "t64": (T64_NUM, 1000)}


def label4(mask):
    labels, _ = ndimage.label(np.asarray(mask) != 0)
    return labels.astype(np.int32)


def patterns(h, w):
    """name -> (pred, truth) int32 label images."""
    s = 1000 * h + w
    zeros, ones = np.zeros((h, w), np.int32), np.ones((h, w), np.int32)
    base = R.label8(R.discs(h, w, s))[0]
    out = {"empty_empty": (zeros, zeros), "empty_full": (zeros, ones), "full_empty": (ones, zeros), "full_full": (ones, ones),
           "self": (base, base)}
    for j, (shift, flip) in enumerate([((0, 0), 0.002), ((1, 0), 0.0), ((0, 1), 0.02), ((1, 2), 0.002), ((2, 2), 0.0)]):
        out["discs_%d" % j] = (R.label8(R.discs(h, w, s, shift, flip, 1))[0], R.label8(R.discs(h, w, s, (0, 0), flip, 2))[0])
    out["salt"] = (R.label8(R.salt(h, w, s + 1))[0], R.label8(R.salt(h, w, s + 2))[0])
    yy, xx = np.mgrid[0:h, 0:w]
    rows = np.where(yy % 2 == 0, yy // 2 + 1, 0).astype(np.int32)      # one-pixel row stripes against one-pixel column stripes:
    cols = np.where(xx % 2 == 0, xx // 2 + 1, 0).astype(np.int32)      # every crossing is a pair of one pixel - the densest table
    out["stripes"] = (rows, cols)
    grid = label4((yy % 2 == 0) & (xx % 2 == 0))                       # every other pixel, 4-connected: the most labels
    out["grid"] = (grid, label4((yy % 2 == 0) & (xx % 2 == 0) | (yy == 0)))
    k = 3 if 3 * max(out["discs_3"][0].max(), out["discs_3"][1].max()) <= h * w else 1
    out["times3"] = (out["discs_3"][0] * k, out["discs_3"][1] * k)     # values need not be contiguous (times 3 wherever h w has room)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def guarded(numel, dtype, fill=POISON):
    """A device buffer with GUARD poison elements on either side -> (whole, the view between the guards)."""
    whole = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD:GUARD + numel]


def guards_intact(whole, fill=POISON):
    a = whole.cpu().numpy()
    return bool((a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all())


def workspace(nbytes):
    """-> (whole, view): ``nbytes`` of workspace with 16 guard bytes on either side (the view stays 8-byte aligned)."""
    assert nbytes > 0
    whole = torch.full((nbytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    view = whole[16:16 + nbytes]
    assert view.data_ptr() % 8 == 0
    return whole, view


def workspace_intact(whole):
    a = whole.cpu().numpy()
    return bool((a[:16] == 0xA5).all() and (a[-16:] == 0xA5).all())


def run_match(pred, truth, label_cap, num, den):
    from segmentation_training_pipeline_amd import ops
    h, w = pred.shape
    T = len(num)
    whole, out = guarded(T + 3, torch.int64)
    ws_whole, ws = workspace(ops.label_match_workspace_bytes(h, w))
    ops.label_match(dev(pred), dev(truth), h, w, label_cap, num, den, out, ws)
    got = out.cpu().numpy().copy()
    assert guards_intact(whole) and workspace_intact(ws_whole)
    return got


def run_overlaps(pred, truth, label_cap):
    """-> (the triples sorted by (a, b), area_p, area_g, out-of-range pixels)."""
    from segmentation_training_pipeline_amd import ops
    h, w = pred.shape
    t_whole, triples = guarded(3 * h * w, torch.int32)
    c_whole, count = guarded(1, torch.int32)
    p_whole, area_p = guarded(label_cap + 1, torch.int32)
    g_whole, area_g = guarded(label_cap + 1, torch.int32)
    o_whole, outside = guarded(1, torch.int64)
    ws_whole, ws = workspace(ops.label_overlaps_workspace_bytes(h, w))
    ops.label_overlaps(dev(pred), dev(truth), h, w, label_cap, triples.view(h * w, 3), count, area_p, area_g, outside, ws)
    n = int(count.cpu().numpy()[0])
    rows = triples.cpu().numpy().reshape(h * w, 3)
    assert 0 <= n <= h * w and (rows[n:] == POISON).all()              # the triples past count are left alone
    for whole in (t_whole, c_whole, p_whole, g_whole, o_whole):
        assert guards_intact(whole)
    assert workspace_intact(ws_whole)
    rows = rows[:n]
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))], area_p.cpu().numpy(), area_g.cpu().numpy(), int(outside.cpu().numpy()[0])


@pytest.fixture(scope="module")
def inputs():
    """Every pattern at every size, computed once and not modified."""
    return {s: patterns(*s) for s in SIZES}


def test_reference_side_properties(inputs):
    """The cases are what they are meant to be: thresholds that discriminate, a dense table, many labels."""
    p, g = inputs[(130, 300)]["stripes"]
    assert len(R.overlaps(p, g, 130 * 300)[0]) == 130 * 300 // 4       # h w / 4 pairs of one pixel each
    p, g = inputs[(101, 101)]["grid"]
    assert p.max() == 51 * 51 and p.max() <= (101 * 101 + 1) // 2
    tp = sum(R.label_match(*inputs[s]["discs_%d" % j], (s[0] * s[1] + 1) // 2) for s in SIZES[3:] for j in range(5))
    print("TP sums per threshold, objects:", tp.tolist())
    assert tp[0] > tp[4] > tp[9] > 0 and tp[0] < tp[11]                # 0 < TP < n_truth, falling with t
    partial = R.label_match(*inputs[(130, 300)]["salt"], 130 * 300)
    assert partial[10] > 50 and partial[11] > 50


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_label_match_equals_the_reference(inputs, size):
    h, w = size
    cap = (h * w + 1) // 2
    for name, (p, g) in inputs[size].items():
        cap_here = h * w if name in ("stripes", "times3") else cap     # (labels above (h w + 1) / 2 occur there)
        assert max(p.max(), g.max()) <= cap_here
        for which in (("default", "t64") if name in ("discs_0", "discs_3", "salt", "full_full", "self") else ("default",)):
            num, den = THRESHOLDS[which]
            got = run_match(p, g, cap_here, num, den)
            assert np.array_equal(got, R.label_match(p, g, cap_here, num, den)), (name, which)
        if name == "self":
            n = len(np.unique(p)) - (1 if (p == 0).any() else 0)
            assert got[:63].tolist() == [n] * 63 and got[63] == 0 and got[64:].tolist() == [n, n, 0]      # every t < 1, not t = 1


@pytest.mark.parametrize("which", ["one", "half"])
def test_label_match_at_the_threshold_bounds(inputs, which):
    num, den = THRESHOLDS[which]
    for size in ((37, 53), (65, 257)):
        h, w = size
        for name in ("full_full", "self", "discs_1", "discs_3", "salt"):
            p, g = inputs[size][name]
            got = run_match(p, g, (h * w + 1) // 2, num, den)
            assert np.array_equal(got, R.label_match(p, g, (h * w + 1) // 2, num, den)), (size, name)
            if which == "one":
                assert got[0] == 0                                     # t = 1 matches nothing, not even IoU 1
            elif name in ("full_full", "self"):
                assert got[0] == got[1] == got[2] > 0


def test_label_values_above_the_cap_are_background_and_counted(inputs):
    for size in ((37, 53), (130, 300)):
        h, w = size
        p, g = (a.copy() for a in inputs[size]["discs_3"])
        cap = int(max(p.max(), g.max())) // 2                          # half of the labels lie above it
        p[0, 0], g[h - 1, w - 1], p[h // 2, w // 2] = -1, np.iinfo(np.int32).max, np.iinfo(np.int32).min
        outside = ((p < 0) | (p > cap) | (g < 0) | (g > cap))
        assert outside.sum() > 3
        got = run_match(p, g, cap, *THRESHOLDS["default"])
        assert got[12] == np.count_nonzero(outside)
        pz, gz = np.where((p < 0) | (p > cap), 0, p), np.where((g < 0) | (g > cap), 0, g)
        assert np.array_equal(got[:12], R.label_match(pz, gz, cap)[:12]) and np.array_equal(got, R.label_match(p, g, cap))
        triples, area_p, area_g, n_out = run_overlaps(p, g, cap)
        want = R.overlaps(p, g, cap)
        assert np.array_equal(triples, want[0]) and np.array_equal(area_p, want[1]) and np.array_equal(area_g, want[2]) and n_out == want[3]
    got = run_match(np.full((5, 70), 3, np.int32), np.full((5, 70), 3, np.int32), 0, [1], 2)      # label_cap 0: everything is outside
    assert got.tolist() == [0, 0, 0, 350]


def test_two_launches_give_identical_bytes(inputs):
    for size, name in (((130, 300), "salt"), ((130, 300), "stripes"), ((65, 257), "discs_3")):
        p, g = inputs[size][name]
        cap = size[0] * size[1]
        first, second = run_match(p, g, cap, *THRESHOLDS["default"]), run_match(p, g, cap, *THRESHOLDS["default"])
        assert first.tobytes() == second.tobytes()
        a, b = run_overlaps(p, g, cap), run_overlaps(p, g, cap)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_label_overlaps_equals_the_reference(inputs, size):
    h, w = size
    for name, (p, g) in inputs[size].items():
        cap = int(max(p.max(), g.max(), 0))                            # the areas have label_cap + 1 entries: the smallest that serves
        triples, area_p, area_g, outside = run_overlaps(p, g, cap)
        want = R.overlaps(p, g, cap)
        assert triples.dtype == np.int32 and np.array_equal(triples, want[0]), name
        assert np.array_equal(area_p, want[1]) and np.array_equal(area_g, want[2]) and outside == 0, name


def test_object_overlaps_returns_sorted_triples_and_areas(inputs):
    from segmentation_pipeline.segmentation import PipelineConfig
    p, g = inputs[(65, 257)]["times3"]
    pairs, area_p, area_g = PipelineConfig.object_overlaps(p, g.astype(np.int64))
    want = R.overlaps(p, g, int(max(p.max(), g.max())))
    assert np.array_equal(pairs, want[0]) and np.array_equal(area_p, want[1]) and np.array_equal(area_g, want[2])
    assert len(pairs) > 10 and (np.diff(pairs[:, 0]) >= 0).all()


# ------------------------------------------------------------------------------------------------ refusals: none launches anything
def test_refusals():
    from segmentation_training_pipeline_amd import _lib, ops
    h, w = 37, 53
    lab = torch.ones((h, w), dtype=torch.int32, device="cuda")
    out = torch.full((67,), POISON, dtype=torch.int64, device="cuda")
    triples = torch.full((h * w, 3), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
    areas = torch.full((2, h * w + 1), POISON, dtype=torch.int32, device="cuda")
    outside = torch.full((1,), POISON, dtype=torch.int64, device="cuda")
    lib = _lib.load()
    size = ops.label_match_workspace_bytes(h, w)
    assert size == lib.stp_label_match_workspace_bytes(h, w) == ops.label_overlaps_workspace_bytes(h, w) == lib.stp_label_overlaps_workspace_bytes(h, w)
    ws = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()                                           # noqa: E731
    BADARG, WORKSPACE = -1, -3
    arr = lambda *v: (C.c_int32 * len(v))(*v)                            # noqa: E731

    def match(num, T, den, pred=p(lab), truth=p(lab), hh=h, ww=w, cap=h * w, o=p(out), wsp=p(ws), nbytes=size):
        return lib.stp_label_match(pred, truth, hh, ww, cap, num, T, den, o, wsp, nbytes, None)

    def overlaps(pred=p(lab), hh=h, ww=w, cap=h * w, tr=p(triples), cnt=p(count), capacity=h * w, ap=p(areas[0]), ag=p(areas[1]),
                 oo=p(outside), wsp=p(ws), nbytes=size):
        return lib.stp_label_overlaps(pred, p(lab), hh, ww, cap, tr, cnt, capacity, ap, ag, oo, wsp, nbytes, None)
    ok = arr(10, 15)
    assert match(arr(9), 1, 20) == BADARG                               # 2 * num < den
    assert match(arr(21), 1, 20) == BADARG                              # num > den
    assert match(arr(15, 15), 2, 20) == BADARG and match(arr(15, 10), 2, 20) == BADARG      # not ascending
    assert match(ok, 0, 20) == BADARG and match(arr(*range(500, 565)), 65, 1000) == BADARG      # T = 0, T = 65
    assert match(ok, 2, 0) == BADARG and match(arr(1001), 1, 1001) == BADARG                    # den = 0, den = 1001
    assert match(ok, 2, 20, pred=None) == BADARG and match(ok, 2, 20, truth=None) == BADARG     # NULL pointers
    assert match(None, 2, 20) == BADARG and match(ok, 2, 20, o=None) == BADARG and match(ok, 2, 20, wsp=None) == BADARG
    assert match(ok, 2, 20, hh=0) == BADARG and match(ok, 2, 20, ww=0) == BADARG and match(ok, 2, 20, hh=-1) == BADARG
    assert match(ok, 2, 20, cap=-1) == BADARG and match(ok, 2, 20, cap=h * w + 1) == BADARG
    assert match(ok, 2, 20, nbytes=size - 1) == WORKSPACE               # one byte below the query
    assert overlaps(pred=None) == BADARG and overlaps(tr=None) == BADARG and overlaps(cnt=None) == BADARG
    assert overlaps(ap=None) == BADARG and overlaps(ag=None) == BADARG and overlaps(oo=None) == BADARG and overlaps(wsp=None) == BADARG
    assert overlaps(hh=0) == BADARG and overlaps(ww=-2) == BADARG and overlaps(cap=h * w + 1) == BADARG
    assert overlaps(capacity=h * w - 1) == BADARG                       # capacity one short
    assert overlaps(nbytes=size - 1) == WORKSPACE
    for query in (ops.label_match_workspace_bytes, ops.label_overlaps_workspace_bytes):
        assert query(0, w) == 0 and query(h, 0) == 0 and query(1 << 16, 1 << 15) == 0            # h * w = 2^31 is refused
    with pytest.raises(_lib.StpError, match="BADARG"):
        ops.label_match(lab, lab, h, w, h * w, [9], 20, out, ws)
    with pytest.raises(_lib.StpError, match="WORKSPACE"):
        ops.label_overlaps(lab, lab, h, w, h * w, triples, count, areas[0], areas[1], outside, ws[:size - 8])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all() and (triples.cpu().numpy() == POISON).all()       # nothing was launched
    assert (count.cpu().numpy() == POISON).all() and (areas.cpu().numpy() == POISON).all() and (outside.cpu().numpy() == POISON).all()
    assert (ws.cpu().numpy() == 0xA5).all()
