"""GPU tests of the connected-component kernels (csrc/components.hip) at op level: stp_mask_label, stp_mask_area_filter and stp_label_rle
(with stp_mask_label_workspace_bytes, stp_mask_area_filter_workspace_bytes, stp_label_rle_workspace_bytes) against their host statements
(tests/_components_reference.py: scipy.ndimage.label, skimage's remove_small_* restated, impl.rle).  Everything is exact integer work:
every comparison is ``np.array_equal`` or string equality.

Outputs are pre-filled with a poison value, carry one guard element past their end and - the run triples - must be untouched past
``count``.  The conditions that keep a case from being vacuous (component counts that differ between the connectivities, pixels removed
and filled, both kinds of column wrap) are asserted on the reference side.

Inputs: the seeded Gaussian field of test_masks_ops_gpu.py above 0.35 / 0.5 at 3 x 5 (smaller than a 64-pixel row segment and than every
tile), 64 x 64 (one tile), 37 x 53, 70 x 133 and 129 x 67 (odd, several segments per row, several tiles, several workgroups); two
salt-and-pepper images drawn in turn from ONE ``default_rng(5)`` (p = 0.45, then p = 0.6); a serpentine - one component whose path
crosses every segment and workgroup border many times, the deep chain for ``find`` - and its transpose; a checkerboard (the most
components an image can have); all zeros, all ones and images of one row, one column, one pixel."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import _components_reference as R

pytestmark = pytest.mark.gpu

FIELD_SIZES = [(3, 5), (64, 64), (37, 53), (70, 133), (129, 67)]
THRESHOLDS = (0.35, 0.5)
POISON = -5


def field(h, w):
    rng = np.random.default_rng(1000 * h + w)
    f = ndimage.gaussian_filter(rng.random((h, w)), 2.0)
    return ((f - f.min()) / (f.max() - f.min())).astype(np.float32)


def make_inputs():
    out = {}
    for s in FIELD_SIZES:
        f = field(*s)
        for thr in THRESHOLDS:
            out["field_%dx%d_%g" % (s + (thr,))] = (f > thr).astype(np.uint8)
    rng = np.random.default_rng(5)                                          # ONE generator: the second image is its second draw
    out["salt_0.45"] = (rng.random((70, 133)) < 0.45).astype(np.uint8)
    out["salt_0.6"] = (rng.random((70, 133)) < 0.6).astype(np.uint8)
    out["serpentine"] = R.serpentine(67, 71)
    out["serpentine_T"] = np.ascontiguousarray(R.serpentine(67, 71).T)
    out["checkerboard"] = (np.indices((33, 35)).sum(axis=0) % 2 == 0).astype(np.uint8)
    for s in ((1, 1), (1, 130), (130, 1), (37, 53)):
        out["zeros_%dx%d" % s] = np.zeros(s, np.uint8)
        out["ones_%dx%d" % s] = np.full(s, 255, np.uint8)                   # any non-zero byte is mask
    out["dots_1x130"] = (np.arange(130)[None, :] % 3 != 0).astype(np.uint8)
    out["dots_130x1"] = (np.arange(130)[:, None] % 3 != 0).astype(np.uint8)
    return out


INPUTS = make_inputs()
NAMES = sorted(INPUTS)


@pytest.fixture(scope="module")
def scipy_labels():
    """(labels, count) of every input at both connectivities, computed once and not modified."""
    return {(n, c): R.label(INPUTS[n], c) for n in NAMES for c in (1, 2)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def workspace(nbytes):
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 8 == 0
    return ws


def run_label(mask, connectivity, invert=0):
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    labels = torch.full((h * w + 1,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((2,), POISON, dtype=torch.int32, device="cuda")
    ops.mask_label(dev(mask), h, w, connectivity, invert, labels[:h * w], count[:1], workspace(ops.mask_label_workspace_bytes(h, w)))
    got, n = labels.cpu().numpy(), count.cpu().numpy()
    assert got[-1] == POISON and n[1] == POISON                              # the guard elements
    return got[:-1].reshape(h, w), int(n[0])


def run_area(mask, connectivity, invert, min_size, in_place=False):
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    ws = workspace(ops.mask_area_filter_workspace_bytes(h, w))
    if in_place:
        buf = torch.cat([dev(mask).reshape(-1), torch.full((1,), 7, dtype=torch.uint8, device="cuda")])
        ops.mask_area_filter(buf[:h * w], buf[:h * w], h, w, connectivity, invert, min_size, ws)
    else:
        buf = torch.full((h * w + 1,), 7, dtype=torch.uint8, device="cuda")
        ops.mask_area_filter(dev(mask), buf[:h * w], h, w, connectivity, invert, min_size, ws)
    got = buf.cpu().numpy()
    assert got[-1] == 7
    return got[:-1].reshape(h, w)


def run_label_rle(labels):
    """-> (count, the int32 triples as written; the triples past count must be left alone)."""
    from segmentation_training_pipeline_amd import ops
    h, w = labels.shape
    runs = torch.full((h * w + 1, 3), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((2,), POISON, dtype=torch.int32, device="cuda")
    ops.label_rle(dev(labels.astype(np.int32)), h, w, runs[:h * w], count[:1], workspace(ops.label_rle_workspace_bytes(h, w)))
    n, got = count.cpu().numpy(), runs.cpu().numpy()
    assert n[1] == POISON and 0 <= n[0] <= h * w and (got[n[0]:] == POISON).all()
    return int(n[0]), got[:n[0]]


# ------------------------------------------------------------------------------------------------ the inputs are what they are meant to be
def test_reference_side_properties(scipy_labels):
    counts = {n: (scipy_labels[n, 1][1], scipy_labels[n, 2][1]) for n in NAMES}
    assert counts["salt_0.45"] == (903, 105) and counts["salt_0.6"] == (287, 11)          # the two connectivities must differ
    assert counts["field_70x133_0.5"] == (8, 7) and counts["field_129x67_0.5"] == (39, 37)
    assert counts["checkerboard"] == (578, 1) and 578 == (33 * 35 + 1) // 2                # the most a 33 x 35 image can have
    assert counts["serpentine"] == counts["serpentine_T"] == (1, 1) and int(INPUTS["serpentine"].sum()) == 2447
    salt = INPUTS["salt_0.45"]
    assert [int(salt.sum()) - int(R.remove_small_objects(salt, m).sum()) for m in (2, 9, 64)] == [452, 1642, 4068]
    assert int(R.remove_small_holes(salt, 9).sum()) - int(salt.sum()) == 761
    gaps = np.bincount(R.label(INPUTS["serpentine"], 1, invert=1)[0].ravel())[1:]
    assert gaps.tolist() == [70] * 33                                                      # 33 gaps of exactly 70 pixels
    for n in ("field_70x133_0.5", "field_129x67_0.5"):                                    # holes of 1..25 pixels
        holes = np.bincount(R.label(INPUTS[n], 1, invert=1)[0].ravel())[1:]
        assert ((holes >= 1) & (holes <= 25)).sum() >= 3
    assert R.column_wraps(scipy_labels["field_70x133_0.5", 1][0]) == (32, 28)              # both wrap rules of stp_label_rle


# ------------------------------------------------------------------------------------------------ stp_mask_label
@pytest.mark.parametrize("name", NAMES)
def test_label_equals_scipy(scipy_labels, name):
    m = INPUTS[name]
    for connectivity in (1, 2):
        want, n = scipy_labels[name, connectivity]
        got, count = run_label(m, connectivity)
        assert count == n and np.array_equal(got, want), (name, connectivity)
        want, n = R.label(m, connectivity, invert=1)
        got, count = run_label(m, connectivity, invert=1)
        assert count == n and np.array_equal(got, want), (name, connectivity, "invert")


@pytest.mark.parametrize("name", ["salt_0.45", "serpentine", "field_129x67_0.5"])
def test_label_is_the_same_from_run_to_run(name):
    first = run_label(INPUTS[name], 2)
    second = run_label(INPUTS[name], 2)
    assert first[1] == second[1] and first[0].tobytes() == second[0].tobytes()
    a, b = run_area(INPUTS[name], 1, 0, 9), run_area(INPUTS[name], 1, 0, 9)
    assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ stp_mask_area_filter
@pytest.mark.parametrize("name", NAMES)
def test_area_filter_equals_the_reference(name):
    m = INPUTS[name]
    h, w = m.shape
    for connectivity in (1, 2):
        for min_size in (0, 1, 2, 9, 64, h * w + 1):
            want = R.remove_small_objects(m, min_size, connectivity)
            assert np.array_equal(run_area(m, connectivity, 0, min_size), want), (name, connectivity, min_size)
            want = R.remove_small_holes(m, min_size, connectivity)
            assert np.array_equal(run_area(m, connectivity, 1, min_size), want), (name, connectivity, min_size, "holes")
    assert np.array_equal(run_area(m, 1, 0, 0), (m != 0).astype(np.uint8))                 # min_size 0: the binarised source


@pytest.mark.parametrize("name", ["salt_0.45", "field_70x133_0.5", "field_129x67_0.5", "serpentine", "ones_1x130"])
def test_area_filter_in_place_and_chained(name):
    m = INPUTS[name]
    for invert in (0, 1):
        for min_size in (1, 9, 64):
            assert np.array_equal(run_area(m, 1, invert, min_size, in_place=True), run_area(m, 1, invert, min_size))
    want = R.remove_small_holes(R.remove_small_objects(m, 64), 64)                         # the README's clean-up
    assert np.array_equal(run_area(run_area(m, 1, 0, 64), 1, 1, 64, in_place=True), want)


def test_area_filter_strict_less_than():
    s = INPUTS["serpentine"]                                                               # gaps of exactly 70 pixels
    assert np.array_equal(run_area(s, 1, 1, 70), s) and np.array_equal(R.remove_small_holes(s, 70), s)
    assert run_area(s, 1, 1, 71).all() and R.remove_small_holes(s, 71).all()
    assert np.array_equal(run_area(s, 1, 0, 2447), s) and run_area(s, 1, 0, 2448).sum() == 0


# ------------------------------------------------------------------------------------------------ stp_label_rle
def check_label_rle(labels):
    n, runs = run_label_rle(labels)
    want = R.label_runs(labels)
    assert n == len(want) and np.array_equal(runs, want)
    return runs


@pytest.mark.parametrize("name", NAMES)
def test_label_rle_of_scipys_label_images(scipy_labels, name):
    for connectivity in (1, 2):
        labels, count = scipy_labels[name, connectivity]
        runs = check_label_rle(labels)
        assert R.group_runs(runs, count) == [R.rle_encode(labels == k) for k in range(1, count + 1)]
        if connectivity == 2:
            assert R.group_runs(runs, count) == R.multi_rle(INPUTS[name])


def test_label_rle_of_the_densest_image():
    labels = np.random.default_rng(9).integers(0, 4, (37, 53)).astype(np.int32)            # nearly every pixel is its own run
    runs = check_label_rle(labels)
    assert len(runs) > 37 * 53 // 2 and (runs[:, 2] == 1).sum() > len(runs) // 2
    assert R.group_runs(runs, 3) == [R.rle_encode(labels == k) for k in (1, 2, 3)]


def test_label_then_rle_is_multi_rle_encode():
    for name in ("salt_0.45", "field_129x67_0.5", "checkerboard", "zeros_37x53"):
        labels, count = run_label(INPUTS[name], 2)
        n, runs = run_label_rle(labels)
        assert R.group_runs(runs, count) == R.multi_rle(INPUTS[name]), name


def test_image_of_several_scan_passes():
    """520 x 515 = 267800 pixels: 1047 workgroups of 256 pixels for the root counts and 262 of 1024 for the run counts - the one-workgroup
    scans of both make more than one pass of 256 - with blobs, specks and holes."""
    h, w = 520, 515
    m = ((field(h, w) > 0.5) ^ (np.random.default_rng(3).random((h, w)) < 0.02)).astype(np.uint8)
    for connectivity in (1, 2):
        want, n = R.label(m, connectivity)
        assert n > 256                                                                     # roots in many of the 1047 workgroups
        got, count = run_label(m, connectivity)
        assert count == n and np.array_equal(got, want)
        runs = check_label_rle(want)
        assert len(runs) > 262 * 16                                                        # runs in every workgroup of 1024 values
    for invert, reference in ((0, R.remove_small_objects), (1, R.remove_small_holes)):
        want = reference(m, 9)
        assert not np.array_equal(want, m)
        assert np.array_equal(run_area(m, 1, invert, 9), want) and np.array_equal(run_area(m, 1, invert, 9, in_place=True), want)


# ------------------------------------------------------------------------------------------------ refusals: none launches anything
def test_refusals():
    from segmentation_training_pipeline_amd import _lib, ops
    h, w = 37, 53
    img = dev(INPUTS["ones_37x53"])
    labels = torch.full((h * w,), POISON, dtype=torch.int32, device="cuda")
    count = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
    dst = torch.full((h * w,), 7, dtype=torch.uint8, device="cuda")
    runs = torch.full((h * w, 3), POISON, dtype=torch.int32, device="cuda")
    lab_in = torch.ones((h, w), dtype=torch.int32, device="cuda")
    lib = _lib.load()
    sizes = {"label": ops.mask_label_workspace_bytes(h, w), "area": ops.mask_area_filter_workspace_bytes(h, w),
             "rle": ops.label_rle_workspace_bytes(h, w)}
    assert sizes == {"label": lib.stp_mask_label_workspace_bytes(h, w), "area": lib.stp_mask_area_filter_workspace_bytes(h, w),
                     "rle": lib.stp_label_rle_workspace_bytes(h, w)}
    ws = workspace(max(sizes.values()))
    p, big = (lambda t: t.data_ptr()), max(sizes.values())
    BADARG, WORKSPACE = -1, -3
    for connectivity in (0, 3):
        assert lib.stp_mask_label(p(img), h, w, connectivity, 0, p(labels), p(count), p(ws), big, None) == BADARG
        assert lib.stp_mask_area_filter(p(img), p(dst), h, w, connectivity, 0, 9, p(ws), big, None) == BADARG
    assert lib.stp_mask_area_filter(p(img), p(dst), h, w, 1, 0, -1, p(ws), big, None) == BADARG            # negative min_size
    assert lib.stp_label_rle(p(lab_in), h, w, p(runs), p(count), h * w - 1, p(ws), big, None) == BADARG      # capacity one short
    assert lib.stp_mask_label(p(img), h, w, 1, 0, p(labels), p(count), p(ws), sizes["label"] - 1, None) == WORKSPACE
    assert lib.stp_mask_area_filter(p(img), p(dst), h, w, 1, 0, 9, p(ws), sizes["area"] - 1, None) == WORKSPACE
    assert lib.stp_label_rle(p(lab_in), h, w, p(runs), p(count), h * w, p(ws), sizes["rle"] - 1, None) == WORKSPACE
    assert lib.stp_mask_label(None, h, w, 1, 0, p(labels), p(count), p(ws), big, None) == BADARG             # NULL pointers
    assert lib.stp_mask_label(p(img), h, w, 1, 0, p(labels), None, p(ws), big, None) == BADARG
    assert lib.stp_mask_area_filter(p(img), None, h, w, 1, 0, 9, p(ws), big, None) == BADARG
    assert lib.stp_label_rle(p(lab_in), h, w, None, p(count), h * w, p(ws), big, None) == BADARG
    assert lib.stp_label_rle(p(lab_in), h, w, p(runs), p(count), h * w, None, big, None) == BADARG
    assert lib.stp_mask_label(p(img), 0, w, 1, 0, p(labels), p(count), p(ws), big, None) == BADARG           # h = 0
    assert lib.stp_mask_area_filter(p(img), p(dst), 0, w, 1, 0, 9, p(ws), big, None) == BADARG
    assert lib.stp_label_rle(p(lab_in), 0, w, p(runs), p(count), h * w, p(ws), big, None) == BADARG
    for query in (ops.mask_label_workspace_bytes, ops.mask_area_filter_workspace_bytes, ops.label_rle_workspace_bytes):
        assert query(0, w) == 0 and query(1 << 16, 1 << 15) == 0                                             # h * w = 2^31 is refused
    with pytest.raises(_lib.StpError, match="BADARG"):
        ops.mask_label(img, h, w, 3, 0, labels, count, ws)
    with pytest.raises(_lib.StpError, match="WORKSPACE"):
        ops.label_rle(lab_in, h, w, runs, count, ws[:sizes["rle"] - 8])
    torch.cuda.synchronize()
    assert (labels.cpu().numpy() == POISON).all() and (count.cpu().numpy() == POISON).all()                  # nothing was launched
    assert (dst.cpu().numpy() == 7).all() and (runs.cpu().numpy() == POISON).all()
