"""GPU tests of the mask kernels (csrc/mask.hip) at op level: stp_mask_threshold, stp_mask_morph, stp_mask_rle (with
stp_mask_rle_workspace_bytes) and stp_threshold_counts (with stp_threshold_counts_workspace_bytes) against their host statements
(tests/_mask_reference.py: numpy, scipy.ndimage, impl.rle).  Everything is exact integer work: every comparison is ``np.array_equal`` or
string equality.

Inputs: a seeded ``gaussian_filter(rng.random((h, w)), 2.0)`` stretched to [0, 1] as float32 at 3 x 5 (smaller than the disk and than
every tile), 37 x 53 and 70 x 133 (odd, no multiple of a tile, more than one RLE tile, more than one bit word per column) and 64 x 64
(exactly one tile).  The conditions that keep a case from being vacuous - the mask has both values, the opening changes it, a run goes
on across a column boundary - are asserted on the reference side."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import _mask_reference as R

pytestmark = pytest.mark.gpu

SIZES = [(3, 5), (37, 53), (70, 133), (64, 64)]
BIG = [(37, 53), (70, 133)]
THRESHOLDS = (0.35, 0.5)
MORPH_TILE = (64, 256)          # rows x columns of output pixels a workgroup of stp_mask_morph owns (MORPH_ROWS, 64 * MORPH_WORDS)
RLE_TILE = (64, 64)             # the tile stp_mask_rle transposes; a workgroup of its later launches owns 256 words = 16384 pixels


def field(h, w):
    rng = np.random.default_rng(1000 * h + w)
    f = ndimage.gaussian_filter(rng.random((h, w)), 2.0)
    return ((f - f.min()) / (f.max() - f.min())).astype(np.float32)


@pytest.fixture(scope="module")
def fields():
    return {s: field(*s) for s in SIZES}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def run_threshold(arr, channel, mode, thr, out_ld=None, offset=0):
    """-> the mask; the bytes between the rows and around the buffer must be left alone."""
    from segmentation_training_pipeline_amd import ops
    h, w, C = arr.shape
    ld = w if out_ld is None else out_ld
    buf = torch.full((offset + h * ld + 16,), 7, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    ops.mask_threshold(dev(arr), h, w, C, channel, mode, thr, buf[offset:], ld)
    got = buf.cpu().numpy()
    body = got[offset:offset + h * ld].reshape(h, ld)
    assert (got[:offset] == 7).all() and (got[offset + (h - 1) * ld + w:] == 7).all() and (body[:-1, w:] == 7).all()
    return body[:, :w]


def run_morph(mask, r, op):
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    dst = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
    ops.mask_morph(dev(mask), dst, h, w, r, op)
    return dst.cpu().numpy()


def run_rle(mask, capacity=None):
    """-> (count, the int32 pairs as written; the pairs past count must be left alone)."""
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    cap = (h * w + 1) // 2 if capacity is None else capacity
    runs = torch.full((cap + 1, 2), -5, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    nbytes = ops.mask_rle_workspace_bytes(h, w)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ops.mask_rle(dev(mask), h, w, runs[:cap], count, ws)
    n = int(count.item())
    got = runs.cpu().numpy()
    assert 0 <= n <= cap and (got[n:] == -5).all()
    return n, got[:n]


def run_counts(arr, target, thresholds, channel=0):
    from segmentation_training_pipeline_amd import ops
    h, w, C = arr.shape
    T = len(thresholds)
    counts = torch.full((T, 2), -5, dtype=torch.int64, device="cuda")
    totals = torch.full((2,), -5, dtype=torch.int64, device="cuda")
    ws = torch.empty(ops.threshold_counts_workspace_bytes(T), dtype=torch.uint8, device="cuda")
    ops.threshold_counts(dev(arr), dev(target.astype(np.uint8)), h, w, C, channel, thresholds, counts, totals, ws)
    return counts.cpu().numpy(), totals.cpu().numpy()


def three_channels(f):
    rng = np.random.default_rng(7)
    return np.stack([rng.random(f.shape).astype(np.float32), 1 - f, f], axis=2)


# ------------------------------------------------------------------------------------------------ stp_mask_threshold
@pytest.mark.parametrize("size", SIZES)
def test_threshold_one_and_three_channels(fields, size):
    f = fields[size]
    for thr in THRESHOLDS:
        want = R.threshold_mask(f[:, :, None], 0, 0, thr)
        assert 0 < want.sum() < want.size                                   # the mask has both values
        assert np.array_equal(run_threshold(f[:, :, None], 0, 0, thr), want)
        a3 = three_channels(f)
        assert np.array_equal(run_threshold(a3, 2, 0, thr), want)
        assert np.array_equal(run_threshold(a3, 1, 0, thr), R.threshold_mask(a3, 1, 0, thr))


def test_threshold_rounds_the_threshold_to_float32_once(fields):
    f = fields[(37, 53)].copy()
    third = np.float32(1 / 3)                                               # float32(1/3) > 1/3 as a double
    f[4, 4], f[4, 5] = third, np.nextafter(third, np.float32(1))
    want = R.threshold_mask(f[:, :, None], 0, 0, 1 / 3)
    assert want[4, 4] == 0 and want[4, 5] == 1                              # `arr > 1/3` on a float32 array compares with float32(1/3)
    assert np.array_equal(run_threshold(f[:, :, None], 0, 0, 1 / 3), want)


def test_threshold_nan_is_never_larger(fields):
    f = fields[(37, 53)].copy()
    f[5, 5] = f[36, 52] = np.nan
    got = run_threshold(f[:, :, None], 0, 0, 0.0)
    assert got[5, 5] == 0 and got[36, 52] == 0 and np.array_equal(got, R.threshold_mask(f[:, :, None], 0, 0, 0.0))
    a3 = three_channels(f)                                                   # mode 1: a NaN never replaces the running maximum
    for c in range(3):
        assert np.array_equal(run_threshold(a3, c, 1, 0.5), R.threshold_mask(a3, c, 1))


@pytest.mark.parametrize("size", SIZES)
def test_threshold_argmax_mode_with_exact_ties(fields, size):
    a3 = three_channels(fields[size])
    a3[0, 0] = 0.5                                                           # three-way tie: index 0
    a3[-1, -1, 1:] = 2.0                                                     # channels 1 and 2 tie above channel 0: index 1
    a3[1, 2, 0] = a3[1, 2, 2] = 3.0                                          # channels 0 and 2 tie: index 0
    for c in range(3):
        want = R.threshold_mask(a3, c, 1)
        assert np.array_equal(want, np.argmax(a3, axis=2) == c)
        assert np.array_equal(run_threshold(a3, c, 1, 0.5), want)
    assert run_threshold(a3, 0, 1, 0.5)[0, 0] == 1 and run_threshold(a3, 1, 1, 0.5)[-1, -1] == 1
    wide = np.random.default_rng(8).integers(0, 4, size=size + (32,)).astype(np.float32)      # C = 32, ties everywhere
    assert np.array_equal(run_threshold(wide, 5, 1, 0.5), np.argmax(wide, axis=2) == 5)


@pytest.mark.parametrize("ld,offset", [(64, 0), (55, 0), (64, 3), (53, 16), (128, 32)])
def test_threshold_pitch_and_alignment(fields, ld, offset):
    """out_ld > w with 16-byte rows (one store per 16 pixels and a scalar tail), with odd rows and off a 16-byte base (one byte a thread)."""
    f = fields[(37, 53)]
    want = R.threshold_mask(f[:, :, None], 0, 0, 0.5)
    assert np.array_equal(run_threshold(f[:, :, None], 0, 0, 0.5, out_ld=ld, offset=offset), want)
    a3 = three_channels(f)
    assert np.array_equal(run_threshold(a3, 1, 1, 0.5, out_ld=ld, offset=offset), R.threshold_mask(a3, 1, 1))


def test_threshold_refusals(fields):
    from segmentation_training_pipeline_amd import _lib, ops
    f = dev(fields[(37, 53)][:, :, None])
    out = torch.zeros(37 * 53, dtype=torch.uint8, device="cuda")
    for kw in ({"channel": 1}, {"channel": -1}, {"mode": 2}, {"out_ld": 52}):
        a = dict({"channel": 0, "mode": 0, "out_ld": 53}, **kw)
        with pytest.raises(_lib.StpError, match="BADARG"):
            ops.mask_threshold(f, 37, 53, 1, a["channel"], a["mode"], 0.5, out, a["out_ld"])
    with pytest.raises(_lib.StpError, match="BADARG"):
        ops.mask_threshold(torch.zeros(4 * 4 * 33, device="cuda"), 4, 4, 33, 0, 1, 0.5, out)


# ------------------------------------------------------------------------------------------------ stp_mask_morph
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("r", [1, 2, 3, 7])
def test_erosion_dilation_opening_closing(fields, size, r):
    for thr in THRESHOLDS:
        m = R.threshold_mask(fields[size][:, :, None], 0, 0, thr)
        er, di = run_morph(m, r, 0), run_morph(m, r, 1)
        assert np.array_equal(er, R.erode(m, r)) and np.array_equal(di, R.dilate(m, r))
        opened, closed = run_morph(er, r, 1), run_morph(di, r, 0)
        want_open, want_close = R.opening(m, r), R.closing(m, r)
        assert np.array_equal(opened, want_open) and np.array_equal(closed, want_close)
        if size in BIG and r <= 3:
            removed = int(m.sum()) - int(want_open.sum())
            assert 7 <= removed <= 1495                                      # the opening changes the mask
            assert (want_close > m).any() and (want_close < m).any()         # scipy's closing adds pixels and clears the border band
        if size == (3, 5) and r >= 2:
            assert want_open.sum() == 0                                      # smaller than the disk: nothing survives


def test_all_ones_and_scipys_border_band():
    ones = np.ones((9, 11), np.uint8)
    opened = run_morph(run_morph(ones, 2, 0), 2, 1)
    closed = run_morph(run_morph(ones, 2, 1), 2, 0)
    assert int(opened.sum()) == 87 and np.array_equal(opened, R.opening(ones, 2))
    assert int(closed.sum()) == 35 and np.array_equal(closed, R.closing(ones, 2))
    assert closed[2:-2, 2:-2].all()                                          # the 5 x 7 interior


@pytest.mark.parametrize("corner", [(0, 0), (0, 10), (8, 0), (8, 10)])
def test_single_pixel_at_a_corner(corner):
    m = np.zeros((9, 11), np.uint8)
    m[corner] = 1
    for r in (1, 2, 7):
        di = run_morph(m, r, 1)
        assert np.array_equal(di, R.dilate(m, r)) and di.sum() > 1
        assert run_morph(m, r, 0).sum() == 0


def test_object_across_the_tile_boundary():
    """A blob over the corner where four workgroup tiles meet (MORPH_TILE = 64 rows x 256 columns), and a line along each seam."""
    th, tw = MORPH_TILE
    m = np.zeros((th + 30, tw + 40), np.uint8)
    yy, xx = np.mgrid[:m.shape[0], :m.shape[1]]
    m[(yy - th) ** 2 + (xx - tw) ** 2 <= 11 ** 2] = 1
    m[th - 1:th + 1, 5:100] = 1
    m[3:40, tw - 2:tw + 1] = 1
    m[th - 8:th + 8:3, tw - 9:tw + 9:2] ^= 1                                 # holes and specks inside the blob
    for r in (1, 2, 3, 7):
        er, di = run_morph(m, r, 0), run_morph(m, r, 1)
        assert np.array_equal(er, R.erode(m, r)) and np.array_equal(di, R.dilate(m, r)), r
        assert np.array_equal(run_morph(er, r, 1), R.opening(m, r)) and np.array_equal(run_morph(di, r, 0), R.closing(m, r)), r
    quadrants = [(ys, xs) for ys in (slice(0, th), slice(th, None)) for xs in (slice(0, tw), slice(tw, None))]
    assert all(m[q].any() and R.erode(m, 1)[q].any() and not R.dilate(m, 7)[q].all() for q in quadrants)      # the object lies in all four tiles


def test_morph_refusals():
    from segmentation_training_pipeline_amd import _lib, ops
    a = torch.zeros((9, 11), dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    for r, op, dst in ((0, 0, b), (8, 0, b), (2, 2, b), (2, -1, b), (2, 0, a)):
        with pytest.raises(_lib.StpError, match="BADARG"):
            ops.mask_morph(a, dst, 9, 11, r, op)


# ------------------------------------------------------------------------------------------------ stp_mask_rle
def check_rle(mask):
    n, runs = run_rle(mask)
    want = R.rle_runs(mask)
    assert n == len(want) and np.array_equal(runs, want)
    assert R.format_runs(runs) == R.rle_encode(mask)
    return n


@pytest.mark.parametrize("size", SIZES + [(130, 7), (1, 1), (1, 200), (200, 1)])
def test_rle_of_plain_images(size):
    h, w = size
    assert check_rle(np.ones(size, np.uint8)) == 1                           # one run over every column boundary
    assert check_rle(np.zeros(size, np.uint8)) == 0
    board = np.zeros((w, h), np.uint8)
    board.reshape(-1)[::2] = 1                                               # every other pixel of the flat column-major array
    assert check_rle(np.ascontiguousarray(board.T)) == (h * w + 1) // 2      # the most runs an image can have: the capacity
    assert check_rle(np.ascontiguousarray(1 - board.T)) == (h * w) // 2
    assert check_rle((np.ones(size) * 255).astype(np.uint8)) == 1            # any non-zero byte is mask


@pytest.mark.parametrize("size", SIZES)
def test_rle_of_the_filtered_masks(fields, size):
    for thr in THRESHOLDS:
        m = R.threshold_mask(fields[size][:, :, None], 0, 0, thr)
        n = check_rle(m)
        if size in BIG:
            assert n >= 12 and R.column_crossings(m) >= 38                   # many runs, and runs that go on across a column boundary
        for r in (1, 2, 3):
            opened = R.opening(m, r)
            n = check_rle(opened)
            if size == (3, 5) and r >= 2:
                assert n == 0 and R.rle_encode(opened) == ""                 # the empty code
            check_rle(R.closing(m, r))


def test_rle_runs_across_words_and_workgroups():
    """Columns of 200 rows are 4 bit words (the last with 8 valid bits); 300 of them are 1200 words = 5 workgroups of the count / write
    launches: runs that start in one word, or one workgroup, and end in a later one."""
    rng = np.random.default_rng(11)
    flat = np.zeros(200 * 300, np.uint8)                                      # the column-major order
    pos = 0
    while pos < flat.size:                                                    # run lengths from 1 pixel to several columns
        run = 20000 if 10000 <= pos < 10700 else int(rng.choice([1, 2, 63, 64, 65, 199, 200, 201, 700]))
        gap = int(rng.choice([1, 1, 2, 64, 190]))
        flat[pos:pos + run] = 1
        pos += run + gap
    m = np.ascontiguousarray(flat.reshape(300, 200).T)
    n = check_rle(m)
    assert n > 100 and (R.rle_runs(m)[:, 1] > 16384).any()                   # a run longer than a workgroup's 16384 pixels


def test_rle_refusals():
    from segmentation_training_pipeline_amd import _lib, ops
    m = np.ones((37, 53), np.uint8)
    cap = (37 * 53 + 1) // 2
    with pytest.raises(_lib.StpError, match="BADARG"):
        run_rle(m, capacity=cap - 1)                                         # one pair short of what the image could need
    runs = torch.zeros((cap, 2), dtype=torch.int32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    small = torch.empty(ops.mask_rle_workspace_bytes(37, 53) - 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.StpError, match="WORKSPACE"):
        ops.mask_rle(dev(m), 37, 53, runs, count, small)
    assert ops.mask_rle_workspace_bytes(1 << 16, 1 << 15) == 0               # h * w = 2^31 is refused


# ------------------------------------------------------------------------------------------------ stp_threshold_counts
SWEEPS = {1: [0.5], 19: [d / 20 for d in range(1, 20)], 64: [(i + 1) / 66 for i in range(64)]}


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("T", [1, 19, 64])
def test_threshold_counts(fields, size, T):
    f = fields[size].copy()
    thr = SWEEPS[T]
    f[0, 0] = np.float32(thr[0])                                             # exactly a threshold: not above it
    f[-1, -1] = np.float32(thr[-1])
    f[0, 1] = np.nan                                                         # above nothing
    target = ndimage.binary_dilation(f > 0.55, R.disk(1))
    want_counts, want_totals = R.threshold_counts(f[:, :, None], target, thr)
    assert 0 < want_totals[0] < want_totals[1] and want_counts[0, 0] >= want_counts[0, 1] > 0
    assert size == (3, 5) or want_counts[0, 0] > want_counts[0, 1]           # pixels above the threshold on and off the target
    counts, totals = run_counts(f[:, :, None], target, thr)
    assert np.array_equal(counts, want_counts) and np.array_equal(totals, want_totals)
    a3 = three_channels(f)
    counts, totals = run_counts(a3, target, thr, channel=2)
    assert np.array_equal(counts, want_counts) and np.array_equal(totals, want_totals)
    counts, _ = run_counts(a3, target, thr, channel=1)
    assert np.array_equal(counts, R.threshold_counts(a3, target, thr, channel=1)[0])


def test_threshold_counts_over_several_workgroups():
    """300 x 400 pixels are 118 workgroups of 1024 pixels: their tables meet in the finalize launch."""
    f = field(300, 400)
    target = f > 0.6
    thr = SWEEPS[19]
    counts, totals = run_counts(f[:, :, None], target, thr)
    want = R.threshold_counts(f[:, :, None], target, thr)
    assert np.array_equal(counts, want[0]) and np.array_equal(totals, want[1]) and totals[1] == 120000


def test_threshold_counts_refusals(fields):
    from segmentation_training_pipeline_amd import _lib
    f = fields[(37, 53)][:, :, None]
    target = f[:, :, 0] > 0.5
    for bad in ([0.5, 0.25], [0.25, 0.25], [0.1, float("nan")], [0.1, float("inf")], [], [i / 100 for i in range(65)]):
        with pytest.raises(_lib.StpError, match="BADARG"):
            run_counts(f, target, bad) if bad else run_counts_empty(f, target)


def run_counts_empty(arr, target):
    from segmentation_training_pipeline_amd import ops
    z = torch.zeros((1, 2), dtype=torch.int64, device="cuda")
    ops.threshold_counts(dev(arr), dev(target.astype(np.uint8)), 37, 53, 1, 0, [], z, z.reshape(-1), torch.empty(8192, dtype=torch.uint8, device="cuda"))
