"""GPU tests of the sliding-window entry points (csrc/window.hip): stp_window_gather_u8, stp_window_accumulate and stp_window_finish,
each called directly on seeded data and compared with the numpy host statement of tests/_window_reference.py by ``np.array_equal``:
the kernels do one fp32 multiplication and one fp32 addition per window in window order and one correctly rounded division - the
operations numpy performs.

Shapes: an image / canvas of 13 x 17 (rows of 17 or 51 elements: no row pitch is a multiple of 16 bytes, one element per thread) and of
16 x 32 (every row on a 16-byte boundary: the 16-byte accesses), 8 x 8 windows (and 8 x 16: window rows of whole 16-byte vectors), a
5 x 6 image smaller than its window, 1 / 4 / 64 windows per call and 70 through the wrapper (two calls)."""
import numpy as np
import pytest
import torch

import _window_reference as R
from test_ops_rest_gpu import BADARG, DEV, keep, rc  # noqa: F401
from test_ops_rest_gpu import _release_device_temporaries, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def up(a):
    return keep(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(params=["bf16", "fp16"])
def build(request):
    """Both builds of the library carry the same window kernels."""
    from segmentation_training_pipeline_amd import _lib
    with _lib.storage(request.param):
        yield request.param


# ---------------------------------------------------------------- gather
GATHER_ORIGINS = [(0, 0), (5, 9), (9, 13), (12, 16)]          # (9, 13) and (12, 16): an 8 x 8 window hangs over both edges of 13 x 17


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("win", [(8, 8), (8, 16)])
def test_gather_equals_numpy(ops, win, n, C):
    H, W = win
    img = np.random.RandomState(10 * n + C).randint(0, 256, size=(13, 17, C)).astype(np.uint8)
    org = GATHER_ORIGINS[2:3] if n == 1 else GATHER_ORIGINS
    out = keep(torch.full((n + 1, H, W, C), 0x5A, dtype=torch.uint8, device=DEV))
    ops.window_gather_u8(up(img), 13, 17, C, org, out, H, W)
    got = down(out)
    assert np.array_equal(got[:n], np.stack([R.cut(img, y0, x0, H, W) for y0, x0 in org])), (win, n, C)
    assert (got[n] == 0x5A).all()                                                # nothing behind the n windows is written
    assert np.array_equal(got[0][:4, :4], img[org[0][0]:org[0][0] + 4, org[0][1]:org[0][1] + 4])


@pytest.mark.parametrize("C", [1, 3])
def test_gather_pads_a_small_image_by_its_edge(ops, build, C):
    """A 5 x 6 image under an 8 x 8 (element-wise) and an 8 x 16 (16-byte stores) window: np.pad(mode="edge"); and into a buffer that
    starts one byte behind a 16-byte boundary."""
    img = np.random.RandomState(20 + C).randint(0, 256, size=(5, 6, C)).astype(np.uint8)
    for H, W in ((8, 8), (8, 16)):
        want = np.pad(img, ((0, H - 5), (0, W - 6), (0, 0)), mode="edge")
        for off in (0, 1):
            buf = keep(torch.full((H * W * C + 16,), 0x5A, dtype=torch.uint8, device=DEV))
            ops.window_gather_u8(up(img), 5, 6, C, [(0, 0)], buf[off:], H, W)
            got = down(buf)
            assert np.array_equal(got[off:off + H * W * C].reshape(H, W, C), want), (H, W, off)
            assert (got[:off] == 0x5A).all() and (got[off + H * W * C:] == 0x5A).all()


# ---------------------------------------------------------------- accumulate
def accumulate_origins(n, h, w, rng):
    """(0, 0), (3, 5) twice and (5, 9): pixel (5, 6) lies in three windows, two of them at one origin; then random ones."""
    if n == 1:
        return [(2, 3)]
    first = [(0, 0), (3, 5), (3, 5), (5, 9)]
    return first + [(int(rng.randint(0, h)), int(rng.randint(0, w))) for _ in range(n - 4)]


def six_decades(rng, shape):
    return (10.0 ** rng.uniform(-3, 3, size=shape)).astype(np.float32)


@pytest.mark.parametrize("overlap", [0, 2, 4])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("n", [1, 4, 64, 70])
@pytest.mark.parametrize("canvas", [(13, 17), (16, 32)])
def test_accumulate_equals_numpy_in_window_order(ops, canvas, n, C, overlap):
    h, w = canvas
    H = W = 8
    rng = np.random.RandomState(1000 * n + 10 * C + overlap + h)
    org = accumulate_origins(n, h, w, rng)
    acc = six_decades(rng, (n, H, W, C))
    start = six_decades(rng, (h, w, C))
    want = R.accumulate(start.copy(), acc, org, overlap)
    accd = up(acc)
    got = []
    for _ in range(2):                                  # a second call on a fresh canvas is byte-identical
        cv = up(start)
        ops.window_accumulate(accd, H, W, C, org, overlap, cv, h, w)
        got.append(down(cv))
    assert np.array_equal(got[0], want), (canvas, n, C, overlap)
    assert got[0].tobytes() == got[1].tobytes()
    if n > 1:                                           # the order of the additions shows: the reversed order gives another sum somewhere
        assert not np.array_equal(R.accumulate(start.copy(), acc[::-1], org[::-1], overlap), want)
    else:                                               # rows no window touches are unchanged (here: all but rows 2..9)
        assert np.array_equal(got[0][:2], start[:2]) and np.array_equal(got[0][10:], start[10:])
        assert not np.array_equal(got[0][2:10], start[2:10])


def test_accumulate_leaves_the_rows_outside_the_batch_alone(ops, build):
    """The launch covers rows 5..12 only: NaN sentinels above and below stay bit for bit (a NaN + 0 would not), on both builds, and
    on a canvas that starts one float behind a 16-byte boundary."""
    h, w, C, H, W = 16, 32, 3, 8, 8
    rng = np.random.RandomState(6)
    acc = six_decades(rng, (2, H, W, C))
    org = [(5, 0), (5, 20)]
    for off in (0, 1):
        start = six_decades(rng, (h, w, C))
        start[:5], start[13:] = np.float32("nan"), np.float32("nan")
        buf = keep(torch.full((h * w * C + 4,), -3.0, dtype=torch.float32, device=DEV))
        buf[off:off + h * w * C] = torch.from_numpy(start.reshape(-1)).to(DEV)
        ops.window_accumulate(up(acc), H, W, C, org, 2, buf[off:], h, w)
        got = down(buf)
        body = got[off:off + h * w * C].reshape(h, w, C)
        assert np.isnan(body[:5]).all() and np.isnan(body[13:]).all()
        assert np.array_equal(body[5:13], R.accumulate(start.copy(), acc, org, 2)[5:13]), off
        assert (got[:off] == -3.0).all() and (got[off + h * w * C:] == -3.0).all()


# ---------------------------------------------------------------- finish
def finish_case(rng, h, w, C, k):
    """A canvas as the windows of an h x w image leave it: probabilities times the exact weight sums of 8 x 8 windows at overlap 2."""
    sy, sx = R.sums(h, 8, 2), R.sums(w, 8, 2)
    den = (np.float32(k) * sy.astype(np.float32)[:, None] * sx.astype(np.float32)[None, :])[..., None]
    return (rng.uniform(0, 1, size=(h, w, C)).astype(np.float32) * den).astype(np.float32), sy, sx


def new_out(mode, h, w, c):
    if mode == 0:
        return keep(torch.full((h, w, c), float("nan"), dtype=torch.float32, device=DEV))
    return keep(torch.full((h, w) if mode == 2 else (h, w, c), 0x5A, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("C", [1, 3, 32])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("size", [(13, 17), (16, 32)])
def test_finish_equals_numpy(ops, size, mode, C):
    h, w = size
    rng = np.random.RandomState(100 * mode + C + h)
    for k in (1, 6):
        canvas, sy, sx = finish_case(rng, h, w, C, k)
        assert len(set(sy.tolist())) > 1 and len(set(sx.tolist())) > 1              # the weight sums differ along both axes
        out = new_out(mode, h, w, C)
        ops.window_finish(up(canvas), h, w, C, k, up(sy.astype(np.float32)), up(sx.astype(np.float32)), mode, out)
        got, want = down(out), R.finish(canvas, k, sy, sx, mode)
        assert got.dtype == want.dtype and np.array_equal(got, want), (size, mode, C, k)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("x0", [0, 3, 4, 16])
def test_finish_writes_only_its_rectangle(ops, build, mode, x0):
    """out_ld > w: a 13 x 17 map finished into a rectangle of a sentinel-filled 20 x 48 map; everything outside it stays untouched.
    x0 = 0 / 4 / 16 put the corner on a 16-byte boundary for some of the modes (vector stores + a row tail), 3 for none."""
    h, w, C, k, y0, full_h, full_w = 13, 17, 3, 3, 2, 20, 48
    canvas, sy, sx = finish_case(np.random.RandomState(5 + mode), h, w, C, k)
    sentinel = 77.0 if mode == 0 else 0x5A
    shape = (full_h, full_w) if mode == 2 else (full_h, full_w, C)
    full = keep(torch.full(shape, sentinel, dtype=torch.float32 if mode == 0 else torch.uint8, device=DEV))
    ops.window_finish(up(canvas), h, w, C, k, up(sy.astype(np.float32)), up(sx.astype(np.float32)), mode, full[y0:y0 + h, x0:x0 + w],
                      out_ld=full_w)
    want = np.full(shape, sentinel, np.float32 if mode == 0 else np.uint8)
    want[y0:y0 + h, x0:x0 + w] = R.finish(canvas, k, sy, sx, mode)
    assert np.array_equal(down(full), want)


def test_finish_labels_a_nan_never_wins(ops):
    """Label maps: a NaN channel (behind channel 0) is never the largest, ties take the first index, and a one-class head is > 0.5."""
    h, w, C, k = 13, 17, 3, 2
    rng = np.random.RandomState(8)
    canvas, sy, sx = finish_case(rng, h, w, C, k)
    canvas[::2, ::3, 1] = np.float32("nan")
    canvas[1::4, 1::2, 2] = np.float32("nan")
    canvas[3, 4] = canvas[3, 4, 0]                                                    # a three-way tie: the first index
    syd, sxd = up(sy.astype(np.float32)), up(sx.astype(np.float32))
    out = new_out(2, h, w, C)
    ops.window_finish(up(canvas), h, w, C, k, syd, sxd, 2, out)
    v = R.finish(canvas, k, sy, sx, 0)
    want = np.argmax(np.where(np.isnan(v), -np.inf, v), axis=2)
    got = down(out)
    assert np.array_equal(got, want) and got[3, 4] == 0 and np.isnan(v).any()
    assert not np.array_equal(want, np.argmax(v, axis=2))                             # (numpy's own argmax lets a NaN win)
    one = canvas[:, :, :1].copy()
    one[0, 0] = np.float32("nan")
    out = new_out(2, h, w, 1)
    ops.window_finish(up(one), h, w, 1, k, syd, sxd, 2, out)
    v1 = R.finish(one, k, sy, sx, 0)[:, :, 0]
    assert np.array_equal(down(out), v1 > 0.5) and (v1 > 0.5).any() and not (v1 > 0.5).all()


def test_refusals(ops):
    """With real buffers: the good call returns 0, each entry of the header's list STP_E_BADARG."""
    import ctypes
    u8, u8b = keep(torch.zeros(8192, dtype=torch.uint8, device=DEV)), keep(torch.zeros(8192, dtype=torch.uint8, device=DEV))
    f, fb = keep(torch.zeros(8192, dtype=torch.float32, device=DEV)), keep(torch.zeros(8192, dtype=torch.float32, device=DEV))
    s1, s2 = keep(torch.ones(64, dtype=torch.float32, device=DEV)), keep(torch.ones(64, dtype=torch.float32, device=DEV))
    st = ops.stream()
    org = (ctypes.c_int32 * 4)(0, 0, 5, 9)
    out = (ctypes.c_int32 * 4)(0, 0, 13, 0)
    assert rc("stp_window_gather_u8", ops.ptr(u8), 13, 17, 3, org, 2, ops.ptr(u8b), 8, 8, st) == 0
    assert rc("stp_window_gather_u8", ops.ptr(u8), 13, 17, 3, out, 2, ops.ptr(u8b), 8, 8, st) == BADARG
    assert rc("stp_window_gather_u8", ops.ptr(u8), 13, 17, 3, org, 0, ops.ptr(u8b), 8, 8, st) == BADARG
    assert rc("stp_window_gather_u8", ops.ptr(u8), 13, 17, 3, org, 2, ops.ptr(u8), 8, 8, st) == BADARG
    assert rc("stp_window_accumulate", ops.ptr(f), 8, 8, 3, org, 2, 4, ops.ptr(fb), 13, 17, st) == 0
    assert rc("stp_window_accumulate", ops.ptr(f), 8, 8, 3, org, 2, 5, ops.ptr(fb), 13, 17, st) == BADARG
    assert rc("stp_window_accumulate", ops.ptr(f), 8, 8, 3, out, 2, 4, ops.ptr(fb), 13, 17, st) == BADARG
    assert rc("stp_window_accumulate", ops.ptr(f), 8, 8, 3, org, 2, 4, ops.ptr(f), 13, 17, st) == BADARG
    assert rc("stp_window_finish", ops.ptr(f), 13, 17, 3, 2, ops.ptr(s1), ops.ptr(s2), 0, ops.ptr(fb), 17, st) == 0
    assert rc("stp_window_finish", ops.ptr(f), 13, 17, 3, 2, ops.ptr(s1), ops.ptr(s2), 0, ops.ptr(fb), 16, st) == BADARG
    assert rc("stp_window_finish", ops.ptr(f), 13, 17, 3, 2, ops.ptr(s1), ops.ptr(s2), 3, ops.ptr(fb), 17, st) == BADARG
    assert rc("stp_window_finish", ops.ptr(f), 13, 17, 33, 2, ops.ptr(s1), ops.ptr(s2), 2, ops.ptr(u8), 17, st) == BADARG
    assert rc("stp_window_finish", ops.ptr(f), 13, 17, 32, 2, ops.ptr(s1), ops.ptr(s2), 2, ops.ptr(u8), 17, st) == 0
    torch.cuda.synchronize()
