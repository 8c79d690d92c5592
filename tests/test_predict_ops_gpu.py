"""GPU tests of the prediction entry points (csrc/predict.hip): stp_flip_u8, stp_predict_accumulate and stp_predict_finish, each called
directly on seeded random data and compared with the numpy restatement of tests/_predict_reference.py - the arithmetic of the host
chain in segmentation_pipeline/segmentation.py.  Every comparison is ``np.array_equal``: the kernels do one fp32 add, one correctly
rounded division, one multiplication and a truncation, exactly the operations numpy performs.

Shapes: (1, 1, 1, 1); (2, 5, 7, 3) odd with a centre row and column, rows of 21 elements (not a multiple of the 16-byte vector: one
element per thread); (3, 8, 8, 4) all 16-byte accesses for the floats; (2, 6, 9, 20); (1, 4, 33, 1); (2, 4, 16, 3) all 16-byte accesses
for the bytes too; and one buffer that starts 1 element off a 16-byte boundary (vector-sized rows, unaligned base)."""
import numpy as np
import pytest
import torch

import _predict_reference as R
from test_ops_rest_gpu import BADARG, DEV, keep, rc  # noqa: F401
from test_ops_rest_gpu import _release_device_temporaries, ops  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (3, 8, 8, 4), (2, 6, 9, 20), (1, 4, 33, 1), (2, 4, 16, 3)]


def up(a):
    return keep(torch.from_numpy(np.ascontiguousarray(a)).to(DEV))


def down(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def probs_like(rng, shape):
    return rng.uniform(0, 1, size=shape).astype(np.float32)


@pytest.fixture(params=["bf16", "fp16"])
def build(request):
    """Both builds of the library carry the same prediction kernels."""
    from segmentation_training_pipeline_amd import _lib
    with _lib.storage(request.param):
        yield request.param


@pytest.mark.parametrize("shape", SHAPES)
def test_flip_u8_equals_numpy(ops, shape):
    n, h, w, c = shape
    x = np.random.RandomState(sum(shape)).randint(0, 256, size=shape).astype(np.uint8)
    xd = up(x)
    for f in R.FLIPS:
        out = keep(torch.full(shape, 0x5A, dtype=torch.uint8, device=DEV))
        ops.flip_u8(xd, out, n, h, w, c, f)
        assert np.array_equal(down(out), R.flip(x, f)), (shape, f)


@pytest.mark.parametrize("shape", SHAPES)
def test_predict_accumulate_equals_numpy(ops, shape):
    """One add into a non-zero accumulator per flip, then six successive adds (two models x three flips) into one zeroed buffer."""
    n, h, w, c = shape
    rng = np.random.RandomState(7 + sum(shape))
    start = probs_like(rng, shape)
    maps = [probs_like(rng, shape) for _ in range(6)]
    for f in R.FLIPS:
        acc = up(start)
        ops.predict_accumulate(up(maps[0]), acc, n, h, w, c, f)
        assert np.array_equal(down(acc), R.accumulate(start.copy(), maps[0], f)), (shape, f)
    acc, ref = up(np.zeros(shape, np.float32)), np.zeros(shape, np.float32)
    for i, p in enumerate(maps):
        ops.predict_accumulate(up(p), acc, n, h, w, c, i % 3)
        R.accumulate(ref, p, i % 3)
    assert np.array_equal(down(acc), ref), shape


def test_flip_and_accumulate_on_both_builds_and_unaligned_buffers(ops, build):
    """Rows of a whole number of 16-byte vectors in buffers that start one element behind a 16-byte boundary take the element-wise
    kernels; the result is the same.  (Run against libstp_hip.so and libstp_hip_f16.so.)"""
    shape = n, h, w, c = (2, 3, 8, 4)
    rng = np.random.RandomState(11)
    x = rng.randint(0, 256, size=shape).astype(np.uint8)
    p, a = probs_like(rng, shape), probs_like(rng, shape)
    size = x.size
    for f in R.FLIPS:
        for off in (0, 1):
            src8 = keep(torch.zeros(size + 16, dtype=torch.uint8, device=DEV))
            dst8 = keep(torch.full((size + 16,), 0x5A, dtype=torch.uint8, device=DEV))
            src8[off:off + size] = torch.from_numpy(x.reshape(-1)).to(DEV)
            ops.flip_u8(src8[off:], dst8[off:], n, h, w, c, f)
            got = down(dst8)
            assert np.array_equal(got[off:off + size].reshape(shape), R.flip(x, f)), (f, off)
            assert (got[:off] == 0x5A).all() and (got[off + size:] == 0x5A).all(), (f, off)
            srcf = keep(torch.zeros(size + 4, dtype=torch.float32, device=DEV))
            accf = keep(torch.full((size + 4,), -3.0, dtype=torch.float32, device=DEV))
            srcf[off:off + size] = torch.from_numpy(p.reshape(-1)).to(DEV)
            accf[off:off + size] = torch.from_numpy(a.reshape(-1)).to(DEV)
            ops.predict_accumulate(srcf[off:], accf[off:], n, h, w, c, f)
            got = down(accf)
            assert np.array_equal(got[off:off + size].reshape(shape), R.accumulate(a.copy(), p, f)), (f, off)
            assert (got[:off] == -3.0).all() and (got[off + size:] == -3.0).all(), (f, off)


SOURCES = [(8, 8), (6, 10)]
TARGETS = [(8, 8), (1, 1), (5, 13), (19, 7), (16, 16)]
KS = (1, 3, 6, 15)


def new_out(mode, h, w, c):
    if mode == 0:
        return keep(torch.full((h, w, c), float("nan"), dtype=torch.float32, device=DEV))
    return keep(torch.full((h, w) if mode == 2 else (h, w, c), 0x5A, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("c", [1, 2, 3, 8, 20, 32])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_predict_finish_equals_numpy(ops, mode, c):
    """Sums of k maps -> mean, nearest gather to h x w, and the mode's output, for every k, source and target size."""
    rng = np.random.RandomState(100 * mode + c)
    for (H, W) in SOURCES:
        for k in KS:
            acc = np.zeros((H, W, c), np.float32)
            for _ in range(k):
                acc += probs_like(rng, (H, W, c))
            accd = up(acc)
            for (h, w) in TARGETS:
                out = new_out(mode, h, w, c)
                ops.predict_finish(accd, H, W, c, k, mode, out, h, w)
                got, want = down(out), R.finish(acc, k, mode, h, w)
                assert got.dtype == want.dtype and np.array_equal(got, want), (mode, c, H, W, k, h, w)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("x0", [0, 3, 4, 16])
def test_predict_finish_writes_only_its_rectangle(ops, mode, x0):
    """out_ld > w: a 5 x 13 map finished into a rectangle of a sentinel-filled 9 x 40 map; everything outside it stays untouched.
    x0 = 0 / 4 / 16 put the corner on a 16-byte boundary for some of the modes (vector stores + a row tail), 3 for none."""
    H, W, c, k, h, w, y0, full_h, full_w = 6, 10, 3, 3, 5, 13, 2, 9, 40
    rng = np.random.RandomState(5 + mode)
    acc = sum(probs_like(rng, (H, W, c)) for _ in range(k)).astype(np.float32)
    sentinel = 77.0 if mode == 0 else 0x5A
    shape = (full_h, full_w) if mode == 2 else (full_h, full_w, c)
    full = keep(torch.full(shape, sentinel, dtype=torch.float32 if mode == 0 else torch.uint8, device=DEV))
    ops.predict_finish(up(acc), H, W, c, k, mode, full[y0:y0 + h, x0:x0 + w], h, w, out_ld=full_w)
    want = np.full(shape, sentinel, np.float32 if mode == 0 else np.uint8)
    want[y0:y0 + h, x0:x0 + w] = R.finish(acc, k, mode, h, w)
    assert np.array_equal(down(full), want)


def test_predict_finish_label_ties_take_the_first_index(ops):
    """Rows with exact ties (sums that are equal, and sums that only become equal once divided and rounded)."""
    H, W, c = 4, 8, 5
    rng = np.random.RandomState(3)
    acc = rng.randint(0, 3, size=(H, W, c)).astype(np.float32)        # small integers: most pixels hold their maximum more than once
    acc[0, 0] = [1, 1, 1, 1, 1]
    acc[0, 1] = [0, 2, 2, 0, 2]
    acc[0, 2] = [0, 0, 0, 0, 0]
    tiny = np.float32(1e-45)                                          # the smallest subnormal: x / 3 rounds 1, 2 -> 0 or 1 ulp alike
    acc[1, 0] = [tiny, 2 * tiny, 2 * tiny, tiny, 0]
    acc[1, 1] = np.float32(1) + np.arange(5, dtype=np.float32) * np.float32(2.0 ** -23)      # neighbours: thirds may coincide
    assert (np.sort(acc.reshape(-1, c), axis=1)[:, -1] == np.sort(acc.reshape(-1, c), axis=1)[:, -2]).any()
    for k in (1, 3):
        for (h, w) in ((H, W), (7, 9)):
            out = new_out(2, h, w, c)
            ops.predict_finish(up(acc), H, W, c, k, 2, out, h, w)
            assert np.array_equal(down(out), R.finish(acc, k, 2, h, w)), (k, h, w)
    two = np.array([[[0.5, 0.5], [0.25, 0.75], [0.75, 0.25]]], np.float32)
    out = new_out(2, 1, 3, 2)
    ops.predict_finish(up(two), 1, 3, 2, 1, 2, out, 1, 3)
    assert down(out).tolist() == [[0, 1, 0]]
    one = np.array([[[0.5], [np.nextafter(np.float32(0.5), np.float32(1))], [0.0], [1.0]]], np.float32)      # > 0.5, not >=
    out = new_out(2, 1, 4, 1)
    ops.predict_finish(up(one), 1, 4, 1, 1, 2, out, 1, 4)
    assert down(out).tolist() == [[0, 1, 0, 1]]


def test_predict_finish_bytes_truncate(ops):
    """Mode 1 on 0, 1, every n / 255 and the float just below it: (uint8)(v * 255.f) truncates as ``(v * 255).astype(np.uint8)``."""
    n = np.arange(1, 256, dtype=np.float32) / np.float32(255)
    v = np.concatenate([np.float32([0, 1]), n, np.nextafter(n, np.float32(0))]).astype(np.float32)
    acc = v.reshape(1, -1, 1)
    W = acc.shape[1]
    out = new_out(1, 1, W, 1)
    ops.predict_finish(up(acc), 1, W, 1, 1, 1, out, 1, W)
    got = down(out)
    assert np.array_equal(got, (acc * 255).astype(np.uint8)) and got[0, 0, 0] == 0 and got[0, 1, 0] == 255
    acc3 = (acc * np.float32(3)).astype(np.float32)                    # and through the division: three equal maps
    out = new_out(1, 1, W, 1)
    ops.predict_finish(up(acc3), 1, W, 1, 3, 1, out, 1, W)
    assert np.array_equal(down(out), R.finish(acc3, 3, 1, 1, W))


def test_refusals(ops):
    """NULL pointers, non-positive sizes, a flip or mode outside its range and source == destination: STP_E_BADARG, nothing launched."""
    u8 = keep(torch.zeros(4096, dtype=torch.uint8, device=DEV))
    u8b = keep(torch.zeros(4096, dtype=torch.uint8, device=DEV))
    f = keep(torch.zeros(4096, dtype=torch.float32, device=DEV))
    fb = keep(torch.zeros(4096, dtype=torch.float32, device=DEV))
    st = ops.stream()
    for name, a, b in (("stp_flip_u8", ops.ptr(u8), ops.ptr(u8b)), ("stp_predict_accumulate", ops.ptr(f), ops.ptr(fb))):
        assert rc(name, a, b, 2, 4, 4, 3, 0, st) == 0
        assert rc(name, None, b, 2, 4, 4, 3, 0, st) == BADARG and rc(name, a, None, 2, 4, 4, 3, 0, st) == BADARG
        assert rc(name, a, a, 2, 4, 4, 3, 0, st) == BADARG
        for dims in ((0, 4, 4, 3), (2, 0, 4, 3), (2, 4, 0, 3), (2, 4, 4, 0), (-1, 4, 4, 3)):
            assert rc(name, a, b, *dims, 0, st) == BADARG, (name, dims)
        for flip in (-1, 3):
            assert rc(name, a, b, 2, 4, 4, 3, flip, st) == BADARG, (name, flip)
    a, o = ops.ptr(f), ops.ptr(fb)
    good = dict(H=4, W=4, C=3, k=2, mode=0, h=5, w=6, ld=6)

    def finish(acc=a, out=o, **kw):
        g = dict(good, **kw)
        return rc("stp_predict_finish", acc, g["H"], g["W"], g["C"], g["k"], g["mode"], out, g["h"], g["w"], g["ld"], st)
    assert finish() == 0
    assert finish(acc=None) == BADARG and finish(out=None) == BADARG and finish(out=a) == BADARG
    for key in ("H", "W", "C", "k", "h", "w"):
        assert finish(**{key: 0}) == BADARG and finish(**{key: -2}) == BADARG, key
    assert finish(mode=-1) == BADARG and finish(mode=3) == BADARG
    assert finish(ld=5) == BADARG                                      # rows closer together than their length
    assert finish(mode=2, C=33, out=ops.ptr(u8)) == BADARG and finish(mode=2, C=32, out=ops.ptr(u8)) == 0
    torch.cuda.synchronize()
