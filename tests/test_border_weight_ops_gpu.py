"""stp_border_weight and stp_sigmoid_bce_dice_weighted on the GPU against tests/_border_weight_reference.py (include/stp_hip.h has the
arithmetic).

The squared distances are integers and must EQUAL the reference.  They are compared with the separable restatement at every shape and
radius, and with the window search of the header where that search is cheap (every shape at radius 1 and 3, the small shapes at 20 and
32); tests/test_border_weight_host.py holds the two restatements equal.  The map is held to 2e-6 * (w0 + max(b0, b1)) of the float64
value: the fp32 error of the exponent's argument a is a few 2^-24 * a and a * exp(-a) <= 1 / e, so the term errs by about w0 * 1e-7, plus
the rounding of the sum; the factor leaves room for a hardware exponential.

The weighted loss is compared with float64 at the tolerances of tests/test_masked_loss_gpu.py::compare (1e-5 relative on the scalars, two
threshold flips on the thresholded ones, REL per storage type plus 2e-5 of the largest gradient on the gradient)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _border_weight_reference as R  # noqa: E402
from test_softmax_losses_gpu import TD, dt_code, lib_for, quantise  # noqa: E402

STP_E_BADARG, STP_E_WORKSPACE = -1, -3
SHAPES = [(1, 1, 1), (2, 5, 7), (3, 33, 65), (2, 64, 64), (1, 40, 257), (2, 96, 130)]
RADII = [1, 3, 20, 32]
GUARD = 64


def run_border(L, w0, sigma, radius, b0=1.0, b1=1.0, distances=True, lib=None):
    """-> (weights float32 [n, h, w], d1sq, d2sq int32 or None); every output has GUARD sentinel elements behind it that must stay."""
    lib = lib or lib_for("fp32")[0]
    L = np.ascontiguousarray(L, np.int32)
    n, h, w = L.shape
    px = n * h * w
    ld = torch.from_numpy(L).cuda()
    wt = torch.full((px + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    d1 = torch.full((px + GUARD,), -7, dtype=torch.int32, device="cuda") if distances else None
    d2 = torch.full((px + GUARD,), -7, dtype=torch.int32, device="cuda") if distances else None
    nb = int(lib.stp_border_weight_workspace_bytes(n, h, w))
    assert nb >= px * 8
    ws = torch.full((nb + GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    rc = lib.stp_border_weight(ld.data_ptr(), n, h, w, w0, sigma, radius, b0, b1, wt.data_ptr(), d1.data_ptr() if distances else None,
                               d2.data_ptr() if distances else None, ws.data_ptr(), nb, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert (wt[px:] == -7.0).all() and (ws[nb:] == 0x5a).all(), "a launch wrote past its buffer"
    out = [wt[:px].cpu().numpy().reshape(n, h, w)]
    for d in (d1, d2):
        if d is not None:
            assert (d[px:] == -7).all(), "a launch wrote past its buffer"
        out.append(d[:px].cpu().numpy().reshape(n, h, w) if d is not None else None)
    return out


_REF = {}


def reference(key, L, radius, fn):
    k = (key, radius, fn.__name__)
    if k not in _REF:
        _REF[k] = fn(L, radius)
        for a in _REF[k]:
            a.setflags(write=False)
    return _REF[k]


def check(key, L, radius, w0=10.0, sigma=None, b0=1.0, b1=1.0, window=None):
    """One launch against the reference; ``window``: compare with the window search too (default: where it is cheap)."""
    L = np.ascontiguousarray(L, np.int32)
    w0, sigma, b0, b1 = (float(np.float32(v)) for v in (w0, radius / 4.0 if sigma is None else sigma, b0, b1))      # as the entry takes them
    got, d1, d2 = run_border(L, w0, sigma, radius, b0, b1)
    r1, r2 = reference(key, L, radius, R.distances_separable)
    assert np.array_equal(d1, r1) and np.array_equal(d2, r2), (key, radius, int((d1 != r1).sum()), int((d2 != r2).sum()))
    if window if window is not None else (radius <= 3 or L.size <= 100):
        s1, s2 = reference(key, L, radius, R.distances_window)
        assert np.array_equal(d1, s1) and np.array_equal(d2, s2), (key, radius)
    want = R.weight_from_distances(L, r1, r2, w0, sigma, b0, b1)
    err = np.abs(got.astype(np.float64) - want).max()
    bound = 2e-6 * (w0 + max(b0, b1))
    print("%s R=%d sigma=%g: max |map - float64| %.3g (bound %.3g), pixels with a term %d of %d" % (key, radius, sigma, err, bound, int(((r2 >= 0) & (L == 0)).sum()),
                                                                                                    L.size))
    assert err <= bound
    assert (got[L > 0] == b1).all()
    return got, d1, d2


def mask_kinds(n, h, w, seed):
    """{name: int32 label images [n, h, w]}"""
    rng = np.random.RandomState(seed)
    one = np.zeros((n, h, w), np.uint8)
    one[:, h // 3:h // 3 + max(1, h // 4), w // 4:w // 4 + max(1, w // 3)] = 1
    return {"empty": np.zeros((n, h, w), np.int32), "full": np.ones((n, h, w), np.int32),
            "one": np.stack([R.label(m) for m in one]),
            "blobs": np.stack([R.label(R.blobs(h, w, seed + i)) for i in range(n)]),
            "salt": np.stack([R.label(R.salt(h, w, seed + 10 + i)) for i in range(n)]),
            # any label image: values that touch, repeat in far corners and are not contiguous
            "touching": (rng.randint(1, 6, (n, h, w)) * 1000 * (rng.rand(n, h, w) < 0.35)).astype(np.int32)}


@pytest.mark.parametrize("shape", SHAPES)
def test_every_mask_kind_at_every_radius(shape):
    """Radii 1, 3, 20, 32 - at and past the image's height and width on the small shapes - with class balances and w0 that differ."""
    n, h, w = shape
    kinds = mask_kinds(n, h, w, seed=h + w)
    for i, (name, L) in enumerate(sorted(kinds.items())):
        for j, radius in enumerate(RADII):
            got, d1, d2 = check("%s%s" % (name, shape), L, radius, w0=(10.0, 3.5)[(i + j) % 2], b0=(1.0, 0.5)[j % 2], b1=(1.0, 2.0)[i % 2])
            if name == "empty":
                assert (d1 == -1).all() and (d2 == -1).all() and (got == got.flat[0]).all()
            if name == "full":
                assert (d1 == 0).all() and (d2 == -1).all()
            if name == "one":
                assert (d2 == -1).all() and ((d1 >= 0) | (L == 0)).all()


@pytest.mark.parametrize("radius", RADII)
def test_two_bars_show_the_edge_of_the_window(radius):
    """Two full-height bars k background columns apart, k = 1 .. R + 2, one sample per k: the pixel next to a bar sees the other bar at
    distance k, inside the window up to k = R and outside from k = R + 1 on."""
    h, w = 6, radius + 2 + 8
    L = np.zeros((radius + 2, h, w), np.int32)
    for k in range(1, radius + 3):
        L[k - 1, :, 1:3] = 1
        L[k - 1, :, 3 + k:5 + k] = 2
    got, d1, d2 = check("bars", L, radius, sigma=radius / 2.0, window=True)
    for k in range(1, radius + 3):
        beside = d2[k - 1, :, 3]                  # the background column next to the left bar
        assert (d1[k - 1, :, 3] == 1).all()
        assert (beside == (k * k if k <= radius else -1)).all(), (k, beside)
        assert ((got[k - 1, :, 3] > 1.0) == (k <= radius)).all()


def test_a_window_never_reaches_the_neighbouring_sample():
    L = np.zeros((2, 8, 40), np.int32)
    L[0, 7, 10:20] = 1                            # the bottom row of sample 0
    L[1, 0, 12:22] = 1                            # over the top row of sample 1
    for radius in (3, 32):
        got, d1, d2 = check("batch edge", L, radius, window=True)
        assert (d2 == -1).all() and (got == 1.0).all()
        assert d1[0, 6, 15] == 1 and d1[1, 1, 15] == 1 and d1[0, 0, 15] == (49 if radius == 32 else -1)
    # the same two rows inside ONE sample do see each other
    both = L.reshape(1, 16, 40).copy()
    both[0, 8] *= 2
    _, _, d2 = check("one sample", both, 3, window=True)
    assert d2[0, 7, 15] == 1 and d2[0, 6, 15] == 4


def test_without_the_distance_outputs_and_run_to_run():
    L = mask_kinds(2, 64, 64, seed=5)["blobs"]
    a = run_border(L, 10.0, 5.0, 20)
    b = run_border(L, 10.0, 5.0, 20)
    c = run_border(L, 10.0, 5.0, 20, distances=False)
    assert c[1] is None and c[2] is None
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    # both builds export the same code
    f16 = run_border(L, 10.0, 5.0, 20, lib=lib_for("fp16")[0])
    assert f16[0].tobytes() == a[0].tobytes() and f16[1].tobytes() == a[1].tobytes()


def test_the_thin_wrapper():
    from segmentation_training_pipeline_amd import ops
    L = mask_kinds(2, 33, 65, seed=9)["blobs"]
    ld = torch.from_numpy(L).cuda()
    out = torch.empty((2, 33, 65), dtype=torch.float32, device="cuda")
    d1 = torch.empty((2, 33, 65), dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.border_weight_workspace_bytes(2, 33, 65), dtype=torch.uint8, device="cuda")
    ops.border_weight(ld, 2, 33, 65, 10.0, 3.0, 12, 1.0, 1.0, out, ws, d1sq=d1)
    torch.cuda.synchronize()
    want = run_border(L, 10.0, 3.0, 12)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(d1.cpu().numpy(), want[1])
    with pytest.raises(ValueError):
        ops.border_weight(ld.to(torch.int64), 2, 33, 65, 10.0, 3.0, 12, 1.0, 1.0, out, ws)


def test_bad_arguments_are_refused_before_any_launch():
    lib = lib_for("fp32")[0]
    n, h, w = 2, 16, 24
    ld = torch.zeros((n, h, w), dtype=torch.int32, device="cuda")
    wt = torch.full((n * h * w,), -7.0, dtype=torch.float32, device="cuda")
    nb = int(lib.stp_border_weight_workspace_bytes(n, h, w))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    nan, inf = float("nan"), float("inf")

    def call(labels=ld.data_ptr(), N=n, H=h, W=w, w0=10.0, sigma=5.0, radius=20, b0=1.0, b1=1.0, weights=wt.data_ptr(), workspace=ws.data_ptr(),
             nbytes=nb):
        return lib.stp_border_weight(labels, N, H, W, w0, sigma, radius, b0, b1, weights, None, None, workspace, nbytes, st)
    for kw in (dict(labels=None), dict(weights=None), dict(workspace=None), dict(N=0), dict(H=0), dict(W=-1), dict(radius=0), dict(radius=33),
               dict(radius=-1), dict(w0=-0.5), dict(w0=nan), dict(w0=inf), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf),
               dict(sigma=1e-30), dict(b0=0.0), dict(b0=-1.0), dict(b0=nan), dict(b1=0.0), dict(b1=inf), dict(N=1 << 15, H=1 << 8, W=1 << 8)):
        assert call(**kw) == STP_E_BADARG, kw
    assert call(nbytes=nb - 1) == STP_E_WORKSPACE
    torch.cuda.synchronize()
    assert (wt == -7.0).all()                     # nothing was launched
    assert call() == 0 and call(w0=0.0) == 0 and call(radius=1) == 0 and call(radius=32) == 0
    torch.cuda.synchronize()
    assert (wt == 1.0).all()


# ------------------------------------------------------------------------------------------------ the weighted loss
BIG = 4096 * 256 + 300                                     # just past the gradient pass's grid cap (4096 workgroups of 256)
COUNTS = [1, 255, 256, 257, 3 * 1024 + 5, BIG]
REL = {"fp32": 1e-5, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}


def loss_case(count, seed):
    rng = np.random.RandomState(seed)
    z = (rng.randn(count) * 2.5).astype(np.float32)
    t = (rng.rand(count) < 0.3).astype(np.uint8)
    if count > 16:                                         # beyond the probability clip on both sides: no cross-entropy gradient there
        z[3], z[7], z[11], z[15] = 40.0, -40.0, 24.0, -24.0
        t[3], t[7] = 0, 1
    pw = np.where(rng.rand(count) < 0.5, 1.0, rng.uniform(0.5, 11.0, count)).astype(np.float32)
    return z, t, pw


def run_weighted(dtype, z, t, pw, w_bce, w_dice, dlc=8, grad_scale=1.0, with_grad=True, entry="stp_sigmoid_bce_dice_weighted", offset=0):
    """-> (scalars [16], gradient [count, dlc] float32 or None).  The gradient buffer is NaN-filled with GUARD elements behind it;
    ``offset`` shifts the operands by that many elements (the scalar path of the value pass)."""
    lib, _lib = lib_for(dtype)
    count = z.size
    zd = torch.zeros(count + offset, dtype=TD[dtype], device="cuda")
    zd[offset:] = torch.from_numpy(z).to(TD[dtype]).cuda()
    td = torch.zeros(count + offset, dtype=torch.uint8, device="cuda")
    td[offset:] = torch.from_numpy(t).cuda()
    sc = torch.full((16,), -3.0, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    dl = torch.full((count * dlc + GUARD,), float("nan"), dtype=TD[dtype], device="cuda") if with_grad else None
    st = torch.cuda.current_stream().cuda_stream
    args = [zd[offset:].data_ptr(), td[offset:].data_ptr(), count, dt_code(_lib, dtype), w_bce, w_dice, sc.data_ptr(),
            dl.data_ptr() if with_grad else None, dlc, grad_scale, ws.data_ptr(), ws.numel() * 4]
    if entry == "stp_sigmoid_bce_dice_weighted":
        pd = torch.zeros(count + offset, dtype=torch.float32, device="cuda")
        pd[offset:] = torch.from_numpy(pw).cuda()
        args.append(pd[offset:].data_ptr())
    rc = getattr(lib, entry)(*args, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    g = None
    if with_grad:
        full = dl.to(torch.float32).cpu().numpy()
        assert np.isnan(full[count * dlc:]).all(), "the gradient pass wrote past its tensor"
        g = full[:count * dlc].reshape(count, dlc)
    return sc.cpu().numpy(), g


def compare(dtype, sc, g, ref, gref, p, grad_scale, slots, what=""):
    """tests/test_masked_loss_gpu.py::compare for one class: scalars at 1e-5 relative (two flips of a probability within rounding of 0.5
    on the thresholded ones), the gradient at REL[dtype] relative + 2e-5 of its largest element, but for elements whose float64
    probability lies within float32 rounding of a clip bound."""
    n = p.size
    y_sum = ref[6]
    near = int((np.abs(p - 0.5) < 1e-5).sum())
    flip = (2 + near) * 2.0 / (2.0 * y_sum + 1.0)
    for i in slots:
        name = R.NAMES[i] if i < 10 else {13: "weighted_bce", 15: "weight_mean"}[i]
        tol = 1e-5 * max(1.0, abs(ref[i]))
        if name in ("dice", "iot"):
            tol += flip
        elif name == "acc":
            tol += (2 + near) / float(n)
        print("%s %s %-12s got %.9g ref %.9g tol %.3g" % (what, dtype, name, sc[i], ref[i], tol))
        assert abs(sc[i] - ref[i]) <= tol, (name, sc[i], ref[i])
    if g is None:
        return
    gs = gref * grad_scale
    scale = np.abs(gs).max() + 1e-30
    err = np.abs(g[:, 0] - gs)
    edge = (np.abs(p - 1e-7) < 1e-13) | (np.abs(p - (1.0 - 1e-7)) < 1.2e-7)
    ok = err <= REL[dtype] * np.abs(gs) + 2e-5 * scale
    print("   gradient: max err / scale %.3g, edge elements %d" % ((err / scale).max(), edge.sum()))
    assert (ok | edge).all(), (err[~(ok | edge)].max(), scale)
    assert edge.sum() <= max(8, 1e-5 * edge.size), edge.sum()
    assert (g[:, 1:] == 0).all(), "padding channels must be exactly zero"


def grad_scale_for(dtype, count, k):
    """1 and 2^14 alternate.  IEEE half takes the scale its build trains under where the unscaled 1 / count gradient falls below
    2e-5 * scale of half a subnormal step (count >= 3077), and 1 where 2^14 / count would overflow the format (count <= 257)."""
    if dtype == "fp16":
        return 16384.0 if count >= 3077 else 1.0
    return (1.0, 16384.0)[k % 2]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("count", COUNTS)
def test_weighted_loss_matches_float64(dtype, count):
    k = COUNTS.index(count)
    dlc = (1, 4, 8)[k % 3] if count < BIG else 8
    gsc = grad_scale_for(dtype, count, k)
    z, t, pw = loss_case(count, seed=count % 1000 + k)
    w_bce, w_dice = ((1.0, 1.0), (1.0, 0.0), (0.5, 2.0))[k % 3]
    ref, gref, p = R.weighted_loss(quantise(z, dtype), t, pw, w_bce, w_dice)
    sc, g = run_weighted(dtype, z, t, pw, w_bce, w_dice, dlc, gsc)
    compare(dtype, sc, g, ref, gref, p, gsc, list(range(10)) + [13, 15], "count=%d dlc=%d scale=%g" % (count, dlc, gsc))
    assert (sc[[10, 11, 12, 14]] == -3.0).all()               # slots the entry does not write
    assert np.isfinite(g).all()
    # the NULL gradient: the same scalars
    s_eval, none = run_weighted(dtype, z, t, pw, w_bce, w_dice, dlc, gsc, with_grad=False)
    assert none is None and np.array_equal(s_eval, sc)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("dlc", [1, 4, 8])
def test_every_gradient_row_width_and_the_unaligned_path(dtype, dlc):
    count = 3 * 1024 + 5
    z, t, pw = loss_case(count, seed=dlc)
    gsc = grad_scale_for(dtype, count, dlc)
    ref, gref, p = R.weighted_loss(quantise(z, dtype), t, pw, 1.0, 1.0)
    for offset in (0, 1):                                     # 1: operands off their vector alignment
        sc, g = run_weighted(dtype, z, t, pw, 1.0, 1.0, dlc, gsc, offset=offset)
        compare(dtype, sc, g, ref, gref, p, gsc, list(range(10)) + [13, 15], "dlc=%d offset=%d" % (dlc, offset))
    # a count that is a multiple of four on aligned operands takes the four-pixel path
    z, t, pw = loss_case(4096, seed=dlc + 50)
    ref, gref, p = R.weighted_loss(quantise(z, dtype), t, pw, 1.0, 0.5)
    sc, g = run_weighted(dtype, z, t, pw, 1.0, 0.5, dlc, gsc)
    compare(dtype, sc, g, ref, gref, p, gsc, list(range(10)) + [13, 15], "dlc=%d vector path" % dlc)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("count", [257, 4096, 3 * 1024 + 5])
def test_weights_of_one_give_the_sibling(dtype, count):
    z, t, _ = loss_case(count, seed=count)
    gsc = grad_scale_for(dtype, count, 0)
    ones = np.ones(count, np.float32)
    s_w, g_w = run_weighted(dtype, z, t, ones, 1.0, 0.5, 8, gsc)
    s_s, g_s = run_weighted(dtype, z, t, None, 1.0, 0.5, 8, gsc, entry="stp_sigmoid_bce_dice")
    p = 1.0 / (1.0 + np.exp(-quantise(z, dtype).astype(np.float64)))
    compare(dtype, s_w, g_w, s_s.astype(np.float64), g_s[:, 0].astype(np.float64) / gsc, p, gsc, list(range(10)), "ones count=%d" % count)
    assert abs(s_w[13] - s_w[1]) <= 1e-6 * max(1.0, abs(s_w[1])) and s_w[15] == 1.0


def test_two_launches_are_bit_identical_and_the_wrapper():
    from segmentation_training_pipeline_amd import ops
    z, t, pw = loss_case(40000, seed=4)
    a = run_weighted("bf16", z, t, pw, 1.0, 1.0)
    b = run_weighted("bf16", z, t, pw, 1.0, 1.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()      # fixed-order reduction, no atomics
    zd, td, pd = torch.from_numpy(z).to(torch.bfloat16).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(pw).cuda()
    sc = torch.full((16,), -3.0, dtype=torch.float32, device="cuda")
    dl = torch.empty((40000, 8), dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(ops.loss_workspace_bytes() // 4, dtype=torch.float32, device="cuda")
    ops.sigmoid_bce_dice_weighted(zd, td, 40000, 1.0, 1.0, sc, dl, 8, 1.0, ws, pd)
    torch.cuda.synchronize()
    assert np.array_equal(sc.cpu().numpy(), a[0]) and np.array_equal(dl.to(torch.float32).cpu().numpy(), a[1])


def test_weighted_loss_bad_arguments():
    lib, _lib = lib_for("fp32")
    zd = torch.zeros(1000, dtype=torch.float32, device="cuda")
    td = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    pd = torch.ones(1000, dtype=torch.float32, device="cuda")
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    dl = torch.zeros((1000, 8), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(logits=zd.data_ptr(), target=td.data_ptr(), count=1000, dtype=_lib.F32, scalars=sc.data_ptr(), dlc=8, workspace=ws.data_ptr(),
             nbytes=ws.numel() * 4, weights=pd.data_ptr(), lib_=lib):
        return lib_.stp_sigmoid_bce_dice_weighted(logits, target, count, dtype, 1.0, 1.0, scalars, dl.data_ptr(), dlc, 1.0, workspace, nbytes, weights, st)
    for kw in (dict(logits=None), dict(target=None), dict(scalars=None), dict(workspace=None), dict(weights=None), dict(count=0), dict(dlc=0),
               dict(dtype=77), dict(dtype=_lib.F16), dict(dtype=_lib.BF16, lib_=lib_for("fp16")[0])):
        assert call(**kw) == STP_E_BADARG, kw
    assert call(nbytes=16) == STP_E_WORKSPACE
    assert call() == 0
    torch.cuda.synchronize()
