"""stp_lovasz_softmax on the GPU, at op level: every case runs AFTER stp_softmax_loss_ex (or stp_softmax_loss_masked, when a label is ignored)
has written the scalars and the gradient, in fp32 and in both 16-bit builds, against the float64 evaluation of
tests/_lovasz_softmax_reference.py on the storage-quantised logits.

Bars.  Value: 2e-5 * max(1, |ref|) (the term is a convex combination of the errors - the rank weights sum to 1 - so its error is bounded by
the fp32 softmax's; the bar of tests/test_softmax_losses_gpu.py).  Gradient on SEPARATED inputs (consecutive sorted errors of a class differ
by >= 1e-4, checked here on the CPU: the order is then unambiguous in fp32): the added gradient to fp32 rounding, rtol 1e-4, plus what the
comparison itself rounds - the sum before + add is rounded once to fp32 (2^-24 |sum|, taken as 2^-23) and the row's sum_c p_c d_c carries the
fp32 rounding of its largest product (1e-6 of the largest element); in the 16-bit builds the summed value to one storage ulp.  Gradient on
RANDOM inputs: a swap of two neighbours in the order changes an element by at most 1 / G^2 against a largest element of about 1 / G, so with
G >= 200 the bar is atol = 1e-2 max|ref| (tests/test_ops_gpu.py does the same for the hinge), plus the storage rounding of the stored sum.

Where separated inputs exist: n errors of a class 1e-4 apart need n <= 10^4, and 20 classes share a total probability of 1, so the separated
cases are the 3- and 5-class shapes whole and the 20-class shape with 64 counted pixels (the rest ignored); the shape whose class segments
span several scan chunks (12 513 pixels) cannot be separated - there the all-equal logits of the tie test fix the order exactly instead."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _lovasz_softmax_reference as R  # noqa: E402
from test_softmax_losses_gpu import TD, dt_code, lib_for, quantise  # noqa: E402

STP_E_BADARG, STP_E_WORKSPACE = -1, -3
DTYPES = ["fp32", "bf16", "fp16"]
GAP = 1e-4


def chunk():
    from segmentation_training_pipeline_amd import _lib
    return _lib.LOVASZ_SOFTMAX_CHUNK


#         name: (pixels as N x H x W, classes, ldc, dlc)
SHAPES = {"c3": ((2, 24, 20), 3, 3, 8), "c5": ((1, 33, 17), 5, 8, 8), "c20": ((2, 16, 16), 20, 24, 24), "chunks": ((1, 97, 129), 3, 4, 8)}


def grad_scale_of(dtype):
    return 1024.0 if dtype == "fp16" else 1.0          # (IEEE half: keeps the 1 / pixels gradients in the normal range)


def storage_ulp(x, dtype):
    """The spacing of the storage type at |x| (float64 array)."""
    ax = np.abs(np.asarray(x, np.float64))
    if dtype == "fp32":
        return np.spacing(ax.astype(np.float32)).astype(np.float64)
    frac, emin = (7, -126) if dtype == "bf16" else (10, -14)
    e = np.floor(np.log2(np.maximum(ax, 2.0 ** emin)))
    return 2.0 ** (np.maximum(e, emin) - frac)


def balanced_targets(rng, pixels, present):
    present = np.asarray(present)
    return present[rng.permutation(np.arange(pixels) % present.size)].astype(np.uint8)


def pad_logits(zc, ldc):
    z = np.full((zc.shape[0], ldc), 1e4, np.float32)      # channels past `classes` must not be read into the loss
    z[:, :zc.shape[1]] = zc
    return z


def separated_case(dtype, pixels, classes, seed, counted=None, scale=1.0):
    """Logits (already representable in the storage type) whose errors, inside every class, lie in bins of width GAP no two of which are
    neighbours: consecutive sorted errors differ by >= GAP.  Pixel by pixel: random rows are drawn until every class finds its bin and
    both neighbours free.  ``counted``: that many pixels count, the rest carry the ignore label 255."""
    rng = np.random.RandomState(seed)
    t = rng.randint(0, classes, pixels).astype(np.uint8)
    on = np.ones(pixels, bool)
    if counted is not None:
        on[:] = False
        on[rng.permutation(pixels)[:counted]] = True
    nb = int(1.0 / GAP) + 3
    used = np.zeros((classes, nb), bool)
    z = np.zeros((pixels, classes), np.float32)
    cols = np.arange(classes)
    for i in range(pixels):
        for _ in range(20000):
            cand = quantise((rng.randn(classes) * scale).astype(np.float32), dtype)
            if not on[i]:
                break
            p = R.softmax(cand[None].astype(np.float64))[0]
            e = np.where(cols == t[i], 1.0 - p, p)
            b = np.floor(e / GAP).astype(np.int64) + 1
            if not (used[cols, b - 1] | used[cols, b] | used[cols, b + 1]).any():
                used[cols, b] = True
                break
        else:
            raise AssertionError("no separated row found for pixel %d" % i)
        z[i] = cand
    t[~on] = 255
    return z, t, (255 if counted is not None else None)


def run(dtype, z, t, classes, ldc, dlc, weight, ignore_label=None, w5=(1.0, 0, 0, 0, 0), with_grad=True, ws_bytes=None, guard=64,
        expect_rc=0, override=None):
    """The first loss launch, then stp_lovasz_softmax -> dict(sc0 / sc1: scalars[16] before / after, g0 / g1: the gradient [P, dlc] as
    float32 before / after, raw1: the gradient in its storage type, rc).  ``override``: arguments of the second launch replaced by name."""
    lib, _lib = lib_for(dtype)
    P = z.shape[0]
    zd = torch.from_numpy(np.array(z, np.float32)).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(np.array(t, np.uint8)).cuda()
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    dl = torch.full((P * dlc + guard,), float("nan"), dtype=TD[dtype], device="cuda") if with_grad else None
    dlp = dl.data_ptr() if dl is not None else None
    gs = grad_scale_of(dtype)
    st = torch.cuda.current_stream().cuda_stream
    w5c = (ctypes.c_float * 5)(*w5)
    if ignore_label is None:
        rc = lib.stp_softmax_loss_ex(zd.data_ptr(), td.data_ptr(), P, classes, ldc, dt_code(_lib, dtype), w5c, sc.data_ptr(), dlp, dlc, gs,
                                     ws.data_ptr(), ws.numel() * 4, st)
    else:
        rc = lib.stp_softmax_loss_masked(zd.data_ptr(), td.data_ptr(), P, classes, ldc, dt_code(_lib, dtype), w5c, sc.data_ptr(), dlp, dlc, gs,
                                         ws.data_ptr(), ws.numel() * 4, ignore_label, None, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = dict(sc0=sc.cpu().numpy(), g0=dl.to(torch.float32).cpu().numpy() if dl is not None else None)
    need = int(lib.stp_lovasz_softmax_workspace_bytes(P, classes))
    assert need > 0
    nbytes = need if ws_bytes is None else ws_bytes
    wl = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    a = dict(pixels=P, classes=classes, ldc=ldc, dtype=dt_code(_lib, dtype), dlc=dlc, ignore_label=-1 if ignore_label is None else ignore_label)
    a.update(override or {})
    rc = lib.stp_lovasz_softmax(zd.data_ptr(), td.data_ptr(), a["pixels"], a["classes"], a["ldc"], a["dtype"], weight, sc.data_ptr(), dlp,
                                a["dlc"], gs, a["ignore_label"], wl.data_ptr(), nbytes, st)
    assert rc == expect_rc, rc
    torch.cuda.synchronize()
    out.update(sc1=sc.cpu().numpy(), rc=rc, need=need)
    if dl is not None:
        full = dl.to(torch.float32).cpu().numpy()
        assert np.isnan(full[P * dlc:]).all(), "the gradient pass wrote past its tensor"
        out["g1"] = full[:P * dlc].reshape(P, dlc)
        out["g0"] = out["g0"][:P * dlc].reshape(P, dlc)
        out["raw1"] = dl[:P * dlc].cpu()
    return out


def check_value(dtype, out, ref, weight, what=""):
    got, want = float(out["sc1"][14]), ref["value"]
    print("%s %s lovasz_softmax got %.9g ref %.9g (present %d)" % (what, dtype, got, want, ref["present"]))
    assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (got, want)
    # scalars[0] grows by exactly weight * scalars[14] in fp32 (two roundings); every other slot stays
    assert out["sc1"][0] == np.float32(out["sc0"][0] + np.float32(np.float32(weight) * out["sc1"][14]))
    keep = [i for i in range(16) if i not in (0, 14)]
    assert (out["sc1"][keep] == out["sc0"][keep]).all()
    assert np.isfinite(out["sc1"]).all()


def check_untouched(out, ref, classes):
    """Rows of ignored pixels and padding channels are exactly what the first launch left (zeros), and everything is finite."""
    g0, g1 = out["g0"], out["g1"]
    assert np.isfinite(g1).all()
    assert (g1[:, classes:] == 0).all(), "padding channels must stay exactly zero"
    assert (g1[~ref["on"]] == 0).all(), "the rows of ignored pixels must stay exactly zero"
    if ref["present"] == 0:
        assert np.array_equal(g0, g1)


def check_separated(dtype, out, ref, weight, classes):
    assert R.min_error_gap(ref) >= GAP, R.min_error_gap(ref)           # the property of the INPUTS the comparison rests on
    gs = grad_scale_of(dtype)
    add = weight * gs * ref["dz"]
    g0, g1 = out["g0"][:, :classes].astype(np.float64), out["g1"][:, :classes].astype(np.float64)
    if dtype == "fp32":
        tol = 1e-4 * np.abs(add) + 2.0 ** -23 * np.abs(g1) + 1e-6 * np.abs(add).max()
        err = np.abs((g1 - g0) - add)
    else:
        want = g0 + add
        tol = storage_ulp(np.maximum(np.abs(want), np.abs(g1)), dtype)
        err = np.abs(g1 - want)
    print("   %s separated gradient: max err / tol %.3g, max |add| %.3g" % (dtype, (err / tol).max(), np.abs(add).max()))
    assert (err <= tol).all(), (err / tol).max()
    check_untouched(out, ref, classes)


def check_random(dtype, out, ref, weight, classes):
    G = ref["positives"]
    assert (G[G > 0] >= 200).all(), G
    gs = grad_scale_of(dtype)
    add = weight * gs * ref["dz"]
    g0, g1 = out["g0"][:, :classes].astype(np.float64), out["g1"][:, :classes].astype(np.float64)
    tol = 1e-2 * np.abs(add).max() + (0.0 if dtype == "fp32" else 1.0) * storage_ulp(g1, dtype) + 2.0 ** -23 * np.abs(g1)
    err = np.abs((g1 - g0) - add)
    print("   %s random gradient: max err / (1e-2 max|ref|) %.3g" % (dtype, err.max() / (1e-2 * np.abs(add).max())))
    assert (err <= tol).all(), (err.max(), np.abs(add).max())
    check_untouched(out, ref, classes)


# ------------------------------------------------------------------------------------------------ separated inputs
_SEP = {}


def separated(dtype, name):
    """(z, t, ignore_label, reference) of a separated case, built once per dtype and shared; never modified."""
    if (dtype, name) not in _SEP:
        (n, h, w), classes, ldc, dlc = SHAPES[name]
        pixels = n * h * w
        # 20 classes share a total probability of 1: 512 errors per class cannot keep 1e-4 apart, so an eighth of the pixels counts
        z, t, ign = separated_case(dtype, pixels, classes, seed=len(name) + classes, counted=64 if name == "c20" else None,
                                   scale=1.0)
        ref = R.reference(quantise(z, dtype), t, ign)
        for a in (z, t):
            a.setflags(write=False)
        _SEP[(dtype, name)] = (z, t, ign, ref)
    return _SEP[(dtype, name)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["c3", "c5", "c20"])
def test_separated_inputs_value_and_gradient(dtype, name):
    _shape, classes, ldc, dlc = SHAPES[name]
    z, t, ign, ref = separated(dtype, name)
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    check_value(dtype, out, ref, 0.5, name)
    check_separated(dtype, out, ref, 0.5, classes)


# ------------------------------------------------------------------------------------------------ random inputs
def random_case(name, seed, present=None, ignore=None):
    (n, h, w), classes, ldc, dlc = SHAPES[name]
    pixels = n * h * w
    rng = np.random.RandomState(seed)
    z = (rng.randn(pixels, classes) * 2.0).astype(np.float32)
    t = balanced_targets(rng, pixels, present if present is not None else np.arange(classes))
    ign = None
    if ignore == "random":
        t[rng.rand(pixels) < 0.15] = 255
        ign = 255
    elif ignore == "image":                       # the first image of the batch entirely ignored
        t[:h * w] = 255
        ign = 255
    elif ignore == "all":
        t[:] = 255
        ign = 255
    return z, t, ign


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,present", [("c3", None), ("c5", (1, 4)), ("c20", (0, 19)), ("chunks", None)])
def test_random_inputs_value_and_gradient(dtype, name, present):
    _shape, classes, ldc, dlc = SHAPES[name]
    z, t, ign = random_case(name, seed=7 + classes, present=present)
    ref = R.reference(quantise(z, dtype), t, ign)
    assert ref["present"] == (classes if present is None else len(present))
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.75, ign)
    check_value(dtype, out, ref, 0.75, name)
    check_random(dtype, out, ref, 0.75, classes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_class_segments_span_scan_chunks(dtype):
    """More than two chunks of counted pixels per class, a count that is no multiple of the chunk, with and without ignored pixels."""
    (n, h, w), classes, ldc, dlc = SHAPES["chunks"]
    for ignore in (None, "random"):
        z, t, ign = random_case("chunks", seed=3, ignore=ignore)
        ref = R.reference(quantise(z, dtype), t, ign)
        counted = int(ref["on"].sum())
        assert counted > 2 * chunk() and counted % chunk() and (n * h * w) % chunk()
        out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 1.0, ign, w5=(0, 0, 0, 0, 0))
        check_value(dtype, out, ref, 1.0, "chunks ignore=%s" % ignore)
        check_random(dtype, out, ref, 1.0, classes)


# ------------------------------------------------------------------------------------------------ the tie rule
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["c3", "chunks"])
def test_ties_follow_the_stable_order(dtype, name):
    """All logits equal: every error is one of two values per class, so the order inside a value is the tie rule alone (ascending pixel
    index) - across the chunk boundaries too.  The first launch has no weight: the gradient is the term's own, compared to rounding."""
    (n, h, w), classes, ldc, dlc = SHAPES[name]
    pixels = n * h * w
    rng = np.random.RandomState(5)
    z = np.zeros((pixels, classes), np.float32)
    t = rng.randint(0, classes, pixels).astype(np.uint8)
    ref = R.reference(z, t)
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 1.0, None, w5=(0, 0, 0, 0, 0))
    check_value(dtype, out, ref, 1.0, "ties " + name)
    assert (out["g0"][:, :classes] == 0).all()
    add = grad_scale_of(dtype) * ref["dz"]
    g1 = out["g1"][:, :classes].astype(np.float64)
    # fp32: rtol 1e-4 and the rounding of the row's sum_c p_c d_c (1e-6 of the largest coefficient, which is 1 / G: ranks near the end of
    # the order have coefficients ~ 1 / n^2, far below the rounding of that sum); 16-bit: one storage ulp on top
    big = np.abs(ref["dz"]).max() * grad_scale_of(dtype) * classes
    tol = 1e-4 * np.abs(add) + 1e-6 * big + (0.0 if dtype == "fp32" else 1.0) * storage_ulp(add, dtype)
    err = np.abs(g1 - add)
    print("   %s ties %s: max err / tol %.3g" % (dtype, name, (err / tol).max()))
    assert (err <= tol).all(), (err / tol).max()


# ------------------------------------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_class_absent(dtype):
    _shape, classes, ldc, dlc = SHAPES["c3"]
    z, t, ign = random_case("c3", seed=21, present=(0, 2))
    ref = R.reference(quantise(z, dtype), t, ign)
    assert ref["present"] == classes - 1
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    check_value(dtype, out, ref, 0.5, "absent")
    check_random(dtype, out, ref, 0.5, classes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_class_owns_every_counted_pixel(dtype):
    _shape, classes, ldc, dlc = SHAPES["c5"]
    z, t, ign = random_case("c5", seed=22, present=(3,), ignore="random")
    ref = R.reference(quantise(z, dtype), t, ign)
    assert ref["present"] == 1
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    check_value(dtype, out, ref, 0.5, "one class")
    # every rank of the class is a positive: g = 1 / G at every rank, whatever the order - the gradient is exact to rounding
    check_random(dtype, out, ref, 0.5, classes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_image_entirely_ignored(dtype):
    _shape, classes, ldc, dlc = SHAPES["c3"]
    z, t, ign = random_case("c3", seed=23, present=(0, 1), ignore="image")
    ref = R.reference(quantise(z, dtype), t, ign)
    assert not ref["on"][:24 * 20].any() and ref["on"][24 * 20:].all()
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    check_value(dtype, out, ref, 0.5, "image ignored")
    check_random(dtype, out, ref, 0.5, classes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_everything_ignored(dtype):
    _shape, classes, ldc, dlc = SHAPES["c3"]
    z, t, ign = random_case("c3", seed=24, ignore="all")
    ref = R.reference(quantise(z, dtype), t, ign)
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    assert out["sc1"][14] == 0.0 and out["sc1"][0] == out["sc0"][0] and np.isfinite(out["sc1"]).all()
    assert np.array_equal(out["g0"], out["g1"]) and np.isfinite(out["g1"]).all()
    check_untouched(out, ref, classes)


@pytest.mark.parametrize("dtype", DTYPES)
def test_null_gradient_writes_scalars_only(dtype):
    _shape, classes, ldc, dlc = SHAPES["c5"]
    z, t, ign = random_case("c5", seed=25, ignore="random")
    ref = R.reference(quantise(z, dtype), t, ign)
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign, with_grad=False)
    check_value(dtype, out, ref, 0.5, "no gradient")
    with_grad = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    assert np.array_equal(out["sc1"], with_grad["sc1"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_runs_are_bit_identical(dtype):
    _shape, classes, ldc, dlc = SHAPES["chunks"]
    z, t, ign = random_case("chunks", seed=26, ignore="random")
    a = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    b = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign)
    assert a["sc1"].tobytes() == b["sc1"].tobytes()
    assert torch.equal(a["raw1"].view(torch.int16 if dtype != "fp32" else torch.int32), b["raw1"].view(torch.int16 if dtype != "fp32" else torch.int32))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_bad_arguments_are_refused_without_a_launch(dtype):
    _shape, classes, ldc, dlc = SHAPES["c5"]
    z, t, ign = random_case("c5", seed=27)
    _lib = lib_for(dtype)[1]
    other = {"fp32": 7, "bf16": _lib.F16, "fp16": _lib.BF16}[dtype]          # the other build's 16-bit code (fp32: garbage)
    bad = [dict(classes=1), dict(classes=33), dict(ldc=classes - 1), dict(dlc=classes - 1), dict(pixels=0), dict(pixels=(1 << 31) // classes + 1),
           dict(ignore_label=-2), dict(ignore_label=256), dict(dtype=other)]
    for override in bad:
        out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign, expect_rc=STP_E_BADARG, override=override)
        assert np.array_equal(out["sc0"], out["sc1"]) and np.array_equal(out["g0"], out["g1"]), override
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign, expect_rc=STP_E_WORKSPACE, ws_bytes=1024)
    assert np.array_equal(out["sc0"], out["sc1"]) and np.array_equal(out["g0"], out["g1"])
    short = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign, expect_rc=0)
    out = run(dtype, pad_logits(z, ldc), t, classes, ldc, dlc, 0.5, ign, expect_rc=STP_E_WORKSPACE, ws_bytes=short["need"] - 16)
    assert np.array_equal(out["sc0"], out["sc1"]) and np.array_equal(out["g0"], out["g1"])
    lib = lib_for(dtype)[0]
    assert lib.stp_lovasz_softmax_workspace_bytes(0, 3) == 0 and lib.stp_lovasz_softmax_workspace_bytes(100, 1) == 0
    assert lib.stp_lovasz_softmax_workspace_bytes(100, 33) == 0 and lib.stp_lovasz_softmax_workspace_bytes((1 << 31) // 3 + 1, 3) == 0
    assert lib.stp_lovasz_softmax_workspace_bytes(1 << 20, 20) >= 24 * 20 * (1 << 20)
