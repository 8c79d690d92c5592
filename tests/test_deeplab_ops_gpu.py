"""GPU op tests of csrc/deeplab.hip (depthwise convolution and its two gradients, align-corners resize and its gradient, element
dropout, sigmoid activation and its gradient) and of the ReLU6 BatchNormalization (relu = 2 of bn.hip / common.h), in fp32 and in
both 16-bit builds.  Each C-ABI entry point is called directly and compared with the float64 numpy restatement of
tests/_deeplab_reference.py - never with a second run of a kernel, and with no tolerance derived from a kernel's output:

* EXACT cases (small integers, dyadic resize ratios, the ReLU6 grid): every product and partial sum is exact in fp32 and the result is
  representable in bf16 and IEEE half (tests/test_deeplab_reference_host.py asserts that condition on these very inputs), so the
  kernel must equal the reference bit for bit in whatever order it adds: ``np.array_equal``.
* ROUNDED cases (random normal inputs, rounded to storage first): the per-element ``rounding_bound`` of the reference - one storage
  rounding of the result plus a worst-case fp32 sum of the element's own absolute products.  The operation counts passed as
  ``n_terms`` are derived next to each call.

A destination that is not accumulated into is pre-filled with NaN, a second identical launch must give identical bytes, refusals are
checked on the return code.  The shapes are the smallest that reach each path: a second trip of the weight gradient's
row loop, a ragged channel slab, dilations beyond the map, tensors above the 4 194 304-item grid of the element-wise launchers.
"""
import functools

import numpy as np
import pytest
import torch

import _deeplab_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = R.TD
DTYPES = R.DTYPES
BADARG, E_WORKSPACE = -1, -3
CAP_DL = R.CAP_DL


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from segmentation_training_pipeline_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _storage_build(request):
    """Tests parametrized with dtype "fp16" call into libstp_hip_f16.so (IEEE-half storage)."""
    from segmentation_training_pipeline_amd import _lib
    dt = request.node.callspec.params.get("dtype") if hasattr(request.node, "callspec") else None
    with _lib.storage("fp16" if dt == "fp16" else "bf16"):
        yield


q = R.through
_KEEP = []


def keep(t):
    _KEEP.append(t)
    return t


def dev(a, dtype):
    """Device copy in the storage dtype, parked until the test ends (the C-ABI holds raw pointers only)."""
    return keep(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TD[dtype]).to(DEV).contiguous())


def nans(shape, dtype):
    return keep(torch.full(shape, float("nan"), dtype=TD[dtype], device=DEV))


def f32(a):
    return keep(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV))


@pytest.fixture(autouse=True)
def _release_device_temporaries():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def host(t):
    torch.cuda.synchronize()
    return t.detach().to(torch.float32).cpu().numpy()


def raw(t):
    torch.cuda.synchronize()
    return t.detach().contiguous().view(torch.uint8).cpu().numpy()


def call(name, *args):
    from segmentation_training_pipeline_amd import _lib
    _lib.call(name, *args)


def rc(name, *args):
    """Return code of a C-ABI call (refusal checks: nothing may be launched, so nothing is synchronised or read afterwards)."""
    from segmentation_training_pipeline_amd import _lib
    return int(getattr(_lib.load(), name)(*args))


def twice(make_dst, launch):
    """Runs ``launch(dst)`` on two destinations made the same way; the second launch must give identical bytes.  -> the first."""
    a, b = make_dst(), make_dst()
    launch(a)
    launch(b)
    assert np.array_equal(raw(a), raw(b)), "a second identical launch gave different bytes"
    return a


def exact(got, want):
    """Equal as numbers with no NaN anywhere (+0 and -0 are the same value)."""
    return not np.isnan(got).any() and np.array_equal(got, np.asarray(want).astype(got.dtype))


def within(got, ref, bound, what):
    assert not np.isnan(got).any(), what + ": an element was not written"
    err = np.abs(got.astype(np.float64) - ref)
    print("%s: max error / bound = %.3f" % (what, float((err / np.maximum(bound, 1e-300)).max())))
    bad = err > bound
    assert not bad.any(), "%s: %d of %d elements outside the bound, worst %.3g against %.3g" % (
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(bound[bad][err[bad].argmax()]))


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise convolution

@functools.lru_cache(maxsize=None)
def dw_exact_reference(case):
    d = R.dw_exact_inputs(case)
    n, h, w, c, k, stride, pt, pl, dil, ho, wo = d["geom"]
    d["y"] = R.dwconv(d["x"], d["w"], stride, pt, pl, dil, ho, wo)[0]
    d["dx"] = [R.dwconv_dgrad(d["dy"], d["w"], d["x"].shape, stride, pt, pl, dil, b)[0] for b in (None, d["base_dx"])]
    d["dw"] = [R.dwconv_wgrad(d["x"], d["dy"], k, stride, pt, pl, dil, b)[0] for b in (None, d["base_dw"])]
    return d


def dw_run(ops, d, dtype):
    """All five launches of a depthwise case -> y, [dx, dx accumulated], [dw, dw accumulated]."""
    n, h, w, c, k, stride, pt, pl, dil, ho, wo = d["geom"]
    xd, dyd, wd = dev(d["x"], dtype), dev(d["dy"], dtype), f32(d["w"])
    geo = d["geom"] + (ops.dt(xd),)
    st = ops.stream()
    y = twice(lambda: nans((n, ho, wo, c), dtype), lambda t: call("stp_dwconv", ops.ptr(xd), ops.ptr(wd), ops.ptr(t), *geo, st))
    ws_bytes = rc("stp_dwconv_wgrad_workspace_bytes", c, k)
    assert ws_bytes == 128 * k * k * c * 4
    dxs, dws = [], []
    for acc in (0, 1):
        dxs.append(twice(lambda: dev(d["base_dx"], dtype) if acc else nans((n, h, w, c), dtype),
                         lambda t: call("stp_dwconv_dgrad", ops.ptr(dyd), ops.ptr(wd), ops.ptr(t), *geo, acc, st)))
        ws = keep(torch.full((ws_bytes // 4,), float("nan"), dtype=torch.float32, device=DEV))
        dws.append(twice(lambda: f32(d["base_dw"]) if acc else nans((k, k, c), "fp32"),
                         lambda t: call("stp_dwconv_wgrad", ops.ptr(xd), ops.ptr(dyd), ops.ptr(t), *geo, acc, ops.ptr(ws), ws_bytes, st)))
    return y, dxs, dws


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.DW_EXACT_CASES, ids=R.dw_case_id)
def test_deeplab_depthwise_convolution_and_gradients_bit_equal_on_integers(ops, dtype, case):
    """stp_dwconv / stp_dwconv_dgrad / stp_dwconv_wgrad (k = 3, TF 'same') on small integers: every product and sum is exact in fp32 and
    representable in both 16-bit formats, so forward, data gradient (accumulate 0 and 1) and weight gradient (accumulate 0 and 1) equal
    the float64 reference bit for bit."""
    d = dw_exact_reference(case)
    y, dxs, dws = dw_run(ops, d, dtype)
    assert exact(host(y), d["y"]), "forward"
    for acc in (0, 1):
        assert exact(host(dxs[acc]), d["dx"][acc]), "data gradient, accumulate = %d" % acc
        assert exact(host(dws[acc]), d["dw"][acc]), "weight gradient, accumulate = %d" % acc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.DW_ROUNDED_CASES, ids=R.dw_case_id)
def test_deeplab_depthwise_convolution_and_gradients_within_the_rounding_bound(ops, dtype, case):
    """The same launches on random normal operands (rounded to storage first; fp32 master weights).  n_terms: an output element is a
    chain of at most 9 fused multiply-adds (+ one addition of the accumulated base, inside the bound's + 2); a weight-gradient element
    is an fp32 sum of at most N * Ho * Wo products in some order (the result is fp32 whatever the storage dtype)."""
    d = R.dw_rounded_inputs(case, dtype)
    n, h, w, c, k, stride, pt, pl, dil, ho, wo = d["geom"]
    y, dxs, dws = dw_run(ops, d, dtype)
    ref, a = R.dwconv(d["x"], d["w"], stride, pt, pl, dil, ho, wo)
    within(host(y), ref, R.rounding_bound(ref, a, k * k, dtype), "forward")
    for acc in (0, 1):
        ref, a = R.dwconv_dgrad(d["dy"], d["w"], d["x"].shape, stride, pt, pl, dil, d["base_dx"] if acc else None)
        within(host(dxs[acc]), ref, R.rounding_bound(ref, a, k * k, dtype), "data gradient, accumulate = %d" % acc)
        ref, a = R.dwconv_wgrad(d["x"], d["dy"], k, stride, pt, pl, dil, d["base_dw"] if acc else None)
        within(host(dws[acc]), ref, R.rounding_bound(ref, a, n * ho * wo, "fp32"), "weight gradient, accumulate = %d" % acc)


def test_deeplab_depthwise_refusals(ops):
    """C % 4 != 0, more rows than the grid's y extent (N * Ho > 65535 forward, N * H > 65535 data gradient) and a workspace one byte
    short (STP_E_WORKSPACE) are refused before any launch."""
    t = keep(torch.zeros(128 * 9 * 8, dtype=torch.float32, device=DEV))
    p, st = ops.ptr(t), ops.stream()
    geom = lambda n, h, w, c: (n, h, w, c, 3, 1, 1, 1, 1, h, w, ops.F32)
    for g in (geom(1, 4, 4, 6), geom(1, 4, 4, 2), geom(0, 4, 4, 4)):
        assert rc("stp_dwconv", p, p, p, *g, st) == BADARG
        assert rc("stp_dwconv_dgrad", p, p, p, *g, 0, st) == BADARG
        assert rc("stp_dwconv_wgrad", p, p, p, *g, 0, p, t.numel() * 4, st) == BADARG
    g = geom(32768, 2, 1, 4)
    assert rc("stp_dwconv", p, p, p, *g, st) == BADARG
    assert rc("stp_dwconv_dgrad", p, p, p, *g, 0, st) == BADARG
    need = rc("stp_dwconv_wgrad_workspace_bytes", 8, 3)
    assert need == t.numel() * 4
    assert rc("stp_dwconv_wgrad", p, p, p, *geom(1, 4, 4, 8), 0, p, need - 1, st) == E_WORKSPACE
    assert rc("stp_dwconv", p, p, p, *geom(1, 4, 4, 4)[:-1], 77, st) == BADARG          # not a dtype code


# ---------------------------------------------------------------------------------------------------------------------------------
# align-corners bilinear resize

@functools.lru_cache(maxsize=None)
def resize_exact_reference(case):
    n, h, w, c, ho, wo, which = case
    d = R.resize_exact_inputs(case)
    if which != "bwd":
        d["y"] = R.resize_ac(d["x"], ho, wo)[0].astype(np.float32)
    if which != "fwd":
        d["dx"] = [R.resize_ac_bwd(d["dy"], h, w, b)[0].astype(np.float32) for b in (None, d["base"])]
    return d


def resize_run(ops, d, dtype, n, h, w, c, ho, wo, which="both"):
    st = ops.stream()
    y, dxs = None, []
    if which != "bwd":
        xd = dev(d["x"], dtype)
        y = twice(lambda: nans((n, ho, wo, c), dtype),
                  lambda t: call("stp_resize_bilinear_ac", ops.ptr(xd), ops.ptr(t), n, h, w, c, ho, wo, ops.dt(xd), st))
    if which != "fwd":
        dyd = dev(d["dy"], dtype)
        for acc in (0, 1):
            dxs.append(twice(lambda: dev(d["base"], dtype) if acc else nans((n, h, w, c), dtype),
                             lambda t: call("stp_resize_bilinear_ac_bwd", ops.ptr(dyd), ops.ptr(t), n, h, w, c, ho, wo, ops.dt(dyd), acc, st)))
    return y, dxs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.RESIZE_EXACT_CASES, ids=R.resize_case_id)
def test_deeplab_align_corners_resize_and_gradient_bit_equal_at_dyadic_ratios(ops, dtype, case):
    """stp_resize_bilinear_ac / _bwd at ratios whose fractions are multiples of 1/4, on small integers: every step of the interpolation
    and of the gather is exact, so forward and gradient (accumulate 0 and 1) equal Ry . x . Rx^T and its adjoint bit for bit - also
    where every thread takes a second trip of the grid-stride loop (the two 129 x 129 cases)."""
    n, h, w, c, ho, wo, which = case
    if which == "fwd":
        assert n * ho * wo * c > CAP_DL
    if which == "bwd":
        assert n * h * w * c > CAP_DL
    d = resize_exact_reference(case)
    y, dxs = resize_run(ops, d, dtype, n, h, w, c, ho, wo, which)
    if which != "bwd":
        assert exact(host(y), d["y"]), "forward"
    if which != "fwd":
        for acc in (0, 1):
            assert exact(host(dxs[acc]), d["dx"][acc]), "gradient, accumulate = %d" % acc


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.RESIZE_ROUNDED_CASES, ids=R.resize_case_id)
def test_deeplab_align_corners_resize_and_gradient_within_the_rounding_bound(ops, dtype, case):
    """An upscale and a DOWNSCALE at ratios that are not dyadic, random normal operands.  n_terms: the forward evaluates
    v0 + (v1 - v0) * f three times (two rows, then between them): 9 roundings, each relative to a partial result that the absolute
    coefficients of that form bound (1 + f at v0, f at v1: R.resize_ac) - n_terms = 8.  The gradient gathers at most ``terms`` outputs,
    each weight (1 - fy) * (1 - fx) * dy costing 4 roundings and each addition one: n_terms = terms + 4."""
    n, h, w, c, ho, wo = case
    d = R.resize_rounded_inputs(case, dtype)
    y, dxs = resize_run(ops, d, dtype, n, h, w, c, ho, wo)
    ref, a = R.resize_ac(d["x"], ho, wo)
    within(host(y), ref, R.rounding_bound(ref, a, 8, dtype), "forward")
    for acc in (0, 1):
        ref, a, terms = R.resize_ac_bwd(d["dy"], h, w, d["base"] if acc else None)
        within(host(dxs[acc]), ref, R.rounding_bound(ref, a, terms + 4, dtype), "gradient, accumulate = %d" % acc)


# ---------------------------------------------------------------------------------------------------------------------------------
# dropout

DROP_COUNT = CAP_DL + 1077


@functools.lru_cache(maxsize=None)
def dropout_input(dtype):
    x = q(np.random.RandomState(61).randn(DROP_COUNT) + 0.25, dtype)
    x[x == 0] = 1.0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rate", [0.1, 0.25])
def test_deeplab_dropout_equals_the_oracles_mask_above_the_grid_cap_and_in_place(ops, dtype, rate):
    """stp_dropout on 4 194 304 + 1 077 elements (every thread of the capped grid takes a second trip, the last one ragged), two salts,
    step counter 0 and - after stp_counter_tick - 1, out of place and in place: the output equals the reference exactly (the oracle's
    mask; float32(x) * (1 / (1 - rate)) rounded once to storage).  The mask depends on the index only: the first 5 000 elements equal a
    5 000-element launch."""
    x = dropout_input(dtype)
    xd = dev(x, dtype)
    state = keep(torch.zeros(2, dtype=torch.int32, device=DEV))
    st = ops.stream()
    for step in (0, 1):
        if step:
            call("stp_counter_tick", ops.ptr(state), st)
        assert state.cpu().tolist() == [step, 0]
        for salt in (7, 0x0D0D):
            want = R.dropout(x, step, salt, rate, dtype)
            assert 0.5 * rate < (want == 0).mean() < 1.5 * rate
            launch = lambda t, src=None: call("stp_dropout", ops.ptr(xd if src is None else src), ops.ptr(t), DROP_COUNT, rate, ops.ptr(state), salt,
                                              ops.dt(xd), st)
            y = twice(lambda: nans((DROP_COUNT,), dtype), launch)
            assert exact(host(y), want), "out of place, step %d, salt %d" % (step, salt)
            inplace = dev(x, dtype)
            launch(inplace, inplace)
            assert np.array_equal(raw(inplace), raw(y)), "in place, step %d, salt %d" % (step, salt)
    small = nans((5000,), dtype)
    call("stp_dropout", ops.ptr(xd), ops.ptr(small), 5000, rate, ops.ptr(state), 0x0D0D, ops.dt(xd), st)
    assert np.array_equal(raw(small), raw(y[:5000]))
    assert np.array_equal(host(xd), x)                                       # the source of the out-of-place launches is intact


@pytest.mark.parametrize("dtype", DTYPES)
def test_deeplab_dropout_rate_zero_returns_the_input_bytes_and_refusals(ops, dtype):
    x = dropout_input(dtype)[:70001]
    xd, y = dev(x, dtype), nans((70001,), dtype)
    state = keep(torch.zeros(2, dtype=torch.int32, device=DEV))
    p, ps, st = ops.ptr(xd), ops.ptr(state), ops.stream()
    call("stp_dropout", p, ops.ptr(y), 70001, 0.0, ps, 3, ops.dt(xd), st)
    assert np.array_equal(raw(y), raw(xd))
    for count, rate in ((100, -0.01), (100, 1.0), (100, 1.5), (0, 0.1), (-5, 0.1)):
        assert rc("stp_dropout", p, ops.ptr(y), count, rate, ps, 3, ops.dt(xd), st) == BADARG, (count, rate)
    assert rc("stp_dropout", p, ops.ptr(y), 100, 0.1, None, 3, ops.dt(xd), st) == BADARG
    assert np.array_equal(raw(y), raw(xd))                                   # a refused call launched nothing


# ---------------------------------------------------------------------------------------------------------------------------------
# sigmoid activation

SIG_EDGES = [0.0, -0.0, 17.0, -17.0, 88.0, -88.0, 104.0, -104.0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_deeplab_sigmoid_activation_above_the_grid_cap_with_padded_rows(ops, dtype):
    """stp_sigmoid_act on 1 400 000 rows x 3 channels (4 200 000 items: above the cap) read from 8-column rows into 4-column rows:
    1e-6 in fp32, one storage rounding + 1e-6 in 16 bit (the bound the project states for this kernel); the logits include
    +-0, +-17, +-88 (exp near the fp32 limit) and +-104 (beyond it); column 3 of p keeps its sentinel."""
    rows, ch, ldz, ldp = 1400000, 3, 8, 4
    assert rows * ch > CAP_DL
    z = np.random.RandomState(62).randn(rows, ldz).astype(np.float32) * 3
    for i, v in enumerate(SIG_EDGES):
        z[i, :] = v
    z = q(z, dtype)
    with np.errstate(over="ignore"):
        ref = R.sigmoid_act(z, ch)
    zd = dev(z, dtype)
    p = twice(lambda: keep(torch.full((rows, ldp), -3.0, dtype=TD[dtype], device=DEV)),
              lambda t: call("stp_sigmoid_act", ops.ptr(zd), ops.ptr(t), rows, ch, ldz, ldp, ops.dt(zd), ops.stream()))
    got = host(p)
    assert np.array_equal(got[:, ch:], np.full((rows, ldp - ch), -3.0, np.float32))
    within(got[:, :ch], ref, (0.0 if dtype == "fp32" else R.U[dtype]) * ref + 1e-6, "sigmoid")
    assert (got[:, :ch] >= 0).all() and (got[:, :ch] <= 1).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_deeplab_sigmoid_activation_gradient_above_the_grid_cap_and_in_place(ops, dtype):
    """stp_sigmoid_act_bwd on 600 000 rows of 8 gradient columns (4 800 000 items), p in 4-column rows: dz = dp * p * (1 - p) - three
    roundings, n_terms = 3 - in the first 3 columns, exact zeros behind them; out of place and with dp == dz."""
    rows, ch, ldp, ldg = 600000, 3, 4, 8
    assert rows * ldg > CAP_DL
    rng = np.random.RandomState(63)
    p = q(1.0 / (1.0 + np.exp(-rng.randn(rows, ldp) * 3)), dtype)
    p[:4, :ch] = np.array([0.0, 1.0, 0.5, 0.25], np.float32)[:, None]
    dp = q(rng.randn(rows, ldg), dtype)
    ref, a = R.sigmoid_act_bwd(p, dp, ch)
    pd, dpd = dev(p, dtype), dev(dp, dtype)
    launch = lambda t, src=None: call("stp_sigmoid_act_bwd", ops.ptr(pd), ops.ptr(dpd if src is None else src), ops.ptr(t), rows, ch, ldp, ldg,
                                      ops.dt(pd), ops.stream())
    dz = twice(lambda: nans((rows, ldg), dtype), launch)
    got = host(dz)
    assert not got[:, ch:].any() and not np.isnan(got).any()
    within(got[:, :ch], ref[:, :ch], R.rounding_bound(ref[:, :ch], a[:, :ch], 3, dtype), "sigmoid gradient")
    inplace = dev(dp, dtype)
    launch(inplace, inplace)
    assert np.array_equal(raw(inplace), raw(dz)), "dp == dz"
    assert np.array_equal(host(dpd), dp)


def test_deeplab_sigmoid_activation_refusals(ops):
    t = keep(torch.zeros(4096, dtype=torch.float32, device=DEV))
    p, st = ops.ptr(t), ops.stream()
    assert rc("stp_sigmoid_act", p, p, 16, 3, 8, 2, ops.F32, st) == BADARG                # ldp < channels
    assert rc("stp_sigmoid_act", p, p, 16, 3, 2, 4, ops.F32, st) == BADARG                # ldz < channels
    assert rc("stp_sigmoid_act_bwd", p, p, p, 16, 3, 2, 8, ops.F32, st) == BADARG         # ldp < channels
    assert rc("stp_sigmoid_act_bwd", p, p, p, 16, 3, 4, 2, ops.F32, st) == BADARG         # ldg < channels
    assert rc("stp_sigmoid_act", p, p, 0, 3, 8, 4, ops.F32, st) == BADARG
    assert rc("stp_sigmoid_act_bwd", p, p, p, 16, 0, 4, 8, ops.F32, st) == BADARG


# ---------------------------------------------------------------------------------------------------------------------------------
# ReLU6 through BatchNormalization

def unit_parameters(C):
    """mean 0, rstd 1, gamma 1, beta 0: scale = 1 and shift = 0 exactly, so the pre-activation fma(x, 1, 0) is x itself."""
    return f32(np.zeros(C)), f32(np.ones(C)), f32(np.ones(C)), f32(np.zeros(C))


def ulp(v, dtype):
    """Spacing of the storage format at |v| (0 at 0)."""
    v = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, 2.0 ** e * 2.0 * R.U[dtype], 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", R.RELU6_CHANNELS)
def test_batchnorm_relu6_forward_is_an_exact_clip_on_the_grid(ops, dtype, C):
    """stp_bn_apply(relu = 2) with unit parameters on {-1, -0.0, 0, 2^-7, 0.5, 5.96875, 6, 6.03125, 7, 100}: clip(x, 0, 6) exactly, through
    the table-driven, the 4-wide and (C % 8 == 0, 16 bit) the 8-wide kernel; stp_bn_inference(relu = 2) with moving_mean 0 and
    moving_var 1 - eps within one storage ulp (1 - eps + eps need not be 1 in fp32) and never above 6 or below 0;
    stp_bn_finalize_apply(relu = 2), where it is eligible, on statistics that give mean 0 and rstd 1 exactly."""
    rows = R.RELU6_ROWS
    x = R.relu6_grid_input(C)
    want = R.bn_act(x, 2)
    xd = dev(x, dtype)
    m, r, g, b = unit_parameters(C)
    y = twice(lambda: nans((rows, C), dtype), lambda t: ops.bn_apply(xd, t, rows, C, C, m, r, g, b, relu=2))
    assert exact(host(y), want), "stp_bn_apply"
    y0 = nans((rows, C), dtype)
    ops.bn_apply(xd, y0, rows, C, C, m, r, g, b, relu=0)
    assert exact(host(y0), x), "stp_bn_apply, relu = 0"
    eps = np.float32(1e-3)
    mv = f32(np.full(C, np.float32(1) - eps))
    yi = twice(lambda: nans((rows, C), dtype), lambda t: ops.bn_inference(xd, t, rows, C, C, m, mv, float(eps), g, b, relu=2))
    got = host(yi)
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - want)
    print("stp_bn_inference: max error in storage ulps = %.3f" % float((err / np.maximum(ulp(want, dtype), 1e-300)).max()))
    assert (err <= ulp(want, dtype)).all() and got.min() >= 0 and got.max() <= 6
    assert np.array_equal(got[x <= 0], np.zeros((x <= 0).sum(), np.float32)) and np.array_equal(got[x > 6], np.full((x > 6).sum(), 6, np.float32))
    ok = rc("stp_bn_finalize_apply_ok", ops.dt(xd), rows, C, 4)
    assert ok == int(dtype != "fp32" and C % 64 == 0)
    if ok:
        # sum x = 0 and sum x^2 = rows * (1 - 2^-10) in one column of the table (both exact in fp32), eps = 2^-10: var + eps = 1
        part = np.zeros((2, C, 4), np.float32)
        part[1, :, 0] = rows * (1.0 - 2.0 ** -10)
        assert float(part[1, 0, 0]) == rows * 1023 / 1024
        pd, mo, ro = f32(part), nans((C,), "fp32"), nans((C,), "fp32")
        yf = twice(lambda: nans((rows, C), dtype),
                   lambda t: call("stp_bn_finalize_apply", ops.ptr(pd), 4, ops.ptr(xd), ops.ptr(t), ops.dt(xd), rows, C, 2.0 ** -10, 0.9, ops.ptr(mo),
                                  ops.ptr(ro), None, None, ops.ptr(g), ops.ptr(b), 2, ops.stream()))
        assert np.array_equal(host(mo), np.zeros(C, np.float32)) and np.array_equal(host(ro), np.ones(C, np.float32))
        assert exact(host(yf), want), "stp_bn_finalize_apply"


def prep_weights(ops, w_hwio, dtype):
    """HWIO numpy -> forward copy of the weights in the layout stp_conv2d reads (as test_ops_gpu.py's helper)."""
    kh, kw, ci, co = w_hwio.shape
    vec = 8 if dtype != "fp32" else 4
    cout_b = (co + vec - 1) // vec * vec
    master = keep(torch.from_numpy(np.ascontiguousarray(w_hwio.transpose(3, 0, 1, 2), dtype=np.float32)).to(DEV))
    fwd = keep(torch.empty((co + 15) // 16 * 16 * kh * kw * ci, dtype=TD[dtype], device=DEV))
    bwd = keep(torch.empty((ci + 15) // 16 * 16 * kh * kw * cout_b, dtype=TD[dtype], device=DEV))
    ops.weight_prepare(master, fwd, bwd, co, kh, kw, ci, kw, ci, cout_b, ops.dt(fwd))
    return fwd


def masked_gradient_from_conv_epilogue(ops, dtype, shape, x, dy, m, r, g, b):
    """The producer of stp_bn_backward_fused's operands: a 3x3 convolution whose epilogue (stp_conv_params.bnb_x, bnb_relu = 2) masks
    its output dY with the ReLU6 mask re-derived from x and reduces the per-tile sums.  Its weights are 1 at the centre tap where
    input channel == output channel % 64 and 0 elsewhere, so dY[..., c] = src[..., c % 64] EXACTLY (one non-zero product per sum):
    ``dy`` [rows][C] is that tensor.  -> (stored masked gradient [rows][C], partial sums, tiles)."""
    n, h, w = shape
    C = dy.shape[1]
    assert n * h * w == dy.shape[0] and (C <= 64 or C % 64 == 0)
    src = np.zeros((dy.shape[0], 64), np.float32)
    src[:, :min(C, 64)] = dy[:, :min(C, 64)]
    assert np.array_equal(src[:, np.arange(C) % 64], dy)
    wt = np.zeros((3, 3, 64, C), np.float32)
    wt[1, 1, np.arange(C) % 64, np.arange(C)] = 1.0
    sd, fwd, xd = dev(src, dtype), prep_weights(ops, wt, dtype), dev(x, dtype)
    gbuf = nans((dy.shape[0], C), dtype)
    P = ops.conv_params(sd, fwd, gbuf, N=n, Hs0=h, Ws0=w, Hv=h, Wv=w, C0=64, KH=3, KW=3, stride=1, pad=1, Ho=h, Wo=w, Cout=C, dtype=ops.dt(gbuf))
    P.bnb_x, P.bnb_mean, P.bnb_rstd, P.bnb_gamma, P.bnb_beta, P.bnb_relu = ops.ptr(xd), ops.ptr(m), ops.ptr(r), ops.ptr(g), ops.ptr(b), 2
    floats = ops.conv2d_stats_floats(P)
    st = keep(torch.full((max(4, floats),), float("nan"), dtype=torch.float32, device=DEV))
    P.stats_partial = ops.ptr(st)
    ops.conv2d(P)
    tiles = floats // (2 * C)
    assert tiles == P.stats_tiles and tiles >= 1
    return xd, gbuf, st, tiles


def bn_backward_bounds(b, rows, dtype, amb_b=0.0, amb_g=0.0, scale=1.0):
    """n_terms: a channel sum is an fp32 sum of ``rows`` products in some order (+ 8 for xhat, the products and the final combination);
    dx = scale * (g - dbeta / M - xhat * dgamma / M) inherits the error of both sums through its abs_terms.  ``amb_*``: what the
    elements within the margin of a kink may add to a channel sum if the kernel's fp32 pre-activation falls on the other side."""
    n = rows + 8
    return dict(dbeta=R.rounding_bound(b["dbeta"], b["abs_dbeta"], n, "fp32") + amb_b,
                dgamma=R.rounding_bound(b["dgamma"], b["abs_dgamma"], n, "fp32") + amb_g,
                dx=R.rounding_bound(b["dx"], b["abs_dx"], n, dtype) + np.abs(scale) * (amb_b / rows + np.abs(b["xhat"]) * (amb_g / rows)))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", R.RELU6_CHANNELS)
def test_batchnorm_relu6_backward_masks_exactly_at_both_kinks_on_the_grid(ops, dtype, C):
    """stp_bn_backward(relu = 2) and the conv epilogue + stp_bn_backward_fused with unit parameters on the grid: the gradient passes
    strictly inside (0, 6).  A gradient that is non-zero ONLY where x <= 0 or x >= 6 must give dx, dgamma and dbeta of exactly zero;
    a random gradient must give the float64 reference (mask 0 < x < 6) within the rounding bound; the masked gradient the epilogue
    stores is dY where 0 < x < 6 and exactly 0 elsewhere."""
    rows = R.RELU6_ROWS
    x = R.relu6_grid_input(C)
    on = R.bn_act_on(x, 2)
    assert np.array_equal(on, (x > 0) & (x < 6)) and 0.25 < on.mean() < 0.35
    rng = np.random.RandomState(70 + C)
    dy = q(rng.randn(rows, C), dtype)
    dy[dy == 0] = 1.0
    m, r, g, b = unit_parameters(C)
    xd = dev(x, dtype)
    ws = keep(torch.empty(ops.bn_workspace_bytes(C) // 4, dtype=torch.float32, device=DEV))
    # 1. nothing may pass outside (0, 6)
    off = dev(np.where(on, 0.0, dy), dtype)
    dx, dg, db = nans((rows, C), dtype), nans((C,), "fp32"), nans((C,), "fp32")
    ops.bn_backward(xd, off, dx, rows, C, m, r, g, b, dg, db, relu=2, accumulate_dx=0, workspace=ws)
    assert exact(host(dx), np.zeros((rows, C))) and exact(host(dg), np.zeros(C)) and exact(host(db), np.zeros(C))
    # 2. a random gradient
    ref = R.bn_backward(x, dy * on, 0.0, 1.0, 1.0)
    bound = bn_backward_bounds(ref, rows, dtype)
    dyd = dev(dy, dtype)
    dx = twice(lambda: nans((rows, C), dtype), lambda t: ops.bn_backward(xd, dyd, t, rows, C, m, r, g, b, dg, db, relu=2, accumulate_dx=0, workspace=ws))
    within(host(dx), ref["dx"], bound["dx"], "stp_bn_backward dx")
    within(host(dg), ref["dgamma"], bound["dgamma"], "stp_bn_backward dgamma")
    within(host(db), ref["dbeta"], bound["dbeta"], "stp_bn_backward dbeta")
    # 3. the fused form: mask and sums in the producing convolution's epilogue
    _, gbuf, st, tiles = masked_gradient_from_conv_epilogue(ops, dtype, (1, 9, 37), x, dy, m, r, g, b)
    stored = host(gbuf)
    assert exact(stored, dy * on), "masked gradient of the epilogue"
    assert not stored[~on].any()
    dx, dg, db = nans((rows, C), dtype), nans((C,), "fp32"), nans((C,), "fp32")
    ops.bn_backward_fused(xd, gbuf, dx, rows, C, m, r, g, st, tiles, dg, db, accumulate_dx=0, workspace=ws)
    within(host(dx), ref["dx"], bound["dx"], "stp_bn_backward_fused dx")
    within(host(dg), ref["dgamma"], bound["dgamma"], "stp_bn_backward_fused dgamma")
    within(host(db), ref["dbeta"], bound["dbeta"], "stp_bn_backward_fused dbeta")


@pytest.mark.parametrize("dtype", DTYPES)
def test_batchnorm_relu6_with_general_parameters_within_the_rounding_bound(ops, dtype):
    """Random gamma, beta, mean and rstd on [4096][64]: stp_bn_apply(relu = 2) against clip(pre, 0, 6) and stp_bn_backward(relu = 2) /
    the epilogue + stp_bn_backward_fused against the float64 backward, element by element where the pre-activation is farther than
    1e-3 from 0 and from 6 (less than 1e-3 of the elements are not; a mask that flips there is accounted for in the bound of the sums).
    n_terms of the forward: scale = rstd * gamma, shift = beta - mean * scale and one fma - 3."""
    G = R.BN_GENERAL
    rows, C = G["rows"], G["C"]
    d = R.bn_general_inputs(dtype)
    safe = d["safe"]
    assert 1.0 - safe.mean() < G["share"]
    xd = dev(d["x"], dtype)
    m, r, g, b = f32(d["mean"]), f32(d["rstd"]), f32(d["gamma"]), f32(d["beta"])
    want = R.bn_act(d["pre"], 2)
    a = np.abs(d["x"] * d["scale"]) + np.abs(d["beta"].astype(np.float64)) + np.abs(d["mean"] * d["scale"])
    y = twice(lambda: nans((rows, C), dtype), lambda t: ops.bn_apply(xd, t, rows, C, C, m, r, g, b, relu=2))
    got = host(y)
    assert not np.isnan(got).any() and got.min() >= 0 and got.max() <= 6
    within(got[safe], want[safe], R.rounding_bound(want, a, 3, dtype)[safe], "stp_bn_apply")
    on = R.bn_act_on(d["pre"], 2)
    xh = (d["x"].astype(np.float64) - d["mean"]) * d["rstd"]
    amb_b, amb_g = (np.abs(d["dy"]) * ~safe).sum(0), (np.abs(d["dy"] * xh) * ~safe).sum(0)
    ws = keep(torch.empty(ops.bn_workspace_bytes(C) // 4, dtype=torch.float32, device=DEV))
    dyd = dev(d["dy"], dtype)
    for acc in (0, 1):
        ref = R.bn_backward(d["x"], d["dy"] * on, d["mean"], d["rstd"], d["scale"], d["base"] if acc else None)
        bound = bn_backward_bounds(ref, rows, dtype, amb_b, amb_g, d["scale"])
        dg, db = nans((C,), "fp32"), nans((C,), "fp32")
        dx = twice(lambda: dev(d["base"], dtype) if acc else nans((rows, C), dtype),
                   lambda t: ops.bn_backward(xd, dyd, t, rows, C, m, r, g, b, dg, db, relu=2, accumulate_dx=acc, workspace=ws))
        within(host(dx)[safe], ref["dx"][safe], bound["dx"][safe], "stp_bn_backward dx, accumulate = %d" % acc)
        within(host(dg), ref["dgamma"], bound["dgamma"], "stp_bn_backward dgamma")
        within(host(db), ref["dbeta"], bound["dbeta"], "stp_bn_backward dbeta")
    _, gbuf, st, tiles = masked_gradient_from_conv_epilogue(ops, dtype, (4, 32, 32), d["x"], d["dy"], m, r, g, b)
    stored = host(gbuf)
    assert not np.isnan(stored).any() and np.array_equal(stored[safe], (d["dy"] * on)[safe])
    for acc in (0, 1):
        ref = R.bn_backward(d["x"], d["dy"] * on, d["mean"], d["rstd"], d["scale"], d["base"] if acc else None)
        bound = bn_backward_bounds(ref, rows, dtype, amb_b, amb_g, d["scale"])
        dg, db = nans((C,), "fp32"), nans((C,), "fp32")
        dx = dev(d["base"], dtype) if acc else nans((rows, C), dtype)
        ops.bn_backward_fused(xd, gbuf, dx, rows, C, m, r, g, st, tiles, dg, db, accumulate_dx=acc, workspace=ws)
        within(host(dx)[safe], ref["dx"][safe], bound["dx"][safe], "stp_bn_backward_fused dx, accumulate = %d" % acc)
        within(host(dg), ref["dgamma"], bound["dgamma"], "stp_bn_backward_fused dgamma")
        within(host(db), ref["dbeta"], bound["dbeta"], "stp_bn_backward_fused dbeta")
