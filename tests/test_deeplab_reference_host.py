"""CPU checks of tests/_deeplab_reference.py, the float64 reference tests/test_deeplab_ops_gpu.py holds csrc/deeplab.hip and the ReLU6
BatchNormalization to: the restated formulas against float64 torch (grouped convolution, align-corners interpolation and their autograd,
the sigmoid), the dropout against the oracle's mask, and the CONDITION under which the GPU test may ask for bit-equality - every exact
case's reference (and accumulated reference) is representable in all three storage dtypes and every sum stays an exact fp32 integer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _deeplab_reference as R
from oracle import deeplab as odeeplab


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).permute(0, 3, 1, 2).clone()


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("case", [(2, 7, 6, 4, 1, 1), (2, 8, 9, 8, 2, 1), (1, 9, 8, 4, 2, 1), (2, 10, 7, 4, 1, 2), (1, 9, 9, 4, 1, 4), (1, 5, 5, 4, 1, 6),
                                  (2, 11, 10, 4, 2, 2)], ids=R.dw_case_id)
def test_depthwise_reference_equals_torch_grouped_convolution_and_autograd(case):
    n, h, w, c, stride, dil = case
    rng = np.random.RandomState(7)
    ho, wo, pt, pl = R.same_geometry(h, w, 3, stride, dil)
    keff = 2 * dil + 1
    pb, pr = max((ho - 1) * stride + keff - h, 0) - pt, max((wo - 1) * stride + keff - w, 0) - pl
    assert 0 <= pb - pt <= 1 and 0 <= pr - pl <= 1                      # bottom / right takes the rest
    x, wt, dy = rng.randn(n, h, w, c), rng.randn(3, 3, c), rng.randn(n, ho, wo, c)
    xt = nchw(x).requires_grad_(True)
    wtt = torch.from_numpy(wt).permute(2, 0, 1)[:, None].clone().requires_grad_(True)
    ref = F.conv2d(F.pad(xt, (pl, pr, pt, pb)), wtt, stride=stride, dilation=dil, groups=c)
    assert tuple(ref.shape[2:]) == (ho, wo)
    ref.backward(nchw(dy))
    y, ay = R.dwconv(x, wt, stride, pt, pl, dil, ho, wo)
    np.testing.assert_allclose(y, nhwc(ref), atol=1e-12)
    assert (ay >= np.abs(y) - 1e-12).all()
    dx, _ = R.dwconv_dgrad(dy, wt, x.shape, stride, pt, pl, dil)
    np.testing.assert_allclose(dx, nhwc(xt.grad), atol=1e-12)
    dw, _ = R.dwconv_wgrad(x, dy, 3, stride, pt, pl, dil)
    np.testing.assert_allclose(dw, wtt.grad[:, 0].permute(1, 2, 0).numpy(), atol=1e-12)
    base = rng.randn(n, h, w, c)
    np.testing.assert_allclose(R.dwconv_dgrad(dy, wt, x.shape, stride, pt, pl, dil, base)[0], dx + base, atol=1e-12)
    np.testing.assert_allclose(R.dwconv_wgrad(x, dy, 3, stride, pt, pl, dil, wt)[0], dw + wt, atol=1e-12)


@pytest.mark.parametrize("sizes", [((5, 9), (17, 33)), ((1, 1), (6, 9)), ((9, 5), (9, 5)), ((3, 5), (5, 9)), ((9, 17), (5, 9)), ((7, 12), (40, 29)),
                                   ((12, 40), (5, 7)), ((4, 6), (1, 1))])
def test_resize_reference_equals_torch_align_corners_interpolation_and_autograd(sizes):
    """At ratios whose float32 coordinates are exact (dyadic scales, the identity, scale 0) to 1e-12; elsewhere the float32 coordinate
    differs from torch's float64 one by ~1e-7 of a pixel: 1e-6 of max|x|."""
    (h, w), (ho, wo) = sizes
    rng = np.random.RandomState(8)
    x, dy = rng.randn(2, h, w, 3), rng.randn(2, ho, wo, 3)
    xt = nchw(x).requires_grad_(True)
    ref = F.interpolate(xt, size=(ho, wo), mode="bilinear", align_corners=True)
    ref.backward(nchw(dy))
    exact = all(o == 1 or ((i - 1) * 64) % (o - 1) == 0 for i, o in ((h, ho), (w, wo)))      # scale a multiple of 1/64
    y, ay = R.resize_ac(x, ho, wo)
    np.testing.assert_allclose(y, nhwc(ref), atol=1e-12 if exact else 1e-6 * np.abs(x).max())
    assert (ay >= np.abs(y) - 1e-12).all()
    dx, adx, terms = R.resize_ac_bwd(dy, h, w)
    np.testing.assert_allclose(dx, nhwc(xt.grad), atol=1e-12 if exact else 1e-6 * np.abs(dy).max() * terms)
    for n_in, n_out in ((h, ho), (w, wo)):
        M = R.resize_ac_matrices(n_in, n_out)
        np.testing.assert_allclose(M.sum(1), 1.0, atol=1e-15)
        assert (M >= 0).all() and ((M != 0).sum(1) <= 2).all()
    base = rng.randn(2, h, w, 3)
    np.testing.assert_allclose(R.resize_ac_bwd(dy, h, w, base)[0], dx + base, atol=1e-12)


def test_sigmoid_reference_equals_torch():
    rng = np.random.RandomState(9)
    z = np.concatenate([rng.randn(50, 8) * 3, np.array([[0.0, -0.0, 17, -17, 88, -88, 104, -104]])])
    zt = torch.from_numpy(z[:, :3].copy()).requires_grad_(True)
    p = torch.sigmoid(zt)
    dp = rng.randn(51, 8)
    p.backward(torch.from_numpy(dp[:, :3].copy()))
    with np.errstate(over="ignore"):
        got = R.sigmoid_act(z, 3)
    np.testing.assert_allclose(got, p.detach().numpy(), atol=1e-12)
    dz, _ = R.sigmoid_act_bwd(got, dp, 3)
    np.testing.assert_allclose(dz[:, :3], zt.grad.numpy(), atol=1e-12)
    assert not dz[:, 3:].any()


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_dropout_reference_uses_the_oracles_mask_on_a_full_tensor(dtype):
    rng = np.random.RandomState(10)
    x = R.through(rng.randn(2, 9, 7, 5) + 3.0, dtype)         # (no zeros: a dropped element is the only zero)
    x[x == 0] = 1.0
    for step, salt, rate in ((0, 7, 0.25), (1, 7, 0.25), (3, odeeplab.DROPOUT_SALT, 0.1)):
        y = R.dropout(x, step, salt, rate, dtype).reshape(x.shape)
        keep = odeeplab.dropout_mask(step, salt, x.size, rate).reshape(x.shape)
        assert np.array_equal(y != 0, keep)
        want = x[keep].astype(np.float64) / (1.0 - rate)
        np.testing.assert_allclose(y[keep], want, rtol=R.U[dtype] + 2.0 ** -22)
        assert R.representable(y, dtype)
    assert np.array_equal(R.dropout(x, 5, 1, 0.0, dtype).reshape(x.shape), x)


def test_bn_reference_equals_torch_autograd_through_relu6():
    rng = np.random.RandomState(11)
    rows, C = 40, 6
    x, dy = rng.randn(rows, C) * 3 + 2, rng.randn(rows, C)
    gamma, beta = rng.rand(C) + 2.5, rng.randn(C) + 3
    xt = torch.from_numpy(x).requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    mean, var = xt.mean(0), xt.var(0, unbiased=False)
    pre = (xt - mean) * torch.rsqrt(var + 1e-3) * gt + bt
    torch.clamp(pre, 0.0, 6.0).backward(torch.from_numpy(dy))
    m, r = mean.detach().numpy(), torch.rsqrt(var + 1e-3).detach().numpy()
    on = R.bn_act_on(pre.detach().numpy(), 2)
    assert 0 < on.sum() < on.size and (pre.detach().numpy() > 6).any()
    b = R.bn_backward(x, dy * on, m, r, r * gamma)
    np.testing.assert_allclose(b["dx"], xt.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(b["dgamma"], gt.grad.numpy(), atol=1e-12)
    np.testing.assert_allclose(b["dbeta"], bt.grad.numpy(), atol=1e-12)
    assert np.array_equal(R.bn_act(R.RELU6_GRID, 2), np.array([0, 0, 0, 2.0 ** -7, 0.5, 5.96875, 6, 6, 6, 6]))
    assert np.array_equal(R.bn_act_on(R.RELU6_GRID, 2), np.array([0, 0, 0, 1, 1, 1, 0, 0, 0, 0], bool))


def test_helpers_representable_and_rounding_bound():
    assert R.representable(np.array([0.5, -54.0, 255.0, 2.0 ** -7]), "bf16") and not R.representable(np.array([257.0]), "bf16")
    assert R.representable(np.array([2049.0 / 2048]), "fp16") is False and R.representable(np.array([1025.0 / 1024]), "fp16")
    assert not R.representable(np.array([1.0 + 2.0 ** -30]), "fp32")
    b = R.rounding_bound(np.array([2.0]), np.array([8.0]), 9, "bf16")
    assert b[0] == 2.0 ** -8 * 2.0 + 11 * 2.0 ** -24 * 8.0
    # a correct round-to-nearest into IEEE half stays inside the bound below the normal range as well, where u * |ref| alone would not hold
    v = np.array([3.1e-8, 1.0e-6, 5.0e-5, 7.0e-5])
    assert (np.abs(R.through(v, "fp16") - v) <= R.rounding_bound(v, 0 * v, 0, "fp16")).all()
    assert (np.abs(R.through(v, "fp16") - v) > 2.0 ** -11 * v)[:2].all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the condition of the exact GPU cases (a condition on the inputs, not a measurement of a kernel)

@pytest.mark.parametrize("case", R.DW_EXACT_CASES, ids=R.dw_case_id)
def test_exact_depthwise_cases_are_representable_in_every_dtype(case):
    d = R.dw_exact_inputs(case)
    n, h, w, c, k, stride, pt, pl, dil, ho, wo = d["geom"]
    y, ay = R.dwconv(d["x"], d["w"], stride, pt, pl, dil, ho, wo)
    dx0, _ = R.dwconv_dgrad(d["dy"], d["w"], d["x"].shape, stride, pt, pl, dil)
    dx1, adx = R.dwconv_dgrad(d["dy"], d["w"], d["x"].shape, stride, pt, pl, dil, d["base_dx"])
    dw0, _ = R.dwconv_wgrad(d["x"], d["dy"], k, stride, pt, pl, dil)
    dw1, adw = R.dwconv_wgrad(d["x"], d["dy"], k, stride, pt, pl, dil, d["base_dw"])
    for dtype in R.DTYPES:
        for a in (d["x"], d["dy"], d["base_dx"], y, dx0, dx1):
            assert R.representable(a, dtype)
    assert np.abs(y).max() <= 54 and np.abs(dx1).max() <= 54            # every partial sum is an integer below 2^8
    assert ay.max() <= 54 and adx.max() <= 54
    assert adw.max() < 2 ** 24                                           # every partial sum of the weight gradient is an exact fp32 integer
    assert R.representable(dw0, "fp32") and R.representable(dw1, "fp32")
    if case == (2, 9, 9, 64, 1, 18):                                     # only the centre tap lands inside the map
        assert np.array_equal(y, d["x"].astype(np.float64) * d["w"][1, 1])


@pytest.mark.parametrize("case", R.RESIZE_EXACT_CASES, ids=R.resize_case_id)
def test_exact_resize_cases_are_representable_in_every_dtype(case):
    n, h, w, c, ho, wo, which = case
    d = R.resize_exact_inputs(case)
    for n_in, n_out in ((h, ho), (w, wo)):
        _, _, f = R.resize_ac_coords(n_in, n_out)
        assert np.array_equal(f * 4, np.round(f * 4))                   # fractions are multiples of 1/4: every lerp step is exact
    outs = []
    if which != "bwd":
        outs.append(R.resize_ac(d["x"], ho, wo)[0])
    if which != "fwd":
        outs += [R.resize_ac_bwd(d["dy"], h, w)[0], R.resize_ac_bwd(d["dy"], h, w, d["base"])[0]]
    for dtype in R.DTYPES:
        for a in outs:
            assert R.representable(a, dtype)


def test_relu6_grid_is_exact_in_every_dtype_and_the_general_case_keeps_its_excluded_share():
    for dtype in R.DTYPES:
        assert R.representable(R.RELU6_GRID, dtype)
        g = R.bn_general_inputs(dtype)
        assert 0 < 1.0 - g["safe"].mean() < R.BN_GENERAL["share"]
        on = R.bn_act_on(g["pre"], 2)
        assert (g["pre"] <= 0).mean() > 0.01 and (g["pre"] >= 6).mean() > 0.01 and on.mean() > 0.5      # all three branches are populated
    for C in R.RELU6_CHANNELS:
        x = R.relu6_grid_input(C)
        assert x.shape == (R.RELU6_ROWS, C) and all((x == v).sum() >= x.size // 10 for v in R.RELU6_GRID[2:])
        assert np.signbit(x).sum() >= 2 * (x.size // 10)                 # -1 and -0.0
