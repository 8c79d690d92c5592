"""Float64 numpy restatement of the operators of csrc/deeplab.hip and of the ReLU6 BatchNormalization (shared by
tests/test_deeplab_reference_host.py and tests/test_deeplab_ops_gpu.py; not collected, calls no kernel, no torch convolution, no autograd).

Every function is written from the index formula of include/stp_hip.h.  Those that feed a rounded comparison also return the float64
sum of the ABSOLUTE products that make up each output element (``abs_terms``): ``rounding_bound`` turns it into the per-element
bound of a correct fp32 evaluation, so no tolerance is scaled by the largest element of a tensor and none is taken from a kernel's
output.  The case tables of both test files live here, so that the host test checks the exactness condition on exactly the inputs
the GPU test runs.
"""
import numpy as np
import torch

from oracle import deeplab as odeeplab

TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTYPES = ["fp32", "bf16", "fp16"]
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "fp32": 2.0 ** -23}     # one storage rounding, relative
CAP_DL = 16384 * 256                                                 # dl_grid (deeplab.hip): items one trip of the capped grid covers


def through(a, dtype):
    """float32 values of ``a`` after one round-to-nearest-even into the storage dtype."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(TD[dtype]).to(torch.float32).numpy()


def representable(a, dtype):
    """True when a round trip through the torch dtype returns the same numbers (``a`` itself must fit float32)."""
    a = np.asarray(a, dtype=np.float64)
    a32 = a.astype(np.float32)
    return bool(np.array_equal(a32.astype(np.float64), a) and np.array_equal(through(a32, dtype), a32))


HALF_SUBNORMAL_SPACING = {"bf16": 2.0 ** -134, "fp16": 2.0 ** -25, "fp32": 2.0 ** -150}


def rounding_bound(ref, abs_terms, n_terms, dtype):
    """u(dtype) * |ref| + (n_terms + 2) * 2^-24 * abs_terms: one storage rounding of the result plus a worst-case fp32 evaluation of a
    sum of ``n_terms`` products (each product and each addition rounds once, relative to a partial sum that ``abs_terms`` bounds).
    Below the format's normal range a rounding is no longer relative: there the storage term is half the spacing of the subnormals
    (2^-25 for IEEE half, whose normal range ends at 6.1e-5 - results of that size are ordinary in a gradient; the kernels keep
    subnormals and round them to nearest)."""
    storage = np.maximum(U[dtype] * np.abs(ref), HALF_SUBNORMAL_SPACING[dtype])
    return storage + (n_terms + 2) * 2.0 ** -24 * np.asarray(abs_terms, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# depthwise convolution:  y[n,ho,wo,c] = sum_{kh,kw} x[n, ho*s - pt + kh*d, wo*s - pl + kw*d, c] * w[kh][kw][c]   (taps outside x are 0)

def same_geometry(H, W, k, stride, dil):
    """TF 'same': Ho = ceil(H / s); total = max((Ho-1)*s + keff - H, 0); pad_t = total // 2, the bottom / right takes the rest."""
    keff = (k - 1) * dil + 1
    Ho, Wo = -(-H // stride), -(-W // stride)
    return Ho, Wo, max((Ho - 1) * stride + keff - H, 0) // 2, max((Wo - 1) * stride + keff - W, 0) // 2


def _axis(n_out, n_in, stride, pad, off):
    o = np.arange(n_out)
    i = o * stride - pad + off
    ok = (i >= 0) & (i < n_in)
    return o[ok], i[ok]


def _taps(x_shape, k, stride, pad_t, pad_l, dil, Ho, Wo):
    """(kh, kw, index into the output block, index into the input block) of every tap with at least one pixel inside."""
    _, H, W, _ = x_shape
    for kh in range(k):
        ho, h = _axis(Ho, H, stride, pad_t, kh * dil)
        for kw in range(k):
            wo, w = _axis(Wo, W, stride, pad_l, kw * dil)
            if len(ho) and len(wo):
                yield kh, kw, np.ix_(range(x_shape[0]), ho, wo), np.ix_(range(x_shape[0]), h, w)


def dwconv(x, w, stride, pad_t, pad_l, dil, Ho, Wo):
    """-> (y, abs_terms), float64 [N,Ho,Wo,C]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    y = np.zeros((x.shape[0], Ho, Wo, x.shape[3]))
    a = np.zeros_like(y)
    for kh, kw, o, i in _taps(x.shape, w.shape[0], stride, pad_t, pad_l, dil, Ho, Wo):
        y[o] += x[i] * w[kh, kw]
        a[o] += np.abs(x[i] * w[kh, kw])
    return y, a


def dwconv_dgrad(dy, w, x_shape, stride, pad_t, pad_l, dil, base=None):
    """dx[n,h,w,c] = (base +) sum over the (tap, output pixel) pairs whose input pixel is (h,w) of dy * w  -> (dx, abs_terms)."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    dx = np.zeros(x_shape) if base is None else np.array(base, dtype=np.float64)
    a = np.abs(dx)
    for kh, kw, o, i in _taps(x_shape, w.shape[0], stride, pad_t, pad_l, dil, dy.shape[1], dy.shape[2]):
        dx[i] += dy[o] * w[kh, kw]                       # (within one tap every input pixel is met at most once)
        a[i] += np.abs(dy[o] * w[kh, kw])
    return dx, a


def dwconv_wgrad(x, dy, k, stride, pad_t, pad_l, dil, base=None):
    """dw[kh][kw][c] = (base +) sum_{n,ho,wo} dy[n,ho,wo,c] * x[n, ho*s - pt + kh*d, wo*s - pl + kw*d, c]  -> (dw, abs_terms)."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    dw = np.zeros((k, k, x.shape[3])) if base is None else np.array(base, dtype=np.float64)
    a = np.abs(dw)
    for kh, kw, o, i in _taps(x.shape, k, stride, pad_t, pad_l, dil, dy.shape[1], dy.shape[2]):
        p = dy[o] * x[i]
        dw[kh, kw] += p.sum((0, 1, 2))
        a[kh, kw] += np.abs(p).sum((0, 1, 2))
    return dw, a


# ---------------------------------------------------------------------------------------------------------------------------------
# align-corners bilinear resize

def resize_ac_coords(H, Ho):
    """Source rows and fraction of every output row, evaluated in float32 as the kernels do: s = float32(H-1) / float32(Ho-1)
    (0 when Ho == 1), src = float32(yo) * s, y0 = floor(src), y1 = min(y0 + 1, H - 1), f = src - y0 (exact)."""
    s = np.float32(H - 1) / np.float32(Ho - 1) if Ho > 1 else np.float32(0)
    src = (np.arange(Ho, dtype=np.float32) * s).astype(np.float32)
    y0 = np.floor(src).astype(np.int64)
    y1 = np.minimum(y0 + 1, H - 1)
    return y0, y1, (src - y0.astype(np.float32)).astype(np.float64)


def resize_ac_matrices(H, Ho, lerp_abs=False):
    """[Ho, H] interpolation matrix with float64 weights: row yo holds 1 - f at y0 and f at y1 (summed where y0 == y1).
    ``lerp_abs``: the absolute coefficients of the form the forward kernel evaluates, v0 + (v1 - v0) * f: 1 + f at y0, f at y1."""
    y0, y1, f = resize_ac_coords(H, Ho)
    R = np.zeros((Ho, H))
    o = np.arange(Ho)
    np.add.at(R, (o, y0), 1.0 + f if lerp_abs else 1.0 - f)
    np.add.at(R, (o, y1), f)
    return R


def resize_ac(x, Ho, Wo):
    """Ry . x . Rx^T per image and channel -> (y, abs_terms of the lerp form)."""
    x = np.asarray(x, np.float64)
    _, H, W, _ = x.shape
    y = np.einsum("ph,nhwc,qw->npqc", resize_ac_matrices(H, Ho), x, resize_ac_matrices(W, Wo), optimize=True)
    a = np.einsum("ph,nhwc,qw->npqc", resize_ac_matrices(H, Ho, True), np.abs(x), resize_ac_matrices(W, Wo, True), optimize=True)
    return y, a


def resize_ac_bwd(dy, H, W, base=None):
    """Ry^T . dy . Rx, the exact adjoint (+ base) -> (dx, abs_terms, largest number of outputs one input pixel gathers)."""
    dy = np.asarray(dy, np.float64)
    Ry, Rx = resize_ac_matrices(H, dy.shape[1]), resize_ac_matrices(W, dy.shape[2])
    dx = np.einsum("ph,npqc,qw->nhwc", Ry, dy, Rx, optimize=True)
    a = np.einsum("ph,npqc,qw->nhwc", Ry, np.abs(dy), Rx, optimize=True)
    if base is not None:
        dx, a = dx + np.asarray(base, np.float64), a + np.abs(base)
    return dx, a, int((Ry != 0).sum(0).max() * (Rx != 0).sum(0).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# dropout, sigmoid

def dropout(x, step, salt, rate, dtype):
    """mask(step, salt, index) * float32(x) * (float32(1) / (float32(1) - float32(rate))), rounded once to the storage dtype."""
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    keep = odeeplab.dropout_mask(step, salt, x.size, rate)
    scale = np.float32(1) / (np.float32(1) - np.float32(rate))
    return through(np.where(keep, (x * scale).astype(np.float32), np.float32(0)), dtype)


def sigmoid_act(z, channels):
    """z [rows][ldz] -> p [rows][channels], float64."""
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)[:, :channels]))


def sigmoid_act_bwd(p, dp, channels):
    """dz [rows][ldg] = dp * p * (1 - p) in the first ``channels`` columns, 0 behind them  -> (dz, abs_terms)."""
    p, dp = np.asarray(p, np.float64), np.asarray(dp, np.float64)
    dz = np.zeros_like(dp)
    dz[:, :channels] = dp[:, :channels] * p[:, :channels] * (1.0 - p[:, :channels])
    return dz, np.abs(dz)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNormalization with its activation (relu: 0 none, 1 ReLU, 2 ReLU6)

def bn_act(v, relu):
    v = np.asarray(v, np.float64)
    return v if relu == 0 else np.clip(v, 0.0, 6.0 if relu == 2 else np.inf)


def bn_act_on(v, relu):
    """Where the gradient passes: strictly inside the linear range (0 < v, and v < 6 for ReLU6)."""
    v = np.asarray(v, np.float64)
    return np.ones(v.shape, bool) if relu == 0 else (v > 0) & ((v < 6) if relu == 2 else True)


def bn_pre(x, mean, rstd, gamma, beta):
    """x * scale + shift with scale = float32(rstd * gamma), shift = float32(beta - mean * scale), as the kernels derive them."""
    sc = (np.asarray(rstd, np.float32) * np.asarray(gamma, np.float32)).astype(np.float32)
    sh = (np.asarray(beta, np.float32) - np.asarray(mean, np.float32) * sc).astype(np.float32)
    return np.asarray(x, np.float64) * sc.astype(np.float64) + sh.astype(np.float64), sc.astype(np.float64)


def bn_backward(x, g, mean, rstd, scale, base=None):
    """g = the gradient already under the activation mask, [rows][C].  dbeta = sum g, dgamma = sum g * xhat,
    dx = scale * (g - dbeta / M - xhat * dgamma / M) (+ base)  -> dict of values and of their abs_terms."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    M = x.shape[0]
    xh = (x - np.asarray(mean, np.float64)) * np.asarray(rstd, np.float64)
    db, dg = g.sum(0), (g * xh).sum(0)
    adb, adg = np.abs(g).sum(0), np.abs(g * xh).sum(0)
    sc = np.asarray(scale, np.float64)
    dx = sc * (g - db / M - xh * (dg / M))
    adx = np.abs(sc) * (np.abs(g) + adb / M + np.abs(xh) * (adg / M))
    if base is not None:
        dx, adx = dx + np.asarray(base, np.float64), adx + np.abs(base)
    return dict(dx=dx, dgamma=dg, dbeta=db, abs_dx=adx, abs_dgamma=adg, abs_dbeta=adb, xhat=xh)


# ---------------------------------------------------------------------------------------------------------------------------------
# case tables (the GPU test runs them; the host test checks the exactness condition on the same inputs)

# (N, H, W, C, stride, dilation), k = 3, TF 'same'
DW_EXACT_CASES = [
    (1, 5, 6, 4, 1, 1),            # the minimum
    (3, 50, 40, 72, 1, 1),         # 150 output rows > 128 workgroups of the weight gradient; two channel slabs, the second 8 of 64 lanes
    (3, 50, 40, 72, 2, 1),         # 'same' with pad_t = 0
    (3, 51, 41, 72, 2, 1),         # 'same' with pad_t = 1
    (2, 20, 24, 32, 1, 2), (2, 20, 24, 32, 1, 4),
    (2, 9, 9, 64, 1, 6), (2, 9, 9, 64, 1, 18),     # ASPP on a 9 x 9 map; at rate 18 only the centre tap is inside
    (2, 9, 9, 728, 1, 1),          # Xception's middle flow: twelve slabs, the last with 24 channels
]
DW_ROUNDED_CASES = [(3, 50, 40, 72, 1, 1), (2, 20, 24, 32, 2, 2)]

# (N, H, W, C, Ho, Wo, which): "both" runs forward and gradient, "fwd" / "bwd" only one of them (the large tensors)
RESIZE_EXACT_CASES = [
    (2, 5, 9, 5, 17, 33, "both"),
    (2, 1, 1, 5, 6, 9, "both"),            # scale 0: every output gathers the one input pixel
    (2, 9, 5, 5, 9, 5, "both"),            # identity
    (2, 33, 33, 128, 129, 129, "fwd"),     # 4 260 096 outputs: above the 4 194 304-item grid
    (2, 65, 65, 512, 129, 129, "bwd"),     # 4 326 400 inputs: above it
]
RESIZE_ROUNDED_CASES = [(2, 7, 12, 5, 40, 29), (2, 7, 12, 24, 40, 29), (2, 12, 40, 5, 5, 7), (2, 12, 40, 24, 5, 7)]

RELU6_GRID = np.array([-1.0, -0.0, 0.0, 2.0 ** -7, 0.5, 5.96875, 6.0, 6.03125, 7.0, 100.0], np.float32)
RELU6_ROWS = 333
RELU6_CHANNELS = [20, 24, 64]      # the scalar-table, the 4-wide and the 8-wide path of stp_bn_apply
BN_GENERAL = dict(rows=4096, C=64, seed=3, margin=1e-3, share=1e-3)


def dw_case_id(c):
    return "%dx%dx%dx%d-s%d-d%d" % c


def resize_case_id(c):
    return "%dx%dx%dx%d-to-%dx%d" % c[:6]


def dw_exact_inputs(case):
    """x in [-3, 3], w in [-2, 2], dy in [-2, 2], accumulate bases in [-3, 3]: all integers."""
    n, h, w, c, stride, dil = case
    ho, wo, pt, pl = same_geometry(h, w, 3, stride, dil)
    rng = np.random.RandomState(1000 + h + 7 * c + 31 * stride + 101 * dil)
    ri = lambda lo, hi, shape: rng.randint(lo, hi + 1, size=shape).astype(np.float32)
    return dict(geom=(n, h, w, c, 3, stride, pt, pl, dil, ho, wo), x=ri(-3, 3, (n, h, w, c)), w=ri(-2, 2, (3, 3, c)),
                dy=ri(-2, 2, (n, ho, wo, c)), base_dx=ri(-3, 3, (n, h, w, c)), base_dw=ri(-3, 3, (3, 3, c)))


def dw_rounded_inputs(case, dtype):
    n, h, w, c, stride, dil = case
    ho, wo, pt, pl = same_geometry(h, w, 3, stride, dil)
    rng = np.random.RandomState(2000 + h + c)
    rn = lambda shape: through(rng.randn(*shape), dtype)
    return dict(geom=(n, h, w, c, 3, stride, pt, pl, dil, ho, wo), x=rn((n, h, w, c)), w=(rng.randn(3, 3, c) / 3).astype(np.float32),
                dy=rn((n, ho, wo, c)), base_dx=rn((n, h, w, c)), base_dw=rng.randn(3, 3, c).astype(np.float32))


def resize_exact_inputs(case):
    """x in [-15, 15], dy in {-1, 0, 1}, base in [-3, 3]: integers, at ratios whose fractions are multiples of 1/4."""
    n, h, w, c, ho, wo, _ = case
    rng = np.random.RandomState(3000 + h + ho + c)
    ri = lambda lo, hi, shape: rng.randint(lo, hi + 1, size=shape).astype(np.float32)
    return dict(x=ri(-15, 15, (n, h, w, c)), dy=ri(-1, 1, (n, ho, wo, c)), base=ri(-3, 3, (n, h, w, c)))


def resize_rounded_inputs(case, dtype):
    n, h, w, c, ho, wo = case
    rng = np.random.RandomState(4000 + h + ho + c)
    rn = lambda shape: through(rng.randn(*shape), dtype)
    return dict(x=rn((n, h, w, c)), dy=rn((n, ho, wo, c)), base=rn((n, h, w, c)))


def relu6_grid_input(C):
    """[RELU6_ROWS][C] cycling through RELU6_GRID (every value is exact in all three storage dtypes)."""
    return RELU6_GRID[np.arange(RELU6_ROWS * C) % len(RELU6_GRID)].reshape(RELU6_ROWS, C).copy()


def bn_general_inputs(dtype):
    """Random BatchNormalization parameters and a [rows][C] input in the storage dtype; ``pre`` is the float64 pre-activation and
    ``safe`` the elements farther than ``margin`` from both kinks of ReLU6."""
    g = BN_GENERAL
    rng = np.random.RandomState(g["seed"])
    x = through(rng.randn(g["rows"], g["C"]) * 1.5 + 0.5, dtype)
    dy = through(rng.randn(g["rows"], g["C"]), dtype)
    base = through(rng.randn(g["rows"], g["C"]), dtype)
    gamma = (rng.rand(g["C"]) + 1.0).astype(np.float32)
    beta = (rng.randn(g["C"]) * 0.5 + 2.0).astype(np.float32)
    mean = (rng.randn(g["C"]) * 0.3 + 0.5).astype(np.float32)
    rstd = (1.0 / (rng.rand(g["C"]) + 1.0)).astype(np.float32)
    pre, scale = bn_pre(x, mean, rstd, gamma, beta)
    safe = (np.abs(pre) > g["margin"]) & (np.abs(pre - 6.0) > g["margin"])
    return dict(x=x, dy=dy, base=base, gamma=gamma, beta=beta, mean=mean, rstd=rstd, pre=pre, scale=scale, safe=safe)
