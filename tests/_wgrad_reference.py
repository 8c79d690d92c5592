"""Float64 numpy restatement of the convolution weight gradient (csrc/conv_wgrad*.hip, the small-channel and stem kernels of
conv_sc_wgrad.hip / conv_sc_lean.hip), shared by tests/test_wgrad_reference_host.py and tests/test_wgrad_ops_gpu.py.  Not collected, calls no
kernel, no torch, no autograd: it is written from the index formula of include/stp_hip.h,

    dW[co][(kh * KW + kw) * (C0 + C1) + c] = sum_{n,ho,wo} dY[n,ho,wo,co] * V[n, ho * stride - pad + kh, wo * stride - pad + kw, c]

with V = concat(nearest2x(src0) or src0, src1) and taps outside V equal to zero (the padding of the NORMALISED tensor when src0 runs
through a fused producer BatchNormalization first).

``wgrad`` returns for every element the value, ``abs_terms`` = sum |V * dY| and ``n_terms`` = the number of in-bounds pixel products
of its tap.  ``rounding_bound`` turns the latter two into the per-element bound of ANY order of fp32 additions over the element's own
products; dW is fp32, so the bound has no storage term.  No bound is scaled by the largest element of a tensor and none is read from a
kernel's output.  The case tables of both test files live here, so the host test asserts the exactness condition and the plan facts on
exactly the inputs and shapes the GPU test runs.
"""
import collections
import functools
import zlib

import numpy as np

DTYPES = ["fp32", "bf16", "fp16"]
H16 = ["bf16", "fp16"]
F32, BF16, F16 = 0, 1, 3                     # stp_dtype codes of include/stp_hip.h
DT_CODE = {"fp32": F32, "bf16": BF16, "fp16": F16}
SRC_DIRECT, SRC_NEAREST2X = 0, 1
SC_TH, SC_TW = 8, 32                         # pixel tile of the small-channel kernels (conv_sc.h)
EXACT_LIMIT = 2.0 ** 24                      # integers up to here are exact in fp32, and so is every partial sum below it


def through(a, dtype):
    """float32 values of ``a`` after one round-to-nearest-even into the storage dtype (numpy only)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "fp32":
        return a.copy()
    if dtype == "fp16":
        return a.astype(np.float16).astype(np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000            # (finite inputs only)
    return bits.astype(np.uint32).view(np.float32).reshape(a.shape)


def nearest2x(x):
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def virtual_source(src0, src1=None, up=False):
    """V of include/stp_hip.h: concat(nearest2x(src0) or src0, src1) along the channels."""
    v = nearest2x(np.asarray(src0)) if up else np.asarray(src0)
    return v if src1 is None else np.concatenate([v, np.asarray(src1)], axis=-1)


def bn_act(x, mean, rstd, gamma, beta, relu):
    """The producer BatchNormalization of stp_wgrad_params.src_bn_*, in float64: (x - mean) * rstd * gamma + beta, then none (0) /
    ReLU (1) / ReLU6 (2).  (Exact cases only: mean 0, rstd 1, gamma 1, beta 0, where every step is exact.)"""
    y = (np.asarray(x, np.float64) - mean) * rstd * gamma + beta
    if relu >= 1:
        y = np.maximum(y, 0.0)
    if relu == 2:
        y = np.minimum(y, 6.0)
    return y + 0.0


def wgrad(v, dy, KH, KW, stride, pad, prev=None):
    """-> (dW, abs_terms, n_terms), float64 / float64 / int64, each [Cout][KH][KW][C].  ``v`` [N,Hv,Wv,C] is the virtual (and, where a
    BatchNormalization is fused, already normalised) source: taps outside it contribute nothing.  ``prev`` = the destination's prior
    contents when the launch accumulates (added to the value; ``rounding_bound`` takes it separately)."""
    v, dy = np.asarray(v, np.float64), np.asarray(dy, np.float64)
    N, Hv, Wv, C = v.shape
    _, Ho, Wo, Cout = dy.shape
    dw = np.zeros((Cout, KH, KW, C))
    ab = np.zeros_like(dw)
    nt = np.zeros(dw.shape, dtype=np.int64)
    for kh in range(KH):
        ho = np.arange(Ho)
        hi = ho * stride - pad + kh
        ho, hi = ho[(hi >= 0) & (hi < Hv)], hi[(hi >= 0) & (hi < Hv)]
        for kw in range(KW):
            wo = np.arange(Wo)
            wi = wo * stride - pad + kw
            wo, wi = wo[(wi >= 0) & (wi < Wv)], wi[(wi >= 0) & (wi < Wv)]
            if not (len(ho) and len(wo)):
                continue
            g = dy[:, ho][:, :, wo].reshape(-1, Cout)
            x = v[:, hi][:, :, wi].reshape(-1, C)
            dw[:, kh, kw, :] = g.T @ x
            ab[:, kh, kw, :] = np.abs(g).T @ np.abs(x)
            nt[:, kh, kw, :] = g.shape[0]
    if prev is not None:
        dw = dw + np.asarray(prev, np.float64)
    return dw, ab, nt


def rounding_bound(n_terms, abs_terms, prev=None):
    """(n_terms + 2 [+ 1 with accumulate]) * 2^-24 * (abs_terms [+ |prev|]): each of the element's products rounds at most once, each
    addition rounds once relative to a partial sum that abs_terms (+ |prev|) bounds, in whatever order and over however many slabs
    they are added.  No storage term: dW is fp32."""
    n = np.asarray(n_terms, np.float64) + 2.0
    a = np.asarray(abs_terms, np.float64)
    if prev is not None:
        n, a = n + 1.0, a + np.abs(np.asarray(prev, np.float64))
    return n * 2.0 ** -24 * a


# ---------------------------------------------------------------------------------------------------------------------------------
# cases.  n, h, w are the size of src0 as stored (the LOW resolution when ``up``); the virtual map is twice that then.

Case = collections.namedtuple("Case", "name family n h w c0 c1 up co kh kw s p splits h16 bn stem note")


def _c(name, family, n, h, w, c0, co, k=3, s=1, p=1, splits=0, c1=0, up=False, h16=False, bn=None, stem=False, kw=None, note=""):
    return Case(name, family, n, h, w, c0, c1, up, co, k, kw or k, s, p, splits, h16, bn, stem, note)


GEMM_CASES = [
    _c("p35_16row", "gemm", 1, 5, 7, 8, 8, note="P = 35 < one pixel step; 16-row tile"),
    _c("ragged_64row", "gemm", 3, 7, 5, 24, 40, splits=2, note="ragged K, M, P; 64-row tile"),
    _c("two_m_tiles", "gemm", 2, 9, 11, 8, 136, splits=3, note="second M tile with 8 live rows; 3 splits asked, 2 planned"),
    _c("32row", "gemm", 1, 24, 20, 16, 32, note="32-row tile (variants 1-3; the automatic choice is the small-channel kernel)"),
    _c("rowu_one_row", "gemm", 1, 2, 128, 64, 64, note="uniform rows, one image row per step"),
    _c("rowu_whole_rows", "gemm", 2, 16, 32, 64, 64, s=2, note="uniform rows, whole rows per step (Wo = 16)"),
    _c("s2_one_slab", "gemm", 2, 12, 12, 128, 256, s=2, splits=1, note="stride 2, one slab"),
    _c("k1_s2", "gemm", 2, 16, 16, 64, 128, k=1, s=2, p=0, note="1x1 stride 2"),
    _c("stem_odd", "gemm", 2, 33, 35, 4, 64, k=7, kw=8, s=2, p=3, stem=True, note="stem, odd width: C4 GEMM in H16, plain GEMM in fp32"),
    _c("sc_forced_gemm", "gemm", 1, 20, 24, 32, 16, splits=5, note="GEMM forced on a small-channel shape"),
]

SC_CASES = [
    _c("one_ragged_tile", "sc", 1, 5, 7, 16, 8),
    _c("ragged_16_16", "sc", 2, 19, 45, 16, 16),
    _c("ragged_32_16", "sc", 2, 19, 45, 32, 16),
    _c("ragged_32_32", "sc", 1, 9, 33, 32, 32),
    _c("cin64", "sc", 1, 16, 64, 64, 32, h16=True),
    _c("two_sources", "sc", 2, 6, 7, 32, 16, c1=16, up=True),
    _c("bn_relu", "sc", 1, 5, 7, 16, 8, bn=1, note="fused producer BatchNormalization + ReLU"),
    _c("stem_lean", "sc", 1, 5, 6, 4, 64, k=7, kw=8, s=2, p=3, stem=True, h16=True, note="lean stem kernel: the smallest even width with a ragged tile"),
]
SC_MULTI_TRIP = _c("second_trip", "sc", 2, 258, 500, 16, 16, note="1056 tiles > 1024 workgroups: exact class only")

ROW_CASES = [
    _c("wo16_64row", "row", 2, 4, 16, 64, 40, h16=True),
    _c("wo192_split3", "row", 1, 4, 192, 64, 64, splits=3, h16=True),
    _c("128row_ragged", "row", 1, 16, 64, 256, 72, h16=True),
    _c("two_m_tiles", "row", 3, 16, 16, 192, 200, h16=True),
    _c("two_sources", "row", 2, 4, 16, 64, 32, c1=64, up=True, h16=True, note="variant 4; the automatic choice is the small-channel kernel"),
    _c("two_sources_auto", "row", 2, 4, 16, 64, 40, c1=64, up=True, h16=True, note="40 outputs: the automatic choice is the row kernel"),
    _c("bn_relu6", "row", 2, 4, 16, 64, 40, h16=True, bn=2),
    _c("bn_none_128row", "row", 1, 4, 64, 64, 72, h16=True, bn=0),
]

# (n, h, w, c0, c1 (> 0: src0 is nearest-2x upsampled and concatenated with a c1-channel skip), cout): tests/test_ops_gpu.py WGRAD_GROUPS
GROUPS = {
    "class128": [(2, 32, 32, 128, 0, 128), (1, 16, 64, 256, 0, 72), (3, 16, 16, 192, 0, 200), (2, 8, 8, 128, 64, 136), (1, 4, 192, 64, 0, 128)],
    "class64": [(2, 32, 32, 64, 0, 64), (2, 4, 16, 64, 0, 40), (2, 4, 32, 128, 64, 64)],
    "class32": [(2, 32, 32, 64, 0, 32), (1, 4, 32, 64, 64, 24), (1, 16, 64, 128, 0, 16)],
    "one_layer": [(4, 32, 32, 128, 0, 256)],
}
GROUP_CLASS = {"class128": 128, "class64": 64, "class32": 32, "one_layer": 128}
# n, h, w, ci, co, k, stride, pad: the lone layers of test_batched_reduce_of_lone_weight_gradients
LONE_LAYERS = [(2, 24, 24, 64, 256, 1, 1, 0), (2, 24, 24, 256, 64, 1, 1, 0), (2, 24, 24, 64, 128, 1, 2, 0), (2, 24, 24, 64, 64, 3, 2, 1),
               (1, 12, 12, 512, 128, 1, 1, 0)]


def group_case(group, i, bn=None):
    n, h, w, c0, c1, co = GROUPS[group][i]
    return _c("%s_%d" % (group, i), "group", n, h, w, c0, co, c1=c1, up=c1 > 0, h16=True, bn=bn)


def lone_case(i):
    n, h, w, ci, co, k, s, p = LONE_LAYERS[i]
    return _c("lone_%d" % i, "lone", n, h, w, ci, co, k=k, s=s, p=p)


def dtypes_of(case):
    """The builds a case runs in: the 16-bit ones only where the kernel is, and fp32's small-channel kernel up to 16 input channels."""
    if case.h16:
        return H16
    if case.family == "sc" and max(case.c0, case.c1) > 16:
        return H16
    return DTYPES


def geometry(case):
    """-> dict of the stp_wgrad_params geometry fields."""
    Hv, Wv = (2 * case.h, 2 * case.w) if case.up else (case.h, case.w)
    Ho, Wo = (Hv + 2 * case.p - (7 if case.stem else case.kh)) // case.s + 1, (Wv + 2 * case.p - (7 if case.stem else case.kw)) // case.s + 1
    return dict(N=case.n, Hs0=case.h, Ws0=case.w, Hv=Hv, Wv=Wv, C0=case.c0, C1=case.c1, src0_mode=SRC_NEAREST2X if case.up else SRC_DIRECT,
                KH=case.kh, KW=case.kw, stride=case.s, pad=case.p, Ho=Ho, Wo=Wo, Cout=case.co, splits=case.splits)


def fill_params(P, case, dtype, src0, dy, dw, src1=None, bn=None, accumulate=0):
    """Fills a segmentation_training_pipeline_amd._lib.WgradParams with the case's geometry and the given device addresses (any
    non-zero integers on a host without a GPU: the plan queries read no memory).  ``bn`` = (mean, rstd, gamma, beta) addresses."""
    for k, val in geometry(case).items():
        setattr(P, k, val)
    P.src0, P.src1, P.dy, P.dw = src0, src1, dy, dw
    P.accumulate, P.dtype = accumulate, DT_CODE[dtype]
    if bn is not None:
        P.src_bn_mean, P.src_bn_rstd, P.src_bn_gamma, P.src_bn_beta = bn
        P.src_bn_relu = case.bn
    return P


def row_eligible(case, dtype):
    """wgrad_row_eligible of conv_wgrad_row.hip restated (variant 4 runs exactly on these)."""
    g = geometry(case)
    return (dtype != "fp32" and case.kh == 3 and case.kw == 3 and case.s == 1 and case.p == 1 and case.c0 % 64 == 0 and case.c1 % 64 == 0 and
            case.co % 8 == 0 and (g["Wo"] % 64 == 0 or (g["Wo"] >= 16 and 64 % g["Wo"] == 0 and (g["Ho"] * g["Wo"]) % 64 == 0)))


def sc_eligible(case, dtype):
    """stp_wgrad_sc_eligible of conv_sc_wgrad.hip restated: the 3x3 small-channel kernel, or the lean stem kernel (even width, 16-bit)."""
    if case.stem:
        return dtype != "fp32" and case.w % 2 == 0
    vec = 4 if dtype == "fp32" else 8
    cin = (16, 32) if vec == 4 else (16, 32, 64)
    return (case.kh == 3 and case.kw == 3 and case.s == 1 and case.p == 1 and case.c0 in cin and (case.c1 == 0 or case.c1 in cin) and
            case.co in ((4, 8, 16, 32) if vec == 4 else (8, 16, 32)) and case.co % vec == 0)


def sc_tiles(case):
    g = geometry(case)
    return g["N"] * (-(-g["Hv"] // SC_TH)) * (-(-g["Wv"] // SC_TW))


def expected_kernel_id(case, dtype):
    """What stp_conv2d_wgrad_kernel_id must answer: 1 small-channel / lean stem, 2 / 3 row-of-taps (128 / 64 rows), 0 the GEMM."""
    if case.splits == 0 and sc_eligible(case, dtype):
        return 1                                       # (GEMM case "32row": its GEMM tile is what variants 1-3 run)
    if case.splits == 0 and row_eligible(case, dtype):
        return 3 if case.co <= 64 else 2
    return 0


def _seed(case, salt):
    return zlib.crc32(("%s/%s/%s" % (case.family, case.name, salt)).encode()) & 0x7FFFFFFF


def _shapes(case):
    g = geometry(case)
    return ((case.n, case.h, case.w, case.c0), (case.n, g["Hv"], g["Wv"], case.c1) if case.c1 else None,
            (case.n, g["Ho"], g["Wo"], case.co), (case.co, case.kh, case.kw, case.c0 + case.c1))


def _reference(case, d):
    """Adds the float64 reference of the plain and of the accumulating launch to the inputs ``d``."""
    act = d["x0"] if case.bn is None else bn_act(d["x0"], *d["bn"], case.bn)
    v = virtual_source(act, d["x1"], case.up)
    d["dw"], d["abs"], d["nt"] = wgrad(v, d["dy"], case.kh, case.kw, case.s, case.p)
    d["dw_acc"] = d["dw"] + d["prev"].astype(np.float64)
    return d


@functools.lru_cache(maxsize=None)
def exact_case(case):
    """EXACT class: x integer in +-3 (a fused BatchNormalization: identity parameters, and -0.0, 6 and 7 among the inputs so that ReLU
    and ReLU6 both act), dy integer in +-2, prior dW integer in +-1000.  The stem's padded 4th channel is the constant 1."""
    rng = np.random.RandomState(_seed(case, "exact"))
    s0, s1, sdy, sdw = _shapes(case)
    x0 = rng.randint(-3, 4, size=s0).astype(np.float32)
    if case.bn is not None:
        flat = x0.reshape(-1)
        flat[0::11] = -0.0
        flat[3::13] = 6.0
        flat[5::17] = 7.0
    if case.stem:
        x0[..., 3] = 1.0
    d = dict(x0=x0, x1=rng.randint(-3, 4, size=s1).astype(np.float32) if s1 else None, dy=rng.randint(-2, 3, size=sdy).astype(np.float32),
             prev=rng.randint(-1000, 1001, size=sdw).astype(np.float32))
    c = case.c0
    d["bn"] = (np.zeros(c, np.float32), np.ones(c, np.float32), np.ones(c, np.float32), np.zeros(c, np.float32)) if case.bn is not None else None
    return _reference(case, d)


def rounded_inputs(case, dtype):
    """ROUNDED class: normal operands rounded to storage first; the prior dW is normal fp32.  (A fused BatchNormalization: the caller
    takes the reference over the tensor stp_bn_apply wrote - ``rounded_reference``.)"""
    rng = np.random.RandomState(_seed(case, "rounded/" + dtype))
    s0, s1, sdy, sdw = _shapes(case)
    x0 = through(rng.randn(*s0) * (2.0 if case.bn is not None else 1.0) + (0.5 if case.bn is not None else 0.0), dtype)
    if case.stem:
        x0[..., 3] = 1.0
    d = dict(x0=x0, x1=through(rng.randn(*s1), dtype) if s1 else None, dy=through(rng.randn(*sdy), dtype),
             prev=(rng.randn(*sdw) * 4.0).astype(np.float32))
    if case.bn is not None:
        c = case.c0
        flat = x0.reshape(-1, c).astype(np.float64)
        d["bn"] = (flat.mean(0).astype(np.float32), (1.0 / np.sqrt(flat.var(0) + 1e-3)).astype(np.float32),
                   (rng.rand(c) + 0.5).astype(np.float32), (rng.randn(c) * 0.3).astype(np.float32))
    else:
        d["bn"] = None
    return d


def rounded_reference(case, d, act=None):
    """Reference of the ROUNDED inputs ``d``; ``act`` = the normalised tensor as stp_bn_apply wrote it (fused-BatchNormalization cases)."""
    v = virtual_source(d["x0"] if act is None else act, d["x1"], case.up)
    d["dw"], d["abs"], d["nt"] = wgrad(v, d["dy"], case.kh, case.kw, case.s, case.p)
    d["dw_acc"] = d["dw"] + d["prev"].astype(np.float64)
    return d


@functools.lru_cache(maxsize=None)
def rounded_case(case, dtype):
    assert case.bn is None
    return rounded_reference(case, rounded_inputs(case, dtype))


def unpad_stem(dw):
    """[Cout][7][8][4] -> [Cout][7][7][3] (stp_weight_grad_unpad)."""
    return dw[:, :, :7, :3]


def all_single_cases():
    return GEMM_CASES + SC_CASES + [SC_MULTI_TRIP] + ROW_CASES
