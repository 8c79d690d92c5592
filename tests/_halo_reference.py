"""Float64 numpy restatement of what stp_conv2d computes with ``tile = 1024 + variant`` (csrc/conv_halo.hip), shared by
tests/test_halo_reference_host.py and tests/test_halo_ops_gpu.py.  Not collected, calls no kernel, no torch, no oracle/: it is written
from the comments of include/stp_hip.h on stp_conv_params,

    V[n,h,w,c]        = concat_c(nearest2x(src0) or src0, src1)                                   (taps outside V contribute nothing)
    out[n,y,x,co]     = sum_{kh,kw,c} V[n, y - 1 + kh, x - 1 + kw, c] * weight[co][kh][kw][c]     (3x3 / stride 1 / pad 1)
                        (+ sum_c fold_src[n,y,x,c] * fold_weight[co][c]: the stride-1 fold, one more centre tap)
    src_bn_*          : V = act(fma(src0, rstd * gamma, beta - mean * rstd * gamma)) rounded ONCE to storage; the padding pads THAT tensor
    epilogue          : ((out + bias) + residual) + prior (accumulate), ReLU, ONE rounding to storage; channels [0, Cd0) -> dst0, the rest dst1
                        (this is the order of the fp32 additions in epilogue_rm of conv_halo.hip and in conv_common.h)
    stats_partial     : [2][C][tiles]: per tile the sum and the sum of squares of the STORED values
    bnb_*             : g = dY where the activation of fma(bnb_x, rstd * gamma, beta - mean * rstd * gamma) passes the gradient (bnb_relu 0:
                        everywhere, 1: > 0, 2: strictly inside (0, 6)), rounded once; tables: sum g and sum g * xhat, xhat = (x - mean) * rstd
    dst_sum2x2        : dst0 [N,Ho/2,Wo/2,Cd0] = the 2 x 2 block sum of the fp32 tile (+ prior), stored and masked as the bnb form; tables
                        and accumulate refer to the low-resolution tensor; dst1 keeps the full resolution
    s2d_dgrad         : KH = KW = 2, pad 0, tap (da, db) reads (a + da, b + db); Cout = 4 Cq class-major, class (py, px) meets the 3x3
                        layer's tap (py + 1 - 2 da, px + 1 - 2 db) or nothing; the shortcut's dY is one more tap of class 0; channel
                        cls * Cq + c of (a, b) is channel c of (2a + py, 2b + px); tables [2][Cq][4 x tiles]

Every result comes with ``abs`` (sum of |products| plus |bias|, |residual|, |prior|) and ``n`` (products plus epilogue additions) per
element, from which ``rounding_bound`` makes the per-element bound of ANY order of fp32 additions ((n + 2) 2^-24 abs).
No bound is scaled by the largest element of a tensor and none is read from a kernel's output.  The case tables live here, so the
host test asserts the exactness condition and the plan facts on exactly the inputs and shapes the GPU test runs.
"""
import collections
import functools
import zlib

import numpy as np

H16 = ["bf16", "fp16"]
F32, BF16, F16 = 0, 1, 3                     # stp_dtype codes of include/stp_hip.h
DT_CODE = {"fp32": F32, "bf16": BF16, "fp16": F16}
SRC_DIRECT, SRC_NEAREST2X = 0, 1
HALO_CFGS = [(16, 128), (8, 128), (16, 64), (8, 64), (32, 64), (8, 64)]      # (TH, channel tile) of variants 0 - 5; tiles are TH x 16 pixels
TW = 16
EXACT_LIMIT = 2.0 ** 24                      # integers up to here are exact in fp32, and so is every partial sum below it
TINY = {"bf16": 2.0 ** -133, "fp16": 2.0 ** -24}      # the smallest positive value of the storage format
MASK_SHARE_CAP = 0.005                       # rounded class: at most this share of a case's elements may sit on a clamp edge
BADARG = -1


def through(a, dtype):
    """float32 values of ``a`` after one round-to-nearest-even into the storage dtype (numpy only; finite inputs)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if dtype == "fp32":
        return a.copy()
    if dtype == "fp16":
        return a.astype(np.float16).astype(np.float32)
    bits = a.view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(a.shape)


def nearest2x(x):
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


def virtual_source(src0, src1=None, up=False):
    v = nearest2x(np.asarray(src0)) if up else np.asarray(src0)
    return v if src1 is None else np.concatenate([v, np.asarray(src1)], axis=-1)


def bn_act(x, mean, rstd, gamma, beta, relu):
    """The producer BatchNormalization in float64: (x - mean) * rstd * gamma + beta, then none (0) / ReLU (1) / ReLU6 (2).  Used on the
    EXACT inputs only (integers, rstd 1), where it equals the kernel's one fma; the caller rounds once to storage."""
    y = (np.asarray(x, np.float64) - mean) * rstd * gamma + beta
    if relu >= 1:
        y = np.maximum(y, 0.0)
    if relu == 2:
        y = np.minimum(y, 6.0)
    return y + 0.0


def conv_taps(v, w, pad, live=None):
    """-> (value, abs, n) of out[n,y,x,co] = sum_{kh,kw,c} v[n, y - pad + kh, x - pad + kw, c] * w[co][kh][kw][c] on the grid of ``v``;
    taps outside ``v`` contribute nothing.  ``live`` [co][kh][kw] = products a tap really has (default: all C): n counts only those."""
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    N, H, W, C = v.shape
    Co, KH, KW, _ = w.shape
    av, aw = np.abs(v), np.abs(w)
    val, ab = np.zeros((N, H, W, Co)), np.zeros((N, H, W, Co))
    nt = np.zeros((H, W, Co), dtype=np.int64)
    live = np.full((Co, KH, KW), C, dtype=np.int64) if live is None else np.asarray(live, np.int64)
    for kh in range(KH):
        y0, y1 = max(0, pad - kh), min(H, H + pad - kh)              # output rows whose tap row y - pad + kh lies in the map
        for kw in range(KW):
            x0, x1 = max(0, pad - kw), min(W, W + pad - kw)
            if y1 <= y0 or x1 <= x0:
                continue
            sl = (slice(None), slice(y0 - pad + kh, y1 - pad + kh), slice(x0 - pad + kw, x1 - pad + kw))
            val[:, y0:y1, x0:x1] += v[sl] @ w[:, kh, kw, :].T
            ab[:, y0:y1, x0:x1] += av[sl] @ aw[:, kh, kw, :].T
            nt[y0:y1, x0:x1] += live[:, kh, kw]
    return val, ab, np.broadcast_to(nt, (N, H, W, Co))


def s2d_dense_weights(w3, cq):
    """The dense 2 x 2-tap matrix of the header from the 3x3 layer's weights w3 [dY channels][3][3][Cq] (forward form: output channel
    first): row cls * Cq + c, tap (da, db) holds w3[:, py + 1 - 2 da, px + 1 - 2 db, c] or nothing.  -> ([4 Cq][2][2][C0], live)."""
    c0 = w3.shape[0]
    wd = np.zeros((4 * cq, 2, 2, c0))
    live = np.zeros((4 * cq, 2, 2), dtype=np.int64)
    for cls in range(4):
        py, px = cls >> 1, cls & 1
        for da in range(2):
            for db in range(2):
                kh, kw = py + 1 - 2 * da, px + 1 - 2 * db
                if 0 <= kh < 3 and 0 <= kw < 3:
                    wd[cls * cq:(cls + 1) * cq, da, db, :] = w3[:, kh, kw, :].T
                    live[cls * cq:(cls + 1) * cq, da, db] = c0
    return wd, live


def depth_to_space(t, cq):
    """[N,H,W,4 Cq] class-major -> [N,2H,2W,Cq]: channel cls * Cq + c of (a, b) is channel c of (2a + (cls >> 1), 2b + (cls & 1))."""
    N, H, W, _ = t.shape
    return np.ascontiguousarray(t.reshape(N, H, W, 2, 2, cq).transpose(0, 1, 3, 2, 4, 5)).reshape(N, 2 * H, 2 * W, cq)


def bwd_copy(w):
    """stp_weight_prepare's data-gradient copy of forward weights w [Cout][3][3][Cin]: [Cin][kh'][kw'][Cout] = w[:, 2 - kh', 2 - kw', :]."""
    return np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


def pad_rows16(w):
    """Weight rows rounded up to a multiple of 16 with zero rows (the layout every weight operand of stp_conv_params has)."""
    rows = -(-w.shape[0] // 16) * 16
    out = np.zeros((rows,) + w.shape[1:], dtype=np.float32)
    out[:w.shape[0]] = w
    return out


def sum2x2(t):
    N, H, W, C = t.shape
    return t.reshape(N, H // 2, 2, W // 2, 2, C).sum(axis=(2, 4))


def tile_sums(t, th, tw=TW):
    """[N,H,W,C] -> [tiles][C], tiles in the order image, tile row, tile column."""
    N, H, W, C = t.shape
    return t.reshape(N, H // th, th, W // tw, tw, C).sum(axis=(2, 4)).reshape(-1, C)


def tile_sums_s2d(t, th, cq):
    """[N,2H,2W,Cq] (depth-to-space destination) -> [Cq][4 classes][tiles]: the tiles are TH x 16 pixels of the dY grid, per parity class."""
    N, H2, W2, _ = t.shape
    r = t.reshape(N, H2 // (2 * th), th, 2, W2 // (2 * TW), TW, 2, cq).sum(axis=(2, 5))      # [N][ty][py][tx][px][Cq]
    return np.ascontiguousarray(r.transpose(5, 2, 4, 0, 1, 3)).reshape(cq, 4, -1)


def rounding_bound(n, abs_terms):
    """(n + 2) * 2^-24 * abs_terms: every product rounds at most once and every addition once, relative to a partial
    sum that abs_terms bounds, in whatever order; ``n`` already counts the additions of the epilogue."""
    return (np.asarray(n, np.float64) + 2.0) * 2.0 ** -24 * np.asarray(abs_terms, np.float64)


def sort_columns(table):
    """Columns of a 2-d table in lexicographic order (the multiset of the per-tile column vectors)."""
    table = np.asarray(table)
    return table[:, np.lexsort(table[::-1])]


# ---------------------------------------------------------------------------------------------------------------------------------
# cases.  n, h, w = the grid the kernel's tiles lie on (the virtual map; for s2d the grid of dY); a nearest-2x src0 is stored at half of it.

Case = collections.namedtuple("Case", "name family n h w c0 c1 up co v cd0 fold_c s2d shortcut exact_only")


def _c(family, n, h, w, c0, co, v, c1=0, up=False, cd0=None, fold_c=0, s2d=False, shortcut=False, exact_only=False, name=None):
    name = name or "%d_%d_%d_%d%s_%d_v%d" % (n, h, w, c0, ("+%d" % c1 if c1 else "") + ("up" if up else ""), co, v)
    return Case(name, family, n, h, w, c0, c1, up, co, v, cd0, fold_c, s2d, shortcut, exact_only)


ONE_CASES = [
    _c("one", 1, 16, 16, 64, 128, 0),            # one tile, one slab: nine K-steps, the ring's prologue and drain only
    _c("one", 2, 16, 32, 192, 144, 0),           # three slabs (buffer 0 re-used), two images, second channel tile with 16 live rows
    _c("one", 2, 8, 16, 192, 80, 1),
    _c("one", 1, 48, 48, 64, 64, 2),             # 3 x 3 tiles: one without an image border
    _c("one", 1, 24, 48, 128, 64, 3),
    _c("one", 1, 24, 16, 256, 64, 3),            # four slabs
    _c("one", 1, 32, 16, 64, 80, 4),
    _c("one", 2, 64, 16, 64, 64, 4),
    _c("one", 1, 8, 16, 64, 64, 5),
]
ONE_MULTI_TRIP = _c("one", 3, 88, 256, 64, 64, 5, exact_only=True)      # 528 tiles against 2 x compute units workgroups
ONE_FIRST = {}                                    # the first case of each variant also runs the epilogue modes
for _case in ONE_CASES:
    ONE_FIRST.setdefault(_case.v, _case)
ONE_MODES = ["plain", "stats"]
ONE_EPILOGUE_MODES = ["bias_res_relu", "acc0", "two_dst"]
TWO_DST_CD0 = 40

TWO_CASES = [
    _c("two", 1, 8, 16, 64, 64, 3, c1=64, up=True),
    _c("two", 1, 16, 16, 128, 128, 0, c1=64, up=True),       # the slab that changes source
    _c("two", 1, 16, 16, 64, 128, 0, c1=128),
    _c("two", 1, 8, 16, 128, 64, 3, up=True),
]
TWO_MODES = ["plain", "stats", "bias_relu_acc"]

PBN_CASES = [_c("pbn", 1, 16, 16, 128, 128, 0), _c("pbn", 2, 8, 16, 192, 128, 1), _c("pbn", 1, 16, 16, 64, 64, 2), _c("pbn", 1, 8, 32, 512, 64, 3)]
PBN_MODES = {"exact": ["pbn%d_%s" % (r, a) for r in (0, 1, 2) for a in ("id", "aff")], "rounded": ["pbn%d_gen" % r for r in (0, 1, 2)]}

BNB_CASES = [_c("bnb", 1, 32, 16, 64, 128, 0), _c("bnb", 1, 16, 16, 64, 128, 1), _c("bnb", 1, 32, 16, 64, 64, 2), _c("bnb", 1, 16, 16, 64, 64, 3),
             _c("bnb", 1, 16, 16, 64, 64, 5)]
BNB_MODES = {"exact": ["bnb%d_%s_%s" % (r, a, l) for r in (0, 1, 2) for a in ("id", "aff") for l in ("first", "last")],
             "rounded": ["bnb%d_gen_%s" % (r, l) for r in (0, 1, 2) for l in ("first", "last")]}

# n, h, w, ci, (Cd0 | Cd1), variant; Cout = Cd0 + Cd1
SUM_CASES = [
    _c("sum", 1, 16, 32, 64, 192, 0, cd0=64),        # as listed: REFUSED, a 128-channel tile would lie in both destinations
    _c("sum", 1, 16, 32, 64, 192, 0, cd0=128),       # the shape that reaches the path on variant 0: (128 | 64)
    _c("sum", 1, 16, 16, 128, 256, 1, cd0=128),
    _c("sum", 1, 32, 16, 64, 128, 4, cd0=64),
    _c("sum", 2, 8, 16, 64, 192, 3, cd0=64),
]
SUM_REFUSED = SUM_CASES[0]
SUM_MODES = {"exact": ["sum1_id", "sum2_aff_acc0", "sum0_id_one"], "rounded": ["sum1_gen", "sum2_gen_acc0", "sum0_gen_one"]}

S2D_CASES = [_c("s2d", n, h, w, c0, 4 * cq, v, c1=(c0 if sc else 0), s2d=True, shortcut=sc, name="%d_%d_%d_%d_q%d_v%d%s" % (n, h, w, c0, cq, v, "_sc" if sc else ""))
             for cq in (32, 64, 96) for (n, h, w, v) in ((1, 16, 16, 0), (2, 8, 32, 1)) for c0 in (64, 128) for sc in (False, True)]
FOLD_CASES = [_c("fold", 1, 8, 16, 64, 64, 3, fold_c=64), _c("fold", 1, 16, 16, 128, 128, 0, fold_c=128), _c("fold", 1, 8, 16, 64, 64, 3, fold_c=128, name="1_8_16_64_64_v3_f128")]
DGRAD_MODES = {"exact": ["plain", "acc0", "bnb1_aff_last"], "rounded": ["plain", "acc0", "bnb1_gen_last"]}

GROUP_CASE = _c("group", 3, 56, 112, 64, 64, 3, exact_only=True)      # 147 tiles, G = 2, the last group short

# refusals: (case, mode, what)
REFUSALS = [
    (_c("refuse", 1, 24, 16, 64, 128, 0), "plain", "Ho % TH != 0"),
    (_c("refuse", 1, 16, 16, 96, 128, 0), "plain", "C0 = 96"),
    (_c("refuse", 1, 32, 16, 128, 64, 4), "plain", "variant 4 with C0 = 128"),
    (_c("refuse", 1, 8, 16, 64, 128, 5), "plain", "variant 5 with Cout = 128"),
    (_c("refuse", 1, 16, 16, 64, 256, 2, s2d=True), "plain", "s2d on variant 2"),
    (_c("refuse", 1, 16, 16, 64, 192, 0, s2d=True), "plain", "s2d with Cout = 192"),
    (_c("refuse", 1, 16, 16, 64, 128, 0), "bnb1_aff_first_nostats", "bnb_x without stats_partial"),
    (_c("refuse", 1, 16, 16, 64, 64, 3, fold_c=64), "bias", "fold with bias"),
    (_c("refuse", 1, 16, 32, 64, 192, 0, cd0=96), "sum1_id", "dst_sum2x2 with Cd0 = 96"),
    (SUM_REFUSED, "sum1_id", "dst_sum2x2 with Cd0 = 64 on 128-channel tiles"),
]
LAUNCH_LEVEL_REFUSALS = ("bnb_x without stats_partial",)      # the plan query answers a variant; stp_conv2d itself returns STP_E_BADARG

Opt = collections.namedtuple("Opt", "bias residual relu acc0 acc1 cd0 stats pbn bnb params sum2x2")


def options(case, mode):
    """What a mode string switches on.  pbn / bnb = the activation code or None; params = "id" (mean 0, gamma 1, beta 0), "aff" (mean 1,
    gamma 2, beta 3; rstd 1 in both) or "gen" (general, rounded class)."""
    parts = mode.split("_")
    head = parts[0]
    pbn = bnb = None
    params = None
    sum_ = False
    if head.startswith("pbn"):
        pbn, params = int(head[3:]), parts[1]
    elif head.startswith("bnb"):
        bnb, params = int(head[3:]), parts[1]
    elif head.startswith("sum"):
        bnb, params, sum_ = int(head[3:]), parts[1], True
    one = "one" in parts
    cd0 = case.cd0 if case.cd0 is not None else case.co
    if mode == "two_dst":
        cd0 = TWO_DST_CD0
    if sum_ and one:
        cd0 = case.cd0                                  # Cout becomes Cd0 (see ``cout_of``)
    return Opt(bias=mode in ("bias_res_relu", "bias_relu_acc", "bias"), residual=mode == "bias_res_relu", relu=mode in ("bias_res_relu", "bias_relu_acc"),
               acc0=mode in ("acc0", "bias_relu_acc") or "last" in parts or "acc0" in parts, acc1=mode == "two_dst" or (sum_ and not one),
               cd0=cd0, stats=(mode == "stats" or pbn is not None or bnb is not None) and "nostats" not in parts, pbn=pbn, bnb=bnb, params=params, sum2x2=sum_)


def cout_of(case, mode):
    return case.cd0 if (mode.startswith("sum") and mode.endswith("_one")) else case.co


def modes_of(case, klass):
    if case.family == "one":
        return ONE_MODES + (ONE_EPILOGUE_MODES if ONE_FIRST[case.v] is case else [])
    if case.family == "two":
        return TWO_MODES
    if case.family == "pbn":
        return PBN_MODES[klass]
    if case.family == "bnb":
        return BNB_MODES[klass]
    if case.family == "sum":
        return SUM_MODES[klass]
    if case.family in ("s2d", "fold"):
        return DGRAD_MODES[klass]
    if case.family == "group":
        return ["stats"]
    raise ValueError(case.family)


def geometry(case, mode):
    """-> dict of the stp_conv_params geometry fields of a launch."""
    o = options(case, mode)
    hs, ws = (case.h // 2, case.w // 2) if case.up else (case.h, case.w)
    k = 2 if case.s2d else 3
    co = cout_of(case, mode)
    return dict(N=case.n, Hs0=hs, Ws0=ws, Hv=case.h, Wv=case.w, C0=case.c0, C1=case.c1, src0_mode=SRC_NEAREST2X if case.up else SRC_DIRECT,
                KH=k, KW=k, stride=1, pad=0 if case.s2d else 1, Ho=case.h, Wo=case.w, Cout=co, Cd0=min(o.cd0, co), tile=1024 + case.v)


def tiles_of(case):
    return case.n * (case.h // HALO_CFGS[case.v][0]) * (case.w // TW)


def stat_channels(case, mode):
    o = options(case, mode)
    return o.cd0 if o.sum2x2 else (case.co // 4 if case.s2d else case.co)


def stats_floats(case, mode):
    """What stp_conv2d_stats_floats must answer: 2 * C * tiles, times 4 for the space-to-depth form (four column blocks per channel)."""
    return 2 * stat_channels(case, mode) * tiles_of(case) * (4 if case.s2d else 1)


def fill_params(P, case, mode, dtype, ptr):
    """Fills a segmentation_training_pipeline_amd._lib.ConvParams from the geometry and ``ptr`` = name -> device address (any non-zero
    integer on a host without a GPU: the plan queries read no memory).  Names: src0 src1 weight bias residual dst0 dst1 stats bnb_x
    bnb_mean bnb_rstd bnb_gamma bnb_beta pbn_mean pbn_rstd pbn_gamma pbn_beta fold_src fold_weight."""
    o = options(case, mode)
    for k, val in geometry(case, mode).items():
        setattr(P, k, val)
    two = min(o.cd0, P.Cout) < P.Cout
    P.src0, P.weight, P.dst0 = ptr["src0"], ptr["weight"], ptr["dst0"]
    P.src1 = ptr["src1"] if case.c1 else None
    P.dst1 = ptr["dst1"] if two else None
    P.bias = ptr["bias"] if o.bias else None
    P.residual = ptr["residual"] if o.residual else None
    P.accumulate0, P.accumulate1, P.relu, P.dtype = int(o.acc0), int(o.acc1 and two), int(o.relu), DT_CODE[dtype]
    P.stats_partial = ptr["stats"] if o.stats else None
    if o.bnb is not None:
        P.bnb_x, P.bnb_mean, P.bnb_rstd, P.bnb_gamma, P.bnb_beta, P.bnb_relu = ptr["bnb_x"], ptr["bnb_mean"], ptr["bnb_rstd"], ptr["bnb_gamma"], ptr["bnb_beta"], o.bnb
    if o.pbn is not None:
        P.src_bn_mean, P.src_bn_rstd, P.src_bn_gamma, P.src_bn_beta, P.src_bn_relu = ptr["pbn_mean"], ptr["pbn_rstd"], ptr["pbn_gamma"], ptr["pbn_beta"], o.pbn
    P.dst_sum2x2 = int(o.sum2x2)
    P.s2d_dgrad = int(case.s2d)
    if case.s2d and case.shortcut:
        P.fold_weight = ptr["fold_weight"]
    if case.fold_c:
        P.fold_src, P.fold_weight, P.fold_C = ptr["fold_src"], ptr["fold_weight"], case.fold_c
    return P


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

def _rng(case, salt):
    return np.random.RandomState(zlib.crc32(("%s/%s/%s" % (case.family, case.name, salt)).encode()) & 0x7FFFFFFF)


def _mask_edges(a, dtype, tiny):
    """Plants the values the activation masks turn on: -0.0, 0, 6, 7 and (``tiny``) ONE element with the smallest positive storage value."""
    flat = a.reshape(-1)
    flat[0::11] = -0.0
    flat[1::11] = 0.0
    flat[3::13] = 6.0
    flat[5::17] = 7.0
    if tiny:
        flat[7] = TINY[dtype]
    return a


def bn_params(c, params, rng=None, x=None):
    """-> (mean, rstd, gamma, beta) float32 [c]."""
    if params == "id":
        return np.zeros(c, np.float32), np.ones(c, np.float32), np.ones(c, np.float32), np.zeros(c, np.float32)
    if params == "aff":
        return np.ones(c, np.float32), np.ones(c, np.float32), np.full(c, 2.0, np.float32), np.full(c, 3.0, np.float32)
    flat = x.reshape(-1, c).astype(np.float64)
    return (flat.mean(0).astype(np.float32), (1.0 / np.sqrt(flat.var(0) + 1e-3)).astype(np.float32), (rng.rand(c) + 0.5).astype(np.float32),
            (rng.randn(c) * 0.3).astype(np.float32))


def weight_range(case):
    """Integer weights of the EXACT class: +-2 as in DESIGN.md 3.31 where the statistic sums of squares stay below 2^24 with it, +-1 for
    192 and more input channels and for the 512-pixel tiles of variant 4 (tests/test_halo_reference_host.py asserts the condition)."""
    return 1 if (case.c0 + case.c1 + case.fold_c >= 192 or case.v == 4 or case.family == "pbn") else 2


def weight_density(case):
    """Share of non-zero integer weights: under the affine producer BatchNormalization (values up to 15, all positive behind a ReLU)
    every fourth one."""
    return 0.25 if case.family == "pbn" else 1.0


@functools.lru_cache(maxsize=None)
def inputs(case, klass, dtype):
    """Every operand a launch of ``case`` may take (the modes pick among them).  EXACT: integers (x in +-3, w in +-weight_range, bias in
    +-8, residual in +-3, priors in +-100; mask inputs with the edge values planted).  ROUNDED: normal values rounded to storage first."""
    rng = _rng(case, klass + ("" if klass == "exact" else "/" + dtype))
    exact = klass == "exact"
    hs, ws = (case.h // 2, case.w // 2) if case.up else (case.h, case.w)
    ctot = case.c0 + case.c1
    d = {}

    def ints(lo, hi, shape):
        return rng.randint(lo, hi + 1, size=shape).astype(np.float32)

    def act(shape, scale=1.0, shift=0.0):
        return ints(-3, 3, shape) if exact else through(rng.randn(*shape) * scale + shift, dtype)

    d["x0"] = act((case.n, hs, ws, case.c0), 2.0 if case.family == "pbn" else 1.0, 0.5 if case.family == "pbn" else 0.0)
    if case.family == "pbn" and exact:
        _mask_edges(d["x0"], dtype, tiny=False)      # (the tiny value is planted under the affine instance only: ``pbn_source``)
    d["x1"] = act((case.n, case.h, case.w, case.c1)) if case.c1 else None
    wr = weight_range(case)
    if case.s2d:
        cq = case.co // 4
        d["w3"] = ints(-wr, wr, (case.c0, 3, 3, cq)) if exact else through(rng.randn(case.c0, 3, 3, cq) / np.sqrt(9 * case.c0), dtype)
        d["wsc"] = (ints(-wr, wr, (case.c1, cq)) if exact else through(rng.randn(case.c1, cq) / np.sqrt(case.c1), dtype)) if case.shortcut else None
        dst = (case.n, 2 * case.h, 2 * case.w, cq)
        d["prior0"], d["prior1"], d["bias"], d["residual"] = (ints(-100, 100, dst) if exact else through(rng.randn(*dst), dtype)), None, None, None
        d["bnb_x"] = _mask_edges(ints(-3, 3, dst), dtype, True) if exact else through(rng.randn(*dst) * 1.5 + 0.3, dtype)
        d["bnb_gen"] = None if exact else bn_params(cq, "gen", rng, d["bnb_x"])
        return d
    d["w"] = ints(-wr, wr, (case.co, 3, 3, ctot)) if exact else through(rng.randn(case.co, 3, 3, ctot) / np.sqrt(9 * ctot), dtype)
    if exact and weight_density(case) < 1.0:
        d["w"] = d["w"] * (rng.rand(*d["w"].shape) < weight_density(case))
    if case.fold_c:
        d["fold_src"] = act((case.n, case.h, case.w, case.fold_c))
        d["fold_w"] = ints(-wr, wr, (case.co, case.fold_c)) if exact else through(rng.randn(case.co, case.fold_c) / np.sqrt(case.fold_c), dtype)
    full = (case.n, case.h, case.w, case.co)
    d["bias"] = ints(-8, 8, (case.co,)) if exact else rng.randn(case.co).astype(np.float32)
    d["residual"] = ints(-3, 3, full) if exact else through(rng.randn(*full), dtype)
    d["prior"] = ints(-100, 100, full) if exact else through(rng.randn(*full), dtype)      # sliced into the priors of dst0 / dst1
    if case.family in ("bnb", "fold"):
        d["bnb_x"] = _mask_edges(ints(-3, 3, full), dtype, True) if exact else through(rng.randn(*full) * 1.5 + 0.3, dtype)
        d["bnb_gen"] = None if exact else bn_params(case.co, "gen", rng, d["bnb_x"])
    if case.family == "sum":
        low = (case.n, case.h // 2, case.w // 2, case.cd0)
        d["prior_low"] = ints(-100, 100, low) if exact else through(rng.randn(*low), dtype)
        d["bnb_x"] = _mask_edges(ints(-3, 3, low), dtype, True) if exact else through(rng.randn(*low) * 1.5 + 0.3, dtype)
        d["bnb_gen"] = None if exact else bn_params(case.cd0, "gen", rng, d["bnb_x"])
    if case.family == "pbn":
        d["pbn_gen"] = None if exact else bn_params(case.c0, "gen", rng, d["x0"])
    return d


def pbn_source(case, klass, dtype, params):
    """src0 of a fused-producer launch: the EXACT inputs, with the smallest positive storage value planted under the affine instance
    (fma(tiny, 2, 1) = 1 in fp32 and in float64 alike; under the identity a product of 2^-133 would reach the MFMA, whose handling of
    denormal operands the header leaves open, and decide a sum that is otherwise exactly zero)."""
    x = inputs(case, klass, dtype)["x0"]
    if klass == "exact" and params == "aff":
        x = x.copy()
        x.reshape(-1)[7] = TINY[dtype]
    return x


def bnb_params_of(case, klass, dtype, params):
    d = inputs(case, klass, dtype)
    c = d["bnb_x"].shape[-1]
    return bn_params(c, params) if params in ("id", "aff") else d["bnb_gen"]


def pbn_params_of(case, klass, dtype, params):
    return bn_params(case.c0, params) if params in ("id", "aff") else inputs(case, klass, dtype)["pbn_gen"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference of a launch

def s2d_dgrad(dy, w3, dysc=None, wsc=None):
    """s2d_dgrad as the header states it -> (value, abs, n) on the destination [N,2H,2W,Cq].  dy [N,H,W,C0]; w3 [C0][3][3][Cq] = the 3x3
    layer's forward weights; dysc [N,H,W,C1], wsc [C1][Cq] = the 1x1 / stride-2 shortcut's dY and forward weights."""
    N, H, W, _ = dy.shape
    cq = w3.shape[-1]
    wd, live = s2d_dense_weights(np.asarray(w3, np.float64), cq)
    # tap (da, db) reads (a + da, b + db): a window anchored at the pixel itself, nothing past the bottom / right edge
    val, ab, nt = conv_taps(np.pad(np.asarray(dy, np.float64), ((0, 0), (0, 1), (0, 1), (0, 0))), wd, 0, live)
    val, ab, nt = val[:, :H, :W], ab[:, :H, :W], np.array(nt[:, :H, :W])
    nt[:, -1, :, :] -= live[:, 1, :].sum(axis=1)                       # the products of the padded row / column do not exist
    nt[:, :, -1, :] -= live[:, :, 1].sum(axis=1)
    nt[:, -1, -1, :] += live[:, 1, 1]
    if dysc is not None:                                               # one more tap of class 0 (the even, even pixels)
        sc, ws = np.asarray(dysc, np.float64), np.asarray(wsc, np.float64)
        val[..., :cq] += sc @ ws
        ab[..., :cq] += np.abs(sc) @ np.abs(ws)
        nt[..., :cq] += sc.shape[-1]
    return tuple(depth_to_space(t, cq) for t in (val, ab, nt))


def conv3x3(v, w, fold_src=None, fold_w=None):
    """3x3 / stride 1 / pad 1 over the virtual source ``v`` -> (value, abs, n); fold_src [N,H,W,Cf] through fold_w [Cout][Cf] is one more
    centre tap (the stride-1 fold)."""
    val, ab, nt = conv_taps(v, w, 1)
    if fold_src is not None:
        fs, fw = np.asarray(fold_src, np.float64), np.asarray(fold_w, np.float64)
        val, ab, nt = val + fs @ fw.T, ab + np.abs(fs) @ np.abs(fw).T, nt + fs.shape[-1]
    return val, ab, nt


_CORE = {}


def core(case, klass, dtype, pbn_key=None, act=None):
    """-> (value, abs, n) of the convolution sum before the epilogue, float64, on the destination's grid ([N,2H,2W,Cq] for s2d).  ``act`` =
    the normalised src0 as stp_bn_apply wrote it (ROUNDED class with a fused producer BatchNormalization; not cached)."""
    key = (case, klass, dtype, pbn_key)
    if act is None and key in _CORE:
        return _CORE[key]
    d = inputs(case, klass, dtype)
    if case.s2d:
        out = s2d_dgrad(d["x0"], d["w3"], d["x1"] if case.shortcut else None, d["wsc"])
    else:
        x0 = d["x0"]
        if pbn_key is not None:
            relu, params = pbn_key
            # (EXACT class: the one fma is exact in fp32 - integers, and 1 + 2^-23 where the smallest positive half meets the affine
            # instance - so float64 followed by the ONE rounding to storage is what the kernel holds in LDS)
            x0 = act if act is not None else through(bn_act(pbn_source(case, klass, dtype, params), *pbn_params_of(case, klass, dtype, params), relu), dtype)
        out = conv3x3(virtual_source(x0, d["x1"], case.up), d["w"], d.get("fold_src"), d.get("fold_w"))
    if act is None:
        _CORE[key] = out
    return out


def mask_of(x, mean, rstd, gamma, beta, relu, exact):
    """-> (on, near) of the activation mask the bnb form re-derives from its input.  The kernel computes t = fma(x, sc, sh) with
    sc = fl(rstd * gamma), sh = fl(beta - mean * sc) (the product possibly fused) and lets the gradient pass where t > 0 (ReLU) or
    0 < t < 6 (ReLU6).  ``near`` marks the elements whose t lies within that arithmetic's own rounding, 2^-23 of the magnitudes that
    enter it, of a clamp edge; with ``exact`` (integer constants, rstd 1: every step is exact) there are none."""
    x = np.asarray(x, np.float64)
    sc = (rstd.astype(np.float32) * gamma.astype(np.float32)).astype(np.float64)
    sh = beta.astype(np.float64) - mean.astype(np.float64) * sc
    t = x * sc + sh
    none = np.zeros(x.shape, bool)
    if relu == 0:
        return np.ones(x.shape, bool), none
    margin = 2.0 ** -23 * (np.abs(x * sc) + np.abs(mean.astype(np.float64) * sc) + np.abs(beta.astype(np.float64)))
    on, near = t > 0, np.abs(t) <= margin
    if relu == 2:
        on, near = on & (t < 6), near | (np.abs(t - 6.0) <= margin)
    return on, (none if exact else near)


def _dest(pre, ab, n, relu=False, on=None, near=None):
    return dict(pre=pre, abs=ab, n=n, relu=relu, on=on, near=near)


def stored_reference(dst):
    """float64 value an exact kernel would round to storage: ReLU and the mask applied to ``pre``."""
    v = np.maximum(dst["pre"], 0.0) if dst["relu"] else dst["pre"]
    return np.where(dst["on"], v, 0.0) if dst["on"] is not None else v


def stored_bounds(dst):
    """-> (lo, hi) float64 before the storage rounding: act(pre -+ e) under the mask, e = rounding_bound(n, abs)."""
    e = rounding_bound(dst["n"], dst["abs"])
    lo, hi = dst["pre"] - e, dst["pre"] + e
    if dst["relu"]:
        lo, hi = np.maximum(lo, 0.0), np.maximum(hi, 0.0)
    if dst["on"] is not None:
        lo, hi = np.where(dst["on"], lo, 0.0), np.where(dst["on"], hi, 0.0)
    return lo, hi


def launch_reference(case, mode, klass, dtype, act=None):
    """-> dict(dst0=..., dst1=... or None, bnb=(x, mean, rstd) or None): per destination ``pre`` (the fp32 sum with the epilogue's additions,
    before ReLU / the mask), ``abs``, ``n``, ``relu``, ``on`` / ``near`` (mask).  The tables follow from the stored tensor: ``tables``."""
    o = options(case, mode)
    d = inputs(case, klass, dtype)
    val, ab, nt = core(case, klass, dtype, (o.pbn, o.params) if o.pbn is not None else None, act)
    co = cout_of(case, mode)
    if not case.s2d:
        val, ab, nt = val[..., :co], ab[..., :co], nt[..., :co]
    nt = np.array(nt, dtype=np.float64)
    ab = ab.copy()
    pre = val.copy()
    # the order of the fp32 additions in the epilogue: ((sum + bias) + residual) + prior, then ReLU, then one rounding
    if o.bias:
        pre, ab, nt = pre + d["bias"][:co].astype(np.float64), ab + np.abs(d["bias"][:co]), nt + 1
    if o.residual:
        pre, ab, nt = pre + d["residual"][..., :co], ab + np.abs(d["residual"][..., :co]), nt + 1
    out = dict(dst1=None, bnb=None)
    cd0 = min(o.cd0, co)
    if o.sum2x2:
        p0, a0, n0 = sum2x2(pre[..., :cd0]), sum2x2(ab[..., :cd0]), sum2x2(nt[..., :cd0]) + 3
        if o.acc0:
            p0, a0, n0 = p0 + d["prior_low"], a0 + np.abs(d["prior_low"]), n0 + 1
        m = bnb_params_of(case, klass, dtype, o.params)
        on, near = mask_of(d["bnb_x"], *m, o.bnb, klass == "exact")
        out["dst0"], out["bnb"] = _dest(p0, a0, n0, on=on, near=near), (d["bnb_x"], m[0], m[1])
        if cd0 < co:
            p1, a1, n1 = pre[..., cd0:], ab[..., cd0:], nt[..., cd0:]
            if o.acc1:
                pr = d["prior"][..., cd0:co]
                p1, a1, n1 = p1 + pr, a1 + np.abs(pr), n1 + 1
            out["dst1"] = _dest(p1, a1, n1)
        return out
    prior = d["prior0"] if case.s2d else d["prior"][..., :co]
    acc = np.zeros(pre.shape[-1], bool)
    acc[:cd0], acc[cd0:] = o.acc0, o.acc1
    pre, ab, nt = pre + np.where(acc, prior, 0.0), ab + np.where(acc, np.abs(prior), 0.0), nt + acc
    on = near = None
    if o.bnb is not None:
        m = bnb_params_of(case, klass, dtype, o.params)
        on, near = mask_of(d["bnb_x"], *m, o.bnb, klass == "exact")
        out["bnb"] = (d["bnb_x"], m[0], m[1])
    out["dst0"] = _dest(pre[..., :cd0], ab[..., :cd0], nt[..., :cd0], relu=o.relu, on=on, near=near)
    if cd0 < co:
        out["dst1"] = _dest(pre[..., cd0:], ab[..., cd0:], nt[..., cd0:], relu=o.relu)
    return out


def tables(case, mode, stored, bnb=None):
    """The statistic table of a launch from its STORED destination (float values of what dst0 - and dst1 - hold, channels concatenated):
    -> dict(value, abs, n, slack), each [2][C][columns] float64, columns in the order image, tile row, tile column (s2d: class-major
    blocks of them).  value[0] = sum, value[1] = sum of squares, or with ``bnb`` = (x, mean, rstd) sum g * xhat.  ``abs`` / ``n`` bound
    the kernel's own fp32 arithmetic (rounded class): for sum g * xhat it computes rstd * (sum g * x - mean * sum g), hence
    abs = rstd * (sum |g x| + |mean| sum |g|) and three more roundings.  ``slack`` is zero except in the column that holds the one
    input with the smallest positive storage value: g * tiny is no integer, each fp32 addition keeps or drops it, 2 |g| tiny covers both."""
    o = options(case, mode)
    th = HALO_CFGS[case.v][0]
    s = np.asarray(stored, np.float64)
    if o.sum2x2:
        sums = lambda t: tile_sums(t, th // 2, TW // 2).T
    elif case.s2d:
        cq = case.co // 4
        sums = lambda t: tile_sums_s2d(t, th, cq).reshape(cq, -1)
    else:
        sums = lambda t: tile_sums(t, th).T
    npix = th * TW // (4 if o.sum2x2 else 1)
    v0, a0 = sums(s), sums(np.abs(s))
    slack = np.zeros((2,) + v0.shape)
    if bnb is None:
        v1 = a1 = sums(s * s)
        n1 = npix
    else:
        x, mean, rstd = (np.asarray(t, np.float64) for t in bnb)
        v1 = sums(s * ((x - mean) * rstd))
        a1 = (sums(np.abs(s * x)) + sums(np.abs(s)) * np.abs(mean)[:, None]) * np.abs(rstd)[:, None]
        n1 = npix + 3
        tiny = (x > 0) & (x < 2.0 ** -20)
        slack[1] = 2.0 * sums(np.abs(s) * np.where(tiny, x, 0.0)) * np.abs(rstd)[:, None]
    return dict(value=np.stack([v0, v1]), abs=np.stack([a0, a1]), n=np.stack([np.full(v0.shape, npix), np.full(v0.shape, n1)]), slack=slack)


def group_table(table, G):
    """stats_group_out from stats_partial [2][C][tiles]: groups of G consecutive tiles summed in tile order, the last one may be short."""
    cols = table.shape[-1]
    ng = -(-cols // G)
    out = np.zeros(table.shape[:-1] + (ng,))
    for g in range(ng):
        out[..., g] = table[..., g * G:min(cols, (g + 1) * G)].sum(axis=-1)
    return out


def all_cases():
    return ONE_CASES + [ONE_MULTI_TRIP] + TWO_CASES + PBN_CASES + BNB_CASES + [c for c in SUM_CASES if c is not SUM_REFUSED] + S2D_CASES + FOLD_CASES + [GROUP_CASE]


def device_weights(case, klass, dtype):
    """-> dict of the weight operands as the launch takes them (float32 numpy, rows padded to 16): weight, fold_weight."""
    d = inputs(case, klass, dtype)
    if case.s2d:
        # NO weight copy of its own: the 3x3 layer's ordinary data-gradient copy [Cq^16][3][3][C0] and the shortcut's [Cq^16][C1]
        return dict(weight=pad_rows16(bwd_copy(d["w3"])), fold_weight=pad_rows16(np.ascontiguousarray(d["wsc"].T)) if case.shortcut else None)
    return dict(weight=pad_rows16(d["w"]), fold_weight=pad_rows16(d["fold_w"]) if case.fold_c else None)
