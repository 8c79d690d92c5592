"""Float64 numpy restatement of what stp_conv2d computes on the per-tap tiles of csrc/conv_igemm.hip (tile ids 1 - 7, 32 * STAGES + t,
256 + t), shared by tests/test_igemm_reference_host.py and tests/test_igemm_ops_gpu.py.  Not collected, calls no kernel, no torch, no
oracle/: it is written from the comments of include/stp_hip.h on stp_conv_params,

    V[n,h,w,c]        = concat_c(resample(src0), src1); resample = STP_SRC_DIRECT: src0 itself; STP_SRC_NEAREST2X: V(h, w) = src0(h / 2,
                        w / 2); STP_SRC_ZEROINS2X: V(h, w) = src0(h / 2, w / 2) iff h and w are even, else nothing (Hv = 2 Hs0 - 1)
    out[n,y,x,co]     = sum_{kh,kw,c} V[n, y * stride - pad + kh, x * stride - pad + kw, c] * weight[co][kh][kw][c]      (any KH x KW; taps
                        outside V contribute nothing)
                        (+ sum_c fold_src[n, y / 2, x / 2, c] * fold_weight[co][c] where y and x are even: the folded 1x1 / stride-2
                        shortcut, one more centre tap of parity class 0)
    weight_up         : the header's statement above stp_weight_prepare_upcollapse - class (py, px), tap (ty, tx), row taps of (py, ty):
                        (0,0) {0}, (0,1) {1,2}, (1,0) {0,1}, (1,1) {2}, columns alike: the 3x3 taps that share a low-resolution pixel summed
    epilogue          : ((out + bias) + residual) + prior (accumulate), ReLU, ONE rounding to storage; channels [0, Cd0) -> dst0, the rest dst1
                        (this is the order of the fp32 additions in epilogue_cf AND in epilogue_rm_lin of conv_common.h)
    stats_partial     : [2][Cout][pixel tiles]: per tile of tile_pixels(tile) consecutive pixels the sum and the sum of squares of the STORED
                        values; in the parity-class order of a stride-2 data gradient (and of weight_up) the tiles are LOGICAL ones:
                        class c = (y & 1) * 2 + (x & 1) major, then (n, y >> 1, x >> 1)
    bnb_*             : g = dY where the activation of fma(bnb_x, rstd * gamma, beta - mean * rstd * gamma) passes the gradient (bnb_relu 0:
                        everywhere, 1: > 0, 2: strictly inside (0, 6)), rounded once; tables: sum g and sum g * xhat over the STORED g
    stats_slots       : int64 slots [2][Cout][slots] in 2^-24 units; tile t adds its two sums into slot t % slots

Every result comes with ``abs`` and ``n`` per element as DESIGN.md 3.32 defines them (sum of |products| plus |bias|, |residual|, |prior|;
products that exist plus epilogue additions), from which ``rounding_bound`` of tests/_halo_reference.py makes the bound of ANY order of
fp32 additions.  A product whose V operand is a structural zero of the zero-inserted source is not counted: it is exactly zero whether
the kernel multiplies it (linear order) or skips it (parity-class order).  The case tables live here, so the host test asserts the
exactness condition and the plan facts on exactly the inputs and shapes the GPU test runs.
"""
import collections
import functools
import zlib

import numpy as np

from _halo_reference import (BADARG, DT_CODE, EXACT_LIMIT, H16, MASK_SHARE_CAP, TINY as TINY16, bn_act, bn_params, bwd_copy, mask_of, nearest2x,  # noqa: F401
                             pad_rows16, rounding_bound, sort_columns, stored_bounds, stored_reference, through, virtual_source, group_table)

DTYPES = ["fp32", "bf16", "fp16"]
TINY = dict(TINY16, fp32=2.0 ** -149)        # the smallest positive value of the storage format
SRC_DIRECT, SRC_NEAREST2X, SRC_ZEROINS2X = 0, 1, 2
SLOT_SCALE = 2.0 ** 24
# output channels x pixels of a workgroup's tile, by t = id % 32 (id - 256 for the per-lane-tap form): launch_tile of conv_igemm.hip
TILE_BM = {1: 128, 2: 64, 3: 32, 4: 16, 5: 64, 6: 128, 7: 64}
TILE_BN = {1: 128, 2: 256, 3: 256, 4: 256, 5: 64, 6: 64, 7: 128}
GENERAL_IDS = [1, 2, 3, 4, 5, 6, 7]
UNIFORM_IDS = [65, 66, 67, 68, 69, 70, 71, 97, 98, 101, 102, 103, 133, 134]
PERLANE_IDS = [257, 258, 259, 260, 261, 262]


def tile_t(tile):
    return tile - 256 if tile >= 256 else tile % 32


def tile_pixels(tile):
    return TILE_BN[tile_t(tile)]


def tile_bm(tile):
    return TILE_BM[tile_t(tile)]


def ring_stages(tile):
    return 2 if tile >= 256 else tile // 32


def ke(dtype):
    """Elements of a 128-byte K-tile."""
    return 32 if dtype == "fp32" else 64


# ---------------------------------------------------------------------------------------------------------------------------------
# the operation

def zero_insert(x):
    x = np.asarray(x)
    n, h, w, c = x.shape
    v = np.zeros((n, 2 * h - 1, 2 * w - 1, c), dtype=x.dtype)
    v[:, ::2, ::2] = x
    return v


def resample(src0, mode):
    return zero_insert(src0) if mode == SRC_ZEROINS2X else nearest2x(np.asarray(src0)) if mode == SRC_NEAREST2X else np.asarray(src0)


def conv_general(v, w, stride, pad, ho, wo, live0=None, c0=None):
    """-> (value, abs, n) of out[n,y,x,co] = sum_{kh,kw,c} v[n, y * stride - pad + kh, x * stride - pad + kw, c] * w[co][kh][kw][c] on an
    ho x wo grid; taps outside ``v`` contribute nothing.  ``live0`` [Hv][Wv] bool = where the first ``c0`` channels of ``v`` hold a real
    sample (zero-inserted source): n counts only products that exist."""
    v, w = np.asarray(v, np.float64), np.asarray(w, np.float64)
    N, Hv, Wv, C = v.shape
    Co, KH, KW, _ = w.shape
    c0 = C if c0 is None else c0
    av, aw = np.abs(v), np.abs(w)
    val, ab = np.zeros((N, ho, wo, Co)), np.zeros((N, ho, wo, Co))
    nt = np.zeros((ho, wo), dtype=np.int64)
    ys, xs = np.arange(ho) * stride - pad, np.arange(wo) * stride - pad
    ns = np.arange(N)
    for kh in range(KH):
        yy = np.flatnonzero((ys + kh >= 0) & (ys + kh < Hv))
        for kw in range(KW):
            xx = np.flatnonzero((xs + kw >= 0) & (xs + kw < Wv))
            if not yy.size or not xx.size:
                continue
            src, dst = np.ix_(ns, ys[yy] + kh, xs[xx] + kw), np.ix_(ns, yy, xx)
            val[dst] += v[src] @ w[:, kh, kw, :].T
            ab[dst] += av[src] @ aw[:, kh, kw, :].T
            l0 = 1 if live0 is None else live0[np.ix_(ys[yy] + kh, xs[xx] + kw)].astype(np.int64)
            nt[np.ix_(yy, xx)] += l0 * c0 + (C - c0)
    return val, ab, np.broadcast_to(nt[None, :, :, None], (N, ho, wo, Co))


UP_TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}      # row (column) taps of (parity, collapsed tap)


def collapse_weights(w, c0):
    """weight_up of the header from the master w [Cout][3][3][C0 + C1] -> [Cout][4 classes][2][2][C0] float64."""
    w = np.asarray(w, np.float64)
    out = np.zeros((w.shape[0], 4, 2, 2, c0))
    for py in (0, 1):
        for px in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    out[:, py * 2 + px, ty, tx] = sum(w[:, kh, kw, :c0] for kh in UP_TAPS[(py, ty)] for kw in UP_TAPS[(px, tx)])
    return out


def conv_collapsed(lo, x1, wup, w, c0):
    """The class-collapsed forward: per output parity class (py, px) tap (ty, tx) reads the low-resolution pixel (i + ty - 1 + py,
    j + tx - 1 + px) of ``lo`` [N,H/2,W/2,C0] through wup [Cout][4][2][2][C0]; src1 ``x1`` [N,H,W,C1] takes the plain nine taps of
    w[..., c0:].  -> (value, abs, n) on [N,H,W,Cout]."""
    lo, wup = np.asarray(lo, np.float64), np.asarray(wup, np.float64)
    N, H2, W2, _ = lo.shape
    co = wup.shape[0]
    val, ab, nt = conv_general(x1, np.asarray(w, np.float64)[..., c0:], 1, 1, 2 * H2, 2 * W2)
    val, ab, nt = val.copy(), ab.copy(), np.array(nt)
    lp = np.pad(lo, ((0, 0), (1, 1), (1, 1), (0, 0)))
    inb = np.pad(np.ones((H2, W2), np.int64), 1)
    for py in (0, 1):
        for px in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    sl = (slice(py + ty, py + ty + H2), slice(px + tx, px + tx + W2))
                    wt = wup[:, py * 2 + px, ty, tx]
                    val[:, py::2, px::2] += lp[(slice(None),) + sl] @ wt.T
                    ab[:, py::2, px::2] += np.abs(lp[(slice(None),) + sl]) @ np.abs(wt).T
                    nt[:, py::2, px::2] += (inb[sl] * c0)[None, :, :, None]
    return val, ab, nt


# ---------------------------------------------------------------------------------------------------------------------------------
# cases.  hs, ws = the stored size of src0; hv, wv = the virtual map; c0 / c1 / fold_c as given for 16-bit storage, halved in fp32 where
# ``halve`` (the K-tile count stays the same: KE = 64 elements in 16 bit, 32 in fp32)

Case = collections.namedtuple("Case", "name family n hs ws hv wv mode c0 c1 co kh kw stride pad ho wo tile auto halve fold_c upc wr density builds modes")


def _name(n, h, w, c0, c1, co, kh, kw, s, p, tile, extra=""):
    return "%d_%d_%d_%d%s_%d_k%dx%ds%dp%d_t%d%s" % (n, h, w, c0, "+%d" % c1 if c1 else "", co, kh, kw, s, p, tile, extra)


def fwd(family, n, h, w, c0, co, k, s, p, tile, modes, c1=0, up=False, kw=None, halve=False, upc=False, wr=2, density=1.0, builds=DTYPES, auto=False):
    """Forward form: h, w = the virtual map (src0 stored at half of it when ``up``)."""
    kw = kw or k
    hs, ws = (h // 2, w // 2) if up else (h, w)
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - kw) // s + 1
    return Case(_name(n, h, w, c0, c1, co, k, kw, s, p, tile, ("up" if up else "") + ("c" if upc else "")), family, n, hs, ws, h, w, SRC_NEAREST2X if up else SRC_DIRECT,
                c0, c1, co, k, kw, s, p, ho, wo, tile, auto, halve, 0, upc, wr, density, tuple(builds), tuple(modes))


def dgrad(family, n, h, w, cdy, cin, k, s, p, tile, modes, halve=False, fold=0, wr=2, density=1.0, builds=DTYPES, auto=False):
    """Data gradient of a k x k / stride s / pad p convolution cin -> cdy whose input map is h x w: src0 = dY, stride 1, pad k - 1 - p, the
    zero-inserted source for s = 2; ``fold``: channels of the folded shortcut's dY."""
    hs, ws = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    hv, wv = (2 * hs - 1, 2 * ws - 1) if s == 2 else (hs, ws)
    return Case(_name(n, h, w, cdy, 0, cin, k, k, s, p, tile, "dg" + ("f%d" % fold if fold else "")), family, n, hs, ws, hv, wv, SRC_ZEROINS2X if s == 2 else SRC_DIRECT,
                cdy, 0, cin, k, k, 1, k - 1 - p, h, w, tile, auto, halve, fold, False, wr, density, tuple(builds), tuple(modes))


def dims(case, dtype):
    """-> (c0, c1, fold_c) of the launch in this build."""
    d = 2 if (case.halve and dtype == "fp32") else 1
    return case.c0 // d, case.c1 // d, case.fold_c // d


def ut_ok(case, dtype):
    """fill_args' answer: 1 = uniform-tap eligible, 2 = per-lane-tap eligible, 0 = general kernel only (3 = the 4-channel stem form)."""
    c0, c1, _ = dims(case, dtype)
    if dtype != "fp32" and c0 == 4 and c1 == 0:
        return 3
    k = ke(dtype)
    if (c0 + c1) % k == 0 and c0 % k == 0:
        return 1
    return 2 if (c1 == 0 and k % (c0 + c1) == 0) else 0


def k_tiles(case, dtype):
    c0, c1, _ = dims(case, dtype)
    return -(-(case.kh * case.kw * (c0 + c1)) // ke(dtype))


BNB = ["bnb%d_P_%s" % (r, l) for r in (0, 1, 2) for l in ("first", "last")]
EP_MODES = ["plain", "bias", "bias_relu", "res", "acc", "bias_res_relu_acc", "stats", "stats_res", "stats_acc", "stats_bias"] + BNB + ["two16", "two4"]
PS = ["plain", "stats"]
DG = ["plain", "acc", "bnb1_P_first", "bnb1_P_last"]

GENERAL_CASES = (
    [fwd("general", 3, 7, 5, 24, 40, 3, 1, 1, t, PS) for t in GENERAL_IDS] +                 # K = 216 ragged, Cout ragged, P = 105
    [fwd("general", 1, 9, 11, 32, TILE_BM[t] + 8, 3, 1, 1, t, ["plain"], halve=True) for t in GENERAL_IDS] +      # a second channel tile with 8 live rows
    [fwd("general", 1, 6, 5, 16, co, 3, 1, 1, t, ["bias"]) for co in (1, 3) for t in (4, 5)] +      # the scalar channel tail, weight rows padded to 16
    [fwd("general", 1, 6, 5, 16, 20, 3, 1, 1, 3, ["stats", "stats_bias"])] +                 # the fragment-order sums, Cout % 8 != 0
    [fwd("general", 1, 9, 11, 4, 64, 7, 2, 3, t, PS, kw=8, builds=H16) for t in (2, 5)] +      # the stem geometry on the two C4 instances
    [fwd("general", 2, 6, 10, 8, 24, 3, 1, 1, t, PS, c1=16, up=True) for t in (3, 5)] +
    [dgrad("general", 2, 9, 11, 16, 24, 3, 2, 1, 5, ["plain", "acc"]), dgrad("general", 2, 8, 8, 16, 24, 1, 2, 0, 5, ["plain", "acc"]),
     fwd("general", 1, 8, 8, 16, 16, 4, 2, 1, 4, ["plain"])]
)
STEM_CASES = [c for c in GENERAL_CASES if c.kw == 8]

UNIFORM_CASES = (
    [fwd("uniform", 1, 9, 11, 64, tile_bm(t) + 8, 3, 1, 1, t, PS, halve=True) for t in UNIFORM_IDS] +      # P = 99: pixels and channels ragged; nine K-tiles
    # ring depth against K-tiles: nk = 1, 2, 3 on rings of 2, 3, 4 stages
    [fwd("ring", 2, 5, 7, c, co, 1, 1, 0, t, ["plain"], halve=True) for c in (64, 128, 192) for (co, ts) in ((72, (69, 101, 133)), (136, (70, 102, 134))) for t in ts] +
    [fwd("uniform", 1, 8, 12, 64, 72, 3, 1, 1, t, ["plain", "stats", "bias_relu_acc"], c1=64, up=True, halve=True) for t in (69, 133)] +
    [fwd("uniform", 1, 8, 12, 64, 72, 3, 1, 1, t, ["plain", "stats", "bias_relu_acc"], c1=128, halve=True, wr=1) for t in (69, 133)] +
    [dgrad("uniform", 1, 9, 11, 64, 72, 3, 2, 1, 69, ["plain", "acc"], halve=True)]                      # ZEROINS2X on an odd map: no parity order
)
RING_CASES = [c for c in UNIFORM_CASES if c.family == "ring"]

PERLANE_CASES = (
    [fwd("perlane", 1, 9, 11, c, tile_bm(t) + 8, 3, 1, 1, t, PS if c == 16 else ["plain"], halve=True) for t in PERLANE_IDS for c in (8, 16, 32)] +
    [fwd("perlane", 1, 8, 12, 16, 24, 3, 1, 1, 259, PS, up=True, halve=True),
     dgrad("perlane", 2, 12, 12, 32, 16, 3, 2, 1, 260, ["plain", "acc"], halve=True)]
)

# parity-class order: (dx map, id) pairs whose quarter is a multiple of the id's pixel tile
_PAR = [(1, 16, 16, 69), (1, 16, 16, 133), (1, 16, 32, 65), (1, 16, 32, 70), (1, 16, 32, 71), (1, 16, 32, 103), (1, 32, 32, 66), (2, 16, 16, 69)]
PARITY_CASES = (
    [dgrad("parity", n, h, w, 64, 64, 3, 2, 1, t, DG, halve=True) for (n, h, w, t) in _PAR] +
    [dgrad("parity", 1, 16, 16, 64, cin, 3, 2, 1, t, DG, halve=True) for cin in (72, 20) for t in (69, 133)] +
    [dgrad("parity", 1, 16, 16, 64, cin, 1, 2, 0, 69, DG, halve=True) for cin in (64, 20)]                 # three classes without a live tap: nk == 0
)
# one condition of zperm_applies missed: the same reference in the linear order
PARITY_MISSES = [dgrad("miss", 1, 15, 16, 64, 64, 3, 2, 1, 69, ["plain", "stats_acc"], halve=True),      # odd Ho
                 dgrad("miss", 1, 16, 16, 64, 64, 3, 2, 1, 65, ["plain", "stats_acc"], halve=True)]      # P / 4 = 64 against 128-pixel tiles

FOLD_MODES = ["plain", "acc", "bnb1_P_last"]
FOLD_CASES = [dgrad("fold", 1, 16, 16, 64, 64, 3, 2, 1, 69, FOLD_MODES, halve=True, fold=64, auto=True),
              dgrad("fold", 1, 16, 16, 64, 128, 3, 2, 1, 133, FOLD_MODES, halve=True, fold=64, auto=True),
              dgrad("fold", 2, 16, 16, 64, 64, 3, 2, 1, 69, FOLD_MODES, halve=True, fold=64, auto=True)]

UPC_MODES = ["plain", "stats", "bias_relu_acc"]
UPC_CASES = [fwd("upc", 1, 16, 16, 64, 64, 3, 1, 1, t, UPC_MODES, c1=64, up=True, halve=True, upc=True) for t in (69, 133)] + \
            [fwd("upc", 1, 16, 32, 128, 128, 3, 1, 1, 65, UPC_MODES, c1=64, up=True, halve=True, upc=True, wr=1)]
UPC_MISS = fwd("upcmiss", 1, 8, 12, 64, 64, 3, 1, 1, 69, ["plain", "stats"], c1=64, up=True, halve=True, upc=True)      # P / 4 = 24: the plain gather

EP_CASES = [fwd("ep", 3, 7, 5, 24, 40, 3, 1, 1, 5, EP_MODES), fwd("ep", 1, 9, 11, 64, 40, 3, 1, 1, 69, EP_MODES, halve=True),
            fwd("ep", 1, 9, 11, 16, 40, 3, 1, 1, 261, EP_MODES, halve=True)]

SLOT_COUNTS = (1, 4, 64)
SLOT_MODES = [m for s in SLOT_COUNTS for m in ("stats_s%d" % s, "bnb1_P_last_s%d" % s)]
SLOT_CASES = [fwd("slots", 1, 8, 16, 64, 64, 3, 1, 1, 69, SLOT_MODES, halve=True), fwd("slots", 2, 35, 64, 64, 64, 3, 1, 1, 69, SLOT_MODES, halve=True)]

GROUP_CASE = fwd("group", 1, 43, 192, 64, 64, 3, 1, 1, 69, ["stats"], builds=H16)      # 129 columns: G = 2, 65 groups, the last one short

# forced DMA ids on a shape whose channels do not admit them: refused, and the automatic choice then works
FORCED_DMA_REFUSED = [fwd("forced", 1, 9, 11, 24, 40, 3, 1, 1, 69, ["plain"]), fwd("forced", 1, 9, 11, 24, 40, 3, 1, 1, 261, ["plain"]),
                      fwd("forced", 1, 9, 11, 64, 40, 3, 1, 1, 261, ["plain"], halve=True)]

# refusals: (case, mode, overrides, what); every one is answered by stp_conv2d itself
_RBASE = fwd("refuse", 1, 9, 11, 64, 40, 3, 1, 1, 69, ["plain"], halve=True)
_RFOLD = FOLD_CASES[0]
REFUSALS = [
    (_RBASE, "plain", dict(dst_sum2x2=1), "dst_sum2x2 on a shape only this family serves"),
    (_RBASE, "plain", dict(src_bn_mean=True), "src_bn_mean on a shape only this family serves"),
    (_RBASE, "bnb1_id_first", dict(stats_partial=None), "bnb_x without stats_partial"),
    (_RBASE, "bnb1_id_first", dict(relu=1), "bnb_x with relu"),
    (_RBASE, "bnb1_id_first", dict(residual=True), "bnb_x with residual"),
    (_RBASE, "two16", dict(stats_partial=True), "statistics with two destinations"),
    (_RBASE, "stats", dict(stats_slots=3), "stats_slots = 3"),
    (_RBASE, "stats", dict(stats_slots=128), "stats_slots = 128"),
    (_RBASE, "stats_s4", dict(stats_group=2), "stats_group with slots"),
    (_RBASE, "plain", dict(C0=10), "C0 % vec != 0"),
    (_RBASE, "plain", dict(s2d_dgrad=1), "s2d_dgrad where the halo kernel declines"),
    (_RFOLD, "plain", dict(fold_C=8), "fold_C != C0"),
    (dgrad("refuse", 1, 16, 16, 64, 32, 3, 2, 1, 67, FOLD_MODES, halve=True, fold=64, auto=True), "plain", {}, "a Cout whose automatic tile breaks the P / 4 condition"),
    (_RFOLD, "plain", dict(tile=69), "a fold on a forced tile"),
]
FOLD_REFUSED_BY_QUERY = ("a Cout whose automatic tile breaks the P / 4 condition", "a fold on a forced tile")      # stp_conv2d_fold_ok answers 0


def all_cases():
    return GENERAL_CASES + UNIFORM_CASES + PERLANE_CASES + PARITY_CASES + PARITY_MISSES + FOLD_CASES + UPC_CASES + [UPC_MISS] + EP_CASES + SLOT_CASES + [GROUP_CASE]


Opt = collections.namedtuple("Opt", "bias residual relu acc0 acc1 cd0 stats slots bnb params")


def options(case, mode):
    """What a mode string switches on: tokens plain bias relu res acc stats s<slots> bnb<relu> id|aff|gen first|last two<Cd0>."""
    parts = mode.split("_")
    bnb = params = None
    slots, cd0, acc1 = 0, case.co, False
    for t in parts:
        if t.startswith("bnb"):
            bnb = int(t[3:])
        elif t in ("id", "aff", "gen"):
            params = t
        elif t.startswith("two"):
            cd0, acc1 = int(t[3:]), True
        elif t[0] == "s" and t[1:].isdigit():
            slots = int(t[1:])
    return Opt(bias="bias" in parts, residual="res" in parts, relu="relu" in parts, acc0="acc" in parts or "last" in parts, acc1=acc1, cd0=cd0,
               stats="stats" in parts or bnb is not None, slots=slots, bnb=bnb, params=params)


def modes_of(case, klass):
    out = []
    for m in case.modes:
        if "_P_" in m:
            out += [m.replace("_P_", "_%s_" % p) for p in (("id", "aff") if klass == "exact" else ("gen",))]
        else:
            out.append(m)
    return out


def classes_of(case):
    return ["exact"] if case.family == "group" else ["exact", "rounded"]


def epilogue_is_row_major(case, mode, dtype, no_rm=False):
    """epilogue_rm_ok of conv_common.h for the kernel that has the row-major epilogue (the buffer-DMA kernel in 16-bit storage)."""
    o = options(case, mode)
    cd0 = min(o.cd0, case.co)
    return (dtype != "fp32" and case.tile >= 64 and not no_rm and case.co % 8 == 0 and cd0 % 8 == 0 and (case.co - cd0) % 8 == 0 and not o.slots)


def parity_order(case, dtype):
    """zperm_applies / the weight_up condition of stp_conv2d: does this launch take the parity-class pixel order?"""
    tile, P = case.tile, case.n * case.ho * case.wo
    c0, c1, _ = dims(case, dtype)
    even = case.ho % 2 == 0 and case.wo % 2 == 0 and (P // 4) % tile_pixels(tile) == 0
    if case.mode == SRC_ZEROINS2X:
        return ut_ok(case, dtype) == 1 and 64 <= tile < 256 and case.stride == 1 and case.kh <= 3 and case.kw <= 3 and c1 == 0 and even
    if case.upc:
        return (case.mode == SRC_NEAREST2X and ut_ok(case, dtype) == 1 and (64 <= tile < 96 or tile == 133) and (case.kh, case.kw, case.stride, case.pad) == (3, 3, 1, 1)
                and (case.ho, case.wo) == (case.hv, case.wv) and c1 > 0 and c1 % ke(dtype) == 0 and even)
    return False


def pixel_order(case, dtype):
    """Flattened real pixel of every logical pixel, or None for the linear order (zperm_decode of conv_common.h)."""
    if not parity_order(case, dtype):
        return None
    P = case.n * case.ho * case.wo
    pl = np.arange(P)
    pc, h2w2, w2 = P // 4, (case.ho // 2) * (case.wo // 2), case.wo // 2
    c, q = pl // pc, pl % pc
    n, rem = q // h2w2, q % h2w2
    y, x = 2 * (rem // w2) + (c >> 1), 2 * (rem % w2) + (c & 1)
    return (n * case.ho + y) * case.wo + x


def live_k_tiles(case, dtype):
    """K-tiles each parity class runs in the parity-class order of a zero-inserted source (znk + zfn of the kernel), class 0 first."""
    c0, _, fc = dims(case, dtype)
    out = []
    for c in range(4):
        kh0, kw0 = ((c >> 1) + case.pad) & 1, ((c & 1) + case.pad) & 1
        out.append(((case.kh - kh0 + 1) >> 1) * ((case.kw - kw0 + 1) >> 1) * (c0 // ke(dtype)) + (fc // ke(dtype) if c == 0 else 0))
    return out


def stats_tiles(case):
    return -(-(case.n * case.ho * case.wo) // tile_pixels(case.tile))


def stats_floats(case):
    return 2 * case.co * stats_tiles(case)


def geometry(case, mode, dtype):
    o = options(case, mode)
    c0, c1, fc = dims(case, dtype)
    return dict(N=case.n, Hs0=case.hs, Ws0=case.ws, Hv=case.hv, Wv=case.wv, C0=c0, C1=c1, src0_mode=case.mode, KH=case.kh, KW=case.kw, stride=case.stride,
                pad=case.pad, Ho=case.ho, Wo=case.wo, Cout=case.co, Cd0=min(o.cd0, case.co), tile=0 if case.auto else case.tile)


def fill_params(P, case, mode, dtype, ptr, **over):
    """Fills a segmentation_training_pipeline_amd._lib.ConvParams; ``ptr`` = name -> device address (any non-zero integer on a host
    without a GPU: the plan queries read no memory).  Names: src0 src1 weight weight_up bias residual dst0 dst1 stats bnb_x bnb_mean bnb_rstd
    bnb_gamma bnb_beta fold_src fold_weight group_out counters pbn.  ``over``: fields set afterwards (True = the pointer of that name)."""
    o = options(case, mode)
    for k, val in geometry(case, mode, dtype).items():
        setattr(P, k, val)
    two = P.Cd0 < P.Cout
    c0, c1, fc = dims(case, dtype)
    P.src0, P.weight, P.dst0 = ptr["src0"], ptr["weight"], ptr["dst0"]
    P.src1 = ptr["src1"] if c1 else None
    P.dst1 = ptr["dst1"] if two else None
    P.bias = ptr["bias"] if o.bias else None
    P.residual = ptr["residual"] if o.residual else None
    P.accumulate0, P.accumulate1, P.relu, P.dtype = int(o.acc0), int(o.acc1 and two), int(o.relu), DT_CODE[dtype]
    P.stats_partial = ptr["stats"] if o.stats else None
    P.stats_slots = o.slots
    if o.bnb is not None:
        P.bnb_x, P.bnb_mean, P.bnb_rstd, P.bnb_gamma, P.bnb_beta, P.bnb_relu = ptr["bnb_x"], ptr["bnb_mean"], ptr["bnb_rstd"], ptr["bnb_gamma"], ptr["bnb_beta"], o.bnb
    if case.upc:
        P.weight_up = ptr["weight_up"]
    if fc:
        P.fold_src, P.fold_weight, P.fold_C = ptr["fold_src"], ptr["fold_weight"], fc
    for k, val in over.items():
        if k == "stats_partial":
            P.stats_partial = ptr["stats"] if val else None
        elif k == "residual":
            P.residual = ptr["residual"]
        elif k == "src_bn_mean":
            P.src_bn_mean, P.src_bn_rstd = ptr["pbn"], ptr["pbn"]
        elif k == "stats_group":
            P.stats_group, P.stats_group_out, P.stats_group_counters = val, ptr["group_out"], ptr["counters"]
        else:
            setattr(P, k, val)
    return P


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

def _rng(case, salt):
    return np.random.RandomState(zlib.crc32(("%s/%s/%s" % (case.family, case.name, salt)).encode()) & 0x7FFFFFFF)


@functools.lru_cache(maxsize=None)
def inputs(case, klass, dtype):
    """Every operand a launch of ``case`` may take (the modes pick among them).  EXACT: integers (x in +-3, w in +-case.wr thinned to
    case.density, bias in +-8, residual in +-3, priors in +-100; mask inputs with -0.0, 0, 6, 7 and one smallest positive storage value).
    ROUNDED: normal values rounded to storage first.  The fp32 build of a halved case has its own (narrower) operands."""
    rng = _rng(case, klass + "/" + (dtype if (klass != "exact" or (case.halve and dtype == "fp32")) else "any"))
    exact = klass == "exact"
    c0, c1, fc = dims(case, dtype)
    ctot = c0 + c1
    d = {}

    def ints(lo, hi, shape):
        return rng.randint(lo, hi + 1, size=shape).astype(np.float32)

    def act(shape):
        return ints(-3, 3, shape) if exact else through(rng.randn(*shape), dtype)

    d["x0"] = act((case.n, case.hs, case.ws, c0))
    d["x1"] = act((case.n, case.hv, case.wv, c1)) if c1 else None
    k = case.kh * case.kw * ctot
    d["w"] = ints(-case.wr, case.wr, (case.co, case.kh, case.kw, ctot)) if exact else through(rng.randn(case.co, case.kh, case.kw, ctot) / np.sqrt(k), dtype)
    if exact and case.density < 1.0:
        d["w"] = (d["w"] * (rng.rand(*d["w"].shape) < case.density)).astype(np.float32)
    if fc:
        d["fold_src"] = act((case.n, case.hs, case.ws, fc))
        d["fold_w"] = ints(-case.wr, case.wr, (case.co, fc)) if exact else through(rng.randn(case.co, fc) / np.sqrt(fc), dtype)
    full = (case.n, case.ho, case.wo, case.co)
    d["bias"] = ints(-8, 8, (case.co,)) if exact else rng.randn(case.co).astype(np.float32)
    if exact:
        d["bias"][d["bias"] == 0] = 5.0      # no channel whose dropped bias would go unseen
    d["residual"] = ints(-3, 3, full) if exact else through(rng.randn(*full), dtype)
    d["prior"] = ints(-100, 100, full) if exact else through(rng.randn(*full), dtype)
    if any("bnb" in m for m in case.modes) or case.family == "refuse":
        if exact:
            d["bnb_x"] = ints(-3, 3, full)
            flat = d["bnb_x"].reshape(-1)
            flat[0::11], flat[1::11], flat[3::13], flat[5::17], flat[7] = -0.0, 0.0, 6.0, 7.0, TINY[dtype]
            d["bnb_gen"] = None
        else:
            d["bnb_x"] = through(rng.randn(*full) * 1.5 + 0.3, dtype)
            d["bnb_gen"] = bn_params(case.co, "gen", rng, d["bnb_x"])
    return d


def bnb_params_of(case, klass, dtype, params):
    return bn_params(case.co, params) if params in ("id", "aff") else inputs(case, klass, dtype)["bnb_gen"]


def device_weights(case, klass, dtype):
    """-> dict of the weight operands as the launch takes them (float32 numpy, rows padded to 16): weight, fold_weight; master = the fp32
    master [Cout][3][3][C0 + C1] stp_weight_prepare_upcollapse reads."""
    d = inputs(case, klass, dtype)
    return dict(weight=pad_rows16(d["w"]), fold_weight=pad_rows16(d["fold_w"]) if case.fold_c else None, master=d["w"] if case.upc else None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference of a launch

_CORE = {}


def core(case, klass, dtype, wup=None):
    """-> (value, abs, n) of the convolution sum before the epilogue, float64, on [N,Ho,Wo,Cout].  ``wup``: the class-collapsed copy as
    stp_weight_prepare_upcollapse wrote it (ROUNDED class of a launch that takes it: the kernel multiplies THOSE values; not cached)."""
    key = (case, klass, dtype)
    if wup is None and key in _CORE:
        return _CORE[key]
    d = inputs(case, klass, dtype)
    c0, c1, fc = dims(case, dtype)
    if wup is not None:
        out = conv_collapsed(d["x0"], d["x1"], wup, d["w"], c0)
    else:
        v = virtual_source(resample(d["x0"], case.mode), d["x1"])
        assert v.shape[1:3] == (case.hv, case.wv)
        live0 = None
        if case.mode == SRC_ZEROINS2X:
            live0 = np.zeros((case.hv, case.wv), bool)
            live0[::2, ::2] = True
        val, ab, nt = conv_general(v, d["w"], case.stride, case.pad, case.ho, case.wo, live0, c0)
        if fc:      # one more centre tap of parity class 0: the (even, even) pixels
            fs, fw = np.asarray(d["fold_src"], np.float64), np.asarray(d["fold_w"], np.float64)
            val, ab, nt = val.copy(), ab.copy(), np.array(nt)
            val[:, ::2, ::2] += fs @ fw.T
            ab[:, ::2, ::2] += np.abs(fs) @ np.abs(fw).T
            nt[:, ::2, ::2] += fc
        out = (val, ab, nt)
    if wup is None:
        _CORE[key] = out
    return out


def _dest(pre, ab, n, relu=False, on=None, near=None):
    return dict(pre=pre, abs=ab, n=n, relu=relu, on=on, near=near)


def launch_reference(case, mode, klass, dtype, wup=None):
    """-> dict(dst0=..., dst1=... or None, bnb=(x, mean, rstd) or None): per destination ``pre`` (the fp32 sum with the epilogue's additions,
    before ReLU / the mask), ``abs``, ``n``, ``relu``, ``on`` / ``near`` (mask).  The tables follow from the stored tensor: ``tables``."""
    o = options(case, mode)
    d = inputs(case, klass, dtype)
    val, ab, nt = core(case, klass, dtype, wup)
    pre, ab, nt = val.copy(), ab.copy(), np.array(nt, dtype=np.float64)
    # the order of the fp32 additions in epilogue_cf and in epilogue_rm_lin: ((sum + bias) + residual) + prior, then ReLU, then one rounding
    if o.bias:
        pre, ab, nt = pre + d["bias"].astype(np.float64), ab + np.abs(d["bias"]), nt + 1
    if o.residual:
        pre, ab, nt = pre + d["residual"], ab + np.abs(d["residual"]), nt + 1
    cd0 = min(o.cd0, case.co)
    acc = np.zeros(case.co, bool)
    acc[:cd0], acc[cd0:] = o.acc0, o.acc1
    pre, ab, nt = pre + np.where(acc, d["prior"], 0.0), ab + np.where(acc, np.abs(d["prior"]), 0.0), nt + acc
    out = dict(dst1=None, bnb=None)
    on = near = None
    if o.bnb is not None:
        m = bnb_params_of(case, klass, dtype, o.params)
        on, near = mask_of(d["bnb_x"], *m, o.bnb, klass == "exact")
        out["bnb"] = (d["bnb_x"], m[0], m[1])
    out["dst0"] = _dest(pre[..., :cd0], ab[..., :cd0], nt[..., :cd0], relu=o.relu, on=on, near=near)
    if cd0 < case.co:
        out["dst1"] = _dest(pre[..., cd0:], ab[..., cd0:], nt[..., cd0:], relu=o.relu)
    return out


def tile_columns(case, dtype, t):
    """[N,Ho,Wo,C] -> [C][pixel tiles]: sums over the tile_pixels(tile) consecutive LOGICAL pixels of every tile (the last may be short)."""
    P, tp = case.n * case.ho * case.wo, tile_pixels(case.tile)
    flat = np.asarray(t, np.float64).reshape(P, -1)
    order = pixel_order(case, dtype)
    if order is not None:
        flat = flat[order]
    cols = -(-P // tp)
    full = np.zeros((cols * tp, flat.shape[1]))
    full[:P] = flat
    return full.reshape(cols, tp, -1).sum(axis=1).T


def tables(case, mode, dtype, stored, bnb=None):
    """The statistic table of a launch from its STORED destination: -> dict(value, abs, n, slack), each [2][C][tiles] float64, column t =
    logical tile t.  value[0] = sum, value[1] = sum of squares, or with ``bnb`` = (x, mean, rstd) sum g * xhat.  ``abs`` / ``n`` bound the
    kernel's own fp32 arithmetic (rounded class); for sum g * xhat the row-major epilogue computes rstd * (sum g x - mean sum g) and the
    fragment-order one sum g * ((x - mean) * rstd): abs = rstd * (sum |g x| + |mean| sum |g|) bounds the terms of both, with three more
    roundings.  ``slack``: 2 |g| tiny in the column that holds the one smallest positive input."""
    s = np.asarray(stored, np.float64)
    sums = lambda t: tile_columns(case, dtype, t)
    npix = tile_pixels(case.tile)
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


def slot_sums(table, slots):
    """[2][C][tiles] -> [2][C][slots]: slot s holds the tiles t with t % slots == s (linear-tile assignment pix0 = tile_n * BN)."""
    out = np.zeros(table.shape[:-1] + (slots,))
    for t in range(table.shape[-1]):
        out[..., t % slots] += table[..., t]
    return out
