"""Float64 numpy restatement of what stp_conv2d computes on the small-channel tiles - id 512 (csrc/conv_sc.hip, conv_sc_lean.hip), 640
(conv_sc_wide.hip), 704 (conv_sc_narrow.hip) and 768 (conv_sc_stem.hip, the persistent stem kernel of conv_sc_lean.hip) - shared by
tests/test_sc_reference_host.py and tests/test_sc_ops_gpu.py.  Not collected, calls no kernel, no torch, no oracle/: it is written from
the comments of include/stp_hip.h on stp_conv_params, never from a kernel's loop,

    V[n,h,w,c]        = concat_c(src0 or nearest2x(src0), src1)                                     (taps outside V contribute nothing)
    out[n,y,x,co]     = sum_{kh,kw,c} V[n, y * stride - pad + kh, x * stride - pad + kw, c] * weight[co][kh][kw][c]
                        (3x3 / stride 1 / pad 1; the stem: 7x8 / stride 2 / pad 3 over 4 stored channels)
    src_bn_*          : V = act(fma(src0, rstd * gamma, beta - mean * rstd * gamma)) rounded ONCE to storage; the padding pads THAT tensor
    epilogue          : (out + bias) + prior (accumulate), ReLU, ONE rounding to storage (the order of ScEpilogue::finish and DESIGN.md 3.33)
    dst_sum2x2        : dst0 [N,Ho/2,Wo/2,Cd0] = the four pixels' fp32 sums added BEFORE the one rounding, then + prior; with a second
                        destination (id 640) only the first Cd0 channels are summed, the rest stay at full resolution
    bnb_*             : g = dY where the activation of the forward's single fma(bnb_x, rstd * gamma, beta - mean * rstd * gamma) passes the
                        gradient (0: everywhere, 1: > 0, 2: strictly inside (0, 6)); tables: sum g and sum g * xhat over the STORED g
    stats_partial     : [2][C][columns]; the header says only "one column per tile, or one per persistent workgroup" - NOT which tiles a
                        workgroup owns - so a table is known here by its per-channel TOTALS only (``totals``)
    stats_slots       : int64 slots [2][C][slots] in 2^-24 units; known by the per-channel sum of the slots

Every result comes with ``abs`` and ``n`` per element as DESIGN.md 3.32 defines them; for a 2 x 2-summed element both run over all four
pixels' products plus the three additions.  ``rounding_bound`` of tests/_halo_reference.py makes the bound of ANY order of fp32 additions
from them.  The case tables live here, so the host test asserts the exactness condition and the plan facts on exactly the inputs and
shapes the GPU test runs.

EXACT operands (the ranges the host test proves sufficient): x in +-2 (+-1 in the trip-loop cases), weights in +-1 with about
``WEIGHT_TERMS`` non-zero taps per output channel (so a sum of four pixels plus a prior stays an integer a bf16 holds: |value| <= 256),
bias in +-8 (+-2 in the trip-loop cases) without zero, priors in +-50, mask inputs in +-3 with -0.0, 0, 6, 7 and one smallest positive storage value planted.
"""
import collections
import functools
import zlib

import numpy as np

import _halo_reference as H
from _halo_reference import (EXACT_LIMIT, MASK_SHARE_CAP, TINY as TINY16, bn_act, bwd_copy, conv_taps, mask_of, pad_rows16, rounding_bound,  # noqa: F401
                             sum2x2, through, virtual_source)
from _igemm_reference import SLOT_SCALE, conv_general

DTYPES = ["fp32", "bf16", "fp16"]
H16 = H.H16
DT_CODE = H.DT_CODE
BADARG = H.BADARG
TINY = dict(TINY16, fp32=2.0 ** -149)      # the smallest positive value of the storage format
SRC_DIRECT, SRC_NEAREST2X = 0, 1
TILE = {"sc": 512, "scw": 640, "scn": 704, "stem": 768}
ELIGIBLE = {"sc": "stp_conv2d_sc_eligible", "scw": "stp_conv2d_scw_eligible", "scn": "stp_conv2d_scn_eligible", "stem": "stp_conv2d_stem_eligible"}
TH, TW = 8, 32                              # every kernel here owns 8 x 32 output pixels per tile
WEIGHT_TERMS = 24.0                         # EXACT class: expected number of (input, tap) pairs of an output channel that may hold a weight

# ---------------------------------------------------------------------------------------------------------------------------------
# cases.  n, h, w = the virtual grid (= the output grid; the stem: the INPUT map).  cin as given for 16-bit storage, halved in fp32 (id 512
# only: 8, 16, 32 -> 4, 8, 16).  xr: EXACT x in +-xr.

Case = collections.namedtuple("Case", "name kind n h w cin cout up cd0 modes builds xr exact_only")


def _c(kind, n, h, w, cin, cout, modes, up=False, cd0=None, builds=None, xr=2, exact_only=False):
    builds = tuple(builds or (DTYPES if kind == "sc" else H16))
    name = "%d_%d_%d_%d%s_%d%s" % (n, h, w, cin, "up" if up and kind == "sc" else "", cout, "_d%d" % cd0 if cd0 else "")
    return Case(name, kind, n, h, w, cin, cout, up, cd0, tuple(modes), builds, xr, exact_only)


def sc(n, h, w, cin, cout, modes, **kw):
    return _c("sc", n, h, w, cin, cout, modes, **kw)


def tiles_of(case):
    ho, wo = out_hw(case)
    return case.n * -(-ho // TH) * -(-wo // TW)


def out_hw(case):
    return ((case.h - 1) // 2 + 1, (case.w - 1) // 2 + 1) if case.kind == "stem" else (case.h, case.w)


def cin_of(case, dtype):
    return case.cin // 2 if (case.kind == "sc" and dtype == "fp32") else case.cin


PS = ["plain", "stats"]
_PAIRS = [(8, 16), (16, 32), (32, 8), (16, 24), (32, 1), (8, 3), (16, 5)]      # every cin and every cout of the issue once per shape
SHAPES = [(1, 3, 5), (1, 8, 32), (1, 9, 33), (2, 19, 45), (1, 21, 67)]         # 1 partial / 1 full / 2 x 2 with one-pixel edges / ragged / 3 x 3 tiles
SHAPE_CASES = [sc(n, h, w, ci, co, PS if co % 4 == 0 else ["plain"]) for (n, h, w) in SHAPES[:4] for (ci, co) in _PAIRS]

BNB_FIRST = ["bnb%d_P_first" % r for r in (0, 1, 2)]
BNB_LAST = ["bnb%d_P_last" % r for r in (0, 1, 2)]
PBN = ["pbn%d_P" % r for r in (0, 1, 2)] + ["pbn1_P_stats"]
EPILOGUE = ["plain", "bias", "bias_relu", "acc", "bias_relu_acc"]
SLOTS = ["stats_s1", "stats_s4", "stats_s64", "bnb1_P_last_s4"]
MODES = EPILOGUE + ["stats", "stats_bias"] + SLOTS + BNB_FIRST + BNB_LAST + PBN
SUM_MODES = ["sum2", "sum2_acc", "sum2_bnb1_P_first", "sum2_bnb1_P_last"]
UP_MODES = ["plain", "stats", "pbn1_P_stats", "acc"]            # the issue's up, up_stats, up_pbn1_stats, up_acc: ``up`` is the case's source mode
HEAD_MODES = ["plain", "bias", "pbn1_P_bias"]
CINS = (8, 16, 32)
# every mode on the 3 x 3-tile shape for every cin: Cout 16 and 32 (the lean kernel where it serves), 8 / 24 (generic, vector path), 3 / 5
# (generic, scalar tail), 1 (head)
MODE_CASES = ([sc(1, 21, 67, ci, co, MODES) for ci in CINS for co in (16, 32)] +
              [sc(1, 21, 67, ci, co, MODES) for ci, co in ((8, 24), (16, 8), (32, 24))] +
              [sc(1, 21, 67, ci, co, EPILOGUE) for ci, co in ((8, 3), (16, 5), (32, 3))] +
              [sc(1, 21, 67, ci, 1, HEAD_MODES) for ci in CINS])
SUM_CASES = ([sc(1, 22, 68, ci, co, SUM_MODES) for ci in CINS for co in (16, 32)] + [sc(1, 22, 68, 16, 24, SUM_MODES)] +
             [sc(1, 2, 6, 8, 16, SUM_MODES), sc(2, 20, 46, 32, 32, SUM_MODES), sc(2, 20, 46, 16, 8, SUM_MODES)])
UP_CASES = [sc(1, 22, 68, ci, co, UP_MODES, up=True) for ci, co in ((8, 16), (16, 32), (32, 16), (16, 24))]

# second and third trip of the tile loop: EXACT class only, thinned operands (x in +-1)
TRIP_MODES = ["stats", "bnb1_P_first"]
# (stats_bias on the first: with a bias the 16-bit builds take the GENERIC streaming kernel, whose carried sums the lean kernel would
#  otherwise hide from every 16-bit trip case - the hand-made fault in them was seen by the fp32 build alone)
TRIP_SC = [sc(1, 277, 948, ci, co, TRIP_MODES + (["stats_bias"] if (ci, co) == (16, 16) else []), xr=1, exact_only=True)
           for ci, co in ((16, 16), (16, 32), (32, 16))]                                                              # 35 x 30 = 1050 tiles, 1050 & 7 = 2
TRIP_SC_SUM = sc(1, 278, 948, 16, 32, ["sum2_bnb1_P_first"], xr=1, exact_only=True)
TRIP_SC_UP = sc(1, 278, 948, 16, 16, ["stats"], up=True, xr=1, exact_only=True)                                     # from low resolution 1,139,474
TRIP_BUILDS = {TRIP_SC[0]: DTYPES, TRIP_SC[1]: H16, TRIP_SC[2]: H16, TRIP_SC_SUM: H16, TRIP_SC_UP: H16}              # fp32: 8 -> 16 on 1,277,948

SCW_MODES = ["plain", "acc0", "acc1", "acc0_acc1", "bnb0_P", "bnb1_P", "bnb2_P", "bnb1_P_acc0"]
SCW_CASES = [_c("scw", n, h, w, 32, 128, SCW_MODES, cd0=cd0) for cd0 in (32, 64, 96) for (n, h, w) in ((2, 20, 72), (1, 22, 68))]
TRIP_SCW = _c("scw", 1, 274, 470, 32, 128, ["bnb1_P"], cd0=64, xr=1, exact_only=True)                                # 35 x 15 = 525 tiles > 512

SCN_MODES = ["plain", "bias", "bias_relu_acc", "stats", "stats_bias"]
SCN_CASES = [_c("scn", 1, 22, 68, 128, 32, SCN_MODES, up=True), _c("scn", 2, 20, 46, 128, 32, SCN_MODES, up=True)]      # low resolution 1,11,34 and 2,10,23
TRIP_SCN = _c("scn", 1, 142, 470, 128, 32, ["stats"], up=True, xr=1, exact_only=True)                                # 18 x 15 = 270 tiles > 256

STEM_CASES = [_c("stem", 1, 17, 66, 4, 64, PS), _c("stem", 2, 37, 140, 4, 64, PS), _c("stem", 1, 19, 67, 4, 64, PS)]      # the last: odd width, the single-shot kernel
TRIP_STEM = _c("stem", 1, 548, 940, 4, 64, ["stats"], xr=1, exact_only=True)                                        # output 274 x 470: 525 tiles > 512

TRIP_CASES = TRIP_SC + [TRIP_SC_SUM, TRIP_SC_UP, TRIP_SCW, TRIP_SCN, TRIP_STEM]
SWITCH_CASES = MODE_CASES + SUM_CASES[:7] + UP_CASES + STEM_CASES      # what STP_SC_LEAN=0, STP_SC_STREAM=0 and STP_STEM_LEAN=0 rerun (EXACT class)


def all_cases():
    return SHAPE_CASES + MODE_CASES + SUM_CASES + UP_CASES + SCW_CASES + SCN_CASES + STEM_CASES + TRIP_CASES


def builds_of(case):
    return tuple(TRIP_BUILDS.get(case, case.builds))


def classes_of(case):
    return ["exact"] if case.exact_only else ["exact", "rounded"]


Opt = collections.namedtuple("Opt", "bias relu acc0 acc1 stats slots bnb pbn params sum2")


def options(case, mode):
    """What a mode string switches on: tokens plain bias relu acc|acc0 acc1 stats s<slots> bnb<relu> pbn<relu> id|aff|gen first|last sum2
    (last = the accumulating consumer: accumulate0)."""
    parts = mode.split("_")
    bnb = pbn = params = None
    slots = 0
    for t in parts:
        if t.startswith("bnb"):
            bnb = int(t[3:])
        elif t.startswith("pbn"):
            pbn = int(t[3:])
        elif t in ("id", "aff", "gen"):
            params = t
        elif t[0] == "s" and t[1:].isdigit():
            slots = int(t[1:])
    return Opt(bias="bias" in parts, relu="relu" in parts, acc0="acc" in parts or "acc0" in parts or "last" in parts, acc1="acc1" in parts,
               stats=("stats" in parts or bnb is not None) and "nostats" not in parts, slots=slots, bnb=bnb, pbn=pbn, params=params,
               sum2="sum2" in parts or case.kind == "scw")


def modes_of(case, klass):
    out = []
    for m in case.modes:
        if "_P" in m:
            out += [m.replace("_P", "_%s" % p, 1) for p in (("id", "aff") if klass == "exact" else ("gen",))]
        else:
            out.append(m)
    return out


def stat_channels(case):
    return case.cd0 if case.kind == "scw" else case.cout


def geometry(case, mode, dtype):
    o = options(case, mode)
    ho, wo = out_hw(case)
    hs, ws = (case.h // 2, case.w // 2) if case.up else (case.h, case.w)
    g = dict(N=case.n, Hs0=hs, Ws0=ws, Hv=case.h, Wv=case.w, C0=cin_of(case, dtype), C1=0, src0_mode=SRC_NEAREST2X if case.up else SRC_DIRECT, KH=3, KW=3,
             stride=1, pad=1, Ho=ho, Wo=wo, Cout=case.cout, Cd0=case.cd0 or case.cout, tile=0, dst_sum2x2=int(o.sum2))
    if case.kind == "scn":
        g.update(C0=64, C1=64)
    if case.kind == "stem":
        g.update(KH=7, KW=8, stride=2, pad=3)
    return g


def fill_params(P, case, mode, dtype, ptr, **over):
    """Fills a segmentation_training_pipeline_amd._lib.ConvParams; ``ptr`` = name -> device address (any non-zero integer on a host
    without a GPU: the plan queries read no memory).  Names: src0 src1 weight bias dst0 dst1 stats bnb_x bnb_mean bnb_rstd bnb_gamma bnb_beta
    pbn_mean pbn_rstd pbn_gamma pbn_beta.  ``over``: fields set afterwards (pointer fields: a name of ``ptr`` or None)."""
    o = options(case, mode)
    for k, val in geometry(case, mode, dtype).items():
        setattr(P, k, val)
    P.src0, P.weight, P.dst0 = ptr["src0"], ptr["weight"], ptr["dst0"]
    P.src1 = ptr["src1"] if case.kind == "scn" else None
    P.dst1 = ptr["dst1"] if case.kind == "scw" else None
    P.bias = ptr["bias"] if o.bias else None
    P.accumulate0, P.accumulate1, P.relu, P.dtype = int(o.acc0), int(o.acc1), int(o.relu), DT_CODE[dtype]
    P.stats_partial = ptr["stats"] if o.stats else None
    P.stats_slots = o.slots
    if o.bnb is not None:
        P.bnb_x, P.bnb_mean, P.bnb_rstd, P.bnb_gamma, P.bnb_beta, P.bnb_relu = ptr["bnb_x"], ptr["bnb_mean"], ptr["bnb_rstd"], ptr["bnb_gamma"], ptr["bnb_beta"], o.bnb
    if o.pbn is not None:
        P.src_bn_mean, P.src_bn_rstd, P.src_bn_gamma, P.src_bn_beta, P.src_bn_relu = ptr["pbn_mean"], ptr["pbn_rstd"], ptr["pbn_gamma"], ptr["pbn_beta"], o.pbn
    for k, val in over.items():
        setattr(P, k, ptr[val] if isinstance(val, str) else val)
    return P


# refusals: (case, mode, overrides, what, eligible).  ``eligible``: what the kernel's own eligibility query answers - 1 where only the
# launch (stp_conv2d) looks at the combination, 0 where the id is forced on a shape its query rejects.
_R = sc(1, 22, 68, 16, 16, ["plain"])
REFUSALS = [
    (_R, "bnb1_id_first", dict(stats_partial=None), "bnb_x without stats_partial", 1),
    (sc(1, 22, 68, 16, 5, ["plain"]), "stats", {}, "stats_partial with Cout % 4 != 0", 1),
    (_R, "stats", dict(stats_slots=3), "stats_slots = 3", 1),
    (_R, "stats", dict(stats_slots=128), "stats_slots = 128", 1),
    (sc(1, 21, 68, 16, 16, ["plain"]), "sum2", {}, "dst_sum2x2 with odd Ho", 1),
    (_R, "sum2_bias", {}, "dst_sum2x2 with bias", 1),
    (_R, "sum2_stats", {}, "dst_sum2x2 with stats_partial but no bnb_x", 1),
    (_R, "pbn1_id", dict(src_bn_rstd=None), "src_bn_mean without src_bn_rstd", 1),
    (SCW_CASES[0], "stats", {}, "scw with stats_partial but no bnb_x", 1),
    (_c("sc", 1, 22, 68, 128, 16, ["plain"], builds=H16), "plain", dict(tile=512), "id 512 forced on 64 input channels", 0),
    (_c("scw", 1, 22, 68, 32, 128, ["plain"], cd0=48), "plain", dict(tile=640), "id 640 forced on Cd0 = 48", 0),
    (SCN_CASES[0], "plain", dict(tile=704, dst_sum2x2=1), "id 704 forced with dst_sum2x2", 0),
    (STEM_CASES[0], "plain", dict(tile=768, relu=1), "id 768 forced with relu", 0),
]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs

def _rng(case, salt):
    return np.random.RandomState(zlib.crc32(("%s/%s/%s" % (case.kind, case.name, salt)).encode()) & 0x7FFFFFFF)


def weight_shape(case, dtype):
    if case.kind == "stem":
        return (64, 7, 8, 4)
    return (case.cout, 3, 3, cin_of(case, dtype))


def low_shape(case):
    return (case.n, case.h // 2, case.w // 2, stat_channels(case))


@functools.lru_cache(maxsize=None)
def inputs(case, klass, dtype):
    """Every operand a launch of ``case`` may take (the modes pick among them); the fp32 build has its own (half as many channels).
    EXACT: the integers of the module docstring.  ROUNDED: normal values rounded to storage first.  The stem: the fourth input channel
    and the eighth tap column carry non-zero DATA against zero WEIGHTS."""
    rng = _rng(case, klass + "/" + (dtype if (klass != "exact" or dtype == "fp32") else "any"))
    exact = klass == "exact"
    cin = cin_of(case, dtype)
    ho, wo = out_hw(case)
    hs, ws = (case.h // 2, case.w // 2) if case.up else (case.h, case.w)
    d = {}

    def ints(lo, hi, shape):
        return rng.randint(lo, hi + 1, size=shape).astype(np.float32)

    def act(shape, scale=1.0, shift=0.0):
        return ints(-case.xr, case.xr, shape) if exact else through(rng.randn(*shape) * scale + shift, dtype)

    c0 = 64 if case.kind == "scn" else cin
    d["x0"] = act((case.n, hs, ws, c0))
    d["x1"] = act((case.n, case.h, case.w, 64)) if case.kind == "scn" else None
    ws_ = weight_shape(case, dtype)
    k = int(np.prod(ws_[1:]))
    if exact:
        d["w"] = (ints(-1, 1, ws_) * (rng.rand(*ws_) < min(1.0, WEIGHT_TERMS / k))).astype(np.float32)
    else:
        d["w"] = through(rng.randn(*ws_) / np.sqrt(k), dtype)
    if case.kind == "stem":
        d["w"][:, :, 7, :] = 0.0
        d["w"][..., 3] = 0.0
    full = (case.n, ho, wo, case.cout)
    br = 8 if case.xr > 1 else 2      # (trip-loop cases: bias^2 over a quarter of a million pixels must stay below 2^24 as well)
    d["bias"] = ints(-br, br, (case.cout,)) if exact else rng.randn(case.cout).astype(np.float32)
    if exact:
        d["bias"][d["bias"] == 0] = 5.0 if br == 8 else 1.0      # no channel whose dropped bias would go unseen
    d["prior"] = ints(-50, 50, full) if exact else through(rng.randn(*full), dtype)
    wants = lambda tok: any(tok in m for m in case.modes)
    if wants("sum2") or case.kind == "scw":
        d["prior_low"] = ints(-50, 50, low_shape(case)) if exact else through(rng.randn(*low_shape(case)), dtype)
    if wants("bnb"):
        for key, shape in (("bnb_x", full), ("bnb_x_low", low_shape(case))):
            if (key == "bnb_x_low") != (wants("sum2") or case.kind == "scw"):
                continue
            d[key] = H._mask_edges(ints(-3, 3, shape), dtype, False) if exact else through(rng.randn(*shape) * 1.5 + 0.3, dtype)
            if exact:
                d[key].reshape(-1)[7] = TINY[dtype]
            d[key + "_gen"] = None if exact else H.bn_params(shape[-1], "gen", rng, d[key])
    if wants("pbn"):
        if exact:
            d["x0"] = H._mask_edges(ints(-case.xr, case.xr, d["x0"].shape), dtype, False)      # (the tiny value: under the affine instance only, ``pbn_source``)
        else:
            d["x0"] = through(rng.randn(*d["x0"].shape) * 2.0 + 0.5, dtype)
        d["pbn_gen"] = None if exact else H.bn_params(cin, "gen", rng, d["x0"])
    return d


def pbn_source(case, klass, dtype, params):
    """src0 of a fused-producer launch: the EXACT inputs, with the smallest positive storage value planted under the affine instance only
    (fma(tiny, 2, 1) = 1 in fp32 and in float64 alike; under the identity a denormal product would reach the MFMA - DESIGN.md 3.32)."""
    x = inputs(case, klass, dtype)["x0"]
    if klass == "exact" and params == "aff":
        x = x.copy()
        x.reshape(-1)[7] = TINY[dtype]
    return x


def bnb_key(case, mode):
    return "bnb_x_low" if options(case, mode).sum2 else "bnb_x"


def bnb_params_of(case, mode, klass, dtype):
    o = options(case, mode)
    d = inputs(case, klass, dtype)
    key = bnb_key(case, mode)
    return H.bn_params(d[key].shape[-1], o.params) if o.params in ("id", "aff") else d[key + "_gen"]


def pbn_params_of(case, mode, klass, dtype):
    o = options(case, mode)
    return H.bn_params(cin_of(case, dtype), o.params) if o.params in ("id", "aff") else inputs(case, klass, dtype)["pbn_gen"]


def device_weight(case, klass, dtype):
    """The weight operand as the launch takes it: rows padded to a multiple of 16 with zero rows."""
    return pad_rows16(inputs(case, klass, dtype)["w"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference of a launch

_CORE = {}


def core(case, klass, dtype, pbn_key=None, act=None):
    """-> (value, abs, n) of the convolution sum before the epilogue, float64, on [N,Ho,Wo,Cout].  ``act`` = the normalised src0 as
    stp_bn_apply wrote it (ROUNDED class with a fused producer BatchNormalization; not cached)."""
    key = (case, klass, dtype if (klass != "exact" or dtype == "fp32" or pbn_key is not None) else "any", pbn_key)      # (EXACT: the 16-bit builds share their operands)
    if act is None and key in _CORE:
        return _CORE[key]
    d = inputs(case, klass, dtype)
    if case.kind == "stem":
        out = conv_general(d["x0"], d["w"], 2, 3, *out_hw(case))
    else:
        x0 = d["x0"]
        if pbn_key is not None:
            relu, params, mode = pbn_key
            # EXACT: the one fma is exact in fp32 (integers; 1 + 2^-23.. where the tiny value meets the affine instance), so float64 followed
            # by the ONE rounding to storage is what the kernel holds in LDS
            x0 = act if act is not None else through(bn_act(pbn_source(case, klass, dtype, params), *pbn_params_of(case, mode, klass, dtype), relu), dtype)
        out = conv_taps(virtual_source(x0, d["x1"], case.up), d["w"], 1)
    out = tuple(np.array(t) for t in out)
    if act is None:
        if case.exact_only:
            _CORE.clear()      # the trip-loop tensors are large: one at a time
        _CORE[key] = out
    return out


def _dest(pre, ab, n, relu=False, on=None, near=None):
    return dict(pre=pre, abs=ab, n=n, relu=relu, on=on, near=near)


stored_reference = H.stored_reference
stored_bounds = H.stored_bounds


def launch_reference(case, mode, klass, dtype, act=None):
    """-> dict(dst0=..., dst1=... or None, bnb=(x, mean, rstd) or None): per destination ``pre`` (the fp32 sum with the epilogue's additions,
    before ReLU / the mask), ``abs``, ``n``, ``relu``, ``on`` / ``near`` (mask).  The tables follow from the stored tensor: ``totals``."""
    o = options(case, mode)
    d = inputs(case, klass, dtype)
    pk = (o.pbn, o.params, mode) if o.pbn is not None else None
    val, ab, nt = core(case, klass, dtype, pk, act)
    pre, ab, nt = val.copy(), ab.copy(), np.array(nt, dtype=np.float64)
    if o.bias:
        pre, ab, nt = pre + d["bias"].astype(np.float64), ab + np.abs(d["bias"]), nt + 1
    out = dict(dst1=None, bnb=None)
    on = near = None
    if o.bnb is not None:
        x = d[bnb_key(case, mode)]
        m = bnb_params_of(case, mode, klass, dtype)
        on, near = mask_of(x, *m, o.bnb, klass == "exact")
        out["bnb"] = (x, m[0], m[1])
    if o.sum2:      # the four pixels' sums added before the one rounding (three more additions), then + prior
        cd0 = stat_channels(case)
        p0, a0, n0 = sum2x2(pre[..., :cd0]), sum2x2(ab[..., :cd0]), sum2x2(nt[..., :cd0]) + 3
        if o.acc0:
            p0, a0, n0 = p0 + d["prior_low"], a0 + np.abs(d["prior_low"]), n0 + 1
        out["dst0"] = _dest(p0, a0, n0, on=on, near=near)
        if cd0 < case.cout:
            p1, a1, n1 = pre[..., cd0:], ab[..., cd0:], nt[..., cd0:]
            if o.acc1:
                pr = d["prior"][..., cd0:]
                p1, a1, n1 = p1 + pr, a1 + np.abs(pr), n1 + 1
            out["dst1"] = _dest(p1, a1, n1)
        return out
    if o.acc0:
        pre, ab, nt = pre + d["prior"], ab + np.abs(d["prior"]), nt + 1
    out["dst0"] = _dest(pre, ab, nt, relu=o.relu, on=on, near=near)
    return out


def totals(stored, bnb=None):
    """Per-channel totals of a statistic table from the STORED destination [.., C]: -> dict(value, abs, n, slack), each [2][C] float64.
    value[0] = sum, value[1] = sum of squares, or with ``bnb`` = (x, mean, rstd) sum g * xhat.  ``abs`` / ``n`` bound the kernels' own fp32
    arithmetic (rounded class) with the number of summed terms as n; sum g * xhat is computed as rstd * (sum g x - mean sum g) by the lean
    kernel and as sum g * ((x - mean) * rstd) by the generic one: abs = rstd * (sum |g x| + |mean| sum |g|) bounds the terms of both, with
    three more roundings.  ``slack``: 2 |g| tiny in the channel that holds the one smallest positive input (g * tiny is no integer: each
    fp32 addition keeps or drops it)."""
    s = np.asarray(stored, np.float64)
    c = s.shape[-1]
    s = s.reshape(-1, c)
    npix = s.shape[0]
    v0, a0 = s.sum(0), np.abs(s).sum(0)
    slack = np.zeros((2, c))
    if bnb is None:
        v1 = a1 = (s * s).sum(0)
        n1 = npix
    else:
        x, mean, rstd = (np.asarray(t, np.float64) for t in bnb)
        x = x.reshape(-1, c)
        v1 = (s * ((x - mean) * rstd)).sum(0)
        a1 = (np.abs(s * x).sum(0) + np.abs(s).sum(0) * np.abs(mean)) * np.abs(rstd)
        n1 = npix + 3
        tiny = (x > 0) & (x < 2.0 ** -20)
        slack[1] = 2.0 * (np.abs(s) * np.where(tiny, x, 0.0)).sum(0) * np.abs(rstd)
    return dict(value=np.stack([v0, v1]), abs=np.stack([a0, a1]), n=np.stack([np.full(c, npix), np.full(c, n1)]), slack=slack)
