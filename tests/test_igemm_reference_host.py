"""Host checks of tests/_igemm_reference.py: the float64 restatement of what the per-tap convolution kernels compute
against float64 torch, the exactness condition of the EXACT class and the mask-edge cap of the ROUNDED class on the very inputs
tests/test_igemm_ops_gpu.py runs, and the plan facts each GPU case relies on, asked of the library built on this host."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _igemm_reference as R

F = torch.nn.functional


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 3, 1, 2)))


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def oihw(w):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(w, np.float64).transpose(0, 3, 1, 2)))


def close(a, b):
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def ident(c):
    return "%s-%s" % (c.family, c.name)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement against float64 torch

GEOMETRIES = [(1, 1, 1, 0), (3, 3, 1, 1), (3, 3, 2, 1), (4, 4, 2, 1), (7, 8, 2, 3)]      # kh, kw, stride, pad


@pytest.mark.parametrize("mode", [R.SRC_DIRECT, R.SRC_NEAREST2X, R.SRC_ZEROINS2X])
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("c1", [0, 3])
def test_index_formula_equals_conv2d_on_the_materialised_virtual_source(geom, mode, c1):
    kh, kw, s, p = geom
    rng = np.random.RandomState(3)
    n, hs, ws, c0, co = 2, 5, 6, 4, 7
    x0 = rng.randn(n, hs, ws, c0)
    v0 = R.resample(x0, mode)
    hv, wv = v0.shape[1:3]
    assert (hv, wv) == {R.SRC_DIRECT: (hs, ws), R.SRC_NEAREST2X: (2 * hs, 2 * ws), R.SRC_ZEROINS2X: (2 * hs - 1, 2 * ws - 1)}[mode]
    if mode == R.SRC_ZEROINS2X:
        assert np.array_equal(v0[:, ::2, ::2], x0) and not v0[:, 1::2].any() and not v0[:, :, 1::2].any()
    if mode == R.SRC_NEAREST2X:
        assert np.array_equal(v0[:, 3, 5], x0[:, 1, 2])
    v = R.virtual_source(v0, rng.randn(n, hv, wv, c1) if c1 else None)
    wt = rng.randn(co, kh, kw, c0 + c1)
    want = nhwc(F.conv2d(nchw(v), oihw(wt), stride=s, padding=p))
    ho, wo = want.shape[1:3]
    assert (ho, wo) == ((hv + 2 * p - kh) // s + 1, (wv + 2 * p - kw) // s + 1)
    live0 = None
    if mode == R.SRC_ZEROINS2X:
        live0 = np.zeros((hv, wv), bool)
        live0[::2, ::2] = True
    val, ab, nt = R.conv_general(v, wt, s, p, ho, wo, live0, c0)
    assert close(val, want)
    assert close(ab, nhwc(F.conv2d(nchw(np.abs(v)), oihw(np.abs(wt)), stride=s, padding=p)))
    exists = np.ones_like(v)
    if live0 is not None:
        exists[..., :c0] *= live0[None, :, :, None]
    ones = nhwc(F.conv2d(nchw(exists), oihw(np.ones_like(wt)), stride=s, padding=p))       # products that exist per element
    assert np.array_equal(nt, np.rint(ones).astype(np.int64))
    # an output grid larger than the formula's own (the data gradient onto an even map): the rows past it see fewer taps, never other ones
    val2, _, nt2 = R.conv_general(v, wt, s, p, ho + 1, wo + 1, live0, c0)
    big = nhwc(F.conv2d(nchw(np.pad(v, ((0, 0), (0, s), (0, s), (0, 0)))), oihw(wt), stride=s, padding=p))[:, :ho + 1, :wo + 1]
    assert close(val2, big) and close(val2[:, :ho, :wo], val)


@pytest.mark.parametrize("geom,shortcut", [((3, 1, 9, 11), False), ((3, 1, 8, 6), False), ((3, 1, 8, 6), True), ((1, 0, 8, 6), False)])
def test_zero_inserted_form_equals_the_autograd_data_gradient(geom, shortcut):
    """stp_conv2d over the zero-inserted dY with the flipped / transposed weight copy, pad k - 1 - p, == d/dx of conv k x k / stride 2 /
    pad p in float64 autograd, onto odd and even maps; with the 1x1 / stride-2 sibling as one more tap of the (even, even) pixels."""
    k, p, h, w = geom
    rng = np.random.RandomState(5)
    n, cdy, cin, cf = 2, 6, 4, 5
    hs, ws = (h + 2 * p - k) // 2 + 1, (w + 2 * p - k) // 2 + 1
    dy, dysc = rng.randn(n, hs, ws, cdy), rng.randn(n, hs, ws, cf)
    wf, wsc = rng.randn(cdy, k, k, cin), rng.randn(cf, cin)
    x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
    loss = (F.conv2d(x, oihw(wf), stride=2, padding=p) * nchw(dy)).sum()
    if shortcut:
        loss = loss + (F.conv2d(x, torch.from_numpy(wsc)[:, :, None, None], stride=2) * nchw(dysc)).sum()
    ref = nhwc(torch.autograd.grad(loss, x)[0])
    v = R.zero_insert(dy)
    live0 = np.zeros(v.shape[1:3], bool)
    live0[::2, ::2] = True
    val, ab, nt = R.conv_general(v, R.bwd_copy(wf), 1, k - 1 - p, h, w, live0)
    val = val.copy()
    if shortcut:
        val[:, ::2, ::2] += dysc @ wsc                   # fold_weight [Cout][fold_C] = wsc.T
    assert close(val, ref)
    # live taps per parity class: 1, 2, 2, 4 of nine; 1, 0, 0, 0 of one
    per = [int(nt[0, 2 + (c >> 1), 2 + (c & 1), 0]) // cdy for c in range(4)]
    assert per == ([1, 2, 2, 4] if k == 3 else [1, 0, 0, 0])


def test_collapsed_weights_equal_the_plain_3x3_over_the_materialised_upsampling():
    rng = np.random.RandomState(7)
    n, h2, w2, c0, c1, co = 2, 3, 4, 5, 3, 6
    lo, x1, w = rng.randn(n, h2, w2, c0), rng.randn(n, 2 * h2, 2 * w2, c1), rng.randn(co, 3, 3, c0 + c1)
    plain = R.conv_general(R.virtual_source(R.nearest2x(lo), x1), w, 1, 1, 2 * h2, 2 * w2)
    wup = R.collapse_weights(w, c0)
    assert wup.shape == (co, 4, 2, 2, c0) and np.allclose(wup[:, 3, 0, 0], w[:, 0, 0, :c0] + w[:, 0, 1, :c0] + w[:, 1, 0, :c0] + w[:, 1, 1, :c0])
    val, ab, nt = R.conv_collapsed(lo, x1, wup, w, c0)
    assert close(val, plain[0])
    assert close(val, nhwc(F.conv2d(nchw(R.virtual_source(R.nearest2x(lo), x1)), oihw(w), padding=1)))
    assert (ab >= np.abs(val) - 1e-12).all() and nt.max() == 4 * c0 + 9 * c1


def test_tile_tables_and_helpers():
    assert [R.tile_pixels(t) for t in (1, 5, 7, 66, 71, 103, 133, 134, 257, 260, 262)] == [128, 64, 128, 256, 128, 128, 64, 64, 128, 256, 64]
    assert [R.tile_bm(t) for t in (4, 71, 103, 134, 259)] == [16, 64, 64, 128, 32] and [R.ring_stages(t) for t in (69, 101, 133, 261)] == [2, 3, 4, 2]
    case = R.PARITY_CASES[0]
    order = R.pixel_order(case, "bf16")
    assert sorted(order) == list(range(256)) and order[0] == 0 and order[1] == 2 and order[64] == 1 and order[128] == 16 and order[192] == 17
    assert R.pixel_order(R.PARITY_MISSES[0], "bf16") is None and R.pixel_order(R.PARITY_MISSES[1], "fp32") is None
    assert R.pixel_order(R.UPC_CASES[0], "fp16") is not None and R.pixel_order(R.UPC_MISS, "bf16") is None
    t = np.arange(256.0).reshape(1, 16, 16, 1)
    cols = R.tile_columns(case, "bf16", t)
    assert cols.shape == (1, 4) and cols[0, 0] == t[0, ::2, ::2, 0].sum() and cols[0, 3] == t[0, 1::2, 1::2, 0].sum()
    assert np.array_equal(R.slot_sums(np.arange(5.0)[None, None, :], 4), [[[4, 1, 2, 3]]])
    o = R.options(case, "bnb2_aff_last_s4")
    assert (o.bnb, o.params, o.acc0, o.slots, o.stats) == (2, "aff", True, 4, True) and R.options(case, "two16").cd0 == 16


def test_the_named_paths_are_in_the_tables():
    """Tiles 7 / 71 / 103, nk in {0, 2, 3} on the deep rings, every id of launch_tile, the fold, every passes(...) copy."""
    ids = lambda cases: sorted({c.tile for c in cases})
    assert ids([c for c in R.GENERAL_CASES if c.co == 40]) == R.GENERAL_IDS and ids([c for c in R.UNIFORM_CASES if c.family == "uniform" and c.c1 == 0 and c.mode == 0]) == R.UNIFORM_IDS
    assert ids(R.PERLANE_CASES[:18]) == R.PERLANE_IDS and {c.c0 for c in R.PERLANE_CASES[:18]} == {8, 16, 32}
    for dtype in R.DTYPES:
        assert sorted((R.ring_stages(c.tile), R.k_tiles(c, dtype)) for c in R.RING_CASES) == sorted((s, k) for s in (2, 3, 4) for k in (1, 2, 3) for _ in (0, 1))
        assert {R.k_tiles(c, dtype) for c in R.UNIFORM_CASES if c.family == "uniform" and c.c1 == 0 and c.mode == 0} == {9}
        assert [R.k_tiles(c, dtype) for c in R.PERLANE_CASES[:3]] == [2, 3, 5]      # 8, 4, 2 taps per K-tile: the last tile partly past KH * KW
        assert R.live_k_tiles(R.PARITY_CASES[-2], dtype) == [1, 0, 0, 0] and R.live_k_tiles(R.PARITY_CASES[0], dtype) == [1, 2, 2, 4]
        assert [R.live_k_tiles(c, dtype) for c in R.FOLD_CASES] == [[2, 2, 2, 4]] * 3
        for c in R.PARITY_CASES + R.FOLD_CASES + R.UPC_CASES:
            assert R.parity_order(c, dtype), ident(c)
        for c in R.PARITY_MISSES + [R.UPC_MISS] + R.UNIFORM_CASES + R.GENERAL_CASES + R.PERLANE_CASES:
            assert not R.parity_order(c, dtype), ident(c)
    assert {7, 71, 103} <= {c.tile for c in R.all_cases()}
    assert [(c.n, c.co, c.fold_c) for c in R.FOLD_CASES] == [(1, 64, 64), (1, 128, 64), (2, 64, 64)]
    assert R.stats_tiles(R.SLOT_CASES[0]) == 2 and R.stats_tiles(R.SLOT_CASES[1]) == 70 and R.stats_tiles(R.GROUP_CASE) == 129
    assert len(R.REFUSALS) == 14


def test_every_epilogue_branch_has_a_mode():
    """The passes(...) dispatch of epilogue_rm_lin, restated: every one of its 13 specialised copies and the all-operands copy is named
    by a mode of the epilogue table, on a case that takes the row-major epilogue; the fragment-order epilogue gets the same table."""
    def copy_of(o):
        if o.bnb is not None:
            return ("bnb", o.acc0, o.bnb == 1)
        key = (o.bias, o.residual, o.acc0, o.relu)
        special = {(False, False, False, False): "plain", (False, True, False, False): "res", (False, False, True, False): "acc"}
        if o.stats:
            return ("stats", special.get(key, "all"))
        special.update({(True, False, False, False): "bias", (True, False, False, True): "bias_relu"})
        return ("none", special.get(key, "all"))
    for case in R.EP_CASES[1:]:
        for klass in ("exact", "rounded"):
            seen = {copy_of(R.options(case, m)) for m in R.modes_of(case, klass) if R.epilogue_is_row_major(case, m, "bf16")}
            assert seen == ({("bnb", a, r) for a in (False, True) for r in (False, True)} | {("stats", k) for k in ("plain", "res", "acc", "all")}
                            | {("none", k) for k in ("plain", "res", "acc", "bias", "bias_relu", "all")}), (ident(case), klass)
    for case in R.EP_CASES:
        for m in R.modes_of(case, "exact"):
            for dtype in R.DTYPES:
                rm = R.epilogue_is_row_major(case, m, dtype)
                assert rm == (dtype != "fp32" and case.tile >= 64 and m != "two4"), (ident(case), m, dtype)
                assert not R.epilogue_is_row_major(case, m, dtype, no_rm=True)
    for dtype in R.H16:
        assert all(R.epilogue_is_row_major(c, m, dtype) == (c.co != 20) for c in R.PARITY_CASES for m in R.modes_of(c, "exact"))
        assert not any(R.epilogue_is_row_major(c, m, dtype) for c in R.SLOT_CASES for m in R.modes_of(c, "exact"))      # slots: fragment order with PRE
        assert all(R.epilogue_is_row_major(c, m, dtype) for c in R.FOLD_CASES + R.UPC_CASES + [R.GROUP_CASE] for m in R.modes_of(c, "exact"))
        assert not any(R.epilogue_is_row_major(c, m, dtype) for c in R.GENERAL_CASES for m in R.modes_of(c, "exact"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the exactness condition and the mask-edge cap, on the inputs the GPU test runs

@pytest.mark.parametrize("case", R.all_cases(), ids=ident)
def test_exact_class_sums_are_exact_in_fp32(case):
    """Integers whose absolute terms sum below 2^24 per element, per statistic column and per bnb column: every partial sum of every
    order of additions is an integer below 2^24, hence exact in fp32; the operands are representable in every storage format, and
    every stored value stays below the largest IEEE half."""
    for dtype in case.builds:
        d = R.inputs(case, "exact", dtype)
        for key, a in d.items():
            if isinstance(a, np.ndarray):
                assert np.array_equal(R.through(a, dtype), a), key
        assert (d["bias"] != 0).all()      # a dropped bias shows on every channel
        if "bnb_x" in d:
            x = d["bnb_x"]
            assert np.signbit(x[x == 0]).any() and (x == 6).any() and (x == 7).any() and int((x == R.TINY[dtype]).sum()) == 1
        for key in ("x0", "x1", "w", "fold_src", "fold_w"):      # nothing but integers ever reaches an MFMA
            if d.get(key) is not None:
                assert np.array_equal(d[key], np.rint(d[key])), key
        if case.upc:
            wup = R.collapse_weights(d["w"], R.dims(case, dtype)[0])
            assert np.array_equal(R.through(wup, dtype), wup)      # integer masters: the collapsed sums are exact in storage
        for mode in R.modes_of(case, "exact"):
            o = R.options(case, mode)
            r = R.launch_reference(case, mode, "exact", dtype)
            stored = []
            for name in ("dst0", "dst1"):
                dst = r[name]
                if dst is None:
                    continue
                assert np.array_equal(dst["pre"], np.rint(dst["pre"])), (mode, name)
                assert float(dst["abs"].max()) < R.EXACT_LIMIT, (mode, name)
                assert dst["near"] is None or not dst["near"].any()
                s = R.through(R.stored_reference(dst), dtype)
                assert float(np.abs(s).max()) < 65504.0
                stored.append(s)
            if o.stats:
                t = R.tables(case, mode, dtype, np.concatenate(stored, axis=-1), r["bnb"])
                assert t["value"].size == R.stats_floats(case)
                assert float(t["abs"].max()) < R.EXACT_LIMIT, (mode, dtype, float(t["abs"].max()))
                assert int((t["slack"] > 0).sum()) <= 1 and not t["slack"][0].any()      # the one tiny input touches one bnb column
                if o.slots:      # a slot is an int64 sum of exact tile sums in 2^-24 units
                    assert float(R.slot_sums(t["abs"], o.slots).max()) * R.SLOT_SCALE < 2.0 ** 62


@pytest.mark.parametrize("case", [c for c in R.all_cases() if any("bnb" in m for m in c.modes)], ids=ident)
def test_rounded_class_mask_inputs_stay_under_the_edge_cap(case):
    for dtype in case.builds:
        d = R.inputs(case, "rounded", dtype)
        for mode in R.modes_of(case, "rounded"):
            o = R.options(case, mode)
            if o.bnb is None:
                continue
            on, near = R.mask_of(d["bnb_x"], *R.bnb_params_of(case, "rounded", dtype, o.params), o.bnb, False)
            assert float(near.mean()) <= R.MASK_SHARE_CAP, (mode, float(near.mean()))
            if o.bnb:
                assert 0.05 < float(on.mean()) < 0.95


# ---------------------------------------------------------------------------------------------------------------------------------
# plan facts, from the library built on this host

FAKE = 0x10000          # never read: the plan queries look at shapes and at which pointers are set
NAMES = "src0 src1 weight weight_up bias residual dst0 dst1 stats bnb_x bnb_mean bnb_rstd bnb_gamma bnb_beta fold_src fold_weight group_out counters pbn".split()
PTR = dict.fromkeys(NAMES, FAKE)


@pytest.fixture(scope="module")
def lib_of():
    from segmentation_training_pipeline_amd import _lib
    return lambda dtype: _lib.load("fp16" if dtype == "fp16" else "bf16")


def params(case, mode, dtype, **over):
    from segmentation_training_pipeline_amd import _lib
    return R.fill_params(_lib.ConvParams(), case, mode, dtype, PTR, **over)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_plan_facts_of_every_case(lib_of, dtype):
    lib = lib_of(dtype)
    for case in R.all_cases() + R.FORCED_DMA_REFUSED:
        if dtype not in case.builds:
            continue
        for klass in R.classes_of(case):
            for mode in R.modes_of(case, klass):
                P = params(case, mode, dtype)
                what = "%s %s %s" % (ident(case), mode, dtype)
                assert int(P.tile) == (0 if case.auto else case.tile)
                assert int(lib.stp_conv2d_tile_for(C.byref(P))) == case.tile, what      # (auto cases: the automatic choice is the id the case names)
                if R.options(case, mode).stats and not R.options(case, mode).slots:
                    assert int(lib.stp_conv2d_stats_floats(C.byref(P))) == R.stats_floats(case) == 2 * case.co * -(-(case.n * case.ho * case.wo) // R.tile_pixels(case.tile)), what
                assert int(lib.stp_conv2d_halo_variant(C.byref(P))) == -1 and int(lib.stp_conv2d_stats_group_for(C.byref(P))) == 0, what
                assert int(lib.stp_conv2d_fold_ok(C.byref(P))) == int(case.family == "fold"), what
        # what the ids rely on: fill_args' eligibility answer in this build
        if case in R.STEM_CASES:
            want = 3
        elif case.family == "forced":
            want = [0, 0, 1][R.FORCED_DMA_REFUSED.index(case)]
        elif case.family == "ep":
            want = {5: 0, 69: 1, 261: 2}[case.tile]
        else:
            want = {"general": None, "perlane": 2}.get(case.family, 1)      # (a forced general id runs whatever the channels admit)
        assert want is None or R.ut_ok(case, dtype) == want, ident(case)
    if dtype != "fp32":      # the 4-channel form has two instances: every other forced id answers tile 2
        for t in (1, 3, 4, 6, 7, 69, 261):
            P = params(R.STEM_CASES[0], "plain", dtype, tile=t)
            assert int(lib.stp_conv2d_tile_for(C.byref(P))) == 2
    for case in R.FOLD_CASES:      # the fold needs the automatic tile: forcing even the same id turns the query off
        assert int(lib.stp_conv2d_fold_ok(C.byref(params(case, "plain", dtype, tile=case.tile)))) == 0
    for case, mode, over, what in R.REFUSALS:
        if what in R.FOLD_REFUSED_BY_QUERY:
            assert int(lib.stp_conv2d_fold_ok(C.byref(params(case, mode, dtype, **over)))) == 0, what
    miss = R.REFUSALS[12][0]
    assert int(lib.stp_conv2d_tile_for(C.byref(params(miss, "plain", dtype)))) == 67 and (miss.ho * miss.wo // 4) % R.tile_pixels(67) != 0


PROBE = """
import ctypes as C, json, sys
sys.path.insert(0, %r)
import _igemm_reference as R
from segmentation_training_pipeline_amd import _lib
out = {}
for dtype in R.H16:
    lib = _lib.load(dtype)
    P = R.fill_params(_lib.ConvParams(), R.GROUP_CASE, "stats", dtype, dict.fromkeys(%r, 0x10000))
    G = int(lib.stp_conv2d_stats_group_for(C.byref(P)))
    out[dtype] = dict(G=G, counters=int(lib.stp_conv2d_stats_group_counters(C.byref(P), G)))
P = R.fill_params(_lib.ConvParams(), R.GROUP_CASE, "stats", "fp32", dict.fromkeys(%r, 0x10000))
out["fp32"] = dict(G=int(_lib.load("bf16").stp_conv2d_stats_group_for(C.byref(P))))
print("PROBE " + json.dumps(out))
"""


def test_group_size_in_a_process_with_the_switch_on():
    """STP_STATS_GROUP is read once per process: with it the 129-column case gets G = 2, 65 groups (the last one short) and one
    counter per 16 channels and group; the fp32 build has no row-major epilogue and hence no group form."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, STP_STATS_GROUP="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", PROBE % (os.path.join(root, "tests"), NAMES, NAMES)], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("PROBE ")][-1][6:])
    for dtype in R.H16:
        assert out[dtype] == dict(G=2, counters=4 * 65), out
    assert out["fp32"]["G"] == 0
