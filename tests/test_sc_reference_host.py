"""Host checks of tests/_sc_reference.py: the float64 restatement of what the small-channel and stem kernels compute
against float64 torch, the exactness condition of the EXACT class and the mask-edge cap of the ROUNDED class on the very inputs
tests/test_sc_ops_gpu.py runs, and the plan facts each GPU case relies on, asked of the library built on this host."""
import ctypes as C

import numpy as np
import pytest
import torch

import _sc_reference as R

F = torch.nn.functional


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).transpose(0, 3, 1, 2)))


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def close(a, b):
    return a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


def ident(c):
    return "%s-%s" % (c.kind, c.name)


def conv(v, w, stride=1, pad=1):
    return nhwc(F.conv2d(nchw(v), nchw(w), stride=stride, padding=pad))


def upsampled(x):
    return nhwc(F.interpolate(nchw(x), scale_factor=2, mode="nearest"))


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement against float64 torch

def check_core(dst, v, w, extra=0.0, extra_abs=0.0, extra_n=0, stride=1, pad=1, relu=False):
    """value, abs and n of a destination against conv2d of the operands, of their absolute values, and of ones."""
    want = conv(v, w, stride, pad) + extra
    assert close(dst["pre"], want)
    assert close(R.stored_reference(dst), np.maximum(want, 0.0) if relu else want)
    assert close(dst["abs"], conv(np.abs(v), np.abs(w), stride, pad) + extra_abs)
    assert np.array_equal(dst["n"], np.rint(conv(np.ones_like(v), np.ones_like(w), stride, pad)) + extra_n)


def test_direct_source_with_the_epilogue_operands():
    case, dt = R.MODE_CASES[0], "bf16"
    d = {k: (a.astype(np.float64) if isinstance(a, np.ndarray) else a) for k, a in R.inputs(case, "rounded", dt).items()}
    r = R.launch_reference(case, "bias_relu_acc", "rounded", dt)
    assert r["dst1"] is None and r["bnb"] is None
    check_core(r["dst0"], d["x0"], d["w"], d["bias"].astype(np.float64) + d["prior"], np.abs(d["bias"]) + np.abs(d["prior"]), 2, relu=True)
    check_core(R.launch_reference(case, "plain", "rounded", dt)["dst0"], d["x0"], d["w"])
    # fp32 runs half as many input channels
    assert R.inputs(case, "rounded", "fp32")["x0"].shape[-1] == case.cin // 2 and R.geometry(case, "plain", "fp32")["C0"] == case.cin // 2


def test_nearest2x_source_and_the_second_source():
    case = R.UP_CASES[0]
    d = R.inputs(case, "rounded", "fp16")
    assert d["x0"].shape[1:3] == (11, 34)
    check_core(R.launch_reference(case, "plain", "rounded", "fp16")["dst0"], upsampled(d["x0"]), d["w"])
    case = R.SCN_CASES[0]
    d = {k: (a.astype(np.float64) if isinstance(a, np.ndarray) else a) for k, a in R.inputs(case, "rounded", "bf16").items()}
    assert d["x0"].shape == (1, 11, 34, 64) and d["x1"].shape == (1, 22, 68, 64) and d["w"].shape == (32, 3, 3, 128)
    v = np.concatenate([upsampled(d["x0"]), d["x1"]], axis=-1)
    check_core(R.launch_reference(case, "bias", "rounded", "bf16")["dst0"], v, d["w"], d["bias"].astype(np.float64), np.abs(d["bias"]), 1)


def test_fused_producer_batchnorm_is_rounded_once_and_padded_afterwards():
    case, dt = R.MODE_CASES[0], "bf16"
    d = R.inputs(case, "rounded", dt)
    for mode in ("pbn0_gen", "pbn1_gen", "pbn2_gen"):
        mean, rstd, gamma, beta = [torch.from_numpy(a.astype(np.float64)) for a in R.pbn_params_of(case, mode, "rounded", dt)]
        y = (torch.from_numpy(d["x0"].astype(np.float64)) - mean) * rstd * gamma + beta
        relu = R.options(case, mode).pbn
        y = y if relu == 0 else y.clamp(min=0) if relu == 1 else y.clamp(0, 6)
        act = R.through(y.numpy(), dt)
        assert (act != y.numpy()).any()                     # the storage rounding is there
        assert beta.abs().min() > 0                         # normalised padding would not be zero: padding must come afterwards
        check_core(R.launch_reference(case, mode, "rounded", dt)["dst0"], act, d["w"])
        other = R.through(act * 0.5, dt)                    # the tensor stp_bn_apply wrote takes its place when given
        check_core(R.launch_reference(case, mode, "rounded", dt, act=other)["dst0"], other, d["w"])


def test_summed_destination_is_the_autograd_gradient_of_the_upsampling():
    case, dt = R.SUM_CASES[-3], "bf16"      # 1,2,6
    d = {k: (a.astype(np.float64) if isinstance(a, np.ndarray) else a) for k, a in R.inputs(case, "rounded", dt).items()}
    x = torch.zeros((1, case.cout, 1, 3), dtype=torch.float64, requires_grad=True)
    hi = conv(d["x0"], d["w"])
    (F.interpolate(x, scale_factor=2, mode="nearest") * nchw(hi)).sum().backward()
    r = R.launch_reference(case, "sum2_acc", "rounded", dt)["dst0"]
    assert close(r["pre"], nhwc(x.grad) + d["prior_low"])
    assert close(r["abs"], R.sum2x2(conv(np.abs(d["x0"]), np.abs(d["w"]))) + np.abs(d["prior_low"]))
    # n: all four pixels' products plus the three additions, plus the prior
    assert np.array_equal(r["n"], R.sum2x2(np.rint(conv(np.ones_like(d["x0"]), np.ones_like(d["w"])))) + 3 + 1)
    m = R.launch_reference(case, "sum2_bnb1_gen_first", "rounded", dt)
    x_bn, mean, rstd = m["bnb"]
    assert x_bn.shape == (1, 1, 3, case.cout) and m["dst0"]["on"].shape == x_bn.shape
    assert close(R.stored_reference(m["dst0"]), np.where(m["dst0"]["on"], nhwc(x.grad), 0.0))


def test_two_destinations_of_the_wide_form():
    case, dt = R.SCW_CASES[0], "fp16"      # 2,20,72, Cd0 = 32
    d = {k: (a.astype(np.float64) if isinstance(a, np.ndarray) else a) for k, a in R.inputs(case, "rounded", dt).items()}
    hi = conv(d["x0"], d["w"])
    r = R.launch_reference(case, "acc0_acc1", "rounded", dt)
    assert r["dst0"]["pre"].shape == (2, 10, 36, 32) and r["dst1"]["pre"].shape == (2, 20, 72, 96)
    assert close(r["dst0"]["pre"], R.sum2x2(hi[..., :32]) + d["prior_low"]) and close(r["dst1"]["pre"], hi[..., 32:] + d["prior"][..., 32:])
    ones = np.rint(conv(np.ones_like(d["x0"]), np.ones_like(d["w"])))
    assert np.array_equal(r["dst0"]["n"], R.sum2x2(ones[..., :32]) + 4) and np.array_equal(r["dst1"]["n"], ones[..., 32:] + 1)
    p = R.launch_reference(case, "plain", "rounded", dt)
    assert close(p["dst0"]["pre"], R.sum2x2(hi[..., :32])) and close(p["dst1"]["pre"], hi[..., 32:]) and p["bnb"] is None
    b = R.launch_reference(case, "bnb2_gen", "rounded", dt)
    assert b["dst0"]["on"].shape == (2, 10, 36, 32) and b["dst1"]["on"] is None and 0.05 < b["dst0"]["on"].mean() < 0.95


def test_stem_is_the_7x7_convolution_of_three_channels():
    case, dt = R.STEM_CASES[1], "bf16"
    d = R.inputs(case, "rounded", dt)
    assert d["x0"].shape == (2, 37, 140, 4) and d["w"].shape == (64, 7, 8, 4)
    assert np.abs(d["x0"][..., 3]).min() > 0 and not d["w"][:, :, 7].any() and not d["w"][..., 3].any()      # data against zero weights
    r = R.launch_reference(case, "plain", "rounded", dt)["dst0"]
    want = conv(d["x0"][..., :3], d["w"][:, :, :7, :3], 2, 3)
    assert want.shape == (2, 19, 70, 64) and close(r["pre"], want)
    assert close(r["abs"], conv(np.abs(d["x0"][..., :3]), np.abs(d["w"][:, :, :7, :3]), 2, 3))
    # n counts the products the 7x8x4 geometry has, zero weights or not
    pad = np.pad(np.ones_like(d["x0"]), ((0, 0), (3, 4), (3, 4), (0, 0)))
    pad[:, :3], pad[:, -4:], pad[:, :, :3], pad[:, :, -4:] = 0, 0, 0, 0
    assert np.array_equal(r["n"], np.rint(conv(pad, np.ones_like(d["w"]), 2, 0))[:, :19, :70])


def test_table_totals_and_the_mode_grammar():
    rng = np.random.RandomState(1)
    s, x = rng.randn(2, 3, 5, 4), rng.randn(2, 3, 5, 4)
    mean, rstd = rng.randn(4), rng.rand(4) + 0.5
    t = R.totals(s)
    assert close(t["value"][0], s.sum((0, 1, 2))) and close(t["value"][1], (s * s).sum((0, 1, 2))) and (t["n"] == 30).all()
    t = R.totals(s, (x, mean, rstd))
    assert close(t["value"][1], (s * (x - mean) * rstd).sum((0, 1, 2))) and (t["n"][1] == 33).all() and not t["slack"].any()
    assert (t["abs"][1] >= np.abs(t["value"][1])).all()
    o = R.options(R.MODE_CASES[0], "bnb1_aff_last_s4")
    assert (o.bnb, o.params, o.acc0, o.slots, o.stats, o.sum2) == (1, "aff", True, 4, True, False)
    o = R.options(R.SCW_CASES[0], "bnb1_id_acc0")
    assert (o.bnb, o.acc0, o.acc1, o.sum2, o.stats) == (1, True, False, True, True)
    assert R.options(R.MODE_CASES[0], "pbn1_gen_stats").pbn == 1 and not R.options(R.MODE_CASES[0], "pbn1_gen").stats
    assert R.modes_of(R.MODE_CASES[0], "exact").count("bnb1_id_last_s4") == 1 and "bnb2_gen_first" in R.modes_of(R.MODE_CASES[0], "rounded")


def test_the_named_cases_are_in_the_tables():
    sc = [c for c in R.all_cases() if c.kind == "sc"]
    assert {(c.n, c.h, c.w) for c in R.SHAPE_CASES + R.MODE_CASES} == set(R.SHAPES)
    assert {c.cin for c in R.MODE_CASES} == {8, 16, 32} and {c.cout for c in sc} == {1, 3, 5, 8, 16, 24, 32}
    for ci in (8, 16, 32):      # every mode for every cin
        assert {m for c in R.MODE_CASES if c.cin == ci for m in c.modes} == set(R.MODES + R.HEAD_MODES)
        assert {m for c in R.SUM_CASES if c.cin == ci for m in c.modes} == set(R.SUM_MODES) and any(c.cin == ci for c in R.UP_CASES)
    assert {(c.n, c.h, c.w) for c in R.SUM_CASES} == {(1, 2, 6), (1, 22, 68), (2, 20, 46)}
    assert [R.tiles_of(c) for c in R.SHAPE_CASES[::7]] == [1, 1, 4, 12] and R.tiles_of(R.MODE_CASES[0]) == 9
    assert sorted({c.cd0 for c in R.SCW_CASES}) == [32, 64, 96] and {(c.n, c.h, c.w) for c in R.SCW_CASES} == {(2, 20, 72), (1, 22, 68)}
    assert [R.tiles_of(c) for c in R.STEM_CASES] == [4, 18, 4] and [R.tiles_of(c) for c in R.SCN_CASES] == [9, 12]
    assert [R.tiles_of(c) for c in R.TRIP_CASES] == [1050, 1050, 1050, 1050, 1050, 525, 270, 525] and 1050 & 7 == 2
    assert len(R.REFUSALS) == 13


# ---------------------------------------------------------------------------------------------------------------------------------
# the exactness condition and the mask-edge cap, on the inputs the GPU test runs

@pytest.mark.parametrize("case", R.all_cases(), ids=ident)
def test_exact_class_sums_are_exact_in_fp32(case):
    """Per element the absolute terms sum below 2^24 and every reference value is an integer the storage type holds exactly; per channel,
    over the WHOLE tensor, sum |stored|, sum stored^2, sum |g| and sum |g x| + |mean| sum |g| stay below 2^24 - whole-tensor totals bound
    every partial sum, whatever the tile-to-workgroup map, so any order of fp32 additions is exact."""
    for dtype in R.builds_of(case):
        d = R.inputs(case, "exact", dtype)
        for key, a in d.items():
            if isinstance(a, np.ndarray):
                assert np.array_equal(R.through(a, dtype), a), key
        assert (d["bias"] != 0).all()
        for key in ("bnb_x", "bnb_x_low"):
            if key in d:
                x = d[key]
                assert np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any() and (x == 6).any() and (x == 7).any()
                assert int((x == R.TINY[dtype]).sum()) == 1
        for key in ("x0", "x1", "w"):      # nothing but integers ever reaches an MFMA
            if d.get(key) is not None:
                assert np.array_equal(d[key], np.rint(d[key])), key
        assert float(np.abs(d["w"]).sum(axis=(1, 2, 3)).min()) > 0      # no output channel without a weight
        for mode in R.modes_of(case, "exact"):
            o = R.options(case, mode)
            r = R.launch_reference(case, mode, "exact", dtype)
            stored = None
            for name in ("dst0", "dst1"):
                dst = r[name]
                if dst is None:
                    continue
                assert float(dst["abs"].max()) < R.EXACT_LIMIT, (mode, name)
                assert dst["near"] is None or not dst["near"].any()
                ref = R.stored_reference(dst)
                assert np.array_equal(ref, np.rint(ref)) and np.array_equal(dst["pre"], np.rint(dst["pre"])), (mode, name)
                assert np.array_equal(R.through(ref, dtype), ref), (mode, name, dtype, float(np.abs(ref).max()))
                stored = ref if stored is None else stored
            if o.stats:
                t = R.totals(stored, r["bnb"])
                assert t["value"].shape == (2, R.stat_channels(case))
                assert float(t["abs"].max()) < R.EXACT_LIMIT, (mode, dtype, float(t["abs"].max()))
                assert int((t["slack"] > 0).sum()) <= 1 and not t["slack"][0].any()      # the one tiny input touches one bnb channel
                if o.slots:
                    assert float(t["abs"].max()) * R.SLOT_SCALE < 2.0 ** 62


@pytest.mark.parametrize("case", [c for c in R.all_cases() if not c.exact_only and any("bnb" in m for m in c.modes)], ids=ident)
def test_rounded_class_mask_inputs_stay_under_the_edge_cap(case):
    for dtype in R.builds_of(case):
        for mode in R.modes_of(case, "rounded"):
            o = R.options(case, mode)
            if o.bnb is None:
                continue
            dst = R.launch_reference(case, mode, "rounded", dtype)["dst0"]
            assert float(dst["near"].mean()) <= R.MASK_SHARE_CAP, (mode, float(dst["near"].mean()))
            if o.bnb:
                assert 0.05 < float(dst["on"].mean()) < 0.95


# ---------------------------------------------------------------------------------------------------------------------------------
# plan facts, from the library built on this host

FAKE = 0x10000          # never read: the plan queries look at shapes and at which pointers are set
NAMES = "src0 src1 weight bias dst0 dst1 stats bnb_x bnb_mean bnb_rstd bnb_gamma bnb_beta pbn_mean pbn_rstd pbn_gamma pbn_beta".split()
PTR = dict.fromkeys(NAMES, FAKE)
WORKGROUPS = {("sc", 16, 16): 1024, ("sc", 16, 32): 512, ("sc", 32, 16): 768, ("sc", 8, 16): 768, "scw": 512, "scn": 256, "stem": 512}


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
    for case in R.all_cases():
        if dtype not in R.builds_of(case):
            continue
        for klass in R.classes_of(case):
            for mode in R.modes_of(case, klass):
                P = params(case, mode, dtype)
                what = "%s %s %s" % (ident(case), mode, dtype)
                assert int(P.tile) == 0 and int(lib.stp_conv2d_tile_for(C.byref(P))) == R.TILE[case.kind], what
                for kind, query in R.ELIGIBLE.items():      # the ids are tried in this order: an earlier kernel must decline
                    assert bool(getattr(lib, query)(C.byref(P))) == (kind == case.kind), (what, query)
                o = R.options(case, mode)
                if o.stats and not o.slots:
                    floats = int(lib.stp_conv2d_stats_floats(C.byref(P)))
                    cols = int(getattr(lib, "stp_conv2d_%s_stats_tiles" % case.kind)(C.byref(P)))
                    assert floats == 2 * R.stat_channels(case) * cols and 1 <= cols <= R.tiles_of(case), what
                    if case.exact_only:      # the trip loop: fewer workgroups than tiles
                        key = (case.kind, R.cin_of(case, dtype), case.cout) if case.kind == "sc" else case.kind
                        assert cols == WORKGROUPS[key] < R.tiles_of(case), what
                    elif R.tiles_of(case) <= 256:
                        assert cols == R.tiles_of(case), what


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_fp32_serves_id_512_only_and_refusals_answer_their_queries(lib_of, dtype):
    lib = lib_of(dtype)
    for case, mode, over, what, eligible in R.REFUSALS:
        if dtype not in case.builds:
            continue
        P = params(case, mode, dtype, **over)
        assert bool(getattr(lib, R.ELIGIBLE[case.kind])(C.byref(P))) == bool(eligible), what
        if eligible:      # the kernel is chosen; its launch function refuses the combination
            assert int(lib.stp_conv2d_tile_for(C.byref(P))) == R.TILE[case.kind], what
        else:             # (stp_conv2d_tile_for echoes a forced id the generic path would be asked for: the eligibility query is the answer)
            assert int(P.tile) == R.TILE[case.kind], what
    if dtype == "fp32":
        for case in (R.SCW_CASES[0], R.SCN_CASES[0], R.STEM_CASES[0]):
            assert not getattr(lib, R.ELIGIBLE[case.kind])(C.byref(params(case, "plain", "fp32")))
        for cin in (8, 16, 32):      # 4, 8, 16 input channels in fp32
            assert lib.stp_conv2d_sc_eligible(C.byref(params(R.sc(1, 21, 67, cin, 16, ["plain"]), "plain", "fp32")))
