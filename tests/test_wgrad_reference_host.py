"""Host checks of tests/_wgrad_reference.py: the float64 restatement of the weight gradient against float64 torch
autograd, the exactness condition of the EXACT class on the very inputs tests/test_wgrad_ops_gpu.py runs, and the plan facts each GPU
case relies on, asked of the library built on this host (the compute-unit count answers 256 without a GPU, as on the MI355X)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _wgrad_reference as R


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement against the convolution's autograd weight gradient

def torch_wgrad(v, dy, KH, KW, stride, pad):
    """d(sum(conv(v, w) * dy)) / dw in float64; the window is anchored at -pad and the map is zero-padded as far as the taps reach."""
    N, Hv, Wv, Cc = v.shape
    _, Ho, Wo, Co = dy.shape
    x = torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2))).double()
    need_h, need_w = (Ho - 1) * stride + KH, (Wo - 1) * stride + KW
    x = torch.nn.functional.pad(x, (pad, max(need_w - Wv - pad, 0), pad, max(need_h - Hv - pad, 0)))[:, :, :need_h, :need_w]
    w = torch.zeros((Co, Cc, KH, KW), dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x, w, stride=stride)
    assert tuple(y.shape) == (N, Co, Ho, Wo)
    (y * torch.from_numpy(np.ascontiguousarray(dy.transpose(0, 3, 1, 2))).double()).sum().backward()
    return w.grad.permute(0, 2, 3, 1).numpy()


RESTATEMENT = {
    "3x3_s1_p1": dict(n=2, h=7, w=9, c0=5, c1=0, up=False, co=6, kh=3, kw=3, s=1, p=1, ho=7, wo=9),
    "3x3_s2_p1": dict(n=2, h=8, w=11, c0=4, c1=0, up=False, co=3, kh=3, kw=3, s=2, p=1, ho=4, wo=6),
    "1x1_s2_p0": dict(n=1, h=9, w=6, c0=7, c1=0, up=False, co=5, kh=1, kw=1, s=2, p=0, ho=5, wo=3),
    "7x8_s2_p3_c4": dict(n=2, h=13, w=15, c0=4, c1=0, up=False, co=8, kh=7, kw=8, s=2, p=3, ho=7, wo=8),
    "two_sources_up": dict(n=2, h=3, w=4, c0=5, c1=3, up=True, co=4, kh=3, kw=3, s=1, p=1, ho=6, wo=8),
}


@pytest.mark.parametrize("name", sorted(RESTATEMENT))
def test_restatement_equals_float64_autograd(name):
    g = RESTATEMENT[name]
    rng = np.random.RandomState(3)
    x0 = rng.randn(g["n"], g["h"], g["w"], g["c0"])
    H, W = (2 * g["h"], 2 * g["w"]) if g["up"] else (g["h"], g["w"])
    x1 = rng.randn(g["n"], H, W, g["c1"]) if g["c1"] else None
    dy = rng.randn(g["n"], g["ho"], g["wo"], g["co"])
    v = R.virtual_source(x0, x1, g["up"])
    assert v.shape == (g["n"], H, W, g["c0"] + g["c1"])
    prev = rng.randn(g["co"], g["kh"], g["kw"], g["c0"] + g["c1"])
    dw, ab, nt = R.wgrad(v, dy, g["kh"], g["kw"], g["s"], g["p"])
    ref = torch_wgrad(v, dy, g["kh"], g["kw"], g["s"], g["p"])
    assert np.abs(dw - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert np.abs(ab - torch_wgrad(np.abs(v), np.abs(dy), g["kh"], g["kw"], g["s"], g["p"])).max() <= 1e-12 * ab.max()
    ones = torch_wgrad(np.ones_like(v), np.ones_like(dy), g["kh"], g["kw"], g["s"], g["p"])       # in-bounds pixel products per element
    assert np.array_equal(nt, np.rint(ones).astype(np.int64)) and nt.min() >= 1 and nt.max() <= g["n"] * g["ho"] * g["wo"]
    assert np.array_equal(R.wgrad(v, dy, g["kh"], g["kw"], g["s"], g["p"], prev)[0], dw + prev)
    if name == "7x8_s2_p3_c4":      # the padded tap column kw = 7 is a real tap of the 7x8 window; the stem's gradient is the rest
        assert np.array_equal(R.unpad_stem(dw), R.wgrad(v[..., :3], dy, 7, 7, 2, 3)[0])


def test_storage_rounding_and_bound_helpers():
    rng = np.random.RandomState(5)
    a = np.concatenate([rng.randn(4096) * 10.0 ** rng.randint(-6, 4, 4096), [0.0, -0.0, 1.0, 1.00390625, 1.01171875, 65504.0]]).astype(np.float32)
    t = torch.from_numpy(a)
    assert np.array_equal(R.through(a, "bf16"), t.to(torch.bfloat16).float().numpy())
    assert np.array_equal(R.through(a, "fp16"), t.to(torch.float16).float().numpy())
    assert np.array_equal(R.through(a, "fp32"), a)
    assert R.rounding_bound(6, 8.0) == 8 * 2.0 ** -24 * 8.0
    assert R.rounding_bound(6, 8.0, prev=-2.0) == 9 * 2.0 ** -24 * 10.0
    x = np.array([-0.0, -1.0, 3.0, 6.0, 7.0])
    assert np.array_equal(R.bn_act(x, 0.0, 1.0, 1.0, 0.0, 0), x)
    assert np.array_equal(R.bn_act(x, 0.0, 1.0, 1.0, 0.0, 1), [0, 0, 3, 6, 7]) and np.array_equal(R.bn_act(x, 0.0, 1.0, 1.0, 0.0, 2), [0, 0, 3, 6, 6])


# ---------------------------------------------------------------------------------------------------------------------------------
# the exactness condition, on the inputs the GPU test runs

def every_exact_case():
    cases = list(R.all_single_cases())
    for group in sorted(R.GROUPS):
        cases += [R.group_case(group, i) for i in range(len(R.GROUPS[group]))]
        cases += [R.group_case(group, i, bn=1 + i % 2) for i in range(len(R.GROUPS[group])) if R.GROUPS[group][i][4] == 0]
    return cases + [R.lone_case(i) for i in range(len(R.LONE_LAYERS))]


@pytest.mark.parametrize("case", every_exact_case(), ids=lambda c: "%s-%s%s" % (c.family, c.name, "" if c.bn is None else "-bn%d" % c.bn))
def test_exact_class_sums_are_exact_in_fp32(case):
    """Integers whose absolute products (plus the prior dW where accumulated) sum below 2^24: every partial sum of every order of
    additions is an integer below 2^24, hence exact in fp32, and the operands are representable in bf16 and IEEE half."""
    d = R.exact_case(case)
    for dtype in R.DTYPES:
        for key in ("x0", "x1", "dy"):
            if d[key] is not None:
                assert np.array_equal(R.through(d[key], dtype), d[key])
    assert np.array_equal(d["dw"], np.rint(d["dw"])) and np.array_equal(d["dw_acc"], np.rint(d["dw_acc"]))
    worst = float((d["abs"] + np.abs(d["prev"])).max())
    assert worst < R.EXACT_LIMIT, worst
    assert int(d["nt"].max()) <= case.n * d["dy"].shape[1] * d["dy"].shape[2]
    if case.bn is not None:
        assert np.signbit(d["x0"]).any() and (d["x0"] == 6).any() and (d["x0"] == 7).any() and (d["x0"] == 0).any()
    if case is R.SC_MULTI_TRIP:
        assert d["dy"].shape[:3] == (2, 258, 500) and float(d["abs"].max()) <= 1.55e6
    if case.stem:
        assert (d["x0"][..., 3] == 1).all()


def test_case_tables_are_the_ones_of_the_existing_tests():
    import test_ops_gpu
    assert R.GROUPS == test_ops_gpu.WGRAD_GROUPS


# ---------------------------------------------------------------------------------------------------------------------------------
# plan facts, from the library built on this host

@pytest.fixture(scope="module")
def lib_of():
    from segmentation_training_pipeline_amd import _lib
    return lambda dtype: _lib.load("fp16" if dtype == "fp16" else "bf16")


def params(case, dtype):
    from segmentation_training_pipeline_amd import _lib
    fake = 0x10000          # never read: the plan queries look at shapes and at which pointers are set
    return R.fill_params(_lib.WgradParams(), case, dtype, fake, fake, fake, src1=fake if case.c1 else None,
                         bn=(fake, fake, fake, fake) if case.bn is not None else None)


def single_params():
    return [(c, dt) for c in R.all_single_cases() for dt in R.dtypes_of(c)]


@pytest.mark.parametrize("case,dtype", single_params(), ids=lambda v: v if isinstance(v, str) else "%s-%s" % (v.family, v.name))
def test_plan_facts_of_every_single_layer_case(lib_of, case, dtype):
    lib = lib_of(dtype)
    P = params(case, dtype)
    g = R.geometry(case)
    K = case.kh * case.kw * (case.c0 + case.c1)
    kid = int(lib.stp_conv2d_wgrad_kernel_id(C.byref(P)))
    assert kid == R.expected_kernel_id(case, dtype)
    assert bool(lib.stp_wgrad_sc_eligible(C.byref(P))) == R.sc_eligible(case, dtype)
    slabs = int(lib.stp_conv2d_wgrad_workspace_bytes(C.byref(P))) // (case.co * K * 4)
    assert slabs >= 1
    if case.family == "sc":
        assert kid == 1
        if not case.stem:
            # the workspace holds one slab per persistent workgroup (and at least as many as any GEMM plan of the shape needs), so
            # `slabs` bounds the small-channel kernel's workgroup count from above without naming the slab query itself
            tiles = R.sc_tiles(case)
            if case is R.SC_MULTI_TRIP:
                assert tiles == 1056 and slabs == (512 if dtype == "fp32" else 1024)     # fewer workgroups than tiles: a second trip
            else:
                assert slabs >= tiles                                                    # room for one tile per workgroup
    if case.family == "row":
        assert R.row_eligible(case, dtype)
        if case.name == "two_sources":      # decoder_stage3_conv1: the automatic choice is the small-channel kernel, variant 4 the row kernel
            assert kid == 1
        else:
            assert kid == (0 if case.splits else (3 if case.co <= 64 else 2))
    if case.family == "gemm":
        if case.name != "32row" and not R.row_eligible(case, dtype):
            assert kid == 0
        if case.splits >= 2:
            assert slabs >= 2, "the case is meant to split"
        if case.name == "two_m_tiles":
            # 198 pixels: 4 steps of 64 in 16 bit, 3 asked splits -> 2 steps each -> 2 slabs (rounded down); 7 steps of 32 in fp32 -> 3, 3, 1
            assert case.splits == 3 and slabs == (3 if dtype == "fp32" else 2)
        if case.name == "s2_one_slab":
            assert slabs == 1
        if case.name == "p35_16row":
            assert g["N"] * g["Ho"] * g["Wo"] == 35
        if case.name == "stem_odd":
            assert not R.sc_eligible(case, dtype) and (g["Ho"], g["Wo"]) == (17, 18)
    if case.name == "stem_lean":
        assert (g["Ho"], g["Wo"]) == (3, 3)


@pytest.mark.parametrize("dtype", R.H16)
@pytest.mark.parametrize("group", sorted(R.GROUPS))
def test_group_class_of_every_grouped_layer(lib_of, group, dtype):
    lib = lib_of(dtype)
    for i in range(len(R.GROUPS[group])):
        assert int(lib.stp_wgrad_group_class(C.byref(params(R.group_case(group, i), dtype)))) == R.GROUP_CLASS[group]
        if R.GROUPS[group][i][4] == 0:
            assert int(lib.stp_wgrad_group_class(C.byref(params(R.group_case(group, i, bn=1), dtype)))) == R.GROUP_CLASS[group]


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_lone_layers_keep_plain_slabs(lib_of, dtype):
    """The batched reduce takes a layer only when the automatic choice is the GEMM (plain [splits][Cout * K] slabs)."""
    lib = lib_of(dtype)
    for i in range(len(R.LONE_LAYERS)):
        assert int(lib.stp_conv2d_wgrad_kernel_id(C.byref(params(R.lone_case(i), dtype)))) == 0
