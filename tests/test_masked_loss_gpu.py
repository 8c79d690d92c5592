"""ignore_label / class_weights of the softmax heads, on the GPU: the loss kernel stp_softmax_loss_masked against the float64
evaluation of tests/_masked_loss_reference.py (the definitions of include/stp_hip.h), against its sibling stp_softmax_loss_ex where the
two must agree (compaction, the degenerate case), the confusion kernel stp_class_confusion_ignore against a numpy count, one training
step against the oracle fed the same definitions, and a YAML experiment end to end.  Tolerances are those of
tests/test_softmax_losses_gpu.py."""
import csv
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _masked_loss_reference as R  # noqa: E402
from oracle import nets as onets  # noqa: E402
from oracle import optim as ooptim  # noqa: E402
from oracle import step as ostep  # noqa: E402
from test_softmax_losses_gpu import TD, WEIGHTS, dt_code, label_discs, lib_for, make_case, ordered_bits, quantise, rel_l2  # noqa: E402
from test_softmax_losses_gpu import run_loss as run_loss_ex  # noqa: E402

STP_E_BADARG, STP_E_WORKSPACE = -1, -3
CLASSES = [2, 4, 5, 8, 9, 16, 17, 20, 24, 25, 32]          # both edges of every class bucket (4, 8, 16, 24, 32); 20: 8-byte rows
BIG = 4096 * 256 + 300                                     # just past the gradient pass's grid cap (4096 workgroups of 256)
SIZES = [1, 255, 256, 257, 3 * 1024 + 5]
REL = {"fp32": 1e-5, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}


def pad8(C):
    return (C // 8 + 1) * 8          # the next multiple of 8: 16-byte rows in every storage type


def pad4(C):
    """The first multiple of 4 past C that is no multiple of 8: 8-byte rows of the 16-bit types, 16-byte rows of fp32."""
    p = (C // 4 + 1) * 4
    return p if p % 8 else p + 4


def spread(C):
    return [float(w) for w in np.geomspace(0.25, 4.0, C)]


def ignore_pattern(t, pattern, C, seed):
    """-> (stored targets, ignore_label or None)."""
    t = t.copy()
    rng = np.random.RandomState(seed + 1000)
    if pattern == "none":
        return t, None
    if pattern == "none255":                     # a label is named, no pixel carries it
        return t, 255
    if pattern == "all":
        t[:] = 255
    elif pattern == "wave":                      # the first 64 pixels: a whole wave of the first workgroup
        t[:64] = 255
    elif pattern == "alternate":
        t[::2] = 255
    elif pattern == "random":
        t[rng.rand(t.size) < 0.3] = 255
    elif pattern == "label0":                    # the ignore label lies inside the class range: class 0 is the void
        return t, 0
    else:
        raise ValueError(pattern)
    return t, 255


def run_masked(dtype, z, t, classes, ldc, dlc, weights, ignore_label=None, class_weights=None, grad_scale=1.0, with_grad=True, guard=64):
    """-> (scalars[16], dlogits [P, dlc] float32 or None, the gradient in its storage type); the gradient buffer is filled with NaN and
    ``guard`` elements past its end must stay NaN."""
    lib, _lib = lib_for(dtype)
    P = z.shape[0]
    zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint8)).cuda()
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    dl = torch.full((P * dlc + guard,), float("nan"), dtype=TD[dtype], device="cuda") if with_grad else None
    cw = torch.tensor(class_weights, dtype=torch.float32, device="cuda") if class_weights is not None else None
    w5 = (ctypes.c_float * 5)(*weights)
    rc = lib.stp_softmax_loss_masked(zd.data_ptr(), td.data_ptr(), P, classes, ldc, dt_code(_lib, dtype), w5, sc.data_ptr(),
                                     dl.data_ptr() if dl is not None else None, dlc, grad_scale, ws.data_ptr(), ws.numel() * 4,
                                     -1 if ignore_label is None else ignore_label, cw.data_ptr() if cw is not None else None,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    g, raw = None, None
    if dl is not None:
        full = dl.to(torch.float32).cpu().numpy()
        assert np.isnan(full[P * dlc:]).all(), "the gradient pass wrote past its tensor"
        g = full[:P * dlc].reshape(P, dlc)
        raw = dl[:P * dlc].cpu()
    return sc.cpu().numpy(), g, raw


def edge_elements(pd):
    """Elements whose float64 probability lies within float32 rounding of a 1e-7 clip bound (tests/test_softmax_losses_gpu.py)."""
    return (np.abs(pd - 1e-7) < 1e-13) | (np.abs(pd - (1.0 - 1e-7)) < 1.2e-7)


_REF = {}


def reference(dtype, P, C, ldc, seed, pattern, weights_kind, mix):
    """(z, stored t, ignore_label, class weights, float64 reference) of a case, computed once and shared; never modified."""
    key = (dtype, P, C, ldc, seed, pattern, weights_kind, mix)
    if key not in _REF:
        z, t = make_case(P, C, ldc, seed)
        t, ign = ignore_pattern(t, pattern, C, seed)
        cw = {"null": None, "ones": [1.0] * C, "spread": spread(C)}[weights_kind]
        ref = R.reference(quantise(z, dtype)[:, :C], t, WEIGHTS[mix], ign, cw)
        for a in ref:
            a.setflags(write=False)
        _REF[key] = (z, t, ign, cw, ref)
    return _REF[key]


def compare(dtype, C, sc, g, ref, gref, pd, on, grad_scale, what=""):
    """The scalars and the gradient of a launch against a reference (scalars [>= 12], dL/dz [P, C], float64 probabilities, counted
    mask) at the project's tolerances."""
    n = int(on.sum())
    near = int((np.abs(pd[on] - 0.5) < 1e-5).sum())
    flip = (2 + near) * 2.0 / (2.0 * n + 1.0)
    for i, name in enumerate(R.NAMES[:len(ref)]):
        tol = 1e-5 * max(1.0, abs(ref[i]))
        if name in ("dice", "iot"):
            tol += flip
        elif name == "acc":
            tol += (2 + near) / float(max(n, 1) * C)
        print("%s %s C=%d %-9s got %.9g ref %.9g tol %.3g" % (what, dtype, C, name, sc[i], ref[i], tol))
        assert abs(sc[i] - ref[i]) <= tol, (name, sc[i], ref[i])
    if g is None:
        return
    gs = gref * grad_scale
    scale = np.abs(gs).max() + 1e-30
    err = np.abs(g[:, :C] - gs)
    edge = edge_elements(pd) & on[:, None]
    ok = err <= REL[dtype] * np.abs(gs) + 2e-5 * scale
    print("   gradient: max err / scale %.3g, edge elements %d" % ((err / scale).max(), edge.sum()))
    assert (ok | edge).all(), (err[~(ok | edge)].max(), scale)
    assert edge.sum() <= max(8, 1e-5 * edge.size), edge.sum()
    assert (g[:, C:] == 0).all(), "padding channels must be exactly zero"
    assert (g[~on] == 0).all(), "the rows of ignored pixels must be exactly zero"


def check(dtype, P, C, ldc, dlc, mix, pattern, weights_kind, seed):
    z, t, ign, cw, (ref, gref, pd, on) = reference(dtype, P, C, ldc, seed, pattern, weights_kind, mix)
    gsc = 1024.0 if dtype == "fp16" else 1.0                      # (IEEE half: the loss scale keeps 1/(P*C) gradients normal)
    sc, g, _raw = run_masked(dtype, z, t, C, ldc, dlc, WEIGHTS[mix], ign, cw, gsc)
    what = "P=%d ldc=%d %s %s %s" % (P, ldc, mix, pattern, weights_kind)
    compare(dtype, C, sc, g, ref, gref, pd, on, gsc, what)
    assert sc[12] == float(on.sum()), "slot 12 is the number of counted pixels"
    assert np.isfinite(sc).all() and np.isfinite(g).all()
    if not on.any():          # nothing counted: the means are 0, the overlap terms take their smooth-term values, no gradient
        assert (sc[[0, 1, 2, 4, 5, 6, 7, 10, 11, 12, 13]] == 0).all() and sc[3] == 1 and sc[8] == 1 and sc[9] == 1 and (g == 0).all()
    return sc, g


PATTERNS = ["none", "none255", "all", "wave", "alternate", "random", "label0"]
KINDS = ["null", "ones", "spread"]
MIXES = sorted(WEIGHTS)


def grid_case(C, P):
    """The pattern, weights and loss mix of a (classes, pixels) cell: the grid is walked diagonally, not run whole at every size."""
    k = CLASSES.index(C) * len(SIZES) + SIZES.index(P)
    return PATTERNS[k % len(PATTERNS)], KINDS[(k // 2) % len(KINDS)], ("cce", "cce+dice", "all")[k % 3]


def reference_cases():
    """(classes, pixels, seed) of every case whose gradient is compared under the clip-edge exemption
    (tests/test_masked_loss_host.py confirms that the reference alone has no edge element on them)."""
    out = [(C, P, C * 31 + P) for C in CLASSES for P in SIZES]
    out += [(C, P, C * 31 + P + 1) for C in CLASSES for P in SIZES[-1:]]
    out += [(C, 3077, 7 * C + 1) for C in (3, 20)] + [(5, 3077, 50 + i) for i in range(len(MIXES))] + [(3, BIG, 11)]
    out += [(C, 3077, 100 + C) for C in (3, 20, 5)] + [(C, 20000, C) for C in (3, 4, 5, 20, 32)]      # compaction, the degenerate case
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", CLASSES)
def test_masked_loss_matches_reference(dtype, C):
    for P in SIZES:
        pattern, kind, mix = grid_case(C, P)
        check(dtype, P, C, pad8(C), pad8(C), mix, pattern, kind, seed=C * 31 + P)
    # 8-byte rows of the 16-bit types and a gradient tensor without padding (stores element by element)
    pattern, kind, mix = grid_case(C, SIZES[-1])
    check(dtype, SIZES[-1], C, pad4(C), C, "all", "random", kind, seed=C * 31 + SIZES[-1] + 1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_ignore_pattern_with_every_kind_of_weights(dtype, C, pattern):
    for kind in KINDS:
        # C + 3 (odd strides: rows read element by element) at 3 classes, 16-byte rows at 20
        check(dtype, 3077, C, C + 3 if C == 3 else 24, pad8(C), "all", pattern, kind, seed=7 * C + 1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("mix", MIXES)
def test_every_loss_mix(dtype, mix):
    check(dtype, 3077, 5, 8, 8, mix, "random", "spread", seed=50 + MIXES.index(mix))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_past_the_gradient_grid_cap(dtype):
    """4096 * 256 + 300 pixels: the gradient pass strides its grid, the value pass walks a range per workgroup."""
    check(dtype, BIG, 3, 8 if dtype == "bf16" else 4, 8 if dtype == "bf16" else 4, "all", "random", "spread", seed=11)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C,ldc,dlc", [(3, 8, 8), (20, 24, 24), (5, 5, 5)])
def test_compaction(dtype, C, ldc, dlc):
    """The masked loss on P rows of which k are ignored is stp_softmax_loss_ex on the P - k counted rows; gradient rows by position."""
    P = 3077
    gsc = 1024.0 if dtype == "fp16" else 1.0
    z, t = make_case(P, C, ldc, 100 + C)
    t, ign = ignore_pattern(t, "random", C, 100 + C)
    on = t != ign
    for mix in ("cce+dice", "all"):
        sc, g, _ = run_masked(dtype, z, t, C, ldc, dlc, WEIGHTS[mix], ign, None, gsc)
        s_ex, g_ex, _ = run_loss_ex(dtype, z[on], t[on], C, ldc, dlc, WEIGHTS[mix], gsc)
        pd = torch.softmax(torch.from_numpy(quantise(z, dtype)[:, :C].astype(np.float64)), dim=-1).numpy()
        gref = np.zeros((P, C))
        gref[on] = g_ex[:, :C] / gsc
        compare(dtype, C, sc, g, s_ex[:12].astype(np.float64), gref, pd, on, gsc, "compaction " + mix)
        assert sc[12] == on.sum() == sc[13]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C,ldc,dlc", [(3, 3, 8), (4, 4, 4), (5, 8, 8), (20, 20, 24), (32, 32, 32)])
def test_degenerate_case_is_stp_softmax_loss_ex(dtype, C, ldc, dlc):
    """No ignore label and weights of one (or none): the sibling's scalars and gradient on the same buffers."""
    gsc = 1024.0 if dtype == "fp16" else 1.0
    P = 20000
    z, t = make_case(P, C, ldc, C)
    pd = torch.softmax(torch.from_numpy(quantise(z, dtype)[:, :C].astype(np.float64)), dim=-1).numpy()
    on = np.ones(P, bool)
    for mix in ("cce+dice", "all"):
        s_ex, g_ex, raw_ex = run_loss_ex(dtype, z, t, C, ldc, dlc, WEIGHTS[mix], gsc)
        for cw in (None, [1.0] * C):
            sc, g, raw = run_masked(dtype, z, t, C, ldc, dlc, WEIGHTS[mix], None, cw, gsc)
            compare(dtype, C, sc, g, s_ex[:12].astype(np.float64), g_ex[:, :C] / gsc, pd, on, gsc, "degenerate " + mix)
            assert sc[12] == P == sc[13]
            d = np.abs(ordered_bits(raw) - ordered_bits(raw_ex))
            print(dtype, C, mix, "scalars equal:", np.array_equal(sc[:12], s_ex[:12]), "gradient: max ulp distance", d.max())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_launches_are_bit_identical_and_grad_scale_is_linear(dtype):
    z, t = make_case(40000, 5, 8, 5)
    t, ign = ignore_pattern(t, "random", 5, 5)
    s1, g1, _ = run_masked(dtype, z, t, 5, 8, 8, WEIGHTS["all"], ign, spread(5))
    s2, g2, _ = run_masked(dtype, z, t, 5, 8, 8, WEIGHTS["all"], ign, spread(5))
    assert np.array_equal(s1, s2) and np.array_equal(g1, g2)              # deterministic two-stage reduction, no atomics
    s3, g3, _ = run_masked(dtype, z, t, 5, 8, 8, WEIGHTS["all"], ign, spread(5), 256.0)
    assert np.array_equal(s1, s3)                                           # the scalars do not carry the scale
    np.testing.assert_allclose(g3, 256.0 * g1, rtol=1e-6, atol=0)


def test_ignored_rows_may_hold_anything():
    """The mask is a select: NaN and infinite logits in ignored rows reach neither the scalars nor the gradient."""
    z, t = make_case(3077, 4, 8, 3)
    t, ign = ignore_pattern(t, "random", 4, 3)
    clean_s, clean_g, _ = run_masked("fp32", z, t, 4, 8, 8, WEIGHTS["all"], ign, spread(4))
    z = z.copy()
    bad = np.nonzero(t == ign)[0]
    z[bad[0::3], 0], z[bad[1::3], 1], z[bad[2::3], 2] = np.nan, np.inf, -np.inf
    s, g, _ = run_masked("fp32", z, t, 4, 8, 8, WEIGHTS["all"], ign, spread(4))
    assert np.array_equal(s, clean_s) and np.array_equal(g, clean_g)


def test_without_gradient_and_bad_arguments():
    lib, _lib = lib_for("fp32")
    z, t = make_case(1000, 4, 4, 1)
    t, ign = ignore_pattern(t, "alternate", 4, 1)
    s_eval, g, _ = run_masked("fp32", z, t, 4, 4, 4, WEIGHTS["all"], ign, spread(4), with_grad=False)
    s_train, _, _ = run_masked("fp32", z, t, 4, 4, 4, WEIGHTS["all"], ign, spread(4))
    assert g is None and np.array_equal(s_eval, s_train)
    zd = torch.zeros((1000, 40), dtype=torch.float32, device="cuda")
    td = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    dl = torch.zeros((1000, 40), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    w5 = (ctypes.c_float * 5)(1, 1, 1, 1, 1)
    st = torch.cuda.current_stream().cuda_stream

    def call(classes, ldc, dlc, dtype=_lib.F32, nbytes=None, lib_=lib, ign=255):
        return lib_.stp_softmax_loss_masked(zd.data_ptr(), td.data_ptr(), 1000, classes, ldc, dtype, w5, sc.data_ptr(), dl.data_ptr(),
                                            dlc, 1.0, ws.data_ptr(), ws.numel() * 4 if nbytes is None else nbytes, ign, None, st)
    assert call(1, 8, 8) == STP_E_BADARG
    assert call(33, 40, 40) == STP_E_BADARG
    assert call(4, 3, 8) == STP_E_BADARG              # ldc < classes
    assert call(4, 4, 3) == STP_E_BADARG              # dl_channels < classes
    assert call(4, 4, 4, ign=256) == STP_E_BADARG and call(4, 4, 4, ign=-2) == STP_E_BADARG
    assert call(4, 4, 4, dtype=77) == STP_E_BADARG
    assert call(4, 4, 4, dtype=_lib.F16) == STP_E_BADARG                                   # the other build's 16-bit code
    assert call(4, 4, 4, dtype=_lib.BF16, lib_=lib_for("fp16")[0]) == STP_E_BADARG
    assert call(4, 4, 4, nbytes=16) == STP_E_WORKSPACE
    assert call(4, 4, 4) == 0 and call(32, 40, 40, ign=-1) == 0 and call(4, 4, 4, ign=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ confusion
def run_confusion(dtype, z, t, C, ldc, ignore_label, entry="stp_class_confusion_ignore", guard=8):
    lib, _lib = lib_for(dtype)
    nb = int(lib.stp_class_confusion_workspace_bytes(C))
    zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint8)).cuda()
    cnt = torch.full((C * C + guard,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(nb // 4, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    if entry == "stp_class_confusion_ignore":
        rc = lib.stp_class_confusion_ignore(zd.data_ptr(), td.data_ptr(), z.shape[0], C, ldc, dt_code(_lib, dtype), cnt.data_ptr(), ws.data_ptr(), nb,
                                            ignore_label, st)
    else:
        rc = lib.stp_class_confusion(zd.data_ptr(), td.data_ptr(), z.shape[0], C, ldc, dt_code(_lib, dtype), cnt.data_ptr(), ws.data_ptr(), nb, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = cnt.cpu().numpy()
    assert (out[C * C:] == -7).all(), "the finalize launch wrote past the matrix"
    return out[:C * C].astype(np.int64).reshape(C, C)


def numpy_confusion(zq, t, C, ignore_label):
    on = R.counted(t, ignore_label)
    pred = zq[:, :C].argmax(axis=1)                      # the first index of the row maximum
    m = np.zeros((C, C), np.int64)
    np.add.at(m, (np.minimum(t[on].astype(np.int64), C - 1), pred[on]), 1)
    return m, int(on.sum())


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C,ldc", [(3, 8), (3, 3), (20, 20), (32, 40)])
@pytest.mark.parametrize("mask", ["piecewise", "random"])
def test_class_confusion_ignore_is_a_numpy_count(dtype, C, ldc, mask):
    P = 5 * 1024 + 77                                    # several workgroups of 1024, a ragged last wave
    z, t = make_case(P, C, ldc, 200 + C)
    rng = np.random.RandomState(C)
    if mask == "piecewise":                              # runs of one label, void runs among them: whole waves share a key or have none
        t = np.repeat(rng.randint(0, C + 1, P // 97 + 1), 97)[:P].astype(np.uint8)
        t[t == C] = 255
    else:
        t = t.copy()
        t[rng.rand(P) < 0.3] = 255
    zq = quantise(z, dtype)
    for ign in (255, 0, 1):
        want, n = numpy_confusion(zq, t, C, ign)
        got = run_confusion(dtype, z, t, C, ldc, ign)
        assert np.array_equal(got, want), (ign, got, want)
        assert got.sum() == n                            # the total is the number of counted pixels, exactly
    # no label to ignore: stp_class_confusion's counts (255 then counts as the last class, the clamp of every kernel)
    assert np.array_equal(run_confusion(dtype, z, t, C, ldc, -1), run_confusion(dtype, z, t, C, ldc, None, entry="stp_class_confusion"))
    assert run_confusion(dtype, z, t, C, ldc, -1).sum() == P


def test_class_confusion_ignore_everything_and_bad_arguments():
    z, t = make_case(3000, 4, 4, 9)
    assert run_confusion("fp32", z, np.full(3000, 255, np.uint8), 4, 4, 255).sum() == 0
    lib, _lib = lib_for("fp32")
    nb = int(lib.stp_class_confusion_workspace_bytes(4))
    zd = torch.zeros((100, 4), dtype=torch.float32, device="cuda")
    td = torch.zeros(100, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(16, dtype=torch.int32, device="cuda")
    ws = torch.empty(nb // 4, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(classes=4, ldc=4, dtype=_lib.F32, nbytes=nb, ign=255):
        return lib.stp_class_confusion_ignore(zd.data_ptr(), td.data_ptr(), 100, classes, ldc, dtype, cnt.data_ptr(), ws.data_ptr(), nbytes, ign, st)
    assert call(ign=256) == STP_E_BADARG and call(ign=-2) == STP_E_BADARG and call(classes=1) == STP_E_BADARG and call(ldc=3) == STP_E_BADARG
    assert call(dtype=_lib.F16) == STP_E_BADARG and call(nbytes=nb - 1) == STP_E_WORKSPACE and call() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ whole training step
SPEC = "categorical_crossentropy+0.5*dice_loss+0.3*iou_loss+0.2*jaccard_loss+2.0*focal_loss"
W5 = (1.0, 0.5, 0.3, 0.2, 2.0)
CW = [0.5, 2.0, 1.0]


def ring(y, value=255):
    """A square ring of void pixels, three wide, into label images [n, s, s, 1]."""
    s = y.shape[1]
    yy, xx = np.mgrid[0:s, 0:s]
    d = np.maximum(np.abs(yy - s // 2), np.abs(xx - s // 2))
    y = y.copy()
    y[:, (d >= s // 4) & (d < s // 4 + 3), 0] = value
    return y


class MaskedOracle(ostep.OracleTrainer):
    """oracle.step's training step with the loss of tests/_masked_loss_reference.py in place of composite_loss."""

    def __init__(self, *a, weights5=W5, ignore_label=None, class_weights=None, **kw):
        super().__init__(*a, **kw)
        self.weights5, self.ignore_label, self.class_weights = weights5, ignore_label, class_weights

    def step(self, x_nhwc, y_nhwc, taps=None, apply=True):
        P = onets.to_torch(self.P, self.trainable)
        x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float32))
        logits, bn_updates = self._forward(P, x, True, taps)
        loss, tm, _p, _y, _om = R.loss_of_logits(logits, np.asarray(y_nhwc)[..., 0], self.weights5, self.ignore_label, self.class_weights)
        loss.backward()
        grads = OrderedDict((k, P[k].grad.numpy().copy()) for k in self.trainable)
        out = {"logits": logits.detach().numpy().copy(), "loss": float(loss.detach()), "bce": float(tm[0].detach()),
               "dice_loss": float(tm[1].detach()), "jaccard_loss": float(tm[3].detach()), "focal_loss": float(tm[4].detach()),
               "iou_loss": float(tm[2].detach()), "grads": grads}
        self.steps_done += 1
        if apply:
            self.opt.step(self.P, ooptim.clip_grads(grads, self.clipnorm, self.clipvalue))
            for k, v in bn_updates.items():
                self.P[k] = v.numpy().astype(np.float32)
        return out


def step_pair(dtype, n=2, size=64, classes=3, seed=5, optimizer="sgd", lr=0.02, **kw):
    from segmentation_training_pipeline_amd.backend import HipSegModel
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = label_discs(n, size, classes, seed=seed)
    y = ring(y)
    storage = {"fp32": None, "bf16": "bf16", "fp16": "fp16"}[dtype]
    # (fp16: the oracle's stored gradients carry the build's default loss scale, as in the other IEEE-half step tests)
    tr = MaskedOracle(P, backbone="resnet18", loss=SPEC, optimizer=optimizer, lr=lr, activation="softmax", storage=storage,
                      grad_scale=16384.0 if dtype == "fp16" else None, ignore_label=255, class_weights=CW)
    m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype=dtype, loss=SPEC,
                    optimizer={"sgd": "SGD", "adam": "Adam"}[optimizer], lr=lr, ignore_label=255, class_weights=CW, **kw)
    m.set_weights(P)
    return m, tr, x, y


def logits_gradient(m):
    return m.plan.tensors["final_conv"].grad.to(torch.float32).cpu().numpy()


def test_fp32_masked_step_matches_oracle():
    """The bars of test_fp32_extended_softmax_step_matches_oracle (Unet)."""
    m, tr, x, y = step_pair("fp32", use_graph=False)
    names = [name for _fn, _a, name, _m in m.plan.fwd + m.plan.bwd if name]
    assert names.count("stp_softmax_loss_masked") == 1 and "stp_softmax_loss_ex" not in names and "stp_softmax_cce_dice" not in names
    o = tr.step(x.astype(np.float32), y.astype(np.float32))
    met = m.train_on_batch(x, y)
    print("logits max err %.3g" % np.abs(m.logits() - o["logits"]).max(), "loss", met["loss"], o["loss"])
    np.testing.assert_allclose(m.logits(), o["logits"], atol=1e-3)
    assert abs(met["loss"] - o["loss"]) < 2e-5 * max(1.0, abs(o["loss"]))
    assert abs(met["dice_loss"] - o["dice_loss"]) < 1e-5 and abs(met["categorical_crossentropy"] - o["bce"]) < 1e-5
    for k in ("jaccard_loss", "focal_loss", "iou_loss"):
        print("  ", k, met[k], o[k])
        assert abs(met[k] - o[k]) < 1e-5, (k, met[k], o[k])
    assert met["counted_pixels"] == float((y != 255).sum())
    dz = logits_gradient(m)
    void = y[..., 0] == 255
    assert void.any() and (dz[void] == 0).all() and np.abs(dz[~void]).max() > 0      # the logits' gradient is zero on the ring
    g = m.get_gradients()
    for k, ref in o["grads"].items():
        e = rel_l2(g[k], ref)
        assert e <= (1e-4 if k.startswith("final_conv") else 3e-2), "grad %s: rel L2 %.3g" % (k, e)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_masked_step_close_to_storage_quantised_oracle(dtype):
    """Against the oracle that rounds at the same points, at the bars of test_bf16_extended_softmax_step_close_to_storage_quantised_oracle
    (IEEE half rounds finer than bfloat16: the same bars hold a fortiori; its build runs under the default loss scale, dynamic
    multiplier included)."""
    m, tr, x, y = step_pair(dtype, seed=9, optimizer="adam", lr=1e-3, use_graph=False)
    if dtype == "fp16":
        fwd = [name for _fn, _a, name, _m in m.plan.fwd if name]
        assert m.plan.dls is not None and m.loss_scale == 16384.0 and fwd[fwd.index("stp_softmax_loss_masked") + 1] == "stp_scale_by_device"
    o = tr.step(x.astype(np.float32), y.astype(np.float32))
    met = m.train_on_batch(x, y)
    assert all(np.isfinite(v) for v in met.values()) and m.skipped_steps == 0
    ref = o["logits"]
    err = np.abs(m.logits() - ref)
    rng_ = np.abs(ref).max()
    assert err.mean() < 0.01 * rng_ and err.max() < 0.1 * rng_, (err.max(), err.mean(), rng_)
    assert abs(met["loss"] - o["loss"]) < 1e-2 and abs(met["dice_loss"] - o["dice_loss"]) < 5e-3
    assert met["counted_pixels"] == float((y != 255).sum())
    void = y[..., 0] == 255
    assert (logits_gradient(m)[void] == 0).all()
    g = m.get_gradients()
    for k in ("final_conv/kernel", "final_conv/bias"):
        a, b = g[k].ravel().astype(np.float64), o["grads"][k].ravel().astype(np.float64)
        assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30) > 0.99, k
    losses = [met["loss"]] + [m.train_on_batch(x, y)["loss"] for _ in range(6)]
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("arch,size", [("FPN", 64), ("PSPNet", 96)])
def test_low_resolution_heads_keep_their_resize_and_train(arch, size):
    from segmentation_training_pipeline_amd.backend import HipSegModel
    classes, n = 3, 2
    m = HipSegModel(arch, "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="bf16", loss="categorical_crossentropy+dice_loss",
                    optimizer="Adam", lr=1e-3, ignore_label=255, class_weights=CW, class_metrics=True, use_graph=True)
    names = [name for _fn, _a, name, _m in m.plan.fwd + m.plan.bwd if name]
    assert names.count("stp_softmax_loss_masked") == 1 and names.count("stp_class_confusion_ignore") == 1
    assert "stp_resize_bilinear" in names and "stp_resize_bilinear_bwd" in names and "stp_softmax_cce_dice_up" not in names
    x, y = label_discs(n, size, classes, seed=3)
    y = ring(y)
    mets = [m.train_on_batch(x, y) for _ in range(8)]
    assert all(np.isfinite(v) for d in mets for v in d.values())
    assert mets[-1]["loss"] < mets[0]["loss"]
    assert mets[0]["counted_pixels"] == float((y != 255).sum()) == float(m.confusion().sum())


def test_rerun_over_the_valid_prefix_and_graph_replay():
    """Plan.rerun_loss / rerun_confusion know the new launches (second argument: the pixels of the real samples); two models replaying
    their captured step agree bit for bit."""
    from segmentation_training_pipeline_amd.backend import HipSegModel
    n, size, classes = 4, 64, 3
    x, y = label_discs(n, size, classes, seed=31)
    y = ring(y)
    y[3] = 255                                   # the last sample is void altogether
    out = []
    for _ in range(2):
        m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="bf16", loss=SPEC, ignore_label=255,
                        class_weights=CW, class_metrics=True, use_graph=True)
        m.set_weights(onets.init_unet_resnet("resnet18", classes=classes, seed=42))
        mets = [m.train_on_batch(x, y) for _ in range(3)]
        out.append((mets, m.logits()))
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
    full = m.plan.loss_scalars.cpu().numpy().copy()
    assert full[12] == (y != 255).sum() == m.confusion().sum()
    m.plan.rerun_loss(2)
    torch.cuda.synchronize()
    part = m.plan.loss_scalars.cpu().numpy().copy()
    assert part[12] == (y[:2] != 255).sum() == m.confusion().sum()
    # the same entry point over the first two samples of the plan's own logits and target
    lg, tg = m.plan.tensor("final_conv"), m.plan.inputs["mask"]
    z = lg.buf.to(torch.float32).cpu().numpy().reshape(-1, lg.C)[:2 * size * size]
    sc, _, _ = run_masked("bf16", z, tg.buf.cpu().numpy().reshape(-1)[:2 * size * size], classes, lg.C, lg.gradC, W5, 255, CW, with_grad=False)
    assert np.array_equal(sc[:14], part[:14])


def test_without_the_keys_the_launch_names_are_the_parents():
    from segmentation_training_pipeline_amd.backend import HipSegModel
    for spec, launch in (("categorical_crossentropy+dice_loss", "stp_softmax_cce_dice"), (SPEC, "stp_softmax_loss_ex")):
        m = HipSegModel("Unet", "resnet18", (64, 64, 3), 3, "softmax", batch=2, dtype="bf16", loss=spec, class_metrics=True, use_graph=False)
        names = [name for _fn, _a, name, _m in m.plan.fwd + m.plan.bwd if name]
        assert names.count(launch) == 1 and names.count("stp_class_confusion") == 1
        assert "stp_softmax_loss_masked" not in names and "stp_class_confusion_ignore" not in names
        x, y = label_discs(2, 64, 3, seed=2)
        assert "counted_pixels" not in m.train_on_batch(x, y)


# ------------------------------------------------------------------------------------------ end to end
YAML = """
backbone: resnet18
architecture: Unet
classes: 3
activation: softmax
encoder_weights:
shape: [64, 64, 3]
batch: 4
lr: 0.005
optimizer: Adam
loss: categorical_crossentropy+dice_loss
ignore_label: 255
class_weights: [0.5, 2.0, 1.0]
metrics: [mean_iou]
primary_metric: val_mean_iou
primary_metric_mode: max
folds_count: 2
random_state: 7
dtype: bf16
draw_examples: false
stages:
  - epochs: 2
"""


class VoidLabelSet(object):
    """Ad-hoc dataset: synthetic discs with H x W x 1 label images that carry a ring of 255."""

    def __init__(self, n, size=64, classes=3, seed=0):
        self.x, y = label_discs(n, size, classes, seed)
        self.y = ring(y)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        from segmentation_pipeline.impl.datasets import PredictionItem
        return PredictionItem("disc%03d.png" % i, self.x[i], self.y[i])


def test_yaml_experiment_with_void_labels_end_to_end(tmp_path, monkeypatch):
    from segmentation_pipeline import segmentation
    from segmentation_training_pipeline_amd import pipeline
    cfgp = tmp_path / "void.yaml"
    cfgp.write_text(YAML)
    cfg = segmentation.parse(str(cfgp))
    ds = VoidLabelSet(16, seed=1)
    epochs = []
    run = pipeline.Trainer.run_epoch_sums

    def recording(self, indexes, training):
        idx = [int(i) for i in indexes]
        sums, n = run(self, idx, training)
        assert self.model.masked and self.feeder.ignore_label == 255
        epochs.append((idx, int(np.asarray(sums[pipeline.CONFUSION_KEY]).sum())))
        return sums, n
    monkeypatch.setattr(pipeline.Trainer, "run_epoch_sums", recording)
    out = cfg.fit(ds, foldsToExecute=[0])
    assert len(out) == 1 and np.isfinite(out[0]["val_mean_iou"])
    with open(cfg.metricsPath(0, 0)) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    for col in ("loss", "val_loss", "categorical_crossentropy", "dice_loss", "mean_iou", "val_mean_iou", "categorical_accuracy", "iou_class_0",
                "iou_class_2", "val_iou_class_1"):
        assert all(col in r and np.isfinite(float(r[col])) for r in rows), col
    assert 0.0 < float(rows[1]["val_mean_iou"]) <= 1.0
    # no augmentation, images at the network's size: the epoch's confusion matrix counts exactly the pixels that are not void
    assert len(epochs) == 4
    for idx, total in epochs:
        assert len(idx) == 8 and total == sum(int((ds.y[i] != 255).sum()) for i in idx)
        assert total < len(idx) * 64 * 64
