"""categorical_accuracy and mean IoU of the softmax heads, on the GPU: the confusion kernel stp_class_confusion and its
low-resolution form against numpy's argmax on the stored values (integer counts: exact equality everywhere), the matrix a model
holds after a step against its own logits, the training step left bit-identical by the switch, and a YAML experiment end to end."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DTYPES = ["fp32", "bf16", "fp16"]
STP_E_BADARG, STP_E_WORKSPACE = -1, -3
CLASSES = [2, 3, 4, 5, 8, 9, 16, 17, 20, 24, 25, 32]          # both edges of every class bucket (4, 8, 16, 24, 32); 20: 8-byte rows
GARBAGE, SENTINEL, GUARD = -7, 0x5A5A5A5, 64


def lib_for(dtype):
    from segmentation_training_pipeline_amd import _lib
    return _lib.load("fp16" if dtype == "fp16" else "bf16"), _lib


def dt_code(_lib, dtype):
    return {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}[dtype]


# Pixels the largest grid covers with one pixel per thread: 512 workgroups of 1024 threads (= 2048 x 256); beyond it the kernel strides.
THREAD_CAPACITY = 2048 * 256
PIXELS = [1, 63, 64, 65, 255, 256, 257, 1000, THREAD_CAPACITY + 77]


def test_the_workspace_holds_one_table_per_workgroup_of_the_largest_grid():
    lib, _ = lib_for("fp32")
    for C in (2, 3, 20, 32):
        assert lib.stp_class_confusion_workspace_bytes(C) // (4 * C * C) * 1024 == THREAD_CAPACITY


def quantise(z, dtype):
    return torch.from_numpy(z).to(TD[dtype]).to(torch.float32).numpy()


def reference(zq, t, C):
    """numpy on the stored values: argmax takes the FIRST index of the maximum; the target is clamped as the loss kernels clamp it."""
    pred = np.argmax(zq[:, :C], axis=1)
    tt = np.minimum(t.astype(np.int64), C - 1)
    return np.bincount(tt * C + pred, minlength=C * C).astype(np.int64)


def counts_buffer(C):
    buf = torch.full((C * C + GUARD,), GARBAGE, dtype=torch.int32, device="cuda")      # the kernel overwrites; it does not accumulate
    buf[C * C:] = SENTINEL
    return buf


def read_counts(buf, C):
    out = buf.cpu().numpy().astype(np.int64)
    assert (out[C * C:] == SENTINEL).all(), "the kernel wrote behind entry classes^2"
    return out[:C * C]


def workspace(lib, C):
    nb = int(lib.stp_class_confusion_workspace_bytes(C))
    return torch.empty(nb // 4, dtype=torch.int32, device="cuda"), nb


def run_conf(dtype, z, t, C, ldc):
    """z float32 [P, ldc] (rounded to the storage type here), t uint8 [P] -> the classes^2 counts."""
    lib, _lib = lib_for(dtype)
    zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint8)).cuda()
    ws, nb = workspace(lib, C)
    cnt = counts_buffer(C)
    rc = lib.stp_class_confusion(zd.data_ptr(), td.data_ptr(), z.shape[0], C, ldc, dt_code(_lib, dtype), cnt.data_ptr(), ws.data_ptr(), nb,
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return read_counts(cnt, C)


@functools.lru_cache(maxsize=12)
def random_rows(P, C, seed):
    """Logits of scale 2 (shared by the dtypes and strides of a class count; never written to)."""
    z = np.random.RandomState(seed).randn(P, C).astype(np.float32) * 2.0
    z.setflags(write=False)
    return z


def make_case(P, C, ldc, seed, target="random"):
    z = np.full((P, ldc), 1e4, np.float32)                       # padding channels: must never win
    z[:, :C] = random_rows(P, C, seed)
    rng = np.random.RandomState(seed + 1)
    if target == "first":
        t = np.zeros(P, np.uint8)
    elif target == "last":
        t = np.full(P, C - 1, np.uint8)
    elif target == "255":
        t = np.full(P, 255, np.uint8)
    else:
        t = rng.randint(0, C, P).astype(np.uint8)
    return z, t


def test_bf16_rows_do_tie_and_fp32_rows_do_not():
    """What the tie-break cases below rest on (CPU arithmetic): random logits of scale 2 tie in the row maximum in 33 of 4096 rows at 20
    classes in bf16, in none in fp32."""
    z = np.random.RandomState(0).randn(4096, 20).astype(np.float32) * 2.0
    ties = lambda q: int(((q == q.max(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
    assert ties(quantise(z, "bf16")) == 33 and ties(z) == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", CLASSES)
def test_counts_equal_numpy_argmax(dtype, C):
    pad = (C // 8 + 1) * 8                                        # the next multiple of 8: 16-byte rows
    for P in PIXELS:
        # every target form with either stride; at the strided count the varying and the clamped one
        modes = ("random", "first", "last", "255") if P <= 1000 else ("random", "255")
        for ldc, mode in itertools.product((C, pad), modes):
            z, t = make_case(P, C, ldc, 1000 * C + P, mode)
            if P >= 64:                                           # rows of all-equal values count as class 0; (bf16 rows tie on their own too)
                z[3, :C] = 0.0
                z[P // 2, :C] = -1.5
                z[P - 1, :C] = 7.0
            zq = quantise(z, dtype)
            got, ref = run_conf(dtype, z, t, C, ldc), reference(zq, t, C)
            assert got.sum() == P
            assert np.array_equal(got, ref), (dtype, C, P, ldc, mode, np.abs(got - ref).sum())
            if mode == "255":                                     # clamped: everything in the last row
                assert got.reshape(C, C)[:C - 1].sum() == 0
            if P >= 64:
                pred_equal = np.argmax(zq[[3, P // 2, P - 1], :C], axis=1)
                assert (pred_equal == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_row_is_counted_once(dtype):
    for C, ldc in ((3, 3), (20, 20), (5, 8)):
        z, t = make_case(1000, C, ldc, 5)
        z[10, :C] = np.nan
        z[11, 0] = np.nan
        z[12, C - 1] = np.nan
        z[13, :C] = np.inf
        z[14, :C] = -np.inf
        got = run_conf(dtype, z, t, C, ldc)
        assert got.sum() == 1000 and (got >= 0).all()
        # the rows without a NaN are numpy's
        keep = np.ones(1000, bool)
        keep[10:13] = False
        ref = reference(quantise(z, dtype)[keep], t[keep], C)
        assert ((got - ref) >= 0).all() and (got - ref).sum() == 3


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 20, 32])
def test_wave_aggregation_extremes(dtype, C):
    P = 5000
    # every pixel of every wave carries one key
    z = np.zeros((P, C), np.float32)
    z[:, C - 2] = 3.0
    t = np.full(P, 1, np.uint8)
    got = run_conf(dtype, z, t, C, C).reshape(C, C)
    assert got[1, C - 2] == P and got.sum() == P
    # 64 consecutive pixels with 64 distinct keys: t = i % C, predicted = (i / C) % C
    i = np.arange(P)
    t = (i % C).astype(np.uint8)
    pred = (i // C) % C
    z = np.zeros((P, C), np.float32)
    z[i, pred] = 1.0
    for w in range(0, P - 64, 64):
        assert len(set((t[w:w + 64].astype(int) * C + pred[w:w + 64]).tolist())) == 64
    got = run_conf(dtype, z, t, C, C)
    assert np.array_equal(got, reference(quantise(z, dtype), t, C))
    assert np.array_equal(got, np.bincount(t.astype(np.int64) * C + pred, minlength=C * C))


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_and_a_graph_replay_give_equal_counts(dtype):
    lib, _lib = lib_for(dtype)
    C, P = 20, 70001
    z, t = make_case(P, C, C, 9)
    zd = torch.from_numpy(z).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(t).cuda()
    ws, nb = workspace(lib, C)
    cnt = counts_buffer(C)

    def call():
        rc = lib.stp_class_confusion(zd.data_ptr(), td.data_ptr(), P, C, C, dt_code(_lib, dtype), cnt.data_ptr(), ws.data_ptr(), nb,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    call()
    torch.cuda.synchronize()
    first = read_counts(cnt, C)
    assert np.array_equal(first, reference(quantise(z, dtype), t, C))
    call()                                                        # overwrites: not twice the counts
    torch.cuda.synchronize()
    assert np.array_equal(read_counts(cnt, C), first)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for _ in range(3):
        cnt[:C * C] = GARBAGE
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(read_counts(cnt, C), first)


@pytest.mark.parametrize("build", ["bf16", "fp16"])
def test_bad_arguments_and_workspace(build):
    lib, _lib = lib_for(build)
    own16, other16 = (_lib.BF16, _lib.F16) if build == "bf16" else (_lib.F16, _lib.BF16)
    zd = torch.zeros((1000, 40), dtype=torch.float32, device="cuda")
    td = torch.zeros(1000 * 256, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1024 + GUARD, dtype=torch.int32, device="cuda")
    ws, nb = workspace(lib, 32)
    st = torch.cuda.current_stream().cuda_stream

    def call(classes=4, ldc=4, pixels=1000, dtype=_lib.F32, nbytes=None, rows=zd.data_ptr(), target=td.data_ptr(), counts=cnt.data_ptr(),
             wsp=ws.data_ptr(), lib_=lib):
        return lib_.stp_class_confusion(rows, target, pixels, classes, ldc, dtype, counts, wsp, nb if nbytes is None else nbytes, st)
    assert call(classes=1, ldc=8) == STP_E_BADARG
    assert call(classes=33, ldc=40) == STP_E_BADARG
    assert call(classes=4, ldc=3) == STP_E_BADARG                 # ldc < classes
    for k in ("rows", "target", "counts", "wsp"):
        assert call(**{k: None}) == STP_E_BADARG
    assert call(pixels=0) == STP_E_BADARG and call(pixels=-5) == STP_E_BADARG
    assert call(pixels=1 << 31) == STP_E_BADARG and call(pixels=1 << 40) == STP_E_BADARG
    assert call(dtype=77) == STP_E_BADARG
    assert call(dtype=other16) == STP_E_BADARG                                           # the other build's 16-bit code
    need = int(lib.stp_class_confusion_workspace_bytes(4))
    assert call(nbytes=need - 1) == STP_E_WORKSPACE and call(nbytes=0) == STP_E_WORKSPACE
    assert call(nbytes=need) == 0 and call(classes=32, ldc=40) == 0 and call(dtype=own16) == 0
    # the low-resolution form
    def up(N=2, H=3, W=5, factor=4, classes=3, ldc=4, dtype=_lib.F32, nbytes=None, low=zd.data_ptr(), target=td.data_ptr(), counts=cnt.data_ptr(),
           wsp=ws.data_ptr(), lib_=lib):
        return lib_.stp_class_confusion_up(low, target, N, H, W, factor, classes, ldc, dtype, counts, wsp, nb if nbytes is None else nbytes, st)
    for f in (0, 1, 3, 5, 32):
        assert up(factor=f) == STP_E_BADARG
    assert up(classes=1) == STP_E_BADARG and up(classes=33, ldc=40) == STP_E_BADARG and up(classes=4, ldc=3) == STP_E_BADARG
    for k in ("low", "target", "counts", "wsp"):
        assert up(**{k: None}) == STP_E_BADARG
    assert up(N=0) == STP_E_BADARG and up(H=0) == STP_E_BADARG and up(W=-1) == STP_E_BADARG
    assert up(N=1 << 20, H=8, W=8, factor=16) == STP_E_BADARG     # 2^34 pixels
    assert up(N=1 << 9, H=1 << 7, W=1 << 7, factor=16) == STP_E_BADARG      # exactly 2^31
    assert up(N=1 << 30, H=1 << 30, W=1 << 30, factor=16) == STP_E_BADARG     # (the product leaves 64 bits)
    assert up(dtype=77) == STP_E_BADARG and up(dtype=other16) == STP_E_BADARG
    assert up(nbytes=int(lib.stp_class_confusion_workspace_bytes(3)) - 1) == STP_E_WORKSPACE
    assert up() == 0 and up(dtype=own16) == 0
    torch.cuda.synchronize()


def run_up_and_chain(dtype, low, t, N, H, W, f, C, ldc):
    """-> (counts of stp_class_confusion_up on the low-resolution rows, counts of stp_resize_bilinear + stp_class_confusion)."""
    lib, _lib = lib_for(dtype)
    code = dt_code(_lib, dtype)
    ld = torch.from_numpy(low).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(t).cuda()
    ws, nb = workspace(lib, C)
    st = torch.cuda.current_stream().cuda_stream
    a = counts_buffer(C)
    assert lib.stp_class_confusion_up(ld.data_ptr(), td.data_ptr(), N, H, W, f, C, ldc, code, a.data_ptr(), ws.data_ptr(), nb, st) == 0
    torch.cuda.synchronize()
    up = read_counts(a, C)
    full = torch.zeros((N, H * f, W * f, ldc), dtype=TD[dtype], device="cuda")
    assert lib.stp_resize_bilinear(ld.data_ptr(), full.data_ptr(), N, H, W, ldc, f, ldc, 0, code, st) == 0
    b = counts_buffer(C)
    assert lib.stp_class_confusion(full.data_ptr(), td.data_ptr(), N * H * f * W * f, C, ldc, code, b.data_ptr(), ws.data_ptr(), nb, st) == 0
    torch.cuda.synchronize()
    chain = read_counts(b, C)
    # the chain's second half is numpy's argmax of the resized tensor
    ref = reference(full.to(torch.float32).cpu().numpy().reshape(-1, ldc), t.reshape(-1), C)
    assert np.array_equal(chain, ref)
    return up, chain


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("f", [2, 4, 8, 16])
@pytest.mark.parametrize("C", [3, 20])
def test_low_resolution_form_equals_resize_then_count(dtype, f, C):
    N = 2
    for (H, W), ldc in (((3, 5), C), ((1, 1), C), ((3, 5), (C // 8 + 1) * 8), ((24, 24), C)):
        if H == 24 and f > 8:
            continue
        rng = np.random.RandomState(100 * C + 10 * f + H)
        low = np.full((N, H, W, ldc), 1e4, np.float32)
        low[..., :C] = rng.randn(N, H, W, C).astype(np.float32) * 2.0
        t = rng.randint(0, C, (N, H * f, W * f)).astype(np.uint8)
        if H == 3:                                                # blocks of one class, as a mask has them, and a clamped value
            t[:, :f, :] = 1
            t[0, -1, -1] = 255
        up, chain = run_up_and_chain(dtype, low, t, N, H, W, f, C, ldc)
        assert up.sum() == N * H * f * W * f
        assert np.array_equal(up, chain), (dtype, f, C, H, W, ldc, np.abs(up - chain).sum())


# ------------------------------------------------------------------------------------------ models
LOSS = "categorical_crossentropy+0.5*dice_loss"


def label_discs(n, size, classes, seed):
    """uint8 images and [n, size, size, 1] label images (pixel value = class index): discs of classes 1 .. C - 1 on class 0."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    x = (rng.rand(n, size, size, 3) * 60).astype(np.uint8)
    y = np.zeros((n, size, size, 1), np.uint8)
    for i in range(n):
        for c in list(range(1, classes)) * 2:
            cy, cx, r = rng.randint(0, size), rng.randint(0, size), rng.randint(size // 8, size // 3)
            d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            y[i, :, :, 0][d] = c
            x[i][d] = np.minimum(255, x[i][d].astype(np.int32) + 40 * c).astype(np.uint8)
    return x, y


def model(arch, backbone, size, classes, dtype, batch=2, **kw):
    from segmentation_training_pipeline_amd.backend import HipSegModel
    kw.setdefault("use_graph", False)
    return HipSegModel(arch, backbone, (size, size, 3), classes, "softmax", batch=batch, dtype=dtype, loss=LOSS, optimizer="Adam", lr=1e-3, **kw)


def numpy_confusion(logits, y, classes):
    return reference(logits.reshape(-1, classes), y.reshape(-1), classes).reshape(classes, classes)


@pytest.mark.parametrize("arch,backbone,size,classes,dtype,launch", [
    ("Unet", "resnet18", 64, 3, "fp32", "stp_class_confusion"),
    ("PSPNet", "resnet18", 96, 4, "bf16", "stp_class_confusion_up"),          # factor 8
    ("FPN", "resnet18", 64, 3, "bf16", "stp_class_confusion_up"),             # factor 4
    ("DeepLabV3", "mobilenetv2", 64, 3, "fp32", "stp_class_confusion")])
def test_model_confusion_is_the_argmax_of_its_logits(arch, backbone, size, classes, dtype, launch):
    m = model(arch, backbone, size, classes, dtype, class_metrics=True)
    fwd = [name for _fn, _a, name, _m in m.plan.fwd if name]
    assert fwd.count(launch) == 1 and sum(n.startswith("stp_class_confusion") for n in fwd) == 1
    if launch.endswith("_up"):
        assert "stp_softmax_cce_dice_up" in fwd and "fused:resize->loss" in fwd      # the resized logits stay out of the step
        a = [a for _fn, a, name, _m in m.plan.fwd if name == launch][0]
        assert a[5] == {"PSPNet": 8, "FPN": 4}[arch]
    x, y = label_discs(2, size, classes, seed=3)
    m.load_batch(x, y)
    m.forward_backward()
    torch.cuda.synchronize()
    got = m.confusion()
    assert got.dtype == np.int64 and got.shape == (classes, classes) and got.sum() == 2 * size * size
    ref = numpy_confusion(m.logits(), y, classes)                 # (logits() materialises the resize fused into the loss)
    assert np.array_equal(got, ref), (got, ref)
    met = m.metrics()
    assert met["categorical_accuracy"] == np.trace(ref) / ref.sum()
    from segmentation_training_pipeline_amd.backend import confusion_metrics
    want = confusion_metrics(ref)
    assert all(met[k] == v for k, v in want.items()) and set(want) == {"categorical_accuracy", "mean_iou"} | {"iou_class_%d" % k for k in range(classes)}
    # a padded training batch: the launch re-run over the real samples alone (Plan.rerun_confusion; both forms)
    logits = m.logits()
    m.plan.rerun_confusion(1)
    torch.cuda.synchronize()
    assert np.array_equal(m.confusion(), numpy_confusion(logits[:1], y[:1], classes))


def test_switch_off_metrics_and_refusal():
    m = model("Unet", "resnet18", 64, 3, "fp32")
    x, y = label_discs(2, 64, 3, seed=3)
    met = m.train_on_batch(x, y)
    assert sorted(met) == sorted(["loss", "categorical_crossentropy", "dice_loss", "dice", "binary_accuracy", "iou", "iot"])
    assert m.plan.class_counts is None and not any((n or "").startswith("stp_class_confusion") for _f, _a, n, _m in m.plan.fwd)
    with pytest.raises(ValueError, match="class_metrics"):
        m.confusion()


@pytest.mark.parametrize("arch,size,dtype", [("Unet", 64, "fp32"), ("PSPNet", 96, "bf16")])
def test_training_is_bit_identical_with_the_switch_on_and_off(arch, size, dtype):
    out = []
    batches = [label_discs(2, size, 3, seed=11 + i) for i in range(2)]
    for on in (False, True):
        m = model(arch, "resnet18", size, 3, dtype, class_metrics=on, seed=7)
        scal = []
        for x, y in batches:
            m.train_on_batch(x, y, fetch=False)
            scal.append(m.plan.loss_scalars.cpu().numpy()[:10].copy())      # (stp_softmax_cce_dice writes scalars 0 .. 9)
        out.append((scal, m.get_weights()))
    for a, b in zip(out[0][0], out[1][0]):
        assert np.array_equal(a, b)
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k


@pytest.mark.parametrize("arch,size,dtype", [("Unet", 64, "bf16"), ("FPN", 64, "bf16"), ("Unet", 64, "fp16")])
def test_captured_graph_counts_equal_eager(arch, size, dtype):
    x, y = label_discs(2, size, 3, seed=5)
    got = []
    for use_graph in (False, True):
        m = model(arch, "resnet18", size, 3, dtype, class_metrics=True, use_graph=use_graph, seed=7)
        steps = []
        for _ in range(2):                                        # the second step replays the captured graph on updated weights
            m.train_on_batch(x, y, fetch=False)
            steps.append(m.confusion())
        got.append(steps)
    for a, b in zip(*got):
        assert np.array_equal(a, b) and a.sum() == 2 * size * size


@pytest.mark.parametrize("arch,size,dtype", [("Unet", 64, "fp32"), ("PSPNet", 96, "bf16")])
def test_evaluation_plan_counts_only_the_valid_prefix(arch, size, dtype):
    n, classes = 4, 3
    m = model(arch, "resnet18", size, classes, dtype, batch=n, class_metrics=True)
    ep = m.eval_plan()
    names = [name for _fn, _a, name, _m in ep.fwd if name]
    assert names.count("stp_class_confusion") == 1 and "stp_class_confusion_up" not in names
    x, y = label_discs(n, size, classes, seed=31)
    ep.inputs["image"].buf.copy_(torch.from_numpy(x).reshape(ep.inputs["image"].buf.shape))
    ep.inputs["mask"].buf.copy_(torch.from_numpy(y).reshape(ep.inputs["mask"].buf.shape))
    ep.run(ep.prep); ep.run(ep.fwd)
    torch.cuda.synchronize()
    t = ep.tensor("logits" if "logits" in ep.tensors else "final_conv")
    logits = t.buf.to(torch.float32).cpu().numpy()
    full = m.confusion(ep)
    assert full.sum() == n * size * size and np.array_equal(full, numpy_confusion(logits, y, classes))
    ep.rerun_loss(3)
    torch.cuda.synchronize()
    part = m.confusion(ep)
    assert part.sum() == 3 * size * size
    assert np.array_equal(part, numpy_confusion(logits[:3], y[:3], classes))


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
metrics: [categorical_accuracy, mean_iou]
primary_metric: val_mean_iou
folds_count: 2
random_state: 7
dtype: fp32
draw_examples: false
stages:
  - epochs: 2
"""


class LabelSet(object):
    """Ad-hoc dataset: synthetic discs with H x W x 1 label images."""

    def __init__(self, n, size=64, classes=3, seed=0):
        self.x, self.y = label_discs(n, size, classes, seed)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        from segmentation_pipeline.impl.datasets import PredictionItem
        return PredictionItem("disc%03d.png" % i, self.x[i], self.y[i])


def test_yaml_experiment_logs_and_selects_on_the_class_metrics(tmp_path):
    import csv

    from segmentation_pipeline import segmentation
    cfgp = tmp_path / "cls.yaml"
    cfgp.write_text(YAML)
    cfg = segmentation.parse(str(cfgp))
    ds = LabelSet(18, seed=1)                                     # 9 validation samples per fold: two full batches of 4 and one of 1
    out = cfg.fit(ds, foldsToExecute=[0])
    assert len(out) == 1 and 0.0 <= out[0]["val_mean_iou"] <= 1.0
    with open(cfg.metricsPath(0, 0)) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2
    cols = ["categorical_accuracy", "mean_iou", "iou_class_0", "iou_class_1", "iou_class_2"]
    for r in rows:
        for col in cols + ["val_" + c for c in cols]:
            assert col in r and 0.0 <= float(r[col]) <= 1.0, col
        assert "binary_accuracy" in r and "val_loss" in r
    assert os.path.getsize(cfg.weightsPath(0, 0)) > 0             # the best-weights file, chosen on val_mean_iou
    best = max(range(2), key=lambda e: (float(rows[e]["val_mean_iou"]), -e))
    assert out[0]["best_epoch"] == best and out[0]["val_mean_iou"] == float(rows[best]["val_mean_iou"])


def _accuracy_from_predict(ds, val_idx, impl):
    """predict() takes its argmax on float32 PROBABILITIES, where a softmax can merge near-equal logits: pixels whose two largest
    probabilities differ by < 1e-6 may fall either way."""
    p = impl.predict(np.stack([ds.x[i] for i in val_idx]))
    y = np.stack([ds.y[i] for i in val_idx])[..., 0]
    top2 = np.sort(p, axis=-1)[..., -2:]
    close = int(((top2[..., 1] - top2[..., 0]) < 1e-6).sum())
    return float((np.argmax(p, axis=-1) == y).mean()), close, y.size


def test_yaml_val_categorical_accuracy_matches_predict(tmp_path):
    import csv

    from segmentation_pipeline import segmentation
    from segmentation_training_pipeline_amd import pipeline
    cfgp = tmp_path / "acc.yaml"
    cfgp.write_text(YAML.replace("epochs: 2", "epochs: 1"))
    cfg = segmentation.parse(str(cfgp))
    ds = LabelSet(18, seed=2)
    kept = {}
    orig = pipeline.GenericTaskConfig._compiled

    def keep(self, stage=None, use_graph=True):                   # the model fit() trains, kept for the recomputation
        kept["model"] = orig(self, stage, use_graph)
        return kept["model"]
    pipeline.GenericTaskConfig._compiled = keep
    try:
        cfg.fit(ds, foldsToExecute=[0])
    finally:
        pipeline.GenericTaskConfig._compiled = orig
    with open(cfg.metricsPath(0, 0)) as f:
        row = list(csv.DictReader(f))[-1]
    kf = cfg.kfold(ds, range(len(ds)))
    val_idx = [int(i) for i in kf.sampledIndexes(0, False, cfg.stages[0].validation_negatives)]
    assert len(val_idx) % 4 != 0, "the last validation batch must be a padded one"
    # the model holds the weights of the last (only) epoch, which the validation pass evaluated
    acc, close, pixels = _accuracy_from_predict(ds, val_idx, kept["model"].impl)
    print("val_categorical_accuracy %.9g, from predict() %.9g, %d of %d pixels within 1e-6" % (float(row["val_categorical_accuracy"]), acc, close, pixels))
    assert close <= 1e-3 * pixels                                 # more than 0.1 % that close would make the comparison void
    assert abs(float(row["val_categorical_accuracy"]) - acc) <= close / pixels + 1e-12


def test_yaml_primary_metric_alone_turns_the_switch_on(tmp_path):
    from segmentation_pipeline import segmentation
    cfgp = tmp_path / "prim.yaml"
    cfgp.write_text(YAML.replace("metrics: [categorical_accuracy, mean_iou]\n", "").replace("val_mean_iou", "val_categorical_accuracy")
                    .replace("epochs: 2", "epochs: 1"))
    cfg = segmentation.parse(str(cfgp))
    assert cfg.metrics == []
    out = cfg.fit(LabelSet(16, seed=1), foldsToExecute=[0])
    assert len(out) == 1 and 0.0 <= out[0]["val_categorical_accuracy"] <= 1.0
    assert os.path.getsize(cfg.weightsPath(0, 0)) > 0
