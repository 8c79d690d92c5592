"""Multi-label sigmoid heads on the GPU (``classes: C > 1`` with ``activation: sigmoid``): the loss kernel
stp_sigmoid_multilabel_loss / stp_sigmoid_multilabel_bias_grad against float64 restatements of oracle/losses.py on the
[pixels, C] tensor, one training step of each segmentation_models graph against the oracle, the 1-class path left as it
was, and a YAML experiment end to end."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import losses as olosses  # noqa: E402
from oracle import nets as onets  # noqa: E402
from oracle import step as ostep  # noqa: E402

TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
WEIGHTS = {"bce": (1.0, 0, 0, 0, 0), "bce+dice": (1.0, 1.0, 0, 0, 0), "all": (1.0, 0.5, 0.3, 0.2, 2.0)}
STP_E_BADARG = -1


def lib_for(dtype):
    from segmentation_training_pipeline_amd import _lib
    return _lib.load("fp16" if dtype == "fp16" else "bf16"), _lib


def dt_code(_lib, dtype):
    return {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}[dtype]


def run_loss(dtype, z, bits, classes, ldc, dlc, weights, grad_scale=1.0, with_grad=True, guard=64):
    """-> (scalars[12], dlogits [P, dlc] float32 or None, workspace, device tensors).  ``z``: float32 [P, ldc] (rounded to the
    storage type here); the gradient buffer is filled with NaN, ``guard`` elements past its end must stay NaN."""
    lib, _lib = lib_for(dtype)
    P = z.shape[0]
    zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(np.ascontiguousarray(bits, np.uint8)).cuda()
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    dl = torch.full((P * dlc + guard,), float("nan"), dtype=TD[dtype], device="cuda") if with_grad else None
    w5 = (ctypes.c_float * 5)(*weights)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.stp_sigmoid_multilabel_loss(zd.data_ptr(), td.data_ptr(), P, classes, ldc, dt_code(_lib, dtype), w5, sc.data_ptr(),
                                         dl.data_ptr() if dl is not None else None, dlc, grad_scale, ws.data_ptr(), ws.numel() * 4, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    g = None
    if dl is not None:
        full = dl.to(torch.float32).cpu().numpy()
        assert np.isnan(full[P * dlc:]).all(), "the gradient pass wrote past its tensor"
        g = full[:P * dlc].reshape(P, dlc)
    return sc.cpu().numpy(), g, ws, (zd, td)


def reference(zq, y, weights):
    """float64 restatement of oracle/losses.py over the [P, C] tensor -> (12 scalars as the kernel lays them out, dL/dz)."""
    z = torch.from_numpy(zq.astype(np.float64)).requires_grad_(True)
    yt = torch.from_numpy(y.astype(np.float64))
    p = torch.sigmoid(z)
    w = weights
    terms = [olosses.binary_crossentropy(yt, p), olosses.dice_loss(yt, p), olosses.iou_loss(yt, p), olosses.jaccard_loss(yt, p),
             olosses.focal_loss(yt, p)]
    loss = sum(wi * t for wi, t in zip(w, terms) if wi)
    loss.backward()
    pd = p.detach().numpy()
    t = (pd > 0.5).astype(np.float64)
    sp, sy, spy = pd.sum(), y.sum(), (pd * y).sum()
    loss, terms = loss.detach(), [t.detach() for t in terms]
    sc = np.array([float(loss), float(terms[0]), float(terms[1]), (2 * (t * y).sum() + 1) / (sy + t.sum() + 1), (t == y).mean(),
                   sp, sy, spy, 1 - float(terms[2]), ((t * y).sum() + 1) / (sy + t.sum() - (t * y).sum() + 1),
                   float(terms[3]), float(terms[4])])
    return sc, z.grad.numpy(), pd


def make_case(P, C, ldc, seed, target="random"):
    rng = np.random.RandomState(seed)
    z = np.zeros((P, ldc), np.float32)
    z[:, :C] = rng.randn(P, C).astype(np.float32) * 3.0
    z[:, C:] = 1e4                                          # channels past `classes` must not be read into the loss
    if target == "zeros":
        y = np.zeros((P, C), np.float64)
    elif target == "ones":
        y = np.ones((P, C), np.float64)
    else:
        y = (rng.rand(P, C) < 0.4).astype(np.float64)
    bits = (y.astype(np.uint8) << np.arange(C, dtype=np.uint8)[None, :]).sum(axis=1).astype(np.uint8)
    return z, y, bits


def quantise(z, dtype):
    return torch.from_numpy(z).to(TD[dtype]).to(torch.float32).numpy()


def check(dtype, P, C, ldc, dlc, mix, target="random", seed=0, grad_scale=1.0):
    z, y, bits = make_case(P, C, ldc, seed, target)
    sc, g, _ws, _ = run_loss(dtype, z, bits, C, ldc, dlc, WEIGHTS[mix], grad_scale)
    zq = quantise(z, dtype)[:, :C]
    ref, gref, pd = reference(zq, y, WEIGHTS[mix])
    # thresholded metrics: a probability within rounding of 0.5 may fall either way (two flips)
    near = int((np.abs(pd - 0.5) < 1e-5).sum())
    flip = (2 + near) * 2.0 / (2.0 * y.sum() + 1.0)
    for i, name in enumerate(("loss", "bce", "dice_loss", "dice", "acc", "sum_p", "sum_y", "sum_py", "iou", "iot", "jaccard", "focal")):
        tol = 1e-5 * max(1.0, abs(ref[i]))
        if name in ("dice", "iot"):
            tol += flip
        elif name == "acc":
            tol += (2 + near) / float(P * C)
        elif name in ("sum_p", "sum_py"):
            tol = 1e-5 * max(1.0, abs(ref[i]))
        assert abs(sc[i] - ref[i]) <= tol, (name, sc[i], ref[i])
    gs = gref * grad_scale
    scale = np.abs(gs).max() + 1e-30
    rel = {"fp32": 1e-5, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}[dtype]
    err = np.abs(g[:, :C] - gs)
    # the 1e-7 probability clip passes no gradient outside [eps, 1 - eps]: an element whose float32 probability lies within its rounding
    # of a clip bound (|z| ~ 16) may fall on the other side than the float64 one - at most a handful in 4M elements
    edge = (np.abs(pd - 1e-7) < 1e-13) | (np.abs(pd - (1.0 - 1e-7)) < 1.2e-7)
    ok = err <= rel * np.abs(gs) + 2e-5 * scale
    assert (ok | edge).all(), (err[~(ok | edge)].max(), scale)
    assert edge.sum() <= max(8, 1e-5 * edge.size), edge.sum()
    assert (g[:, C:] == 0).all(), "padding channels must be exactly zero"
    return sc, g


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", [2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("P", [1, 255, 4097, 50 * 1024 + 5])      # (the last: 50 value workgroups - the finalize reduction's prefetched loop and its remainder)
def test_multilabel_loss_matches_reference(dtype, C, P):
    mix = ("bce", "bce+dice", "all")[(C + P) % 3]
    gsc = 1024.0 if dtype == "fp16" else 1.0                      # (IEEE half: the loss scale keeps 1/(P*C) gradients normal)
    check(dtype, P, C, C, C, mix, seed=C * 31 + P, grad_scale=gsc)           # unpadded rows: element / 8-byte access
    check(dtype, P, C, 8, 8, mix, seed=C * 31 + P + 1, grad_scale=gsc)       # the padded rows of the plan: 16-byte access


@pytest.mark.parametrize("mix", ["bce", "bce+dice", "all"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_multilabel_loss_weight_mixes_and_padded_16(dtype, mix):
    check(dtype, 3000, 4, 4, 16, mix, seed=7)
    check(dtype, 3000, 8, 16, 16, mix, seed=8)


@pytest.mark.parametrize("target", ["zeros", "ones"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_multilabel_loss_all_zero_and_all_one_targets(dtype, target):
    check(dtype, 5000, 4, 4, 8, "all", target=target, seed=3)


@pytest.mark.parametrize("dtype,C", [("bf16", 4), ("fp32", 3)])
def test_multilabel_loss_full_batch(dtype, C):
    """16 x 512 x 512 pixels: the value pass at its 1024-workgroup cap, the gradient pass at 2048."""
    check(dtype, 16 * 512 * 512, C, C, 8 if dtype == "bf16" else 4, "all", seed=11)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_multilabel_bias_grad_is_the_per_class_sum(dtype):
    lib, _ = lib_for(dtype)
    for P, C, dlc in ((255, 3, 8), (4097, 8, 8), (300000, 4, 8)):
        z, y, bits = make_case(P, C, C, P + C)
        _sc, g, ws, _keep = run_loss(dtype, z, bits, C, C, dlc, WEIGHTS["all"], grad_scale=1024.0 if dtype == "fp16" else 1.0)
        db = torch.full((C,), 5.0, dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        assert lib.stp_sigmoid_multilabel_bias_grad(ws.data_ptr(), P, C, db.data_ptr(), 0, st) == 0
        got = db.cpu().numpy().astype(np.float64)
        want = g[:, :C].astype(np.float64).sum(axis=0)
        np.testing.assert_allclose(got, want, atol=1e-5 * np.abs(g[:, :C]).sum(axis=0).max() + 1e-12)
        assert lib.stp_sigmoid_multilabel_bias_grad(ws.data_ptr(), P, C, db.data_ptr(), 1, st) == 0      # accumulate
        np.testing.assert_allclose(db.cpu().numpy().astype(np.float64), 2 * got, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_multilabel_grad_scale_is_linear_and_runs_are_bit_identical(dtype):
    z, y, bits = make_case(40000, 5, 8, 5)
    s1, g1, _, _ = run_loss(dtype, z, bits, 5, 8, 8, WEIGHTS["all"], 1.0)
    s2, g2, _, _ = run_loss(dtype, z, bits, 5, 8, 8, WEIGHTS["all"], 1.0)
    assert np.array_equal(s1, s2) and np.array_equal(g1, g2)              # deterministic two-stage reduction
    s3, g3, _, _ = run_loss(dtype, z, bits, 5, 8, 8, WEIGHTS["all"], 256.0)
    assert np.array_equal(s1, s3)                                           # the scalars do not carry the scale
    np.testing.assert_allclose(g3, 256.0 * g1, rtol=1e-6, atol=0)


def test_multilabel_loss_without_gradient_and_bad_arguments():
    lib, _lib = lib_for("fp32")
    z, y, bits = make_case(1000, 4, 4, 1)
    s_eval, g, _, _ = run_loss("fp32", z, bits, 4, 4, 4, WEIGHTS["bce+dice"], with_grad=False)
    s_train, _, _, _ = run_loss("fp32", z, bits, 4, 4, 4, WEIGHTS["bce+dice"])
    assert g is None and np.array_equal(s_eval, s_train)
    zd = torch.zeros((1000, 16), dtype=torch.float32, device="cuda")
    td = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    dl = torch.zeros((1000, 16), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    w5 = (ctypes.c_float * 5)(1, 1, 0, 0, 0)
    st = torch.cuda.current_stream().cuda_stream

    def call(classes, ldc, dlc, dtype=_lib.F32, nbytes=None):
        return lib.stp_sigmoid_multilabel_loss(zd.data_ptr(), td.data_ptr(), 1000, classes, ldc, dtype, w5, sc.data_ptr(), dl.data_ptr(),
                                               dlc, 1.0, ws.data_ptr(), ws.numel() * 4 if nbytes is None else nbytes, st)
    assert call(1, 8, 8) == STP_E_BADARG
    assert call(9, 16, 16) == STP_E_BADARG
    assert call(4, 3, 8) == STP_E_BADARG              # ldc < classes
    assert call(4, 4, 3) == STP_E_BADARG              # dl_channels < classes
    assert call(4, 4, 4, dtype=77) == STP_E_BADARG
    assert call(4, 4, 4, nbytes=16) == -3             # STP_E_WORKSPACE
    assert lib.stp_sigmoid_multilabel_bias_grad(ws.data_ptr(), 1000, 1, sc.data_ptr(), 0, st) == STP_E_BADARG
    assert lib.stp_sigmoid_multilabel_bias_grad(ws.data_ptr(), 1000, 9, sc.data_ptr(), 0, st) == STP_E_BADARG
    assert call(4, 4, 4) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ whole training step
def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


def overlapping_discs(n, size, classes, seed):
    """uint8 images and [n, size, size, classes] {0,1} masks of overlapping discs (a pixel may carry several classes, or none)."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    x = (rng.rand(n, size, size, 3) * 60).astype(np.uint8)
    y = np.zeros((n, size, size, classes), np.uint8)
    for i in range(n):
        for c in range(classes):
            for _ in range(2):
                cy, cx, r = rng.randint(0, size), rng.randint(0, size), rng.randint(size // 8, size // 3)
                d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
                y[i, :, :, c] |= d.astype(np.uint8)
                x[i][d] = np.minimum(255, x[i][d].astype(np.int32) + 40 * (c + 1)).astype(np.uint8)
    return x, y


INIT = {"Unet": onets.init_unet_resnet, "Linknet": onets.init_linknet_resnet, "FPN": onets.init_fpn_resnet,
        "PSPNet": onets.init_pspnet_resnet}


def batch_statistics_as_moving(tr, x):
    """``tr``'s parameters with every BatchNormalization moving mean / variance replaced by the statistics of a training-phase pass of
    its network over ``x`` (batch mean, unbiased batch variance): the training pass blends them into zeroed moving statistics."""
    P = dict(tr.P)
    for k in P:
        if k.endswith(("/moving_mean", "/moving_variance")):
            P[k] = np.zeros_like(P[k])
    with torch.no_grad():
        _, upd = tr._forward(onets.to_torch(P), torch.from_numpy(x.astype(np.float32)), True, None)
    for k, v in upd.items():
        P[k] = (v.numpy().astype(np.float64) / (1.0 - onets.BN_MOMENTUM)).astype(np.float32)
    return P


@pytest.mark.parametrize("arch,backbone,classes,n,size,latol,gtol", [
    ("Unet", "resnet34", 4, 2, 64, 1e-3, 3e-2),
    ("Linknet", "resnet34", 3, 2, 64, 1e-3, 3e-2),
    ("FPN", "resnet50", 4, 1, 128, 2e-3, 6e-2),
    ("PSPNet", "resnet101", 3, 2, 96, 1e-3, 6e-2)])
def test_fp32_multilabel_step_matches_oracle(arch, backbone, classes, n, size, latol, gtol):
    P = INIT[arch](backbone, classes=classes, seed=42)
    x, y = overlapping_discs(n, size, classes, seed=5)
    spec = "binary_crossentropy+1.0*dice_loss"
    tr = ostep.OracleTrainer(P, backbone=backbone, loss=spec, optimizer="sgd", lr=0.02, architecture=arch, activation="sigmoid")
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel(arch, backbone, (size, size, 3), classes, "sigmoid", batch=n, dtype="fp32", loss=spec, optimizer="SGD", lr=0.02,
                    use_graph=False)
    assert m.multilabel and m.head_activation == "sigmoid"
    assert sorted(m.get_weights()) == sorted(P)
    m.set_weights(P)
    o = tr.step(x.astype(np.float32), y.astype(np.float32))
    met = m.train_on_batch(x, y)
    assert "binary_crossentropy" in met and "categorical_crossentropy" not in met
    np.testing.assert_allclose(m.logits(), o["logits"], atol=latol)
    assert abs(met["dice_loss"] - o["dice_loss"]) < 1e-5
    assert abs(met["loss"] - o["loss"]) < 2e-5 * max(1.0, abs(o["loss"]))
    assert abs(met["binary_crossentropy"] - o["bce"]) < 1e-5
    flips = 2 * 2.0 / (2.0 * float(y.sum()) + 1.0)
    assert abs(met["dice"] - o["dice"]) < 1e-5 + flips
    g = m.get_gradients()
    for k, ref in o["grads"].items():
        e = rel_l2(g[k], ref)
        assert e <= (1e-4 if k.startswith("final_conv") else gtol), "grad %s: rel L2 %.3g" % (k, e)
    # inference: C independent sigmoids, on the updated weights with moving statistics that normalise: the batch statistics of the
    # updated network on ANOTHER batch (a forward normalised by x's own statistics misses the bar on > 99 % of the values of every case).
    # The moving statistics one step leaves behind are still ~ their initial (0, 1): FPN/ResNet50's inference logits then reach 2.6e4,
    # only 0.2 % of them lie within +-10, and those carry the fp32 summation-order noise of that range - there the fp32 oracle is itself
    # 5.3e-3 off a float64 evaluation of the same weights.  Here its logits stay within +-16, 83 % of its sigmoids in (1e-3, 1 - 1e-3).
    x2, _ = overlapping_discs(n, size, classes, seed=6)
    tr.P = batch_statistics_as_moving(tr, x2)
    m.set_weights(tr.P)
    pr = m.predict(x)
    ref = 1.0 / (1.0 + np.exp(-tr.forward(x.astype(np.float32)).astype(np.float64)))
    assert pr.shape == (n, size, size, classes)
    # (the logit bar of the step, x 2.5 for FPN/ResNet50's batch of one)
    np.testing.assert_allclose(pr, ref, atol=1e-3 if latol <= 1e-3 else 2.5 * latol)


def test_bf16_multilabel_step_close_to_storage_quantised_oracle():
    """bf16 storage: against the oracle that rounds at the same points (storage="bf16"), at the bars of the 16-bit tests."""
    n, size, classes = 2, 64, 4
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = overlapping_discs(n, size, classes, seed=9)
    spec = "binary_crossentropy+1.0*dice_loss"
    tr = ostep.OracleTrainer(P, backbone="resnet18", loss=spec, optimizer="adam", lr=1e-3, activation="sigmoid", storage="bf16")
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "sigmoid", batch=n, dtype="bf16", loss=spec, optimizer="Adam", lr=1e-3,
                    use_graph=False)
    m.set_weights(P)
    o = tr.step(x.astype(np.float32), y.astype(np.float32))
    met = m.train_on_batch(x, y)
    ref = o["logits"]
    err = np.abs(m.logits() - ref)
    rng_ = np.abs(ref).max()
    assert err.mean() < 0.01 * rng_ and err.max() < 0.1 * rng_, (err.max(), err.mean(), rng_)
    assert abs(met["loss"] - o["loss"]) < 1e-2 and abs(met["dice_loss"] - o["dice_loss"]) < 5e-3
    g = m.get_gradients()
    for k in ("final_conv/kernel", "final_conv/bias"):
        a, b = g[k].ravel().astype(np.float64), o["grads"][k].ravel().astype(np.float64)
        assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30) > 0.99, k
    losses = [met["loss"]] + [m.train_on_batch(x, y)["loss"] for _ in range(6)]
    assert losses[-1] < losses[0]


def test_fp16_multilabel_step_under_default_loss_scale():
    n, size, classes = 2, 64, 3
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = overlapping_discs(n, size, classes, seed=13)
    spec = "binary_crossentropy+1.0*dice_loss"
    tr = ostep.OracleTrainer(P, backbone="resnet18", loss=spec, optimizer="adam", lr=1e-3, activation="sigmoid")
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "sigmoid", batch=n, dtype="fp16", loss=spec, optimizer="Adam", lr=1e-3,
                    use_graph=True)
    assert m.loss_scale == 16384.0
    m.set_weights(P)
    o = tr.step(x.astype(np.float32), y.astype(np.float32))
    met = m.train_on_batch(x, y)
    ref = o["logits"]
    err = np.abs(m.logits() - ref)
    rng_ = np.abs(ref).max()
    assert err.mean() < 0.005 * rng_ and err.max() < 0.05 * rng_, (err.max(), err.mean(), rng_)
    assert abs(met["loss"] - o["loss"]) < 3e-3 and abs(met["dice_loss"] - o["dice_loss"]) < 2e-3
    assert m.skipped_steps == 0
    g = m.get_gradients()
    for k, r in o["grads"].items():
        assert np.isfinite(g[k]).all(), k
    a, b = g["final_conv/kernel"].ravel().astype(np.float64), o["grads"]["final_conv/kernel"].ravel().astype(np.float64)
    assert a @ b / (np.linalg.norm(a) * np.linalg.norm(b)) > 0.999


def test_multilabel_bias_gradient_rides_in_the_loss_kernel():
    """U-Net's class convolution reads its C bias gradients from the loss workspace (no stp_channel_sum over the padded gradient)."""
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel("Unet", "resnet18", (64, 64, 3), 4, "sigmoid", batch=2, dtype="bf16", loss="binary_crossentropy", use_graph=False)
    names = [name for _fn, _a, name, _m in m.plan.bwd if name]
    assert "stp_sigmoid_multilabel_bias_grad" in names
    fwd = [name for _fn, _a, name, _m in m.plan.fwd if name]
    assert "stp_sigmoid_multilabel_loss" in fwd and "stp_softmax_cce_dice" not in fwd and "stp_sigmoid_bce_dice" not in fwd


# ------------------------------------------------------------------------------------------ the 1-class path is unchanged
@pytest.mark.parametrize("loss", ["binary_crossentropy+1.0*dice_loss", "binary_crossentropy+0.5*focal_loss"])
def test_one_class_sigmoid_plan_keeps_its_launches_and_scalars(loss):
    from segmentation_training_pipeline_amd import graph, nets
    from segmentation_training_pipeline_amd.backend import HipSegModel, parse_loss
    m = HipSegModel("Unet", "resnet18", (64, 64, 3), 1, "sigmoid", batch=2, dtype="bf16", loss=loss, use_graph=False)
    assert not m.multilabel
    names = [name for _fn, _a, name, _m in m.plan.fwd + m.plan.bwd if name]
    assert "stp_sigmoid_multilabel_loss" not in names and "stp_sigmoid_multilabel_bias_grad" not in names
    assert "stp_sigmoid_loss_bias_grad" in names
    # the same network declared directly with sigmoid_loss (what the 1-class head always emitted): same launch list, same scalars
    ref = graph.Plan(2, "bf16", "cuda", training=True)
    ref.define(lambda plan: nets.unet_resnet(plan, "resnet18", 64, 64, 3, 1, (256, 128, 64, 32, 16), parse_loss(loss)))
    assert [n for _f, _a, n, _m in ref.fwd + ref.bwd] == [n for _f, _a, n, _m in m.plan.fwd + m.plan.bwd]
    x, y = ostep.synthetic_batch(2, 64, 64, seed=4)
    P = onets.init_unet_resnet("resnet18", seed=4)
    m.set_weights(P)
    a = m.train_on_batch(x, y)
    m2 = HipSegModel("Unet", "resnet18", (64, 64, 3), 1, "sigmoid", batch=2, dtype="bf16", loss=loss, use_graph=False)
    m2.set_weights(P)
    b = m2.train_on_batch(x, y)
    assert a == b


# ------------------------------------------------------------------------------------------ end to end
YAML = """
backbone: resnet18
architecture: Unet
classes: 3
activation: sigmoid
encoder_weights:
shape: [64, 64, 3]
batch: 4
lr: 0.005
optimizer: Adam
loss: binary_crossentropy+dice_loss
metrics: [binary_accuracy, dice]
primary_metric: val_dice
primary_metric_mode: max
folds_count: 2
random_state: 7
dtype: fp32
draw_examples: false
augmentation:
  Fliplr: 0.5
  Flipud: 0.5
  Affine:
    rotate: [-10, 10]
stages:
  - epochs: 4
"""


class DiscSet(object):
    """Ad-hoc dataset: overlapping synthetic discs with H x W x 3 {0,1} masks."""

    def __init__(self, n, size=64, classes=3, seed=0):
        self.x, self.y = overlapping_discs(n, size, classes, seed)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        from segmentation_pipeline.impl.datasets import PredictionItem
        return PredictionItem("disc%03d.png" % i, self.x[i], self.y[i])


def heldout_dice(model, x, y):
    """Dice of one held-out batch under batch statistics (forward + backward, no update): independent of how far the
    moving BatchNormalization statistics have caught up after a few steps."""
    impl = model.impl
    impl.load_batch(x, y)
    impl.forward_backward()
    return impl.metrics()["dice"]


def test_multilabel_yaml_experiment_end_to_end(tmp_path):
    import csv

    from PIL import Image

    from segmentation_pipeline import segmentation
    cfgp = tmp_path / "ml.yaml"
    cfgp.write_text(YAML)
    cfg = segmentation.parse(str(cfgp))
    held = DiscSet(4, seed=99)
    untrained = cfg._compiled(cfg.stages[0], use_graph=False)
    d_untrained = heldout_dice(untrained, held.x, held.y)
    cfg.fit(DiscSet(48, seed=1), foldsToExecute=[0])
    with open(cfg.metricsPath(0, 0)) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 4
    assert "binary_crossentropy" in rows[0] and "val_binary_crossentropy" in rows[0]
    assert "categorical_crossentropy" not in rows[0] and "lovasz_loss" not in rows[0]
    assert float(rows[-1]["loss"]) < float(rows[0]["loss"])
    m = cfg.load_model(0, 0)
    assert m.impl.multilabel
    assert heldout_dice(m, held.x, held.y) > d_untrained
    # predictions: one PNG per class
    src = tmp_path / "imgs"
    src.mkdir()
    for i in range(2):
        Image.fromarray(held.x[i]).save(str(src / ("im%d.png" % i)))
    out = tmp_path / "pred"
    cfg.predict_to_directory(str(src), str(out), fold=0, stage=0, batchSize=4)
    assert sorted(os.listdir(str(out))) == sorted("im%d_%d.png" % (i, c) for i in range(2) for c in range(3))


def test_multilabel_graph_replay_equals_eager():
    from segmentation_training_pipeline_amd.backend import HipSegModel
    n, size, classes = 2, 64, 3
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = overlapping_discs(n, size, classes, seed=21)
    out = []
    for use_graph in (False, True):
        m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "sigmoid", batch=n, dtype="bf16",
                        loss="binary_crossentropy+dice_loss+0.5*jaccard_loss", use_graph=use_graph)
        m.set_weights(P)
        mets = [m.train_on_batch(x, y) for _ in range(2)]
        out.append((mets, m.get_weights()))
    assert out[0][0] == out[1][0]
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
