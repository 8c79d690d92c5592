"""iou_loss, jaccard_loss and focal_loss on the multi-class softmax head, on the GPU: the loss kernel stp_softmax_loss_ex against
float64 evaluations of oracle/losses.py on softmax probabilities and the one-hot target, one training step of each
segmentation_models graph against the oracle, the plain categorical_crossentropy+dice_loss plans left as they were, and a YAML
experiment end to end."""
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
#          categorical_crossentropy, dice_loss, iou_loss, jaccard_loss, focal_loss
WEIGHTS = {"cce": (1.0, 0, 0, 0, 0), "cce+dice": (1.0, 1.0, 0, 0, 0), "all": (1.0, 0.5, 0.3, 0.2, 2.0),
           "iou": (0, 0, 1.0, 0, 0), "jaccard": (0, 0, 0, 1.0, 0), "focal": (0, 0, 0, 0, 1.0)}
STP_E_BADARG, STP_E_WORKSPACE = -1, -3
CLASSES = [2, 3, 4, 5, 8, 9, 16, 17, 20, 24, 25, 32]          # both edges of every class bucket (4, 8, 16, 24, 32); 20: 8-byte rows


def lib_for(dtype):
    from segmentation_training_pipeline_amd import _lib
    return _lib.load("fp16" if dtype == "fp16" else "bf16"), _lib


def dt_code(_lib, dtype):
    return {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16}[dtype]


def run_loss(dtype, z, t, classes, ldc, dlc, weights, grad_scale=1.0, with_grad=True, guard=64, entry="stp_softmax_loss_ex"):
    """-> (scalars[12], dlogits [P, dlc] float32 or None, the gradient in its storage type).  ``z``: float32 [P, ldc] (rounded to the
    storage type here); the gradient buffer is filled with NaN, ``guard`` elements past its end must stay NaN."""
    lib, _lib = lib_for(dtype)
    P = z.shape[0]
    zd = torch.from_numpy(np.ascontiguousarray(z, np.float32)).to(TD[dtype]).cuda().contiguous()
    td = torch.from_numpy(np.ascontiguousarray(t, np.uint8)).cuda()
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    dl = torch.full((P * dlc + guard,), float("nan"), dtype=TD[dtype], device="cuda") if with_grad else None
    st = torch.cuda.current_stream().cuda_stream
    dlp = dl.data_ptr() if dl is not None else None
    if entry == "stp_softmax_loss_ex":
        w5 = (ctypes.c_float * 5)(*weights)
        rc = lib.stp_softmax_loss_ex(zd.data_ptr(), td.data_ptr(), P, classes, ldc, dt_code(_lib, dtype), w5, sc.data_ptr(), dlp, dlc,
                                     grad_scale, ws.data_ptr(), ws.numel() * 4, st)
    else:
        assert not any(weights[2:])
        rc = lib.stp_softmax_cce_dice(zd.data_ptr(), td.data_ptr(), P, classes, ldc, dt_code(_lib, dtype), weights[0], weights[1],
                                      sc.data_ptr(), dlp, dlc, grad_scale, ws.data_ptr(), ws.numel() * 4, st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    g, raw = None, None
    if dl is not None:
        full = dl.to(torch.float32).cpu().numpy()
        assert np.isnan(full[P * dlc:]).all(), "the gradient pass wrote past its tensor"
        g = full[:P * dlc].reshape(P, dlc)
        raw = dl[:P * dlc].cpu()
    return sc.cpu().numpy(), g, raw


def reference(zq, t, weights):
    """float64 evaluation of oracle/losses.py on p = softmax(z) and the one-hot target over the [P, C] tensor ->
    (12 scalars as the kernel lays them out, dL/dz by autograd, p)."""
    z = torch.from_numpy(zq.astype(np.float64)).requires_grad_(True)
    y = np.eye(zq.shape[1], dtype=np.float64)[t]
    yt = torch.from_numpy(y)
    p = torch.softmax(z, dim=-1)
    terms = [olosses.categorical_crossentropy(yt, p), olosses.dice_loss(yt, p), olosses.iou_loss(yt, p), olosses.jaccard_loss(yt, p),
             olosses.focal_loss(yt, p)]
    loss = sum(wi * term for wi, term in zip(weights, terms) if wi)
    loss.backward()
    pd = p.detach().numpy()
    th = (pd > 0.5).astype(np.float64)
    sp, sy, spy = pd.sum(), y.sum(), (pd * y).sum()
    loss, terms = loss.detach(), [term.detach() for term in terms]
    # slots 3, 4, 9 as softmax_loss_finalize_kernel defines them: dice / accuracy / iou of the thresholded probabilities over every element
    sc = np.array([float(loss), float(terms[0]), float(terms[1]), (2 * (th * y).sum() + 1) / (sy + th.sum() + 1), (th == y).mean(),
                   sp, sy, spy, 1 - float(terms[2]), ((th * y).sum() + 1) / (sy + th.sum() - (th * y).sum() + 1),
                   float(terms[3]), float(terms[4]) if weights[4] else 0.0])
    # (slot 11 is documented as 0 when focal_loss has no weight - include/stp_hip.h: its class loop is skipped - and the name then
    #  leaves metrics() and the epoch log: test_unweighted_focal_loss_is_not_logged)
    return sc, z.grad.numpy(), pd


def make_case(P, C, ldc, seed, target="random"):
    rng = np.random.RandomState(seed)
    z = np.zeros((P, ldc), np.float32)
    z[:, :C] = rng.randn(P, C).astype(np.float32) * 2.0
    z[:, C:] = 1e4                                          # channels past `classes` must not be read into the loss
    if target == "first":
        t = np.zeros(P, np.uint8)
    elif target == "last":
        t = np.full(P, C - 1, np.uint8)
    else:
        t = rng.randint(0, C, P).astype(np.uint8)
    return z, t


def quantise(z, dtype):
    return torch.from_numpy(z).to(TD[dtype]).to(torch.float32).numpy()


def check(dtype, P, C, ldc, dlc, mix, target="random", seed=0, grad_scale=1.0):
    z, t = make_case(P, C, ldc, seed, target)
    ref, gref, pd = reference(quantise(z, dtype)[:, :C], t, WEIGHTS[mix])
    sc, g, _raw = run_loss(dtype, z, t, C, ldc, dlc, WEIGHTS[mix], grad_scale)
    y = np.eye(C)[t]
    # thresholded metrics: a probability within rounding of 0.5 may fall either way (two flips)
    near = int((np.abs(pd - 0.5) < 1e-5).sum())
    flip = (2 + near) * 2.0 / (2.0 * y.sum() + 1.0)
    for i, name in enumerate(("loss", "cce", "dice_loss", "dice", "acc", "sum_p", "sum_y", "sum_py", "iou", "iot", "jaccard", "focal")):
        tol = 1e-5 * max(1.0, abs(ref[i]))
        if name in ("dice", "iot"):
            tol += flip
        elif name == "acc":
            tol += (2 + near) / float(P * C)
        print("%s P=%d C=%d ldc=%d %s %-9s got %.9g ref %.9g tol %.3g" % (dtype, P, C, ldc, mix, name, sc[i], ref[i], tol))
        assert abs(sc[i] - ref[i]) <= tol, (name, sc[i], ref[i])
    gs = gref * grad_scale
    scale = np.abs(gs).max() + 1e-30
    rel = {"fp32": 1e-5, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}[dtype]
    err = np.abs(g[:, :C] - gs)
    # the 1e-7 probability clip passes no gradient outside [eps, 1 - eps]: an element whose float32 probability lies within its rounding
    # of a clip bound may fall on the other side than the float64 one.  The cap is a condition: with logits of scale 2 the reference has
    # no such element at any of the sizes below.
    # The largest error over the largest gradient is printed below before the assertion; the bar is the issue's.
    edge = (np.abs(pd - 1e-7) < 1e-13) | (np.abs(pd - (1.0 - 1e-7)) < 1.2e-7)
    ok = err <= rel * np.abs(gs) + 2e-5 * scale
    print("   gradient: max err / scale %.3g, edge elements %d" % ((err / scale).max(), edge.sum()))
    assert (ok | edge).all(), (err[~(ok | edge)].max(), scale)
    assert edge.sum() <= max(8, 1e-5 * edge.size), edge.sum()
    assert (g[:, C:] == 0).all(), "padding channels must be exactly zero"
    return sc, g


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("P", [1, 255, 4097, 50 * 1024 + 5])      # (the last: 50 value workgroups - the finalize reduction's prefetched loop and its remainder)
def test_softmax_loss_ex_matches_reference(dtype, C, P):
    mix = ("cce", "cce+dice", "all")[(C + P) % 3]
    gsc = 1024.0 if dtype == "fp16" else 1.0                      # (IEEE half: the loss scale keeps 1/(P*C) gradients normal)
    pad = (C // 8 + 1) * 8                                        # the next multiple of 8: 16-byte rows
    check(dtype, P, C, C, C, mix, seed=C * 31 + P, grad_scale=gsc)
    check(dtype, P, C, pad, pad, mix, seed=C * 31 + P + 1, grad_scale=gsc)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("mix", ["iou", "jaccard", "focal"])
def test_softmax_loss_ex_each_new_term_alone(dtype, mix):
    gsc = 1024.0 if dtype == "fp16" else 1.0
    for C, ldc, dlc in ((3, 3, 8), (20, 20, 24), (5, 8, 8)):
        check(dtype, 3001, C, ldc, dlc, mix, seed=C + len(mix), grad_scale=gsc)


@pytest.mark.parametrize("mix", ["all", "focal"])
@pytest.mark.parametrize("C", [3, 20])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_softmax_loss_ex_all_terms_at_every_class_count_of_the_workloads(dtype, C, mix):
    check(dtype, 4097, C, C, (C // 8 + 1) * 8, mix, seed=C + 100)


@pytest.mark.parametrize("target", ["first", "last"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_softmax_loss_ex_single_class_targets(dtype, target):
    check(dtype, 5000, 4, 4, 8, "all", target=target, seed=3)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_softmax_loss_ex_large(dtype):
    """1.2M pixels: the value pass past its 1024-workgroup cap (each workgroup walks its range), the gradient pass at its cap."""
    check(dtype, 1_200_000, 3, 3, 8 if dtype == "bf16" else 4, "all", seed=11)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_softmax_loss_ex_grad_scale_is_linear_and_runs_are_bit_identical(dtype):
    z, t = make_case(40000, 5, 8, 5)
    s1, g1, _ = run_loss(dtype, z, t, 5, 8, 8, WEIGHTS["all"], 1.0)
    s2, g2, _ = run_loss(dtype, z, t, 5, 8, 8, WEIGHTS["all"], 1.0)
    assert np.array_equal(s1, s2) and np.array_equal(g1, g2)              # deterministic two-stage reduction
    s3, g3, _ = run_loss(dtype, z, t, 5, 8, 8, WEIGHTS["all"], 256.0)
    assert np.array_equal(s1, s3)                                           # the scalars do not carry the scale
    np.testing.assert_allclose(g3, 256.0 * g1, rtol=1e-6, atol=0)


def ordered_bits(x):
    """The storage words of a float tensor as integers that grow with the value (one step = one ulp)."""
    b = x.view({2: torch.int16, 4: torch.int32}[x.element_size()]).numpy().astype(np.int64)
    lo = -(1 << (8 * x.element_size() - 1))
    return np.where(b < 0, lo - b, b)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("C,ldc,dlc", [(3, 3, 8), (4, 4, 4), (5, 8, 8), (20, 20, 24), (32, 32, 32)])
def test_softmax_loss_ex_with_cce_and_dice_only_is_stp_softmax_cce_dice(dtype, C, ldc, dlc):
    gsc = 1024.0 if dtype == "fp16" else 1.0
    z, t = make_case(20000, C, ldc, C)
    for mix in ("cce", "cce+dice"):
        s_new, g_new, raw_new = run_loss(dtype, z, t, C, ldc, dlc, WEIGHTS[mix], gsc)
        s_old, g_old, raw_old = run_loss(dtype, z, t, C, ldc, dlc, WEIGHTS[mix], gsc, entry="stp_softmax_cce_dice")
        # within 1e-6 - and within one float32 ulp: both finalize kernels sum the same per-workgroup partials in double (in two different
        # fixed orders) and round once
        for i in range(10):
            assert abs(s_new[i] - s_old[i]) <= min(1e-6 * max(1.0, abs(s_old[i])), np.spacing(np.float32(abs(s_old[i])))), (i, s_new[i], s_old[i])
        assert s_new[10] > 0 and s_new[11] == 0                            # jaccard_loss rides along; focal_loss has no weight: not evaluated
        d = np.abs(ordered_bits(raw_new) - ordered_bits(raw_old))
        print(dtype, C, mix, "max ulp distance", d.max())
        assert d.max() <= 1


def test_softmax_loss_ex_without_gradient_and_bad_arguments():
    lib, _lib = lib_for("fp32")
    z, t = make_case(1000, 4, 4, 1)
    s_eval, g, _ = run_loss("fp32", z, t, 4, 4, 4, WEIGHTS["all"], with_grad=False)
    s_train, _, _ = run_loss("fp32", z, t, 4, 4, 4, WEIGHTS["all"])
    assert g is None and np.array_equal(s_eval, s_train)
    zd = torch.zeros((1000, 40), dtype=torch.float32, device="cuda")
    td = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    dl = torch.zeros((1000, 40), dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    w5 = (ctypes.c_float * 5)(1, 1, 1, 1, 1)
    st = torch.cuda.current_stream().cuda_stream

    def call(classes, ldc, dlc, dtype=_lib.F32, nbytes=None, lib_=lib):
        return lib_.stp_softmax_loss_ex(zd.data_ptr(), td.data_ptr(), 1000, classes, ldc, dtype, w5, sc.data_ptr(), dl.data_ptr(),
                                        dlc, 1.0, ws.data_ptr(), ws.numel() * 4 if nbytes is None else nbytes, st)
    assert call(1, 8, 8) == STP_E_BADARG
    assert call(33, 40, 40) == STP_E_BADARG
    assert call(4, 3, 8) == STP_E_BADARG              # ldc < classes
    assert call(4, 4, 3) == STP_E_BADARG              # dl_channels < classes
    assert call(4, 4, 4, dtype=77) == STP_E_BADARG
    assert call(4, 4, 4, dtype=_lib.F16) == STP_E_BADARG                                   # the other build's 16-bit code
    assert call(4, 4, 4, dtype=_lib.BF16, lib_=lib_for("fp16")[0]) == STP_E_BADARG
    assert call(4, 4, 4, nbytes=16) == STP_E_WORKSPACE
    assert call(4, 4, 4) == 0 and call(32, 40, 40) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ whole training step
SPEC = "categorical_crossentropy+0.5*dice_loss+0.3*iou_loss+0.2*jaccard_loss+2.0*focal_loss"
PLAIN = "categorical_crossentropy+0.5*dice_loss"
INIT = {"Unet": onets.init_unet_resnet, "Linknet": onets.init_linknet_resnet, "FPN": onets.init_fpn_resnet,
        "PSPNet": onets.init_pspnet_resnet}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30)


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


def launch_names(m):
    return [name for _fn, _a, name, _m in m.plan.fwd + m.plan.bwd if name]


def oracle_terms(logits, y, classes):
    p = torch.softmax(torch.from_numpy(np.asarray(logits, np.float32)), dim=-1)
    oh = torch.nn.functional.one_hot(torch.from_numpy(y[..., 0].astype(np.int64)), classes).to(torch.float32)
    return {"jaccard_loss": float(olosses.jaccard_loss(oh, p)), "focal_loss": float(olosses.focal_loss(oh, p)),
            "iou_loss": float(olosses.iou_loss(oh, p))}


@pytest.mark.parametrize("arch,backbone,classes,n,size,latol,gtol", [
    ("Unet", "resnet34", 3, 2, 64, 1e-3, 3e-2),
    ("Linknet", "resnet34", 3, 2, 64, 1e-3, 3e-2),
    ("FPN", "resnet50", 3, 1, 128, 2e-3, 6e-2),
    ("PSPNet", "resnet101", 4, 2, 96, 1e-3, 6e-2)])
def test_fp32_extended_softmax_step_matches_oracle(arch, backbone, classes, n, size, latol, gtol):
    P = INIT[arch](backbone, classes=classes, seed=42)
    x, y = label_discs(n, size, classes, seed=5)
    tr = ostep.OracleTrainer(P, backbone=backbone, loss=SPEC, optimizer="sgd", lr=0.02, architecture=arch, activation="softmax")
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel(arch, backbone, (size, size, 3), classes, "softmax", batch=n, dtype="fp32", loss=SPEC, optimizer="SGD", lr=0.02,
                    use_graph=False)
    assert m.loss_w == (1.0, 0.5, 0.3, 0.2, 2.0, 0.0) and m.head_activation == "softmax" and not m.multilabel
    names = launch_names(m)
    assert names.count("stp_softmax_loss_ex") == 1 and "stp_softmax_cce_dice" not in names and "stp_softmax_cce_dice_up" not in names
    if arch in ("FPN", "PSPNet"):      # no low-resolution form of the extended loss: the resize and its gradient launch stay
        assert "stp_resize_bilinear" in names and "stp_resize_bilinear_bwd" in names
    m.set_weights(P)
    o = tr.step(x.astype(np.float32), y.astype(np.float32))
    met = m.train_on_batch(x, y)
    assert "categorical_crossentropy" in met and "binary_crossentropy" not in met and "lovasz_loss" not in met
    print(arch, "logits max err %.3g" % np.abs(m.logits() - o["logits"]).max(), "loss", met["loss"], o["loss"])
    np.testing.assert_allclose(m.logits(), o["logits"], atol=latol)
    assert abs(met["loss"] - o["loss"]) < 2e-5 * max(1.0, abs(o["loss"]))
    assert abs(met["dice_loss"] - o["dice_loss"]) < 1e-5 and abs(met["categorical_crossentropy"] - o["bce"]) < 1e-5
    terms = oracle_terms(o["logits"], y, classes)
    for k, v in terms.items():
        print("  ", k, met[k], v)
        assert abs(met[k] - v) < 1e-5, (k, met[k], v)
    g = m.get_gradients()
    for k, ref in o["grads"].items():
        e = rel_l2(g[k], ref)
        assert e <= (1e-4 if k.startswith("final_conv") else gtol), "grad %s: rel L2 %.3g" % (k, e)


@pytest.mark.parametrize("arch,backbone,classes,size", [("FPN", "resnet50", 3, 128), ("PSPNet", "resnet101", 4, 96)])
def test_plain_softmax_spec_keeps_the_low_resolution_fusion(arch, backbone, classes, size):
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel(arch, backbone, (size, size, 3), classes, "softmax", batch=1, dtype="fp32", loss=PLAIN, optimizer="SGD", use_graph=False)
    names = launch_names(m)
    assert names.count("stp_softmax_cce_dice_up") == 1 and "stp_softmax_loss_ex" not in names
    assert m.loss_w == (1.0, 0.5) and m.plan.loss_scalars.numel() == 12


def test_bf16_extended_softmax_step_close_to_storage_quantised_oracle():
    """bf16 storage: against the oracle that rounds at the same points (storage="bf16"), at the bars of the 16-bit tests."""
    n, size, classes = 2, 64, 3
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = label_discs(n, size, classes, seed=9)
    tr = ostep.OracleTrainer(P, backbone="resnet18", loss=SPEC, optimizer="adam", lr=1e-3, activation="softmax", storage="bf16")
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="bf16", loss=SPEC, optimizer="Adam", lr=1e-3,
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


def test_extended_softmax_graph_replay_is_bit_identical():
    from segmentation_training_pipeline_amd.backend import HipSegModel
    n, size, classes = 2, 64, 3
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    batches = [label_discs(n, size, classes, seed=21 + i) for i in range(2)]
    out = []
    for _ in range(2):
        m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="bf16", loss=SPEC, use_graph=True)
        m.set_weights(P)
        mets = [m.train_on_batch(x, y) for x, y in batches + batches]
        out.append((mets, m.logits(), m.get_weights()))
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1])
    for k in out[0][2]:
        assert np.array_equal(out[0][2][k], out[1][2][k]), k


def test_fp16_extended_softmax_step_under_default_loss_scale():
    n, size, classes = 2, 64, 3
    P = onets.init_unet_resnet("resnet18", classes=classes, seed=42)
    x, y = label_discs(n, size, classes, seed=13)
    from segmentation_training_pipeline_amd.backend import HipSegModel
    m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="fp16", loss=SPEC, optimizer="Adam", lr=1e-3,
                    use_graph=True)
    names = [name for _fn, _a, name, _m in m.plan.fwd if name]
    assert m.plan.dls is not None and m.loss_scale == 16384.0      # the default: static 2^14 and the dynamic multiplier on top,
    assert names[names.index("stp_softmax_loss_ex") + 1] == "stp_scale_by_device"      # which scales the gradient the loss launch wrote
    m.set_weights(P)
    met = m.train_on_batch(x, y)
    assert all(np.isfinite(v) for v in met.values()), met
    assert m.skipped_steps == 0
    for k, v in m.get_gradients().items():
        assert np.isfinite(v).all(), k
    assert np.isfinite(m.logits()).all()


def test_extended_softmax_rerun_loss_over_the_valid_prefix():
    """An evaluation batch with n_valid < N: Plan.rerun_loss gives the scalars of a launch over that prefix alone."""
    from segmentation_training_pipeline_amd.backend import HipSegModel
    n, size, classes = 4, 64, 3
    m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="fp32", loss=SPEC, use_graph=False)
    m.set_weights(onets.init_unet_resnet("resnet18", classes=classes, seed=42))
    x, y = label_discs(n, size, classes, seed=31)
    m.load_batch(x, y)
    m.forward_backward()
    full = m.plan.loss_scalars.cpu().numpy().copy()
    m.plan.rerun_loss(3)
    torch.cuda.synchronize()
    part = m.plan.loss_scalars.cpu().numpy().copy()
    assert not np.array_equal(part[:12], full[:12])
    # the same entry point over the first three samples of the plan's own logits and target
    lib, _lib = lib_for("fp32")
    lg, tg = m.plan.tensor("final_conv"), m.plan.inputs["mask"]
    rows = 3 * size * size
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
    w5 = (ctypes.c_float * 5)(*m.loss_w[:5])
    rc = lib.stp_softmax_loss_ex(lg.buf.data_ptr(), tg.buf.data_ptr(), rows, classes, lg.C, _lib.F32, w5, sc.data_ptr(), None, lg.gradC, 1.0,
                                 ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(sc.cpu().numpy()[:12], part[:12])
    # and they are the oracle's losses of those three samples
    terms = oracle_terms(m.logits()[:3], y[:3], classes)
    assert abs(part[10] - terms["jaccard_loss"]) < 1e-5 and abs(part[11] - terms["focal_loss"]) < 1e-5


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
loss: categorical_crossentropy+focal_loss
metrics: [dice]
primary_metric: val_focal_loss
primary_metric_mode: min
folds_count: 2
random_state: 7
dtype: fp32
draw_examples: false
stages:
  - epochs: 1
"""


def test_unweighted_focal_loss_is_not_logged(tmp_path):
    """stp_softmax_loss_ex skips focal_loss' class loops when the spec gives it no weight (scalar 11 is then 0): the name leaves
    metrics() and the epoch log, and a primary_metric that names it is refused before the first epoch."""
    from segmentation_pipeline import segmentation
    from segmentation_training_pipeline_amd.backend import HipSegModel
    n, size, classes = 2, 64, 3
    spec = "categorical_crossentropy+jaccard_loss"
    m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="fp32", loss=spec, use_graph=False)
    assert m.unevaluated_terms == ("focal_loss",)
    m.set_weights(onets.init_unet_resnet("resnet18", classes=classes, seed=42))
    x, y = label_discs(n, size, classes, seed=3)
    met = m.train_on_batch(x, y)
    assert "focal_loss" not in met and met["jaccard_loss"] > 0 and met["iou_loss"] > 0
    terms = oracle_terms(m.logits(), y, classes)
    assert abs(met["jaccard_loss"] - terms["jaccard_loss"]) < 1e-5
    weighted = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="fp32", loss=SPEC, use_graph=False)
    assert weighted.unevaluated_terms == ()
    cfgp = tmp_path / "nofocal.yaml"
    cfgp.write_text(YAML.replace("loss: categorical_crossentropy+focal_loss", "loss: " + spec))
    cfg = segmentation.parse(str(cfgp))
    with pytest.raises(ValueError, match="val_focal_loss"):
        cfg.fit(LabelSet(16, seed=1), foldsToExecute=[0])


class LabelSet(object):
    """Ad-hoc dataset: synthetic discs with H x W x 1 label images."""

    def __init__(self, n, size=64, classes=3, seed=0):
        self.x, self.y = label_discs(n, size, classes, seed)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        from segmentation_pipeline.impl.datasets import PredictionItem
        return PredictionItem("disc%03d.png" % i, self.x[i], self.y[i])


def test_extended_softmax_yaml_experiment_end_to_end(tmp_path):
    import csv

    from segmentation_pipeline import segmentation
    cfgp = tmp_path / "smx.yaml"
    cfgp.write_text(YAML)
    cfg = segmentation.parse(str(cfgp))
    out = cfg.fit(LabelSet(16, seed=1), foldsToExecute=[0])
    assert len(out) == 1 and np.isfinite(out[0]["val_focal_loss"])
    with open(cfg.metricsPath(0, 0)) as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 1
    for col in ("focal_loss", "val_focal_loss", "categorical_crossentropy", "val_categorical_crossentropy", "jaccard_loss", "iou_loss"):
        assert col in rows[0] and np.isfinite(float(rows[0][col])), col
    assert "lovasz_loss" not in rows[0] and "binary_crossentropy" not in rows[0]
    assert float(rows[0]["focal_loss"]) > 0
    assert os.path.getsize(cfg.weightsPath(0, 0)) > 0          # the best-weights file, chosen on val_focal_loss
