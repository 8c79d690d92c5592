"""CPU reference of the squeeze-and-excitation operator and of the SE-ResNet-18/34 encoders (helper of tests/test_se_*.py; not collected).

The reference does not pin the arithmetic of classification_models' `seresnet18/34` (that package is not vendored): it is fixed by this
repository - include/stp_hip.h, stp_se_* - and restated here twice:

* ``se_forward64`` / ``se_backward64``: float64 numpy, for the op-level tests;
* ``se_resnet_encoder``: oracle.nets._resnet_encoder with the gate on the residual branch of every basic unit (conv2 STORED, then
  z / h / s in fp32, then the one rounding of u * s + shortcut).  ``install(monkeypatch)`` puts it in place of
  oracle.nets._resnet_encoder for the duration of a test, so that the unchanged OracleTrainer - called with backbone 'resnet18' /
  'resnet34' and the SE tensors added to its parameters - steps U-Net, Linknet, FPN and PSPNet over the SE encoders.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import nets as onets

BASE = {"seresnet18": "resnet18", "seresnet34": "resnet34"}
REDUCTION = 16


# ------------------------------------------------------------------------------------------------ float64 numpy
def se_forward64(u, sc, W1, b1, W2, b2):
    """u, sc [N,H,W,C]; W1 [C,R], b1 [R], W2 [R,C], b2 [C] -> z, h, s, x (float64)."""
    u, sc = u.astype(np.float64), sc.astype(np.float64)
    z = u.mean(axis=(1, 2))
    h = np.maximum(z @ W1.astype(np.float64) + b1.astype(np.float64), 0.0)
    s = 1.0 / (1.0 + np.exp(-(h @ W2.astype(np.float64) + b2.astype(np.float64))))
    return z, h, s, u * s[:, None, None, :] + sc


def se_backward64(dx, u, W1, W2, z, h, s):
    """-> dict(ds, da2, da1, dz, dW1, db1, dW2, db2, du), float64; the shortcut's gradient is dx itself."""
    dx, u = dx.astype(np.float64), u.astype(np.float64)
    W1, W2 = W1.astype(np.float64), W2.astype(np.float64)
    hw = u.shape[1] * u.shape[2]
    ds = (dx * u).sum(axis=(1, 2))
    da2 = ds * s * (1.0 - s)
    dh = da2 @ W2.T
    da1 = dh * (h > 0)
    dz = da1 @ W1.T
    return dict(ds=ds, da2=da2, da1=da1, dz=dz, dW1=z.T @ da1, db1=da1.sum(0), dW2=h.T @ da2, db2=da2.sum(0),
                du=dx * s[:, None, None, :] + dz[:, None, None, :] / hw)


# ------------------------------------------------------------------------------------------------ oracle parameters
def se_names(P):
    return [k for k in P if "_se_fc" in k]


def add_se_params(P, seed=7, b2_range=0.0):
    """Adds the four SE tensors of every basic unit whose conv2 is in ``P`` (Keras Conv2D(1x1, use_bias=True) layouts): he_uniform
    kernels, zero biases - the model's own initialisation - or, with ``b2_range`` > 0, fc2 biases uniform in +-b2_range (gates spread
    over (0.05, 0.95) instead of sitting near 0.5) and small non-zero fc1 biases."""
    rng = np.random.RandomState(seed)
    out = type(P)(P)
    for k in list(P):
        if k.startswith("stage") and k.endswith("_conv2/kernel"):
            pre = k[:-len("conv2/kernel")]
            c = int(P[k].shape[3])
            r = c // REDUCTION
            out[pre + "se_fc1/kernel"] = rng.uniform(-np.sqrt(6.0 / c), np.sqrt(6.0 / c), size=(1, 1, c, r)).astype(np.float32)
            out[pre + "se_fc1/bias"] = (rng.uniform(-0.2, 0.2, size=r) if b2_range else np.zeros(r)).astype(np.float32)
            out[pre + "se_fc2/kernel"] = rng.uniform(-np.sqrt(6.0 / r), np.sqrt(6.0 / r), size=(1, 1, r, c)).astype(np.float32)
            out[pre + "se_fc2/bias"] = (rng.uniform(-b2_range, b2_range, size=c) if b2_range else np.zeros(c)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ oracle encoder
def _gate(ctx, u, shortcut, pre):
    """The operator on NCHW torch tensors: fp32 z / h / s, ONE rounding of u * s + shortcut."""
    P = ctx.P
    c = u.shape[1]
    z = u.mean(dim=(2, 3))
    h = F.relu(z @ P[pre + "se_fc1/kernel"].reshape(c, -1) + P[pre + "se_fc1/bias"])
    s = torch.sigmoid(h @ P[pre + "se_fc2/kernel"].reshape(-1, c) + P[pre + "se_fc2/bias"])
    return ctx.st(u * s.view(s.shape[0], c, 1, 1) + shortcut)


def se_resnet_encoder(ctx, x_nhwc, backbone, stop_at=None):
    """oracle.nets._resnet_encoder (basic units only) with the gate before the Add of every unit."""
    units = onets.RESNET_UNITS[backbone]
    assert onets.expansion(backbone) == 1
    eps = onets.BN_EPS_ENCODER
    x = x_nhwc.permute(0, 3, 1, 2)
    x = onets._bn_apply(ctx, x, "bn_data", eps, relu=False)
    ctx.tap("bn_data", x)
    x = onets._conv(ctx, x, "conv0", stride=2, pad=3)
    ctx.tap("conv0", x)
    x = onets._bn_apply(ctx, x, "bn0", eps, relu=True)
    skips = {"relu0": x}
    ctx.tap("relu0", x)
    x = ctx.st(F.max_pool2d(F.pad(x, (1, 1, 1, 1)), kernel_size=3, stride=2))
    ctx.tap("pooling0", x)
    for s, (n_units, f) in enumerate(zip(units, onets.STAGE_FILTERS), start=1):
        for u in range(1, n_units + 1):
            pre = "stage%d_unit%d_" % (s, u)
            stride = 2 if (u == 1 and s > 1) else 1
            a = onets._bn_apply(ctx, x, pre + "bn1", eps, relu=True)
            if u == 1:
                skips[pre + "relu1"] = a
                ctx.tap(pre + "relu1", a)
                if stop_at == pre + "relu1":
                    return None, skips
                shortcut = onets._conv(ctx, a, pre + "sc", stride=stride, pad=0)
            else:
                shortcut = x
            y = onets._conv(ctx, a, pre + "conv1", stride=stride, pad=1)
            y = onets._bn_apply(ctx, y, pre + "bn2", eps, relu=True)
            y = onets._conv(ctx, y, pre + "conv2", stride=1, pad=1, store=True)       # u is a stored tensor of its own
            x = _gate(ctx, y, shortcut, pre)
            ctx.tap(pre + "out", x)
    x = onets._bn_apply(ctx, x, "bn1", eps, relu=True)
    ctx.tap("relu1", x)
    return x, skips


def install(monkeypatch):
    monkeypatch.setattr(onets, "_resnet_encoder", se_resnet_encoder)


def init(arch, backbone, seed=42, b2_range=0.0, **kw):
    """Oracle parameters of ``arch`` over the SE encoder ``backbone`` ('seresnet18' / 'seresnet34')."""
    fn = {"Unet": onets.init_unet_resnet, "Linknet": onets.init_linknet_resnet, "FPN": onets.init_fpn_resnet,
          "PSPNet": onets.init_pspnet_resnet}[arch]
    return add_se_params(fn(BASE[backbone], seed=seed, **kw), b2_range=b2_range)
