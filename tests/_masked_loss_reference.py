"""float64 evaluation of the masked softmax loss as include/stp_hip.h fixes it (stp_softmax_loss_masked); helper of
tests/test_masked_loss_host.py and tests/test_masked_loss_gpu.py, not collected.

    v_i = [t_i != ignore_label],  class of a counted pixel min(t_i, classes - 1),  omega_i = v_i w_class,  n = sum_i v_i
    categorical_crossentropy = sum_i omega_i ce_i / max(n, 1)      jaccard_loss = sum_i omega_i jac_i / max(n, 1)
    focal_loss = sum_i omega_i sum_c focal_ic / (max(n, 1) classes)
    dice_loss, iou_loss and the thresholded metrics: oracle/losses.py on the counted rows alone, no weights

The region terms ARE the oracle's functions applied to the counted rows.  The three means need the per-pixel value before the mean, so
their bodies are restated here line by line from oracle/losses.py with the mean replaced by the weighted sum;
test_masked_loss_host.py holds them to the oracle's functions where the two must agree (all weights 1)."""
import numpy as np
import torch

from oracle import losses as olosses

NAMES = ("loss", "cce", "dice_loss", "dice", "acc", "sum_p", "sum_y", "sum_py", "iou", "iot", "jaccard", "focal", "n", "sum_omega")


def cce_pixels(y, p):
    """oracle.losses.categorical_crossentropy before its mean."""
    eps = torch.tensor(olosses.KERAS_EPSILON)
    p = p / p.sum(dim=-1, keepdim=True)
    p = torch.clamp(p, eps, 1.0 - eps)
    return -(y * torch.log(p)).sum(dim=-1)


def jaccard_pixels(y, p, smooth=100.0):
    """oracle.losses.jaccard_loss before its mean."""
    inter = (y * p).abs().sum(dim=-1)
    tot = (y.abs() + p.abs()).sum(dim=-1)
    return (1.0 - (inter + smooth) / (tot - inter + smooth)) * smooth


def focal_elements(y, p, gamma=2.0, alpha=0.25):
    """oracle.losses.focal_loss before its two means (both run over the same elements, so their sum is the mean of this)."""
    eps = float(olosses.KERAS_EPSILON)
    pt1 = torch.clamp(torch.where(y == 1, p, torch.ones_like(p)), eps, 1.0 - eps)
    pt0 = torch.clamp(torch.where(y == 0, p, torch.zeros_like(p)), eps, 1.0 - eps)
    return -(alpha * (1.0 - pt1) ** gamma * torch.log(pt1)) - ((1.0 - alpha) * pt0 ** gamma * torch.log(1.0 - pt0))


def counted(t, ignore_label):
    t = np.asarray(t)
    return np.ones(t.shape, bool) if ignore_label is None or ignore_label < 0 else t != ignore_label


def terms(y, p, om):
    """The five terms on the counted rows y, p [n, C] (torch) with om [n] = omega of those rows."""
    n, C = p.shape
    d = float(max(n, 1))
    return [(om * cce_pixels(y, p)).sum() / d, olosses.dice_loss(y, p), olosses.iou_loss(y, p), (om * jaccard_pixels(y, p)).sum() / d,
            (om[:, None] * focal_elements(y, p)).sum() / (d * C)]


def loss_of_logits(z, t, weights5, ignore_label=None, class_weights=None):
    """z: torch [..., C] logits (any float type, may require grad); t: integer array of the leading shape -> (loss, the five terms,
    p of the counted rows, y of the counted rows, omega of the counted rows)."""
    C = z.shape[-1]
    t = np.asarray(t).reshape(-1).astype(np.int64)
    on = counted(t, ignore_label)
    idx = torch.from_numpy(np.nonzero(on)[0])
    cls = np.minimum(t[on], C - 1)
    w = np.ones(C) if class_weights is None else np.asarray(class_weights, np.float64)
    p = torch.softmax(z.reshape(-1, C), dim=-1)[idx]
    y = torch.from_numpy(np.eye(C)[cls].reshape(-1, C)).to(p.dtype)
    om = torch.from_numpy(w[cls]).to(p.dtype)
    tm = terms(y, p, om)
    loss = sum(wi * term for wi, term in zip(weights5, tm) if wi)
    if not torch.is_tensor(loss):          # a spec of zeros
        loss = p.sum() * 0.0
    return loss, tm, p, y, om


def reference(zq, t, weights5, ignore_label=None, class_weights=None):
    """zq: float [P, C] logits as the kernel reads them; t: uint8 [P] stored targets -> (the 14 scalars in the kernel's layout, dL/dz
    [P, C] by autograd - zero rows where ignored -, the float64 probabilities [P, C], the counted mask [P])."""
    z = torch.from_numpy(np.asarray(zq, np.float64)).requires_grad_(True)
    loss, tm, p, y, om = loss_of_logits(z, t, weights5, ignore_label, class_weights)
    loss.backward()
    pd, yd = p.detach().numpy(), y.numpy()
    n, C = pd.shape
    th = (pd > 0.5).astype(np.float64)
    sp, sy, spy = pd.sum(), yd.sum(), (pd * yd).sum()
    tv = [float(x.detach()) for x in tm]
    sc = np.array([float(loss.detach()), tv[0], tv[1], (2 * (th * yd).sum() + 1) / (sy + th.sum() + 1),
                   float((th == yd).sum()) / (max(n, 1) * C), sp, sy, spy, 1 - tv[2],
                   ((th * yd).sum() + 1) / (sy + th.sum() - (th * yd).sum() + 1), tv[3], tv[4] if weights5[4] else 0.0,
                   float(n), float(om.sum())])
    return sc, z.grad.numpy(), torch.softmax(z.detach(), dim=-1).numpy(), counted(t, ignore_label)
