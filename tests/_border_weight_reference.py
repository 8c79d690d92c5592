"""The U-Net border weight map and the pixel-weighted one-class loss of include/stp_hip.h, restated in numpy and float64 (test
infrastructure, no GPU): the window search the header states, the separable algorithm the kernels run, the untruncated scipy form the
window truncates, and the weighted loss with its gradient."""
import numpy as np
from scipy import ndimage

BIG = 1 << 30
EIGHT = ndimage.generate_binary_structure(2, 2)


# ------------------------------------------------------------------------------------------------ masks
def blobs(h, w, seed, k=6, r=(2, 6)):
    """Six discs: each draws cy = randint(0, h), cx = randint(0, w), r = randint(2, 6), in that order."""
    rng = np.random.RandomState(seed)
    m = np.zeros((h, w), np.uint8)
    yy, xx = np.mgrid[:h, :w]
    for _ in range(k):
        cy, cx, rr = rng.randint(0, h), rng.randint(0, w), rng.randint(*r)
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= rr * rr] = 1
    return m


def salt(h, w, seed, p=0.15):
    return (np.random.RandomState(seed).rand(h, w) < p).astype(np.uint8)


def label(mask):
    """scipy.ndimage.label with the 8-neighbourhood (stp_mask_label, connectivity 2) -> int32 [h, w]."""
    return ndimage.label(np.asarray(mask) != 0, EIGHT)[0].astype(np.int32)


def _shifted(a, dy, dx, fill):
    """b[..., y, x] = a[..., y + dy, x + dx] inside the image, ``fill`` outside: the last two axes are the image, the axes in front of
    them (the samples of a batch) never mix."""
    h, w = a.shape[-2:]
    b = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        b[..., yd, xd] = a[..., ys, xs]
    return b


# ------------------------------------------------------------------------------------------------ distances
def distances_window(L, R):
    """The header's statement on label images [..., h, w] (values >= 0; every leading index is a sample of its own): over the
    (2R + 1)^2 offsets, the two smallest squared distances to pixels of DISTINCT labels -> (D1^2, D2^2) int64, -1 where there is none.
    State per pixel: (d1, l1) the nearest label, (d2, l2) the nearest label other than l1; an offset's candidate (d, l) updates it in
    one of four ways."""
    L = np.asarray(L).astype(np.int64)
    d1 = np.full(L.shape, BIG, np.int64)
    d2 = np.full(L.shape, BIG, np.int64)
    l1 = np.zeros(L.shape, np.int64)
    l2 = np.zeros(L.shape, np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            l = _shifted(L, dy, dx, 0)
            d = dy * dy + dx * dx
            on = l > 0
            same1 = on & (l == l1)
            first = on & ~same1 & (d < d1)
            rest = on & ~same1 & ~first
            same2 = rest & (l == l2)
            second = rest & ~same2 & (d < d2)
            d1 = np.where(same1, np.minimum(d1, d), d1)
            d2 = np.where(first, d1, d2)
            l2 = np.where(first, l1, l2)
            d1 = np.where(first, d, d1)
            l1 = np.where(first, l, l1)
            d2 = np.where(same2, np.minimum(d2, d), d2)
            l2 = np.where(second, l, l2)
            d2 = np.where(second, d, d2)
    return np.where(d1 == BIG, -1, d1), np.where(d2 == BIG, -1, d2)


def distances_separable(L, R):
    """The algorithm of csrc/border_weight.hip on label images [..., h, w]: the row pass keeps the nearest labelled pixel of the row
    within +-R as (dxA, labelA) and the nearest one with another label as dxB (|dx| ascending, left before right); the column pass
    scans dy twice."""
    L = np.asarray(L).astype(np.int64)
    dA = np.full(L.shape, BIG, np.int64)
    dB = np.full(L.shape, BIG, np.int64)
    lA = np.zeros(L.shape, np.int64)
    for dx in range(0, R + 1):
        for s in ((-dx, dx) if dx else (0,)):
            l = _shifted(L, 0, s, 0)
            on = l > 0
            first = on & (dA == BIG)
            other = on & ~first & (l != lA) & (dB == BIG)
            dA = np.where(first, dx, dA)
            lA = np.where(first, l, lA)
            dB = np.where(other, dx, dB)
    d1 = np.full(L.shape, BIG, np.int64)
    l1 = np.zeros(L.shape, np.int64)
    for dy in range(-R, R + 1):
        a, la = _shifted(dA, dy, 0, BIG), _shifted(lA, dy, 0, 0)
        v = np.where(a == BIG, BIG, dy * dy + a * a)
        better = v < d1
        d1 = np.where(better, v, d1)
        l1 = np.where(better, la, l1)
    d2 = np.full(L.shape, BIG, np.int64)
    for dy in range(-R, R + 1):
        a, b, la = _shifted(dA, dy, 0, BIG), _shifted(dB, dy, 0, BIG), _shifted(lA, dy, 0, 0)
        c = np.where((a != BIG) & (la != l1), a, b)
        d2 = np.minimum(d2, np.where(c == BIG, BIG, dy * dy + c * c))
    d2 = np.where(d1 == BIG, BIG, d2)
    return np.where(d1 == BIG, -1, d1), np.where(d2 == BIG, -1, d2)


# ------------------------------------------------------------------------------------------------ weights
def weight_from_distances(L, d1, d2, w0, sigma, b0=1.0, b1=1.0):
    """float64 map: (L ? b1 : b0) + w0 exp(-(sqrt(D1^2) + sqrt(D2^2))^2 / (2 sigma^2)) on the background where D2^2 >= 0."""
    L = np.asarray(L)
    s = np.sqrt(np.maximum(d1, 0).astype(np.float64)) + np.sqrt(np.maximum(d2, 0).astype(np.float64))
    term = np.where((L == 0) & (d2 >= 0), float(w0) * np.exp(-s * s / (2.0 * float(sigma) ** 2)), 0.0)
    return np.where(L != 0, float(b1), float(b0)) + term


def weight_map(L, w0=10.0, sigma=5.0, R=20, b0=1.0, b1=1.0, fn=distances_window):
    """[..., h, w] label images -> the float64 map of the header."""
    L = np.asarray(L)
    d1, d2 = fn(L, R)
    return weight_from_distances(L, d1, d2, w0, sigma, b0, b1)


def term_fraction(L, R, fn=distances_window):
    """The share of the background pixels with two objects in their window (a non-zero border term)."""
    L = np.asarray(L)
    _d1, d2 = fn(L, R)
    bg = L == 0
    return float(((d2 >= 0) & bg).sum()) / float(max(bg.sum(), 1))


def untruncated(L, w0=10.0, sigma=5.0, b0=1.0, b1=1.0):
    """The usual statement on ONE label image: scipy's distance_transform_edt per label, the two smallest distances, no window."""
    L = np.asarray(L)
    wc = np.where(L != 0, float(b1), float(b0)).astype(np.float64)
    values = [v for v in np.unique(L) if v > 0]
    if len(values) < 2:
        return wc
    d = np.stack([ndimage.distance_transform_edt(L != v) for v in values], -1)
    d.sort(-1)
    return wc + float(w0) * np.exp(-0.5 * ((d[..., 0] + d[..., 1]) / float(sigma)) ** 2) * (L == 0)


def truncation_bound(w0, sigma, R):
    return float(w0) * np.exp(-(R + 1) ** 2 / (2.0 * float(sigma) ** 2))


# ------------------------------------------------------------------------------------------------ weighted loss
EPS = float(np.float32(1e-7))
HI = float(np.float32(1.0) - np.float32(1e-7))
NAMES = ("loss", "bce", "dice_loss", "dice", "acc", "sum_p", "sum_y", "sum_py", "iou", "iot")


def weighted_loss(z, t, pw, w_bce, w_dice):
    """float64: logits z [count], target t [count] (non-zero = 1), pixel weights pw [count] -> (scalars float64 [16] in the layout of
    stp_sigmoid_bce_dice_weighted, dL/dz [count], probabilities).  [1] is the UNWEIGHTED binary_crossentropy, [13] the weighted one,
    [15] the mean weight; the slots the entry does not write are 0."""
    z = np.asarray(z, np.float64).reshape(-1)
    y = (np.asarray(t).reshape(-1) != 0).astype(np.float64)
    pw = np.asarray(pw, np.float64).reshape(-1)
    n = z.size
    p = 1.0 / (1.0 + np.exp(-z))
    inr = (p >= EPS) & (p <= HI)
    pc = np.clip(p, EPS, HI)
    zc = np.log(pc / (1.0 - pc))
    bce = np.maximum(zc, 0.0) - zc * y + np.log1p(np.exp(-np.abs(zc)))
    sp, sy, spy = p.sum(), y.sum(), (p * y).sum()
    th = (p > 0.5).astype(np.float64)
    st, sty = th.sum(), (th * y).sum()
    s = np.zeros(16)
    s[1] = bce.sum() / n
    s[2] = 1.0 - (2.0 * spy + 1.0) / (sy + sp + 1.0)
    s[3] = (2.0 * sty + 1.0) / (sy + st + 1.0)
    s[4] = (th == y).sum() / n
    s[5], s[6], s[7] = sp, sy, spy
    s[8] = (spy + 1.0) / (sy + sp - spy + 1.0)
    s[9] = (sty + 1.0) / (sy + st - sty + 1.0)
    s[13] = (pw * bce).sum() / n
    s[15] = pw.sum() / n
    s[0] = w_bce * s[13] + w_dice * s[2]
    den, num = sy + sp + 1.0, 2.0 * spy + 1.0
    g = np.where(inr, w_bce * pw * (p - y) / n, 0.0) + w_dice * (-(2.0 * y * den - num) / (den * den)) * (p * (1.0 - p))
    return s, g, p


# ------------------------------------------------------------------------------------------------ whole step
def weighted_oracle(*args, border=None, **kw):
    """oracle.step.OracleTrainer whose step weights the cross-entropy of the one-class head with the reference map of the batch's own
    masks (``border`` = {"w0", "sigma", "radius", "class_balance"}); dice_loss and every metric stay unweighted."""
    from collections import OrderedDict

    import torch
    from oracle import losses, nets as onets, optim as ooptim, step as ostep

    class WeightedOracle(ostep.OracleTrainer):
        def step(self, x_nhwc, y_nhwc, taps=None, apply=True):
            P = onets.to_torch(self.P, self.trainable)
            x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float32))
            y = torch.from_numpy(np.ascontiguousarray(y_nhwc, dtype=np.float32))
            logits, bn_updates = self._forward(P, x, True, taps)
            p = torch.sigmoid(logits)
            b0, b1 = border["class_balance"]
            L = np.stack([label(m[..., 0]) for m in np.asarray(y_nhwc)])
            omega = weight_map(L, border["w0"], border["sigma"], border["radius"], b0, b1)
            om = torch.from_numpy(omega[..., None].astype(np.float32))
            eps, one = torch.tensor(losses.KERAS_EPSILON), torch.tensor(np.float32(1.0))
            pc = torch.clamp(p, eps, one - eps)
            z = torch.log(pc / (one - pc))
            ce = torch.clamp(z, min=0) - z * y + torch.log1p(torch.exp(-torch.abs(z)))
            terms = {name: w for w, name in losses.parse_loss(self.loss_spec)}
            wbce = (om * ce).mean()
            loss = terms.get("binary_crossentropy", 0.0) * wbce + terms.get("dice_loss", 0.0) * losses.dice_loss(y, p)
            loss.backward()
            grads = OrderedDict((k, P[k].grad.numpy().copy()) for k in self.trainable)
            out = {"logits": logits.detach().numpy().copy(), "loss": float(loss.detach()), "bce": float(ce.detach().mean()),
                   "weighted_bce": float(wbce.detach()), "weight_mean": float(omega.mean()), "omega": omega,
                   "dice_loss": float(losses.dice_loss(y, p.detach())), "dice": float(losses.dice_metric(y, p.detach())),
                   "binary_accuracy": float(losses.binary_accuracy(y, p.detach())), "grads": grads}
            self.steps_done += 1
            if apply:
                self.opt.step(self.P, ooptim.clip_grads(grads, self.clipnorm, self.clipvalue))
                for k, v in bn_updates.items():
                    self.P[k] = v.numpy().astype(np.float32)
            return out

    return WeightedOracle(*args, **kw)
