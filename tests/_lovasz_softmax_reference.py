"""float64 evaluation of lovasz_softmax as include/stp_hip.h fixes it (stp_lovasz_softmax); helper of tests/test_lovasz_softmax_*.py, not
collected.  numpy only.

  p = softmax(z) over the classes; t_i the stored target, v_i = [t_i != ignore_label]; the class of a counted pixel is min(t_i, classes - 1),
  y its one-hot target.  Per class c over the counted pixels of the whole batch: e_ic = y_ic ? 1 - p_ic : p_ic, G_c = sum_i v_i y_ic, the
  errors ordered by descending e with ties by ascending pixel index (np.argsort(-e, kind="stable")), c1_r / c0_r the positives / negatives
  among ranks 0..r, g_r = 1 / (G + c0_r) for a positive and (G - c1_r) / ((G + c0_r - 1) (G + c0_r)) for a negative, loss_c = sum_r e_(r) g_r.
  lovasz_softmax = mean of loss_c over the P present classes (G_c > 0); P == 0: 0 and a zero gradient.
  Gradient with g held constant: d_ic = (y_ic ? -1 : +1) g_rank(i,c) / P, dz_ik = p_ik (d_ik - sum_c p_ic d_ic)."""
import numpy as np


def softmax(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def rank_weights(ys):
    """g_r of a class from its sorted {0,1} targets (float64; G = ys.sum() > 0)."""
    ys = np.asarray(ys, np.float64)
    G = ys.sum()
    c1 = np.cumsum(ys)
    c0 = np.arange(1, ys.size + 1, dtype=np.float64) - c1
    den = G + c0
    neg_den = np.where(ys > 0, 1.0, (den - 1.0) * den)          # (a negative has c0 >= 1: (den - 1) den >= G (G + 1) > 0)
    return np.where(ys > 0, 1.0 / den, (G - c1) / neg_den)


def reference(z, t, ignore_label=None):
    """z [pixels, classes] (any float type, taken as float64), t uint8 [pixels] -> dict(value, dz [pixels, classes] = d value / d z,
    present = P, positives = G_c [classes], p, on = counted mask [pixels], errors = e [pixels, classes], y)."""
    z = np.asarray(z, np.float64)
    t = np.asarray(t).astype(np.int64).reshape(-1)
    pixels, classes = z.shape
    on = np.ones(pixels, bool) if ignore_label is None else (t != int(ignore_label))
    cls = np.minimum(t, classes - 1)
    y = np.zeros((pixels, classes), np.float64)
    y[np.arange(pixels)[on], cls[on]] = 1.0
    p = softmax(z)
    e = np.where(y > 0, 1.0 - p, p)
    idx = np.nonzero(on)[0]
    G = y.sum(axis=0)
    present = int((G > 0).sum())
    d = np.zeros((pixels, classes), np.float64)
    total = 0.0
    for c in range(classes):
        if G[c] <= 0:
            continue
        ec = e[idx, c]
        order = np.argsort(-ec, kind="stable")
        ys = y[idx, c][order]
        g = rank_weights(ys)
        total += float((ec[order] * g).sum())
        d[idx[order], c] = np.where(ys > 0, -g, g) / present
    value = total / present if present else 0.0
    dz = p * (d - (p * d).sum(axis=1, keepdims=True))
    return dict(value=value, dz=dz, present=present, positives=G, p=p, on=on, errors=e, y=y)


def min_error_gap(ref):
    """The smallest difference between consecutive sorted errors inside a class, over the counted pixels of the present classes."""
    gap = np.inf
    on = ref["on"]
    for c in range(ref["p"].shape[1]):
        if ref["positives"][c] > 0 and on.sum() > 1:
            s = np.sort(ref["errors"][on, c])
            gap = min(gap, float(np.diff(s).min()))
    return gap
