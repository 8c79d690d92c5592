"""Numpy restatement of the dihedral (D4) test-time augmentation kernels (csrc/dihedral.hip) and of the group they implement (helper of
tests/test_dihedral_*.py and tests/_dihedral_time.py; numpy only, not collected, not imported by the package).

``op`` is an integer 0..7 on ``x`` [N, H, W, C]: transpose if ``op & 4``, then columns reversed if ``op & 1``, then rows reversed if
``op & 2``.  Whole pixels move; the channels keep their order.  0, 1, 2 are ``_predict_reference.flip``'s flips, 3 the half turn, 4 the
transpose, 5 and 6 the quarter turns, 7 the anti-transpose.  Nothing here computes: the values are moved, and ``accumulate`` is the one
float32 add per element the host loop performs, so device results are compared with ``np.array_equal``."""
import numpy as np

OPS = tuple(range(8))


def apply(x, op):
    """g_op: [N, H, W, C] -> [N, H', W', C], (H', W') = (W, H) if op & 4 else (H, W)."""
    t = x.transpose(0, 2, 1, 3) if op & 4 else x
    t = t[:, :, ::-1] if op & 1 else t
    t = t[:, ::-1] if op & 2 else t
    return t


def invert(y, op):
    """inv_op: the steps of ``apply`` undone in reverse order; ``invert(apply(x, op), op) == x``."""
    u = y[:, ::-1] if op & 2 else y
    u = u[:, :, ::-1] if op & 1 else u
    u = u.transpose(0, 2, 1, 3) if op & 4 else u
    return u


def accumulate(acc, probs, op):
    acc += invert(probs, op)          # (in place, as the host loop adds)
    return acc


def batch_sum(models, xs):
    """The ``"d4"`` host loop without its division: (float32 sums [n, H, W, classes], k); per model the eight members in ascending
    order, each map un-transformed before it is added."""
    acc, k = None, 0
    for m in models:
        for op in OPS:
            p = invert(m.predict(np.ascontiguousarray(apply(xs, op))), op)
            acc = np.zeros(p.shape, np.float32) if acc is None else acc
            acc += p; k += 1
    return acc, k
