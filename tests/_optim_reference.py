"""Float64 statements of the optimizer-step kernels (csrc/optim.hip) with a derived error bound for every output (helper of
tests/test_optim_reference_host.py and tests/test_optim_ops_gpu.py; not collected, calls no kernel).

Every update rule takes the fp32 arrays the kernel reads, evaluates one step in float64 and returns ``(outputs, bounds)``.  The
scalars the kernel receives as ``float`` (b1, b2, rho, mu, eps, lr, clipvalue, gscale) are rounded to fp32 once and widened; ``1 - b``
is the fp32 subtraction the kernel does.  The scalars the preparation kernels compute in double and store as float (Adam's lr_t,
Nadam's fstate[1..5]) are arguments: ``adam_lr_t`` / ``nadam_prep`` restate their formulas.

Bounds.  u = 2^-24 is the unit roundoff of fp32 (round to nearest; the build keeps the correctly rounded fp32 division and square
root, so each is one rounding like + and *).  An expression evaluated with k roundings on its way carries a relative error of at
most k u + O(u^2); where terms of either sign are added, the error is bounded on the SUM OF MAGNITUDES of the terms, never on the
(possibly cancelled) result.  Each bound below states its count k per term; the total gets a factor 2 for the O(u^2) terms and for
the first-order expansion of 1 / (den (1 + d)).  A fused multiply-add (-ffp-contract=on) drops one rounding, so the same bound holds.
No constant here is measured; tests/test_optim_reference_host.py shows that a plain fp32 evaluation stays inside the bounds and that
wrong rules do not.  The generator keeps every magnitude either zero or far from the subnormal range, so no count depends on gradual
underflow."""
import numpy as np

U = 2.0 ** -24
SKIP = -1.0            # gscale[0] of a skipped step


def _w(x):
    """A `float` argument of the C-ABI: rounded to fp32 once, then widened."""
    return np.float64(np.float32(x))


def _one_minus(b):
    """1.f - b as the kernel computes it (an fp32 subtraction; exact for b in [0.5, 1], one rounding below)."""
    return np.float64(np.float32(1.0) - np.float32(b))


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _on(mask, n):
    """The kernel updates an element when its mask BYTE is non-zero (any of 1..255); no mask: every element."""
    return np.ones(n, bool) if mask is None else (np.asarray(mask).reshape(-1) != 0)


def grad_seen(g, gscale, clipvalue):
    """g' = clip(g * gscale, +-clipvalue): the scale first (global-norm clip and 1 / (world x loss scale)), the value clip second -
    Keras' Optimizer.get_gradients.  One rounding in the kernel (the product; min / max are exact)."""
    gp = _f64(g)
    if gscale is not None:
        gp = gp * _w(gscale)
    c = _w(clipvalue)
    if c > 0:
        gp = np.clip(gp, -c, c)
    return gp


def _finish(on, news, olds, bounds):
    """Masked elements keep their bits: output = input, bound 0."""
    outs = tuple(None if o is None else np.where(on, n_, _f64(o)) for n_, o in zip(news, olds))
    bnds = tuple(None if o is None else np.where(on, b, 0.0) for b, o in zip(bounds, olds))
    return outs, bnds


def _moments(g, m, v, gscale, clipvalue, b1, b2):
    """m' = b1 m + (1 - b1) g'   and   v' = b2 v + (1 - b2) g' g'   (shared by Adam and Nadam).
      m': b1 m is 1 product + the add = 2 roundings; (1 - b1) g' is g' (1) + the product (1) + the add (1) = 3; terms of either
          sign: |err| <= 3 u A,  A = |b1 m| + |(1 - b1) g'|.
      v': all terms >= 0.  b2 v: 1 + 1 = 2; ((1 - b2) g') g': g' twice (2) + 2 products + the add = 5:  |err| <= 5 u v'."""
    gp = grad_seen(g, gscale, clipvalue)
    t1, t2 = _w(b1) * _f64(m), _one_minus(b1) * gp
    A = np.abs(t1) + np.abs(t2)
    vn = _w(b2) * _f64(v) + _one_minus(b2) * gp * gp
    return gp, t1 + t2, A, vn


def adam(p, g, m, v, mask, gscale, clipvalue, lr_t, b1, b2, eps):
    """p' = p - lr_t m' / (sqrt(v') + eps)  (Keras 2.2.4).  -> ((p', m', v'), (bound_p, bound_m, bound_v)).
      den = sqrt(v') + eps: v' carries 5 u, halved by the root (2.5), + the root's rounding (1) + the add (1; both terms >= 0) = 4.5.
      s = (lr_t m') / den: m' carries the ABSOLUTE error 3 u A (scaled by lr_t / den); the product 1, the quotient 1, den 4.5:
          |err| <= u (6.5 |s| + 3 lr_t A / den).
      p' = p - s: the subtraction rounds once on its result: u |p'|."""
    with np.errstate(all="ignore"):
        gp, mn, A, vn = _moments(g, m, v, gscale, clipvalue, b1, b2)
        lr_t = np.float64(lr_t)
        den = np.sqrt(vn) + _w(eps)
        s = lr_t * mn / den
        pn = _f64(p) - s
        bm = 2 * U * 3 * A
        bv = 2 * U * 5 * vn
        bp = 2 * U * (np.abs(pn) + 6.5 * np.abs(s) + 3 * lr_t * A / den)
    return _finish(_on(mask, len(pn)), (pn, mn, vn), (p, m, v), (bp, bm, bv))


def nadam(p, g, m, v, mask, gscale, clipvalue, lr, fstate, b1, b2, eps):
    """Keras 2.2.4 Nadam with the step's scalars fstate[1..5] = (ig, im, iv, cg, cm) = (1 / (1 - m_schedule_new),
    1 / (1 - m_schedule_next), 1 / (1 - b2^t), 1 - mu_t, mu_{t+1}) taken as given (widened, not rounded again):
    mbar = cg (g' ig) + cm (m' im);  p' = p - lr mbar / (sqrt(v' iv) + eps).  -> ((p', m', v'), bounds).
      T1 = cg (g' ig): g' (1) + 2 products + the add = 4.   T2 = cm (m' im): 2 products + the add = 3 relative, and the absolute
          error 3 u A of m' scaled by cm im.  Either sign:  |err mbar| <= u (4 |T1| + 3 |T2| + 3 cm im A).
      den = sqrt(v' iv) + eps: v' 5 + the product 1 = 6, halved 3, + the root 1 + the add 1 = 5.
      s = (lr mbar) / den: product 1 + quotient 1 + den 5 = 7 relative, plus lr |err mbar| / den.   p' = p - s: u |p'|."""
    ig, im, iv, cg, cm = [np.float64(x) for x in fstate]
    with np.errstate(all="ignore"):
        gp, mn, A, vn = _moments(g, m, v, gscale, clipvalue, b1, b2)
        lr = _w(lr)
        T1, T2 = cg * (gp * ig), cm * (mn * im)
        den = np.sqrt(vn * iv) + _w(eps)
        s = lr * (T1 + T2) / den
        pn = _f64(p) - s
        bm = 2 * U * 3 * A
        bv = 2 * U * 5 * vn
        bp = 2 * U * (np.abs(pn) + 7 * np.abs(s) + lr * (4 * np.abs(T1) + 3 * np.abs(T2) + 3 * cm * im * A) / den)
    return _finish(_on(mask, len(pn)), (pn, mn, vn), (p, m, v), (bp, bm, bv))


def rmsprop(p, g, acc, mask, gscale, clipvalue, lr, rho, eps):
    """a' = rho a + (1 - rho) g' g';  p' = p - lr g' / (sqrt(a') + eps).  -> ((p', a'), (bound_p, bound_a)).
      a': as v' of Adam, 5 u a'.   den = sqrt(a') + eps: 2.5 + 1 + 1 = 4.5.
      s = (lr g') / den: g' 1 + product 1 + quotient 1 + den 4.5 = 7.5 (one term, no cancellation).   p' = p - s: u |p'|."""
    with np.errstate(all="ignore"):
        gp = grad_seen(g, gscale, clipvalue)
        an = _w(rho) * _f64(acc) + _one_minus(rho) * gp * gp
        s = _w(lr) * gp / (np.sqrt(an) + _w(eps))
        pn = _f64(p) - s
        ba = 2 * U * 5 * an
        bp = 2 * U * (np.abs(pn) + 7.5 * np.abs(s))
    return _finish(_on(mask, len(pn)), (pn, an), (p, acc), (bp, ba))


def sgd(p, g, vel, mask, gscale, clipvalue, lr, mu, nesterov):
    """v' = mu v - lr g';  p' = p + v'  or, Nesterov,  p' = (p + mu v') - lr g'.  vel = None: v = 0 and no velocity output.
    -> ((p', v' | None), (bound_p, bound_v | None)).
      v': a1 = mu v is 1 product + the subtraction = 2; a2 = lr g' is g' 1 + product 1 + the subtraction 1 = 3; either sign:
          |err| <= 3 u S,  S = |a1| + |a2|.
      plain: p' = p + v': 3 u S + the add's u |p'|.
      Nesterov: q = mu v': mu 3 u S + u |q|;  (p + q): u (|p| + |q|);  a2: 2 u |a2| (g' and the product);  the subtraction: u |p'|:
          |err| <= u (|p'| + |p| + 2 |q| + 3 mu S + 2 |a2|)."""
    with np.errstate(all="ignore"):
        gp = grad_seen(g, gscale, clipvalue)
        mu_, p64 = _w(mu), _f64(p)
        a1 = mu_ * (_f64(vel) if vel is not None else np.zeros_like(gp))
        a2 = _w(lr) * gp
        S = np.abs(a1) + np.abs(a2)
        vn = a1 - a2
        if nesterov:
            q = mu_ * vn
            pn = (p64 + q) - a2
            bp = 2 * U * (np.abs(pn) + np.abs(p64) + 2 * np.abs(q) + 3 * mu_ * S + 2 * np.abs(a2))
        else:
            pn = p64 + vn
            bp = 2 * U * (np.abs(pn) + 3 * S)
        bv = 2 * U * 3 * S
    return _finish(_on(mask, len(pn)), (pn, vn), (p, vel), (bp, bv))


# -------------------------------------------------------------------------------------------------------------------------------
# the scalars of the preparation kernels (double arithmetic on the widened float arguments, stored as float)

def adam_lr_t(lr, b1, b2, t):
    """state[1] after the step that makes the counter t: lr sqrt(1 - b2^t) / (1 - b1^t)."""
    return np.float32(_w(lr) * np.sqrt(1.0 - _w(b2) ** float(t)) / (1.0 - _w(b1) ** float(t)))


def nadam_prep(m_schedule, b1, b2, schedule_decay, t):
    """fstate[0..5] after the step that makes the counter t, from fstate[0] = m_schedule before it (a float)."""
    b1, sd = _w(b1), _w(schedule_decay)
    mu_t = b1 * (1.0 - 0.5 * 0.96 ** (float(t) * sd))
    mu_t1 = b1 * (1.0 - 0.5 * 0.96 ** (float(t + 1) * sd))
    ms_new = _w(m_schedule) * mu_t
    ms_next = ms_new * mu_t1
    return np.array([ms_new, 1.0 / (1.0 - ms_new), 1.0 / (1.0 - ms_next), 1.0 / (1.0 - _w(b2) ** float(t)), 1.0 - mu_t, mu_t1],
                    dtype=np.float32)


# -------------------------------------------------------------------------------------------------------------------------------
# global gradient norm -> gscale, and the dynamic loss-scale record

def norm_partition(count):
    """(blocks, elements per block) of the sum-of-squares launch: count / 4096 blocks, at least 1, at most 1024."""
    blocks = min(max(count // 4096, 1), 1024)
    return blocks, -(-count // blocks)


def norm_rel_bound(count):
    """Relative bound on a gscale[0] that the clip determines.  The sum of squares (all terms >= 0) is fp32 up to the block partial:
    a thread squares (1 rounding) and accumulates at most ceil(per / 256) terms (one add each), six wave-reduction adds and three
    cross-wave adds follow: T = ceil(per / 256) + 10 roundings on the longest path, relative error T u.  The sum of the partials, the
    root, the scale and the quotient are double (2^-53: nothing).  The root halves the error, the store as float adds one rounding:
    (T / 2 + 1) u, times 2 as everywhere."""
    per = norm_partition(count)[1]
    T = -(-per // 256) + 10
    return 2 * U * (T / 2.0 + 1)


def sum_of_squares(g):
    """float64 sum of squares, or None when any element is inf / NaN (the arena overflowed: the step is skipped)."""
    g = np.asarray(g, dtype=np.float32)
    if not np.isfinite(g).all():
        return None
    g = g.astype(np.float64)
    return float(np.dot(g, g))


def _clip_factor(norm, clipnorm, rel):
    """min(1, clipnorm / norm); refuses a norm so close to the threshold that fp32 summation could decide either way."""
    c = float(np.float32(clipnorm))
    if not c > 0:
        return 1.0, False
    if abs(norm - c) <= 2 * rel * c:
        raise ValueError("clipnorm within the norm's error bound: the case decides nothing")
    return (c / norm, True) if norm > c else (1.0, False)


def global_scale(g, clipnorm, base):
    """stp_grad_global_scale: gscale[0] = min(1, clipnorm / (||g|| base)) base -> (value, relative bound, clip binds).  The clip
    compares the norm of the gradient the optimizer will see (||g|| base) with clipnorm.  Where the clip does not bind the value is
    float(base) exactly (bound 0); a non-finite element gives the skip marker."""
    ss = sum_of_squares(g)
    if ss is None:
        return SKIP, 0.0, False
    rel = norm_rel_bound(np.asarray(g).size)
    b = _w(base)
    k, binds = _clip_factor(np.sqrt(ss) * b, clipnorm, rel)
    return (k * b, rel, True) if binds else (float(np.float32(b)), 0.0, False)


def dls_step(dls, gscale, sumsq_or_nonfinite, clipnorm, base, rel=0.0):
    """stp_grad_global_scale_dls on the record documented above scale_by_device_kernel: dls[0] multiplier of the NEXT backward pass,
    [1] clean steps since the last change, [2] growth interval, [3] smallest multiplier, [4] multiplier the gradients in the arena
    were produced under, [5] largest multiplier.  ``sumsq_or_nonfinite``: the arena's sum of squares, or None for an arena with an
    inf / NaN.  -> (dls after, gscale after, clip binds).  Everything is a power of two or a small integer: compared with ==, except
    a gscale[0] the clip binds (within norm_rel_bound)."""
    d = [float(np.float32(x)) for x in dls]
    gs = [float(np.float32(x)) for x in gscale]
    m = d[0]
    eff = _w(base) / d[4]                      # 1 / dls[4], NOT 1 / dls[0]: the pass that filled the arena ran under dls[4]
    ss = sumsq_or_nonfinite
    if ss is None or not np.isfinite(ss):
        d[0], d[1] = max(m * 0.5, d[3]), 0.0
        return d, [SKIP, gs[1] + 1.0], False
    k, binds = _clip_factor(np.sqrt(ss) * eff, clipnorm, rel)
    gs[0] = k * eff if binds else float(np.float32(eff))
    clean = d[1] + 1.0
    if clean >= d[2]:
        d[0], d[1] = min(m * 2.0, d[5]), 0.0
    else:
        d[1] = clean
    return d, gs, binds


# dls = [next multiplier, clean steps, interval, floor, multiplier of the arena, cap]; gscale = [scale, skipped steps]
# written out by hand for base = 2^-3 and an arena of norm 16 (sum of squares 256); None = an arena with an inf / NaN
DLS_TABLE_BASE = 2.0 ** -3
DLS_TABLE = [
    # name, dls before, gscale before, arena, clipnorm -> dls after, gscale after
    ("clean step below the interval", [1024, 3, 5, 1, 1024, 65536], [9, 2], 256.0, 0.0, [1024, 4, 5, 1, 1024, 65536], [2.0 ** -13, 2]),
    ("clean step reaching the interval", [1024, 4, 5, 1, 1024, 65536], [9, 2], 256.0, 0.0, [2048, 0, 5, 1, 1024, 65536], [2.0 ** -13, 2]),
    ("clean step at the cap", [65536, 4, 5, 1, 65536, 65536], [9, 2], 256.0, 0.0, [65536, 0, 5, 1, 65536, 65536], [2.0 ** -19, 2]),
    ("overflow", [1024, 3, 5, 1, 1024, 65536], [9, 2], None, 0.0, [512, 0, 5, 1, 1024, 65536], [-1, 3]),
    ("overflow at the floor", [8, 3, 5, 8, 8, 65536], [9, 2], None, 0.0, [8, 0, 5, 8, 8, 65536], [-1, 3]),
    # the arena ran under 512, the next pass runs under 1024: the scale folds in 1 / 512 and the doubling starts from 1024
    ("dls[4] != dls[0]", [1024, 4, 5, 1, 512, 65536], [9, 2], 256.0, 0.0, [2048, 0, 5, 1, 512, 65536], [2.0 ** -12, 2]),
    # norm seen by the optimizer = 16 x 2^-3 / 1024 = 2^-9 > clipnorm 2^-11: k = 1 / 4
    ("clean step, clip binds", [1024, 0, 5, 1, 1024, 65536], [9, 2], 256.0, 2.0 ** -11, [1024, 1, 5, 1, 1024, 65536], [2.0 ** -15, 2]),
    # ... and a clipnorm between the scaled norm 2^-9 and the unscaled norm 16 does not bind
    ("clean step, clip above the scaled norm", [1024, 0, 5, 1, 1024, 65536], [9, 2], 256.0, 1.0, [1024, 1, 5, 1, 1024, 65536], [2.0 ** -13, 2]),
]


# -------------------------------------------------------------------------------------------------------------------------------
# inputs

def generate(n, seed):
    """One optimizer state of n elements -> dict of fp32 arrays p, g, m, v (>= 0; also RMSprop's accumulator), vel.
      g: magnitudes log-uniform over [1e-8, 1e2], either sign: eps = 1e-7 dominates sqrt(v) for some elements, is nothing for others.
      m, vel: either sign independent of g's (half oppose it: b1 m + (1 - b1) g and mu v - lr g cancel), magnitudes tied to |g| over
         3.5 / 2 decades so that some pairs cancel almost fully;  v: (|g| 10^[-1, 1])^2.
      about 5 % of the gradients and about 5 % of the moments (m, v and vel together) are exactly 0, a quarter of those together.
      p: magnitudes log-uniform over [1e-3, 1] (Keras initialisers), either sign.
    Every non-zero magnitude is at least 1e-11 and every non-zero square at least 1e-20: normal fp32 numbers."""
    rng = np.random.default_rng(seed)
    sign = lambda: rng.integers(0, 2, n) * 2.0 - 1.0
    mag = 10.0 ** rng.uniform(-8, 2, n)
    zero_g = rng.random(n) < 0.05
    g = np.where(zero_g, 0.0, sign() * mag)
    m = sign() * mag * 10.0 ** rng.uniform(-3, 0.5, n)
    v = (mag * 10.0 ** rng.uniform(-1, 1, n)) ** 2
    vel = sign() * 0.05 * mag * 10.0 ** rng.uniform(-1, 1, n)
    zero_s = (rng.random(n) < 0.04) | (zero_g & (rng.random(n) < 0.25))
    if n >= 8:          # the three combinations exist at every size
        zero_g[5], zero_s[5] = True, True
        zero_g[6], zero_s[6] = True, False
        zero_g[7], zero_s[7] = False, True
        g = np.where(zero_g, 0.0, np.where(g == 0, mag, g))
    m, v, vel = [np.where(zero_s, 0.0, a) for a in (m, v, vel)]
    p = sign() * 10.0 ** rng.uniform(-3, 0, n)
    out = {k: a.astype(np.float32) for k, a in dict(p=p, g=g, m=m, v=v, vel=vel).items()}
    for k, a in out.items():
        nz = np.abs(a[a != 0]).astype(np.float64)
        floor = 1e-19 if k == "v" else 1e-12                  # v is a square already; 1e-12^2 x 1e-3 is still 1e11 x the smallest normal
        assert nz.size == 0 or (nz.min() >= floor and nz.max() < 1e7), k
    assert (out["v"] >= 0).all()
    return out
