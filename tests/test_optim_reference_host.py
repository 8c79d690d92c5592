"""CPU checks of tests/_optim_reference.py, the float64 reference tests/test_optim_ops_gpu.py holds csrc/optim.hip to.

* not too tight: a plain numpy fp32 evaluation in the kernel's operation order stays within the derived bounds on 2^20 generated
  elements, with and without gscale, clipvalue and a mask;
* not too loose: every listed wrong rule leaves the bounds on at least half of the unmasked elements;
* the fp32 Keras restatement oracle/optim.py agrees with the reference within the same bounds, three steps from a zero state;
* the loss-scale state machine against a table written out by hand.
"""
import numpy as np
import pytest

import _optim_reference as R
from oracle import optim as ooptim

f32 = np.float32
N = 1 << 20
B1, B2, RHO, MU, EPS, SD = 0.9, 0.999, 0.9, 0.9, 1e-7, 0.004
LR = 0.05              # large enough that a step is visible next to p (|p| in [1e-3, 1]) over most of the gradient range
GS = 0.37
CLIP = 1e-5            # 70 % of the generated |g| lie above it: the order of scale and clip matters for most elements
RULES = ["adam", "nadam", "rmsprop", "sgd", "sgd_nesterov", "sgd_novel"]


@pytest.fixture(scope="module")
def data():
    d = R.generate(N, 20240)
    rng = np.random.default_rng(7)
    d["mask"] = rng.choice(np.array([0, 0, 1, 0x80, 0xff], np.uint8), N)
    for a in d.values():
        a.setflags(write=False)
    return d


# -------------------------------------------------------------------------------------------------------------------------------
# the kernels' statements in numpy fp32, operation for operation, with the wrong variants behind `wrong`

def grad_seen32(g, gscale, clipvalue, clip_first):
    gv, c = g, f32(clipvalue)
    if clip_first and c > 0:
        gv = np.clip(gv, -c, c)
    if gscale is not None:
        gv = gv * f32(gscale)
    if not clip_first and c > 0:
        gv = np.clip(gv, -c, c)
    return gv


def fp32_step(rule, d, mask, gscale, clipvalue, sc, wrong=None):
    """One step of `rule` in fp32 -> tuple of outputs in the order of the reference."""
    one = f32(1.0)
    gv = grad_seen32(d["g"], gscale, clipvalue, wrong == "clip_first")
    p, eps = d["p"], f32(EPS)
    on = np.ones(len(p), bool) if mask is None else mask != 0
    with np.errstate(all="ignore"):
        if rule in ("adam", "nadam"):
            b1, b2 = (f32(B2), f32(B1)) if wrong == "betas_swapped" else (f32(B1), f32(B2))
            mn = b1 * d["m"] + (one - b1) * gv
            vn = b2 * d["v"] + (one - b2) * gv * gv
            if rule == "adam":
                den = np.sqrt(vn + eps) if wrong == "eps_inside" else np.sqrt(vn) + eps
                pn = p - (f32(LR) if wrong == "lr_for_lr_t" else sc["lr_t"]) * mn / den
            else:
                ig, im, iv, cg, cm = sc["fstate"]
                if wrong == "no_v_correction":
                    iv = one
                mbar = cg * (gv * ig) + cm * (mn * im)
                den = np.sqrt(vn * iv + eps) if wrong == "eps_inside" else np.sqrt(vn * iv) + eps
                pn = p - f32(LR) * mbar / den
            news, olds = (pn, mn, vn), (p, d["m"], d["v"])
        elif rule == "rmsprop":
            rho = f32(RHO)
            an = rho * d["v"] + (one - rho) * gv * gv
            den = np.sqrt(an + eps) if wrong == "eps_inside" else np.sqrt(an) + eps
            news, olds = (p - f32(LR) * gv / den, an), (p, d["v"])
        else:
            mu, l = f32(MU), f32(LR)
            vel = np.zeros_like(p) if rule == "sgd_novel" else d["vel"]
            vn = mu * vel - l * gv
            nesterov = (rule == "sgd_nesterov") != (wrong == "nesterov_swapped")
            pn = p + mu * vn - l * gv if nesterov else p + vn
            news, olds = (pn, vn), (p, vel)
    for a in news:
        assert a.dtype == np.float32
    outs = tuple(np.where(on, n_, o) for n_, o in zip(news, olds))
    return outs[:1] if rule == "sgd_novel" else outs


def reference(rule, d, mask, gscale, clipvalue, sc):
    if rule == "adam":
        return R.adam(d["p"], d["g"], d["m"], d["v"], mask, gscale, clipvalue, sc["lr_t"], B1, B2, EPS)
    if rule == "nadam":
        return R.nadam(d["p"], d["g"], d["m"], d["v"], mask, gscale, clipvalue, LR, sc["fstate"], B1, B2, EPS)
    if rule == "rmsprop":
        return R.rmsprop(d["p"], d["g"], d["v"], mask, gscale, clipvalue, LR, RHO, EPS)
    outs, bnds = R.sgd(d["p"], d["g"], None if rule == "sgd_novel" else d["vel"], mask, gscale, clipvalue, LR, MU, rule == "sgd_nesterov")
    return (outs[:1], bnds[:1]) if rule == "sgd_novel" else (outs, bnds)


def scalars(t):
    """The preparation kernels' scalars for the step that makes the counter t (Nadam's schedule followed from 1)."""
    ms = f32(1.0)
    for k in range(1, t + 1):
        fs = R.nadam_prep(ms, B1, B2, SD, k)
        ms = fs[0]
    return {"lr_t": R.adam_lr_t(LR, B1, B2, t), "fstate": fs[1:6]}


def violations(got, ref):
    """Per element: does ANY output leave its bound (the GPU test asserts every output of every element)."""
    outs, bnds = ref
    bad = np.zeros(len(outs[0]), bool)
    for a, r, b in zip(got, outs, bnds):
        bad |= ~(np.abs(a.astype(np.float64) - r) <= b)          # (a NaN violates)
    return bad


# -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["plain", "gscale", "clip", "mask", "gscale+clip+mask"])
@pytest.mark.parametrize("rule,t", [(r, t) for r in RULES for t in ((1, 7) if r in ("adam", "nadam") else (1,))])
def test_bound_is_not_too_tight(data, rule, t, variant):
    """0 violations of the derived bounds by a correct fp32 evaluation; the largest error / bound ratio is printed."""
    sc = scalars(t)
    gs = GS if "gscale" in variant else None
    cv = CLIP if "clip" in variant else 0.0
    mask = data["mask"] if "mask" in variant else None
    got = fp32_step(rule, data, mask, gs, cv, sc)
    ref = reference(rule, data, mask, gs, cv, sc)
    worst = []
    for a, r, b in zip(got, *ref):
        err = np.abs(a.astype(np.float64) - r)
        assert (err[b == 0] == 0).all()                                       # masked elements and exact zeros: bit-identical
        worst.append(float((err[b > 0] / b[b > 0]).max()))
    print("%s t=%d %s: max err / bound per output %s" % (rule, t, variant, ["%.3f" % w for w in worst]))
    assert int(violations(got, ref).sum()) == 0, worst
    if mask is not None:
        assert np.array_equal(got[0][mask == 0], data["p"][mask == 0])


def test_zero_gradient_and_zero_state_give_a_zero_step(data):
    """g = 0 on v = 0 (and m = 0): the step is 0 / (0 + eps) = 0 exactly, in the reference and in fp32: the output equals p."""
    z = (data["g"] == 0) & (data["v"] == 0) & (data["m"] == 0)
    assert z.sum() > N // 200
    sc = scalars(1)
    for rule in ("adam", "nadam", "rmsprop"):
        outs, _ = reference(rule, data, None, GS, 0.0, sc)
        assert np.array_equal(outs[0][z], data["p"][z].astype(np.float64)), rule
        assert np.array_equal(fp32_step(rule, data, None, GS, 0.0, sc)[0][z], data["p"][z]), rule


WRONG = [("adam", "eps_inside"), ("adam", "lr_for_lr_t"), ("adam", "betas_swapped"), ("adam", "clip_first"),
         ("nadam", "eps_inside"), ("nadam", "betas_swapped"), ("nadam", "clip_first"), ("nadam", "no_v_correction"),
         ("rmsprop", "eps_inside"), ("rmsprop", "clip_first"),
         ("sgd", "nesterov_swapped"), ("sgd_nesterov", "nesterov_swapped"), ("sgd", "clip_first"), ("sgd_nesterov", "clip_first"),
         ("sgd_novel", "clip_first")]


@pytest.mark.parametrize("rule,wrong", WRONG, ids=lambda x: x)
def test_bound_is_not_too_loose(data, rule, wrong):
    """Each wrong rule leaves the bounds on at least half of the unmasked elements (a condition on the bounds: were they k times
    wider, these fractions would fall).  The clip-order variant runs with gscale and clipvalue on - it is the identity otherwise -
    the others with gscale alone; t = 1, where lr_t and 1 / (1 - b2^t) are far from their limits lr and 1."""
    sc = scalars(1)
    cv = CLIP if wrong == "clip_first" else 0.0
    mask = data["mask"]
    ref = reference(rule, data, mask, GS, cv, sc)
    bad = violations(fp32_step(rule, data, mask, GS, cv, sc, wrong), ref)
    on = mask != 0
    assert not bad[~on].any()
    frac = bad[on].mean()
    print("%s / %s: outside the bound on %.1f %% of the unmasked elements" % (rule, wrong, 100 * frac))
    assert frac >= 0.5


# -------------------------------------------------------------------------------------------------------------------------------
# oracle/optim.py (fp32 Keras 2.2.4) against the reference

# the oracle rounds the DOUBLE 1 - beta to fp32 where Keras and the kernel subtract in fp32 (1 - fl(0.999) and fl(1 - 0.999) differ by
# 1.3e-5 relative); with betas that are fp32 numbers whose complement is one too, both are the same number and the comparison is
# about the update rule alone
OB1, OB2, ORHO = 1 - 2.0 ** -3, 1 - 2.0 ** -9, 1 - 2.0 ** -3


@pytest.mark.parametrize("rule", ["adam", "nadam", "rmsprop", "sgd", "sgd_nesterov"])
def test_keras_oracle_agrees_with_the_reference(rule):
    """Three steps from a zero state: after each, the oracle's fp32 parameters and moments lie within the reference's bounds of one
    float64 step from the oracle's previous state.  Nadam's oracle DIVIDES by its fp32 denominators where the kernel multiplies by
    the stored reciprocals: the reference is given the float64 reciprocals of those denominators, so it states the same numbers."""
    n = 1 << 14
    lr = 0.002 if rule == "nadam" else 0.01
    ctor = {"adam": lambda: ooptim.Adam(lr=lr, beta_1=OB1, beta_2=OB2), "nadam": lambda: ooptim.Nadam(lr=lr, beta_1=OB1, beta_2=OB2),
            "rmsprop": lambda: ooptim.RMSprop(lr=lr, rho=ORHO), "sgd": lambda: ooptim.SGD(lr=lr, momentum=MU),
            "sgd_nesterov": lambda: ooptim.SGD(lr=lr, momentum=MU, nesterov=True)}[rule]
    o = ctor()
    P = {"w": R.generate(n, 5)["p"]}
    zeros = np.zeros(n, np.float32)
    for t in (1, 2, 3):
        g = R.generate(n, 10 + t)["g"]
        p0 = P["w"].copy()
        if rule in ("adam", "nadam"):
            m0, v0 = o.m.get("w", zeros).copy(), o.v.get("w", zeros).copy()
            ms0 = getattr(o, "m_schedule", None)
        elif rule == "rmsprop":
            v0 = o.a.get("w", zeros).copy()
        else:
            v0 = o.vel.get("w", zeros).copy()
        o.step(P, {"w": g})
        if rule == "adam":
            lr_t = f32(lr * (np.sqrt(1.0 - OB2 ** t) / (1.0 - OB1 ** t)))
            ref, got = R.adam(p0, g, m0, v0, None, None, 0.0, lr_t, OB1, OB2, EPS), (P["w"], o.m["w"], o.v["w"])
        elif rule == "nadam":
            mu_t, mu_t1 = OB1 * (1.0 - 0.5 * 0.96 ** (t * SD)), OB1 * (1.0 - 0.5 * 0.96 ** ((t + 1) * SD))
            ms_new = ms0 * mu_t
            fst = [1.0 / np.float64(f32(1.0 - ms_new)), 1.0 / np.float64(f32(1.0 - ms_new * mu_t1)), 1.0 / np.float64(f32(1.0 - OB2 ** t)),
                   np.float64(f32(1.0 - mu_t)), np.float64(f32(mu_t1))]
            ref, got = R.nadam(p0, g, m0, v0, None, None, 0.0, lr, fst, OB1, OB2, EPS), (P["w"], o.m["w"], o.v["w"])
        elif rule == "rmsprop":
            ref, got = R.rmsprop(p0, g, v0, None, None, 0.0, lr, ORHO, EPS), (P["w"], o.a["w"])
        else:
            ref, got = R.sgd(p0, g, v0, None, None, 0.0, lr, MU, rule == "sgd_nesterov"), (P["w"], o.vel["w"])
        for a in got:
            assert a.dtype == np.float32
        assert int(violations(got, ref).sum()) == 0, (rule, t)


# -------------------------------------------------------------------------------------------------------------------------------
# the loss-scale record

@pytest.mark.parametrize("row", R.DLS_TABLE, ids=lambda r: r[0])
def test_dls_step_against_the_table(row):
    _, dls, gs, arena, clipnorm, dls_after, gs_after = row
    d, g, binds = R.dls_step(dls, gs, arena, clipnorm, R.DLS_TABLE_BASE)
    assert d == [float(x) for x in dls_after] and g == [float(x) for x in gs_after]
    assert binds == ("clip binds" in row[0])
    assert d[2:] == [float(x) for x in dls[2:]]                  # interval, floor, arena multiplier and cap are inputs only
    assert R.dls_step(dls, gs, float("inf"), clipnorm, R.DLS_TABLE_BASE)[1][0] == R.SKIP


def test_global_scale_reference():
    """sqrt(sum g^2) base against clipnorm, float(base) exactly where the clip does not bind, the skip marker, and the summation
    shape the bound counts: 8191 elements in one block are 32 terms per thread."""
    g = np.full(256, 1.0, np.float32)                              # norm 16
    assert R.global_scale(g, 0.0, 0.25) == (0.25, 0.0, False)
    assert R.global_scale(g, 8.0, 0.25) == (0.25, 0.0, False)       # 16 x 0.25 = 4 < 8 <= 16: the scaled norm decides
    val, rel, binds = R.global_scale(g, 2.0, 0.25)
    assert binds and val == 0.125 and rel == R.norm_rel_bound(256)
    g[17] = np.inf
    assert R.global_scale(g, 2.0, 0.25)[0] == R.SKIP
    assert R.norm_partition(8191) == (1, 8191) and R.norm_partition(3 * 4096 + 5) == (3, 4098)
    assert R.norm_partition(4096 * 1024 + 12345) == (1024, 4109)
    assert R.norm_rel_bound(8191) == 2 * R.U * ((32 + 10) / 2.0 + 1)
    with pytest.raises(ValueError):
        R.global_scale(np.full(256, 1.0, np.float32), 4.0, 0.25)    # on the threshold: decides nothing
