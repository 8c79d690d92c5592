"""GPU op tests of csrc/optim.hip: the four Keras update rules, the global gradient norm with its overflow guard, the dynamic
loss-scale record and stp_scale_by_device.  Each C-ABI entry point is called directly and compared with the float64 statements of
tests/_optim_reference.py, element by element within the bound DERIVED there (operation counts x 2^-24 on sums of magnitudes;
tests/test_optim_reference_host.py shows that a correct fp32 evaluation stays inside and wrong rules do not).  No tolerance here is a
literal: where a result is a power of two, a small integer or an untouched input it is compared with ==.

Conventions as in test_ops_rest_gpu.py: device temporaries stay alive until the test ends, pure outputs are pre-filled with NaN,
refusals are checked on the return code and nothing is read afterwards.  Every read-modify-write buffer carries 64 canary elements
behind its end that must come back bit-identical, and the gradient must come back bit-identical too.  Sizes: one vector (4), two
workgroups with a ragged second (1028) and one above the launchers' grid cap (CAP + 1028: the grid-stride loop takes a second trip for
the first 257 vectors only, so a wrong stride shows as untouched or twice-updated elements).  ``build`` / ``dtype`` route a case to
libstp_hip.so or libstp_hip_f16.so: the optimizer kernels are fp32 in both and must compute the same in both.
"""
import numpy as np
import pytest
import torch

import _optim_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
TD = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
BADARG, WORKSPACE = -1, -3
CAP = 4096 * 256 * 4                  # elements one trip of the capped optimizer grid covers; also where the norm's block count caps
BIG = CAP + 1028
GUARD = 64
CANARY = -24576.0                     # -1.5 x 2^14: exact in every storage dtype; no case here produces it
B1, B2, RHO, MU, EPS, SD, LR = 0.9, 0.999, 0.9, 0.9, 1e-7, 0.004, 0.05
GS = 0.37
CLIP = 1e-3                           # half of the generated |g| lie below it, half above
RULES = ["adam", "nadam", "rmsprop", "sgd", "sgd_nesterov", "sgd_novel"]
f32 = np.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from segmentation_training_pipeline_amd import ops as o
    return o


@pytest.fixture(autouse=True)
def _storage_build(request):
    """Cases parametrized with build = "fp16" or dtype = "fp16" call into libstp_hip_f16.so."""
    from segmentation_training_pipeline_amd import _lib
    prm = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    with _lib.storage("fp16" if "fp16" in (prm.get("build"), prm.get("dtype")) else "bf16"):
        yield


_KEEP = []


def keep(t):
    _KEEP.append(t)
    return t


@pytest.fixture(autouse=True)
def _release_device_temporaries():
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dev(a):
    return keep(torch.from_numpy(np.array(a)).to(DEV))          # (a copy: the shared inputs are read-only)


def guarded(a):
    """Device copy of a numpy array with GUARD canary elements behind it (the kernel gets the pointer to element 0)."""
    a = np.ascontiguousarray(a)
    return dev(np.concatenate([a, np.full(GUARD, CANARY, a.dtype)]))


def back(t, n):
    """Host copy of a guarded buffer's first n elements, after checking the canary behind them bit for bit."""
    torch.cuda.synchronize()
    h = t.cpu().numpy()
    assert h.size == n + GUARD and np.array_equal(h[n:], np.full(GUARD, CANARY, h.dtype)), "canary overwritten"
    return h[:n]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint16)


def rc(name, *args):
    """Return code of a C-ABI call (refusals: nothing may be launched, so nothing is synchronised or read afterwards)."""
    from segmentation_training_pipeline_amd import _lib
    return int(getattr(_lib.load(), name)(*args))


def same_or_adjacent(got, want):
    """A double formula rounded to float: the device pow and the host pow may differ in the last bit of the double, which moves
    the float by at most one step."""
    got, want = f32(got), f32(want)
    return got == want or got == np.nextafter(want, f32(np.inf)) or got == np.nextafter(want, f32(-np.inf))


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs of the update rules

def mask_bytes(n):
    """Vector j carries the on / off pattern (j + 5) % 16 of its four elements - all 16 from 16 vectors on, 0b0101 for a single vector -
    and the non-zero bytes cycle through 1, 0x80 and 0xff."""
    i = np.arange(n)
    on = (((i // 4 + 5) % 16) >> (i % 4)) & 1
    return np.where(on == 1, np.array([1, 0x80, 0xff], np.uint8)[i % 3], 0).astype(np.uint8)


def plant_clip_edges(g, gscale, clip):
    """g[0]: |g gs| below the clip value, g[1]: above, g[2]: EXACTLY equal in fp32 (found among the neighbours of clip / gs)."""
    gs, c = f32(1.0 if gscale is None else gscale), f32(clip)
    g[0], g[1] = c / gs / f32(8), -f32(16) * c / gs
    up = dn = c / gs
    cands = [up]
    for _ in range(4):
        up, dn = np.nextafter(up, f32(np.inf)), np.nextafter(dn, f32(-np.inf))
        cands += [up, dn]
    hit = [x for x in cands if f32(x * gs) == c]
    assert hit, "no fp32 g with g * gs == clipvalue near clipvalue / gs"
    g[2] = hit[0]
    a = np.abs(g * gs)
    assert (a[g != 0] < c).any() and (a > c).any() and (a == c).any()


def make_case(n, seed, gscale, clip, use_mask, poison=False):
    """Generated state of n elements (+ mask, clip edges, non-finite gradients on masked elements); read-only."""
    d = R.generate(n, seed)
    if clip > 0:
        plant_clip_edges(d["g"], gscale, clip)
    d["mask"] = mask_bytes(n) if use_mask else None
    if use_mask and n >= 64:
        pat = (d["mask"].reshape(-1, 4) != 0) @ np.array([1, 2, 4, 8])
        assert len(set(pat.tolist())) == 16 and set(d["mask"].tolist()) == {0, 1, 0x80, 0xff}
    if poison:
        off = np.nonzero(d["mask"] == 0)[0]
        d["g"][off] = np.array([np.inf, np.nan, -np.inf], np.float32)[np.arange(off.size) % 3]
        assert ((d["mask"].reshape(-1, 4) != 0).any(1) & (d["mask"].reshape(-1, 4) == 0).any(1)).any()   # mixed vectors exist
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


def nadam_schedule(t0):
    """fstate[0] (m_schedule, a float) after t0 steps from 1."""
    ms = f32(1.0)
    for k in range(1, t0 + 1):
        ms = R.nadam_prep(ms, B1, B2, SD, k)[0]
    return ms


def run_rule(ops, rule, d, n, gscale, clip, t0=0):
    """One launch of `rule` on device copies of d; checks the step counters and prepared scalars, the canaries, the gradient's and the
    masked elements' bits and every output element against the float64 reference within its bound."""
    mask = d["mask"]
    p, g = guarded(d["p"]), dev(d["g"])
    md = None if mask is None else dev(mask)
    gsd = None if gscale is None else dev(np.array([gscale, 5.0], np.float32))
    lr = dev(np.array([LR], np.float32))
    if rule in ("adam", "nadam"):
        m, v = guarded(d["m"]), guarded(d["v"])
        state = keep(torch.tensor([t0, 0x7fc00000], dtype=torch.int32, device=DEV))          # state[1]: NaN bits until the step writes lr_t
        if rule == "adam":
            ops.adam(p, g, m, v, n, lr, B1, B2, EPS, state, mask=md, gscale=gsd, clipvalue=clip)
            torch.cuda.synchronize()
            st = state.cpu().numpy()
            lr_t = st[1:].view(np.float32)[0]
            assert st[0] == t0 + 1 and same_or_adjacent(lr_t, R.adam_lr_t(LR, B1, B2, t0 + 1)), (st, lr_t)
            ref = R.adam(d["p"], d["g"], d["m"], d["v"], mask, gscale, clip, lr_t, B1, B2, EPS)
        else:
            ms0 = nadam_schedule(t0)
            fstate = dev(np.array([ms0, np.nan, np.nan, np.nan, np.nan, np.nan, CANARY, CANARY], np.float32))
            ops.nadam(p, g, m, v, n, lr, B1, B2, EPS, SD, state, fstate, mask=md, gscale=gsd, clipvalue=clip)
            torch.cuda.synchronize()
            fs, want = fstate.cpu().numpy(), R.nadam_prep(ms0, B1, B2, SD, t0 + 1)
            assert int(state[0].item()) == t0 + 1 and int(state[1].item()) == 0x7fc00000
            assert all(same_or_adjacent(a, b) for a, b in zip(fs[:6], want)) and (fs[6:] == f32(CANARY)).all(), (fs, want)
            ref = R.nadam(d["p"], d["g"], d["m"], d["v"], mask, gscale, clip, LR, fs[1:6], B1, B2, EPS)
        got, olds, names = (back(p, n), back(m, n), back(v, n)), (d["p"], d["m"], d["v"]), "pmv"
    elif rule == "rmsprop":
        acc = guarded(d["v"])
        ops.rmsprop(p, g, acc, n, lr, RHO, EPS, mask=md, gscale=gsd, clipvalue=clip)
        ref = R.rmsprop(d["p"], d["g"], d["v"], mask, gscale, clip, LR, RHO, EPS)
        got, olds, names = (back(p, n), back(acc, n)), (d["p"], d["v"]), "pa"
    else:
        vel = None if rule == "sgd_novel" else guarded(d["vel"])
        ops.sgd(p, g, vel, n, lr, MU, rule == "sgd_nesterov", mask=md, gscale=gsd, clipvalue=clip)
        outs, bnds = R.sgd(d["p"], d["g"], None if vel is None else d["vel"], mask, gscale, clip, LR, MU, rule == "sgd_nesterov")
        if vel is None:
            ref, got, olds, names = (outs[:1], bnds[:1]), (back(p, n),), (d["p"],), "p"
        else:
            ref, got, olds, names = (outs, bnds), (back(p, n), back(vel, n)), (d["p"], d["vel"]), "pv"
    assert np.array_equal(bits(g.cpu().numpy()), bits(d["g"])), "the gradient was written"
    if gsd is not None:
        assert gsd.cpu().numpy().tolist() == [f32(gscale), 5.0]
    off = np.zeros(n, bool) if mask is None else mask == 0
    for name, a, r, b, old in zip(names, got, ref[0], ref[1], olds):
        assert not np.isnan(a).any(), name
        err = np.abs(a.astype(np.float64) - r)
        bad = ~(err <= b)
        assert not bad.any(), "%s: %d of %d outside the bound, first at %d, worst err / bound %.3g" % (
            name, bad.sum(), n, np.nonzero(bad)[0][0], (err[bad] / np.maximum(b[bad], 1e-300)).max())
        assert np.array_equal(bits(a[off]), bits(old[off])), name + ": a masked element changed"
    if mask is None and not gscale and not clip:
        z = (d["g"] == 0) & (d["v"] == 0) & (d["m"] == 0) & (d["vel"] == 0)
        assert np.array_equal(got[0][z], d["p"][z])              # zero gradient on a zero state: the step is exactly 0


@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("use_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("clip", [0.0, CLIP], ids=["noclip", "clip"])
@pytest.mark.parametrize("gscale", [None, GS], ids=["nogs", "gs"])
@pytest.mark.parametrize("n", [4, 1028])
@pytest.mark.parametrize("rule", RULES)
def test_update_rule_one_step_within_the_derived_bound(ops, rule, n, gscale, clip, use_mask, build):
    """One step of every rule from a generated non-zero state (gradient magnitudes over ten decades, moments of either sign, exact
    zeros), gscale absent / 0.37, clipvalue 0 / 1e-3 with |g gs| below, above and exactly on it, mask absent / present."""
    run_rule(ops, rule, make_case(n, 31 + n, gscale, clip, use_mask), n, gscale, clip)


@pytest.mark.parametrize("rule", RULES)
def test_masked_elements_ignore_non_finite_gradients(ops, rule):
    """Masked elements carry inf / NaN / -inf gradients (no gscale, so no guard skips the step): their p, m, v keep their bits, and
    their unmasked neighbours in the same 4-element vector still meet the bound."""
    run_rule(ops, rule, make_case(1028, 77, None, 0.0, True, poison=True), 1028, None, 0.0)


@pytest.mark.parametrize("rule,t0", [("adam", 0), ("adam", 6), ("adam", 9999), ("nadam", 0), ("nadam", 6)])
def test_step_counters_and_prepared_scalars(ops, rule, t0):
    """state[0] advances by exactly one from t0; Adam's lr_t and Nadam's fstate[0..5] are the double formulas rounded to float (or the
    adjacent float); the update uses them (gscale, clipvalue and mask on)."""
    run_rule(ops, rule, make_case(1028, 5 + t0, GS, CLIP, True), 1028, GS, CLIP, t0=t0)


@pytest.fixture(scope="module")
def big_case():
    return make_case(BIG, 99, GS, CLIP, True)


@pytest.mark.parametrize("rule", ["adam", "nadam", "rmsprop", "sgd_nesterov"])
def test_update_rule_above_the_grid_cap(ops, rule, big_case):
    """CAP + 1028 elements, gscale, clipvalue and mask on: production arenas (24 M floats) run entirely on this side of the cap."""
    run_rule(ops, rule, big_case, BIG, GS, CLIP, t0=6)


def test_update_rule_refusals(ops):
    """count 0, negative or not a multiple of 4, and every required pointer NULL in turn: STP_E_BADARG from all four rules.  mask,
    gscale and SGD's velocity are optional."""
    t = keep(torch.zeros(64, dtype=torch.float32, device=DEV))
    s = keep(torch.zeros(2, dtype=torch.int32, device=DEV))
    p, ps, st = ops.ptr(t), ops.ptr(s), ops.stream()
    calls = {
        "stp_adam": (lambda a, n: rc("stp_adam", a[0], a[1], a[2], a[3], n, a[4], B1, B2, EPS, a[5], None, None, 0.0, st), [p, p, p, p, p, ps]),
        "stp_nadam": (lambda a, n: rc("stp_nadam", a[0], a[1], a[2], a[3], n, a[4], B1, B2, EPS, SD, a[5], a[6], None, None, 0.0, st),
                      [p, p, p, p, p, ps, p]),
        "stp_rmsprop": (lambda a, n: rc("stp_rmsprop", a[0], a[1], a[2], n, a[3], RHO, EPS, None, None, 0.0, st), [p, p, p, p]),
        "stp_sgd": (lambda a, n: rc("stp_sgd", a[0], a[1], None, n, a[2], MU, 0, None, None, 0.0, st), [p, p, p]),
    }
    for name, (call, args) in calls.items():
        for n in (0, -4, 6, 3, 1023):
            assert call(args, n) == BADARG, (name, n)
        for k in range(len(args)):
            assert call(args[:k] + [None] + args[k + 1:], 8) == BADARG, (name, k)
    torch.cuda.synchronize()
    assert torch.count_nonzero(t).item() == 0 and torch.count_nonzero(s).item() == 0            # nothing ran


# ---------------------------------------------------------------------------------------------------------------------------------
# stp_grad_global_scale

NORM_COUNTS = [1, 4095, 8191, 3 * 4096 + 5, CAP + 12345]       # one block (three times), ragged last block, capped block count
BASES = [1.0, 0.25, 1.0 / 16384]


def arena(count, seed=3):
    """randn scaled by 1 + (i // 1000) % 7: a dropped or double-counted range moves the norm by far more than the bound."""
    g = np.random.default_rng(seed).standard_normal(count, dtype=np.float32)
    g *= (1 + (np.arange(count) // 1000) % 7).astype(np.float32)
    assert float(np.abs(g).max()) * np.sqrt(count) < 1e18
    return g


def workspace():
    """Exactly the 1024 floats the entry points ask for, NaN, with a canary behind them."""
    return guarded(np.full(1024, np.nan, np.float32))


def check_workspace(ws):
    back(ws, 1024)


def call_norm(ops, gd, count, clipnorm, base, gs, ws, dls=None):
    from segmentation_training_pipeline_amd import _lib
    if dls is None:
        _lib.call("stp_grad_global_scale", ops.ptr(gd), count, float(clipnorm), float(base), ops.ptr(gs), ops.ptr(ws), 4096, ops.stream())
    else:
        _lib.call("stp_grad_global_scale_dls", ops.ptr(gd), count, float(clipnorm), float(base), ops.ptr(gs), ops.ptr(dls), ops.ptr(ws),
                  4096, ops.stream())
    torch.cuda.synchronize()
    return gs.cpu().numpy()


def within(got, want, rel):
    return abs(float(got) - want) <= rel * abs(want)


@pytest.mark.parametrize("build", ["bf16", "fp16"])
@pytest.mark.parametrize("count", NORM_COUNTS)
def test_global_scale_against_the_float64_norm(ops, count, build):
    """gscale[0] = min(1, clipnorm / (||g|| base)) base for clipnorm off / above the norm / below the scaled norm / BETWEEN the scaled
    norm ||g|| base and the norm ||g|| (does not bind: the optimizer sees the scaled gradient) and base 1, 1 / 4, 1 / 16384: float(base)
    exactly where the clip does not bind, within the summation bound of the reference where it does; gscale[1] untouched."""
    g = arena(count)
    gd, ws = dev(g), workspace()
    norm = np.sqrt(R.sum_of_squares(g))
    cases = [(0.0, b, False) for b in BASES] + [(2 * norm, 1.0, False)] + [(norm * b / 4, b, True) for b in BASES] + \
            [(norm * np.sqrt(b), b, False) for b in BASES[1:]]
    for clipnorm, base, binds in cases:
        want, rel, rbinds = R.global_scale(g, clipnorm, base)
        assert rbinds == binds
        gs = dev(np.array([np.nan, 5.0], np.float32))
        got = call_norm(ops, gd, count, clipnorm, base, gs, ws)
        assert got[1] == 5.0
        if binds:
            assert within(got[0], want, rel), (clipnorm, base, got[0], want, abs(got[0] - want) / want / rel)
            assert within(got[0], float(f32(clipnorm)) / norm, rel)                       # = clipnorm / ||g||: base cancels
        else:
            assert got[0] == f32(base), (clipnorm, base, got[0])
    check_workspace(ws)
    assert np.array_equal(bits(gd.cpu().numpy()), bits(g))


def test_global_scale_of_an_all_zero_arena(ops):
    count = 3 * 4096 + 5
    gs = dev(np.array([np.nan, 5.0], np.float32))
    ws = workspace()
    got = call_norm(ops, keep(torch.zeros(count, device=DEV)), count, 0.5, 0.25, gs, ws)
    assert got.tolist() == [0.25, 5.0]


@pytest.mark.parametrize("count", [3 * 4096 + 5, CAP + 12345])
def test_global_scale_overflow_guard_at_every_edge(ops, count):
    """+inf, -inf and NaN at the first element, the last, and either side of the first block boundary: each gives [-1, 6] from
    [0.5, 5]; the clean arena then restores the scale and keeps the count."""
    g = arena(count)
    gd, ws = dev(g), workspace()
    per = R.norm_partition(count)[1]
    assert per < count
    for idx in (0, count - 1, per - 1, per):
        for bad in (np.inf, -np.inf, np.nan):
            gs = dev(np.array([0.5, 5.0], np.float32))
            gd[idx] = float(bad)
            assert call_norm(ops, gd, count, 0.0, 0.25, gs, ws).tolist() == [-1.0, 6.0], (idx, bad)
            gd[idx] = float(g[idx])
            assert call_norm(ops, gd, count, 0.0, 0.25, gs, ws).tolist() == [0.25, 6.0], (idx, bad)
    check_workspace(ws)
    assert np.array_equal(bits(gd.cpu().numpy()), bits(g))


# ---------------------------------------------------------------------------------------------------------------------------------
# stp_grad_global_scale_dls

def run_dls(ops, g, gd, count, dls, gs, overflow, clipnorm, ws):
    """One call on the record `dls` / `gs`; -> (dls after, gscale after, reference dls, reference gscale, clip binds, bound)."""
    dd = dev(np.array(list(dls) + [CANARY, CANARY], np.float32))
    gsd = dev(np.array(gs, np.float32))
    rel = R.norm_rel_bound(count)
    rd, rg, binds = R.dls_step(dls, gs, None if overflow else R.sum_of_squares(g), clipnorm, R.DLS_TABLE_BASE, rel)
    got_g = call_norm(ops, gd, count, clipnorm, R.DLS_TABLE_BASE, gsd, ws, dls=dd)
    got_d = dd.cpu().numpy()
    assert (got_d[6:] == f32(CANARY)).all()
    assert got_d[:6].tolist() == rd, (got_d, rd)
    assert got_d[2:6].tolist() == [float(x) for x in dls[2:6]]                 # interval, floor, arena multiplier, cap: inputs only
    assert got_g[1] == rg[1]
    if binds:
        assert within(got_g[0], rg[0], rel), (got_g[0], rg[0])
    else:
        assert got_g[0] == f32(rg[0]), (got_g[0], rg[0])
    return got_d[:6].tolist(), got_g.tolist(), binds


@pytest.mark.parametrize("row", R.DLS_TABLE, ids=lambda r: r[0])
def test_dls_record_for_every_row_of_the_table(ops, row):
    """The rows of the host table (clean below / reaching the interval, at the cap, overflow, overflow at the floor, dls[4] != dls[0],
    clip binding / not binding on the SCALED norm) on the 3 x 4096 + 5 arena: dls[0..5] and gscale equal dls_step's exactly - and,
    where the clip does not bind, the table's own numbers - except a gscale[0] the clip binds (norm bound)."""
    name, dls, gs, table_arena, clipnorm, dls_after, gs_after = row
    count = 3 * 4096 + 5
    g = arena(count)
    if table_arena is None:
        g[count // 2] = np.nan
    ws = workspace()
    got_d, got_g, binds = run_dls(ops, g, dev(g), count, dls, gs, table_arena is None, clipnorm, ws)
    assert binds == ("clip binds" in name)
    assert got_d == [float(x) for x in dls_after]
    if not binds:
        assert got_g == [float(x) for x in gs_after]
    check_workspace(ws)


@pytest.mark.parametrize("overflow", [False, True], ids=["clean", "nan"])
def test_dls_record_above_the_block_cap(ops, overflow):
    count = CAP + 12345
    g = arena(count)
    if overflow:
        g[count - 7] = np.nan
    ws = workspace()
    row = R.DLS_TABLE[3 if overflow else 6]
    _, _, binds = run_dls(ops, g, dev(g), count, row[1], row[2], overflow, row[4], ws)
    assert binds == (not overflow)
    check_workspace(ws)


def test_norm_entry_point_refusals(ops):
    """A workspace below 4096 bytes: STP_E_WORKSPACE; NULL gscale, NULL dls, NULL gradient or count <= 0: STP_E_BADARG."""
    t = keep(torch.zeros(4096, dtype=torch.float32, device=DEV))
    p, st = ops.ptr(t), ops.stream()
    assert rc("stp_grad_global_scale", p, 1024, 0.0, 1.0, p, p, 4095, st) == WORKSPACE
    assert rc("stp_grad_global_scale_dls", p, 1024, 0.0, 1.0, p, p, p, 4095, st) == WORKSPACE
    assert rc("stp_grad_global_scale", p, 1024, 0.0, 1.0, p, p, 0, st) == WORKSPACE
    for count in (0, -1):
        assert rc("stp_grad_global_scale", p, count, 0.0, 1.0, p, p, 4096, st) == BADARG
        assert rc("stp_grad_global_scale_dls", p, count, 0.0, 1.0, p, p, p, 4096, st) == BADARG
    assert rc("stp_grad_global_scale", p, 1024, 0.0, 1.0, None, p, 4096, st) == BADARG
    assert rc("stp_grad_global_scale", None, 1024, 0.0, 1.0, p, p, 4096, st) == BADARG
    assert rc("stp_grad_global_scale_dls", p, 1024, 0.0, 1.0, None, p, p, 4096, st) == BADARG
    assert rc("stp_grad_global_scale_dls", p, 1024, 0.0, 1.0, p, None, p, 4096, st) == BADARG
    assert rc("stp_grad_global_scale_dls", None, 1024, 0.0, 1.0, p, p, p, 4096, st) == BADARG
    torch.cuda.synchronize()
    assert torch.count_nonzero(t).item() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# stp_scale_by_device

def scale_input(count, dtype, seed=11):
    """Either sign, magnitudes in [2^-10, 2^10], rounded through the storage dtype: x * 0.25, x * 1 and x * 2 are exact in it."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(0, 2, count) * 2.0 - 1.0) * (1.0 + rng.random(count)) * 2.0 ** rng.integers(-10, 10, count)
    t = torch.from_numpy(x.astype(np.float32)).to(TD[dtype])
    assert float(t.abs().min()) >= 2.0 ** -10 and float(t.abs().max()) <= 2.0 ** 10
    return t


def call_scale(ops, x, count, mult, record):
    from segmentation_training_pipeline_amd import _lib
    _lib.call("stp_scale_by_device", ops.ptr(x), count, ops.dt(x), ops.ptr(mult), ops.ptr(record), ops.stream())


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("count", [1, 1027, 8192 * 256 + 1027])
def test_scale_by_device_is_bit_exact(ops, dtype, count):
    """x <- x * m with m read from device memory, m = 0.25 / 1 / 2: bit-equal to the exact product (counts off every vector width; the
    largest takes the grid-stride loop of the 8192-block grid into a second trip for 1027 elements).  record = NULL writes nothing
    else; with a record, record[0] = m and record[1..7] keep their bits.  64 canary elements behind x stay."""
    x0 = scale_input(count, dtype)
    canary = torch.full((GUARD,), CANARY, dtype=TD[dtype])
    for mult in (0.25, 1.0, 2.0):
        for with_record in (False, True):
            x = keep(torch.cat([x0, canary]).to(DEV))
            md = dev(np.array([mult, CANARY], np.float32))
            record = dev(np.full(8, CANARY, np.float32)) if with_record else None
            call_scale(ops, x, count, md, record)
            torch.cuda.synchronize()
            got = x.cpu()
            assert torch.equal(got[count:], canary)
            want = (x0.to(torch.float64) * mult).to(TD[dtype])
            assert torch.equal(want.to(torch.float64), x0.to(torch.float64) * mult)          # the product is exact in the storage dtype
            assert np.array_equal(bits(got[:count].view(torch.int16 if dtype != "fp32" else torch.int32).numpy()),
                                  bits(want.view(torch.int16 if dtype != "fp32" else torch.int32).numpy())), (mult, with_record)
            assert md.cpu().numpy().tolist() == [mult, CANARY]
            if with_record:
                assert record.cpu().numpy().tolist() == [mult] + [CANARY] * 7


@pytest.mark.parametrize("dtype", ["fp16"])
def test_scale_by_device_saturates_fp16_stores(ops, dtype):
    """Products beyond the largest finite half come back as +-65504, not inf: the saturating 16-bit store of the IEEE-half build
    (csrc/common.h).  Products inside the range next to them are exact."""
    x0 = torch.tensor([40000.0, -40000.0, 65504.0, -65504.0, 32752.0, -1.5, 30000.0], dtype=torch.float16)
    x = keep(torch.cat([x0, torch.full((GUARD,), CANARY, dtype=torch.float16)]).to(DEV))
    call_scale(ops, x, x0.numel(), dev(np.array([2.0], np.float32)), None)
    torch.cuda.synchronize()
    got = x.cpu().to(torch.float32).numpy()
    assert got[:7].tolist() == [65504.0, -65504.0, 65504.0, -65504.0, 65504.0, -3.0, 60000.0]
    assert (got[7:] == f32(CANARY)).all()


def test_scale_by_device_refusals(ops):
    """Not a dtype code, uint8, the OTHER build's 16-bit code, NULL pointers and empty ranges: STP_E_BADARG from either library."""
    from segmentation_training_pipeline_amd import _lib
    t = keep(torch.zeros(64, dtype=torch.float32, device=DEV))
    p, st = ops.ptr(t), ops.stream()
    for build, other in (("bf16", ops.F16), ("fp16", ops.BF16)):
        with _lib.storage(build):
            for code in (77, -1, ops.U8, other):
                assert rc("stp_scale_by_device", p, 8, code, p, None, st) == BADARG, (build, code)
            assert rc("stp_scale_by_device", None, 8, ops.F32, p, None, st) == BADARG
            assert rc("stp_scale_by_device", p, 8, ops.F32, None, None, st) == BADARG
            assert rc("stp_scale_by_device", p, 0, ops.F32, p, None, st) == BADARG
            assert rc("stp_scale_by_device", p, -8, ops.F32, p, None, st) == BADARG
    torch.cuda.synchronize()
    assert torch.count_nonzero(t).item() == 0
