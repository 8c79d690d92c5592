"""GPU tests of the per-object measurement kernels (csrc/measure.hip) at op level: stp_label_measure and stp_label_select (with
stp_label_select_workspace_bytes) against their host statement (tests/_measure_reference.py).  Everything is integer work: every
comparison is ``np.array_equal`` or ``==``, and every entry point runs twice with identical bytes.

Outputs are pre-filled with a poison value and carry one guard element past their end.  What keeps a case from being vacuous (object
counts, objects kept and dropped by every selection cell) is asserted on the reference side.

Inputs: the seeded Gaussian field of test_split_ops_gpu.py above 0.5 / 0.6 at 3 x 5, 64 x 64, 37 x 53, 70 x 133, 129 x 67 and 65 x 257,
labelled with the 8-neighbourhood and by ``_split_reference.split(mask, 2)`` (touching objects with ragged borders), the field itself as
channel 1 of a 3-channel map; the ``default_rng(5)`` salt image labelled with the 4-neighbourhood (903 objects, most of which miss the
workgroup's LDS table) under an independent random map; a checkerboard whose every pixel has its own label; all zeros; one label over
the whole image; stretches that cross a 64-pixel segment and a row boundary at w = 65 and 128; labels with gaps; out-of-range labels;
no map; NaN and out-of-range probabilities; two images whose sums pass 2^31 and 2^32; one 768 x 768 field."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import _measure_reference as M
import _split_reference as S

pytestmark = pytest.mark.gpu

FIELD_SIZES = [(3, 5), (64, 64), (37, 53), (70, 133), (129, 67), (65, 257)]
THRESHOLDS = (0.5, 0.6)
CELLS = ((0, 0.0), (8, 0.5), (0, 0.6), (20, 0.55))
SALT_CELLS = ((0, 0.3), (0, 0.5), (0, 0.7))
POISON = -5
BADARG, WORKSPACE = -1, -3


def the_reference_states_the_library():
    """The reference's constants are the public ones and the entry points it restates exist: a test of the reference alone starts here."""
    from segmentation_pipeline.segmentation import PipelineConfig
    from segmentation_training_pipeline_amd import _lib
    assert (M.CONF_ONE, M.CONF_DEN) == (PipelineConfig.CONF_ONE, PipelineConfig.CONF_DEN)
    assert "stp_label_measure" in _lib.SIGNATURES and "stp_label_select" in _lib.SIGNATURES


def field(h, w):
    rng = np.random.default_rng(1000 * h + w)
    f = ndimage.gaussian_filter(rng.random((h, w)), 2.0)
    return ((f - f.min()) / (f.max() - f.min())).astype(np.float32)


def three_channels(f, seed=9):
    """The map ``f`` as channel 1 of a 3-channel map whose other channels hold other values."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([1 - f, f, rng.random(f.shape).astype(np.float32)], axis=2))


def crossing(w):
    """Label 3 runs from x = 60 over the 64-pixel boundary to the end of row 1 and on through the first pixels of row 2; label 2 fills the
    rest of row 2, label 7 a block that starts at x = 63."""
    lab = np.zeros((5, w), np.int32)
    lab[1, 60:] = 3
    lab[2, :5] = 3
    lab[2, 5:] = 2
    lab[3:5, 63:min(w, 70)] = 7
    return lab


def make_inputs():
    """name -> (int32 labels, label_cap, probs [h, w, C] or None, channel)."""
    out = {}
    for s in FIELD_SIZES:
        f = field(*s)
        for thr in THRESHOLDS:
            l8 = ndimage.label(f > thr, np.ones((3, 3)))[0].astype(np.int32)
            out["field_%dx%d_%g_l8" % (s + (thr,))] = (l8, int(l8.max()), three_channels(f), 1)
            sp, n = S.split((f > thr).astype(np.uint8), 2)
            out["field_%dx%d_%g_split" % (s + (thr,))] = (sp, n, three_channels(f), 1)
    rng = np.random.default_rng(5)
    salt = ndimage.label(rng.random((70, 133)) < 0.45)[0].astype(np.int32)
    out["salt"] = (salt, int(salt.max()), np.random.default_rng(6).random((70, 133, 1)).astype(np.float32), 0)
    h, w = 33, 35
    board = np.indices((h, w)).sum(axis=0) % 2 == 0
    out["per_pixel"] = (np.where(board, np.arange(1, h * w + 1).reshape(h, w), 0).astype(np.int32), h * w, three_channels(field(h, w)), 1)
    out["zeros_cap0"] = (np.zeros((37, 53), np.int32), 0, three_channels(field(37, 53)), 1)
    out["zeros_cap5"] = (np.zeros((37, 53), np.int32), 5, None, 0)
    for s in ((1, 1), (1, 130), (130, 1), (37, 53)):
        out["one_%dx%d" % s] = (np.ones(s, np.int32), 1, three_channels(field(*s)) if min(s) > 1 else np.full(s + (1,), 0.75, np.float32),
                                1 if min(s) > 1 else 0)
        out["ones_map_%dx%d" % s] = (np.ones(s, np.int32), 1, np.ones(s + (2,), np.float32), 1)
    for w in (65, 128):
        out["crossing_%d" % w] = (crossing(w), 7, three_channels(field(5, w)), 1)
    gaps = np.zeros((37, 53), np.int32)
    gaps[3:9, 4:40] = 5
    gaps[20:30, 10:50] = 9
    gaps[25, 11] = 5                                                        # a pixel of 5 inside 9: its box spans both
    out["gaps_cap9"] = (gaps, 9, three_channels(field(37, 53)), 1)
    out["gaps_cap12"] = (gaps, 12, three_channels(field(37, 53)), 1)
    wild = ndimage.label(field(70, 133) > 0.5, np.ones((3, 3)))[0].astype(np.int32)
    wild[wild == 2] = -2
    wild[wild == 5] = 70 * 133 + 1
    wild[0, :3] = (-2147483648, 2147483647, 8)
    out["out_of_range"] = (wild, 7, three_channels(field(70, 133)), 1)
    out["no_probs"] = (out["field_70x133_0.5_l8"][0], 7, None, 0)
    special = field(37, 53).copy()
    special[::3, ::2] = np.nan
    special[1::3, ::2] = -0.5
    special[2::3, ::2] = 1.5
    special[5, 5], special[6, 6] = np.inf, -np.inf
    out["special_probs"] = (np.ones((37, 53), np.int32) + (np.arange(53)[None, :] > 30), 2, three_channels(special), 1)
    return out


INPUTS = make_inputs()
NAMES = sorted(INPUTS)


@pytest.fixture(scope="module")
def reference():
    """Per input: (sums, boxes, out_of_range); computed once and not modified."""
    return {n: M.measure(INPUTS[n][0], INPUTS[n][1], INPUTS[n][2], INPUTS[n][3]) for n in NAMES}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def workspace(nbytes):
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 8 == 0
    return ws


def guarded(n, dtype, poison=POISON):
    """A device buffer of n elements and one guard element, all poison."""
    return torch.full((n + 1,), poison, dtype=dtype, device="cuda")


def finish(buf, shape, poison=POISON):
    got = buf.cpu().numpy()
    assert got[-1] == poison                                                # the guard element
    return got[:-1].reshape(shape)


def run_measure(labels, cap, probs=None, channel=0):
    """-> (sums, boxes, out_of_range) of one stp_label_measure call."""
    from segmentation_training_pipeline_amd import ops
    h, w = labels.shape
    sums, boxes, outside = guarded(4 * (cap + 1), torch.int64), guarded(4 * (cap + 1), torch.int32), guarded(1, torch.int64)
    C = 1 if probs is None else probs.shape[2]
    ops.label_measure(dev(labels), None if probs is None else dev(probs), h, w, C, channel, cap, sums[:-1], boxes[:-1], outside[:1])
    return finish(sums, (cap + 1, 4)), finish(boxes, (cap + 1, 4)), int(finish(outside, (1,))[0])


def run_select(labels, cap, sums, boxes, min_area, num, den=M.CONF_DEN, in_place=False):
    """-> (labels, count, sums, boxes) of one stp_label_select call; the rows past the count must still hold the poison."""
    from segmentation_training_pipeline_amd import ops
    h, w = labels.shape
    if in_place:
        out = torch.cat([dev(labels).reshape(-1), torch.full((1,), POISON, dtype=torch.int32, device="cuda")])
        src = out[:h * w]
    else:
        out, src = guarded(h * w, torch.int32), dev(labels)
    count = guarded(1, torch.int32)
    out_sums, out_boxes = guarded(4 * (cap + 1), torch.int64), guarded(4 * (cap + 1), torch.int32)
    ops.label_select(src, h, w, cap, dev(sums), dev(boxes), min_area, num, den, out[:h * w], count[:1], out_sums[:-1], out_boxes[:-1],
                     workspace(ops.label_select_workspace_bytes(cap)))
    n = int(finish(count, (1,))[0])
    s, b = finish(out_sums, (cap + 1, 4)), finish(out_boxes, (cap + 1, 4))
    assert 0 <= n <= cap and (s[n + 1:] == POISON).all() and (b[n + 1:] == POISON).all()
    return finish(out, (h, w)), n, s[:n + 1], b[:n + 1]


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(g, v) and np.asarray(g).dtype == np.asarray(v).dtype for g, v in zip(got, want))


# ------------------------------------------------------------------------------------------------ the inputs are what they are meant to be
def test_reference_side_properties(reference):
    the_reference_states_the_library()
    kept = {}
    for s in FIELD_SIZES[1:]:
        n = "field_%dx%d_0.5_l8" % s
        labels, cap, probs, ch = INPUTS[n]
        kept[s] = [cap] + [M.measure_select(labels, probs, ch, a, c)[1] for a, c in CELLS[1:]]
        assert all(0 < k < cap for k in kept[s][1:]), s                     # every cell keeps an object and drops one
    assert kept == {(37, 53): [2, 1, 1, 1], (64, 64): [4, 3, 3, 2], (70, 133): [7, 6, 3, 5], (129, 67): [37, 32, 2, 16],
                    (65, 257): [27, 19, 8, 12]}
    labels, cap, probs, ch = INPUTS["salt"]
    assert cap == 903 and [M.measure_select(labels, probs, ch, a, c)[1] for a, c in SALT_CELLS] == [710, 434, 167]
    assert INPUTS["field_70x133_0.5_split"][1] == 25 and INPUTS["field_129x67_0.5_split"][1] == 53      # more objects than components
    assert reference["out_of_range"][2] == int((INPUTS["out_of_range"][0] == -2).sum() + (INPUTS["out_of_range"][0] == 9311).sum()) + 3 > 100
    assert reference["out_of_range"][0][[2, 5], 0].tolist() == [0, 0] and (reference["out_of_range"][0][[1, 3, 4, 6, 7], 0] > 0).all()
    assert reference["gaps_cap12"][0][:, 0].tolist() == [0, 0, 0, 0, 0, 217, 0, 0, 0, 399, 0, 0, 0]
    assert reference["gaps_cap12"][1][5].tolist() == [3, 4, 25, 39] and reference["gaps_cap12"][1][10].tolist() == [37, 53, -1, -1]
    assert reference["per_pixel"][0][1:, 0].sum() == 578 and set(reference["per_pixel"][0][:, 0].tolist()) == {0, 1}
    for w in (65, 128):
        assert reference["crossing_%d" % w][1][3].tolist() == [1, 0, 2, w - 1] and reference["crossing_%d" % w][0][3, 0] == w - 60 + 5
    q = M.quantise(INPUTS["special_probs"][2][:, :, 1])
    assert (q == 0).sum() > 500 and (q == 65535).sum() > 300 and reference["special_probs"][0][1:, 3].tolist() == [int(q[:, :31].sum()),
                                                                                                                   int(q[:, 31:].sum())]
    assert (reference["no_probs"][0][:, 3] == 0).all() and np.array_equal(reference["no_probs"][0][:, :3], reference["field_70x133_0.5_l8"][0][:, :3])


# ------------------------------------------------------------------------------------------------ stp_label_measure
@pytest.mark.parametrize("name", NAMES)
def test_measure_equals_the_reference(reference, name):
    labels, cap, probs, ch = INPUTS[name]
    got = run_measure(labels, cap, probs, ch)
    want = reference[name]
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], name
    again = run_measure(labels, cap, probs, ch)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes() and got[2] == again[2]


def test_a_larger_cap_only_adds_empty_rows(reference):
    labels, cap, probs, ch = INPUTS["field_129x67_0.5_l8"]
    sums, boxes, outside = run_measure(labels, 129 * 67, probs, ch)
    assert outside == 0 and np.array_equal(sums[:cap + 1], reference["field_129x67_0.5_l8"][0]) and (sums[cap + 1:] == 0).all()
    assert np.array_equal(boxes[:cap + 1], reference["field_129x67_0.5_l8"][1]) and (boxes[cap + 1:] == (129, 67, -1, -1)).all()


@pytest.mark.parametrize("h,w,with_probs", [(1100, 2049, True), (2100, 2049, False)])
def test_sums_beyond_32_bits(h, w, with_probs):
    """One label over the whole image: closed forms, so that the reference itself cannot overflow unnoticed.  A 32-bit accumulator
    anywhere fails: at 1100 x 2049 the sum of x passes 2^31 and the sum of q 2^32; at 2100 x 2049 the sum of x passes 2^32."""
    labels = np.ones((h, w), np.int32)
    probs = np.ones((h, w, 1), np.float32) if with_probs else None
    want_sums = [h * w, w * (h * (h - 1) // 2), h * (w * (w - 1) // 2), 65535 * h * w if with_probs else 0]
    assert want_sums[2] == (2307993600 if h == 1100 else 4406169600) and want_sums[2] > (2 ** 31 if h == 1100 else 2 ** 32)
    assert not with_probs or want_sums[3] > 2 ** 32
    sums, boxes, outside = run_measure(labels, 1, probs, 0)
    assert outside == 0 and sums.tolist() == [[0, 0, 0, 0], want_sums] and boxes.tolist() == [[h, w, -1, -1], [0, 0, h - 1, w - 1]]
    assert sums.tobytes() == run_measure(labels, 1, probs, 0)[0].tobytes()
    if with_probs:                                                          # (1, 1.0) on the all-ones map: exactly on the bound
        out, n, s, b = run_select(labels, 1, sums, boxes, 1, 10000)
        assert n == 1 and (out == 1).all() and np.array_equal(s, sums) and np.array_equal(b, boxes)


def test_a_768_field():
    f = field(768, 768)
    labels, cap = S.split((f > 0.5).astype(np.uint8), 16)
    assert cap > 150
    probs = three_channels(f)
    want = M.measure(labels, cap, probs, 1)
    got = run_measure(labels, cap, probs, 1)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == 0
    assert got[0].tobytes() == run_measure(labels, cap, probs, 1)[0].tobytes()
    for min_area, conf in CELLS[1:]:
        w = M.select(labels, cap, want[0], want[1], min_area, M.conf_num(conf))
        assert 0 < w[1] < cap
        g = run_select(labels, cap, got[0], got[1], min_area, M.conf_num(conf))
        assert g[1] == w[1] and same(g, w), (min_area, conf)
    sums, boxes, outside = run_measure(np.ones((768, 768), np.int32), 768 * 768, probs, 1)      # one object, the largest cap
    q = int(M.quantise(f).sum())
    assert sums[1].tolist() == [768 * 768, 768 * (768 * 767 // 2), 768 * (768 * 767 // 2), q] and boxes[1].tolist() == [0, 0, 767, 767]
    assert (sums[2:] == 0).all() and (sums[0] == 0).all() and outside == 0


# ------------------------------------------------------------------------------------------------ stp_label_select
@pytest.mark.parametrize("name", NAMES)
def test_select_equals_the_reference(reference, name):
    labels, cap, probs, ch = INPUTS[name]
    sums, boxes, _ = reference[name]
    for min_area, conf in CELLS + (SALT_CELLS if name == "salt" else ()) + ((1, 1.0),):
        num = M.conf_num(conf)
        want = M.select(labels, cap, sums, boxes, min_area, num)
        got = run_select(labels, cap, sums, boxes, min_area, num)
        assert got[1] == want[1] and same(got, want), (name, min_area, conf)
        in_place = run_select(labels, cap, sums, boxes, min_area, num, in_place=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got[::2] + got[3:], in_place[::2] + in_place[3:])), (name, min_area, conf)
    if name.startswith("ones_map"):
        assert run_select(labels, cap, sums, boxes, 1, 10000)[1] == 1       # (1, 1.0) on the all-ones map: exactly on the bound, kept
    if name.endswith("_l8") or name == "salt":
        got = run_select(labels, cap, sums, boxes, 0, 0)                    # neutral: the identity on a contiguous labelling
        assert got[1] == cap and np.array_equal(got[0], labels) and np.array_equal(got[2], sums) and np.array_equal(got[3], boxes)


def test_select_with_other_denominators(reference):
    labels, cap, probs, ch = INPUTS["field_129x67_0.5_l8"]
    sums, boxes, _ = reference["field_129x67_0.5_l8"]
    seen = set()
    for num, den in ((1, 2), (11, 20), (3, 5), (1, 1), (0, 1), (5501, 10000)):
        want = M.select(labels, cap, sums, boxes, 4, num, den)
        got = run_select(labels, cap, sums, boxes, 4, num, den)
        assert got[1] == want[1] and same(got, want), (num, den)
        seen.add(want[1])
    assert len(seen) >= 4


def test_measure_then_select_on_the_device(reference):
    """The chain as the pipeline runs it: the table never leaves the device between the two entry points."""
    from segmentation_training_pipeline_amd import ops
    for name in ("field_65x257_0.5_split", "salt", "out_of_range"):
        labels, cap, probs, ch = INPUTS[name]
        h, w = labels.shape
        dl = dev(labels)
        sums = torch.empty((cap + 1, 4), dtype=torch.int64, device="cuda")
        boxes = torch.empty((cap + 1, 4), dtype=torch.int32, device="cuda")
        outside, count = torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda")
        out_sums, out_boxes = torch.full_like(sums, POISON), torch.full_like(boxes, POISON)
        ops.label_measure(dl, dev(probs), h, w, probs.shape[2], ch, cap, sums, boxes, outside)
        ops.label_select(dl, h, w, cap, sums, boxes, 6, 5200, 10000, dl, count, out_sums, out_boxes,
                         workspace(ops.label_select_workspace_bytes(cap)))
        want = M.select(labels, cap, reference[name][0], reference[name][1], 6, 5200)
        n = int(count.item())
        assert 0 < n == want[1] < cap and np.array_equal(dl.cpu().numpy(), want[0])
        assert np.array_equal(out_sums[:n + 1].cpu().numpy(), want[2]) and np.array_equal(out_boxes[:n + 1].cpu().numpy(), want[3])
        again = M.measure(want[0], n, probs, ch)                            # and the compacted rows are the new image's own table
        assert np.array_equal(again[0], want[2]) and np.array_equal(again[1], want[3])


# ------------------------------------------------------------------------------------------------ refusals: none launches anything
def test_refusals():
    from segmentation_training_pipeline_amd import _lib, ops
    h, w, cap = 37, 53, 9
    lib = _lib.load()
    labels = dev(INPUTS["gaps_cap9"][0])
    probs = dev(INPUTS["gaps_cap9"][2])
    sums = torch.full((cap + 1, 4), POISON, dtype=torch.int64, device="cuda")
    boxes = torch.full((cap + 1, 4), POISON, dtype=torch.int32, device="cuda")
    sums2, boxes2 = sums.clone(), boxes.clone()
    out = torch.full((h * w,), POISON, dtype=torch.int32, device="cuda")
    words = torch.full((2,), POISON, dtype=torch.int64, device="cuda")
    count = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
    need = ops.label_select_workspace_bytes(cap)
    assert need == lib.stp_label_select_workspace_bytes(cap) > 0 and ops.label_select_workspace_bytes(-1) == 0
    ws = workspace(need + 8)
    p = lambda t: t.data_ptr()                                              # noqa: E731
    measure = lambda **kw: lib.stp_label_measure(*[dict(dict(l=p(labels), p=p(probs), h=h, w=w, C=3, ch=1, cap=cap, s=p(sums), b=p(boxes),  # noqa: E731
                                                             o=p(words)), **kw)[k] for k in ("l", "p", "h", "w", "C", "ch", "cap", "s", "b", "o")], None)
    select = lambda **kw: lib.stp_label_select(*[dict(dict(l=p(labels), h=h, w=w, cap=cap, s=p(sums), b=p(boxes), a=0, n=0, d=10000,  # noqa: E731
                                                           o=p(out), c=p(count), os=p(sums2), ob=p(boxes2), ws=p(ws), nb=need), **kw)[k]
                                                 for k in ("l", "h", "w", "cap", "s", "b", "a", "n", "d", "o", "c", "os", "ob", "ws", "nb")], None)
    for hh, ww in ((0, w), (h, 0), (-1, w), (32768, 1), (1, 32768)):        # sizes below 1 and above the bound
        assert measure(h=hh, w=ww, cap=0) == BADARG and select(h=hh, w=ww, cap=0) == BADARG
    for kw in ({"l": None}, {"s": None}, {"b": None}, {"o": None}, {"cap": -1}, {"cap": h * w + 1}, {"C": 0}, {"ch": 3}, {"ch": -1},
               {"s": p(sums) + 4}, {"o": p(words) + 4}):
        assert measure(**kw) == BADARG, kw
    for kw in ({"l": None}, {"s": None}, {"b": None}, {"o": None}, {"c": None}, {"os": None}, {"ob": None}, {"ws": None}, {"cap": -1},
               {"cap": h * w + 1}, {"a": -1}, {"n": -1}, {"n": 10001}, {"d": 0}, {"d": 10001}, {"n": 3, "d": 2}, {"os": p(sums)},
               {"ob": p(boxes)}, {"ws": p(ws) + 4}):
        assert select(**kw) == BADARG, kw
    assert select(nb=need - 1) == WORKSPACE
    with pytest.raises(_lib.StpError, match="BADARG"):                      # aliased tables
        ops.label_select(labels, h, w, cap, sums, boxes, 0, 0, 10000, out, count, sums, boxes2, ws)
    with pytest.raises(_lib.StpError, match="BADARG"):
        ops.label_select(labels, h, w, cap, sums, boxes, 0, 0, 10000, out, count, sums2, boxes, ws)
    with pytest.raises(_lib.StpError, match="WORKSPACE"):
        ops.label_select(labels, h, w, cap, sums, boxes, 0, 0, 10000, out, count, sums2, boxes2, ws[:need - 1])
    with pytest.raises(_lib.StpError, match="BADARG"):
        ops.label_measure(labels, probs, h, w, 3, 3, cap, sums, boxes, words[:1])
    torch.cuda.synchronize()
    for t in (sums, boxes, sums2, boxes2, out, words, count):               # nothing was launched
        assert (t.cpu().numpy() == POISON).all()
