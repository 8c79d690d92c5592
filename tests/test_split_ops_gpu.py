"""GPU tests of the object-splitting kernels (csrc/split.hip) at op level: stp_mask_edt, stp_edt_threshold, stp_label_grow,
stp_label_unclaimed and stp_label_merge (with stp_mask_edt_workspace_bytes, stp_label_grow_workspace_bytes, stp_label_grow_rounds)
against their host statements (tests/_split_reference.py: scipy's distance transform, the synchronous growth iteration).  Everything
is exact integer work: every comparison is ``np.array_equal``, and every entry point runs twice with identical bytes.

Outputs are pre-filled with a poison value and carry one guard element past their end.  What keeps a case from being vacuous (cores,
components without a core, object counts that differ from the plain labelling) is asserted on the reference side.

Inputs: the seeded Gaussian field of test_components_ops_gpu.py above 0.35 / 0.5 at 3 x 5, 64 x 64, 37 x 53, 70 x 133, 129 x 67 and
65 x 257 (smaller than a 64-pixel row segment, one segment, several, odd sizes, several 32-column strips and 64-row chunks) with c2 in
{0, 2, 6, 16}; the two ``default_rng(5)`` salt images; a serpentine grown from one seed in a corner (thousands of synchronous rounds:
the "call again" path); a checkerboard, all zeros, all ones (the no-background rule); one zero pixel in a corner of 130 x 300 (the
longest search); one row, one column, one pixel; 1024 x 33 and 1030 x 37, the tallest strip the column pass holds in LDS and one taller; hand-placed seeds with
ties; one 768 x 768 field."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import _split_reference as R

pytestmark = pytest.mark.gpu

FIELD_SIZES = [(3, 5), (64, 64), (37, 53), (70, 133), (129, 67), (65, 257)]
THRESHOLDS = (0.35, 0.5)
C2S = (0, 2, 6, 16)
POISON = -5
BADARG, WORKSPACE = -1, -3


def field(h, w):
    rng = np.random.default_rng(1000 * h + w)
    f = ndimage.gaussian_filter(rng.random((h, w)), 2.0)
    return ((f - f.min()) / (f.max() - f.min())).astype(np.float32)


def make_inputs():
    out = {}
    for s in FIELD_SIZES:
        f = field(*s)
        for thr in THRESHOLDS:
            out["field_%dx%d_%g" % (s + (thr,))] = (f > thr).astype(np.uint8)
    rng = np.random.default_rng(5)                                          # ONE generator: the second image is its second draw
    out["salt_0.45"] = (rng.random((70, 133)) < 0.45).astype(np.uint8)
    out["salt_0.6"] = (rng.random((70, 133)) < 0.6).astype(np.uint8)
    out["serpentine"] = R.serpentine(67, 71)
    out["checkerboard"] = (np.indices((33, 35)).sum(axis=0) % 2 == 0).astype(np.uint8)
    for s in ((1, 1), (1, 130), (130, 1), (37, 53)):
        out["zeros_%dx%d" % s] = np.zeros(s, np.uint8)
        out["ones_%dx%d" % s] = np.full(s, 255, np.uint8)                   # any non-zero byte is mask
    out["dots_1x130"] = (np.arange(130)[None, :] % 7 != 0).astype(np.uint8)
    out["dots_130x1"] = (np.arange(130)[:, None] % 7 != 0).astype(np.uint8)
    corner = np.ones((130, 300), np.uint8)
    corner[129, 299] = 0
    out["corner_130x300"] = corner
    tall = (field(1030, 37) > 0.45).astype(np.uint8)
    tall[200:900, 5:30] = 1                                                 # a block whose nearest zeros lie hundreds of rows away
    out["tall_1030x37"] = tall
    out["edge_1024x33"] = (field(1024, 33) > 0.5).astype(np.uint8)          # the tallest strip LDS holds, and a second strip of 1 column
    out["two_discs"] = R.two_discs()
    return out


INPUTS = make_inputs()
NAMES = sorted(INPUTS)


@pytest.fixture(scope="module")
def reference():
    """Per input: its D2 and, per c2, (core labels, nc, split labels, count); computed once and not modified."""
    ref = {}
    for n in NAMES:
        ref[n] = {"d2": R.edt2(INPUTS[n])}
        for c2 in C2S:
            _, seeds, nc = R.cores(INPUTS[n], c2)
            ref[n][c2] = (seeds, nc) + R.split(INPUTS[n], c2)
    return ref


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
    assert got[-1] == (poison if got.dtype != np.uint8 else poison & 0xff)      # the guard element
    return got[:-1].reshape(shape)


def run_edt(mask):
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    d2 = guarded(h * w, torch.int32)
    ops.mask_edt(dev(mask), h, w, d2[:h * w], workspace(ops.mask_edt_workspace_bytes(h, w)))
    return finish(d2, (h, w))


def run_threshold(d2, c2):
    from segmentation_training_pipeline_amd import ops
    h, w = d2.shape
    out = guarded(h * w, torch.uint8, 7)
    ops.edt_threshold(dev(d2), h, w, c2, out[:h * w])
    return finish(out, (h, w), 7)


def run_grow_call(mask, seeds):
    """ONE stp_label_grow call -> (labels, the changed word)."""
    from segmentation_training_pipeline_amd import _lib, ops
    h, w = mask.shape
    labels, changed = guarded(h * w, torch.int32), guarded(1, torch.int32)
    ws = workspace(ops.label_grow_workspace_bytes(h, w))
    m, s = dev(mask), dev(seeds.astype(np.int32))
    rc = _lib.load().stp_label_grow(m.data_ptr(), s.data_ptr(), h, w, labels.data_ptr(), changed.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return finish(labels, (h, w)), int(finish(changed, (1,))[0])


def run_grow(mask, seeds, in_place=False):
    """The wrapper, which calls until nothing changes -> (labels, calls)."""
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    changed = guarded(1, torch.int32)
    ws = workspace(ops.label_grow_workspace_bytes(h, w))
    if in_place:
        labels = torch.cat([dev(seeds.astype(np.int32)).reshape(-1), torch.full((1,), POISON, dtype=torch.int32, device="cuda")])
        calls = ops.label_grow(dev(mask), labels[:h * w], h, w, labels[:h * w], changed[:1], ws)
    else:
        labels = guarded(h * w, torch.int32)
        calls = ops.label_grow(dev(mask), dev(seeds.astype(np.int32)), h, w, labels[:h * w], changed[:1], ws)
    assert finish(changed, (1,))[0] == 0
    return finish(labels, (h, w)), calls


def run_unclaimed(mask, labels):
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    out = guarded(h * w, torch.uint8, 7)
    ops.label_unclaimed(dev(mask), dev(labels.astype(np.int32)), h, w, out[:h * w])
    return finish(out, (h, w), 7)


def run_merge(rest, nc, nr, labels):
    from segmentation_training_pipeline_amd import ops
    h, w = rest.shape
    buf = torch.cat([dev(labels.astype(np.int32)).reshape(-1), torch.full((1,), POISON, dtype=torch.int32, device="cuda")])
    total = guarded(1, torch.int32)
    ops.label_merge(dev(rest.astype(np.int32)), dev(np.array([nc], np.int32)), dev(np.array([nr], np.int32)), h, w, buf[:h * w], total[:1])
    return finish(buf, (h, w)), int(finish(total, (1,))[0])


def run_split(mask, c2):
    """Steps 1 to 4 on the device, the counts never leaving it -> (labels, count)."""
    from segmentation_training_pipeline_amd import ops
    h, w = mask.shape
    m = dev(mask)
    d2 = torch.empty((h, w), dtype=torch.int32, device="cuda")
    ops.mask_edt(m, h, w, d2, workspace(ops.mask_edt_workspace_bytes(h, w)))
    part = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    ops.edt_threshold(d2, h, w, c2, part)
    labels, rest = guarded(h * w, torch.int32), torch.empty((h, w), dtype=torch.int32, device="cuda")
    counts = guarded(4, torch.int32)                                         # nc, nr, total, changed
    lws = workspace(ops.mask_label_workspace_bytes(h, w))
    ops.mask_label(part, h, w, 2, 0, labels[:h * w], counts[0:1], lws)
    ops.label_grow(m, labels[:h * w], h, w, labels[:h * w], counts[3:4], workspace(ops.label_grow_workspace_bytes(h, w)))
    ops.label_unclaimed(m, labels[:h * w], h, w, part)
    ops.mask_label(part, h, w, 2, 0, rest, counts[1:2], lws)
    ops.label_merge(rest, counts[0:1], counts[1:2], h, w, labels[:h * w], counts[2:3])
    c = finish(counts, (4,))
    assert c[2] == c[0] + c[1] and c[3] == 0
    return finish(labels, (h, w)), int(c[2])


# ------------------------------------------------------------------------------------------------ the inputs are what they are meant to be
def test_reference_side_properties(reference):
    counts = {n: [reference[n][c2][3] for c2 in C2S] for n in NAMES}
    nc = {n: [reference[n][c2][1] for c2 in C2S] for n in NAMES}
    assert counts["field_70x133_0.5"] == [7, 25, 38, 34] and nc["field_70x133_0.5"] == [7, 23, 36, 29]      # cores and coreless components
    assert counts["field_129x67_0.5"] == [37, 53, 55, 44] and nc["field_129x67_0.5"] == [37, 43, 39, 16]
    assert counts["field_65x257_0.5"] == [27, 42, 67, 60] and counts["field_64x64_0.5"] == [4, 5, 10, 12]
    assert counts["field_3x5_0.35"] == [1, 1, 1, 1] and nc["field_3x5_0.35"] == [1, 1, 1, 0]                # c2 = 16: no core at 3 x 5
    assert counts["two_discs"] == [1, 1, 1, 1] and R.split(INPUTS["two_discs"], 64)[1] == 2
    assert counts["salt_0.45"] == [105, 111, 105, 105] and nc["salt_0.45"] == [105, 9, 0, 0]                # salt has few cores, then none
    assert counts["salt_0.6"] == [11, 71, 11, 11] and nc["salt_0.6"] == [11, 61, 1, 0]
    assert counts["tall_1030x37"] == [15, 30, 59, 73] and nc["tall_1030x37"] == [15, 20, 46, 59]
    assert int(reference["corner_130x300"]["d2"].max()) == 129 * 129 + 299 * 299
    assert int(reference["tall_1030x37"]["d2"].max()) > 12 * 12                                            # found beyond +-12 rows
    for s in ((1, 1), (1, 130), (130, 1), (37, 53)):
        assert (reference["ones_%dx%d" % s]["d2"] == R.NO_BACKGROUND).all() and counts["ones_%dx%d" % s] == [1] * 4
        assert counts["zeros_%dx%d" % s] == [0] * 4
    assert counts["checkerboard"] == [1, 1, 1, 1] and nc["checkerboard"] == [1, 0, 0, 0]                    # D2 = 1 everywhere: no core, one object


# ------------------------------------------------------------------------------------------------ stp_mask_edt, stp_edt_threshold
@pytest.mark.parametrize("name", NAMES)
def test_edt_equals_scipy(reference, name):
    m = INPUTS[name]
    got = run_edt(m)
    assert got.dtype == np.int32 and np.array_equal(got, reference[name]["d2"]), name
    assert got.tobytes() == run_edt(m).tobytes()
    for c2 in C2S + (169, 2147483646):
        core = run_threshold(got, c2)
        assert np.array_equal(core, (reference[name]["d2"] > c2).astype(np.uint8)), (name, c2)
    assert run_threshold(got, 6).tobytes() == run_threshold(got, 6).tobytes()


# ------------------------------------------------------------------------------------------------ stp_label_grow
@pytest.mark.parametrize("name", NAMES)
def test_grow_from_the_cores_equals_the_iteration(reference, name):
    m = INPUTS[name]
    for c2 in C2S:
        seeds = reference[name][c2][0]
        want = R.grow(m, seeds)
        got, calls = run_grow(m, seeds)
        assert np.array_equal(got, want) and calls >= 1, (name, c2)
        again, _ = run_grow(m, seeds, in_place=True)
        assert got.tobytes() == again.tobytes(), (name, c2)


def test_grow_calls_again_until_nothing_changes():
    from segmentation_training_pipeline_amd import _lib
    per_call = _lib.load().stp_label_grow_rounds()
    assert per_call == 32
    m = INPUTS["serpentine"]
    seeds = np.zeros(m.shape, np.int32)
    seeds[0, 0] = 67 * 71                                                   # the largest label an image of this size can hold
    want, rounds = R.grow(m, seeds, return_rounds=True)
    assert rounds == 2380 and (want[m != 0] == 67 * 71).all()               # the corner seed reaches all 2447 pixels, one step a round
    got, changed = run_grow_call(m, seeds)                                  # ONE call: exactly 32 rounds, and more to come
    assert changed == 1 and np.array_equal(got, R.grow(m, seeds, max_rounds=per_call))
    again, changed = run_grow_call(m, seeds)
    assert changed == 1 and got.tobytes() == again.tobytes()
    full, calls = run_grow(m, seeds)
    assert np.array_equal(full, want) and calls == rounds // per_call + 1
    one, changed = run_grow_call(m, want)                                   # a final state: the first round finds nothing, 31 do nothing
    assert changed == 0 and np.array_equal(one, want)


def test_grow_ties_and_arbitrary_seeds():
    m = np.ones((7, 11), np.uint8)
    seeds = np.zeros((7, 11), np.int32)
    seeds[3, 0], seeds[3, 10] = 77, 5                                       # 77 = h * w; column 5 is 5 steps from either
    want = R.grow(m, seeds)
    assert (want[:, :5] == 77).all() and (want[:, 5:] == 5).all() and np.array_equal(want, R.grow_lexicographic(m, seeds))
    assert np.array_equal(run_grow(m, seeds)[0], want)
    m = INPUTS["field_70x133_0.35"]
    rng = np.random.default_rng(11)
    seeds = np.where(rng.random(m.shape) < 0.01, rng.integers(1, 70 * 133 + 1, m.shape), 0).astype(np.int32)      # on and off the foreground
    seeds[np.nonzero(m)[0][0], np.nonzero(m)[1][0]] = 70 * 133
    want = R.grow(m, seeds)
    assert np.array_equal(want, R.grow_lexicographic(m, seeds)) and len(np.unique(want)) > 20 and (want[m == 0] == 0).all()
    assert (seeds[m == 0] != 0).any()                                       # seeds off the foreground, which are dropped
    got, _ = run_grow(m, seeds)
    assert np.array_equal(got, want) and got.tobytes() == run_grow(m, seeds)[0].tobytes()


# ------------------------------------------------------------------------------------------------ stp_label_unclaimed, stp_label_merge
@pytest.mark.parametrize("name", ["field_70x133_0.5", "salt_0.45", "checkerboard", "zeros_37x53", "ones_1x130"])
def test_unclaimed_and_merge(reference, name):
    m = INPUTS[name]
    for c2 in (2, 16):
        seeds, nc, want, count = reference[name][c2]
        grown = R.grow(m, seeds)
        left = run_unclaimed(m, grown)
        assert np.array_equal(left, ((m != 0) & (grown == 0)).astype(np.uint8)) and left.tobytes() == run_unclaimed(m, grown).tobytes()
        rest, nr = R.label(left, 2)
        got, total = run_merge(rest, nc, nr, grown)
        assert total == count == nc + nr and np.array_equal(got, want), (name, c2)
        assert got.tobytes() == run_merge(rest, nc, nr, grown)[0].tobytes()


# ------------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("name", NAMES)
def test_split_equals_the_reference(reference, name):
    m = INPUTS[name]
    for c2 in C2S:
        _, _, want, count = reference[name][c2]
        got, n = run_split(m, c2)
        assert n == count and np.array_equal(got, want), (name, c2)
        if c2 == 0:
            assert np.array_equal(got, R.label(m, 2)[0])                    # the whole mask is core: the plain labelling
    assert run_split(m, 6)[0].tobytes() == run_split(m, 6)[0].tobytes()


def test_the_two_discs_come_apart():
    got, n = run_split(R.two_discs(), 64)
    assert n == 2 and np.bincount(got.ravel())[1:].tolist() == [440, 431]
    got, n = run_split(R.two_discs(), 169)
    assert n == 1 and np.array_equal(got, R.two_discs().astype(np.int32))


def test_a_768_field():
    m = (field(768, 768) > 0.5).astype(np.uint8)
    d2 = R.edt2(m)
    assert np.array_equal(run_edt(m), d2)
    want, count = R.split(m, 16)
    plain = R.label(m, 2)[1]
    assert count > plain > 100 and R.cores(m, 16)[2] < count              # necks cut, and components without a core
    got, n = run_split(m, 16)
    assert n == count and np.array_equal(got, want)
    assert got.tobytes() == run_split(m, 16)[0].tobytes()


# ------------------------------------------------------------------------------------------------ refusals: none launches anything
def test_refusals():
    from segmentation_training_pipeline_amd import _lib, ops
    h, w = 37, 53
    lib = _lib.load()
    img = dev(INPUTS["ones_37x53"])
    d2 = torch.full((h * w,), POISON, dtype=torch.int32, device="cuda")
    labels = torch.full((h * w,), POISON, dtype=torch.int32, device="cuda")
    seeds = torch.ones((h * w,), dtype=torch.int32, device="cuda")
    out = torch.full((h * w,), 7, dtype=torch.uint8, device="cuda")
    words = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
    sizes = {"edt": ops.mask_edt_workspace_bytes(h, w), "grow": ops.label_grow_workspace_bytes(h, w)}
    assert sizes == {"edt": lib.stp_mask_edt_workspace_bytes(h, w), "grow": lib.stp_label_grow_workspace_bytes(h, w)}
    big = max(sizes.values())
    ws = workspace(big)
    p = lambda t: t.data_ptr()                                              # noqa: E731
    nc, nr, total = (words[k:k + 1] for k in range(3))
    for hh, ww in ((0, w), (h, 0), (-1, w), (32768, 1), (1, 32768)):        # sizes below 1 and above the bound
        assert lib.stp_mask_edt(p(img), hh, ww, p(d2), p(ws), big, None) == BADARG
        assert lib.stp_edt_threshold(p(seeds), hh, ww, 4, p(out), None) == BADARG
        assert lib.stp_label_grow(p(img), p(seeds), hh, ww, p(labels), p(total), p(ws), big, None) == BADARG
        assert lib.stp_label_unclaimed(p(img), p(seeds), hh, ww, p(out), None) == BADARG
        assert lib.stp_label_merge(p(seeds), p(nc), p(nr), hh, ww, p(labels), p(total), None) == BADARG
        assert ops.mask_edt_workspace_bytes(hh, ww) == 0 and ops.label_grow_workspace_bytes(hh, ww) == 0
    assert lib.stp_edt_threshold(p(seeds), h, w, -1, p(out), None) == BADARG                                # c2 < 0
    assert lib.stp_mask_edt(None, h, w, p(d2), p(ws), big, None) == BADARG                                   # NULL pointers
    assert lib.stp_mask_edt(p(img), h, w, None, p(ws), big, None) == BADARG
    assert lib.stp_mask_edt(p(img), h, w, p(d2), None, big, None) == BADARG
    assert lib.stp_edt_threshold(None, h, w, 4, p(out), None) == BADARG
    assert lib.stp_label_grow(p(img), None, h, w, p(labels), p(total), p(ws), big, None) == BADARG
    assert lib.stp_label_grow(p(img), p(seeds), h, w, p(labels), None, p(ws), big, None) == BADARG
    assert lib.stp_label_unclaimed(p(img), p(seeds), h, w, None, None) == BADARG
    assert lib.stp_label_merge(p(seeds), None, p(nr), h, w, p(labels), p(total), None) == BADARG
    assert lib.stp_label_merge(p(seeds), p(nc), p(nr), h, w, p(labels), p(nc), None) == BADARG               # total is nc
    assert lib.stp_label_merge(p(labels), p(nc), p(nr), h, w, p(labels), p(total), None) == BADARG           # rest is labels
    assert lib.stp_mask_edt(p(img), h, w, p(d2), p(ws), sizes["edt"] - 1, None) == WORKSPACE
    assert lib.stp_label_grow(p(img), p(seeds), h, w, p(labels), p(total), p(ws), sizes["grow"] - 1, None) == WORKSPACE
    with pytest.raises(_lib.StpError, match="BADARG"):
        ops.edt_threshold(seeds, h, w, -3, out)
    with pytest.raises(_lib.StpError, match="WORKSPACE"):
        ops.mask_edt(img, h, w, d2, ws[:sizes["edt"] - 8])
    torch.cuda.synchronize()
    assert (d2.cpu().numpy() == POISON).all() and (labels.cpu().numpy() == POISON).all()                     # nothing was launched
    assert (out.cpu().numpy() == 7).all() and (words.cpu().numpy() == POISON).all()
