"""GPU tests of stp_surface_distances (csrc/boundary.hip) through ``ops.surface_distances`` against tests/_boundary_reference.py: the
whole ``out`` vector by ``np.array_equal``, twice per case with identical bytes, poisoned before each call, one guard element past its end."""
import numpy as np
import pytest
import torch

import _boundary_reference as R

pytestmark = pytest.mark.gpu

POISON = -5
C2 = [1, 4, 9]
PERCENTILES = [(95, 100), (0, 100), (100, 100), (1, 3)]


def dots(h, w, *points):
    m = np.zeros((h, w), bool)
    m[tuple(zip(*points))] = True
    return m


CASES = {}
for s in [(3, 5), (37, 53), (64, 64), (70, 133), (129, 67), (65, 257), (768, 768)]:
    CASES["field_%dx%d" % s] = (R.field(*s) > 0.5, R.field(*s) > 0.6)
f = R.field(37, 53)
CASES["full"] = (np.ones((37, 53), bool), f > 0.5)                       # the surface of a full mask is the image frame
CASES["one_empty"], CASES["both_empty"], CASES["identical"] = (f > 0.5, f > 2), (f > 2, f > 2), (f > 0.5, f > 0.5)
CASES["single_pixel"] = (dots(9, 9, (4, 4)), dots(9, 9, (4, 6)))
CASES["1x1"] = (np.ones((1, 1), bool), np.ones((1, 1), bool))
line = np.arange(130) % 7 < 4                                          # runs of 4: surfaces on both sides of lanes 63 | 64
CASES["1x130"], CASES["130x1"] = (line[None], np.roll(line, 3)[None]), (line[:, None], np.roll(line, 3)[:, None])
bar = np.zeros((6, 130), bool)
bar[:, 61:68] = True                                                   # rows 0 and h - 1: surface across x = 63 / 64 / 65; inside: none
CASES["segment_edge"] = (bar, np.roll(bar, 1, axis=1))
CASES["far_1x2000"] = (dots(1, 2000, (0, 0)), dots(1, 2000, (0, 1999)))  # D2 = 1999^2 > 2^21: the top digit is live; n = 2
CASES["far_64x64"] = (dots(64, 64, (5, 5)), dots(64, 64, (5, 55)))       # D2 = 2500 > 2^11
CASES["three"] = (dots(3, 70, (1, 0), (1, 69)), dots(3, 70, (1, 3)))     # n = 3: D2 = 9, 9, 4356 - the ranks part in the second digit


def run(pred, truth, c2, num, den):
    from segmentation_training_pipeline_amd import ops
    h, w = pred.shape
    n = 2 * (3 + len(c2)) + 3
    out = torch.full((n + 1,), POISON, dtype=torch.int64, device="cuda")
    ws = torch.empty(ops.surface_distances_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    p, g = (torch.from_numpy(np.ascontiguousarray(m).astype(np.uint8) * 255).to("cuda") for m in (pred, truth))
    ops.surface_distances(p, g, h, w, c2, num, den, out[:n], ws)
    got = out.cpu().numpy()
    assert got[-1] == POISON
    return got[:-1]


def test_reference_side_properties():
    want = {k: R.counters(p, g, C2, 95, 100) for k, (p, g) in CASES.items() if k != "field_768x768"}
    for k in ("field_37x53", "field_64x64", "field_70x133", "field_129x67", "field_65x257"):
        d0, d1, n0, n1 = R.squared_distances(*CASES[k])
        assert min(n0, n1) >= 300 and len(np.unique(np.concatenate([d0, d1]))) >= 30, k
    assert want["full"][0] == 2 * (37 + 53) - 4 and want["identical"][[1, 7, 12, 13]].tolist() == [0, 0, 0, 0]
    assert want["one_empty"][[0, 1, 6, 7]].tolist()[1::2] == [-1, -1] and want["one_empty"][0] > 0 and want["one_empty"][6] == 0
    assert want["both_empty"].tolist() == [0, -1, 0, 0, 0, 0] * 2 + [-1, -1, 0]
    assert want["1x1"].tolist() == [1, 0, 0, 1, 1, 1] * 2 + [0, 0, 95] and want["single_pixel"][[0, 1, 6]].tolist() == [1, 4, 1]
    assert want["segment_edge"][0] == 2 * 7 + 2 * 4 and want["1x130"][0] == want["130x1"][0] == int(np.sum(np.arange(130) % 7 < 4))
    assert want["far_1x2000"][12:].tolist() == [1999 ** 2, 1999 ** 2, 95] and 1999 ** 2 >> 20 > 0
    assert want["far_64x64"][12:14].tolist() == [2500, 2500] and 2500 >> 10 > 0
    assert want["three"][[0, 6, 12, 13]].tolist() == [2, 1, 9, 4356] and 9 >> 10 != 4356 >> 10


@pytest.mark.parametrize("name", sorted(CASES))
def test_counters_equal_the_reference(name):
    pred, truth = CASES[name]
    for num, den in PERCENTILES if name != "field_768x768" else PERCENTILES[:1]:
        want = R.counters(pred, truth, C2, num, den)
        first, second = run(pred, truth, C2, num, den), run(pred, truth, C2, num, den)
        assert np.array_equal(first, want), (name, num, den, first.tolist(), want.tolist())
        assert first.tobytes() == second.tobytes()
    assert np.array_equal(run(pred, truth, [], 95, 100), R.counters(pred, truth, [], 95, 100))      # T = 0


def test_refusals_launch_nothing():
    from segmentation_training_pipeline_amd import _lib, ops
    import ctypes as C
    h, w = 37, 53
    lib, nbytes = _lib.load(), ops.surface_distances_workspace_bytes(37, 53)
    m = torch.ones((h, w), dtype=torch.uint8, device="cuda")
    out = torch.full((15,), POISON, dtype=torch.int64, device="cuda")
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    p, c2 = (lambda t: t.data_ptr()), (C.c_int32 * 3)(*C2)
    call = lambda pred=p(m), c=c2, T=3, num=95, den=100, hh=h, o=p(out), wp=p(ws), nb=nbytes: lib.stp_surface_distances(  # noqa: E731
        pred, p(m), hh, w, c, T, num, den, o, wp, nb, None)
    assert call(pred=None) == call(o=None) == call(wp=None) == call(hh=0) == call(hh=32768) == -1
    assert call(T=17) == call(c=(C.c_int32 * 3)(4, 4, 9)) == call(c=(C.c_int32 * 3)(-1, 4, 9)) == call(c=None) == -1
    assert call(den=0) == call(den=1001) == call(num=101) == call(num=-1) == call(o=p(out) + 4) == -1
    assert call(nb=nbytes - 1) == call(wp=p(ws) + 4) == -3
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all()
