"""stp_softmax_loss_masked next to the unchanged stp_softmax_loss_ex at the softmax workloads' shapes (bf16: 16 x 512 x 512 x 3,
8 x 768 x 768 x 20), the method of scratch/softmax_ex_bench.py: us per call of the value pass (scalars only: value + finalize launches)
and of the whole call (+ gradient pass), device events around 200 calls, two rounds with the entry points alternating; with no pixel
ignored and with 30 % ignored (the masked kernel still reads every row and stores every gradient row - equal work); and each pass's
HBM floor.  ``python scratch/softmax_masked_bench.py [iterations]``"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the repository root: run from anywhere
from segmentation_training_pipeline_amd import _lib  # noqa: E402

IT = int(sys.argv[1]) if len(sys.argv) > 1 else 200
HBM = 6.3e12                      # achievable HBM bandwidth (MI355X_MICROARCH.md), bytes / s
lib = _lib.load("bf16")
dev = "cuda"
st = torch.cuda.current_stream().cuda_stream
ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device=dev)
sc = torch.zeros(16, dtype=torch.float32, device=dev)


def timed(fn):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(IT):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / IT * 1e3


for pixels, C, dlc in ((16 * 512 * 512, 3, 8), (8 * 768 * 768, 20, 24)):
    z = (torch.randn(pixels, C, device=dev) * 2).to(torch.bfloat16)
    t = torch.randint(0, C, (pixels,), device=dev, dtype=torch.uint8)
    t30 = torch.where(torch.rand(pixels, device=dev) < 0.3, torch.full_like(t, 255), t)
    cw = torch.linspace(0.25, 4.0, C, device=dev, dtype=torch.float32)
    dl = torch.empty(pixels, dlc, device=dev, dtype=torch.bfloat16)
    floor_v = pixels * (C * 2 + 1) / HBM * 1e6
    floor_g = pixels * (C * 2 + 1 + dlc * 2) / HBM * 1e6
    print("pixels %d classes %d gradient rows %d: HBM floor value pass %.1f us, gradient pass %.1f us" % (pixels, C, dlc, floor_v, floor_g))

    def ex(grad, w, tt=t):
        w5 = (ctypes.c_float * 5)(*w)
        return lambda: lib.stp_softmax_loss_ex(z.data_ptr(), tt.data_ptr(), pixels, C, C, _lib.BF16, w5, sc.data_ptr(),
                                               dl.data_ptr() if grad else None, dlc, 1.0, ws.data_ptr(), ws.numel() * 4, st)

    def masked(grad, w, tt, ign, weights):
        w5 = (ctypes.c_float * 5)(*w)
        return lambda: lib.stp_softmax_loss_masked(z.data_ptr(), tt.data_ptr(), pixels, C, C, _lib.BF16, w5, sc.data_ptr(),
                                                   dl.data_ptr() if grad else None, dlc, 1.0, ws.data_ptr(), ws.numel() * 4, ign,
                                                   weights.data_ptr() if weights is not None else None, st)

    rows = []
    for mix, w in (("cce+dice", (1.0, 1.0, 0, 0, 0)), ("all five", (1.0, 0.5, 0.3, 0.2, 2.0))):
        rows += [("stp_softmax_loss_ex      %s" % mix, lambda g, w=w: ex(g, w)),
                 ("stp_softmax_loss_masked  %s, none ignored, weights" % mix, lambda g, w=w: masked(g, w, t, 255, cw)),
                 ("stp_softmax_loss_masked  %s, 30%% ignored, weights" % mix, lambda g, w=w: masked(g, w, t30, 255, cw)),
                 ("stp_softmax_loss_masked  %s, 30%% ignored, no weights" % mix, lambda g, w=w: masked(g, w, t30, 255, None))]
    for rnd in range(2):              # two rounds, the entry points alternating: the spread shows next to the difference
        for name, mk in rows:
            v, full = timed(mk(False)), timed(mk(True))
            print("  round %d  %-58s value %.1f us  value + gradient %.1f us  (gradient %.1f us)" % (rnd, name, v, full, full - v), flush=True)
