"""stp_softmax_loss_ex next to stp_softmax_cce_dice at the softmax workloads' shapes (bf16: 16 x 512 x 512 x 3, 8 x 768 x 768 x 20):
us per call of the value pass (scalars only: value + finalize launches) and of the whole call (+ gradient pass), device events
around 200 calls, the two entry points alternating; and each pass's HBM floor (bytes the pass has to move / 6.3 TB/s).
``python scratch/softmax_ex_bench.py [iterations]``"""
import ctypes
import sys

import torch

from segmentation_training_pipeline_amd import _lib

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
    dl = torch.empty(pixels, dlc, device=dev, dtype=torch.bfloat16)
    floor_v = pixels * (C * 2 + 1) / HBM * 1e6
    floor_g = pixels * (C * 2 + 1 + dlc * 2) / HBM * 1e6
    print("pixels %d classes %d gradient rows %d: HBM floor value pass %.1f us, gradient pass %.1f us" % (pixels, C, dlc, floor_v, floor_g))

    def old(grad, w=(1.0, 1.0)):
        return lambda: lib.stp_softmax_cce_dice(z.data_ptr(), t.data_ptr(), pixels, C, C, _lib.BF16, w[0], w[1], sc.data_ptr(),
                                                dl.data_ptr() if grad else None, dlc, 1.0, ws.data_ptr(), ws.numel() * 4, st)

    def new(grad, w):
        w5 = (ctypes.c_float * 5)(*w)
        return lambda: lib.stp_softmax_loss_ex(z.data_ptr(), t.data_ptr(), pixels, C, C, _lib.BF16, w5, sc.data_ptr(),
                                               dl.data_ptr() if grad else None, dlc, 1.0, ws.data_ptr(), ws.numel() * 4, st)

    rows = [("stp_softmax_cce_dice  cce+dice", old), ("stp_softmax_loss_ex   cce+dice", lambda g: new(g, (1.0, 1.0, 0, 0, 0))),
            ("stp_softmax_loss_ex   all five", lambda g: new(g, (1.0, 0.5, 0.3, 0.2, 2.0))),
            ("stp_softmax_loss_ex   focal alone", lambda g: new(g, (0, 0, 0, 0, 1.0))),
            ("stp_softmax_loss_ex   cce+iou+jaccard", lambda g: new(g, (1.0, 0, 0.3, 0.2, 0)))]
    for rnd in range(2):              # two rounds, the entry points alternating: the spread shows next to the difference
        for name, mk in rows:
            v, full = timed(mk(False)), timed(mk(True))
            print("  round %d  %-40s value %.1f us  value + gradient %.1f us  (gradient %.1f us)" % (rnd, name, v, full, full - v))
