"""stp_class_confusion and stp_class_confusion_up at the softmax workloads' shapes (bf16: 16 x 512 x 512 x 3 with the logits at 1 / 4,
8 x 768 x 768 x 20 with the logits at 1 / 8): us per call, device events around 200 calls, two alternating rounds; each form on a
piecewise-constant mask that the logits mostly agree with (a wave shares one key) and on uniformly random targets and logits (the
wave-aggregation worst case); next to the full-resolution form's HBM floor (rows + targets / 6.3 TB/s).
``python scratch/class_confusion_bench.py [iterations]``"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segmentation_training_pipeline_amd import _lib  # noqa: E402

IT = int(sys.argv[1]) if len(sys.argv) > 1 else 200
HBM = 6.3e12                      # achievable HBM bandwidth (MI355X_MICROARCH.md), bytes / s
lib = _lib.load("bf16")
dev = "cuda"
st = torch.cuda.current_stream().cuda_stream


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


for N, S, C, f in ((16, 512, 3, 4), (8, 768, 20, 8)):
    pixels, s = N * S * S, S // f
    ws = torch.empty(int(lib.stp_class_confusion_workspace_bytes(C)) // 4, dtype=torch.int32, device=dev)
    cnt = torch.zeros(C * C, dtype=torch.int32, device=dev)
    print("%d x %d x %d x %d bf16, low-resolution logits at 1 / %d: HBM floor of the full-resolution form %.1f us"
          % (N, S, S, C, f, pixels * (C * 2 + 1) / HBM * 1e6))
    cases = {}
    for mask in ("piecewise", "random"):
        if mask == "piecewise":       # 32 x 32 blocks of one class; the logits favour the target's class
            t_lo = torch.randint(0, C, (N, S // 32, S // 32), device=dev)
            t = t_lo.repeat_interleave(32, 1).repeat_interleave(32, 2)
            agree = 8.0
        else:
            t = torch.randint(0, C, (N, S, S), device=dev)
            agree = 0.0
        onehot = torch.nn.functional.one_hot(t, C).to(torch.float32)
        full = (torch.randn(N, S, S, C, device=dev) * 2 + agree * onehot).to(torch.bfloat16).contiguous()
        low = (torch.randn(N, s, s, C, device=dev) * 2 + agree * onehot[:, ::f, ::f]).to(torch.bfloat16).contiguous()
        t8 = t.to(torch.uint8).contiguous()
        cases[mask] = (full, low, t8)

    def full_form(mask):
        full, _low, t8 = cases[mask]
        return lambda: lib.stp_class_confusion(full.data_ptr(), t8.data_ptr(), pixels, C, C, _lib.BF16, cnt.data_ptr(), ws.data_ptr(), ws.numel() * 4, st)

    def up_form(mask):
        _full, low, t8 = cases[mask]
        return lambda: lib.stp_class_confusion_up(low.data_ptr(), t8.data_ptr(), N, s, s, f, C, C, _lib.BF16, cnt.data_ptr(), ws.data_ptr(), ws.numel() * 4, st)

    for rnd in range(2):              # two rounds, the forms alternating: the spread shows next to the difference
        for mask in ("piecewise", "random"):
            for name, mk in (("stp_class_confusion", full_form), ("stp_class_confusion_up", up_form)):
                us = timed(mk(mask))
                torch.cuda.synchronize()
                assert int(cnt.sum().item()) == pixels
                print("  round %d  %-24s %-10s mask  %.1f us" % (rnd, name, mask, us))
