"""Timing of lovasz_softmax (helper, not collected): ``python tests/_lovasz_softmax_time.py [kernels|steps] ...``.

  * ``kernels``: the launch group of stp_lovasz_softmax alone (key pass, sort, both scan launches, finalize, gradient pass) behind one
    stp_softmax_loss_ex, bf16, at 16 x 512 x 512 with 3 classes and at 8 x 768 x 768 with 20 classes: the mean of 10 calls (and their least
    and largest) between two device events after a warm-up, then the kernels of one call by name from the profiler's kernel records - the
    share of the group the sort takes is the time of every kernel that is not one of csrc/lovasz_softmax.hip's (``lvs_``).
  * ``steps``: the whole training step of U-Net/resnet18, bf16, hipGraph replay, on the same two boxes with
    ``categorical_crossentropy+0.5*lovasz_softmax`` and with ``categorical_crossentropy`` alone: the mean of 10 steps after a warm-up.
    """
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("STP_ALLOW_RANDOM_ENCODER", "1")

BOXES = [(16, 512, 3), (8, 768, 20)]
RUNS = 10


def kernels():
    import torch
    from segmentation_training_pipeline_amd import _lib
    lib = _lib.load("bf16")
    for n, size, classes in BOXES:
        pixels = n * size * size
        ldc = (classes + 7) // 8 * 8
        g = torch.Generator(device="cuda").manual_seed(classes)
        z = (torch.randn((pixels, ldc), device="cuda", generator=g) * 2).to(torch.bfloat16)
        t = torch.randint(0, classes, (pixels,), device="cuda", generator=g).to(torch.uint8)
        sc = torch.zeros(16, dtype=torch.float32, device="cuda")
        dl = torch.zeros((pixels, ldc), dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(int(lib.stp_loss_workspace_bytes()) // 4, dtype=torch.float32, device="cuda")
        need = int(lib.stp_lovasz_softmax_workspace_bytes(pixels, classes))
        wl = torch.empty(need, dtype=torch.uint8, device="cuda")
        w5 = (ctypes.c_float * 5)(1.0, 0, 0, 0, 0)
        st = torch.cuda.current_stream().cuda_stream

        def first():
            _lib.check(lib.stp_softmax_loss_ex(z.data_ptr(), t.data_ptr(), pixels, classes, ldc, _lib.BF16, w5, sc.data_ptr(), dl.data_ptr(), ldc,
                                               1.0, ws.data_ptr(), ws.numel() * 4, st), "stp_softmax_loss_ex")

        def group():
            _lib.check(lib.stp_lovasz_softmax(z.data_ptr(), t.data_ptr(), pixels, classes, ldc, _lib.BF16, 0.5, sc.data_ptr(), dl.data_ptr(), ldc,
                                              1.0, -1, wl.data_ptr(), need, st), "stp_lovasz_softmax")

        def timed(fn):
            for _ in range(2):
                fn()
            ms = []
            for _ in range(RUNS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            return sum(ms) / RUNS, min(ms), max(ms)

        print("box %d x %d x %d, %d classes, bf16: workspace %.1f MB (%.1f bytes per pixel and class)" %
              (n, size, size, classes, need / 1e6, need / float(pixels * classes)), flush=True)
        print("  stp_softmax_loss_ex        %9.3f ms (%.3f .. %.3f)" % timed(first), flush=True)
        mean, lo, hi = timed(group)
        print("  stp_lovasz_softmax group   %9.3f ms (%.3f .. %.3f)   lovasz_softmax = %.6f" % (mean, lo, hi, float(sc[14])), flush=True)
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                group()
                torch.cuda.synchronize()
            rows = {}
            for ev in prof.events():
                if ev.device_type is not None and "cuda" in str(ev.device_type).lower():
                    rows[ev.name] = rows.get(ev.name, 0.0) + float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
            total = sum(rows.values())
            ours = sum(v for k, v in rows.items() if "lvs_" in k)
            for k, v in sorted(rows.items(), key=lambda kv: -kv[1]):
                print("    %10.1f us  %s" % (v, k[:110]), flush=True)
            if total > 0:
                print("  kernels of one call: %.1f us, of which the sort (every kernel but lvs_*) %.1f us = %.0f %%" %
                      (total, total - ours, 100.0 * (total - ours) / total), flush=True)
        except Exception as e:          # (a build of torch without the kernel records: the group time above stands alone)
            print("  no kernel records: %s: %s" % (type(e).__name__, e), flush=True)
        del z, t, dl, wl


def steps():
    import torch
    from segmentation_training_pipeline_amd.backend import HipSegModel
    for n, size, classes in BOXES:
        rng = np.random.RandomState(classes)
        x = rng.randint(0, 256, (n, size, size, 3)).astype(np.uint8)
        y = rng.randint(0, classes, (n, size, size, 1)).astype(np.uint8)
        for spec in ("categorical_crossentropy", "categorical_crossentropy+0.5*lovasz_softmax"):
            m = HipSegModel("Unet", "resnet18", (size, size, 3), classes, "softmax", batch=n, dtype="bf16", loss=spec, optimizer="Adam", lr=1e-3,
                            use_graph=True)
            m.load_batch(x, y)
            for _ in range(3):
                m.train_on_batch(None, None, fetch=False)
            ms = []
            for _ in range(RUNS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.train_on_batch(None, None, fetch=False)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            print("step U-Net/resnet18 bf16 %d x %d x %d, %d classes, %-45s %9.3f ms (%.3f .. %.3f)   loss %.5f" %
                  (n, size, size, classes, spec, sum(ms) / RUNS, min(ms), max(ms), m.metrics()["loss"]), flush=True)
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "steps"]
    if "kernels" in what:
        kernels()
    if "steps" in what:
        steps()
