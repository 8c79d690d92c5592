"""Timing of sliding-window prediction (helper, not collected): ``python tests/_window_time.py DIR`` builds U-Net/resnet18 at 512 x 512,
bf16, batch 8 under DIR, saves one checkpoint and times, for one 2048 x 2048 image (25 windows at overlap 64) and one 1024 x 1024 image
(9 windows), with and without flip test-time augmentation:

  * the device path, ``cfg.windows = 64`` and ``_predict_windows`` (image up once, gather / predict / accumulate per batch, one finish,
    the map back once);
  * the host statement of tests/_window_reference.py around the same model's ``predict`` - what a user of the pipeline would write
    today: numpy windows, one ``predict`` per batch and flip, numpy cross-fade;

each as the mean (and the least) of 10 calls after one untimed call, and asserts that both give the same bits.  Then the three new
launches alone on the 2048 x 2048 shapes, by device events over 50 launches each: stp_window_gather_u8 and stp_window_accumulate of
one batch of 8 windows, stp_window_finish of the whole map."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("STP_ALLOW_RANDOM_ENCODER", "1")

SIZE, BATCH, OVERLAP, REPS, RUNS = 512, 8, 64, 50, 10


def main(out_dir):
    import torch
    import yaml
    import _window_reference as R
    from segmentation_pipeline import segmentation
    from segmentation_training_pipeline_amd import ops
    os.makedirs(out_dir, exist_ok=True)
    cfg_path = os.path.join(out_dir, "config.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"architecture": "Unet", "backbone": "resnet18", "classes": 1, "activation": "sigmoid", "encoder_weights": None,
                        "shape": [SIZE, SIZE, 3], "batch": BATCH, "dtype": "bf16", "loss": "binary_crossentropy", "folds_count": 2,
                        "stages": [{"epochs": 1}]}, f)
    cfg = segmentation.parse(cfg_path)
    net = cfg.createNet1(True)
    net.compile(loss="binary_crossentropy", batch=BATCH, dtype="bf16")
    net.impl.init_weights(11)
    net.save_weights(cfg.weightsPath(0, 0))
    del net
    model = cfg.load_model(0, 0)
    cfg.windows = OVERLAP
    rng = np.random.RandomState(0)

    def timed(fn):
        """(mean seconds, least seconds, result) of RUNS calls, each ended by a device synchronise, after one untimed call."""
        fn()                                                    # untimed: code objects, allocator
        ts = []
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sum(ts) / RUNS, min(ts), out

    for side in (2048, 1024):
        img = rng.randint(0, 256, size=(side, side, 3)).astype(np.uint8)
        n = len(R.raster(side, side, SIZE, SIZE, OVERLAP))
        for ttflips in (False, True):
            td, td0, dev = timed(lambda: cfg._predict_windows([model], ttflips, img))
            th, th0, host = timed(lambda: R.predict_windows([model], ttflips, img, SIZE, SIZE, 3, OVERLAP, BATCH))
            assert np.array_equal(dev, host), "the device path differs from the host statement"
            print("%d x %d, %d windows, ttflips %-5s: device path %.2f ms (least %.2f)   host statement %.2f ms (least %.2f)   ratio %.1f" %
                  (side, side, n, ttflips, td * 1e3, td0 * 1e3, th * 1e3, th0 * 1e3, th / td), flush=True)

    # the three launches alone, 2048 x 2048: one batch of 8 windows (a row of the raster and the start of the next), the whole map
    h = w = 2048
    org = R.raster(h, w, SIZE, SIZE, OVERLAP)[:BATCH]
    src = torch.from_numpy(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).to("cuda")
    xs = torch.empty((BATCH, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda")
    acc = torch.rand((BATCH, SIZE, SIZE, 1), dtype=torch.float32, device="cuda")
    canvas = torch.zeros((h, w, 1), dtype=torch.float32, device="cuda")
    sy = torch.from_numpy(R.sums(h, SIZE, OVERLAP).astype(np.float32)).to("cuda")
    out = torch.empty((h, w, 1), dtype=torch.float32, device="cuda")
    launches = (("stp_window_gather_u8, 8 windows", lambda: ops.window_gather_u8(src, h, w, 3, org, xs, SIZE, SIZE), 2 * xs.numel()),
                ("stp_window_accumulate, 8 windows", lambda: ops.window_accumulate(acc, SIZE, SIZE, 1, org, OVERLAP, canvas, h, w),
                 4 * acc.numel() + 8 * (org[-1][0] + SIZE) * w),
                ("stp_window_finish, mode 0", lambda: ops.window_finish(canvas, h, w, 1, 3, sy, sy, 0, out), 8 * h * w))
    for name, fn, nbytes in launches:
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1000 / REPS
        print("%-34s %8.1f us per launch   %6.1f GB/s of the bytes it touches" % (name, us, nbytes / us / 1e3), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
