"""Timing of dihedral test-time augmentation (helper, not collected): ``python tests/_dihedral_time.py [DIR]`` (without DIR: the
kernels only).

  * The two entry points of csrc/dihedral.hip alone, ops 3..7, next to stp_flip_u8 / stp_predict_accumulate with ``flip=1`` of the same
    build on the same shapes - launches that move exactly the same bytes: 8 x 512 x 512 x 3 bytes, 8 x 512 x 512 x {1, 20} floats.  Each
    figure is the mean of 10 repetitions (and their least and largest) after a warm-up; a repetition is 20 launches between two device
    events.
  * ``predict_on_batch_device`` of U-Net/resnet18, bf16, 512 x 512, batch 8 (built under DIR) with ``ttflips`` False, True and "d4", and
    the numpy "d4" statement around the same model's ``predict``: the mean (and the least) of 10 calls after one untimed call; the two
    "d4" results are asserted to be the same bits.  """
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("STP_ALLOW_RANDOM_ENCODER", "1")

SIZE, BATCH, LAUNCHES, RUNS = 512, 8, 20, 10


def kernels():
    import torch
    from segmentation_training_pipeline_amd import ops

    def measure(fn):
        """(mean, least, largest) microseconds per launch over RUNS repetitions of LAUNCHES launches."""
        for _ in range(LAUNCHES):
            fn()
        us = []
        for _ in range(RUNS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(LAUNCHES):
                fn()
            b.record()
            torch.cuda.synchronize()
            us.append(a.elapsed_time(b) * 1000 / LAUNCHES)
        return sum(us) / RUNS, min(us), max(us)

    def report(name, fn, nbytes):
        mean, lo, hi = measure(fn)
        print("%-48s %8.1f us per launch (%.1f .. %.1f)   %7.1f GB/s" % (name, mean, lo, hi, nbytes / mean / 1e3), flush=True)

    x = torch.randint(0, 256, (BATCH, SIZE, SIZE, 3), dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    report("stp_flip_u8 flip 1, 8x512x512x3", lambda: ops.flip_u8(x, y, BATCH, SIZE, SIZE, 3, 1), 2 * x.numel())
    for op in (3, 4, 5, 6, 7):
        report("stp_dihedral_u8 op %d, 8x512x512x3" % op, lambda: ops.dihedral_u8(x, y, BATCH, SIZE, SIZE, 3, op), 2 * x.numel())
    for c in (1, 20):
        p = torch.rand((BATCH, SIZE, SIZE, c), dtype=torch.float32, device="cuda")
        acc = torch.zeros_like(p)
        report("stp_predict_accumulate flip 1, 8x512x512x%d" % c, lambda: ops.predict_accumulate(p, acc, BATCH, SIZE, SIZE, c, 1),
               12 * p.numel())
        for op in (3, 4, 5, 6, 7):
            report("stp_predict_accumulate_dihedral op %d, 8x512x512x%d" % (op, c),
                   lambda: ops.predict_accumulate_dihedral(p, acc, BATCH, SIZE, SIZE, c, op), 12 * p.numel())


def end_to_end(out_dir):
    import torch
    import yaml
    import _dihedral_reference as D
    from segmentation_pipeline import segmentation
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
    xs = np.random.RandomState(0).randint(0, 256, size=(BATCH, SIZE, SIZE, 3)).astype(np.uint8)
    xd = torch.from_numpy(xs).to("cuda")

    def timed(fn):
        fn()                                                    # untimed: code objects, allocator
        ts = []
        for _ in range(RUNS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return sum(ts) / RUNS, min(ts), out

    base = None
    for ttflips in (False, True, "d4"):
        mean, least, (acc, k) = timed(lambda: cfg.predict_on_batch_device([model], ttflips, xd, BATCH))
        base = base or mean
        print("predict_on_batch_device ttflips %-5r: k %d   %8.2f ms (least %.2f)   %.2f x the plain pass" %
              (ttflips, k, mean * 1e3, least * 1e3, mean / base), flush=True)
    dev = acc.cpu().numpy() / k
    mean, least, host = timed(lambda: D.batch_sum([model], xs))
    assert np.array_equal(dev, host[0] / host[1]), "the device path differs from the host statement"
    print("numpy 'd4' statement around model.predict : k %d   %8.2f ms (least %.2f)" % (host[1], mean * 1e3, least * 1e3), flush=True)


if __name__ == "__main__":
    kernels()
    if len(sys.argv) > 1:
        end_to_end(sys.argv[1])
