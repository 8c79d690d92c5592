"""Timing of the mask path (helper, not collected): ``python tests/_mask_time.py DIR`` builds, per image size (768 x 768 and 101 x 101), a
one-class U-Net/resnet34 (bf16, batch 16, network shape 256 x 256 / 128 x 128) under DIR with a checkpoint from a fixed seed and 64
synthetic images with masks, and times on this machine, in this run, after one untimed pass each:

  * ``predict_masks`` (threshold = the 0.7 quantile of the maps, opening 2) next to the host chain it replaces: ``predict_in_directory`` with a
    callback doing numpy's ``>``, scipy's ``binary_opening(disk(2))`` and ``rle_encode`` - and both chains alone, on maps that are
    already there (host: numpy maps; device: device maps, including the copy of the runs);
  * ``find_threshold`` with 19 thresholds next to the ``evaluateAll`` loop that thresholds every map 19 times and scores it;
  * every new kernel on one map: its time, the bytes it moves, the time of a device copy of as many bytes, and those bytes at the
    copy rate of bench.py's box_calibration on this box - a kernel far off that floor shows here.

The host chain is the baseline, never the code under test; the strings and tables of both sides are compared before a time is printed."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("STP_ALLOW_RANDOM_ENCODER", "1")

IMAGES, BATCH = 64, 16
CASES = ((768, 256), (101, 128))          # (image size, network shape)


def setup(out_dir, size, net):
    import yaml
    from PIL import Image
    from segmentation_pipeline import segmentation
    from segmentation_pipeline.impl.datasets import SimplePNGMaskDataSet
    root = os.path.join(out_dir, "s%d" % size)
    os.makedirs(root, exist_ok=True)
    cfg_path = os.path.join(root, "config.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"architecture": "Unet", "backbone": "resnet34", "classes": 1, "activation": "sigmoid", "encoder_weights": None,
                        "shape": [net, net, 3], "batch": BATCH, "dtype": "bf16", "loss": "binary_crossentropy", "folds_count": 2,
                        "stages": [{"epochs": 1}]}, f)
    cfg = segmentation.parse(cfg_path)
    model = cfg.createNet1(True)
    model.compile(loss="binary_crossentropy", batch=BATCH, dtype="bf16")
    model.impl.init_weights(11)
    w = model.impl.get_weights()          # (keeps the logits of a deep random net small: the maps take both sides of a threshold)
    model.impl.set_weights({k: np.full_like(v, 0.7) for k, v in w.items() if k.endswith("/gamma")})
    model.save_weights(cfg.weightsPath(0, 0))
    del model
    img_dir, msk_dir = os.path.join(root, "images"), os.path.join(root, "masks")
    os.makedirs(img_dir, exist_ok=True); os.makedirs(msk_dir, exist_ok=True)
    rng = np.random.RandomState(0)
    yy, xx = np.mgrid[0:size, 0:size]
    for i in range(IMAGES):
        m = ((yy - size * rng.uniform(0.3, 0.7)) / (size * 0.3)) ** 2 + ((xx - size * rng.uniform(0.3, 0.7)) / (size * 0.2)) ** 2 <= 1
        img = rng.randint(0, 80, size=(size, size, 3)).astype(np.uint8)
        img[m] += 150                                        # a bright ellipse on dark noise: the map has structure
        Image.fromarray(img).save(os.path.join(img_dir, "im%03d.png" % i))
        Image.fromarray((m * 255).astype(np.uint8)).save(os.path.join(msk_dir, "im%03d.png" % i))
    loaded, load_model = {}, cfg.load_model

    def load_once(fold=0, stage=-1):                         # both sides run with the model already loaded
        key = (fold, 0 if stage < 0 else stage)
        if key not in loaded:
            loaded[key] = load_model(*key)
        return loaded[key]
    cfg.load_model = load_once
    return cfg, img_dir, SimplePNGMaskDataSet(img_dir, msk_dir)


def timed(fn):
    import torch
    fn()                                                     # untimed: code objects, allocator, file cache
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_times(size):
    """One 768 x 768 (or 101 x 101) one-class map: each kernel's median time over 50 launches next to a device copy of its bytes."""
    import torch
    from scipy import ndimage
    from segmentation_training_pipeline_amd import ops
    h = w = size
    f = ndimage.gaussian_filter(np.random.default_rng(size).random((h, w)), 4.0)
    probs = torch.from_numpy(((f - f.min()) / (f.max() - f.min())).astype(np.float32)[:, :, None].copy()).to("cuda")
    a = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    target = (probs[:, :, 0] > 0.55).to(torch.uint8)
    runs = torch.empty(((h * w + 1) // 2, 2), dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.mask_rle_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    thr = [d / 20 for d in range(1, 20)]
    counts = torch.empty((19, 2), dtype=torch.int64, device="cuda")
    totals = torch.empty(2, dtype=torch.int64, device="cuda")
    tws = torch.empty(ops.threshold_counts_workspace_bytes(19), dtype=torch.uint8, device="cuda")
    ops.mask_threshold(probs, h, w, 1, 0, 0, 0.5, a)
    ops.mask_rle(a, h, w, runs, count, ws)
    n_runs = int(count.item())
    px = h * w
    words = ops.mask_rle_workspace_bytes(h, w)
    kernels = [
        ("stp_mask_threshold", lambda: ops.mask_threshold(probs, h, w, 1, 0, 0, 0.5, a), 4 * px + px),
        ("stp_mask_morph erode r=2", lambda: ops.mask_morph(a, b, h, w, 2, 0), 2 * px),
        ("stp_mask_morph dilate r=7", lambda: ops.mask_morph(a, b, h, w, 7, 1), 2 * px),
        ("stp_mask_rle (4 launches, %d runs)" % n_runs, lambda: ops.mask_rle(a, h, w, runs, count, ws), px + 3 * words + 8 * n_runs),
        ("stp_threshold_counts T=19 (2 launches)", lambda: ops.threshold_counts(probs, target, h, w, 1, 0, thr, counts, totals, tws), 5 * px),
    ]
    src = torch.zeros(16 * px, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream()

    def median_us(fn, reps=50):
        fn(); torch.cuda.synchronize()
        evs = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st); fn(); e1.record(st)
            evs.append((e0, e1))
        torch.cuda.synchronize()
        return sorted(e0.elapsed_time(e1) for e0, e1 in evs)[reps // 2] * 1e3
    for name, fn, nbytes in kernels:
        half = -(-nbytes // 32) * 16                          # a copy that moves nbytes: reads half, writes half
        copy_us = median_us(lambda: dst[:half].copy_(src[:half]))
        print("  %-44s %8.1f us   %9d bytes   a device copy of as many bytes %6.1f us, at the box's copy rate %6.2f us" %
              (name, median_us(fn), nbytes, copy_us, nbytes / COPY_GBS[0] * 1e-3), flush=True)


COPY_GBS = []          # bench.py's box_calibration: read + write bytes per second of a 1 GiB device copy on this box


def main(out_dir):
    import torch
    from scipy.ndimage import binary_opening
    import _mask_reference as R
    from segmentation_pipeline.impl.rle import rle_encode
    from bench import box_calibration
    COPY_GBS.append(box_calibration("cuda", seconds=0.2)["copy_gbs"])
    print("box_calibration: copy %.1f GB/s" % COPY_GBS[0])
    for size, net in CASES:
        cfg, img_dir, ds = setup(out_dir, size, net)
        maps = {}
        cfg.predict_in_directory(img_dir, 0, 0, lambda name, mp, data: data.__setitem__(name, mp.arr), maps)
        thr = float(np.quantile(np.concatenate([m.reshape(-1)[::17] for m in maps.values()]), 0.7))
        disk2 = R.disk(2)

        def host_chain():
            codes = {}
            cfg.predict_in_directory(img_dir, 0, 0, lambda name, mp, data: data.__setitem__(
                name, rle_encode(binary_opening(mp.arr[:, :, 0] > thr, disk2))), codes)
            return codes

        def device_chain():
            return dict(cfg.predict_masks(img_dir, fold=0, stage=0, threshold=thr, opening=2))
        th, want = timed(host_chain)
        td, got = timed(device_chain)
        assert got == want, "predict_masks differs from the host chain"
        print("%d x %d, %d images, %d runs in all" % (size, size, IMAGES, sum(len(c.split()) // 2 for c in want.values())))
        print("  host chain (predict_in_directory + numpy + scipy + rle_encode): %.3f s;  predict_masks: %.3f s" % (th, td))
        dev_maps = {k: torch.from_numpy(v).to("cuda") for k, v in maps.items()}
        th, _ = timed(lambda: {k: rle_encode(binary_opening(v[:, :, 0] > thr, disk2)) for k, v in maps.items()})
        td, alone = timed(lambda: {k: cfg._device_rle(cfg._device_mask(v, 0, thr, 2, 0, 0)) for k, v in dev_maps.items()})
        assert alone == want
        print("  the chains alone, maps already there: host %.3f s;  device (kernels + copy of the runs + formatting) %.3f s" % (th, td))
        sweep = [d / 20 for d in range(1, 20)]

        def host_sweep():
            per_image = []
            for b in cfg.evaluateAll(ds, 0):
                per_image += [R.threshold_counts(p.arr, g.arr[:, :, 0], sweep) for p, g in zip(b.predicted_maps_aug, b.segmentation_maps)]
            return R.sweep_table(per_image, "dice", "image").tolist()
        th, want_table = timed(host_sweep)
        td, (best, table) = timed(lambda: cfg.find_threshold(ds, 0, metric="dice"))
        assert [table[t] for t in sweep] == want_table, "find_threshold differs from the evaluateAll loop"
        print("  evaluateAll + 19 numpy thresholds + scores: %.3f s;  find_threshold: %.3f s  (%d validation images)" %
              (th, td, len(cfg.kfold(ds, range(len(ds))).sampledIndexes(0, False, "real"))))
        kernel_times(size)


if __name__ == "__main__":
    main(sys.argv[1])
