"""Timing of the per-object measurement path (helper, not collected): ``python tests/_measure_time.py DIR [--ops-only]`` times on this
machine, in this run, at 768 x 768 and 101 x 101:

  (a) stp_label_measure (2 launches) and stp_label_select (4 launches) per image, each the median of 50, on three kinds of label images
      under a random map: "salt" (the 4-connected components of salt and pepper: tens of thousands of objects, nearly every stretch
      misses the workgroup's LDS table), "few" (the 8-connected components of a smoothed field) and "one" (one object that fills the
      image: every stretch of every wave meets the same eight words);
  (b) the host chain they replace on the same image: the label image and the map copied back, ``np.bincount``,
      ``scipy.ndimage.find_objects``, ``center_of_mass`` and ``mean``; the areas, boxes and float64 columns of both sides are compared
      before a time is printed;
  (c) without ``--ops-only``, on the experiment of tests/_mask_time.py (a one-class U-Net/resnet34 with a checkpoint from a fixed seed and
      64 synthetic images per size): one ``find_confidence`` grid of 3 thresholds x 5 confidences next to one ``score_instances`` cell on
      the same validation items; one cell of the table is compared with ``score_instances_ex`` before a time is printed.

``STP_LIB`` names another build of the library (segmentation_training_pipeline_amd/_lib.py): the numbers of DESIGN.md 3.29 for the form
without the LDS table come from a build of csrc/measure.hip with ``-DMS_COMBINE=0``.  The host chain is the baseline, never the code under
test."""
import sys
import time

import numpy as np

import _mask_time as T          # (sets sys.path and the environment; the experiment and the timers are its)
from _object_match_time import MapTargets, median_us

SIZES = (768, 101)
CONFIDENCES = (0.0, 0.3, 0.4, 0.5, 0.6)
SPLIT = 2


def label_images(size):
    from scipy import ndimage
    rng = np.random.default_rng(size)
    salt = ndimage.label(rng.random((size, size)) < 0.45)[0].astype(np.int32)
    f = ndimage.gaussian_filter(rng.random((size, size)), 4.0)
    few = ndimage.label(f > np.quantile(f, 0.7), np.ones((3, 3)))[0].astype(np.int32)
    return (("salt", salt), ("few", few), ("one", np.ones((size, size), np.int32)))


def host_chain(dl, dp):
    """What the two entry points replace: two copies back, then numpy and scipy per object."""
    from scipy import ndimage
    labels, probs = dl.cpu().numpy(), dp.cpu().numpy()[:, :, 0]
    n = int(labels.max())
    index = np.arange(1, n + 1)
    area = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    boxes = ndimage.find_objects(labels)
    com = np.array(ndimage.center_of_mass(np.ones_like(labels), labels, index)).reshape(-1, 2)
    mean = ndimage.mean(probs, labels, index)
    return area, boxes, com, mean


def op_times(size):
    import torch
    import _measure_reference as M
    from segmentation_pipeline.segmentation import PipelineConfig as P
    from segmentation_training_pipeline_amd import ops
    h = w = size
    probs = np.random.default_rng(size + 1).random((h, w, 1)).astype(np.float32)
    dp = torch.from_numpy(probs).to("cuda")
    for kind, labels in label_images(size):
        cap = int(labels.max())
        dl = torch.from_numpy(labels).to("cuda")
        sums = torch.empty((cap + 1, 4), dtype=torch.int64, device="cuda")
        boxes = torch.empty((cap + 1, 4), dtype=torch.int32, device="cuda")
        outside = torch.empty(1, dtype=torch.int64, device="cuda")
        out, count = torch.empty_like(dl), torch.empty(1, dtype=torch.int32, device="cuda")
        out_sums, out_boxes = torch.empty_like(sums), torch.empty_like(boxes)
        ws = torch.empty(ops.label_select_workspace_bytes(cap), dtype=torch.uint8, device="cuda")
        t_measure = median_us(lambda: ops.label_measure(dl, dp, h, w, 1, 0, cap, sums, boxes, outside))
        t_select = median_us(lambda: ops.label_select(dl, h, w, cap, sums, boxes, 4, 5000, P.CONF_DEN, out, count, out_sums, out_boxes, ws))
        want = M.measure(labels, cap, probs, 0)
        assert np.array_equal(sums.cpu().numpy(), want[0]) and np.array_equal(boxes.cpu().numpy(), want[1]), "the table differs from the reference"
        sel = M.select(labels, cap, want[0], want[1], 4, 5000)
        assert int(count.item()) == sel[1] and np.array_equal(out.cpu().numpy(), sel[0]), "the selection differs from the reference"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        area, slices, com, mean = host_chain(dl, dp)
        th = time.perf_counter() - t0
        t = P.object_table(want[0], want[1], cap)
        assert np.array_equal(t["area"], area) and all((t["y0"][k], t["y1"][k], t["x0"][k], t["x1"][k]) ==
                                                       (s[0].start, s[0].stop, s[1].start, s[1].stop) for k, s in enumerate(slices))
        assert np.abs(t["cy"] - com[:, 0]).max() < 1e-9 and np.abs(t["confidence"] - mean).max() < 1e-4, "the host chain differs"
        print("%d x %d [%s] %d objects, %d kept:  stp_label_measure %8.1f us;  stp_label_select %8.1f us;  host chain (two copies back, "
              "bincount, find_objects, center_of_mass, mean) %10.1f us" % (size, size, kind, cap, sel[1], t_measure, t_select, th * 1e6),
              flush=True)


def sweep_times(out_dir, size, net):
    cfg, img_dir, ds = T.setup(out_dir, size, net)
    maps = {}
    cfg.predict_in_directory(img_dir, 0, 0, lambda name, mp, data: data.__setitem__(name, mp.arr), maps)
    sample = np.concatenate([m.reshape(-1)[::17] for m in maps.values()])
    thr_t = float(np.quantile(sample, 0.35))
    mds = MapTargets(ds, {k[:k.index(".")]: (v[:, :, 0] > thr_t).astype(np.uint8)[:, :, None] for k, v in maps.items()})
    thresholds = [float(t) for t in np.quantile(sample, [0.25, 0.3, 0.4]).astype(np.float32)]
    td, (best, table) = T.timed(lambda: cfg.find_confidence(mds, 0, thresholds=thresholds, confidences=CONFIDENCES, split=SPLIT))
    cell = (thresholds[1], CONFIDENCES[2])
    assert table[cell] == cfg.score_instances_ex(mds, 0, threshold=cell[0], split=SPLIT, min_confidence=cell[1])["score"], \
        "find_confidence differs from score_instances_ex"
    ti, _ = T.timed(lambda: cfg.score_instances(mds, 0, threshold=thresholds[1], split=SPLIT))
    te, _ = T.timed(lambda: cfg.score_instances_ex(mds, 0, threshold=thresholds[1], split=SPLIT, min_confidence=cell[1]))
    n = len(cfg.kfold(mds, range(len(mds))).sampledIndexes(0, False, "real"))
    print("%d x %d, %d validation images: find_confidence over %d x %d cells %.3f s (best %r, scores %.4f..%.4f);  one score_instances cell "
          "%.3f s;  one score_instances_ex cell %.3f s" % (size, size, n, len(thresholds), len(CONFIDENCES), td, best, min(table.values()),
                                                           max(table.values()), ti, te), flush=True)


def main(out_dir, ops_only):
    from segmentation_training_pipeline_amd import _lib
    print("library: %s" % _lib.LIB_PATH, flush=True)
    for size in SIZES:
        op_times(size)
    if not ops_only:
        for size, net in T.CASES:
            sweep_times(out_dir, size, net)


if __name__ == "__main__":
    main(sys.argv[1], "--ops-only" in sys.argv[2:])
