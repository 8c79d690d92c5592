"""Timing of the object-splitting path (helper, not collected): ``python tests/_split_time.py DIR`` uses the experiment of
tests/_mask_time.py - per image size (768 x 768 and 101 x 101) a one-class U-Net/resnet34 with a checkpoint from a fixed seed and 64
synthetic images - and times on this machine, in this run, at two kinds of masks (the maps above their 0.3 quantile: most pixels of
an untrained net's map set, large components joined by necks; above their 0.97 quantile: what is left are few small objects), split
radius 2:

  (a) the device chain on masks that are already there - stp_mask_edt, stp_edt_threshold, stp_mask_label, stp_label_grow,
      stp_label_unclaimed, stp_mask_label, stp_label_merge, the label images of all 64 masks copied back - after one untimed pass;
  (b) the host chain it replaces: the mask copied back, ``scipy.ndimage.distance_transform_edt``, ``scipy.ndimage.label``, the growth
      loop and the second labelling of tests/_split_reference.py;
  (c) on one image: stp_mask_edt alone, one stp_label_grow call alone (1 + 32 launches) with the number of rounds the growth needs, and
      the whole split, each the median of 50;
  (d) one ``find_split`` grid of 3 thresholds x 4 radii next to one ``score_objects`` cell (the yardstick of DESIGN.md 3.26) on the same
      validation images; one cell of the table is compared with ``score_instances``.

The host chain is the baseline, never the code under test; the label images of both sides are compared before a time is printed."""
import sys
import time

import numpy as np

import _mask_time as T          # (sets sys.path and the environment; the experiment and the timers are its)
from _object_match_time import MapTargets, median_us

QUANTILES = (0.3, 0.97)
RADIUS = 2
SPLITS = (0, 2, 4, 6)


def kernel_times(size, mask, tag):
    import torch
    import _split_reference as R
    from segmentation_pipeline.segmentation import PipelineConfig as P
    from segmentation_training_pipeline_amd import ops
    h = w = size
    a = torch.from_numpy(mask).to("cuda")
    d2 = torch.empty((h, w), dtype=torch.int32, device="cuda")
    ews = torch.empty(ops.mask_edt_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    gws = torch.empty(ops.label_grow_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
    c2 = R.c2_of(RADIUS)
    _, seeds, nc = R.cores(mask, c2)
    rounds = R.grow(mask, seeds, return_rounds=True)[1]
    s = torch.from_numpy(seeds).to("cuda")
    labels = torch.empty((h, w), dtype=torch.int32, device="cuda")
    changed = torch.empty(1, dtype=torch.int32, device="cuda")
    from segmentation_training_pipeline_amd import _lib
    lib, st = _lib.load(), ops.stream

    def one_grow_call():
        _lib.check(lib.stp_label_grow(a.data_ptr(), s.data_ptr(), h, w, labels.data_ptr(), changed.data_ptr(), gws.data_ptr(), gws.numel(), st()))
    t_edt = median_us(lambda: ops.mask_edt(a, h, w, d2, ews))
    t_grow = median_us(one_grow_call)
    t_all = median_us(lambda: P._device_split(a, c2))
    t_plain = median_us(lambda: P._device_labels(a))
    print("  [%s] stp_mask_edt (2 launches) %8.1f us;  one stp_label_grow call (1 + 32 launches; %d cores, the growth needs %d rounds) %8.1f us;  "
          "the whole split (with its host reads) %8.1f us;  stp_mask_label alone %8.1f us" % (tag, t_edt, nc, rounds, t_grow, t_all, t_plain),
          flush=True)


def main(out_dir):
    import torch
    import _split_reference as R
    from segmentation_pipeline.segmentation import PipelineConfig as P
    for size, net in T.CASES:
        cfg, img_dir, ds = T.setup(out_dir, size, net)
        maps = {}
        cfg.predict_in_directory(img_dir, 0, 0, lambda name, mp, data: data.__setitem__(name, mp.arr), maps)
        sample = np.concatenate([m.reshape(-1)[::17] for m in maps.values()])
        c2 = R.c2_of(RADIUS)
        for q in QUANTILES:
            thr = float(np.quantile(sample, q))
            masks = {k: (v[:, :, 0] > thr).astype(np.uint8) for k, v in maps.items()}
            dev_masks = {k: torch.from_numpy(v).to("cuda") for k, v in masks.items()}

            def device_chain():
                return {k: P._device_split(m, c2)[0].cpu().numpy() for k, m in dev_masks.items()}

            def host_chain():
                return {k: R.split(m.cpu().numpy(), c2)[0] for k, m in dev_masks.items()}
            td, got = T.timed(device_chain)
            t0 = time.perf_counter()
            want = host_chain()
            th = time.perf_counter() - t0
            assert all(np.array_equal(got[k], want[k]) for k in want), "the device labels differ from the host chain"
            plain = [R.label(m, 2)[1] for m in list(masks.values())[:8]]
            after = [int(want[k].max()) for k in list(masks)[:8]]
            print("%d x %d, %d images, masks above the %.2f quantile, split radius %g: %d components per image become %d objects (means of 8)" %
                  (size, size, T.IMAGES, q, RADIUS, int(np.mean(plain)), int(np.mean(after))), flush=True)
            print("  masks already there, label images copied back: host (copy back + distance_transform_edt + label + growth loop + label) "
                  "%.3f s;  device %.4f s" % (th, td), flush=True)
            first = sorted(masks)[0]
            kernel_times(size, masks[first], "q%.2f" % q)
        thr_t = float(np.quantile(sample, 0.35))
        mds = MapTargets(ds, {k[:k.index(".")]: (v[:, :, 0] > thr_t).astype(np.uint8)[:, :, None] for k, v in maps.items()})
        thresholds = [float(t) for t in np.quantile(sample, [0.25, 0.3, 0.4]).astype(np.float32)]
        td, (best, table) = T.timed(lambda: cfg.find_split(mds, 0, thresholds=thresholds, splits=SPLITS))
        cell = (thresholds[1], SPLITS[1])
        assert table[cell] == cfg.score_instances(mds, 0, threshold=cell[0], split=cell[1])["score"], "find_split differs from score_instances"
        ty, _ = T.timed(lambda: cfg.score_objects(mds, 0, threshold=thresholds[1]))
        ti, _ = T.timed(lambda: cfg.score_instances(mds, 0, threshold=thresholds[1], split=RADIUS))
        n = len(cfg.kfold(mds, range(len(mds))).sampledIndexes(0, False, "real"))
        print("  %d validation images: find_split over %d x %d cells %.3f s (best %r, scores %.4f..%.4f);  one score_objects cell %.3f s;  one "
              "score_instances cell %.3f s" % (n, len(thresholds), len(SPLITS), td, best, min(table.values()), max(table.values()), ty, ti),
              flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
