"""Timing of the object-score path (helper, not collected): ``python tests/_object_match_time.py DIR`` uses the experiment of
tests/_mask_time.py - per image size (768 x 768 and 101 x 101) a one-class U-Net/resnet34 with a checkpoint from a fixed seed and 64
synthetic images - and times on this machine, in this run, at two kinds of masks (the maps above their 0.7 quantile: an untrained
net's salt and pepper, thousands of objects per image; above their 0.97 quantile: few objects; the target is the map above a slightly
higher quantile, so the objects overlap without being equal):

  (a) the device chain of one sweep cell on masks that are already there - stp_mask_label of the mask, stp_label_match against the
      labelled target, the T + 3 integers of all 64 images copied back once - after one untimed pass;
  (b) the host chain it replaces: the mask copied back, ``scipy.ndimage.label`` of mask and target, the pair histogram and the
      comparisons of tests/_object_match_reference.py;
  (c) ``find_object_threshold`` over 19 thresholds x 4 min_sizes next to the 76 host passes over the same validation images (maps from
      ``evaluateAll``, numpy's ``>``, remove_small_objects, label, the reference; the target - the map above its 0.72 quantile - labelled
      once per image on both sides);
  (d) stp_label_match alone on one image: its median time over 50 launches, and the same on two all-zero label images - no table insert,
      no area: what is left is the clear and the final pass over the 2 * h * w slots plus reading the pixels - next to a device copy of
      as many bytes as the table has.

The host chain is the baseline, never the code under test; the counters of both sides are compared before a time is printed."""
import sys
import time

import numpy as np

import _mask_time as T          # (sets sys.path and the environment; the experiment and the timers are its)

QUANTILES = ((0.7, 0.72), (0.97, 0.975))          # (scored masks, target masks)
NUMS, DEN = list(range(500, 1000, 50)), 1000
MIN_SIZES = (0, 4, 16, 64)


def median_us(fn, reps=50):
    import torch
    st = torch.cuda.current_stream()
    fn(); torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st); fn(); e1.record(st)
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in evs)[reps // 2] * 1e3


def kernel_times(size, pred, truth, tag):
    import torch
    from segmentation_training_pipeline_amd import ops
    h = w = size
    cap = (h * w + 1) // 2
    out = torch.empty(len(NUMS) + 3, dtype=torch.int64, device="cuda")
    nbytes = ops.label_match_workspace_bytes(h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    zeros = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    full = median_us(lambda: ops.label_match(pred, truth, h, w, cap, NUMS, DEN, out, ws))
    counters = out.cpu().numpy().tolist()
    empty = median_us(lambda: ops.label_match(zeros, zeros, h, w, cap, NUMS, DEN, out, ws))
    copy = median_us(lambda: dst.copy_(src))
    print("  [%s] stp_label_match (3 launches) %8.1f us;  on all-zero images (clear + final pass over the slots + the pixels) %8.1f us;  "
          "workspace %d bytes, a device copy of as many %6.1f us;  n_pred %d n_truth %d TP@0.5 %d" %
          (tag, full, empty, nbytes, copy, counters[10], counters[11], counters[0]), flush=True)


class MapTargets(object):
    """The items of ``ds`` with the masks ``targets[id]`` in place of their own."""

    def __init__(self, ds, targets):
        self.ds, self.targets = ds, targets

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        it = self.ds[i]
        it.y = self.targets[it.id]
        return it

    def isPositive(self, i):
        return True


def main(out_dir):
    import torch
    import _components_reference as CR
    import _object_match_reference as R
    from segmentation_training_pipeline_amd import ops
    for size, net in T.CASES:
        cfg, img_dir, ds = T.setup(out_dir, size, net)
        maps = {}
        cfg.predict_in_directory(img_dir, 0, 0, lambda name, mp, data: data.__setitem__(name, mp.arr), maps)
        sample = np.concatenate([m.reshape(-1)[::17] for m in maps.values()])
        h = w = size
        cap = (h * w + 1) // 2
        for q, qt in QUANTILES:
            thr, thr_t = float(np.quantile(sample, q)), float(np.quantile(sample, qt))
            masks = {k: (v[:, :, 0] > thr).astype(np.uint8) for k, v in maps.items()}
            targets = {k: (v[:, :, 0] > thr_t).astype(np.uint8) for k, v in maps.items()}
            dev_masks = {k: torch.from_numpy(v).to("cuda") for k, v in masks.items()}
            dev_targets = {k: cfg._device_labels(torch.from_numpy(v).to("cuda"))[0] for k, v in targets.items()}
            ws = torch.empty(ops.label_match_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")

            def device_cell():
                out = torch.empty((len(dev_masks), len(NUMS) + 3), dtype=torch.int64, device="cuda")
                for i, k in enumerate(dev_masks):
                    ops.label_match(cfg._device_labels(dev_masks[k])[0], dev_targets[k], h, w, cap, NUMS, DEN, out[i], ws)
                return out.cpu().numpy()

            def host_cell():
                return np.stack([R.label_match(R.label8(dev_masks[k].cpu().numpy())[0], R.label8(targets[k])[0], cap, NUMS, DEN)
                                 for k in dev_masks])
            td, got = T.timed(device_cell)
            t0 = time.perf_counter()
            want = host_cell()
            th = time.perf_counter() - t0
            assert np.array_equal(got, want), "the device counters differ from the host chain"
            print("%d x %d, %d images, masks above the %.2f quantile, targets above the %.3f: %d predicted and %d target objects per image, "
                  "TP at 0.5 / 0.75 / 0.95: %d / %d / %d (sums: %d, %d; %d, %d, %d)" %
                  ((size, size, T.IMAGES, q, qt) + tuple(int(v) for v in want[:, [10, 11, 0, 5, 9]].mean(axis=0)) +
                   tuple(int(v) for v in want[:, [10, 11, 0, 5, 9]].sum(axis=0))), flush=True)
            print("  one sweep cell, masks already there: host (copy back + scipy label x 2 + pair histogram) %.3f s;  device (label + match + "
                  "one copy of the counters) %.4f s" % (th, td), flush=True)
            first = sorted(dev_masks)[0]
            kernel_times(size, cfg._device_labels(dev_masks[first])[0], dev_targets[first], "q%.2f" % q)
        # (c) the grid: the items' targets are the maps above their 0.72 quantile - against the dataset's own masks (one ellipse per image)
        # an untrained net scores 0 in every cell, and equal tables of zeros would show nothing
        thr_t = float(np.quantile(sample, QUANTILES[0][1]))
        ds = MapTargets(ds, {k[:k.index(".")]: (v[:, :, 0] > thr_t).astype(np.uint8)[:, :, None] for k, v in maps.items()})
        thresholds = [float(t) for t in np.unique(np.quantile(sample, [0.5 + 0.025 * d for d in range(1, 20)]).astype(np.float32))]
        cells = [(t, m) for t in thresholds for m in MIN_SIZES]

        def host_grid():
            pairs = []
            for b in cfg.evaluateAll(ds, 0):
                pairs += [(p.arr[:, :, 0], R.label8(g.arr[:, :, 0])[0]) for p, g in zip(b.predicted_maps_aug, b.segmentation_maps)]
            table = {}
            for c, (t, m) in enumerate(cells):
                counts = np.stack([R.label_match(R.label8(CR.remove_small_objects(p > np.float32(t), m))[0], g, cap, NUMS, DEN) for p, g in pairs])
                per = R.object_score("f2", counts[:, :10], counts[:, 10:11], counts[:, 11:12])
                table[(t, m)] = float(per.mean(axis=1).mean())
                if c % 8 == 7:
                    print("    host pass %d of %d" % (c + 1, len(cells)), flush=True)
            return table, len(pairs)
        td, (best, table) = T.timed(lambda: cfg.find_object_threshold(ds, 0, thresholds=thresholds, min_sizes=MIN_SIZES))
        t0 = time.perf_counter()
        want, n = host_grid()
        th = time.perf_counter() - t0
        assert table == want, "find_object_threshold differs from the host passes"
        assert len(set(table.values())) > len(cells) // 2, "the grid does not move the score"
        print("  %d x %d grid, %d validation images: evaluateAll + %d host passes %.2f s;  find_object_threshold %.3f s;  best cell %r, "
              "score %.4f (worst %.4f)" % (len(thresholds), len(MIN_SIZES), n, len(cells), th, td, best, table[best], min(table.values())),
              flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
