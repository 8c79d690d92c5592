"""Timing of the boundary-score path (helper, not collected): ``python tests/_boundary_time.py`` times on this machine, in this run, one
768 x 768 and one 101 x 101 image at two kinds of masks - salt and pepper (a uniform random map above 0.7 / 0.72: nearly every foreground
pixel is surface) and few objects (a Gaussian field, sigma 12, above 0.6 / 0.62) -:

  (a) stp_surface_distances alone, masks and target on the device (device events around the 12 launches);
  (b) the cell of ``score_boundaries`` / ``find_boundary_threshold``: ``_device_mask`` of the finished device map, stp_surface_distances
      against the device target, the counters copied back (host clock, ends in the copy);
  (c) the host chain it replaces: the map copied back, ``>``, the two surfaces and two ``scipy.ndimage.distance_transform_edt``
      (``squared_distances`` of tests/_boundary_reference.py; its counters - a Python loop - are left out of the time).

Each figure is the mean of 10 runs after one untimed run, with the least and the largest.  The host chain is the baseline, never the code
under test; the counters of both sides are compared before a time is printed."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

C2, NUM, DEN, RUNS = [1, 4, 9], 950, 1000, 10


def maps(size, kind):
    from scipy import ndimage
    f = np.random.default_rng(size).random((size, size))
    if kind == "few objects":
        f = ndimage.gaussian_filter(f, 12.0)
        f = (f - f.min()) / (f.max() - f.min())
    return f.astype(np.float32), (0.7, 0.72) if kind == "salt and pepper" else (0.6, 0.62)


def stats(times):
    return "%9.3f ms (%.3f .. %.3f)" % (1e3 * float(np.mean(times)), 1e3 * min(times), 1e3 * max(times))


def host_clock(fn):
    fn()
    times = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t0)
    return times, out


def main():
    import torch
    import _boundary_reference as R
    from segmentation_pipeline.segmentation import PipelineConfig
    from segmentation_training_pipeline_amd import ops
    cfg = PipelineConfig(architecture="Unet", backbone="resnet18", classes=1, activation="sigmoid", shape=[64, 64, 3], batch=1)
    for size in (768, 101):
        h = w = size
        for kind in ("salt and pepper", "few objects"):
            f, (thr, thr_t) = maps(size, kind)
            probs = torch.from_numpy(f[:, :, None].copy()).to("cuda")
            target = torch.from_numpy((f > np.float32(thr_t)).view(np.uint8)).to("cuda")
            mask = cfg._device_mask(probs, 0, thr, 0, 0, 0)
            out = torch.empty(2 * (3 + len(C2)) + 3, dtype=torch.int64, device="cuda")
            ws = torch.empty(ops.surface_distances_workspace_bytes(h, w), dtype=torch.uint8, device="cuda")
            st = torch.cuda.current_stream()

            def entry():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                ops.surface_distances(mask, target, h, w, C2, NUM, DEN, out, ws)
                e1.record(st)
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e-3

            def cell():
                ops.surface_distances(cfg._device_mask(probs, 0, thr, 0, 0, 0), target, h, w, C2, NUM, DEN, out, ws)
                return out.cpu().numpy()

            def host():      # (without the reference's per-pixel math.isqrt and sort: the part no host user could avoid)
                return R.squared_distances(probs.cpu().numpy()[:, :, 0] > np.float32(thr), f > np.float32(thr_t))
            entry()
            t_entry = [entry() for _ in range(RUNS)]
            t_cell, got = host_clock(cell)
            t_host, _ = host_clock(host)
            want = R.counters(f > np.float32(thr), f > np.float32(thr_t), C2, NUM, DEN)
            assert np.array_equal(got, want), "the device counters differ from the host chain"
            print("%d x %d, %s: %d + %d surface pixels, max D2 %d" % (size, size, kind, want[0], want[3 + len(C2)], max(want[1], want[7])))
            print("  (a) stp_surface_distances alone          %s" % stats(t_entry))
            print("  (b) device cell: mask + entry + counters %s" % stats(t_cell))
            print("  (c) host chain: copy back + 2 x edt      %s" % stats(t_host), flush=True)


if __name__ == "__main__":
    main()
