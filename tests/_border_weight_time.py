"""Timing of border_weights (helper, not collected): ``python tests/_border_weight_time.py [kernels|steps] ...``.

  * ``kernels``: at 16 x 512 x 512, bf16, on masks of 40 discs per sample, the three launch groups a keyed step adds or swaps, each alone
    between two device events, the mean of 10 calls (and their least and largest) after a warm-up: the 16 stp_mask_label calls (6 launches
    each), stp_border_weight at radius 20 and 32 (2 launches), stp_sigmoid_bce_dice_weighted with its gradient (3 launches) next to
    stp_sigmoid_bce_dice on the same logits.
  * ``steps``: the whole training step of U-Net/resnet18, bf16, hipGraph replay, 16 x 512 x 512, with
    ``border_weights: {w0: 10, sigma: 5, radius: 20}`` and without the key, same spec otherwise: the mean of 10 steps after a warm-up.
    """
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("STP_ALLOW_RANDOM_ENCODER", "1")

N, SIZE, RUNS = 16, 512, 10
SPEC = "binary_crossentropy+dice_loss"


def disc_masks(n, size, seed=0, discs=40):
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:size, :size]
    y = np.zeros((n, size, size, 1), np.uint8)
    for i in range(n):
        for _ in range(discs):
            cy, cx, r = rng.randint(0, size), rng.randint(0, size), rng.randint(6, 30)
            y[i, :, :, 0][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1
    return y


def timed(fn):
    import torch
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


def kernels():
    import torch
    from segmentation_training_pipeline_amd import ops
    px = N * SIZE * SIZE
    mask = torch.from_numpy(disc_masks(N, SIZE)).cuda().reshape(N, SIZE, SIZE)
    labels = torch.empty((N, SIZE, SIZE), dtype=torch.int32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    ws_l = torch.empty(ops.mask_label_workspace_bytes(SIZE, SIZE), dtype=torch.uint8, device="cuda")
    ws_w = torch.empty(ops.border_weight_workspace_bytes(N, SIZE, SIZE), dtype=torch.uint8, device="cuda")
    wmap = torch.empty((N, SIZE, SIZE), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(1)
    z = (torch.randn(px, device="cuda", generator=g) * 2).to(torch.bfloat16)
    sc = torch.zeros(16, dtype=torch.float32, device="cuda")
    dl = torch.zeros((px, 8), dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(ops.loss_workspace_bytes() // 4, dtype=torch.float32, device="cuda")

    def label_all():
        for n in range(N):
            ops.mask_label(mask[n], SIZE, SIZE, 2, 0, labels[n], count, ws_l)

    print("box %d x %d x %d, bf16" % (N, SIZE, SIZE), flush=True)
    print("  %d x stp_mask_label                  %9.3f ms (%.3f .. %.3f)" % ((N,) + timed(label_all)), flush=True)
    print("    objects per sample: %s" % [int(labels[n].max()) for n in range(N)], flush=True)
    for radius, sigma in ((20, 5.0), (32, 8.0)):
        t = timed(lambda: ops.border_weight(labels, N, SIZE, SIZE, 10.0, sigma, radius, 1.0, 1.0, wmap, ws_w))
        print("  stp_border_weight, radius %2d          %9.3f ms (%.3f .. %.3f)   mean weight %.4f" % ((radius,) + t + (float(wmap.mean()),)), flush=True)
    ops.border_weight(labels, N, SIZE, SIZE, 10.0, 5.0, 20, 1.0, 1.0, wmap, ws_w)
    t = timed(lambda: ops.sigmoid_bce_dice_weighted(z, mask, px, 1.0, 1.0, sc, dl, 8, 1.0, ws, wmap))
    print("  stp_sigmoid_bce_dice_weighted         %9.3f ms (%.3f .. %.3f)   weighted bce %.5f, bce %.5f" % (t + (float(sc[13]), float(sc[1]))), flush=True)
    t = timed(lambda: ops.sigmoid_bce_dice(z, mask, px, 1.0, 1.0, sc, dl, 8, 1.0, ws))
    print("  stp_sigmoid_bce_dice (the sibling)    %9.3f ms (%.3f .. %.3f)" % t, flush=True)


def steps():
    import torch
    from segmentation_training_pipeline_amd.backend import HipSegModel
    rng = np.random.RandomState(0)
    x = rng.randint(0, 256, (N, SIZE, SIZE, 3)).astype(np.uint8)
    y = disc_masks(N, SIZE)
    for key in (None, {"w0": 10, "sigma": 5, "radius": 20}):
        m = HipSegModel("Unet", "resnet18", (SIZE, SIZE, 3), 1, "sigmoid", batch=N, dtype="bf16", loss=SPEC, optimizer="Adam", lr=1e-3,
                        use_graph=True, border_weights=key)
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
        print("step U-Net/resnet18 bf16 %d x %d x %d, %s, border_weights %-40s %9.3f ms (%.3f .. %.3f)   loss %.5f" %
              (N, SIZE, SIZE, SPEC, key, sum(ms) / RUNS, min(ms), max(ms), m.metrics()["loss"]), flush=True)
        del m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1:] or ["kernels", "steps"]
    if "kernels" in what:
        kernels()
    if "steps" in what:
        steps()
