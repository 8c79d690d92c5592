"""Timing of the prediction path (helper, not collected): ``python tests/_predict_time.py DIR`` builds U-Net/resnet34 at 512 x 512,
bf16, batch 16 under DIR, saves two checkpoints from different seeds, writes 64 synthetic 512 x 512 PNGs and times
``predict_in_directory`` over them with both folds and flip test-time augmentation (6 forward passes per image), after one untimed
pass.  Only public calls are used, so the same file runs on any revision of the repository: run it on two revisions on one machine
to compare them ("Prediction on the device").  Prints the seconds and images/s of the whole call (which loads the two fold
models), the same with the models already loaded, and a digest of every map the callback received - equal digests mean equal bits."""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault("STP_ALLOW_RANDOM_ENCODER", "1")

IMAGES, SIZE, BATCH = 64, 512, 16


def main(out_dir):
    import torch
    import yaml
    from PIL import Image
    from segmentation_pipeline import segmentation
    os.makedirs(out_dir, exist_ok=True)
    cfg_path = os.path.join(out_dir, "config.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump({"architecture": "Unet", "backbone": "resnet34", "classes": 1, "activation": "sigmoid", "encoder_weights": None,
                        "shape": [SIZE, SIZE, 3], "batch": BATCH, "dtype": "bf16", "loss": "binary_crossentropy", "folds_count": 2,
                        "stages": [{"epochs": 1}]}, f)
    cfg = segmentation.parse(cfg_path)
    net = cfg.createNet1(True)
    net.compile(loss="binary_crossentropy", batch=BATCH, dtype="bf16")
    for fold, seed in ((0, 11), (1, 23)):
        net.impl.init_weights(seed)
        net.save_weights(cfg.weightsPath(fold, 0))
    del net
    src = os.path.join(out_dir, "images")
    os.makedirs(src, exist_ok=True)
    rng = np.random.RandomState(0)
    for i in range(IMAGES):
        Image.fromarray(rng.randint(0, 256, size=(SIZE, SIZE, 3)).astype(np.uint8)).save(os.path.join(src, "im%03d.png" % i))

    def run():
        digest = hashlib.sha256()

        def cb(name, mp, data):
            digest.update(name.encode())
            digest.update(np.ascontiguousarray(mp.arr).tobytes())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cfg.predict_in_directory(src, [0, 1], 0, cb, None, ttflips=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, digest.hexdigest()[:16]

    run()                                                   # untimed: code objects, allocator, file cache
    t, d = run()
    print("predict_in_directory, 2 folds x 3 flips, %d images %dx%d: %.3f s  %.1f images/s  digest %s" % (IMAGES, SIZE, SIZE, t, IMAGES / t, d))
    loaded, load_model = {}, cfg.load_model

    def load_once(fold=0, stage=-1):
        if (fold, stage) not in loaded:
            loaded[(fold, stage)] = load_model(fold, stage)
        return loaded[(fold, stage)]
    cfg.load_model = load_once
    run()                                                   # untimed: loads the two models once
    t, d = run()
    print("the same with both models loaded: %.3f s  %.1f images/s  digest %s" % (t, IMAGES / t, d), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
