"""bench.py's step with the class metrics switched on (the confusion launch behind the softmax loss): what the launch costs the step.
``python scratch/class_confusion_step_bench.py --config 4 --steps 60 --warmup 10`` (the arguments are bench.py's; run bench.py itself
with the same arguments on the same box for the step without the launch)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from segmentation_training_pipeline_amd import backend  # noqa: E402

_init = backend.HipSegModel.__init__


def init(self, *a, **k):
    if (a[4] if len(a) > 4 else k.get("activation")) == "softmax":
        k.setdefault("class_metrics", True)
    _init(self, *a, **k)


backend.HipSegModel.__init__ = init
bench.main()
