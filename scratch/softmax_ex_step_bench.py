"""bench.py's step with another loss spec on the softmax configs: what leaving the low-resolution (_up) loss fusion costs.
``python scratch/softmax_ex_step_bench.py "categorical_crossentropy+dice_loss+focal_loss" --config 4 --steps 60 --warmup 10``
(the remaining arguments are bench.py's; the spec replaces its LOSS_SOFTMAX)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

bench.LOSS_SOFTMAX = sys.argv[1]
sys.argv = ["bench.py"] + sys.argv[2:]
bench.main()
