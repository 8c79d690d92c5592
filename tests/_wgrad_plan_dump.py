"""Host decisions of the weight-gradient family as text (a tool in the manner of tests/_plan_dump.py; not collected, needs no GPU):
what the planner of csrc/conv_wgrad*.hip answers for every case of tests/_wgrad_reference.py, so that two builds of the library can be
compared with ``diff -r``.  The queries look at shapes and at which pointers are set, never at memory: every pointer is ``fake``.

``python tests/_wgrad_plan_dump.py OUT_DIR`` writes one file per (case, dtype) into one subdirectory per switch setting:

* single-layer cases (``all_single_cases()``): stp_conv2d_wgrad_kernel_id, stp_wgrad_sc_eligible, stp_wgrad_group_class,
  stp_conv2d_wgrad_workspace_bytes;
* lone layers (``LONE_LAYERS``): the return value and the descriptor bytes of stp_wgrad_reduce_desc_fill;
* groups (every group of ``GROUPS``, and the 128 / 64 / 32 classes with one fused producer BatchNormalization, as
  tests/test_wgrad_ops_gpu.py forms them): stp_wgrad_group_table_bytes, stp_wgrad_group_workspace_bytes, the return code of
  stp_wgrad_group_build and the sha256 of the table it filled (the builder clears the table, and the compute-unit query answers 256
  without a device: the bytes are a function of the shapes).

The library reads its switches once per process, so each setting of SWITCHES runs in a fresh child process.  STP_LIB / STP_LIB_F16
select the library, as everywhere else.  No golden file is kept: tuning a plan must not churn one."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _wgrad_reference as R  # noqa: E402

SWITCHES = [None, ("STP_WGRAD_TAPS9", "0"), ("STP_WGRAD_TAPS9", "2"), ("STP_WGRAD_ROW", "0")]
FAKE = 0x10000


def switch_name(switch):
    return "default" if switch is None else "%s=%s" % switch


def _lib_of(dtype):
    from segmentation_training_pipeline_amd import _lib
    return _lib.load("fp16" if dtype == "fp16" else "bf16")


def _params(case, dtype):
    from segmentation_training_pipeline_amd import _lib
    return R.fill_params(_lib.WgradParams(), case, dtype, FAKE, FAKE, FAKE, src1=FAKE if case.c1 else None,
                         bn=(FAKE, FAKE, FAKE, FAKE) if case.bn is not None else None)


def single_text(case, dtype):
    lib, P = _lib_of(dtype), _params(case, dtype)
    return "kernel_id %d\nsc_eligible %d\ngroup_class %d\nworkspace_bytes %d\n" % (
        int(lib.stp_conv2d_wgrad_kernel_id(C.byref(P))), int(lib.stp_wgrad_sc_eligible(C.byref(P))),
        int(lib.stp_wgrad_group_class(C.byref(P))), int(lib.stp_conv2d_wgrad_workspace_bytes(C.byref(P))))


def lone_text(i, dtype):
    lib, P = _lib_of(dtype), _params(R.lone_case(i), dtype)
    db = int(lib.stp_wgrad_reduce_desc_bytes())
    table = (C.c_char * (db * 2))()
    count = int(lib.stp_wgrad_reduce_desc_fill(C.addressof(table), 1, C.byref(P), FAKE))
    return "desc_bytes %d\ndesc_fill %d\ndesc %s\n" % (db, count, bytes(table).hex())


def group_text(group, dtype, fused_index=None):
    from segmentation_training_pipeline_amd import _lib
    lib = _lib_of(dtype)
    cases = [R.group_case(group, i, bn=(1 + i % 2) if i == fused_index else None) for i in range(len(R.GROUPS[group]))]
    params = [_params(c, dtype) for c in cases]
    n = len(params)
    arr = (C.POINTER(_lib.WgradParams) * n)(*[C.pointer(p) for p in params])
    tb = int(lib.stp_wgrad_group_table_bytes(arr, n))
    wsb = int(lib.stp_wgrad_group_workspace_bytes(arr, n))
    host = (C.c_char * max(tb, 16))()
    rc = int(lib.stp_wgrad_group_build(arr, n, C.addressof(host), tb))
    header = list((C.c_int32 * 16).from_buffer_copy(bytes(host)[:64])) if tb >= 64 else []
    return "table_bytes %d\nworkspace_bytes %d\nbuild %d\nheader %s\ntable sha256 %s\n" % (
        tb, wsb, rc, header, hashlib.sha256(bytes(host)[:tb]).hexdigest())


def cells():
    """(file name, function producing its text), in a fixed order."""
    out = []
    for case in R.all_single_cases():
        for dtype in R.dtypes_of(case):
            out.append(("single-%s-%s-%s" % (case.family, case.name, dtype), lambda c=case, d=dtype: single_text(c, d)))
    for i in range(len(R.LONE_LAYERS)):
        for dtype in R.DTYPES:
            out.append(("lone-%d-%s" % (i, dtype), lambda i=i, d=dtype: lone_text(i, d)))
    for group in sorted(R.GROUPS):
        for dtype in R.H16:
            out.append(("group-%s-%s" % (group, dtype), lambda g=group, d=dtype: group_text(g, d)))
    for group in ("class128", "class64", "class32"):
        direct = [i for i, s in enumerate(R.GROUPS[group]) if s[4] == 0]
        for dtype in R.H16:
            out.append(("group-%s-bn-%s" % (group, dtype), lambda g=group, d=dtype, f=direct[len(direct) // 2]: group_text(g, d, f)))
    return out


def dump(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    for name, fn in cells():
        text = fn()
        with open(os.path.join(out_dir, name + ".txt"), "w") as f:
            f.write(text)
        print("%s  %s" % (name, hashlib.sha256(text.encode()).hexdigest()[:16]), flush=True)


def main(argv):
    if len(argv) == 2 and argv[0] == "--one":      # the child: the environment holds the switch
        return dump(argv[1])
    out_dir = argv[0]
    for switch in SWITCHES:
        env = {k: v for k, v in os.environ.items() if k not in [s[0] for s in SWITCHES[1:]]}
        if switch is not None:
            env[switch[0]] = switch[1]
        print("== %s" % switch_name(switch), flush=True)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--one", os.path.join(out_dir, switch_name(switch))], env=env, check=True)


if __name__ == "__main__":
    main(sys.argv[1:])
