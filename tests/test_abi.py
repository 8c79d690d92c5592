"""CPU tests: the C-ABI library builds/loads and exports every symbol include/stp_hip.h declares
(no compute calls - there is no GPU here), and the product has no CPU fallback."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    with open(os.path.join(ROOT, "include", "stp_hip.h")) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(stp_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from segmentation_training_pipeline_amd import _lib, build
    build.build()
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "libstp_hip.so does not export %s" % n
    assert lib.stp_abi_version() == 1
    assert lib.stp_storage_dtype() == _lib.BF16
    # the IEEE-half build of the same sources: same symbols, STP_F16 storage
    f16 = _lib.load("fp16")
    for n in names:
        assert hasattr(f16, n), "libstp_hip_f16.so does not export %s" % n
    assert f16.stp_storage_dtype() == _lib.F16 == 3 and f16.stp_abi_version() == 1


def test_ctypes_signatures_cover_the_header():
    from segmentation_training_pipeline_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()


def test_param_structs_match_header_field_order():
    from segmentation_training_pipeline_amd import _lib
    with open(os.path.join(ROOT, "include", "stp_hip.h")) as f:
        src = f.read()
    for struct, cls in (("stp_conv_params", _lib.ConvParams), ("stp_wgrad_params", _lib.WgradParams)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            names = decl.split()[-1] if "," not in decl else None
            if names is None:
                first, rest = decl.split(",", 1)
                fields.append(first.split()[-1].lstrip("*"))
                fields += [r.strip().lstrip("*") for r in rest.split(",")]
            else:
                fields.append(names.lstrip("*"))
        assert fields == [f[0] for f in cls._fields_], struct


def test_no_cpu_fallback():
    import torch
    from segmentation_training_pipeline_amd import _lib, graph, nets, ops
    plan = graph.Plan(2, "bf16", "cpu", training=True)
    plan.define(lambda p: nets.unet_resnet(p, "resnet18", 64, 64))
    with pytest.raises(_lib.StpError):
        plan.run(plan.fwd)                       # a plan can be built for inspection, never run, off-GPU
    with pytest.raises(_lib.StpError):
        ops.bn_stats(torch.zeros(4, 4), 4, 4, 1e-3, 0.99, torch.zeros(4), torch.zeros(4), None, None, torch.zeros(8192))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.StpError):
            graph.Plan(2, "bf16", "cuda")


# Entry points of include/stp_hip.h that no file under tests/ names (as `stp_<name>` or through its thin wrapper `ops.<name>(`).
# Everything else the header declares must be named by a test: a kernel added without an op-level test fails
# test_every_compute_entry_point_is_named_by_a_test.  Only queries, calibration helpers and dispatch targets that the suite
# reaches through their dispatcher belong here - each with its reason.
UNNAMED_ENTRY_POINTS = {
    # calibration micro-kernels of bench.py's roofline (no result to compare: they measure the machine)
    "stp_calib_mfma_flops": "query: FLOP count of the calibration kernel",
    "stp_calib_mfma": "calibration: MFMA peak",
    "stp_calib_copy": "calibration: copy bandwidth",
    # host-side queries
    "stp_wgrad_sc_slabs": "query: slab count of the small-channel weight gradient (read by stp_conv2d_wgrad_workspace_bytes)",
    # (stp_wgrad_group_table_bytes, _workspace_bytes and _build - used by ops.WgradGroup, which the grouped weight-gradient tests
    #  construct - left this list when tests/_wgrad_plan_dump.py began to call them by name)
    # dispatch targets: the tests reach them through their dispatcher with a forced tile id / an asserted kernel id
    "stp_conv2d_sc": "stp_conv2d with tile 512 (tests assert stp_conv2d_tile_for == 512)",
    "stp_conv2d_stem": "stp_conv2d with tile 768",
    "stp_conv2d_halo": "stp_conv2d with tile 1024 + variant",
    "stp_wgrad_sc_partial": "stp_conv2d_wgrad_partial variant 0 where stp_wgrad_sc_eligible (tests assert stp_conv2d_wgrad_kernel_id == 1)",
}


def test_every_compute_entry_point_is_named_by_a_test():
    here = os.path.join(ROOT, "tests")
    text = ""
    for f in sorted(os.listdir(here)):
        if f.endswith(".py"):
            with open(os.path.join(here, f)) as fh:
                body = fh.read()
            if f == "test_abi.py":
                body = body.split("UNNAMED_ENTRY_POINTS = {")[0]         # (the allow-list itself names nothing)
            text += body + "\n"
    unnamed = [n for n in declared_symbols()
               if not re.search(r"\b%s\b" % n, text) and not re.search(r"\bops\.%s\(" % n[len("stp_"):], text)]
    assert sorted(unnamed) == sorted(UNNAMED_ENTRY_POINTS), (sorted(set(unnamed) - set(UNNAMED_ENTRY_POINTS)),
                                                            sorted(set(UNNAMED_ENTRY_POINTS) - set(unnamed)))
