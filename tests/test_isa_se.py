"""Static check of the squeeze-and-excitation kernels (CPU, no GPU): csrc/se.hip compiled to gfx950 assembly, in both storage builds,
keeps every kernel free of scratch, moves the tensors of its two element-wise passes (scale-add, backward apply) with 16-byte global
accesses, holds no floating-point atomic anywhere (every reduction is two-stage in a fixed order: replays are bit-identical) and no
buffer store with a register soffset (the wide-store form that needs the fenced slots of round 6, tests/test_isa_hazards.py)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "segmentation_training_pipeline_amd", "csrc", "se.hip")
KERNELS = ("se_reduce_kernel", "se_apply_kernel", "se_excite_kernel", "se_excite_bwd_kernel", "se_param_grad_kernel")


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def asm(request, tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("isa") / ("se_%s.s" % request.param))
    extra = ["-DSTP_STORAGE_F16=1"] if request.param == "fp16" else []
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=on", "-Wno-unused-result", "--cuda-device-only"]
                       + extra + ["-S", SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return f.read()


def kernels(text):
    """{kernel symbol: its instruction lines}"""
    out, cur = {}, None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].strip()
        m = re.match(r"^([A-Za-z_][\w$.]*):$", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
            out[cur] = []
        elif cur is not None and line and not line.startswith("."):
            out[cur].append(line)
        if line.startswith(".Lfunc_end"):
            cur = None
    return out


def test_se_hip_compiles_to_every_kernel(asm):
    ks = kernels(asm)
    for name in KERNELS:
        assert any(name in k for k in ks), name
    # squeeze / backward reduce x {fp32, 16-bit}; scale-add with and without statistics + backward apply x {fp32, 16-bit}
    assert len([k for k in ks if "se_reduce_kernel" in k]) == 4
    assert len([k for k in ks if "se_apply_kernel" in k]) == 6


def test_se_kernels_use_no_scratch(asm):
    sizes = re.findall(r"\.name:\s+(_Z\S*se_\S+)[\s\S]*?\.private_segment_fixed_size:\s+(\d+)", asm)
    assert len(sizes) >= 13
    for name, n in sizes:
        assert int(n) == 0, name


def test_element_wise_passes_move_16_bytes_per_lane(asm):
    ks = {k: v for k, v in kernels(asm).items() if "se_apply_kernel" in k}
    assert ks
    for k, lines in ks.items():
        assert any(ln.startswith("global_load_dwordx4") for ln in lines), k
        assert any(ln.startswith("global_store_dwordx4") for ln in lines), k
        # (nothing narrower touches the tensors: the only other global accesses are the per-image gate vectors and the table columns)
        assert not any(re.match(r"global_(load|store)_(ushort|short|ubyte|byte|short_d16)", ln) for ln in lines), k
    # ... and so do the two reduction passes on their operands
    for k, lines in kernels(asm).items():
        if "se_reduce_kernel" in k:
            assert any(ln.startswith("global_load_dwordx4") for ln in lines), k


def test_no_float_atomics_and_no_register_soffset_buffer_stores(asm):
    assert not re.search(r"atomic_add_f32|atomic_pk_add|atomic_add_f64|ds_add_f32|ds_add_rtn_f32", asm)
    for k, lines in kernels(asm).items():
        assert not any("atomic" in ln for ln in lines), k
        bad = [ln for ln in lines if ln.startswith("buffer_store") and re.search(r",\s*s\d+\s+(offen|idxen|offset)|,\s*s\d+$", ln)]
        assert not bad, (k, bad[:3])
