"""CPU tests of the SE-ResNet-18/34 encoders (no GPU compute): the plans build on device="cpu" under every segmentation_models
architecture, declare the ResNet's parameters plus exactly four squeeze-and-excitation tensors per unit, honour freeze_encoder, pass the
YAML surface, are refused for DeepLabV3, and leave the plain ResNet plans without an SE launch or parameter."""
import ctypes as C

import pytest
import yaml

from segmentation_pipeline import segmentation
from segmentation_training_pipeline_amd import _lib, backend, graph, models, nets

NETS = {"Unet": (nets.unet_resnet, 64), "Linknet": (nets.linknet_resnet, 64), "FPN": (nets.fpn_resnet, 64), "PSPNet": (nets.pspnet_resnet, 96)}
SE_ENTRY_POINTS = ("stp_se_chunks", "stp_se_workspace_bytes", "stp_se_squeeze", "stp_se_excite", "stp_se_scale_add", "stp_se_bwd_reduce",
                   "stp_se_excite_bwd", "stp_se_bwd_apply")


def plan_of(arch, backbone, training=True, dtype="bf16", frozen=False):
    fn, size = NETS[arch]
    p = graph.Plan(2, dtype, "cpu", training=training)
    if frozen:
        p.frozen_prefixes = nets.ENCODER_PREFIXES
    p.define(lambda pl: fn(pl, backbone, size, size, with_loss=training))
    return p


def se_params(p):
    return [k for k in p.params if "_se_fc" in k]


@pytest.mark.parametrize("arch", sorted(NETS))
@pytest.mark.parametrize("backbone", ["seresnet18", "seresnet34"])
def test_plans_build_on_the_cpu_with_four_se_tensors_per_unit(arch, backbone):
    p = plan_of(arch, backbone)
    base = plan_of(arch, nets.SE_RESNETS[backbone])
    se = se_params(p)
    # the ResNet's parameters, plus the SE tensors, nothing else
    assert [k for k in p.params if k not in se] == list(base.params)
    for k in base.params:
        assert p.params[k].shape == base.params[k].shape and p.params[k].kind == base.params[k].kind
    units = sorted(set(k.split("_se_")[0] for k in se))
    convs = sorted(k[:-len("_conv2/kernel")] for k in p.params if k.startswith("stage") and k.endswith("_conv2/kernel"))
    assert units == convs and len(se) == 4 * len(units)
    for pre in units:
        c = p.params[pre + "_conv2/kernel"].shape[0]
        r = c // 16
        assert r in (4, 8, 16, 32)
        assert p.params[pre + "_se_fc1/kernel"].shape == (1, 1, c, r) and p.params[pre + "_se_fc1/bias"].shape == (r,)
        assert p.params[pre + "_se_fc2/kernel"].shape == (1, 1, r, c) and p.params[pre + "_se_fc2/bias"].shape == (c,)
    # forward: squeeze, excite, scale-add per unit; backward: reduce, excite backward (two kernels, one entry point), apply
    fwd, bwd = [r[2] for r in p.fwd], [r[2] for r in p.bwd]
    n = len(units)
    assert [fwd.count(k) for k in ("stp_se_squeeze", "stp_se_excite", "stp_se_scale_add")] == [n, n, n]
    assert [bwd.count(k) for k in ("stp_se_bwd_reduce", "stp_se_excite_bwd", "stp_se_bwd_apply")] == [n, n, n]
    # the next BatchNormalization takes its statistics from the scale-add pass: no standalone statistics pass was added
    assert fwd.count("stp_bn_stats") == [r[2] for r in base.fwd].count("stp_bn_stats")
    assert all(rec[1][-1] is not None for rec in p.fwd if rec[2] == "stp_se_scale_add")
    assert p.bwd_monotone            # the data-parallel reducer may still overlap: SE gradients are asked for in arena order


def test_seresnet34_has_16_units_and_seresnet18_has_8():
    assert len(se_params(plan_of("Unet", "seresnet34"))) == 4 * 16
    assert len(se_params(plan_of("Unet", "seresnet18"))) == 4 * 8


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_plans_build_in_the_other_dtypes(dtype):
    p = plan_of("Unet", "seresnet18", dtype=dtype)
    assert len(se_params(p)) == 32


def test_inference_plan_emits_the_three_forward_launches_without_a_table():
    p = plan_of("Unet", "seresnet18", training=False)
    names = [r[2] for r in p.fwd]
    assert names.count("stp_se_squeeze") == names.count("stp_se_excite") == names.count("stp_se_scale_add") == 8
    assert all(rec[1][-1] is None for rec in p.fwd if rec[2] == "stp_se_scale_add")        # the inference form: no statistics
    assert not p.bwd


def test_freeze_encoder_masks_the_se_tensors():
    p = plan_of("Unet", "seresnet18", frozen=True)
    se = se_params(p)
    assert se and all(not p.params[k].trainable for k in se)
    p.set_trainable_mask()
    for k in se:
        info = p.params[k]
        assert int(p.mask[info.offset:info.offset + info.numel].sum()) == 0
    assert p.params["decoder_stage0_conv1/kernel"].trainable
    q = plan_of("Unet", "seresnet18")
    assert all(q.params[k].trainable for k in se)


def test_plain_resnet_plans_hold_no_se_launch_and_no_se_parameter():
    for arch in sorted(NETS):
        p = plan_of(arch, "resnet18")
        assert not se_params(p)
        assert not [r[2] for r in p.fwd + p.bwd if r[2] and r[2].startswith("stp_se_")]


def test_yaml_surface_and_refusals(tmp_path):
    assert "seresnet18" in models.known_backbones() and "seresnet34" in nets.known_backbones()
    base = {"architecture": "Unet", "backbone": "SEResNet34", "classes": 1, "activation": "sigmoid", "shape": [64, 64, 3], "optimizer": "Adam",
            "batch": 2, "loss": "binary_crossentropy", "stages": [{"epochs": 1}], "metrics": ["binary_accuracy"],
            "primary_metric": "val_binary_accuracy"}
    for arch, shape in (("Unet", 64), ("Linknet", 64), ("FPN", 64), ("PSPNet", 96)):
        path = str(tmp_path / ("%s.yaml" % arch))
        with open(path, "w") as f:
            yaml.safe_dump(dict(base, architecture=arch, shape=[shape, shape, 3]), f)
        m = segmentation.parse(path).createNet()
        assert m.backbone_name == "seresnet34" and m.architecture == arch
    for fn in (models.Unet, models.Linknet, models.FPN, models.PSPNet):
        with pytest.raises(ValueError, match="Unknown backbone"):
            fn(backbone_name="seresnet50", input_shape=(96, 96, 3))          # the bottleneck SE families are not built
    with pytest.raises(ValueError, match="Unknown backbone"):
        backend.HipSegModel("DeepLabV3", "seresnet18", (64, 64, 3), 1, "sigmoid", device="cpu")
    with pytest.raises(ValueError, match="Unknown backbone"):
        graph.Plan(2, "bf16", "cpu").define(lambda pl: nets.deeplab(pl, "seresnet18", 64, 64))


def test_operator_refuses_shapes_the_kernels_do_not_serve():
    def net(channels):
        def f(pl):
            img = pl.input_u8("image", 32, 32, 3)
            x = pl.input_cast("input_cast", img)
            a = pl.conv("a", x, channels, 3, pad=1)
            b = pl.conv("b", x, channels, 3, pad=1)
            return pl.se("gate", a, b)
        return f
    graph.Plan(2, "bf16", "cpu").define(net(64))
    for channels in (8, 520, 1024):           # C / 16 < 1; more channels than the per-image kernels hold
        with pytest.raises(graph.StpShapeError):
            graph.Plan(2, "bf16", "cpu").define(net(channels))


def test_ctypes_signatures_and_host_only_sizing_queries():
    vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
    for name in SE_ENTRY_POINTS:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["stp_se_workspace_bytes"] == (sz, [i32, i64, i32])
    assert _lib.SIGNATURES["stp_se_scale_add"] == (i32, [vp, vp, vp, i32, i32, i64, i32, vp, vp, vp])
    lib = _lib.load()
    # host-only queries (plans are sized without a GPU): [N][chunks][C] floats; a batch of 2 still gets >= 512 workgroups at 256 x 256
    for n, hw, c in ((2, 4, 512), (16, 128 * 128, 64), (2, 256 * 256, 64), (3, 24 * 40, 128)):
        ch = int(lib.stp_se_chunks(n, hw, c))
        assert ch >= 1 and int(lib.stp_se_workspace_bytes(n, hw, c)) == 4 * n * ch * c
        assert ch == 1 or hw // ch >= 64
    assert 2 * int(lib.stp_se_chunks(2, 256 * 256, 64)) >= 512
    for c in (12, 8, 520):
        assert int(lib.stp_se_chunks(2, 64, c)) == 0 and int(lib.stp_se_workspace_bytes(2, 64, c)) == 0
