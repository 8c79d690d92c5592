"""Canonical text of a defined plan (helper of tests/test_host.py; not collected): one line per launch record of ``prep``, ``fwd``
and ``bwd``, addresses replaced by what they point to, so that the plans two versions of the plan builder produce can be compared
with ``diff``.  Plans build on ``device="cpu"``: nothing here needs a GPU.

* Pointers: every integer that lies inside a buffer the plan owns - the tensors and ctypes objects of ``_keep``, the arenas and
  workspaces, every tensor's activation / gradient buffer, the inputs - is written as ``@ordinal+offset/size``, the ordinal counting
  buffers by FIRST APPEARANCE in the launch stream (a harmless reordering of allocations does not show).
* Structs: a ``byref`` argument is written as the fields of its struct; a struct reached through a table is written once, as a line
  of its own, when it first appears.
* Tables (host and device descriptor tables: weight preparation, class collapse, weight-gradient groups, batched reduces): hashed
  after the same resolution of every aligned 8-byte word, once, when they first appear.
* Summary lines: ``bwd_marks``, ``bwd_monotone``, ``wgroups``, the parameter and state declarations, the tensors, the bytes ``_keep``
  holds.
* An integer of 2^40 or more that resolves to no buffer is an error, not a token.

``python tests/_plan_dump.py OUT_DIR [plan ...]`` writes ``<plan>@<switch>.txt`` for every cell of PLANS x SWITCHES (or of the named plans)
and prints one ``cell  records  sha256[:16]`` line each (22 plans x 19 switches = 418 cells; DESIGN.md 4.1 and 4.3 compare such tables).  To compare two versions of
the plan builder, run it in a checkout of each and ``diff -r`` the two directories."""
import bisect
import ctypes as C
import hashlib
import os
import struct
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_CDATA = C.Structure.__mro__[1]          # ctypes._CData: Structure, Array, ...
_BIG = 1 << 40


class _Buffers(object):
    """The address ranges a plan owns, numbered as the launch stream meets them."""

    def __init__(self):
        self.ranges = {}                 # start -> (end, object)
        self.starts = None
        self.ordinal = {}
        self.tables = set()              # ids of the device descriptor tables (the one-dimensional byte tensors of ``_keep``)
        self.pending = []                # structs / tables met for the first time: written after the current record

    def add(self, obj):
        if obj is None:
            return
        if isinstance(obj, torch.Tensor):
            start, size = obj.data_ptr(), obj.numel() * obj.element_size()
        else:
            start, size = C.addressof(obj), C.sizeof(obj)
        if size and self.ranges.get(start, (0, None))[0] < start + size:
            self.ranges[start] = (start + size, obj)
        self.starts = None

    def resolve(self, v):
        if self.starts is None:
            self.starts = sorted(self.ranges)
        i = bisect.bisect_right(self.starts, v) - 1
        if i < 0:
            return None
        start = self.starts[i]
        end, obj = self.ranges[start]
        if v >= end:
            return None
        if start not in self.ordinal:
            self.ordinal[start] = len(self.ordinal)
            if isinstance(obj, _CDATA) or id(obj) in self.tables:
                self.pending.append((self.ordinal[start], obj))
        return "@%d+%d/%d" % (self.ordinal[start], v - start, end - start)

    def value(self, v, strict=True):
        if v is None:
            return "0"
        if isinstance(v, bool):
            return str(int(v))
        if isinstance(v, int):
            r = self.resolve(v)
            if r is None and strict and v >= _BIG:
                raise ValueError("address %#x belongs to no buffer of the plan" % v)
            return r if r is not None else str(v)
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, bytes):
            return "bytes:" + hashlib.sha256(v).hexdigest()[:16]
        if isinstance(v, C.Structure):
            return self.struct(v)
        if hasattr(v, "_obj"):           # ctypes.byref(struct)
            return self.struct(v._obj)
        raise TypeError("launch argument of type %s" % type(v).__name__)

    def struct(self, s):
        return "%s{%s}" % (type(s).__name__, ",".join("%s=%s" % (f[0], self.value(getattr(s, f[0]))) for f in s._fields_))

    def table(self, obj):
        raw = bytes(obj.numpy().tobytes()) if isinstance(obj, torch.Tensor) else bytes(bytearray(obj))
        n8 = len(raw) // 8
        words = [self.value(w, strict=False) for w in struct.unpack("<%dQ" % n8, raw[:8 * n8])]
        return "table[%d]:%s" % (len(raw), hashlib.sha256((" ".join(words) + "|").encode() + raw[8 * n8:]).hexdigest()[:16])

    def drain(self, out):
        while self.pending:
            ordinal, obj = self.pending.pop(0)
            out.append("  @%d = %s" % (ordinal, self.struct(obj) if isinstance(obj, C.Structure) else self.table(obj)))


def _meta(m):
    return "-" if m is None else "{%s}" % ",".join("%s=%r" % (k, m[k]) for k in sorted(m))


def dump(plan, model=None):
    """The canonical text of a defined plan (``model``: the HipSegModel that owns it - its ``opt`` list and buffers are included)."""
    b = _Buffers()
    for t in plan._keep:
        b.add(t)
        if isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 1:
            b.tables.add(id(t))
    for name in ("P", "G", "S", "mask", "ws_wgrad", "ws_bn", "ws_loss", "ws_dw", "ws_lovasz", "slot_arena", "loss_scalars", "_loss_weights",
                 "step_state", "dls", "probs"):
        b.add(getattr(plan, name, None))
    for t in list(plan.tensors.values()) + list(plan.inputs.values()):
        b.add(t.buf)
        b.add(t.grad)
    lists = [("prep", plan.prep), ("fwd", plan.fwd), ("bwd", plan.bwd)]
    if model is not None:
        for name in ("m", "v", "vel", "lr", "opt_state", "opt_fstate", "gscale", "ws_norm", "dls"):
            b.add(getattr(model, name, None))
        lists.append(("opt", plan.opt))
    out = []
    for lname, lst in lists:
        for i, (fn, args, name, meta) in enumerate(lst):
            out.append("%s[%d] %s(%s) %s" % (lname, i, name, ", ".join(b.value(a) for a in args), _meta(meta)))
            b.drain(out)
    out.append("bwd_marks %s" % [(n, int(low)) for n, low in plan.bwd_marks])
    out.append("bwd_monotone %s" % bool(plan.bwd_monotone))
    out.append("wgroups %s" % [(list(names), int(cls)) for names, cls in plan.wgroups])
    for k, p in plan.params.items():
        out.append("param %s %d %s %s %d" % (k, p.offset, tuple(p.shape), p.kind, int(p.trainable)))
    for k, s in plan.states.items():
        out.append("state %s %s" % (k, tuple(s)))
    for k, t in plan.tensors.items():
        out.append("tensor %s %dx%dx%dx%d gradC=%d needs_grad=%d grad=%s uses=%s folded=%d" % (
            k, t.N, t.H, t.W, t.C, t.gradC, int(t.needs_grad), b.value(t.grad.data_ptr()) if t.grad is not None else "-",
            t.meta.get("uses", 0), int(bool(t.meta.get("dgrad_folded")))))
    kept = [t for t in plan._keep if isinstance(t, torch.Tensor)]
    out.append("keep %d objects, %d tensors, %d bytes" % (len(plan._keep), len(kept), sum(t.numel() * t.element_size() for t in kept)))
    return "\n".join(out) + "\n"


def records(text):
    return sum(1 for l in text.splitlines() if l.startswith(("prep[", "fwd[", "bwd[", "opt[")))


def digest(text):
    return hashlib.sha256(text.encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------------------ the matrix of DESIGN.md
class _HostLovaszSize(object):
    """The library with the lovasz_loss sort-workspace query answered on the host (the library sizes it on a device; the launch
    records hold the number, nothing else depends on it)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def stp_lovasz_workspace_bytes(self, count, images):
        return 64 * int(count) + 4096 * int(images)


def _plan(net, backbone, size, batch, dtype, training=True, frozen=False, in_ch=3, dynamic_loss_scale=False, **kw):
    def build():
        from segmentation_training_pipeline_amd import graph, nets
        plan = graph.Plan(batch, dtype, "cpu", training=training)
        if len(kw.get("loss", ())) > 5 and kw["loss"][5]:
            plan.lib = _HostLovaszSize(plan.lib)
        if dtype == "fp16":
            plan.loss_scale = 16384.0
        if dynamic_loss_scale:      # the device record backend.HipSegModel gives an fp16 plan: stp_scale_by_device follows the loss
            plan.dls = torch.zeros(8, dtype=torch.float32)
        if frozen:
            plan.frozen_prefixes = nets.ENCODER_PREFIXES
        classes = kw.get("classes", 1)

        def fn(p):
            logits = nets.NETWORKS[net](p, backbone, size, size, in_ch, with_loss=training, **kw)
            if not training and net != "DeepLabV3":
                (p.sigmoid_out if classes == 1 or kw.get("multilabel") else p.softmax_out)(logits)
        return plan.define(fn)
    return build


PLANS = {
    # the four benchmarked shapes at their size, batch and dtype
    "unet_r34_512_b16_bf16": _plan("Unet", "resnet34", 512, 16, "bf16"),
    "linknet_r34_512_b16_bf16": _plan("Linknet", "resnet34", 512, 16, "bf16"),
    "fpn_r50_1024_b4_fp16": _plan("FPN", "resnet50", 1024, 4, "fp16", classes=3),
    "pspnet_r101_768_b8_bf16": _plan("PSPNet", "resnet101", 768, 8, "bf16", classes=20),
    # small ones
    "unet_r18_64_fp32_frozen": _plan("Unet", "resnet18", 64, 2, "fp32", frozen=True),
    "unet_r18_64_fp16": _plan("Unet", "resnet18", 64, 2, "fp16"),
    "linknet_r18_128_transpose_bf16": _plan("Linknet", "resnet18", 128, 2, "bf16", decoder_block_type="transpose"),
    "unet_r34_128_transpose_bf16": _plan("Unet", "resnet34", 128, 2, "bf16", decoder_block_type="transpose"),
    "unet_vgg16_64_bf16": _plan("Unet", "vgg16", 64, 2, "bf16"),
    "fpn_vgg16_128_bf16": _plan("FPN", "vgg16", 128, 2, "bf16", classes=4),
    "deeplab_mobilenetv2_96_bf16": _plan("DeepLabV3", "mobilenetv2", 96, 2, "bf16", classes=3),
    "deeplab_xception_96_bf16": _plan("DeepLabV3", "xception", 96, 2, "bf16"),
    "unet_seresnet34_128_bf16": _plan("Unet", "seresnet34", 128, 2, "bf16"),
    "unet_r18_64_multilabel3_bf16": _plan("Unet", "resnet18", 64, 2, "bf16", classes=3, multilabel=True),
    "unet_r18_64_5ch_bf16": _plan("Unet", "resnet18", 64, 2, "bf16", in_ch=5),
    "unet_r34_256_inference_bf16": _plan("Unet", "resnet34", 256, 2, "bf16", training=False),
    "fpn_r50_256_fp16": _plan("FPN", "resnet50", 256, 4, "fp16", classes=3),
    "pspnet_r50_192_bf16": _plan("PSPNet", "resnet50", 192, 2, "bf16", classes=20),
    # the loss heads no cell above reaches: the extended (iou / jaccard / focal) terms and lovasz_loss
    "unet_r18_64_sigmoid_ex_bf16": _plan("Unet", "resnet18", 64, 2, "bf16", loss=(1.0, 0.5, 0.25, 0.125, 0.0625)),
    "unet_r18_64_lovasz_bf16": _plan("Unet", "resnet18", 64, 2, "bf16", loss=(1.0, 1.0, 0.0, 0.0, 0.0, 0.5)),
    "unet_r18_64_softmax3_ex_bf16": _plan("Unet", "resnet18", 64, 2, "bf16", classes=3, loss=(1.0, 0.5, 0.25, 0.125, 0.0625)),
    "unet_r18_64_sigmoid_ex_fp16_dls": _plan("Unet", "resnet18", 64, 2, "fp16", loss=(1.0, 0.5, 0.25, 0.125, 0.0625), dynamic_loss_scale=True),
}

SWITCHES = [None, ("STP_HALO", "0"), ("STP_S2D", "0"), ("STP_SCATTER_1X1S2", "0"), ("STP_UPCOLLAPSE", "0"), ("STP_UPCOLLAPSE_BWD", "1"),
            ("STP_HALO_FOLD_UP", "0"), ("STP_FUSE_UP_BN", "0"), ("STP_FOLD_UPSAMPLE_GRAD", "0"), ("STP_FUSE_BN_BACKWARD", "0"),
            ("STP_FUSE_BN_BACKWARD_LAST", "0"), ("STP_FUSE_BN_SC", "0"), ("STP_FUSE_BN_HALO", "1"), ("STP_BN_SLOTS", "1"),
            ("STP_BN_FUSE_FINALIZE", "0"), ("STP_WGRAD_GROUP_GFLOP", "0"), ("STP_WGRAD_LONE_GROUP_GFLOP", "0"), ("STP_WGRAD_REDUCE_BATCH", "4"),
            ("STP_FUSE_POOL_BN", "1")]


def cell_name(plan, switch):
    return "%s@%s" % (plan, "default" if switch is None else "%s=%s" % switch)


def run_cell(plan, switch):
    """(canonical text or the error a cell raises, as text)."""
    saved = {k: os.environ.pop(k) for k, _ in SWITCHES[1:] if k in os.environ}
    try:
        if switch is not None:
            os.environ[switch[0]] = switch[1]
        try:
            return dump(PLANS[plan]())
        except Exception as e:           # a cell that raises must raise the same error on both sides of a comparison
            return "raised %s: %s\n" % (type(e).__name__, e)
    finally:
        if switch is not None:
            os.environ.pop(switch[0], None)
        os.environ.update(saved)


def main(argv):
    out_dir, only = argv[0], set(argv[1:])
    os.makedirs(out_dir, exist_ok=True)
    for plan in PLANS:
        if only and plan not in only:
            continue
        for switch in SWITCHES:
            text = run_cell(plan, switch)
            name = cell_name(plan, switch)
            with open(os.path.join(out_dir, name + ".txt"), "w") as f:
                f.write(text)
            print("%s  %d  %s" % (name, records(text), digest(text)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
