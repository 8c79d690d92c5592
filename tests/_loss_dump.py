"""Outputs of every loss entry point on seeded inputs, as files (helper in the style of tests/_plan_dump.py; not collected): the
scalars, the gradient tensor and the bias gradient (where one exists) of the seven launches of ``Plan.LOSS_LAUNCHES`` plus
``stp_softmax_cce_dice_up``, ``stp_sigmoid_loss_bias_grad`` and ``stp_sigmoid_multilabel_bias_grad``, the masked softmax loss
(``stp_softmax_loss_masked``) and the counts of ``stp_class_confusion`` / ``stp_class_confusion_ignore``, in fp32, bf16 and fp16.  The
loss kernels promise a fixed order of additions, so two builds of the library that compute the same thing give the same BYTES: run

    python tests/_loss_dump.py OUT_A
    STP_LIB=<other>/libstp_hip.so STP_LIB_F16=<other>/libstp_hip_f16.so python tests/_loss_dump.py OUT_B

on one GPU and ``diff -r OUT_A OUT_B``.  Only ``_lib`` / ``ops`` are used, so the script runs against any build with the same C ABI.

The sizes are the smallest that reach every path of the shared reduction (csrc/loss_reduce.h):
    1                  the smallest input
    255                fewer than one workgroup
    4097               the tail
    8 x 1024 x 3       (one-class sigmoid families) the 16-byte value-pass path of 16-bit logits
    50 x 1024 + 5      50 value workgroups: the four-in-flight loop of the 16-wide finalize, with a remainder
    230 x 1024 + 77    230 value workgroups: the eight-in-flight loop of the 8-wide finalize, with a remainder
    1 100 000          more than 4096 x 256 work items: a second trip of the capped gradient grid
Softmax families: 3 classes at every size, 5 / 20 / 32 at two; multi-label: 3 at every size, 8 at two.

``python tests/_loss_dump.py --time`` (under the same two variables) prints instead the median time per call of
``stp_softmax_loss_ex``, ``stp_softmax_loss_masked``, ``stp_class_confusion`` and ``stp_class_confusion_ignore``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from segmentation_training_pipeline_amd import _lib, ops  # noqa: E402

SIZES = (1, 255, 4097, 50 * 1024 + 5, 230 * 1024 + 77, 1100000)
SIZE_VEC16 = 8 * 1024 * 3
SIZES_MORE_CLASSES = (4097, 50 * 1024 + 5)
W5 = (1.0, 0.5, 0.25, 0.125, 0.0625)
W5_FIRST_TWO = (1.0, 0.5, 0.0, 0.0, 0.0)
DTYPES = (("fp32", "bf16", torch.float32), ("bf16", "bf16", torch.bfloat16), ("fp16", "fp16", torch.float16))
DEV = "cuda"


def _np(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16).numpy() if t.element_size() == 2 else t.numpy()


class Dump(object):
    def __init__(self, out_dir):
        self.out_dir, self.count = out_dir, 0
        self.ws = torch.zeros(ops.loss_workspace_bytes() // 4, dtype=torch.float32, device=DEV)

    def save(self, case, **tensors):
        for k, t in tensors.items():
            if t is not None:
                np.save(os.path.join(self.out_dir, "%s.%s.npy" % (case, k)), _np(t))
                self.count += 1

    def call(self, name, *args):
        _lib.call(name, *args, ops.stream())
        torch.cuda.synchronize()


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _logits(seed, rows, cols, dtype):
    return (torch.randn(rows, cols, generator=_gen(seed)) * 3.0).to(dtype).to(DEV)


def _padded(classes, dtype):
    v = 16 // torch.empty(0, dtype=dtype).element_size()
    return (classes + v - 1) // v * v


def _weights(w5):
    import ctypes as C
    arr = (C.c_float * 5)(*w5)
    return arr, C.addressof(arr)


def sigmoid_families(d, tag, dtype):
    for n in SIZES + (SIZE_VEC16,):
        z = _logits(n, n, 1, dtype)
        y = (torch.rand(n, generator=_gen(n + 1)) < 0.3).to(torch.uint8).to(DEV)
        p = torch.sigmoid(z.float().cpu()).to(dtype).to(DEV)
        dlc = _padded(1, dtype)
        variants = [("w2", None, dlc)] + [("w5", W5, dlc)] + ([("w5first2", W5_FIRST_TWO, dlc), ("w5narrow", W5, 3)] if n == 4097 else [])
        for vname, w5, ch in variants:
            s = torch.zeros(16, dtype=torch.float32, device=DEV)
            dl = torch.zeros(n, ch, dtype=dtype, device=DEV)
            db = torch.zeros(1, dtype=torch.float32, device=DEV)
            if w5 is None:
                d.call("stp_sigmoid_bce_dice", z.data_ptr(), y.data_ptr(), n, ops.dt(z), 1.0, 0.5, s.data_ptr(), dl.data_ptr(), ch, 2.0,
                       d.ws.data_ptr(), d.ws.numel() * 4)
                name = "sigmoid_bce_dice"
            else:
                keep, addr = _weights(w5)
                d.call("stp_sigmoid_loss_ex", z.data_ptr(), y.data_ptr(), n, ops.dt(z), addr, s.data_ptr(), dl.data_ptr(), ch, 2.0,
                       d.ws.data_ptr(), d.ws.numel() * 4)
                name = "sigmoid_loss_ex"
            d.call("stp_sigmoid_loss_bias_grad", d.ws.data_ptr(), n, db.data_ptr(), 0)
            d.save("%s.%s.%d.%s" % (name, tag, n, vname), scalars=s, grad=dl, bias=db)
        s = torch.zeros(16, dtype=torch.float32, device=DEV)
        dp = torch.zeros(n, dlc, dtype=dtype, device=DEV)
        d.call("stp_prob_bce_dice", p.data_ptr(), y.data_ptr(), n, ops.dt(p), 1.0, 0.5, s.data_ptr(), dp.data_ptr(), dlc, d.ws.data_ptr(),
               d.ws.numel() * 4)
        d.save("prob_bce_dice.%s.%d" % (tag, n), scalars=s, grad=dp)


def class_families(d, tag, dtype):
    for classes, sizes in ((3, SIZES), (5, SIZES_MORE_CLASSES), (20, SIZES_MORE_CLASSES), (32, SIZES_MORE_CLASSES)):
        for n in sizes:
            z = _logits(n + classes, n, classes, dtype)
            t = torch.randint(0, classes, (n,), generator=_gen(n + 7), dtype=torch.int64).to(torch.uint8).to(DEV)
            p = torch.softmax(z.float().cpu(), dim=1).to(dtype).to(DEV)
            dlc = _padded(classes, dtype)
            for vname, w5, ch in [("w2", None, dlc), ("w5", W5, dlc)] + ([("w5first2", W5_FIRST_TWO, dlc), ("w5narrow", W5, classes + 1),
                                                                          ("w2narrow", None, classes + 1)] if n == 4097 else []):
                s = torch.zeros(16, dtype=torch.float32, device=DEV)
                dl = torch.zeros(n, ch, dtype=dtype, device=DEV)
                if w5 is None:
                    d.call("stp_softmax_cce_dice", z.data_ptr(), t.data_ptr(), n, classes, classes, ops.dt(z), 1.0, 0.5, s.data_ptr(),
                           dl.data_ptr(), ch, 2.0, d.ws.data_ptr(), d.ws.numel() * 4)
                    name = "softmax_cce_dice"
                else:
                    keep, addr = _weights(w5)
                    d.call("stp_softmax_loss_ex", z.data_ptr(), t.data_ptr(), n, classes, classes, ops.dt(z), addr, s.data_ptr(), dl.data_ptr(),
                           ch, 2.0, d.ws.data_ptr(), d.ws.numel() * 4)
                    name = "softmax_loss_ex"
                d.save("%s.%s.c%d.%d.%s" % (name, tag, classes, n, vname), scalars=s, grad=dl)
            s = torch.zeros(16, dtype=torch.float32, device=DEV)
            dp = torch.zeros(n, dlc, dtype=dtype, device=DEV)
            d.call("stp_prob_cce_dice", p.data_ptr(), t.data_ptr(), n, classes, classes, ops.dt(p), 1.0, 0.5, s.data_ptr(), dp.data_ptr(), dlc,
                   d.ws.data_ptr(), d.ws.numel() * 4)
            d.save("prob_cce_dice.%s.c%d.%d" % (tag, classes, n), scalars=s, grad=dp)


def multilabel_family(d, tag, dtype):
    for classes, sizes in ((3, SIZES), (8, SIZES_MORE_CLASSES)):
        for n in sizes:
            z = _logits(n + 31 * classes, n, classes, dtype)
            bits = torch.randint(0, 1 << classes, (n,), generator=_gen(n + 9), dtype=torch.int64).to(torch.uint8).to(DEV)
            dlc = _padded(classes, dtype)
            for vname, w5, ch in [("w5", W5, dlc)] + ([("w5first2", W5_FIRST_TWO, dlc), ("w5narrow", W5, classes + 1)] if n == 4097 else []):
                s = torch.zeros(16, dtype=torch.float32, device=DEV)
                dl = torch.zeros(n, ch, dtype=dtype, device=DEV)
                db = torch.zeros(8, dtype=torch.float32, device=DEV)
                keep, addr = _weights(w5)
                d.call("stp_sigmoid_multilabel_loss", z.data_ptr(), bits.data_ptr(), n, classes, classes, ops.dt(z), addr, s.data_ptr(),
                       dl.data_ptr(), ch, 2.0, d.ws.data_ptr(), d.ws.numel() * 4)
                d.call("stp_sigmoid_multilabel_bias_grad", d.ws.data_ptr(), n, classes, db.data_ptr(), 0)
                d.save("sigmoid_multilabel_loss.%s.c%d.%d.%s" % (tag, classes, n, vname), scalars=s, grad=dl, bias=db)


def up_family(d, tag, dtype):
    N, H, W = 2, 24, 24
    lib = _lib.load()
    for classes in (3, 20):
        for f in (2, 8):
            if not lib.stp_softmax_cce_dice_up_ok(f, classes, ops.dt(torch.empty(0, dtype=dtype))):
                raise _lib.StpError("stp_softmax_cce_dice_up is switched off")
            low = _logits(100 * classes + f, N * H * W, classes, dtype)
            t = torch.randint(0, classes, (N * H * f * W * f,), generator=_gen(f + classes), dtype=torch.int64).to(torch.uint8).to(DEV)
            dlc = _padded(classes, dtype)
            nb = int(lib.stp_softmax_cce_dice_up_corner_bytes(N, H, W, classes))
            corners = torch.zeros(nb // 4, dtype=torch.float32, device=DEV)
            for vname, scale in (("plain", None), ("devscale", torch.tensor([4.0], dtype=torch.float32, device=DEV))):
                s = torch.zeros(16, dtype=torch.float32, device=DEV)
                dlow = torch.zeros(N * H * W, dlc, dtype=dtype, device=DEV)
                rec = torch.zeros(1, dtype=torch.float32, device=DEV) if scale is not None else None
                d.call("stp_softmax_cce_dice_up", low.data_ptr(), t.data_ptr(), N, H, W, f, classes, classes, ops.dt(low), 1.0, 0.5, s.data_ptr(),
                       dlow.data_ptr(), dlc, 2.0, ops.ptr(scale), ops.ptr(rec), d.ws.data_ptr(), d.ws.numel() * 4, corners.data_ptr(), nb)
                d.save("softmax_cce_dice_up.%s.c%d.f%d.%s" % (tag, classes, f, vname), scalars=s, grad=dlow, record=rec)


def _ignored(t, n, seed):
    """``t`` with 255 in a seeded 30 % of its pixels"""
    return torch.where((torch.rand(n, generator=_gen(seed)) < 0.3).to(DEV), torch.full_like(t, 255), t)


def masked_family(d, tag, dtype):
    """stp_softmax_loss_masked: the sizes and classes of class_families; ignore label 255 / none (-1) x spread class weights / NULL,
    and every pixel ignored at 4097"""
    for classes, sizes in ((3, SIZES), (5, SIZES_MORE_CLASSES), (20, SIZES_MORE_CLASSES), (32, SIZES_MORE_CLASSES)):
        spread = (0.5 + 0.25 * torch.arange(classes, dtype=torch.float32)).to(DEV)
        for n in sizes:
            z = _logits(n + classes, n, classes, dtype)
            t = _ignored(torch.randint(0, classes, (n,), generator=_gen(n + 7), dtype=torch.int64).to(torch.uint8).to(DEV), n, n + 11)
            dlc = _padded(classes, dtype)
            cases = [("ign255.cw", t, 255, spread), ("ign255.nocw", t, 255, None), ("noign.cw", t, -1, spread), ("noign.nocw", t, -1, None)]
            if n == 4097:
                cases.append(("allignored.cw", torch.full_like(t, 255), 255, spread))
            for cname, tt, ign, cw in cases:
                for vname, w5 in [("w5", W5)] + ([("w5first2", W5_FIRST_TWO)] if n == 4097 else []):
                    s = torch.zeros(16, dtype=torch.float32, device=DEV)
                    dl = torch.zeros(n, dlc, dtype=dtype, device=DEV)
                    keep, addr = _weights(w5)
                    d.call("stp_softmax_loss_masked", z.data_ptr(), tt.data_ptr(), n, classes, classes, ops.dt(z), addr, s.data_ptr(), dl.data_ptr(),
                           dlc, 2.0, d.ws.data_ptr(), d.ws.numel() * 4, ign, ops.ptr(cw))
                    d.save("softmax_loss_masked.%s.c%d.%d.%s.%s" % (tag, classes, n, cname, vname), scalars=s, grad=dl)


CONF_SIZES = (5 * 1024 + 77, 600000)      # the second: past 512 workgroups x 1024 pixels, a second trip of the capped grid


def _confusion_ws(classes):
    nb = int(_lib.load().stp_class_confusion_workspace_bytes(classes))
    return torch.zeros(nb // 4, dtype=torch.int32, device=DEV), nb


def confusion_family(d, tag, dtype):
    """stp_class_confusion and stp_class_confusion_ignore (label 255, and -1): the int32 counts"""
    for classes in (3, 20, 32):
        ws, nb = _confusion_ws(classes)
        for n in CONF_SIZES:
            rows = _logits(n + 3 * classes, n, classes, dtype)
            targets = (("runs", (torch.arange(n) // 97 % classes).to(torch.uint8).to(DEV)),
                       ("random", torch.randint(0, classes, (n,), generator=_gen(n + 13), dtype=torch.int64).to(torch.uint8).to(DEV)))
            for tname, t in targets:
                t = _ignored(t, n, n + 17)
                for name, tail in (("class_confusion", ()), ("class_confusion_ignore", (255,)), ("class_confusion_ignore", (-1,))):
                    counts = torch.zeros(classes * classes, dtype=torch.int32, device=DEV)
                    d.call("stp_" + name, rows.data_ptr(), t.data_ptr(), n, classes, classes, ops.dt(rows), counts.data_ptr(), ws.data_ptr(), nb, *tail)
                    d.save("%s.%s.c%d.%d.%s%s" % (name, tag, classes, n, tname, "".join(".ign%d" % v for v in tail)), counts=counts)


def time_calls(warmup=10, calls=50):
    """--time: the median device-event time per call of the two extended softmax losses (with gradient, W5) and the two full-resolution
    confusion counts, at sizes a user runs"""
    for tag, storage, dtype, classes, n, ldc in (("bf16", "bf16", torch.bfloat16, 20, 8 * 768 * 768, 24), ("fp16", "fp16", torch.float16, 3, 4 * 1024 * 1024, 8)):
        with _lib.storage(storage):
            z = _logits(classes, n, ldc, dtype)
            t = _ignored(torch.randint(0, classes, (n,), generator=_gen(7), dtype=torch.int64).to(torch.uint8).to(DEV), n, 11)
            cw = (0.5 + 0.25 * torch.arange(classes, dtype=torch.float32)).to(DEV)
            s = torch.zeros(16, dtype=torch.float32, device=DEV)
            dl = torch.zeros(n, ldc, dtype=dtype, device=DEV)
            lws = torch.zeros(ops.loss_workspace_bytes() // 4, dtype=torch.float32, device=DEV)
            counts = torch.zeros(classes * classes, dtype=torch.int32, device=DEV)
            cws, nb = _confusion_ws(classes)
            keep, addr = _weights(W5)
            loss = (z.data_ptr(), t.data_ptr(), n, classes, ldc, ops.dt(z), addr, s.data_ptr(), dl.data_ptr(), ldc, 2.0, lws.data_ptr(), lws.numel() * 4)
            conf = (z.data_ptr(), t.data_ptr(), n, classes, ldc, ops.dt(z), counts.data_ptr(), cws.data_ptr(), nb)
            for name, args in (("stp_softmax_loss_ex", loss), ("stp_softmax_loss_masked", loss + (255, cw.data_ptr())),
                               ("stp_class_confusion", conf), ("stp_class_confusion_ignore", conf + (255,))):
                ms = []
                for k in range(warmup + calls):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _lib.call(name, *args, ops.stream())
                    e1.record()
                    e1.synchronize()
                    if k >= warmup:
                        ms.append(e0.elapsed_time(e1))
                print("time %-28s %s c%d %d px stride %d  median %.1f us  (min %.1f)" % (name, tag, classes, n, ldc, 1e3 * float(np.median(ms)), 1e3 * min(ms)),
                      flush=True)


def main(argv):
    if argv and argv[0] == "--time":
        return time_calls()
    out_dir = argv[0]
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for tag, storage, dtype in DTYPES:
        with _lib.storage(storage):
            d = Dump(out_dir)
            for family in (sigmoid_families, class_families, multilabel_family, up_family, masked_family, confusion_family):
                family(d, tag, dtype)
            total += d.count
            print("%s  %d files" % (tag, d.count), flush=True)
    print("%d files in %s" % (total, out_dir))


if __name__ == "__main__":
    main(sys.argv[1:])
