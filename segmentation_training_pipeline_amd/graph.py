"""Static training/inference plan: the host-side runtime of the HIP hot path.

A network definition (``nets.py``) is executed ONCE against a :class:`Plan`; every layer call
records the C-ABI launches of its forward, pushes a closure for its backward, and declares its
parameters inside flat fp32 arenas (master weights ``P``, gradients ``G``, optimizer state,
BN moving statistics ``S``).  The result is three launch lists - ``prep`` (weight compute
copies), ``fwd`` (+loss), ``bwd`` - plus ``opt``; a step replays them on one HIP stream, eagerly or
as a captured hipGraph.  There is no tracing compiler and no autograd: gradients meet by
plan-time bookkeeping (first writer overwrites, later writers accumulate in the GEMM epilogue).

PyTorch supplies device memory (``torch.empty``), the stream handle and - in ``distributed.py`` -
the RCCL process group; all arithmetic happens in libstp_hip.so.
"""
import os
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib, ops

_TD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


class StpShapeError(ValueError):
    pass


def _rup(a, b):
    return (a + b - 1) // b * b


class DT(object):
    """Device tensor handle: NHWC activation + (optional) gradient buffer."""
    __slots__ = ("name", "N", "H", "W", "C", "buf", "grad", "_grad_ready", "grad_writes", "needs_grad", "gradC", "meta")

    def __init__(self, name, N, H, W, Cn, buf=None, needs_grad=False):
        self.name, self.N, self.H, self.W, self.C = name, N, H, W, Cn
        self.buf, self.grad, self._grad_ready, self.needs_grad = buf, None, False, needs_grad
        self.grad_writes = 0
        self.gradC = Cn
        self.meta = {}

    @property
    def grad_ready(self):
        return self._grad_ready

    @grad_ready.setter
    def grad_ready(self, v):
        """Set by every consumer's backward after it wrote / accumulated its contribution: ``grad_writes`` counts them, so the
        consumer that finds ``grad_writes == uses - 1`` knows it completes the gradient (BatchNormalization-backward fusion)."""
        self._grad_ready = bool(v)
        if v:
            self.grad_writes += 1

    @property
    def rows(self):
        return self.N * self.H * self.W


class ParamInfo(object):
    __slots__ = ("name", "offset", "numel", "shape", "kind", "trainable", "pending_slices")

    def __init__(self, name, offset, shape, kind, trainable):
        self.name, self.offset, self.shape, self.kind, self.trainable = name, offset, tuple(shape), kind, trainable
        self.numel = int(np.prod(shape))
        self.pending_slices = 0       # column ranges of a shared 1x1 kernel whose weight gradient has not been planned yet (Plan.conv param_cols)

    @property
    def end(self):
        """One past the parameter's last element in the arenas."""
        return self.offset + self.numel


class Plan(object):
    def __init__(self, batch, dtype="bf16", device="cuda", training=True, class_metrics=False):
        if dtype not in _TD:
            raise ValueError("dtype must be 'bf16', 'fp16' or 'fp32'")
        self.device = torch.device(device)
        # A plan may be BUILT on CPU tensors (structure/shape checks in the CPU test suite);
        # it can only RUN on the GPU: run() raises otherwise - there is no CPU compute path.
        if self.device.type == "cuda" and not torch.cuda.is_available():
            raise _lib.StpError("the HIP training path needs a GPU; there is no CPU fallback")
        # the 16-bit storage format is a build parameter of the kernel set: fp16 plans run on libstp_hip_f16.so
        self.lib = _lib.load("fp16" if dtype == "fp16" else "bf16")
        self.loss_scale = 1.0          # fp16: the loss gradient is seeded times this; the optimizer's gscale divides it out
        self.dls = None                # fp16: device record of the dynamic multiplier on top of it (backend.HipSegModel, stp_scale_by_device)
        self.N = batch
        self.dtype = dtype
        self.tdt = _TD[dtype]
        self.cdt = {"bf16": ops.BF16, "fp16": ops.F16, "fp32": ops.F32}[dtype]
        self.vec = 4 if dtype == "fp32" else 8
        self.training = training
        self.params = OrderedDict()
        self.states = OrderedDict()
        self._poff = 0
        self._soff = 0
        self.dry = True
        self.frozen_prefixes = ()
        self._keep = []
        self.tensors = OrderedDict()
        self.P = self.G = self.S = None
        self.prep, self.fwd, self.bwd, self.opt = [], [], [], []
        self._tape = []
        self._goffs = []
        self.bwd_marks, self.bwd_monotone = [], True
        self._prep_layers = []
        self._upc_layers = []
        self._upc4_layers = []
        self._wg_ws_bytes = 0
        self._bn_ws_c = 4
        self.bn_momentum = 0.99
        self.fuse_bn_backward = os.environ.get("STP_FUSE_BN_BACKWARD", "1") != "0"
        self.fuse_bn_backward_last = os.environ.get("STP_FUSE_BN_BACKWARD_LAST", "1") != "0"
        self.fold_upsample_grad = os.environ.get("STP_FOLD_UPSAMPLE_GRAD", "1") != "0"
        # grouped weight gradients (stp_wgrad_group_*): the row-of-taps layers of a stage are collected and issued as ONE partial
        # + ONE reduce launch once their work reaches this many GFLOP (0: every layer is launched alone, as in round 2)
        self.wgrad_group_gflop = float(os.environ.get("STP_WGRAD_GROUP_GFLOP", "300"))
        # a LONE row-of-taps layer of the 128-channel class this large runs as a one-layer group on the all-taps kernel (_flush_wgroup):
        # FPN/ResNet50's `fpn_final` (512 -> 512 at 4 x 256 x 256, 1.24 TFLOP) 14.30 -> 14.04 and 14.62 -> 14.49 ms per step on two boxes
        # (profiles/r06e_step_ab.txt); 0 = never
        self.wgrad_lone_group_gflop = float(os.environ.get("STP_WGRAD_LONE_GROUP_GFLOP", "600"))
        # lone weight gradients with plain slabs (the bottleneck ResNets' 1x1 layers, stride-2 layers): their reduces can wait in a table and
        # run as ONE launch per STP_WGRAD_REDUCE_BATCH layers.  OPT-IN (default 0 = one reduce launch per layer): measured SLOWER on the
        # step - FPN/ResNet50 14.62 -> 14.77 ms, PSPNet/ResNet101 8.06 -> 8.07, U-Net/ResNet34 6.350 -> 6.370 (same box, two interleaved
        # repetitions, profiles/r06e_step_ab.txt): the 59 / 30 / 7 launches saved (~9 us each in the eager table, ~3 in the graph) cost less
        # than reading 1 - 16 MB of slabs per layer back from HBM instead of from the cache the partial launch just wrote them through
        self.reduce_batch = int(os.environ.get("STP_WGRAD_REDUCE_BATCH", "0"))
        self._pending_reduces, self._pending_reduce_hi = [], 0
        self._wgroup, self._wgroup_cls, self._wgroup_flops, self._wgroup_hi = [], 0, 0.0, 0
        self._wgroup_reads = set()      # dY buffers of the pending layers: nothing may rewrite them before the group is issued
        self.wgroups = []               # (layer names, class) of every issued group (inspection / tests)
        self._dw_ws_bytes = 0
        self.step_state = None
        # fused BatchNormalization sums in fixed-point slots (stp_conv_params.stats_slots): no finalize kernels
        self.bn_slots = os.environ.get("STP_BN_SLOTS", "0") == "1"   # measured: no gain over the finalize kernels, kept opt-in
        # BatchNormalization whose only consumers are small-channel convolutions: normalised inside their halo staging
        # (stp_conv_params.src_bn_mean), the normalised tensor is never written
        self.fuse_bn_sc = os.environ.get("STP_FUSE_BN_SC", "1") != "0"
        # producer BatchNormalization applied in LDS by the halo kernel (needs its automatic selection: STP_HALO != 0) AND by the
        # weight gradient of the same layer (row-of-taps kernel, single-layer or grouped: conv_wgrad_row.hip's PBN instances): the
        # normalised tensor is never written, the stp_bn_apply launch disappears.  OPT-IN (STP_FUSE_BN_HALO=1): measured slower in
        # round 1 (the weight gradient still read the normalised tensor) and again in round 4 with the grouped weight gradient
        # normalising its operand itself (profiles/r04b_*): 6.99 vs 6.79 ms per step on one box.  The launches it removes cost
        # 178 + 45 us (31 stp_bn_apply / finalize_apply at 7-14 us, near the HBM roofline); the in-LDS transform costs the halo
        # forward +2.5..+6.5 us per launch (stage 1: +16 us: ~28 VALU instructions per 16-byte vector, by all 8 waves, with the MFMA
        # pipe idle) = +220 us, and the grouped weight gradients +140 us (every tile over a pixel range repeats the transform).
        self.fuse_bn_halo = os.environ.get("STP_FUSE_BN_HALO", "0") != "0" and os.environ.get("STP_HALO", "1") != "0"
        self.bn_slots_max_rows = int(os.environ.get("STP_BN_SLOTS_MAXROWS", "1073741824"))
        self._slot_need = 0          # int64 elements, counted in the dry pass
        self._slot_used = 0
        self.slot_arena = None
        self.loss_scalars = None
        # multi-class heads: one confusion launch (stp_class_confusion / _up) directly behind the loss launch writes class_counts,
        # int32 [classes][classes] (target class, predicted class) - categorical_accuracy, mean_iou, iou_class_k.  Off: no launch
        self.class_metrics = bool(class_metrics)
        # the softmax head's ignore label / class weights: {"ignore_label": .., "class_weights": ..} read by softmax_loss (set before
        # define, as loss_scale is), and the device tensor of the weights that launch reads
        self.masked_loss = None
        # the softmax head's lovasz_softmax weight, read by softmax_loss (set before ``define``, as masked_loss is): non-zero adds the
        # stp_lovasz_softmax launch behind the extended loss launch
        self.lovasz_softmax = 0.0
        # the one-class head's U-Net border weight map, read by sigmoid_loss (set before ``define``, as masked_loss is):
        # {"w0", "sigma", "radius", "class_balance"} puts the label launches, stp_border_weight and the weighted loss launch in the place
        # of stp_sigmoid_bce_dice; None: the plan of before
        self.border_weights = None
        self.class_weights = None
        self.class_counts = None
        self.inputs = {}

    # ------------------------------------------------------------------ definition driver
    def define(self, net_fn, share=None):
        """Runs ``net_fn(plan)`` twice: a dry pass that sizes the arenas, then the real pass.
        ``share``: another plan of the same network whose parameter / moving-statistics arenas
        are reused (the inference plan shares the training plan's weights)."""
        self.dry = True
        net_fn(self)
        n = _rup(self._poff, 4)
        if share is not None:
            if [(k, v.offset, v.shape) for k, v in share.params.items()] != [(k, v.offset, v.shape) for k, v in self.params.items()] \
                    or list(share.states.items()) != list(self.states.items()):
                raise StpShapeError("plans that share weights must declare identical parameters")
            self.P, self.S, self.G = share.P, share.S, None
        else:
            self.P = torch.zeros(n, dtype=torch.float32, device=self.device)
            self.G = torch.zeros(n, dtype=torch.float32, device=self.device) if self.training else None
            self.S = torch.zeros(max(_rup(self._soff, 4), 4), dtype=torch.float32, device=self.device)
        self.mask = torch.ones(n, dtype=torch.uint8, device=self.device)
        self.ws_wgrad = torch.empty(max(self._wg_ws_bytes // 4, 4) + 4, dtype=torch.float32, device=self.device)
        self.ws_bn = torch.empty(ops.bn_workspace_bytes(_rup(self._bn_ws_c, 4)) // 4, dtype=torch.float32, device=self.device)
        self.ws_loss = torch.empty(ops.loss_workspace_bytes() // 4, dtype=torch.float32, device=self.device)
        self.ws_dw = torch.empty(max(self._dw_ws_bytes // 4, 4), dtype=torch.float32, device=self.device)
        if self.training and self.bn_slots and self._slot_need:
            self.slot_arena = torch.zeros(_rup(self._slot_need, 2), dtype=torch.int64, device=self.device)
        self.dry = False
        self._tape = []
        self._prep_layers = []
        self._upc_layers = []
        self._upc4_layers = []
        self.tensors = OrderedDict()
        net_fn(self)
        self._fuse_bn_finalize(self._fuse_bn_into_consumers())
        self._finish_prep()
        if self.training:
            # bwd_marks[i] = (launches issued after the i-th backward closure, lowest gradient offset written so far):
            # gradients at or above that offset are final from that launch on, PROVIDED layers finish in descending
            # arena order (true when parameters are declared in call order); otherwise bwd_monotone is cleared and
            # the reducer falls back to one all-reduce after the whole backward
            self.bwd_marks, self.bwd_monotone = [], True
            low = self.G.numel() if self.G is not None else 0
            for back in reversed(self._tape):
                self._goffs = []
                back()
                if self._goffs:
                    if max(e for _, e in self._goffs) > low:
                        self.bwd_monotone = False
                    low = min(low, min(o for o, _ in self._goffs))
                # a pending grouped weight gradient has asked for its addresses but not been launched: the arena is final only
                # above the highest pending layer
                # (... and below the highest layer whose reduce waits in the batched table)
                self.bwd_marks.append((len(self.bwd), max(low, self._wgroup_hi, self._pending_reduce_hi)))
            if self._wgroup or self._pending_reduces:
                self._flush_wgroup()
                self._flush_reduces()
                self.bwd_marks.append((len(self.bwd), low))
        self._tape = []
        return self

    @staticmethod
    def _nslots(Cn):
        """Slots per channel: as many as keep 2 * C * slots int64 reads in the consumer's prologue small (<= 16)."""
        n = 16
        while n > 1 and n * Cn > 1024:
            n //= 2
        return n

    def _slots(self, Cn):
        """(device pointer, slots per channel) of a zero-initialised [2][Cn][n] slice of the slot arena."""
        n = self._nslots(Cn)
        off = self._slot_used
        self._slot_used += 2 * Cn * n
        if self._slot_used > self.slot_arena.numel():
            raise StpShapeError("slot arena exhausted")
        return self.slot_arena.data_ptr() + 8 * off, n

    def _table(self, raw):
        """A descriptor table built on the host, as a device tensor the plan keeps."""
        dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(self.device)
        self._keep.append(dev)
        return dev

    def _finish_prep(self):
        """One batched weight-preparation launch for all conv layers (descriptor table lives on the device)."""
        if self.slot_arena is not None:
            self._emit(self.prep, "stp_zero_bytes", self.slot_arena.data_ptr(), self.slot_arena.numel() * 8)
        n = len(self._prep_layers)
        if not n:
            return
        dsz = int(self.lib.stp_weight_prepare_desc_bytes())
        host = (C.c_char * (dsz * n))()
        total = 0
        for i, lay in enumerate(self._prep_layers):
            total += int(self.lib.stp_weight_prepare_desc_fill(C.cast(host, C.c_void_p), i, total, *lay))
        dev = self._table(bytes(host))
        self._emit(self.prep, "stp_weight_prepare_batched", dev.data_ptr(), n, total, self.cdt)
        if self._upc_layers:      # class-collapsed weight copies of the convolutions over upsample + concat (Plan.conv)
            import struct
            assert int(self.lib.stp_weight_prepare_upcollapse_desc_bytes()) == 32
            tab = b"".join(struct.pack("<QQiiii", *lay) for lay in self._upc_layers)
            udev = self._table(tab)
            self._emit(self.prep, "stp_weight_prepare_upcollapse_batched", udev.data_ptr(), len(self._upc_layers), self.cdt)
            if self._upc4_layers:
                tab4 = b"".join(struct.pack("<QQiiii", *lay) for lay in self._upc4_layers)
                udev4 = self._table(tab4)
                self._emit(self.prep, "stp_weight_prepare_upcollapse_bwd_batched", udev4.data_ptr(), len(self._upc4_layers), self.cdt)

    # ------------------------------------------------------------------ parameters / state
    def param(self, name, shape, kind="weight"):
        if self.dry and name in self.params and tuple(self.params[name].shape) == tuple(shape) and self.params[name].kind == kind:
            return self.params[name]          # (a parameter several launches read: the column ranges of a shared 1x1 kernel, Plan.conv param_cols)
        if self.dry:
            off = _rup(self._poff, 4)
            trainable = not any(name.startswith(p) for p in self.frozen_prefixes)
            self.params[name] = ParamInfo(name, off, shape, kind, trainable)
            self._poff = off + int(np.prod(shape))
        return self.params[name]

    def state(self, name, numel, init=0.0):
        if self.dry:
            off = _rup(self._soff, 4)
            self.states[name] = (off, numel, init)
            self._soff = off + numel
        return self.states[name][0]

    def _pptr(self, info):
        return self.P.data_ptr() + 4 * info.offset

    def _gptr(self, info):
        # the backward closures ask for gradient addresses in backward order: the running minimum tells the
        # data-parallel reducer which tail of the arena is final after each layer (bwd_marks)
        self._goffs.append((info.offset, info.end))
        return self.G.data_ptr() + 4 * info.offset

    def _sptr(self, off):
        return self.S.data_ptr() + 4 * off

    # ------------------------------------------------------------------ buffers / launches
    def _alloc(self, shape, dtype=None):
        t = torch.empty(shape, dtype=dtype or self.tdt, device=self.device)
        self._keep.append(t)
        return t

    def _new(self, name, H, W, Cn, needs_grad, dtype=None):
        t = DT(name, self.N, H, W, Cn, None if self.dry else self._alloc((self.N, H, W, Cn), dtype), needs_grad)
        self.tensors[name] = t
        return t

    def _gradbuf(self, t):
        """Gradient buffer of ``t`` for a kernel that is about to WRITE it (a dY aliased as a residual gradient may still be
        the operand of a pending grouped weight gradient: _guard_write)."""
        if t.grad is None:
            t.grad = self._alloc((t.N, t.H, t.W, t.gradC))
        self._guard_write(t.grad)
        return t.grad

    def _guard_write(self, buf):
        """The hazard rule for a kernel about to write ``buf`` (None: nothing to write) - a gradient buffer _gradbuf hands out, or a dY
        that stp_relu_bwd masks in place: a pending grouped weight gradient that still reads it as its dY is issued first."""
        if buf is not None and self._wgroup_reads and buf.data_ptr() in self._wgroup_reads:
            self._flush_wgroup()

    @staticmethod
    def _use(*ts):
        """Counts the consumers of a tensor: a BatchNormalization output read by exactly one convolution gets its
        backward partial sums from that convolution's data-gradient epilogue (stp_conv_params.bnb_x)."""
        for t in ts:
            if t is not None:
                t.meta["uses"] = t.meta.get("uses", 0) + 1

    # Does a launch that writes (`acc`: accumulates) its share of t's gradient complete it, so that its epilogue or pass can mask it and
    # reduce the BatchNormalization-backward sums?  Yes for the only consumer, or the LAST of several (every other consumer has already
    # written or accumulated its share, this one accumulates on top: STP_FUSE_BN_BACKWARD_LAST).  `promoted`: the launch carries a
    # sibling consumer's share too, so two consumers count as one.  `last_ok`: the launch may be the accumulating last one.
    def _completes_grad(self, t, acc, promoted=False, last_ok=True):
        uses = t.meta.get("uses", 0)
        sole = (uses == 1 or (promoted and uses == 2 and t.grad_writes == 1)) and not acc
        return bool(sole or (last_ok and self.fuse_bn_backward_last and uses > 1 and t.grad_writes == uses - 1 and acc))

    # A pass `fname` that writes (accumulates) its share of t's gradient: where that completes the gradient of a BatchNormalization output
    # (and `enabled`), the pass's `_bn` form masks it and reduces the backward sums on the way (meta["bnb"] = their table and its columns)
    def _emit_grad_pass(self, fname, t, acc, tile_args, args, enabled=True):
        bnm = t.meta.get("bn")
        ntl = int(getattr(self.lib, fname + "_bn_tiles")(*tile_args)) if (
            self.fuse_bn_backward and bnm is not None and self._completes_grad(t, acc) and self.slot_arena is None and enabled) else 0
        if ntl > 0:
            st = self._alloc((2 * t.C * ntl,), torch.float32)
            self._emit(self.bwd, fname + "_bn", *args, *bnm, st.data_ptr())
            t.meta["bnb"] = (st, ntl)
        else:
            self._emit(self.bwd, fname, *args)

    # a launch record is (C function, args without the trailing stream, entry-point name, meta);
    # meta carries the layer name and the ALGORITHMIC flops of GEMM launches for bench.py's roofline.
    def _emit(self, lst, fname, *args):
        lst.append((getattr(self.lib, fname), args, fname, None))

    # meta["bn"] of a BatchNormalization output = (pre-normalisation tensor, mean, rstd, gamma, beta, activation)
    @staticmethod
    def _set_src_bn(p, bn):
        """The producer BatchNormalization ``bn`` as the src_bn_* operands of a ConvParams / WgradParams."""
        p.src_bn_mean, p.src_bn_rstd, p.src_bn_gamma, p.src_bn_beta, p.src_bn_relu = bn[1:]

    @staticmethod
    def _set_bnb(q, bn):
        """The BatchNormalization ``bn`` whose output gradient the data gradient ``q`` completes, as its bnb_* operands; None clears them."""
        q.bnb_x, q.bnb_mean, q.bnb_rstd, q.bnb_gamma, q.bnb_beta, q.bnb_relu = bn or (None, None, None, None, None, 0)

    def _fuse_bn_into_consumers(self):
        """BatchNormalization(+activation) outputs that only convolutions with a fused-producer path read:

        * every consumer is a small-channel convolution (conv_sc.hip / conv_sc_wgrad.hip: forward AND weight gradient normalise the pre-BN tensor
          while staging it): the stp_bn_apply launch is dropped; ``tensor(name)`` still materialises the tensor on demand;
        * some consumers are halo-kernel convolutions (conv_halo.hip: the forward normalises the slab in LDS): when every one of
          their weight gradients runs on the row-of-taps kernel (conv_wgrad_row.hip normalises its halo tile the same way) the launch
          is dropped as well; otherwise a weight gradient still reads the normalised tensor and the stp_bn_apply launch stays, a
          launch of its own (returned: the ids of these records, which _fuse_bn_finalize leaves alone).

        The data gradient and the BatchNormalization backward never read the normalised tensor."""
        drop, kept = set(), set()
        for t in self.tensors.values():
            rec, sc, halo = t.meta.get("apply_rec"), t.meta.get("sc_consumers") or [], t.meta.get("halo_consumers") or []
            if rec is None or not (sc or halo) or len(sc) + len(halo) != t.meta.get("uses", 0):
                continue
            bn = t.meta["bn"]
            halo_full = bool(halo) and all(ok for _, _, ok in halo)      # every weight gradient fuses the BatchNormalization too
            for cp, wp in sc + [h[:2] for h in halo]:
                cp.src0 = bn[0]
                self._set_src_bn(cp, bn)
                # (with a halo consumer whose weight gradient cannot normalise its operand the normalised tensor exists anyway: all read it)
                if not halo or halo_full:
                    self._set_src_bn(wp, bn)
            if halo and not halo_full:
                kept.add(id(rec))
            else:
                t.meta["deferred"] = rec
                t.meta["src_override"] = bn[0]
                drop.add(id(rec))
        self.fwd = [r for r in self.fwd if id(r) not in drop]
        return kept

    def _fuse_bn_finalize(self, keep=()):
        """stp_bn_finalize directly followed by the stp_bn_apply of the same BatchNormalization -> ONE stp_bn_finalize_apply launch where
        the library takes it (16-bit dtype, whole 64-channel slabs, <= 128 partial-sum columns): the apply pass reduces the partial
        sums of its own channel slab in its prologue, the single-workgroup-per-channel finalize launch (~5 us of latency on the
        critical chain conv -> finalize -> apply -> conv) disappears.  The backward pair is merged inside stp_bn_backward_fused(_add).
        ``keep``: ids of stp_bn_apply records that stay launches of their own (_fuse_bn_into_consumers)."""
        if os.environ.get("STP_BN_FUSE_FINALIZE", "1") == "0":
            return
        out, i, fwd = [], 0, self.fwd
        while i < len(fwd):
            r = fwd[i]
            nxt = fwd[i + 1] if i + 1 < len(fwd) else None
            if (r[2] == "stp_bn_finalize" and nxt is not None and nxt[2] == "stp_bn_apply" and id(nxt) not in keep
                    and nxt[1][7] == r[1][6] and nxt[1][8] == r[1][7] and nxt[1][1] == nxt[1][3] == self.cdt and nxt[1][5] == nxt[1][6] == r[1][3]
                    and nxt[1][12] == 0.0):
                part, tiles, rows, Cn, eps, mom, mean, rstd, mm, mv = r[1]
                x, _, y, _, rows2, _, _, _, _, gp, beta, relu, _ = nxt[1]
                if rows2 == rows and int(self.lib.stp_bn_finalize_apply_ok(self.cdt, rows, Cn, tiles)):
                    out.append((self.lib.stp_bn_finalize_apply, (part, tiles, x, y, self.cdt, rows, Cn, eps, mom, mean, rstd, mm, mv, gp, beta, relu),
                                "stp_bn_finalize_apply", None))
                    i += 2
                    continue
            out.append(r)
            i += 1
        self.fwd = out

    def tensor(self, name):
        """The named tensor with its buffer valid: a normalised tensor that only exists inside its consumers' staging is
        computed here with the launch the plan dropped (inspection / tests; not part of the step)."""
        t = self.tensors[name]
        rec = t.meta.get("deferred")
        if rec is not None:
            fn, args = rec[0], rec[1]
            rc = fn(*args, torch.cuda.current_stream().cuda_stream)
            if rc != 0:
                raise _lib.StpError("%s failed with %d" % (rec[2], rc))
        return t

    def _scratch(self, nbytes):
        """(pointer, bytes) of a plan-time fp32 scratch buffer for a two-stage reduction; (None, 0) if the op needs none."""
        nbytes = int(nbytes)
        if nbytes <= 0:
            return None, 0
        buf = self._alloc((nbytes // 4,), torch.float32)
        return buf.data_ptr(), nbytes

    def _group_stats(self, p, st, Cs):
        """Group-level pre-reduction of a convolution's statistic columns (stp_conv_params.stats_group): where the kernel that serves
        ``p`` has the epilogue and its table has more than 128 columns, the launch also writes a [2][Cs][columns / G] table that the
        one-launch finalize + apply kernels take - returns (the table a BatchNormalization should read, its columns)."""
        cols = int(self.lib.stp_conv2d_stats_floats(C.byref(p))) // (2 * Cs)
        G = int(self.lib.stp_conv2d_stats_group_for(C.byref(p)))
        if G < 2:
            return st, cols
        ng = -(-cols // G)
        out = self._alloc((2 * Cs * ng,), torch.float32)
        cnt = torch.zeros((max(1, int(self.lib.stp_conv2d_stats_group_counters(C.byref(p), G))),), dtype=torch.int32, device=self.device)
        self._keep.append(cnt)
        p.stats_group_out, p.stats_group_counters, p.stats_group = out.data_ptr(), cnt.data_ptr(), G
        return out, ng

    def _emit_conv(self, lst, p, meta=None):
        self._keep.append(p)
        if meta is not None and meta.get("tile") == 512:
            meta = dict(meta, sc=(int(p.C0), 1 if p.Cout <= 16 else 2))    # the small-channel kernel's instance <Cin, 16-channel tiles> (bench.py)
        if meta is not None and meta.get("tile") == 800:
            meta = dict(meta, pw=(int(p.C0), int(p.Cout)))                  # the pointwise streaming kernel's instance <Cin, Cout, ...> (bench.py)
        lst.append((self.lib.stp_conv2d, (C.byref(p),), "stp_conv2d", meta))

    def _emit_wgrad(self, p, name, flops, defer_hi=0):
        """The weight gradient of ONE layer: split partial sums + fixed-order reduce, two launch records so that each kernel can be
        timed on its own (bench.py) - same arithmetic as stp_conv2d_wgrad.
        ``defer_hi`` > 0 (the end of the layer's range in the gradient arena; only when nothing reads dW before the optimizer): a layer
        with plain slabs writes them into a workspace of its own and its reduce joins the pending table (_flush_reduces)."""
        lst = self.bwd
        self._keep.append(p)
        meta = {"layer": name, "pass": "wgrad", "flops": flops, "cout": p.Cout, "sc": bool(self.lib.stp_wgrad_sc_eligible(C.byref(p))),
                "kernel_id": int(self.lib.stp_conv2d_wgrad_kernel_id(C.byref(p)))}
        if defer_hi > 0 and self.reduce_batch > 0:
            db = int(self.lib.stp_wgrad_reduce_desc_bytes())
            wsb = int(self.lib.stp_conv2d_wgrad_workspace_bytes(C.byref(p)))
            ws = self._alloc((max(wsb // 4, 4) + 4,), torch.float32)
            desc = (C.c_char * db)()
            count = int(self.lib.stp_wgrad_reduce_desc_fill(C.addressof(desc), 0, C.byref(p), ws.data_ptr()))
            if count > 0:
                lst.append((self.lib.stp_conv2d_wgrad_partial, (C.byref(p), ws.data_ptr(), ws.numel() * 4, 0), "stp_conv2d_wgrad", meta))
                self._pending_reduces.append((bytes(desc), count))
                self._pending_reduce_hi = max(self._pending_reduce_hi, int(defer_hi))
                if len(self._pending_reduces) >= self.reduce_batch:
                    self._flush_reduces()
                return
            self._keep = [t for t in self._keep if t is not ws]          # (row-of-taps slabs: the layer keeps its own reduce launch)
        lst.append((self.lib.stp_conv2d_wgrad_partial, (C.byref(p), self.ws_wgrad.data_ptr(), self.ws_wgrad.numel() * 4, 0),
                    "stp_conv2d_wgrad", meta))
        lst.append((self.lib.stp_conv2d_wgrad_reduce, (C.byref(p), self.ws_wgrad.data_ptr(), 0), "stp_conv2d_wgrad_reduce", None))

    def _flush_reduces(self):
        """One stp_wgrad_reduce_batched launch for the pending lone-layer reduces (see _emit_wgrad)."""
        if not self._pending_reduces:
            return
        table = b"".join(d for d, _ in self._pending_reduces)
        dev = self._table(table)
        n, maxc = len(self._pending_reduces), max(c for _, c in self._pending_reduces)
        self.bwd.append((self.lib.stp_wgrad_reduce_batched, (dev.data_ptr(), n, maxc), "stp_wgrad_reduce_batched", {"layers": n}))
        self._pending_reduces, self._pending_reduce_hi = [], 0

    def _flush_wgroup(self):
        """Issues the pending grouped weight gradient: descriptor table (built now - every pointer is final), one partial launch
        and one reduce launch.  Each group owns its partial-slab workspace."""
        if not self._wgroup:
            return
        layers, cls = self._wgroup, self._wgroup_cls
        self._wgroup, self._wgroup_cls, self._wgroup_flops, self._wgroup_hi, self._wgroup_reads = [], 0, 0.0, 0, set()
        n = len(layers)
        # (... unless the lone layer is large enough to fill the all-taps kernel by itself: FPN's 512 -> 512 3x3 `fpn_final` at 4 x 256 x 256,
        #  1.24 TFLOP - 1284 us on the per-layer row-of-taps kernel at 963 TFLOP/s; STP_WGRAD_LONE_GROUP_GFLOP: the threshold, 0 = never)
        lone_group = cls == 128 and 0 < self.wgrad_lone_group_gflop * 1e9 <= layers[0][2]
        if n == 1 and cls != 32 and not lone_group:
            # a lone layer gains nothing from the work list (measured on the bottleneck ResNets, whose 3x3 layers never neighbour:
            # FPN/ResNet50 1024x1024 18.25 -> 17.85 ms, PSPNet/ResNet101 768x768 10.13 -> 10.03 ms with the per-layer launch and its
            # tuned split count); the 32-channel class exists only as a grouped kernel (the per-layer one pads it to 64)
            self._emit_wgrad(*layers[0])
            return
        arr = (C.POINTER(_lib.WgradParams) * n)(*[C.pointer(wp) for wp, _, _ in layers])
        tb = int(self.lib.stp_wgrad_group_table_bytes(arr, n))
        wsb = int(self.lib.stp_wgrad_group_workspace_bytes(arr, n))
        if tb <= 0 or wsb <= 0:
            raise StpShapeError("grouped weight gradient: the layers %s do not form a group" % [nm for _, nm, _ in layers])
        host = (C.c_char * tb)()
        _lib.check(self.lib.stp_wgrad_group_build(arr, n, C.addressof(host), tb), "stp_wgrad_group_build")
        dev = self._table(bytes(host))
        ws = self._alloc((wsb // 4,), torch.float32)
        self._keep += [arr, host] + [wp for wp, _, _ in layers]
        names = [nm for _, nm, _ in layers]
        self.wgroups.append((names, cls))
        hdr = (C.c_int32 * 16).from_buffer_copy(bytes(host)[:64])      # WgGroupHeader: [14] = fused producer BN instance, [15] = all-taps tiles
        meta = {"layer": "group[%d]:%s..%s" % (n, names[0], names[-1]), "pass": "wgrad", "flops": sum(f for _, _, f in layers), "cout": cls,
                "bm": cls, "layers": names, "taps9": int(hdr[15]), "pbn": int(hdr[14])}
        self.bwd.append((self.lib.stp_wgrad_group_partial, (C.addressof(host), dev.data_ptr(), ws.data_ptr(), wsb), "stp_wgrad_group_partial", meta))
        self.bwd.append((self.lib.stp_wgrad_group_reduce, (C.addressof(host), dev.data_ptr(), ws.data_ptr()), "stp_wgrad_group_reduce", None))

    # ------------------------------------------------------------------ layers
    def input_u8(self, name, H, W, Cn):
        t = DT(name, self.N, H, W, Cn, None if self.dry else self._alloc((self.N, H, W, Cn), torch.uint8))
        self.inputs[name] = t
        return t

    def input_bn(self, name, x, eps):
        """BatchNormalization(scale=False) on the raw uint8 image -> dtype tensor padded to 4 channels (8 for images of 4..7
        channels, reference segmentation.py:135-155 builds N-channel models) whose channel x.C is the constant 1 (see
        stp_stem_beta_grad) and whose remaining channels are also 1 (their stem weights are zero: the unpadding drops their gradient)."""
        if x.C > 7:
            raise StpShapeError("input_bn handles up to 7 image channels")
        Cp = 4 if x.C <= 3 else 8
        beta = self.param(name + "/beta", (x.C,), "beta")
        mm = self.state(name + "/moving_mean", x.C, 0.0)
        mv = self.state(name + "/moving_variance", x.C, 1.0)
        out = self._new(name, x.H, x.W, Cp, False)
        out.meta["real_c"] = x.C
        out.meta["input_bn_beta"] = beta
        if self.dry:
            return out
        if self.training:
            mean, rstd = self._alloc((x.C,), torch.float32), self._alloc((x.C,), torch.float32)
            self._emit(self.fwd, "stp_bn_stats", x.buf.data_ptr(), ops.U8, x.rows, x.C, eps, self.bn_momentum,
                       mean.data_ptr(), rstd.data_ptr(), self._sptr(mm), self._sptr(mv), self.ws_bn.data_ptr(),
                       self.ws_bn.numel() * 4)
            self._emit(self.fwd, "stp_bn_apply", x.buf.data_ptr(), ops.U8, out.buf.data_ptr(), self.cdt, x.rows, x.C, Cp,
                       mean.data_ptr(), rstd.data_ptr(), None, self._pptr(beta), 0, 1.0)
        else:
            self._emit(self.fwd, "stp_bn_inference", x.buf.data_ptr(), ops.U8, out.buf.data_ptr(), self.cdt, x.rows, x.C, Cp,
                       self._sptr(mm), self._sptr(mv), eps, None, self._pptr(beta), 0, 1.0)
        return out

    def input_cast(self, name, x):
        """Raw uint8 image -> dtype tensor padded to 4 channels (zeros), no normalisation: the input of the keras.applications
        VGG encoders, which segmentation_models feeds with raw pixels (no in-graph preprocessing)."""
        if x.C > 7:
            raise StpShapeError("input_cast handles up to 7 image channels")
        Cp = 4 if x.C <= 3 else 8
        out = self._new(name, x.H, x.W, Cp, False)
        out.meta["real_c"] = x.C
        if self.dry:
            return out
        zero, one = self._alloc((8,), torch.float32), self._alloc((8,), torch.float32)
        zero.zero_(); one.fill_(1.0)
        # y = x * 1 + 0 through the uint8 BatchNorm-apply kernel (mean 0, rstd 1, no gamma/beta), padded channel = 0
        self._emit(self.fwd, "stp_bn_apply", x.buf.data_ptr(), ops.U8, out.buf.data_ptr(), self.cdt, x.rows, x.C, Cp,
                   zero.data_ptr(), one.data_ptr(), None, None, 0, 0.0)
        return out

    def bn(self, name, x, eps, relu=True, scale=True, momentum=None):
        """``relu``: False/0 none, True/1 ReLU, 2 ReLU6 (MobileNetV2).  ``momentum``: Keras BatchNormalization momentum (0.99)."""
        Cn = x.C
        relu = int(relu)
        momentum = self.bn_momentum if momentum is None else float(momentum)
        gamma = self.param(name + "/gamma", (Cn,), "gamma") if scale else None
        beta = self.param(name + "/beta", (Cn,), "beta")
        mm = self.state(name + "/moving_mean", Cn, 0.0)
        mv = self.state(name + "/moving_variance", Cn, 1.0)
        out = self._new(name, x.H, x.W, Cn, x.needs_grad or beta.trainable)
        self._bn_ws_c = max(self._bn_ws_c, Cn)
        self._use(x)
        if self.dry:
            self._slot_need += 4 * Cn * self._nslots(Cn)       # forward statistics + backward sums
            return out
        gp = self._pptr(gamma) if gamma else None
        if not self.training:
            self._emit(self.fwd, "stp_bn_inference", x.buf.data_ptr(), self.cdt, out.buf.data_ptr(), self.cdt, x.rows, Cn, Cn,
                       self._sptr(mm), self._sptr(mv), eps, gp, self._pptr(beta), int(relu), 0.0)
            return out
        mean, rstd = self._alloc((Cn,), torch.float32), self._alloc((Cn,), torch.float32)
        table = x.meta.get("stats_table")      # [2][C][columns] sums and their column count: a convolution's epilogue, or Plan.se's scale-add pass
        slots = x.meta.get("stats_slots")
        if slots is not None:
            # statistics from the producing convolution's fixed-point slots: finalize + normalise + activation in one kernel
            self._emit(self.fwd, "stp_bn_apply_slots", x.buf.data_ptr(), out.buf.data_ptr(), self.cdt, x.rows, Cn, slots[0], slots[1], eps,
                       momentum, mean.data_ptr(), rstd.data_ptr(), self._sptr(mm), self._sptr(mv), gp, self._pptr(beta), int(relu))
        elif table is not None:
            self._emit(self.fwd, "stp_bn_finalize", table[0].data_ptr(), table[1], x.rows, Cn, eps, momentum, mean.data_ptr(),
                       rstd.data_ptr(), self._sptr(mm), self._sptr(mv))
        else:
            self._emit(self.fwd, "stp_bn_stats", x.buf.data_ptr(), self.cdt, x.rows, Cn, eps, momentum, mean.data_ptr(),
                       rstd.data_ptr(), self._sptr(mm), self._sptr(mv), self.ws_bn.data_ptr(), self.ws_bn.numel() * 4)
        if slots is None:
            self._emit(self.fwd, "stp_bn_apply", x.buf.data_ptr(), self.cdt, out.buf.data_ptr(), self.cdt, x.rows, Cn, Cn,
                       mean.data_ptr(), rstd.data_ptr(), gp, self._pptr(beta), int(relu), 0.0)
        out.meta["bn"] = (x.buf.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gp, self._pptr(beta), int(relu))
        if self.fuse_bn_sc and slots is None:
            out.meta["apply_rec"] = self.fwd[-1]
            out.meta["sc_consumers"], out.meta["halo_consumers"] = [], []

        def back():
            if not out.needs_grad or not out.grad_ready:
                return
            # dx is always produced (it is cheap relative to skipping logic); frozen params are masked in the optimizer
            bslots = out.meta.get("bnb_slots")
            dadd = None
            if (x.needs_grad and x.grad_ready and x.grad is not None and x.grad.data_ptr() in self._wgroup_reads and bslots is None
                    and out.meta.get("bnb") is not None):
                # x's gradient so far is the dY of a convolution whose weight gradient waits in the pending group (the residual
                # branch aliases it): accumulate OUT OF PLACE - the sum lands in a fresh buffer, the dY stays intact
                dadd, x.grad = x.grad, None
            dx = self._gradbuf(x) if x.needs_grad else self._alloc((x.N, x.H, x.W, Cn))
            if bslots is not None:
                self._emit(self.bwd, "stp_bn_backward_slots", x.buf.data_ptr(), out.grad.data_ptr(), dx.data_ptr(), self.cdt, x.rows, Cn,
                           mean.data_ptr(), rstd.data_ptr(), gp, bslots[0], bslots[1], self._gptr(gamma) if gamma else None,
                           self._gptr(beta), int(x.grad_ready and x.needs_grad))
            elif out.meta.get("bnb") is not None:
                # the only consumer's data-gradient epilogue already masked dY and reduced the per-tile sums
                st, q = out.meta["bnb"]
                tiles = q if isinstance(q, int) else int(self.lib.stp_conv2d_stats_floats(C.byref(q))) // (2 * Cn)
                if dadd is not None:
                    self._emit(self.bwd, "stp_bn_backward_fused_add", x.buf.data_ptr(), out.grad.data_ptr(), dx.data_ptr(), dadd.data_ptr(),
                               self.cdt, x.rows, Cn, mean.data_ptr(), rstd.data_ptr(), gp, st.data_ptr(), tiles,
                               self._gptr(gamma) if gamma else None, self._gptr(beta), 1, self.ws_bn.data_ptr(), self.ws_bn.numel() * 4)
                else:
                    self._emit(self.bwd, "stp_bn_backward_fused", x.buf.data_ptr(), out.grad.data_ptr(), dx.data_ptr(), self.cdt,
                               x.rows, Cn, mean.data_ptr(), rstd.data_ptr(), gp, st.data_ptr(), tiles,
                               self._gptr(gamma) if gamma else None, self._gptr(beta), int(x.grad_ready and x.needs_grad),
                               self.ws_bn.data_ptr(), self.ws_bn.numel() * 4)
            else:
                self._emit(self.bwd, "stp_bn_backward", x.buf.data_ptr(), out.grad.data_ptr(), dx.data_ptr(), self.cdt, x.rows, Cn,
                           mean.data_ptr(), rstd.data_ptr(), gp, self._pptr(beta), self._gptr(gamma) if gamma else None,
                           self._gptr(beta), int(relu), int(x.grad_ready and x.needs_grad), self.ws_bn.data_ptr(), self.ws_bn.numel() * 4)
            if x.needs_grad:
                x.grad_ready = True

        self._tape.append(back)
        return out

    def _emit_bias_grad(self, dy, rows, gradC, Cout, b):
        """Bias gradient = the channel sums of ``dy`` ([rows][gradC], the first ``Cout`` channels real)."""
        tmp = self._alloc((gradC,), torch.float32)
        self._emit(self.bwd, "stp_channel_sum", dy.data_ptr(), self.cdt, rows, gradC, tmp.data_ptr(), 0, self.ws_bn.data_ptr(), self.ws_bn.numel() * 4)
        self._emit(self.bwd, "stp_weight_grad_unpad", tmp.data_ptr(), self._gptr(b), Cout, 1, 1, 1, 1, 1, 0)

    def conv3x3_taps(self, name, x, Cout, bias=False):
        """``Conv2D(Cout, 3x3, padding 1)`` with few output channels over many input channels (the class heads of FPN / PSPNet: 512 -> 3 /
        20) as a 1x1 convolution into 9 x Cout tap channels + stp_tapsum_fwd (elementwise.hip: W_t . shift_t(x) = shift_t(W_t . x)).  The
        parameters keep the layer's names and shapes (``name/kernel`` = (Cout, 3, 3, Cin), ``name/bias``): the 1x1 launch reads the 3x3
        kernel's own bytes as [9 Cout][Cin], its weight gradient IS the kernel's gradient."""
        cin = x.meta.get("real_c", x.C)
        # (the gradient of the tap channels in rows of 64: the data gradient's K is then whole 64-channel steps of the buffer-DMA kernel -
        #  with K = 32 it ran at 1.8 TB/s, 302 us on FPN's 4 x 256 x 256 x 512 map)
        z = self.conv(name + "_taps", x, 9 * Cout, 1, param_name=name, param_shape=(Cout, 3, 3, cin), cout_pad=64 if self.dtype != "fp32" else None)
        b = self.param(name + "/bias", (Cout,), "bias") if bias else None
        out = self._new(name, x.H, x.W, Cout, z.needs_grad or (b is not None and b.trainable))
        out.gradC = _rup(Cout, self.vec)
        if bias:
            self._bn_ws_c = max(self._bn_ws_c, out.gradC)
        self._use(z)
        if self.dry:
            return out
        self._emit(self.fwd, "stp_tapsum_fwd", z.buf.data_ptr(), out.buf.data_ptr(), self._pptr(b) if b is not None else None, self.N, x.H, x.W,
                   Cout, z.C, Cout, self.cdt)
        if not self.training:
            return out

        def back():
            if not out.grad_ready:
                return
            dy = out.grad
            if b is not None and b.trainable:
                self._emit_bias_grad(dy, out.rows, out.gradC, Cout, b)
            if z.needs_grad:
                self._emit(self.bwd, "stp_tapsum_bwd", dy.data_ptr(), self._gradbuf(z).data_ptr(), self.N, x.H, x.W, Cout, out.gradC, z.gradC, self.cdt)
                z.grad_ready = True

        self._tape.append(back)
        return out

    def conv(self, name, x, Cout, k, stride=1, pad=0, src1=None, upsample=False, bias=False, residual=None, bn_stats=False,
             transpose=False, relu=False, same_tf=False, fold_shortcut=None, param_name=None, param_shape=None, cout_pad=None,
             param_cols=None, flops_as=None):
        """Conv2D (explicit symmetric ZeroPadding + 'valid').  ``upsample`` folds UpSampling2D(2) of x,
        ``src1`` folds Concatenate([up(x), src1]) into the GEMM gather; ``residual`` folds Add().

        ``fold_shortcut``: the output tensor of the 1x1 / stride-2 projection shortcut that reads the same ``x`` as this 3x3 / stride-2
        convolution (ResNet basic block): its data gradient is folded into this layer's data-gradient launch (stp_conv_params.fold_*).

        ``param_cols`` = (first column, total columns): this 1x1 convolution multiplies by the COLUMN RANGE [first, first + Cin) of the shared
        kernel ``param_name/kernel`` of shape (Cout, 1, 1, total) - the PSPNet head without its concatenation (nets.pspnet_resnet): the range is
        copied into a dense fp32 matrix in front of the weight preparation (stp_copy_cols_f32) and the weight gradient is copied back into it.

        ``transpose``: Keras ``Conv2DTranspose(Cout, k, strides=2, padding='same')`` (k even, 4 in segmentation_models'
        transpose decoder blocks).  TF pads the equivalent forward convolution by k/2-1 on each side, so the transposed
        convolution is a stride-1 convolution over the ZERO-INSERTED input (2H-1 x 2W-1) with pad k-1-(k/2-1) and the
        spatially flipped kernel - the zero-insertion gather that the stride-2 data-gradients already use.  The master
        parameter holds the flipped OHWI kernel (kind "tkernel"; set/get_weights convert from Keras' (kh,kw,out,in))."""
        L = ConvLayer(self, name, x, Cout, k, stride, pad, src1, upsample, residual, transpose, relu, same_tf, fold_shortcut, param_cols)
        L.declare(param_name, param_shape, cout_pad, bias)
        if self.dry:
            return L.out
        L.forward(bn_stats, flops_as)
        if self.training:
            self._tape.append(L.backward)
        return L.out

    def add(self, name, y, skip):
        """Keras ``Add()([y, skip])`` computed in place on y's buffer (y must have no other consumer): Linknet's
        decoder adds the encoder feature AFTER BatchNormalization + ReLU, so it cannot ride in a conv epilogue."""
        if (y.H, y.W, y.C) != (skip.H, skip.W, skip.C):
            raise StpShapeError("%s: cannot add %dx%dx%d and %dx%dx%d" % (name, y.H, y.W, y.C, skip.H, skip.W, skip.C))
        out = DT(name, self.N, y.H, y.W, y.C, y.buf, y.needs_grad or skip.needs_grad)
        out.gradC = y.gradC
        self.tensors[name] = out
        self._use(y, skip)
        if self.dry:
            return out
        self._emit(self.fwd, "stp_add_inplace", y.buf.data_ptr(), skip.buf.data_ptr(), y.rows * y.C, self.cdt)
        if not self.training:
            return out

        def back():
            if not out.needs_grad or not out.grad_ready:
                return
            dy = out.grad
            if y.needs_grad:
                y.grad, y.grad_ready = dy, True          # alias: read by y's backward, issued before any later writer below
            if skip.needs_grad:
                if not skip.grad_ready and skip.gradC == out.gradC:
                    skip.grad, skip.grad_ready = dy, True   # first gradient of the skip tensor: alias, later writers accumulate
                else:
                    self._emit(self.bwd, "stp_add_inplace", self._gradbuf(skip).data_ptr(), dy.data_ptr(), y.rows * out.gradC,
                               self.cdt)

        self._tape.append(back)
        return out

    def se(self, name, u, shortcut, reduction=16, bn_stats=True):
        """Channel squeeze-and-excitation on the residual branch of an SE-ResNet basic unit, with the unit's Add():
        ``x = u * sigmoid(relu(mean_hw(u) W1 + b1) W2 + b2) + shortcut`` (csrc/se.hip; the arithmetic and its rounding points are
        stated at stp_se_* in include/stp_hip.h).  Parameters in the Keras Conv2D(1x1, use_bias=True) layouts: ``name_fc1/kernel``
        (1, 1, C, C / reduction), ``name_fc1/bias``, ``name_fc2/kernel`` (1, 1, C / reduction, C), ``name_fc2/bias`` - fp32 masters, read
        as they are.  ``bn_stats``: the scale-add pass also sums the tensor it stores for the BatchNormalization that follows."""
        if (u.H, u.W, u.C) != (shortcut.H, shortcut.W, shortcut.C) or u.gradC != u.C or shortcut.gradC != u.C:
            raise StpShapeError("%s: cannot gate %dx%dx%d onto a %dx%dx%d shortcut" % (name, u.H, u.W, u.C, shortcut.H, shortcut.W, shortcut.C))
        Cn, HW = u.C, u.H * u.W
        R = Cn // int(reduction)
        chunks = int(self.lib.stp_se_chunks(self.N, HW, Cn))
        if chunks < 1 or not 1 <= R <= 32:
            raise StpShapeError("%s: squeeze-and-excitation serves 16..512 channels in multiples of 8 with 1..32 hidden units (got %d / %d)"
                                % (name, Cn, R))
        w1 = self.param(name + "_fc1/kernel", (1, 1, Cn, R), "sekernel")
        b1 = self.param(name + "_fc1/bias", (R,), "bias")
        w2 = self.param(name + "_fc2/kernel", (1, 1, R, Cn), "sekernel")
        b2 = self.param(name + "_fc2/bias", (Cn,), "bias")
        out = self._new(name, u.H, u.W, Cn, u.needs_grad or shortcut.needs_grad or w1.trainable)
        self._use(u, shortcut)
        if self.dry:
            return out
        wsp, wsb = self._scratch(self.lib.stp_se_workspace_bytes(self.N, HW, Cn))      # [N][chunks][C] partial sums, forward and backward
        z, s = self._alloc((self.N * Cn,), torch.float32), self._alloc((self.N * Cn,), torch.float32)
        h = self._alloc((_rup(self.N * R, 4),), torch.float32)
        tiles = self.N * chunks
        st = self._alloc((2 * Cn * tiles,), torch.float32) if (bn_stats and self.training) else None
        self._emit(self.fwd, "stp_se_squeeze", u.buf.data_ptr(), self.cdt, self.N, HW, Cn, wsp, wsb)
        self._emit(self.fwd, "stp_se_excite", wsp, self.N, HW, Cn, R, self._pptr(w1), self._pptr(b1), self._pptr(w2), self._pptr(b2),
                   z.data_ptr(), h.data_ptr(), s.data_ptr())
        self._emit(self.fwd, "stp_se_scale_add", u.buf.data_ptr(), shortcut.buf.data_ptr(), out.buf.data_ptr(), self.cdt, self.N, HW, Cn,
                   s.data_ptr(), st.data_ptr() if st is not None else None)
        if st is not None:
            out.meta["stats_table"] = (st, tiles)        # no meta["stats"]: Plan.bn hands the table to stp_bn_finalize as it is
        if not self.training:
            return out

        def back():
            if not out.needs_grad or not out.grad_ready:
                return
            dx = out.grad           # read three times below, never rewritten here
            if shortcut.needs_grad:
                if not shortcut.grad_ready:
                    shortcut.grad, shortcut.grad_ready = dx, True      # first gradient of the shortcut: alias, later writers accumulate
                else:
                    self._emit(self.bwd, "stp_add_inplace", self._gradbuf(shortcut).data_ptr(), dx.data_ptr(), out.rows * Cn, self.cdt)
            da2, dz = self._alloc((self.N * Cn,), torch.float32), self._alloc((self.N * Cn,), torch.float32)
            da1 = self._alloc((_rup(self.N * R, 4),), torch.float32)
            self._emit(self.bwd, "stp_se_bwd_reduce", dx.data_ptr(), u.buf.data_ptr(), self.cdt, self.N, HW, Cn, wsp, wsb)
            # (parameter gradients are WRITTEN, summed over the images in image order; addresses asked in declaration order reversed)
            g2b, g2, g1b, g1 = self._gptr(b2), self._gptr(w2), self._gptr(b1), self._gptr(w1)
            self._emit(self.bwd, "stp_se_excite_bwd", wsp, self.N, HW, Cn, R, self._pptr(w1), self._pptr(w2), z.data_ptr(), h.data_ptr(),
                       s.data_ptr(), da2.data_ptr(), da1.data_ptr(), dz.data_ptr(), g1, g1b, g2, g2b)
            if u.needs_grad:
                # u's gradient is conv2's dY, which a pending grouped weight gradient reads until it is issued: a buffer of its own
                if u.grad_ready:
                    raise StpShapeError("%s: the gated tensor must have no other consumer" % name)
                self._emit(self.bwd, "stp_se_bwd_apply", dx.data_ptr(), self._gradbuf(u).data_ptr(), self.cdt, self.N, HW, Cn, s.data_ptr(),
                           dz.data_ptr())
                u.grad_ready = True

        self._tape.append(back)
        return out

    def relu(self, name, x):
        """Keras ``Activation('relu')`` as a tensor of its own (DeepLab's xception blocks activate a tensor that its other
        consumers - the shortcut convolution, the Add - read raw, model.py:133-134): y = max(x, 0) through the BatchNormalization
        apply kernel with the identity affine; the gradient is masked in place by y > 0 and joins x's other gradients."""
        Cn = x.C
        out = self._new(name, x.H, x.W, Cn, x.needs_grad)
        out.gradC = x.gradC
        self._use(x)
        if self.dry:
            return out
        zero, one = self._alloc((Cn,), torch.float32), self._alloc((Cn,), torch.float32)
        zero.zero_(); one.fill_(1.0)
        self._emit(self.fwd, "stp_bn_apply", x.buf.data_ptr(), self.cdt, out.buf.data_ptr(), self.cdt, x.rows, Cn, Cn, zero.data_ptr(),
                   one.data_ptr(), None, None, 1, 0.0)
        if not self.training:
            return out

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            dy = out.grad
            if out.gradC != Cn:
                raise StpShapeError("%s: standalone ReLU needs an unpadded channel count" % name)
            self._guard_write(dy)
            self._emit(self.bwd, "stp_relu_bwd", out.buf.data_ptr(), dy.data_ptr(), x.rows * Cn, self.cdt)
            if not x.grad_ready and x.gradC == out.gradC:
                x.grad, x.grad_ready = dy, True
            else:
                self._emit(self.bwd, "stp_add_inplace", self._gradbuf(x).data_ptr(), dy.data_ptr(), x.rows * Cn, self.cdt)

        self._tape.append(back)
        return out

    def upsample_add(self, name, x, m):
        """FPN top-down step ``Add()([x, UpSampling2D(2)(m)])`` in place on x's buffer (x must have no other consumer yet)."""
        if (x.H, x.W, x.C) != (2 * m.H, 2 * m.W, m.C):
            raise StpShapeError("%s: %dx%dx%d cannot take the 2x upsampling of %dx%dx%d" % (name, x.H, x.W, x.C, m.H, m.W, m.C))
        out = DT(name, self.N, x.H, x.W, x.C, x.buf, x.needs_grad or m.needs_grad)
        out.gradC = x.gradC
        self.tensors[name] = out
        self._use(x, m)
        if self.dry:
            return out
        self._emit(self.fwd, "stp_upsample2x_add", x.buf.data_ptr(), m.buf.data_ptr(), self.N, x.H, x.W, x.C, self.cdt)
        if not self.training:
            return out

        def back():
            if not out.needs_grad or not out.grad_ready:
                return
            dy = out.grad
            if m.needs_grad:
                self._emit(self.bwd, "stp_upsample2x_bwd", dy.data_ptr(), self._gradbuf(m).data_ptr(), self.N, m.H, m.W, m.C, out.gradC,
                           self.cdt, int(m.grad_ready))
                m.grad_ready = True
            if x.needs_grad:
                x.grad, x.grad_ready = dy, True

        self._tape.append(back)
        return out

    def upsample_sum(self, name, parts):
        """``sum_i ResizeImage(f_i, 'bilinear')(t_i)`` of up to four maps with equal channel counts (TF 1.x bilinear, integer factors; one fp32
        sum, one rounding): the resized pyramid terms of the PSPNet head, computed behind their 1x1 convolutions (nets.pspnet_resnet).  The
        gradient of each part is the bilinear-resize gradient of the sum's gradient."""
        if not 1 <= len(parts) <= 4:
            raise StpShapeError("%s: one to four parts" % name)
        Ho, Wo, Cn = parts[0][0].H * parts[0][1], parts[0][0].W * parts[0][1], parts[0][0].C
        if Ho != Wo or any((t.H * f, t.W * f, t.C) != (Ho, Wo, Cn) or t.H != t.W for t, f in parts):
            raise StpShapeError("%s: the parts must be square maps of equal channel count that resize to one size" % name)
        out = self._new(name, Ho, Wo, Cn, any(t.needs_grad for t, _ in parts))
        self._use(*[t for t, _ in parts])
        if self.dry:
            return out
        ptrs = [t.buf.data_ptr() for t, _ in parts] + [None] * (4 - len(parts))
        hs = [t.H for t, _ in parts] + [0] * (4 - len(parts))
        self._emit(self.fwd, "stp_upsample_sum", ptrs[0], ptrs[1], ptrs[2], ptrs[3], hs[0], hs[1], hs[2], hs[3], out.buf.data_ptr(), self.N, Ho, Wo, Cn,
                   self.cdt)
        if not self.training:
            return out

        def back():
            if not out.needs_grad or not out.grad_ready:
                return
            for t, f in parts:
                if not t.needs_grad:
                    continue
                wp, wb = self._scratch(self.lib.stp_resize_bilinear_bwd_workspace_bytes(self.N, t.H, t.W, t.C, f))
                self._emit(self.bwd, "stp_resize_bilinear_bwd", out.grad.data_ptr(), self._gradbuf(t).data_ptr(), self.N, t.H, t.W, t.C, f, out.gradC, 0,
                           self.cdt, int(t.grad_ready), wp, wb)
                t.grad_ready = True

        self._tape.append(back)
        return out

    def concat_resize(self, name, parts, nearest=False):
        """``Concatenate()([ResizeImage(f_i, interpolation)(t_i) ...])``: every part is resized (TF 1.x bilinear, or nearest;
        integer factor; 1 = copy) straight into its channel slice of the output."""
        Ho, Wo = parts[0][0].H * parts[0][1], parts[0][0].W * parts[0][1]
        if any((t.H * f, t.W * f) != (Ho, Wo) for t, f in parts):
            raise StpShapeError("%s: resized parts differ in size" % name)
        Ct = sum(t.C for t, _ in parts)
        out = self._new(name, Ho, Wo, Ct, any(t.needs_grad for t, _ in parts))
        self._use(*[t for t, _ in parts])
        if self.dry:
            return out
        off = 0
        for t, f in parts:
            self._emit(self.fwd, "stp_resize_nearest" if nearest else "stp_resize_bilinear", t.buf.data_ptr(), out.buf.data_ptr(), self.N, t.H,
                       t.W, t.C, f, Ct, off, self.cdt)
            off += t.C
        if not self.training:
            return out

        def back():
            if not out.needs_grad or not out.grad_ready:
                return
            o = 0
            for t, f in parts:
                if t.needs_grad and nearest:
                    self._emit(self.bwd, "stp_resize_nearest_bwd", out.grad.data_ptr(), self._gradbuf(t).data_ptr(), self.N, t.H, t.W,
                               t.C, f, out.gradC, o, self.cdt, int(t.grad_ready))
                    t.grad_ready = True
                elif t.needs_grad:
                    wp, wb = self._scratch(self.lib.stp_resize_bilinear_bwd_workspace_bytes(self.N, t.H, t.W, t.C, f))
                    self._emit(self.bwd, "stp_resize_bilinear_bwd", out.grad.data_ptr(), self._gradbuf(t).data_ptr(), self.N, t.H, t.W,
                               t.C, f, out.gradC, o, self.cdt, int(t.grad_ready), wp, wb)
                    t.grad_ready = True
                o += t.C

        self._tape.append(back)
        return out

    def resize(self, name, x, factor, nearest=False):
        """``ResizeImage(factor, 'bilinear' | 'nearest')`` of a tensor whose gradient carries padded channels (the class logits)."""
        out = self._new(name, x.H * factor, x.W * factor, x.C, x.needs_grad)
        out.gradC = x.gradC
        self._use(x)
        if self.dry:
            return out
        self._emit(self.fwd, "stp_resize_nearest" if nearest else "stp_resize_bilinear", x.buf.data_ptr(), out.buf.data_ptr(), self.N, x.H, x.W,
                   x.C, factor, x.C, 0, self.cdt)
        if not self.training:
            return out
        if not nearest:      # (softmax_loss may take this launch and its gradient over: stp_softmax_cce_dice_up)
            out.meta["resize_rec"] = (len(self.fwd) - 1, x, int(factor))

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            if nearest:
                self._emit(self.bwd, "stp_resize_nearest_bwd", out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.gradC,
                           factor, x.gradC, 0, self.cdt, int(x.grad_ready))
                x.grad_ready = True
                return
            wp, wb = self._scratch(self.lib.stp_resize_bilinear_bwd_workspace_bytes(self.N, x.H, x.W, x.gradC, factor))
            self._emit(self.bwd, "stp_resize_bilinear_bwd", out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.gradC,
                       factor, x.gradC, 0, self.cdt, int(x.grad_ready), wp, wb)
            x.grad_ready = True

        self._tape.append(back)
        return out

    def dwconv(self, name, x, k=3, stride=1, dilation=1, explicit_pad=False):
        """Keras ``DepthwiseConv2D(k, strides, padding='same', dilation_rate, use_bias=False)`` (DeepLab model.py:136, 255-259).
        The fp32 master kernel [k][k][C] is read directly by the kernels (kind "dw": Keras' (kh,kw,C,1) layout as stored)."""
        Cn = x.C
        if Cn % 4:
            raise StpShapeError("%s: depthwise convolution needs a multiple of 4 channels" % name)
        keff = (k - 1) * dilation + 1
        Ho, Wo = -(-x.H // stride), -(-x.W // stride)
        pt, pl = max((Ho - 1) * stride + keff - x.H, 0) // 2, max((Wo - 1) * stride + keff - x.W, 0) // 2
        if explicit_pad:
            # ZeroPadding2D((pad_beg, pad_end)) + 'valid' (DeepLab SepConv_BN with stride > 1, model.py:126-132): the padding does
            # not depend on the input size, unlike TF 'same'
            pt = pl = (keff - 1) // 2
            Ho, Wo = (x.H + (keff - 1) - keff) // stride + 1, (x.W + (keff - 1) - keff) // stride + 1
        w = self.param(name + "/depthwise_kernel", (k, k, Cn), "dw")
        out = self._new(name, Ho, Wo, Cn, x.needs_grad or w.trainable)
        self._use(x)
        self._dw_ws_bytes = max(self._dw_ws_bytes, int(self.lib.stp_dwconv_wgrad_workspace_bytes(Cn, k)))
        if self.dry:
            return out
        geo = (self.N, x.H, x.W, Cn, k, stride, pt, pl, dilation, Ho, Wo, self.cdt)
        self._emit(self.fwd, "stp_dwconv", x.buf.data_ptr(), self._pptr(w), out.buf.data_ptr(), *geo)
        if not self.training:
            return out

        def back():
            if not out.needs_grad or not out.grad_ready:
                return
            if w.trainable:
                self._emit(self.bwd, "stp_dwconv_wgrad", x.buf.data_ptr(), out.grad.data_ptr(), self._gptr(w), *geo, 0,
                           self.ws_dw.data_ptr(), self.ws_dw.numel() * 4)
            if x.needs_grad:
                self._emit(self.bwd, "stp_dwconv_dgrad", out.grad.data_ptr(), self._pptr(w), self._gradbuf(x).data_ptr(), *geo,
                           int(x.grad_ready))
                x.grad_ready = True

        self._tape.append(back)
        return out

    def dropout(self, name, x, rate, salt, spatial=False):
        """Keras ``Dropout(rate)`` / ``SpatialDropout2D(rate)`` (``spatial``: one decision per sample and channel): training =
        inverted dropout in place (mask = hash of the device step counter, which the first dropout of the plan ticks once per
        forward); inference = identity."""
        if not self.training:
            return x
        out = DT(name, self.N, x.H, x.W, x.C, x.buf, x.needs_grad)
        out.gradC = x.gradC
        self.tensors[name] = out
        self._use(x)
        if self.dry:
            return out
        if self.step_state is None:
            self.step_state = torch.zeros(2, dtype=torch.int32, device=self.device)
            self._keep.append(self.step_state)
            self._emit(self.fwd, "stp_counter_tick", self.step_state.data_ptr())
        cnt = x.rows * x.C
        if spatial:
            self._emit(self.fwd, "stp_dropout_spatial", x.buf.data_ptr(), x.buf.data_ptr(), self.N, x.H * x.W, x.C, float(rate),
                       self.step_state.data_ptr(), int(salt), self.cdt)
        else:
            self._emit(self.fwd, "stp_dropout", x.buf.data_ptr(), x.buf.data_ptr(), cnt, float(rate), self.step_state.data_ptr(), int(salt), self.cdt)

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            dy = out.grad
            if spatial:
                if out.gradC != x.C:
                    raise StpShapeError("%s: spatial dropout needs an unpadded channel count" % name)
                self._emit(self.bwd, "stp_dropout_spatial", dy.data_ptr(), dy.data_ptr(), self.N, x.H * x.W, x.C, float(rate),
                           self.step_state.data_ptr(), int(salt), self.cdt)
            else:
                self._emit(self.bwd, "stp_dropout", dy.data_ptr(), dy.data_ptr(), x.rows * out.gradC, float(rate), self.step_state.data_ptr(),
                           int(salt), self.cdt)
            x.grad, x.grad_ready = dy, True

        self._tape.append(back)
        return out

    def resize_ac(self, name, x, Ho, Wo):
        """``BilinearUpsampling`` (DeepLab model.py:56-100): tf.image.resize_bilinear(align_corners=True) to (Ho, Wo)."""
        out = self._new(name, Ho, Wo, x.C, x.needs_grad)
        out.gradC = x.gradC
        self._use(x)
        if self.dry:
            return out
        self._emit(self.fwd, "stp_resize_bilinear_ac", x.buf.data_ptr(), out.buf.data_ptr(), self.N, x.H, x.W, x.C, Ho, Wo, self.cdt)
        if not self.training:
            return out

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            self._emit(self.bwd, "stp_resize_bilinear_ac_bwd", out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.gradC,
                       Ho, Wo, self.cdt, int(x.grad_ready))
            x.grad_ready = True

        self._tape.append(back)
        return out

    def sigmoid_act(self, name, z):
        """The activation of DeepLab's last convolution as a layer (model.py:485): sigmoid for one class, channel softmax for
        2..32 classes."""
        out = self._new(name, z.H, z.W, z.C, z.needs_grad)
        out.gradC = z.gradC
        self._use(z)
        if self.dry:
            return out
        fn = "stp_sigmoid_act" if z.C == 1 else "stp_softmax_act"
        self._emit(self.fwd, fn, z.buf.data_ptr(), out.buf.data_ptr(), z.rows, z.C, z.C, z.C, self.cdt)
        if not self.training:
            return out

        def back():
            if not (z.needs_grad and out.grad_ready):
                return
            self._emit(self.bwd, fn + "_bwd", out.buf.data_ptr(), out.grad.data_ptr(), self._gradbuf(z).data_ptr(), z.rows, z.C,
                       z.C, z.gradC, self.cdt)
            z.grad_ready = True

        self._tape.append(back)
        return out

    def prob_loss(self, probs, target, w_ce, w_dice):
        """w*binary_crossentropy (one class) or w*categorical_crossentropy (class-index target) + w_dice*dice_loss on
        PROBABILITIES; seeds the backward pass."""
        if self.dry:
            return
        if self.training and self.loss_scale != 1.0:
            raise StpShapeError("the losses on probabilities (DeepLabV3) have no loss-scaling form: use loss_scale=1 (or bf16)")
        self.loss_scalars = self._alloc((12,), torch.float32)
        dp = self._gradbuf(probs) if self.training else None
        if probs.C == 1:
            self._emit(self.fwd, "stp_prob_bce_dice", probs.buf.data_ptr(), target.buf.data_ptr(), probs.rows, self.cdt, float(w_ce),
                       float(w_dice), self.loss_scalars.data_ptr(), dp.data_ptr() if dp is not None else None, probs.gradC,
                       self.ws_loss.data_ptr(), self.ws_loss.numel() * 4)
        else:
            self._emit(self.fwd, "stp_prob_cce_dice", probs.buf.data_ptr(), target.buf.data_ptr(), probs.rows, probs.C, probs.C, self.cdt,
                       float(w_ce), float(w_dice), self.loss_scalars.data_ptr(), dp.data_ptr() if dp is not None else None, probs.gradC,
                       self.ws_loss.data_ptr(), self.ws_loss.numel() * 4)
            self._emit_confusion(probs, target)       # (an argmax does not care whether the rows hold logits or probabilities)
        probs.grad_ready = self.training

    def probs_out(self, probs):
        """Inference output when the model itself ends in probabilities: float32 copy."""
        if self.dry:
            return None
        if self.tdt == torch.float32:
            self.probs = probs.buf                      # already float32
            return self.probs
        self.probs = self._alloc((probs.N, probs.H, probs.W, probs.C), torch.float32)
        self._emit(self.fwd, "stp_cast_bf16_to_f32", probs.buf.data_ptr(), self.probs.data_ptr(), probs.rows * probs.C, 1.0)
        return self.probs

    def avgpool(self, name, x, k):
        """AveragePooling2D(pool_size = strides = k) with exact division (PSPNet pyramid levels)."""
        if x.H % k or x.W % k:
            raise StpShapeError("%s: %dx%d is not divisible by the pooling size %d" % (name, x.H, x.W, k))
        out = self._new(name, x.H // k, x.W // k, x.C, x.needs_grad)
        self._use(x)
        if self.dry:
            return out
        wp, wb = self._scratch(self.lib.stp_avgpool_workspace_bytes(self.N, x.H, x.W, x.C, k))
        self._emit(self.fwd, "stp_avgpool", x.buf.data_ptr(), out.buf.data_ptr(), self.N, x.H, x.W, x.C, k, self.cdt, wp, wb)
        if not self.training:
            return out

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            self._emit(self.bwd, "stp_avgpool_bwd", out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.C, k, self.cdt,
                       int(x.grad_ready))
            x.grad_ready = True

        self._tape.append(back)
        return out

    def avgpool_pyramid(self, names, x, ks):
        """The AveragePooling2D(k) of PSPNet's pyramid levels (one per name / window size) of ONE tensor: where the windows nest (every k a
        multiple of the smallest one) a single pass over ``x`` (stp_avgpool_pyramid) and a single pass over its gradient instead of one per
        level; otherwise the separate launches of ``avgpool``.  Returns the pooled tensors in the order of ``names``."""
        order = sorted(range(len(ks)), key=lambda i: ks[i])
        kk = [int(ks[i]) for i in order] + [0] * (4 - len(ks))
        if (len(ks) < 2 or len(ks) > 4 or any(x.H % k or x.W % k for k in ks)
                or not self.lib.stp_avgpool_pyramid_ok(self.N, x.H, x.W, x.C, kk[0], kk[1], kk[2], kk[3], self.cdt)):
            return [self.avgpool(nm, x, k) for nm, k in zip(names, ks)]
        outs = [self._new(nm, x.H // k, x.W // k, x.C, x.needs_grad) for nm, k in zip(names, ks)]
        for _ in outs:
            self._use(x)
        if self.dry:
            return outs
        so = [outs[i] for i in order]
        wp, wb = self._scratch(self.lib.stp_avgpool_pyramid_workspace_bytes(self.N, x.H, x.W, x.C, kk[0], self.cdt))
        yp = [t.buf.data_ptr() for t in so] + [None] * (4 - len(so))
        self._emit(self.fwd, "stp_avgpool_pyramid", x.buf.data_ptr(), yp[0], yp[1], yp[2], yp[3], kk[0], kk[1], kk[2], kk[3], self.N, x.H, x.W,
                   x.C, self.cdt, wp, wb)
        if not self.training:
            return outs

        def back():
            if not x.needs_grad:
                return
            ready = [t for t in so if t.grad_ready]
            if len(ready) == len(so):
                gp = [t.grad.data_ptr() for t in so] + [None] * (4 - len(so))
                self._emit(self.bwd, "stp_avgpool_pyramid_bwd", gp[0], gp[1], gp[2], gp[3], kk[0], kk[1], kk[2], kk[3], self._gradbuf(x).data_ptr(),
                           self.N, x.H, x.W, x.C, self.cdt, int(x.grad_ready))
                x.grad_ready = True
                return
            for t, k in zip(so, kk):      # (a level without a gradient: the separate launches for the others)
                if t.grad_ready:
                    self._emit(self.bwd, "stp_avgpool_bwd", t.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.C, k, self.cdt,
                               int(x.grad_ready))
                    x.grad_ready = True

        self._tape.append(back)
        return outs

    def maxpool_k(self, name, x, k):
        """MaxPooling2D(pool_size = strides = k) (PSPNet ``psp_pooling_type: max``)."""
        if x.H % k or x.W % k:
            raise StpShapeError("%s: %dx%d is not divisible by the pooling size %d" % (name, x.H, x.W, k))
        out = self._new(name, x.H // k, x.W // k, x.C, x.needs_grad)
        self._use(x)
        if self.dry:
            return out
        idx = self._alloc((self.N, x.H // k, x.W // k, x.C), torch.int32) if self.training else None
        self._emit(self.fwd, "stp_maxpool_k", x.buf.data_ptr(), out.buf.data_ptr(), idx.data_ptr() if idx is not None else None, self.N, x.H,
                   x.W, x.C, k, self.cdt)
        if not self.training:
            return out

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            self._emit(self.bwd, "stp_maxpool_k_bwd", idx.data_ptr(), out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.C, k,
                       self.cdt, int(x.grad_ready))
            x.grad_ready = True

        self._tape.append(back)
        return out

    def maxpool2(self, name, x):
        """MaxPooling2D(2, 2) without padding (VGG blocks)."""
        if x.H % 2 or x.W % 2:
            raise StpShapeError("%s: 2x2 pooling needs even height/width" % name)
        out = self._new(name, x.H // 2, x.W // 2, x.C, x.needs_grad)
        self._use(x)
        if self.dry:
            return out
        idx = self._alloc((self.N, x.H // 2, x.W // 2, x.C), torch.uint8) if self.training else None
        self._emit(self.fwd, "stp_maxpool2x2", x.buf.data_ptr(), out.buf.data_ptr(), idx.data_ptr() if idx is not None else None,
                   self.N, x.H, x.W, x.C, self.cdt)

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            self._emit(self.bwd, "stp_maxpool2x2_bwd", idx.data_ptr(), out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N,
                       x.H, x.W, x.C, self.cdt, int(x.grad_ready))
            x.grad_ready = True

        if self.training:
            self._tape.append(back)
        return out

    def maxpool(self, name, x):
        Ho, Wo = (x.H + 2 - 3) // 2 + 1, (x.W + 2 - 3) // 2 + 1
        out = self._new(name, Ho, Wo, x.C, x.needs_grad)
        self._use(x)
        if self.dry:
            return out
        idx = self._alloc((self.N, Ho, Wo, x.C), torch.uint8) if self.training else None
        last = self.fwd[-1] if self.fwd else None
        if (self.training and self.dtype != "fp32" and last is not None and last[2] == "stp_bn_apply" and last[1][2] == x.buf.data_ptr()
                and last[1][1] == last[1][3] == self.cdt and last[1][5] == last[1][6] == x.C and last[1][12] == 0.0 and x.C % 8 == 0
                and x.H % 2 == 0 and x.W % 2 == 0 and x.meta.get("apply_rec") in (None, last) and not x.meta.get("sc_consumers")
                and not x.meta.get("halo_consumers") and os.environ.get("STP_FUSE_BN_POOL_FWD", "1") != "0"):
            # the BatchNormalization apply that produced x is the previous launch (the stem: bn0 -> relu0 -> pooling0): ONE launch normalises,
            # stores x (the decoder's skip tensor) and pools - the 134 MB pre-normalisation tensor is read once instead of twice
            xa = last[1]
            self.fwd.pop()
            x.meta.pop("apply_rec", None)      # (the launch no longer exists on its own: nothing may drop or move it)
            self._emit(self.fwd, "stp_bn_apply_maxpool3x3s2", xa[0], x.buf.data_ptr(), out.buf.data_ptr(), idx.data_ptr() if idx is not None else None,
                       self.N, x.H, x.W, x.C, self.cdt, xa[7], xa[8], xa[9], xa[10], xa[11])
        else:
            self._emit(self.fwd, "stp_maxpool3x3s2", x.buf.data_ptr(), out.buf.data_ptr(), idx.data_ptr() if idx is not None else None,
                       self.N, x.H, x.W, x.C, self.cdt)

        def back():
            if not (x.needs_grad and out.grad_ready):
                return
            acc = int(x.grad_ready)
            # the pool gradient completes dY of a BatchNormalization output (bn0: the other consumer is a decoder skip): OPT-IN -
            # measured: 10.06 -> 10.14 ms when on (the gather + x read + reduce in one kernel runs at half the rate of the pair)
            self._emit_grad_pass("stp_maxpool3x3s2_bwd", x, acc, (self.N, x.H, x.W, x.C, self.cdt),
                                 (idx.data_ptr(), out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.C, self.cdt, acc),
                                 os.environ.get("STP_FUSE_POOL_BN", "0") == "1")
            x.grad_ready = True

        if self.training:
            self._tape.append(back)
        return out

    def _emit_loss(self, name, logits, target, dims, weights, tail=(), then=None):
        """The tail the loss launches on logits share: the gradient buffer (None outside training), the weights (two floats, or the
        registry's five as a host array), `... gradC, loss_scale, workspace` [, ``tail``: the arguments an entry takes behind its
        workspace], then the dynamic loss-scale multiplier.  ``then(dl)``: emits the launches that ADD to the scalars and the gradient
        of this one (stp_lovasz_softmax) - behind it and in front of stp_scale_by_device, so that the dynamic scale covers them too.
        Returns the gradient buffer."""
        dl = self._gradbuf(logits) if self.training else None
        if len(weights) == 5:
            self._loss_weights = (C.c_float * 5)(*weights)     # host array read at launch
            weights = (C.addressof(self._loss_weights),)
        else:
            weights = tuple(float(w) for w in weights)
        self._emit(self.fwd, name, logits.buf.data_ptr(), target.buf.data_ptr(), *dims, self.cdt, *weights, self.loss_scalars.data_ptr(),
                   dl.data_ptr() if dl is not None else None, logits.gradC, float(self.loss_scale), self.ws_loss.data_ptr(),
                   self.ws_loss.numel() * 4, *tail)
        if then is not None:
            then(dl)
        if self.training and self.dls is not None:
            self._emit(self.fwd, "stp_scale_by_device", dl.data_ptr(), logits.rows * logits.gradC, self.cdt, self.dls.data_ptr(), self.dls.data_ptr() + 16)
        return dl

    def _emit_confusion(self, rows, target, factor=0, ignore_label=None):
        """With ``class_metrics`` on: the confusion launch of a multi-class head into ``class_counts``.  ``rows``: the tensor the argmax
        runs over - at the mask's resolution, or (``factor``) the logits held at 1 / factor of it (stp_class_confusion_up).
        ``ignore_label`` (not None: the masked loss, -1 = class weights alone): stp_class_confusion_ignore, full resolution only."""
        if not self.class_metrics:
            return
        classes = rows.C
        nb = int(self.lib.stp_class_confusion_workspace_bytes(classes))
        if nb <= 0:
            raise StpShapeError("class metrics need a head of 2..32 classes")
        self.class_counts = self._alloc((classes * classes,), torch.int32)
        ws = self._alloc((nb // 4,), torch.int32)
        if factor:
            self._emit(self.fwd, "stp_class_confusion_up", rows.buf.data_ptr(), target.buf.data_ptr(), self.N, rows.H, rows.W, factor, classes,
                       rows.C, self.cdt, self.class_counts.data_ptr(), ws.data_ptr(), nb)
        elif ignore_label is not None:
            self._emit(self.fwd, "stp_class_confusion_ignore", rows.buf.data_ptr(), target.buf.data_ptr(), rows.rows, classes, rows.C, self.cdt,
                       self.class_counts.data_ptr(), ws.data_ptr(), nb, int(ignore_label))
        else:
            self._emit(self.fwd, "stp_class_confusion", rows.buf.data_ptr(), target.buf.data_ptr(), rows.rows, classes, rows.C, self.cdt,
                       self.class_counts.data_ptr(), ws.data_ptr(), nb)

    def sigmoid_loss(self, logits, target, w_bce, w_dice, w_iou=0.0, w_jaccard=0.0, w_focal=0.0, w_lovasz=0.0):
        """sigmoid + w_bce*binary_crossentropy + w_dice*dice_loss [+ w*iou_loss + w*jaccard_loss + w*focal_loss + w*lovasz_loss,
        the rest of the registry at reference segmentation.py:15-22]; seeds the backward pass.  ``Plan.border_weights`` (set before
        define, as loss_scale is; the parameter list above stays): the cross-entropy weighted by the U-Net border weight map of the
        target (_border_weighted_loss); None: the plan of before."""
        if logits.C != 1:
            raise StpShapeError("binary loss expects one class")
        if self.dry:
            return
        self.loss_scalars = self._alloc((16,), torch.float32)
        self.loss_scalars.zero_()
        count = logits.rows
        if self.border_weights:
            self._border_weighted_loss(logits, target, w_bce, w_dice, w_iou or w_jaccard or w_focal or w_lovasz)
            return
        if w_iou or w_jaccard or w_focal:
            dl = self._emit_loss("stp_sigmoid_loss_ex", logits, target, (count,), (w_bce, w_dice, w_iou, w_jaccard, w_focal))
        else:
            dl = self._emit_loss("stp_sigmoid_bce_dice", logits, target, (count,), (w_bce, w_dice))
        # the class convolution reads its bias gradient from the gradient kernel's per-workgroup sums (not when another launch
        # adds to / rescales the gradient afterwards)
        logits.meta["loss_bias_grad"] = bool(self.training and not w_lovasz and self.dls is None)
        if w_lovasz:      # per-image Lovasz hinge: ADDS to scalars[0] and to the gradient the launch above wrote
            if self.training and self.loss_scale != 1.0:
                raise StpShapeError("lovasz_loss has no loss-scaling form: use loss_scale=1 (or bf16) with it")
            nbytes = int(self.lib.stp_lovasz_workspace_bytes(count, self.N))
            if nbytes <= 0:
                raise StpShapeError("lovasz_loss: the sort workspace cannot be sized (no device)")
            self.ws_lovasz = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._emit(self.fwd, "stp_lovasz_hinge", logits.buf.data_ptr(), target.buf.data_ptr(), self.N, count // self.N, self.cdt,
                       float(w_lovasz), self.loss_scalars.data_ptr(), dl.data_ptr() if dl is not None else None, logits.gradC,
                       self.ws_lovasz.data_ptr(), nbytes)
        logits.grad_ready = self.training

    def _border_weighted_loss(self, logits, target, w_bce, w_dice, other_terms):
        """``Plan.border_weights`` = {"w0", "sigma", "radius", "class_balance": (b0, b1)}: the one-class loss with the cross-entropy
        weighted by the U-Net border weight map of the step's own (augmented) target, computed on the device (include/stp_hip.h has the
        arithmetic).  In this order: N x stp_mask_label (connectivity 2, one per sample, one shared workspace and count word) into one
        [N][H][W] label buffer, one stp_border_weight, then stp_sigmoid_bce_dice_weighted through _emit_loss.  The weighted gradient pass
        leaves no per-workgroup sums, so the class convolution takes its bias gradient the general way."""
        if other_terms:
            raise StpShapeError("border_weights weight binary_crossentropy only: the loss may name binary_crossentropy and dice_loss")
        bw = self.border_weights
        H, W = target.H, target.W
        if target.C != 1 or self.N * H * W != logits.rows:
            raise StpShapeError("border_weights need a one-channel mask at the logits' resolution")
        n_label = int(self.lib.stp_mask_label_workspace_bytes(H, W))
        n_weight = int(self.lib.stp_border_weight_workspace_bytes(self.N, H, W))
        if n_label <= 0 or n_weight <= 0:
            raise StpShapeError("border_weights: the label / weight workspace cannot be sized for %d x %d x %d" % (self.N, H, W))
        self.border_labels = self._alloc((self.N, H, W), torch.int32)
        self.border_map = self._alloc((self.N, H, W), torch.float32)
        self.border_count = self._alloc((4,), torch.int32)
        ws_label = self._alloc(((n_label + 7) // 8,), torch.int64)
        ws_weight = self._alloc(((n_weight + 7) // 8,), torch.int64)
        for n in range(self.N):
            self._emit(self.fwd, "stp_mask_label", target.buf.data_ptr() + n * H * W, H, W, 2, 0, self.border_labels.data_ptr() + 4 * n * H * W,
                       self.border_count.data_ptr(), ws_label.data_ptr(), ws_label.numel() * 8)
        b0, b1 = bw["class_balance"]
        self._emit(self.fwd, "stp_border_weight", self.border_labels.data_ptr(), self.N, H, W, float(bw["w0"]), float(bw["sigma"]),
                   int(bw["radius"]), float(b0), float(b1), self.border_map.data_ptr(), None, None, ws_weight.data_ptr(), ws_weight.numel() * 8)
        self._emit_loss("stp_sigmoid_bce_dice_weighted", logits, target, (logits.rows,), (w_bce, w_dice), tail=(self.border_map.data_ptr(),))
        logits.meta["loss_bias_grad"] = False
        logits.grad_ready = self.training

    def sigmoid_multilabel_loss(self, logits, target, w_bce, w_dice, w_iou=0.0, w_jaccard=0.0, w_focal=0.0):
        """Multi-label head (classes: C = 2..8, activation: sigmoid): C independent sigmoids and the weighted sum of
        binary_crossentropy, dice_loss, iou_loss, jaccard_loss, focal_loss over the [pixels, C] tensor; target = one byte per
        pixel, bit c = class c.  Seeds the backward pass."""
        if not 2 <= logits.C <= 8:
            raise StpShapeError("multi-label loss expects 2..8 classes")
        if self.dry:
            return
        self.loss_scalars = self._alloc((16,), torch.float32)
        self.loss_scalars.zero_()
        self._emit_loss("stp_sigmoid_multilabel_loss", logits, target, (logits.rows, logits.C, logits.C), (w_bce, w_dice, w_iou, w_jaccard, w_focal))
        # the class convolution reads its C bias gradients from the gradient pass's per-workgroup, per-class sums (not when
        # stp_scale_by_device rescales the gradient afterwards)
        logits.meta["loss_bias_grad"] = "multilabel" if (self.training and self.dls is None) else False
        logits.grad_ready = self.training

    def softmax_loss(self, logits, target, w_cce, w_dice, w_iou=0.0, w_jaccard=0.0, w_focal=0.0):
        """channel softmax + w_cce*categorical_crossentropy + w_dice*dice_loss [+ w*iou_loss + w*jaccard_loss + w*focal_loss on the
        one-hot target: stp_softmax_loss_ex] (target = class index per pixel).  ``Plan.masked_loss`` = {"ignore_label": 0..255 or None,
        "class_weights": one positive float per class or None} (set before define, as loss_scale is; the parameter list above is
        pinned by tests/test_softmax_losses_host.py): stp_softmax_loss_masked (include/stp_hip.h has the arithmetic); None: the plan
        of before.  ``Plan.lovasz_softmax`` (a weight, set the same way; 0: the plan of before): the extended full-resolution branch with
        one stp_lovasz_softmax launch directly behind the loss launch."""
        if logits.C < 2:
            raise StpShapeError("categorical loss expects at least two classes")
        if self.dry:
            return
        opts = self.masked_loss or {}
        ignore_label, class_weights = opts.get("ignore_label"), opts.get("class_weights")
        masked = ignore_label is not None or class_weights is not None
        w_lovasz = float(self.lovasz_softmax or 0.0)
        if masked or w_iou or w_jaccard or w_focal or w_lovasz:
            # one launch on the full-resolution logits: the extended loss, masked or not, has no low-resolution (_up) form, so FPN /
            # PSPNet keep their stp_resize_bilinear and its gradient launch
            name, tail, ign = "stp_softmax_loss_ex", (), None
            if masked:
                # the weights live in a plan-owned device tensor filled here
                if logits.C > 32:
                    raise StpShapeError("ignore_label / class_weights need a head of 2..32 classes")
                ign = -1 if ignore_label is None else int(ignore_label)
                cw = None
                if class_weights is not None:
                    if len(class_weights) != logits.C:
                        raise StpShapeError("class_weights: %d weights for %d classes" % (len(class_weights), logits.C))
                    cw = self._alloc((logits.C,), torch.float32)
                    cw.copy_(torch.tensor([float(w) for w in class_weights], dtype=torch.float32))
                self.class_weights = cw
                name, tail = "stp_softmax_loss_masked", (ign, cw.data_ptr() if cw is not None else None)
            self.loss_scalars = self._alloc((16,), torch.float32)
            self.loss_scalars.zero_()
            then = None
            if w_lovasz:
                # Lovasz-Softmax: ADDS to scalars[0] and to the gradient the launch above wrote (include/stp_hip.h has the arithmetic); the
                # static loss scale goes in as its grad_scale, class weights do not enter it
                nbytes = int(self.lib.stp_lovasz_softmax_workspace_bytes(logits.rows, logits.C))
                if nbytes <= 0:
                    raise StpShapeError("lovasz_softmax: the sort workspace cannot be sized (2..32 classes, pixels * classes < 2^31, a device)")
                self.ws_lovasz = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

                def then(dl):
                    self._emit(self.fwd, "stp_lovasz_softmax", logits.buf.data_ptr(), target.buf.data_ptr(), logits.rows, logits.C, logits.C,
                               self.cdt, w_lovasz, self.loss_scalars.data_ptr(), dl.data_ptr() if dl is not None else None, logits.gradC,
                               float(self.loss_scale), -1 if ignore_label is None else int(ignore_label), self.ws_lovasz.data_ptr(), nbytes)
            self._emit_loss(name, logits, target, (logits.rows, logits.C, logits.C), (w_cce, w_dice, w_iou, w_jaccard, w_focal), tail=tail,
                            then=then)
            if w_lovasz:
                logits.meta["loss_bias_grad"] = False      # a later launch adds to the gradient: no bias gradient from the first one's workgroup sums
            self._emit_confusion(logits, target, ignore_label=ign)
            logits.grad_ready = self.training
            return
        self.loss_scalars = self._alloc((12,), torch.float32)
        rec = logits.meta.get("resize_rec")
        if (self.training and rec is not None and self.fwd[rec[0]][2] == "stp_resize_bilinear" and rec[1].needs_grad
                and not rec[1].grad_ready and target.buf.data_ptr() % 4 == 0
                and self.lib.stp_softmax_cce_dice_up_ok(rec[2], logits.C, self.cdt)
                and (not self.class_metrics or self.lib.stp_class_confusion_up_ok(rec[2], logits.C, self.cdt))):
            # the logits are a bilinear resize of the class convolution's output (PSPNet, FPN) and only this loss reads them: both loss passes
            # interpolate from the low-resolution tensor, the gradient pass reduces straight into its gradient - the resized logits, their
            # gradient, the resize launch, stp_scale_by_device and stp_resize_bilinear_bwd leave the step (the launch record is kept for
            # HipSegModel.logits(), which materialises the resized tensor on demand)
            idx, lo, f = rec
            logits.meta["deferred"] = (self.fwd[idx][0], self.fwd[idx][1], self.fwd[idx][2])
            self.fwd[idx] = (None, (), "fused:resize->loss", None)
            nb = int(self.lib.stp_softmax_cce_dice_up_corner_bytes(self.N, lo.H, lo.W, logits.C))
            corners = self._alloc((nb // 4,), torch.float32)
            dlow = self._gradbuf(lo)
            dls = self.dls.data_ptr() if self.dls is not None else None
            self._emit(self.fwd, "stp_softmax_cce_dice_up", lo.buf.data_ptr(), target.buf.data_ptr(), self.N, lo.H, lo.W, f, logits.C, lo.C,
                       self.cdt, float(w_cce), float(w_dice), self.loss_scalars.data_ptr(), dlow.data_ptr(), lo.gradC, float(self.loss_scale),
                       dls, (dls + 16) if dls is not None else None, self.ws_loss.data_ptr(), self.ws_loss.numel() * 4, corners.data_ptr(), nb)
            self._emit_confusion(lo, target, f)       # on the same low-resolution tensor: the resized logits stay out of the step
            lo.grad_ready = True
            logits.grad_ready = False
            logits.meta["fused_into_loss"] = True
            return
        self._emit_loss("stp_softmax_cce_dice", logits, target, (logits.rows, logits.C, logits.C), (w_cce, w_dice))
        self._emit_confusion(logits, target)
        logits.grad_ready = self.training

    def softmax_out(self, logits):
        """Activation('softmax') of the head for inference: float32 probabilities."""
        if self.dry:
            return None
        probs = self._alloc((logits.N, logits.H, logits.W, logits.C), torch.float32)
        self._emit(self.fwd, "stp_softmax", logits.buf.data_ptr(), probs.data_ptr(), logits.rows, logits.C, logits.C, self.cdt)
        self.probs = probs
        return probs

    def sigmoid_out(self, logits):
        """Activation('sigmoid') of the head for inference: float32 probabilities."""
        if self.dry:
            return None
        probs = self._alloc((logits.N, logits.H, logits.W, logits.C), torch.float32)
        self._emit(self.fwd, "stp_sigmoid", logits.buf.data_ptr(), probs.data_ptr(), logits.rows * logits.C, self.cdt)
        self.probs = probs
        return probs

    # ------------------------------------------------------------------ execution
    def run(self, launches):
        if self.device.type != "cuda":
            raise _lib.StpError("plans execute on the GPU only (no CPU fallback)")
        st = torch.cuda.current_stream().cuda_stream
        for fn, args, name, _meta in launches:
            if fn is None:                      # the forward's "fused:resize->loss" marker: a name for inspection, no launch
                continue
            rc = fn(*args, st)
            if rc != 0:
                _lib.check(rc, name)

    # loss launches whose third argument is the element / pixel count of the batch ([N, ...] -> the first n_valid samples)
    LOSS_LAUNCHES = ("stp_sigmoid_bce_dice", "stp_softmax_cce_dice", "stp_prob_bce_dice", "stp_sigmoid_loss_ex", "stp_prob_cce_dice",
                     "stp_sigmoid_multilabel_loss", "stp_softmax_loss_ex", "stp_softmax_loss_masked", "stp_sigmoid_bce_dice_weighted")

    def rerun_loss(self, n_valid):
        """Re-evaluates the loss / metric reduction over the first ``n_valid`` samples only (an evaluation batch whose tail
        was filled by wrapping around: the duplicates must not enter val_loss / dice - Keras evaluates a short last batch
        as it is).  Samples are the slowest dimension of every tensor, so the real ones are a prefix of the element range.
        ``stp_lovasz_hinge`` ADDS its term to the scalars the first launch wrote, so it is re-run after it with
        ``images = n_valid`` (its third argument).  The confusion launch behind the loss (``class_metrics``) is re-run the same way
        (``rerun_confusion``): its third argument is the pixel count (``stp_class_confusion``, ``_ignore``) or the image count (``_up``), and every
        call overwrites the counts."""
        n_valid = int(n_valid)
        if not 0 < n_valid <= self.N:
            raise ValueError("n_valid out of range")
        st = torch.cuda.current_stream().cuda_stream
        done = False
        for fn, args, name, _meta in self.fwd:
            if name in self.LOSS_LAUNCHES and not done:
                a = list(args)
                a[2] = args[2] // self.N * n_valid        # element / pixel count: [N, ...] -> [n_valid, ...]
                _lib.check(fn(*a, st), name)
                done = True
            elif name == "stp_lovasz_hinge" and done:
                a = list(args)
                a[2] = n_valid                            # images
                _lib.check(fn(*a, st), name)
            elif name == "stp_lovasz_softmax" and done:   # ADDS its term to the scalars the first launch wrote: re-run behind it
                a = list(args)
                a[2] = args[2] // self.N * n_valid        # pixels
                _lib.check(fn(*a, st), name)
        if not done:
            raise _lib.StpError("the plan has no loss launch")
        self.rerun_confusion(n_valid)

    def rerun_confusion(self, n_valid):
        """Re-runs the confusion launch (``class_metrics``) over the first ``n_valid`` samples: ``class_counts`` then holds the real
        samples of a padded batch alone.  It reads the head's output as the step left it; a plan without the launch does nothing."""
        n_valid = int(n_valid)
        if not 0 < n_valid <= self.N:
            raise ValueError("n_valid out of range")
        st = torch.cuda.current_stream().cuda_stream
        for fn, args, name, _meta in self.fwd:
            if name in ("stp_class_confusion", "stp_class_confusion_up", "stp_class_confusion_ignore"):
                a = list(args)
                a[2] = n_valid if name.endswith("_up") else args[2] // self.N * n_valid      # images / pixels
                _lib.check(fn(*a, st), name)

    def init_states(self):
        for name, (off, numel, init) in self.states.items():
            self.S[off:off + numel] = init

    def set_trainable_mask(self):
        self.mask.fill_(1)
        for info in self.params.values():
            if not info.trainable:
                self.mask[info.offset:info.offset + info.numel] = 0


class Dgrad(object):
    """What ConvLayer's data-gradient chooser settled on: the launch parameters ``q`` and what the chosen form did with the layer."""

    def __init__(self, q, layer, s2d=False, fold1=False, folded_up=False, two_dest=False, collapsed=False):
        self.q, self.s2d, self.fold1, self.folded_up, self.two_dest = q, s2d, fold1, folded_up, two_dest
        # (the class-collapsed form leaves the skip's gradient to a launch of its own: this one serves the first C0 channels only)
        self.C1 = 0 if collapsed else layer.C1
        self.flops = layer.flops * (layer.C0 - 0.0) / (layer.C0 + layer.C1) if collapsed else layer.flops


# The plan of ONE convolution - one Plan.conv call, which documents the arguments: the layer's geometry and operands as attributes, one
# method per planning step.  The constructor and `declare` run in both passes of Plan.define, `forward` in the real pass, `backward` from
# the tape, in backward order.  Order is behaviour here: _gptr calls feed bwd_marks, _gradbuf calls may issue the pending weight-gradient
# group, so every call stays at its point of the launch list.
class ConvLayer(object):

    def __init__(self, plan, name, x, Cout, k, stride, pad, src1, upsample, residual, transpose, relu, same_tf, fold_shortcut, param_cols):
        """Validates the operands; derives padding, the virtual input size (Hv, Wv), the output size and the channel counts."""
        if transpose:
            if stride != 1 or upsample or src1 is not None or residual is not None or k % 2:
                raise StpShapeError("transpose=True is the plain stride-2 'same' Conv2DTranspose with an even kernel")
            pad = k - 1 - (k // 2 - 1)
        real_c0 = x.meta.get("real_c", x.C)
        stem = real_c0 != x.C
        if stem and (src1 is not None or upsample):
            raise StpShapeError("padded-channel input supports a plain conv only")
        C0, C1 = x.C, (src1.C if src1 is not None else 0)
        if not stem and (C0 % plan.vec or C1 % plan.vec):
            raise StpShapeError("%s: input channels (%d,%d) must be multiples of %d for dtype %s" % (name, C0, C1, plan.vec, plan.dtype))
        Hv, Wv = (2 * x.H, 2 * x.W) if upsample else ((2 * x.H - 1, 2 * x.W - 1) if transpose else (x.H, x.W))
        if src1 is not None and (src1.H, src1.W) != (Hv, Wv):
            raise StpShapeError("%s: skip tensor is %dx%d, expected %dx%d" % (name, src1.H, src1.W, Hv, Wv))
        Ho, Wo = (Hv + 2 * pad - k) // stride + 1, (Wv + 2 * pad - k) // stride + 1
        if same_tf:
            # TF / Keras padding='same': ceil(size / stride) outputs, the odd padding pixel goes to the bottom / right.  The
            # kernels take the top/left padding and the output size; taps past the far edge are out of bounds = zero.
            Ho, Wo = -(-Hv // stride), -(-Wv // stride)
            pad = max((Ho - 1) * stride + k - Hv, 0) // 2
            if max((Wo - 1) * stride + k - Wv, 0) // 2 != pad:
                raise StpShapeError("%s: 'same' padding differs between height and width" % name)
        self.KWp = k + (k & 1) if (stem and x.C == 4) else k      # 4 padded channels: one 16-byte vector = two horizontally adjacent taps
        self.plan, self.name, self.x, self.src1, self.residual, self.fs, self.param_cols = plan, name, x, src1, residual, fold_shortcut, param_cols
        self.Cout, self.k, self.stride, self.pad, self.upsample, self.transpose, self.relu = Cout, k, stride, pad, upsample, transpose, relu
        self.real_c0, self.stem, self.C0, self.C1, self.Hv, self.Wv, self.Ho, self.Wo = real_c0, stem, C0, C1, Hv, Wv, Ho, Wo
        self.Cin_master, self.Cinp = real_c0 + C1, C0 + C1
        self.src_mode = ops.SRC_NEAREST2X if upsample else (ops.SRC_ZEROINS2X if transpose else ops.SRC_DIRECT)

    def declare(self, param_name, param_shape, cout_pad, bias):
        """Parameters, the output tensor, and what the dry pass sizes: the weight-gradient and bias-gradient workspaces."""
        pl, name, x, src1, residual, Cout, k, Cin_master, param_cols = self.plan, self.name, self.x, self.src1, self.residual, self.Cout, self.k, self.Cin_master, self.param_cols
        # (param_name / param_shape: conv3x3_taps - the 1x1 launch over the bytes of a 3x3 kernel registered under the layer's own name)
        if param_cols is not None:
            if k != 1 or self.stem or self.transpose or self.C1 or Cout % pl.vec or Cin_master % 4 or param_cols[0] % 4 or param_cols[1] % 4 \
                    or param_cols[0] + Cin_master > param_cols[1]:
                raise StpShapeError("%s: a column range of a shared kernel serves a plain 1x1 convolution with aligned channel counts" % name)
            param_shape = None
        w = pl.param((param_name or name) + "/kernel", (Cout, 1, 1, param_cols[1]) if param_cols is not None else (param_shape or (Cout, k, k, Cin_master)),
                     "tkernel" if self.transpose else "kernel")
        if param_shape is not None and int(np.prod(param_shape)) != Cout * k * k * Cin_master:
            raise StpShapeError("%s: parameter view of %s does not match %d x %d x %d x %d" % (name, param_shape, Cout, k, k, Cin_master))
        self.w, self.b = w, (pl.param(name + "/bias", (Cout,), "bias") if bias else None)
        CoutB = self.CoutB = _rup(Cout, cout_pad or pl.vec)      # channels of the gradient buffer = K of the data gradient (cout_pad: conv3x3_taps)
        self.x_ng, self.s_ng = x.needs_grad, (src1.needs_grad if src1 is not None else False)
        self.out = pl._new(name, self.Ho, self.Wo, Cout, self.x_ng or self.s_ng or w.trainable or (residual is not None and residual.needs_grad))
        self.out.gradC = CoutB
        if bias:
            pl._bn_ws_c = max(pl._bn_ws_c, CoutB)      # the bias gradient (stp_channel_sum) shares the BN workspace
        pl._use(x, src1, residual)
        # workspace sizing needs the wgrad plan: query the library (cheap, host only)
        wp = self.wp = _lib.WgradParams()
        wp.N, wp.Hs0, wp.Ws0, wp.Hv, wp.Wv, wp.C0, wp.C1, wp.src0_mode = pl.N, x.H, x.W, self.Hv, self.Wv, self.C0, self.C1, self.src_mode
        wp.KH, wp.KW, wp.stride, wp.pad, wp.Ho, wp.Wo, wp.Cout = k, self.KWp, self.stride, self.pad, self.Ho, self.Wo, CoutB
        wp.accumulate, wp.dtype, wp.splits = 0, pl.cdt, 0
        if pl.training and w.trainable:
            pl._wg_ws_bytes = max(pl._wg_ws_bytes, int(pl.lib.stp_conv2d_wgrad_workspace_bytes(C.byref(wp))))

    # ------------------------------------------------------------------ forward
    def forward(self, bn_stats, flops_as):
        """Weight copies, the launch parameters with their epilogue (bias, ReLU, statistics), the launch."""
        pl, x, src1, residual, out, k, Cout = self.plan, self.x, self.src1, self.residual, self.out, self.k, self.Cout
        self._weight_copies()
        p = self.p = ops.conv_params(x.buf, self.wf, out.buf, N=pl.N, Hs0=x.H, Ws0=x.W, Hv=self.Hv, Wv=self.Wv, C0=self.C0, C1=self.C1,
                                     src1=src1.buf if src1 is not None else None,
                                     mode=self.src_mode, KH=k, KW=self.KWp, stride=self.stride, pad=self.pad,
                                     Ho=self.Ho, Wo=self.Wo, Cout=Cout, dtype=pl.cdt, residual=residual.buf if residual is not None else None)
        self._collapsed_copies()
        self._register_bn_consumer()
        if self.b is not None:
            p.bias = pl._pptr(self.b)
        if self.relu:
            if self.CoutB != Cout:
                raise StpShapeError("%s: a fused ReLU needs Cout to be a multiple of %d" % (self.name, pl.vec))
            p.relu = 1        # Conv2D(activation='relu'): fused into the epilogue; its gradient masks dY first (stp_relu_bwd)
        if bn_stats and pl.training and pl.slot_arena is not None and pl.N * self.Ho * self.Wo <= pl.bn_slots_max_rows:
            p.stats_partial, p.stats_slots = out.meta["stats_slots"] = pl._slots(Cout)
        elif bn_stats and pl.training:
            # the BatchNormalization that follows takes its batch statistics from this conv's epilogue
            nfl = int(pl.lib.stp_conv2d_stats_floats(C.byref(p)))
            st = pl._alloc((max(nfl, 4),), torch.float32)
            p.stats_partial = st.data_ptr()
            out.meta["stats_table"] = pl._group_stats(p, st, Cout)       # (table, columns) the BatchNormalization reads
        # algorithmic work of this layer: 2 * pixels * Cout * KH*KW*Cin with the REAL (unpadded) dims
        self.flops = 2.0 * pl.N * self.Ho * self.Wo * Cout * k * k * self.Cin_master / (4.0 if self.transpose else 1.0)   # zero-inserted taps are not work
        if flops_as is not None:
            # (a launch of a RESTRUCTURED reference layer - the PSPNet head without its concatenation: the roofline bookkeeping keeps
            #  counting the reference graph's convolution, SURVEY 8d's convention, not the cheaper form that is executed)
            self.flops = float(flops_as)
        pl._emit_conv(pl.fwd, p, {"layer": self.name, "pass": "fwd", "flops": self.flops, "tile": int(pl.lib.stp_conv2d_tile_for(C.byref(p))),
                                  "src2": bool(self.C1 or self.upsample)})

    def _weight_copies(self):
        """The forward and data-gradient compute copies of the kernel, rebuilt from the fp32 master once per step."""
        pl, w, Cout, k, KWp, Cinp, Cin_master, param_cols = self.plan, self.w, self.Cout, self.k, self.KWp, self.Cinp, self.Cin_master, self.param_cols
        wf = self.wf = pl._alloc((_rup(Cout, 16) * k * KWp * Cinp,))
        self.need_dgrad = pl.training and (self.x_ng or self.s_ng) and not self.stem
        wb = self.wb = pl._alloc((_rup(Cinp, 16) * k * k * self.CoutB,)) if self.need_dgrad else None
        self.out.meta["wb"] = wb
        wsrc = pl._pptr(w)
        if param_cols is not None:
            w.pending_slices += 1      # (backward: the LAST range written makes the parameter's gradient final)
            # the column range as a dense [Cout][Cin] fp32 matrix, refreshed every step in front of the batched weight preparation
            wm = pl._alloc((Cout * Cin_master,), torch.float32)
            pl._emit(pl.prep, "stp_copy_cols_f32", wm.data_ptr(), Cin_master, wsrc + 4 * int(param_cols[0]), int(param_cols[1]), Cout, Cin_master, 0)
            wsrc = wm.data_ptr()
        self.out.meta["w_master"] = (wsrc, Cout, Cin_master, k)      # (the space-to-depth data gradient builds its weights from the masters)
        # collected here, issued as ONE batched launch per step (see _finish_prep)
        pl._prep_layers.append((wsrc, wf.data_ptr(), wb.data_ptr() if wb is not None else None, Cout, k, k, Cin_master, KWp, Cinp, self.CoutB))

    def _collapsed_copies(self):
        """The class-collapsed weight copies of a convolution over upsample + concat, where its kernel takes them."""
        pl, p, C0, C1, rows_f = self.plan, self.p, self.C0, self.C1, _rup(self.Cout, 16)
        self.w4 = None
        if not (self.upsample and self.src1 is not None and self.k == 3 and self.KWp == 3 and self.stride == 1 and self.pad == 1
                and self.Cinp == self.Cin_master == C0 + C1
                and os.environ.get("STP_UPCOLLAPSE", "1") != "0" and not pl.lib.stp_conv2d_scn_eligible(C.byref(p))
                and int(pl.lib.stp_conv2d_halo_variant(C.byref(p))) < 0):
            # (the narrow-output kernel - 64 + 64 -> 32 channels - keeps both halos in LDS and takes the plain weight copy; so does the
            #  two-source form of the halo kernel, round 5: 128+ output channels)
            return
        # decoder conv1 = conv3x3(concat(UpSampling2D(2)(x), skip)): per output parity class the taps over the upsampled half read
        # 2 x 2 low-resolution pixels - the forward multiplies them by class-summed weights (4 x C0 + 9 x C1 K columns instead
        # of 9 x (C0 + C1)); the summed copy is rebuilt from the fp32 master with the other weight copies, once per step
        wup = pl._alloc((rows_f * 16 * C0,))
        pl._upc_layers.append((pl._pptr(self.w), wup.data_ptr(), self.Cout, rows_f, C0, C0 + C1))     # one batched launch (_finish_prep)
        p.weight_up = wup.data_ptr()
        if self.need_dgrad and self.x_ng and C0 % 16 == 0 and os.environ.get("STP_UPCOLLAPSE_BWD", "0") == "1":
            # ... and the data gradient w.r.t. x is a 4x4 / stride-2 convolution of dY with the row / column tap sums.  OPT-IN:
            # measured slower with today's kernels for the two resulting shapes, kept for the next round
            self.w4 = pl._alloc((C0 * 16 * self.CoutB,))
            pl._upc4_layers.append((pl._pptr(self.w), self.w4.data_ptr(), self.Cout, self.CoutB, C0, C0 + C1))

    def _register_bn_consumer(self):
        """Tells the BatchNormalization that produces ``x`` that this launch can normalise ``x`` itself (_fuse_bn_into_consumers)."""
        pl, x, p, wp, w = self.plan, self.x, self.p, self.wp, self.w
        if not pl.training or x.meta.get("apply_rec") is None or self.src1 is not None or self.transpose or self.stem:
            return
        if self.residual is None and pl.lib.stp_conv2d_sc_eligible(C.byref(p)) and (not w.trainable or pl.lib.stp_wgrad_sc_eligible(C.byref(wp))):
            x.meta["sc_consumers"].append((p, wp))
        elif pl.fuse_bn_halo and not self.upsample and pl.lib.stp_conv2d_halo_variant(C.byref(p)) >= 0:
            # (p, wp, can the weight gradient normalise its operand itself: row-of-taps kernel - or no weight gradient at all)
            x.meta["halo_consumers"].append((p, wp, (not w.trainable) or int(pl.lib.stp_conv2d_wgrad_kernel_id(C.byref(wp))) in (2, 3)))

    # ------------------------------------------------------------------ backward
    def backward(self):
        """Backward entry (ReLU mask, residual gradient), then the weight, bias and data gradients."""
        pl, out, residual, b = self.plan, self.out, self.residual, self.b
        if not out.needs_grad or not out.grad_ready:
            return
        dy = self.dy = out.grad
        if self.relu:
            pl._guard_write(dy)
            pl._emit(pl.bwd, "stp_relu_bwd", out.buf.data_ptr(), dy.data_ptr(), out.rows * out.gradC, pl.cdt)
        # residual branch: d(residual) = dY
        if residual is not None and residual.needs_grad:
            if not residual.grad_ready and residual.gradC == out.gradC:
                residual.grad = dy          # alias: dY is dead once this layer's backward has been issued
                residual.grad_ready = True
            else:
                pl._emit(pl.bwd, "stp_add_inplace", pl._gradbuf(residual).data_ptr(), dy.data_ptr(), out.rows * out.gradC, pl.cdt)
        if self.w.trainable:
            self._weight_grad()
        if b is not None and b.trainable and out.meta.get("loss_bias_grad") and self.Cout == 1:
            # the 1-class head: the loss gradient kernel left the per-workgroup sums of dL/dlogit in its workspace
            pl._emit(pl.bwd, "stp_sigmoid_loss_bias_grad", pl.ws_loss.data_ptr(), out.rows, pl._gptr(b), 0)
        elif b is not None and b.trainable and out.meta.get("loss_bias_grad") == "multilabel":
            # the multi-label head: one partial sum per class and gradient workgroup, left by stp_sigmoid_multilabel_loss
            pl._emit(pl.bwd, "stp_sigmoid_multilabel_bias_grad", pl.ws_loss.data_ptr(), out.rows, self.Cout, pl._gptr(b), 0)
        elif b is not None and b.trainable:
            pl._emit_bias_grad(dy, out.rows, self.CoutB, self.Cout, b)
        if self.need_dgrad and not out.meta.get("dgrad_folded"):
            # (folded: a projection shortcut whose data gradient rode in its sibling's launch - fold_shortcut: nothing to issue)
            self._data_grad()

    # weight gradient: issued here (dY is final), or collected into the pending group, which is issued before any kernel
    # rewrites a dY it reads (_guard_write) and at the end of the launch list at the latest
    def _weight_grad(self):
        """Destination (the arena, or a padded / column-range matrix), the launch - grouped or alone - and the copy back from such a matrix."""
        pl, x, src1, w, wp, k, Cout, Cin_master, param_cols = self.plan, self.x, self.src1, self.w, self.wp, self.k, self.Cout, self.Cin_master, self.param_cols
        padded, gcols = self.stem or self.CoutB != Cout, None
        if padded:
            dwp = pl._alloc((self.CoutB * k * self.KWp * self.Cinp,), torch.float32)
            wp.dw = dwp.data_ptr()
        elif param_cols is not None:
            gcols = pl._alloc((Cout * Cin_master,), torch.float32)       # dense gradient of the column range, copied back below
            wp.dw = gcols.data_ptr()
        else:
            wp.dw = pl._gptr(w)
        wp.src0, wp.src1, wp.dy = x.meta.get("src_override") or x.buf.data_ptr(), (src1.buf.data_ptr() if src1 is not None else None), self.dy.data_ptr()
        cls = int(pl.lib.stp_wgrad_group_class(C.byref(wp))) if (pl.wgrad_group_gflop > 0 and not padded and gcols is None) else 0
        if cls:
            self._wgrad_join_group(cls)
        else:
            # a layer outside the groups (stride 2, 1x1, stem, small-channel): the pending group is issued first, so a group
            # = consecutive row-of-taps layers (a network stage) and the gradient arena stays final above the last visited layer
            pl._flush_wgroup()
            # (a padded dW is unpadded right below)
            pl._emit_wgrad(wp, self.name, self.flops, defer_hi=0 if (padded or gcols is not None) else w.end)
        if gcols is not None:
            # (the arena range of the shared kernel is reported final - _gptr, bwd_marks - by the last of its ranges only)
            w.pending_slices -= 1
            gbase = pl._gptr(w) if w.pending_slices == 0 else pl.G.data_ptr() + 4 * w.offset
            pl._emit(pl.bwd, "stp_copy_cols_f32", gbase + 4 * int(param_cols[0]), int(param_cols[1]), gcols.data_ptr(), Cin_master, Cout, Cin_master, 0)
        if padded:
            pl._emit(pl.bwd, "stp_weight_grad_unpad", dwp.data_ptr(), pl._gptr(w), Cout, k, k, Cin_master, self.KWp, self.Cinp, 0)
        beta = x.meta.get("input_bn_beta")
        if self.stem and beta is not None and beta.trainable:
            pl._emit(pl.bwd, "stp_stem_beta_grad", dwp.data_ptr(), pl._pptr(w), pl._gptr(beta), Cout, k, k, self.real_c0, self.KWp, self.Cinp, self.real_c0)

    # row-of-taps layer: joins the pending group (one launch per stage instead of one per layer); dY stays untouched
    # until the group is issued (_gradbuf / the BatchNormalization backward's out-of-place accumulate see to that)
    def _wgrad_join_group(self, cls):
        pl = self.plan
        if pl._wgroup and pl._wgroup_cls != cls:
            pl._flush_wgroup()
        pl._wgroup.append((self.wp, self.name, self.flops))
        pl._wgroup_cls = cls
        pl._wgroup_flops += self.flops
        pl._wgroup_hi = max(pl._wgroup_hi, self.w.end)
        pl._wgroup_reads.add(self.dy.data_ptr())
        if pl._wgroup_flops >= pl.wgrad_group_gflop * 1e9:
            pl._flush_wgroup()

    # ------------------------------------------------------------------ data gradient
    # The chooser.  The forms in the order they are tried - the first that takes the layer wins; a form that declines has issued nothing
    # and leaves the plain launch parameters `q` untouched (a candidate is built, the library is asked, and it is adopted only on a yes):
    #   scatter      1x1 / stride 2: low-resolution GEMM + scatter pass (issues its own launches: nothing else follows)
    #   s2d          3x3 / stride 2 on the halo kernel, space-to-depth; the sibling shortcut's dY rides as a second source
    #   parity fold  3x3 / stride 2, zero-inserted: the sibling shortcut's dY as one more tap of the (even, even) class
    #   fold1        3x3 / stride 1 on the halo kernel: the sibling 1x1 / stride-1 shortcut's dY as a second source
    #   collapsed    conv(concat(up(x), skip)) with STP_UPCOLLAPSE_BWD=1: 4x4 / stride-2 launch for x, a launch of its own for the skip
    #   sum2x2       conv(up(x)) / conv(concat(up(x), skip)): the 2x2 sums of UpSampling2D's gradient in the epilogue of the small-channel
    #                / wide-output kernel, else of the halo kernel (there only with the fused BatchNormalization backward)
    #   plain        `q` as it is (an upsampled source then gets its gradient from the trailing stp_upsample2x_bwd pass)
    # Then: the BatchNormalization-backward sums where this launch completes that gradient, the launch, the trailing pass.
    def _data_grad(self):
        pl, x = self.plan, self.x
        self._dgrad_dests()
        q = self._dgrad_plain()
        if self.stride not in (1, 2):
            raise StpShapeError("data gradient supports stride 1 and 2")
        if self._form_scatter():
            return
        form = (self._form_s2d() or self._form_parity_fold(q) or self._form_fold1(q) or self._form_collapsed()
                or self._form_sum2x2_stream(q) or self._form_sum2x2_halo(q) or Dgrad(q, self))
        if form.folded_up and self.d0_hires is not None:
            # the full-resolution gradient of the upsampled tensor is never written: give its buffer back (33-134 MB per decoder
            # stage at batch 16, 512 x 512 - it used to stay allocated for the life of the plan)
            pl._keep = [t for t in pl._keep if t is not self.d0_hires]
            self.d0 = self.d0_hires = None
        self._attach_bn_sums(form)
        pl._emit_conv(pl.bwd, form.q, {"layer": self.name, "pass": "dgrad", "flops": form.flops,
                                       "tile": int(pl.lib.stp_conv2d_tile_for(C.byref(form.q))), "s2d": form.s2d, "fold1": form.fold1})
        if self.upsample and self.x_ng and not form.folded_up:
            # the un-folded gradient of UpSampling2D as a pass of its own; where it completes dY of a BatchNormalization output: mask +
            # backward sums in the same pass
            acc = int(x.grad_ready)
            pl._emit_grad_pass("stp_upsample2x_bwd", x, acc, (pl.N, x.H, x.W, self.C0, self.C0, pl.cdt),
                               (self.d0.data_ptr(), pl._gradbuf(x).data_ptr(), pl.N, x.H, x.W, self.C0, self.C0, pl.cdt, acc),
                               os.environ.get("STP_FUSE_UP_BN", "1") != "0")
        if self.x_ng:
            x.grad_ready = True
        if self.s_ng:
            self.src1.grad_ready = True

    def _dgrad_dests(self):
        """Destinations (d0, d1) and accumulate flags of the data gradient; an upsampled source gets a full-resolution buffer first."""
        pl, x, src1, shape = self.plan, self.x, self.src1, (self.plan.N, self.Hv, self.Wv)
        self.d0_hires = None
        if self.upsample:
            d0 = self.d0_hires = pl._alloc(shape + (self.C0,)) if self.x_ng else None      # released when the launch folds the 2 x 2 sums
            self.acc0 = 0
        else:
            d0 = pl._gradbuf(x) if self.x_ng else None
            self.acc0 = int(x.grad_ready)
        d1 = pl._gradbuf(src1) if self.s_ng else None
        self.acc1 = int(src1.grad_ready) if self.s_ng else 0
        if d0 is None:
            d0 = pl._alloc(shape + (self.C0,))      # gradient not wanted: scratch sink
        if self.C1 and d1 is None:
            d1 = pl._alloc(shape + (self.C1,))
        self.d0, self.d1 = d0, d1

    def _dgrad_plain(self):
        """The plain form: a stride-1 convolution of (zero-inserted, for stride 2) dY with the flipped kernel copy ``wb``."""
        pl, x, k, stride, Ho, Wo, C0 = self.plan, self.x, self.k, self.stride, self.Ho, self.Wo, self.C0
        if self.transpose:
            # gradient of the zero-inserted input at its even positions only = a plain stride-2 convolution of dY
            return ops.conv_params(self.dy, self.wb, self.d0, N=pl.N, Hs0=Ho, Ws0=Wo, Hv=Ho, Wv=Wo, C0=self.CoutB, mode=ops.SRC_DIRECT, KH=k, KW=k,
                                   stride=2, pad=k - 1 - self.pad, Ho=x.H, Wo=x.W, Cout=C0, dtype=pl.cdt, accumulate0=self.acc0)
        return ops.conv_params(self.dy, self.wb, self.d0, N=pl.N, Hs0=Ho, Ws0=Wo,
                               Hv=(2 * Ho - 1 if stride == 2 else Ho), Wv=(2 * Wo - 1 if stride == 2 else Wo),
                               C0=self.CoutB, mode=(ops.SRC_ZEROINS2X if stride == 2 else ops.SRC_DIRECT), KH=k, KW=k, stride=1,
                               pad=k - 1 - self.pad, Ho=self.Hv, Wo=self.Wv, Cout=C0 + self.C1, dtype=pl.cdt, dst1=self.d1, Cd0=C0,
                               accumulate0=self.acc0, accumulate1=self.acc1)

    # 1x1 / stride 2 (the projection shortcut of a bottleneck ResNet's first unit): the zero-inserted form runs the GEMM
    # over all four parity classes of the high-resolution grid (229 us for 256 <- 512 channels at 4 x 256 x 256).  Instead:
    # t = W^T dY at LOW resolution (a plain 1x1 / stride-1 launch), then one pass that puts t at the even positions of the
    # gradient - and, when that completes the gradient of a BatchNormalization output, masks it and reduces the sums
    def _form_scatter(self):
        pl, x, N, Ho, Wo, C0 = self.plan, self.x, self.plan.N, self.Ho, self.Wo, self.C0
        if not (self.stride == 2 and self.k == 1 and self.pad == 0 and not self.transpose and not self.upsample and self.src1 is None and self.x_ng
                and self.fs is None and C0 % 4 == 0 and os.environ.get("STP_SCATTER_1X1S2", "1") != "0"):
            return False
        t_low = pl._alloc((N, Ho, Wo, C0))
        qg = ops.conv_params(self.dy, self.wb, t_low, N=N, Hs0=Ho, Ws0=Wo, Hv=Ho, Wv=Wo, C0=self.CoutB, mode=ops.SRC_DIRECT, KH=1, KW=1,
                             stride=1, pad=0, Ho=Ho, Wo=Wo, Cout=C0, dtype=pl.cdt)
        pl._emit_conv(pl.bwd, qg, {"layer": self.name, "pass": "dgrad", "flops": 2.0 * N * Ho * Wo * self.Cout * self.Cin_master,
                                   "tile": int(pl.lib.stp_conv2d_tile_for(C.byref(qg)))})
        pl._emit_grad_pass("stp_scatter2x_bwd", x, self.acc0, (N, x.H, x.W, C0, pl.cdt),
                           (t_low.data_ptr(), self.d0.data_ptr(), N, x.H, x.W, C0, pl.cdt, self.acc0))
        x.grad_ready = True
        return True

    def _sibling_ready(self):
        """The sibling projection shortcut (``fold_shortcut``) has its dY and its data-gradient weights at this layer's output size."""
        fs = self.fs
        return (fs is not None and self.src1 is None and self.x_ng and not self.transpose and fs.needs_grad and fs.grad_ready
                and fs.meta.get("wb") is not None and (fs.H, fs.W) == (self.Ho, self.Wo))

    def _fold_sibling(self):
        """The sibling's share of x's gradient arrives with this launch (read by the sole / last decision of _attach_bn_sums)."""
        self.fs.meta["dgrad_folded"] = True
        self.x.grad_writes += 1

    # SPACE-TO-DEPTH form (round 5, stp_conv_params.s2d_dgrad): the four output parity classes as ONE dense 2 x 2-tap
    # convolution of dY into 4 x C0 class-major channels on the halo kernel, stored depth-to-space; the sibling 1x1 /
    # stride-2 shortcut's dY rides along as a second source (its weights live at class 0 / tap 0 only)
    def _form_s2d(self):
        pl, fs, dy, Ho, Wo, C0, CoutB = self.plan, self.fs, self.dy, self.Ho, self.Wo, self.C0, self.CoutB
        if not (self.stride == 2 and self.k == 3 and self.pad == 1 and not self.transpose and self.src1 is None and self.x_ng and pl.dtype != "fp32"
                and not self.stem and self.Cout == CoutB and C0 == self.Cin_master and (self.Hv, self.Wv) == (2 * Ho, 2 * Wo)
                and os.environ.get("STP_S2D", "1") != "0"
                and os.environ.get("STP_HALO", "1") != "0"):      # (stp_conv2d_halo_variant ignores the A/B switch; the dispatcher honours it)
            return None
        fold = self._sibling_ready() and fs.gradC == CoutB and fs.meta.get("w_master", (0, 0, 0, 0))[1:] == (self.Cout, C0, 1)
        qs = ops.conv_params(dy, dy, self.d0, N=pl.N, Hs0=Ho, Ws0=Wo, Hv=Ho, Wv=Wo, C0=CoutB, C1=(CoutB if fold else 0),
                             src1=(fs.grad if fold else None), mode=ops.SRC_DIRECT, KH=2, KW=2, stride=1, pad=0, Ho=Ho, Wo=Wo,
                             Cout=4 * C0, dtype=pl.cdt, accumulate0=self.acc0)
        qs.s2d_dgrad = 1
        qs.weight = self.wb.data_ptr()                   # the ordinary data-gradient copies: the kernel addresses them per parity class
        if fold:
            qs.fold_weight = fs.meta["wb"].data_ptr()
        if int(pl.lib.stp_conv2d_halo_variant(C.byref(qs))) < 0:
            return None
        if fold:
            self._fold_sibling()
        return Dgrad(qs, self, s2d=True)

    # the shortcut's 1x1 / stride-2 data gradient = one more (centre) tap of this launch's (even, even) parity class
    def _form_parity_fold(self, q):
        fs = self.fs
        if not (self.stride == 2 and self.k == 3 and self._sibling_ready() and fs.gradC == self.CoutB and int(self.plan.lib.stp_conv2d_fold_ok(C.byref(q)))):
            return None
        q.fold_src, q.fold_weight, q.fold_C = fs.grad.data_ptr(), fs.meta["wb"].data_ptr(), self.CoutB
        self._fold_sibling()
        return Dgrad(q, self)

    # the sibling 1x1 / stride-1 shortcut (first unit of ResNet18 / 34's stage 1): its dY is a second source of this launch
    # whose centre tap carries the shortcut's weights (conv_halo.hip, FOLD1) - no separate launch accumulates into dX
    def _form_fold1(self, q):
        pl, fs = self.plan, self.fs
        if not (self.stride == 1 and self.k == 3 and self.pad == 1 and not self.upsample and self._sibling_ready()
                and fs.meta.get("w_master", (0, 0, 0, 0))[2:] == (self.C0, 1) and pl.dtype != "fp32" and os.environ.get("STP_HALO", "1") != "0"):
            return None
        c = _lib.ConvParams.from_buffer_copy(q)
        c.fold_src, c.fold_weight, c.fold_C = fs.grad.data_ptr(), fs.meta["wb"].data_ptr(), fs.gradC
        if int(pl.lib.stp_conv2d_halo_variant(C.byref(c))) < 0:
            return None
        self._fold_sibling()
        return Dgrad(c, self, fold1=True)

    # conv3x3(concat(UpSampling2D(2)(x), skip)): the skip gradient is the plain 3x3 data gradient with the skip's rows
    # of the flipped weight copy; the gradient of x is a 4x4 / stride-2 convolution of dY with the tap sums (w4) that
    # lands on the low-resolution tensor directly - no high-resolution gradient, no stp_upsample2x_bwd
    def _form_collapsed(self):
        pl, x, dy, wb, k, Ho, Wo, C0, C1, CoutB = self.plan, self.x, self.dy, self.wb, self.k, self.Ho, self.Wo, self.C0, self.C1, self.CoutB
        if self.w4 is None:
            return None
        if self.s_ng:
            q1 = ops.conv_params(dy, wb, self.d1, N=pl.N, Hs0=Ho, Ws0=Wo, Hv=Ho, Wv=Wo, C0=CoutB, mode=ops.SRC_DIRECT, KH=k, KW=k,
                                 stride=1, pad=k - 1 - self.pad, Ho=self.Hv, Wo=self.Wv, Cout=C1, dtype=pl.cdt, accumulate0=self.acc1)
            q1.weight = wb.data_ptr() + C0 * k * k * CoutB * wb.element_size()
            pl._emit_conv(pl.bwd, q1, {"layer": self.name, "pass": "dgrad", "flops": self.flops * C1 / float(C0 + C1),
                                       "tile": int(pl.lib.stp_conv2d_tile_for(C.byref(q1)))})
        q = ops.conv_params(dy, self.w4, pl._gradbuf(x), N=pl.N, Hs0=Ho, Ws0=Wo, Hv=Ho, Wv=Wo, C0=CoutB, mode=ops.SRC_DIRECT,
                            KH=4, KW=4, stride=2, pad=1, Ho=x.H, Wo=x.W, Cout=C0, dtype=pl.cdt, accumulate0=int(x.grad_ready))
        return Dgrad(q, self, folded_up=True, collapsed=True)

    # the small-channel kernel sums each 2x2 block in its epilogue: the hi-res gradient of the upsampled
    # tensor is never written and stp_upsample2x_bwd disappears
    # ... and the wide-output kernel does the same for conv3x3(concat(UpSampling2D(2)(x), skip)): the first C0
    # channels are summed into the low-resolution gradient, the skip's C1 channels stay at full resolution
    def _form_sum2x2_stream(self, q):
        pl, x = self.plan, self.x
        if not (self.upsample and self.x_ng and pl.fold_upsample_grad):
            return None
        c = _lib.ConvParams.from_buffer_copy(q)
        c.dst_sum2x2 = 1
        if not (pl.lib.stp_conv2d_scw_eligible(C.byref(c)) if self.C1 else (pl.lib.stp_conv2d_sc_eligible(C.byref(c)) and self.C0 % 4 == 0)):
            return None
        c.dst0, c.accumulate0 = pl._gradbuf(x).data_ptr(), int(x.grad_ready)
        return Dgrad(c, self, folded_up=True, two_dest=bool(self.C1))

    # ... and the halo kernel (64+ channel decoder stages, round 4): its epilogue sums the 2 x 2 blocks of the channel
    # tiles of the upsampled source and runs the fused BatchNormalization backward on the LOW-resolution result
    # (EP 3) - only in that fused form, i.e. when this launch completes the gradient of a BatchNormalization output
    # that nothing else reads.  With a skip (two destinations) its C1 channels stay at full resolution.
    def _form_sum2x2_halo(self, q):
        pl, x, bnm = self.plan, self.x, self.x.meta.get("bn")
        if not (self.upsample and self.x_ng and pl.fold_upsample_grad
                and pl.fuse_bn_backward and bnm is not None and x.meta.get("uses", 0) == 1 and not x.grad_ready
                and pl.slot_arena is None and os.environ.get("STP_HALO_FOLD_UP", "1") != "0"
                and os.environ.get("STP_HALO", "1") != "0"):      # (the dispatcher honours STP_HALO=0: plan and dispatcher agree)
            return None
        c = _lib.ConvParams.from_buffer_copy(q)
        c.dst_sum2x2, c.dst0, c.accumulate0 = 1, pl._gradbuf(x).data_ptr(), 0
        pl._set_bnb(c, bnm)
        if int(pl.lib.stp_conv2d_halo_variant(C.byref(c))) < 0:
            return None
        return Dgrad(c, self, folded_up=True, two_dest=bool(self.C1))

    # the only consumer, or the LAST of several (every other consumer has already written or accumulated its
    # share, this data gradient accumulates on top): its epilogue sees the complete gradient of the BN output; this launch
    # and a sibling folded into it may be the only two consumers: the gradient is complete as well (Plan._completes_grad)
    def _attach_bn_sums(self, form):
        pl, x, q, C0, bnm = self.plan, self.x, form.q, self.C0, self.x.meta.get("bn")
        done = pl._completes_grad(x, q.accumulate0, promoted=form.fold1 or form.s2d, last_ok=not self.upsample)
        if not (pl.fuse_bn_backward and bnm is not None and done and (form.folded_up or not self.upsample) and (form.C1 == 0 or form.two_dest)
                and self.x_ng and C0 % 4 == 0):
            return
        pl._set_bnb(q, bnm)
        if pl.slot_arena is not None and pl.N * self.Hv * self.Wv <= pl.bn_slots_max_rows and not form.two_dest:
            # (the two-destination kernel has no slot form - stp_conv2d_scw_eligible was checked without them, and with
            #  slots the launch would fall through to the generic kernel, which refuses dst_sum2x2: float partial sums there)
            q.stats_partial, q.stats_slots = x.meta["bnb_slots"] = pl._slots(C0)
        else:
            nfl = int(pl.lib.stp_conv2d_stats_floats(C.byref(q)))
            st = pl._alloc((max(nfl, 4),), torch.float32)
            q.stats_partial = st.data_ptr()
            gt, gcols = pl._group_stats(q, st, C0)
            # (gt is not st: the pre-reduced table ([2][C0][columns / G]) and its column count)
            x.meta["bnb"] = (st, q) if gt is st else (gt, gcols)
