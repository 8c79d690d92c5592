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
from .graph_conv import BnApply, BnFinalize, ConvLayer, DT, ParamInfo, StpShapeError, _rup      # (the value types are re-exported)
from .graph_heads import HeadsMixin
from .graph_layers import LayersMixin

_TD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


# The planner in four modules: this one holds the core - arenas and ``define``, parameters and states, the launch-record emitters, the
# frame of a layer (``_layer``) and the three gradient hand-offs, the BatchNormalization peepholes, ``run`` and ``rerun_*`` - with ``bn``,
# ``conv`` and ``conv3x3_taps``; the other layer methods are ``graph_layers.LayersMixin``, the loss and output heads
# ``graph_heads.HeadsMixin``, the plan of one convolution ``graph_conv.ConvLayer``.
class Plan(LayersMixin, HeadsMixin):
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

    @staticmethod
    def _ptr(t):
        """The device pointer of an optional tensor."""
        return t.data_ptr() if t is not None else None

    @staticmethod
    def _ws(buf):
        """(pointer, bytes) of an fp32 workspace - ``ws_bn``, ``ws_loss``, ``ws_dw`` - as a launch takes it."""
        return buf.data_ptr(), buf.numel() * 4

    @staticmethod
    def _pad4(vals, fill=None):
        """The operands of a launch that takes up to four maps, padded to its four slots."""
        return list(vals) + [fill] * (4 - len(vals))

    # ------------------------------------------------------------------ the frame of a layer
    def _layer(self, out, inputs, emit, guard=None):
        """The frame every layer method shares.  Counts ``out`` as a consumer of ``inputs``; the dry pass ends here.  ``emit()`` records the
        forward launches and returns the layer's backward body; in training that body goes on the tape behind the guard "the output needs
        and has a gradient" (``guard``: a layer whose condition is another one says so there).  Returns ``out``."""
        self._use(*inputs)
        if self.dry:
            return out
        backward = emit()
        if self.training:
            ready = guard or (lambda: out.needs_grad and out.grad_ready)

            def back():
                if ready():
                    backward()

            self._tape.append(back)
        return out

    def _view(self, name, x, needs_grad):
        """The output of an in-place layer: a tensor of its own name on x's buffer, its gradient padded as x's is."""
        out = DT(name, self.N, x.H, x.W, x.C, x.buf, needs_grad)
        out.gradC = x.gradC
        self.tensors[name] = out
        return out

    # The three ways a backward body hands a gradient to the tensor ``t`` it read.  Each is an ordering contract with the pending grouped
    # weight gradient: _gradbuf may issue that group, so it runs BEFORE the body's own record is appended (and after the _scratch call of a
    # body that has one); the accumulate flag is read before ``t`` is marked ready.
    def _grad_into(self, t):
        """Write or accumulate: (pointer of t's gradient buffer, accumulate flag) for the launch that adds this layer's share - the first
        writer overwrites, later ones accumulate.  Marks ``t`` ready."""
        ptr, acc = self._gradbuf(t).data_ptr(), int(t.grad_ready)
        t.grad_ready = True
        return ptr, acc

    def _grad_alias_or_add(self, t, out):
        """``t`` receives out's gradient as it is (a residual, a skip, a shortcut, a standalone activation).  The FIRST gradient of ``t``
        aliases the buffer - dY is dead once the layer's backward has been issued, later writers accumulate into it; otherwise (``t`` has
        a gradient, or pads its channels differently) stp_add_inplace on top, which does not count as one more write."""
        if not t.grad_ready and t.gradC == out.gradC:
            self._grad_alias(t, out.grad)
        else:
            self._emit(self.bwd, "stp_add_inplace", self._gradbuf(t).data_ptr(), out.grad.data_ptr(), out.rows * out.gradC, self.cdt)

    @staticmethod
    def _grad_alias(t, dy):
        """Plain alias: ``dy`` IS t's gradient (``t`` has no other consumer, or its backward is issued before any later writer)."""
        t.grad, t.grad_ready = dy, True

    def _emit_resize_grad(self, out, t, Cn, f, off, nearest):
        """t's share of the gradient of a resize by ``f``, nearest or bilinear (TF 1.x, with its scratch workspace): the channels
        [off, off + Cn) of out's gradient, written or accumulated."""
        tail = () if nearest else self._scratch(self.lib.stp_resize_bilinear_bwd_workspace_bytes(self.N, t.H, t.W, Cn, f))
        dx, acc = self._grad_into(t)
        self._emit(self.bwd, "stp_resize_nearest_bwd" if nearest else "stp_resize_bilinear_bwd", out.grad.data_ptr(), dx, self.N, t.H, t.W, Cn, f,
                   out.gradC, off, self.cdt, acc, *tail)

    def _emit_identity_apply(self, x, xdtype, out, n, relu):
        """y = x * 1 + 0 [ReLU] through the BatchNormalization apply kernel (mean 0, rstd 1 in two buffers of ``n`` floats, no gamma / beta):
        x's real channels into out's, the padded ones zero."""
        zero, one = self._alloc((n,), torch.float32), self._alloc((n,), torch.float32)
        zero.zero_(); one.fill_(1.0)
        self._emit(self.fwd, "stp_bn_apply", *BnApply(x.buf.data_ptr(), xdtype, out.buf.data_ptr(), self.cdt, x.rows, x.C, out.C, zero.data_ptr(),
                                                      one.data_ptr(), None, None, relu, 0.0))

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
            if r[2] == "stp_bn_finalize" and nxt is not None and nxt[2] == "stp_bn_apply" and id(nxt) not in keep:
                f, a = BnFinalize(*r[1]), BnApply(*nxt[1])
                if ((a.mean, a.rstd) == (f.mean, f.rstd) and a.xdtype == a.ydtype == self.cdt and a.C == a.Cy == f.C and a.pad_value == 0.0
                        and a.rows == f.rows and int(self.lib.stp_bn_finalize_apply_ok(self.cdt, f.rows, f.C, f.tiles))):
                    out.append((self.lib.stp_bn_finalize_apply, (f.partial, f.tiles, a.x, a.y, self.cdt, f.rows, f.C, f.eps, f.momentum, f.mean, f.rstd,
                                                                 f.moving_mean, f.moving_var, a.gamma, a.beta, a.relu), "stp_bn_finalize_apply", None))
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
                lst.append((self.lib.stp_conv2d_wgrad_partial, (C.byref(p), *self._ws(ws), 0), "stp_conv2d_wgrad", meta))
                self._pending_reduces.append((bytes(desc), count))
                self._pending_reduce_hi = max(self._pending_reduce_hi, int(defer_hi))
                if len(self._pending_reduces) >= self.reduce_batch:
                    self._flush_reduces()
                return
            self._keep = [t for t in self._keep if t is not ws]          # (row-of-taps slabs: the layer keeps its own reduce launch)
        lst.append((self.lib.stp_conv2d_wgrad_partial, (C.byref(p), *self._ws(self.ws_wgrad), 0),
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
                       mean.data_ptr(), rstd.data_ptr(), self._sptr(mm), self._sptr(mv), *self._ws(self.ws_bn))
            self._emit(self.fwd, "stp_bn_apply", *BnApply(x.buf.data_ptr(), ops.U8, out.buf.data_ptr(), self.cdt, x.rows, x.C, Cp,
                                                          mean.data_ptr(), rstd.data_ptr(), None, self._pptr(beta), 0, 1.0))
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
        self._emit_identity_apply(x, ops.U8, out, 8, 0)      # (the uint8 form of the kernel)
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
        if self.dry:
            self._slot_need += 4 * Cn * self._nslots(Cn)       # forward statistics + backward sums

        def emit():
            xp, yp, moving = x.buf.data_ptr(), out.buf.data_ptr(), (self._sptr(mm), self._sptr(mv))
            gp, bp = self._pptr(gamma) if gamma else None, self._pptr(beta)
            if not self.training:
                self._emit(self.fwd, "stp_bn_inference", xp, self.cdt, yp, self.cdt, x.rows, Cn, Cn, *moving, eps, gp, bp, relu, 0.0)
                return None
            mean, rstd = self._alloc((Cn,), torch.float32), self._alloc((Cn,), torch.float32)
            mp, rp = mean.data_ptr(), rstd.data_ptr()
            table = x.meta.get("stats_table")      # [2][C][columns] sums and their column count: a convolution's epilogue, or Plan.se's scale-add pass
            slots = x.meta.get("stats_slots")
            if slots is not None:
                # statistics from the producing convolution's fixed-point slots: finalize + normalise + activation in one kernel
                self._emit(self.fwd, "stp_bn_apply_slots", xp, yp, self.cdt, x.rows, Cn, slots[0], slots[1], eps, momentum, mp, rp, *moving, gp, bp, relu)
            elif table is not None:
                self._emit(self.fwd, "stp_bn_finalize", *BnFinalize(table[0].data_ptr(), table[1], x.rows, Cn, eps, momentum, mp, rp, *moving))
            else:
                self._emit(self.fwd, "stp_bn_stats", xp, self.cdt, x.rows, Cn, eps, momentum, mp, rp, *moving, *self._ws(self.ws_bn))
            if slots is None:
                self._emit(self.fwd, "stp_bn_apply", *BnApply(xp, self.cdt, yp, self.cdt, x.rows, Cn, Cn, mp, rp, gp, bp, relu, 0.0))
            out.meta["bn"] = (xp, mp, rp, gp, bp, relu)
            if self.fuse_bn_sc and slots is None:
                out.meta["apply_rec"] = self.fwd[-1]
                out.meta["sc_consumers"], out.meta["halo_consumers"] = [], []

            # (the common guard; the BODY differs from the other layers: dx is produced even when x needs no gradient - it is cheap
            #  relative to skipping logic - into a buffer of its own; frozen params are masked in the optimizer)
            def back():
                bslots, bnb = out.meta.get("bnb_slots"), out.meta.get("bnb")
                dadd = None
                if x.needs_grad and x.grad_ready and x.grad is not None and x.grad.data_ptr() in self._wgroup_reads and bslots is None and bnb is not None:
                    # x's gradient so far is the dY of a convolution whose weight gradient waits in the pending group (the residual
                    # branch aliases it): accumulate OUT OF PLACE - the sum lands in a fresh buffer, the dY stays intact
                    dadd, x.grad = x.grad, None
                dx, acc = self._grad_into(x) if x.needs_grad else (self._alloc((x.N, x.H, x.W, Cn)).data_ptr(), 0)
                head = (xp, out.grad.data_ptr(), dx)
                if bslots is not None:
                    self._emit(self.bwd, "stp_bn_backward_slots", *head, self.cdt, x.rows, Cn, mp, rp, gp, bslots[0], bslots[1],
                               self._gptr(gamma) if gamma else None, self._gptr(beta), acc)
                elif bnb is not None:
                    # the only consumer's data-gradient epilogue already masked dY and reduced the per-tile sums
                    st, q = bnb
                    tiles = q if isinstance(q, int) else int(self.lib.stp_conv2d_stats_floats(C.byref(q))) // (2 * Cn)
                    if dadd is not None:
                        head += (dadd.data_ptr(),)
                    self._emit(self.bwd, "stp_bn_backward_fused_add" if dadd is not None else "stp_bn_backward_fused", *head, self.cdt, x.rows, Cn, mp, rp,
                               gp, st.data_ptr(), tiles, self._gptr(gamma) if gamma else None, self._gptr(beta), acc, *self._ws(self.ws_bn))
                else:
                    self._emit(self.bwd, "stp_bn_backward", *head, self.cdt, x.rows, Cn, mp, rp, gp, bp, self._gptr(gamma) if gamma else None,
                               self._gptr(beta), relu, acc, *self._ws(self.ws_bn))
            return back

        return self._layer(out, (x,), emit)

    def _emit_bias_grad(self, dy, rows, gradC, Cout, b):
        """Bias gradient = the channel sums of ``dy`` ([rows][gradC], the first ``Cout`` channels real)."""
        tmp = self._alloc((gradC,), torch.float32)
        self._emit(self.bwd, "stp_channel_sum", dy.data_ptr(), self.cdt, rows, gradC, tmp.data_ptr(), 0, *self._ws(self.ws_bn))
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

        def emit():
            self._emit(self.fwd, "stp_tapsum_fwd", z.buf.data_ptr(), out.buf.data_ptr(), self._pptr(b) if b is not None else None, self.N, x.H, x.W,
                       Cout, z.C, Cout, self.cdt)

            def back():
                dy = out.grad
                if b is not None and b.trainable:
                    self._emit_bias_grad(dy, out.rows, out.gradC, Cout, b)
                if z.needs_grad:
                    self._emit(self.bwd, "stp_tapsum_bwd", dy.data_ptr(), self._grad_into(z)[0], self.N, x.H, x.W, Cout, out.gradC, z.gradC, self.cdt)
            return back

        # (its own guard, as it has always been: a gradient that is there is propagated whether or not ``out`` asked for one)
        return self._layer(out, (z,), emit, guard=lambda: out.grad_ready)

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
