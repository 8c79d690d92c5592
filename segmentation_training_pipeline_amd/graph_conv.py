"""The plan's value types (tensor handle, parameter record, the argument records of the BatchNormalization launches the peepholes
read) and the plan of one convolution: ``ConvLayer``, one ``Plan.conv`` call, with ``Dgrad``, what its data-gradient chooser settled on.
The lowest module of the planner: ``graph`` (``Plan``), ``graph_layers`` and ``graph_heads`` import from here."""
import os
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops


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


# The arguments of stp_bn_apply and stp_bn_finalize (include/stp_hip.h, without the stream), in the ABI's order: every emit site builds
# its record through these, the peepholes that take such a record over (Plan._fuse_bn_finalize, Plan.maxpool) read it by field name.  The
# launch record itself keeps a plain tuple of the same values.
BnApply = namedtuple("BnApply", "x xdtype y ydtype rows C Cy mean rstd gamma beta relu pad_value")
BnFinalize = namedtuple("BnFinalize", "partial tiles rows C eps momentum mean rstd moving_mean moving_var")


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
            pl._grad_alias_or_add(residual, out)
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