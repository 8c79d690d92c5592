"""The loss and output heads of a plan: the launches that end the forward list and seed the backward pass (``Plan`` inherits them)."""
import ctypes as C

import torch

from .graph_conv import StpShapeError


class HeadsMixin(object):

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
                       float(w_dice), self.loss_scalars.data_ptr(), self._ptr(dp), probs.gradC, *self._ws(self.ws_loss))
        else:
            self._emit(self.fwd, "stp_prob_cce_dice", probs.buf.data_ptr(), target.buf.data_ptr(), probs.rows, probs.C, probs.C, self.cdt,
                       float(w_ce), float(w_dice), self.loss_scalars.data_ptr(), self._ptr(dp), probs.gradC, *self._ws(self.ws_loss))
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
                   self._ptr(dl), logits.gradC, float(self.loss_scale), *self._ws(self.ws_loss), *tail)
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
                       float(w_lovasz), self.loss_scalars.data_ptr(), self._ptr(dl), logits.gradC,
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
                name, tail = "stp_softmax_loss_masked", (ign, self._ptr(cw))
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
                               self.cdt, w_lovasz, self.loss_scalars.data_ptr(), self._ptr(dl), logits.gradC,
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
            dls = self._ptr(self.dls)
            self._emit(self.fwd, "stp_softmax_cce_dice_up", lo.buf.data_ptr(), target.buf.data_ptr(), self.N, lo.H, lo.W, f, logits.C, lo.C,
                       self.cdt, float(w_cce), float(w_dice), self.loss_scalars.data_ptr(), dlow.data_ptr(), lo.gradC, float(self.loss_scale),
                       dls, (dls + 16) if dls is not None else None, *self._ws(self.ws_loss), corners.data_ptr(), nb)
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
