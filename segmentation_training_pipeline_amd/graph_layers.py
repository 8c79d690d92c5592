"""The layer methods of a plan other than BatchNormalization and the convolutions (``Plan`` inherits them).  Each is its shape check, its
parameters and tensors, and one ``emit`` closure - the forward launches, returning the backward body - handed to ``Plan._layer``, which
owns the frame: consumer counts, the dry pass, inference, the tape and its guard.  Gradients meet through the three hand-offs of
``Plan``: ``_grad_into`` (write or accumulate), ``_grad_alias_or_add`` and ``_grad_alias``."""
import os

import torch

from .graph_conv import BnApply, StpShapeError, _rup


class LayersMixin(object):

    def add(self, name, y, skip):
        """Keras ``Add()([y, skip])`` computed in place on y's buffer (y must have no other consumer): Linknet's
        decoder adds the encoder feature AFTER BatchNormalization + ReLU, so it cannot ride in a conv epilogue."""
        if (y.H, y.W, y.C) != (skip.H, skip.W, skip.C):
            raise StpShapeError("%s: cannot add %dx%dx%d and %dx%dx%d" % (name, y.H, y.W, y.C, skip.H, skip.W, skip.C))
        out = self._view(name, y, y.needs_grad or skip.needs_grad)

        def emit():
            self._emit(self.fwd, "stp_add_inplace", y.buf.data_ptr(), skip.buf.data_ptr(), y.rows * y.C, self.cdt)

            def back():
                if y.needs_grad:
                    self._grad_alias(y, out.grad)          # read by y's backward, issued before any later writer below
                if skip.needs_grad:
                    self._grad_alias_or_add(skip, out)
            return back

        return self._layer(out, (y, skip), emit)

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

        def emit():
            wsp, wsb = self._scratch(self.lib.stp_se_workspace_bytes(self.N, HW, Cn))      # [N][chunks][C] partial sums, forward and backward
            z, s = self._alloc((self.N * Cn,), torch.float32), self._alloc((self.N * Cn,), torch.float32)
            h = self._alloc((_rup(self.N * R, 4),), torch.float32)
            tiles = self.N * chunks
            st = self._alloc((2 * Cn * tiles,), torch.float32) if (bn_stats and self.training) else None
            self._emit(self.fwd, "stp_se_squeeze", u.buf.data_ptr(), self.cdt, self.N, HW, Cn, wsp, wsb)
            self._emit(self.fwd, "stp_se_excite", wsp, self.N, HW, Cn, R, self._pptr(w1), self._pptr(b1), self._pptr(w2), self._pptr(b2),
                       z.data_ptr(), h.data_ptr(), s.data_ptr())
            self._emit(self.fwd, "stp_se_scale_add", u.buf.data_ptr(), shortcut.buf.data_ptr(), out.buf.data_ptr(), self.cdt, self.N, HW, Cn,
                       s.data_ptr(), self._ptr(st))
            if st is not None:
                out.meta["stats_table"] = (st, tiles)        # no meta["stats"]: Plan.bn hands the table to stp_bn_finalize as it is

            def back():
                dx = out.grad           # read three times below, never rewritten here
                if shortcut.needs_grad:
                    self._grad_alias_or_add(shortcut, out)
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
                    self._emit(self.bwd, "stp_se_bwd_apply", dx.data_ptr(), self._grad_into(u)[0], self.cdt, self.N, HW, Cn, s.data_ptr(), dz.data_ptr())
            return back

        return self._layer(out, (u, shortcut), emit)

    def relu(self, name, x):
        """Keras ``Activation('relu')`` as a tensor of its own (DeepLab's xception blocks activate a tensor that its other
        consumers - the shortcut convolution, the Add - read raw, model.py:133-134): y = max(x, 0) through the BatchNormalization
        apply kernel with the identity affine; the gradient is masked in place by y > 0 and joins x's other gradients."""
        Cn = x.C
        out = self._new(name, x.H, x.W, Cn, x.needs_grad)
        out.gradC = x.gradC

        def emit():
            self._emit_identity_apply(x, self.cdt, out, Cn, 1)

            def back():
                dy = out.grad
                if out.gradC != Cn:
                    raise StpShapeError("%s: standalone ReLU needs an unpadded channel count" % name)
                self._guard_write(dy)
                self._emit(self.bwd, "stp_relu_bwd", out.buf.data_ptr(), dy.data_ptr(), x.rows * Cn, self.cdt)
                self._grad_alias_or_add(x, out)
            return back

        return self._layer(out, (x,), emit)

    def upsample_add(self, name, x, m):
        """FPN top-down step ``Add()([x, UpSampling2D(2)(m)])`` in place on x's buffer (x must have no other consumer yet)."""
        if (x.H, x.W, x.C) != (2 * m.H, 2 * m.W, m.C):
            raise StpShapeError("%s: %dx%dx%d cannot take the 2x upsampling of %dx%dx%d" % (name, x.H, x.W, x.C, m.H, m.W, m.C))
        out = self._view(name, x, x.needs_grad or m.needs_grad)

        def emit():
            self._emit(self.fwd, "stp_upsample2x_add", x.buf.data_ptr(), m.buf.data_ptr(), self.N, x.H, x.W, x.C, self.cdt)

            def back():
                if m.needs_grad:
                    dm, acc = self._grad_into(m)
                    self._emit(self.bwd, "stp_upsample2x_bwd", out.grad.data_ptr(), dm, self.N, m.H, m.W, m.C, out.gradC, self.cdt, acc)
                if x.needs_grad:
                    self._grad_alias(x, out.grad)
            return back

        return self._layer(out, (x, m), emit)

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

        def emit():
            self._emit(self.fwd, "stp_upsample_sum", *self._pad4([t.buf.data_ptr() for t, _ in parts]), *self._pad4([t.H for t, _ in parts], 0),
                       out.buf.data_ptr(), self.N, Ho, Wo, Cn, self.cdt)

            def back():
                for t, f in parts:
                    if t.needs_grad:
                        self._emit_resize_grad(out, t, t.C, f, 0, nearest=False)
            return back

        return self._layer(out, [t for t, _ in parts], emit)

    def concat_resize(self, name, parts, nearest=False):
        """``Concatenate()([ResizeImage(f_i, interpolation)(t_i) ...])``: every part is resized (TF 1.x bilinear, or nearest;
        integer factor; 1 = copy) straight into its channel slice of the output."""
        Ho, Wo = parts[0][0].H * parts[0][1], parts[0][0].W * parts[0][1]
        if any((t.H * f, t.W * f) != (Ho, Wo) for t, f in parts):
            raise StpShapeError("%s: resized parts differ in size" % name)
        Ct = sum(t.C for t, _ in parts)
        out = self._new(name, Ho, Wo, Ct, any(t.needs_grad for t, _ in parts))

        def emit():
            off = 0
            for t, f in parts:
                self._emit(self.fwd, "stp_resize_nearest" if nearest else "stp_resize_bilinear", t.buf.data_ptr(), out.buf.data_ptr(), self.N, t.H,
                           t.W, t.C, f, Ct, off, self.cdt)
                off += t.C

            def back():
                o = 0
                for t, f in parts:
                    if t.needs_grad:
                        self._emit_resize_grad(out, t, t.C, f, o, nearest)
                    o += t.C
            return back

        return self._layer(out, [t for t, _ in parts], emit)

    def resize(self, name, x, factor, nearest=False):
        """``ResizeImage(factor, 'bilinear' | 'nearest')`` of a tensor whose gradient carries padded channels (the class logits)."""
        out = self._new(name, x.H * factor, x.W * factor, x.C, x.needs_grad)
        out.gradC = x.gradC

        def emit():
            self._emit(self.fwd, "stp_resize_nearest" if nearest else "stp_resize_bilinear", x.buf.data_ptr(), out.buf.data_ptr(), self.N, x.H, x.W,
                       x.C, factor, x.C, 0, self.cdt)
            if self.training and not nearest:      # (softmax_loss may take this launch and its gradient over: stp_softmax_cce_dice_up)
                out.meta["resize_rec"] = (len(self.fwd) - 1, x, int(factor))
            return lambda: self._emit_resize_grad(out, x, x.gradC, factor, 0, nearest)

        return self._layer(out, (x,), emit)

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
        self._dw_ws_bytes = max(self._dw_ws_bytes, int(self.lib.stp_dwconv_wgrad_workspace_bytes(Cn, k)))

        def emit():
            geo = (self.N, x.H, x.W, Cn, k, stride, pt, pl, dilation, Ho, Wo, self.cdt)
            self._emit(self.fwd, "stp_dwconv", x.buf.data_ptr(), self._pptr(w), out.buf.data_ptr(), *geo)

            def back():
                if w.trainable:
                    self._emit(self.bwd, "stp_dwconv_wgrad", x.buf.data_ptr(), out.grad.data_ptr(), self._gptr(w), *geo, 0, *self._ws(self.ws_dw))
                if x.needs_grad:
                    dx, acc = self._grad_into(x)
                    self._emit(self.bwd, "stp_dwconv_dgrad", out.grad.data_ptr(), self._pptr(w), dx, *geo, acc)
            return back

        return self._layer(out, (x,), emit)

    def dropout(self, name, x, rate, salt, spatial=False):
        """Keras ``Dropout(rate)`` / ``SpatialDropout2D(rate)`` (``spatial``: one decision per sample and channel): training =
        inverted dropout in place (mask = hash of the device step counter, which the first dropout of the plan ticks once per
        forward); inference = identity."""
        if not self.training:
            return x
        out = self._view(name, x, x.needs_grad)

        def emit():
            if self.step_state is None:
                self.step_state = torch.zeros(2, dtype=torch.int32, device=self.device)
                self._keep.append(self.step_state)
                self._emit(self.fwd, "stp_counter_tick", self.step_state.data_ptr())
            tail = (float(rate), self.step_state.data_ptr(), int(salt), self.cdt)
            if spatial:
                self._emit(self.fwd, "stp_dropout_spatial", x.buf.data_ptr(), x.buf.data_ptr(), self.N, x.H * x.W, x.C, *tail)
            else:
                self._emit(self.fwd, "stp_dropout", x.buf.data_ptr(), x.buf.data_ptr(), x.rows * x.C, *tail)

            def back():
                dy = out.grad
                if spatial:
                    if out.gradC != x.C:
                        raise StpShapeError("%s: spatial dropout needs an unpadded channel count" % name)
                    self._emit(self.bwd, "stp_dropout_spatial", dy.data_ptr(), dy.data_ptr(), self.N, x.H * x.W, x.C, *tail)
                else:
                    self._emit(self.bwd, "stp_dropout", dy.data_ptr(), dy.data_ptr(), x.rows * out.gradC, *tail)
                self._grad_alias(x, dy)
            return back

        return self._layer(out, (x,), emit)

    def resize_ac(self, name, x, Ho, Wo):
        """``BilinearUpsampling`` (DeepLab model.py:56-100): tf.image.resize_bilinear(align_corners=True) to (Ho, Wo)."""
        out = self._new(name, Ho, Wo, x.C, x.needs_grad)
        out.gradC = x.gradC

        def emit():
            self._emit(self.fwd, "stp_resize_bilinear_ac", x.buf.data_ptr(), out.buf.data_ptr(), self.N, x.H, x.W, x.C, Ho, Wo, self.cdt)

            def back():
                dx, acc = self._grad_into(x)
                self._emit(self.bwd, "stp_resize_bilinear_ac_bwd", out.grad.data_ptr(), dx, self.N, x.H, x.W, x.gradC, Ho, Wo, self.cdt, acc)
            return back

        return self._layer(out, (x,), emit)

    def sigmoid_act(self, name, z):
        """The activation of DeepLab's last convolution as a layer (model.py:485): sigmoid for one class, channel softmax for
        2..32 classes."""
        out = self._new(name, z.H, z.W, z.C, z.needs_grad)
        out.gradC = z.gradC
        fn = "stp_sigmoid_act" if z.C == 1 else "stp_softmax_act"

        def emit():
            self._emit(self.fwd, fn, z.buf.data_ptr(), out.buf.data_ptr(), z.rows, z.C, z.C, z.C, self.cdt)
            return lambda: self._emit(self.bwd, fn + "_bwd", out.buf.data_ptr(), out.grad.data_ptr(), self._grad_into(z)[0], z.rows, z.C, z.C,
                                      z.gradC, self.cdt)

        return self._layer(out, (z,), emit)

    def avgpool(self, name, x, k):
        """AveragePooling2D(pool_size = strides = k) with exact division (PSPNet pyramid levels)."""
        if x.H % k or x.W % k:
            raise StpShapeError("%s: %dx%d is not divisible by the pooling size %d" % (name, x.H, x.W, k))
        out = self._new(name, x.H // k, x.W // k, x.C, x.needs_grad)

        def emit():
            wp, wb = self._scratch(self.lib.stp_avgpool_workspace_bytes(self.N, x.H, x.W, x.C, k))
            self._emit(self.fwd, "stp_avgpool", x.buf.data_ptr(), out.buf.data_ptr(), self.N, x.H, x.W, x.C, k, self.cdt, wp, wb)
            return lambda: self._emit_avgpool_grad(out, x, k)

        return self._layer(out, (x,), emit)

    def _emit_avgpool_grad(self, y, x, k):
        """The gradient of one AveragePooling2D(k) output ``y`` into x's, written or accumulated."""
        dx, acc = self._grad_into(x)
        self._emit(self.bwd, "stp_avgpool_bwd", y.grad.data_ptr(), dx, self.N, x.H, x.W, x.C, k, self.cdt, acc)

    def avgpool_pyramid(self, names, x, ks):
        """The AveragePooling2D(k) of PSPNet's pyramid levels (one per name / window size) of ONE tensor: where the windows nest (every k a
        multiple of the smallest one) a single pass over ``x`` (stp_avgpool_pyramid) and a single pass over its gradient instead of one per
        level; otherwise the separate launches of ``avgpool``.  Returns the pooled tensors in the order of ``names``."""
        order = sorted(range(len(ks)), key=lambda i: ks[i])
        kk = self._pad4([int(ks[i]) for i in order], 0)
        if (len(ks) < 2 or len(ks) > 4 or any(x.H % k or x.W % k for k in ks)
                or not self.lib.stp_avgpool_pyramid_ok(self.N, x.H, x.W, x.C, *kk, self.cdt)):
            return [self.avgpool(nm, x, k) for nm, k in zip(names, ks)]
        outs = [self._new(nm, x.H // k, x.W // k, x.C, x.needs_grad) for nm, k in zip(names, ks)]

        def emit():
            so = [outs[i] for i in order]
            wp, wb = self._scratch(self.lib.stp_avgpool_pyramid_workspace_bytes(self.N, x.H, x.W, x.C, kk[0], self.cdt))
            self._emit(self.fwd, "stp_avgpool_pyramid", x.buf.data_ptr(), *self._pad4([t.buf.data_ptr() for t in so]), *kk, self.N, x.H, x.W,
                       x.C, self.cdt, wp, wb)

            def back():
                if all(t.grad_ready for t in so):
                    gp = self._pad4([t.grad.data_ptr() for t in so])
                    dx, acc = self._grad_into(x)
                    self._emit(self.bwd, "stp_avgpool_pyramid_bwd", *gp, *kk, dx, self.N, x.H, x.W, x.C, self.cdt, acc)
                    return
                for t, k in zip(so, kk):      # (a level without a gradient: the separate launches for the others)
                    if t.grad_ready:
                        self._emit_avgpool_grad(t, x, k)
            return back

        # (its own guard: there is one backward for the four outputs, which looks at each level's gradient itself)
        return self._layer(outs, [x] * len(outs), emit, guard=lambda: x.needs_grad)

    def maxpool_k(self, name, x, k):
        """MaxPooling2D(pool_size = strides = k) (PSPNet ``psp_pooling_type: max``)."""
        if x.H % k or x.W % k:
            raise StpShapeError("%s: %dx%d is not divisible by the pooling size %d" % (name, x.H, x.W, k))
        out = self._new(name, x.H // k, x.W // k, x.C, x.needs_grad)

        def emit():
            idx = self._alloc((self.N, x.H // k, x.W // k, x.C), torch.int32) if self.training else None
            self._emit(self.fwd, "stp_maxpool_k", x.buf.data_ptr(), out.buf.data_ptr(), self._ptr(idx), self.N, x.H, x.W, x.C, k, self.cdt)

            def back():
                dx, acc = self._grad_into(x)
                self._emit(self.bwd, "stp_maxpool_k_bwd", idx.data_ptr(), out.grad.data_ptr(), dx, self.N, x.H, x.W, x.C, k, self.cdt, acc)
            return back

        return self._layer(out, (x,), emit)

    def maxpool2(self, name, x):
        """MaxPooling2D(2, 2) without padding (VGG blocks)."""
        if x.H % 2 or x.W % 2:
            raise StpShapeError("%s: 2x2 pooling needs even height/width" % name)
        out = self._new(name, x.H // 2, x.W // 2, x.C, x.needs_grad)

        def emit():
            idx = self._alloc((self.N, x.H // 2, x.W // 2, x.C), torch.uint8) if self.training else None
            self._emit(self.fwd, "stp_maxpool2x2", x.buf.data_ptr(), out.buf.data_ptr(), self._ptr(idx), self.N, x.H, x.W, x.C, self.cdt)

            def back():
                dx, acc = self._grad_into(x)
                self._emit(self.bwd, "stp_maxpool2x2_bwd", idx.data_ptr(), out.grad.data_ptr(), dx, self.N, x.H, x.W, x.C, self.cdt, acc)
            return back

        return self._layer(out, (x,), emit)

    def maxpool(self, name, x):
        Ho, Wo = (x.H + 2 - 3) // 2 + 1, (x.W + 2 - 3) // 2 + 1
        out = self._new(name, Ho, Wo, x.C, x.needs_grad)

        def emit():
            idx = self._alloc((self.N, Ho, Wo, x.C), torch.uint8) if self.training else None
            last = self.fwd[-1] if self.fwd else None
            a = BnApply(*last[1]) if last is not None and last[2] == "stp_bn_apply" else None
            if (self.training and self.dtype != "fp32" and a is not None and a.y == x.buf.data_ptr() and a.xdtype == a.ydtype == self.cdt
                    and a.C == a.Cy == x.C and a.pad_value == 0.0 and x.C % 8 == 0 and x.H % 2 == 0 and x.W % 2 == 0
                    and x.meta.get("apply_rec") in (None, last) and not x.meta.get("sc_consumers") and not x.meta.get("halo_consumers")
                    and os.environ.get("STP_FUSE_BN_POOL_FWD", "1") != "0"):
                # the BatchNormalization apply that produced x is the previous launch (the stem: bn0 -> relu0 -> pooling0): ONE launch normalises,
                # stores x (the decoder's skip tensor) and pools - the 134 MB pre-normalisation tensor is read once instead of twice
                self.fwd.pop()
                x.meta.pop("apply_rec", None)      # (the launch no longer exists on its own: nothing may drop or move it)
                self._emit(self.fwd, "stp_bn_apply_maxpool3x3s2", a.x, x.buf.data_ptr(), out.buf.data_ptr(), self._ptr(idx), self.N, x.H, x.W, x.C,
                           self.cdt, a.mean, a.rstd, a.gamma, a.beta, a.relu)
            else:
                self._emit(self.fwd, "stp_maxpool3x3s2", x.buf.data_ptr(), out.buf.data_ptr(), self._ptr(idx), self.N, x.H, x.W, x.C, self.cdt)

            def back():
                # (write or accumulate, spelled out: _emit_grad_pass decides "only / last writer" from x's write count, so x is marked ready
                #  behind it, not by _grad_into)
                acc = int(x.grad_ready)
                # the pool gradient completes dY of a BatchNormalization output (bn0: the other consumer is a decoder skip): OPT-IN -
                # measured: 10.06 -> 10.14 ms when on (the gather + x read + reduce in one kernel runs at half the rate of the pair)
                self._emit_grad_pass("stp_maxpool3x3s2_bwd", x, acc, (self.N, x.H, x.W, x.C, self.cdt),
                                     (idx.data_ptr(), out.grad.data_ptr(), self._gradbuf(x).data_ptr(), self.N, x.H, x.W, x.C, self.cdt, acc),
                                     os.environ.get("STP_FUSE_POOL_BN", "0") == "1")
                x.grad_ready = True
            return back

        return self._layer(out, (x,), emit)
