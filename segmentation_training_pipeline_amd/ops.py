"""Thin Python wrappers over the C-ABI (one function per entry point of include/stp_hip.h).

They take torch tensors that live on the GPU, pass raw device pointers + the current HIP stream,
and raise on any error.  No arithmetic happens in Python or in torch here.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import BF16, F16, F32, U8, SRC_DIRECT, SRC_NEAREST2X, SRC_ZEROINS2X  # noqa: F401

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, torch.uint8: U8}


def dt(t):
    return _DT[t.dtype]


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t):
    if t is not None and not t.is_cuda:
        raise _lib.StpError("tensor must live on the GPU (no CPU fallback)")
    return t


def conv_params(src0, weight, dst0, *, N, Hs0, Ws0, Hv, Wv, C0, KH, KW, stride, pad, Ho, Wo, Cout, dtype,
                src1=None, C1=0, mode=SRC_DIRECT, bias=None, residual=None, dst1=None, Cd0=None,
                accumulate0=0, accumulate1=0, relu=0, tile=0):
    p = _lib.ConvParams()
    p.src0, p.src1, p.weight, p.bias, p.residual = ptr(src0), ptr(src1), ptr(weight), ptr(bias), ptr(residual)
    p.dst0, p.dst1 = ptr(dst0), ptr(dst1)
    p.N, p.Hs0, p.Ws0, p.Hv, p.Wv, p.C0, p.C1 = N, Hs0, Ws0, Hv, Wv, C0, C1
    p.src0_mode, p.KH, p.KW, p.stride, p.pad = mode, KH, KW, stride, pad
    p.Ho, p.Wo, p.Cout, p.Cd0 = Ho, Wo, Cout, (Cout if Cd0 is None else Cd0)
    p.accumulate0, p.accumulate1, p.relu, p.dtype, p.tile = accumulate0, accumulate1, relu, dtype, tile
    return p


def conv2d(p, st=None):
    _lib.check(_lib.load().stp_conv2d(C.byref(p), stream() if st is None else st), "stp_conv2d")


def conv2d_stats_floats(p):
    return int(_lib.load().stp_conv2d_stats_floats(C.byref(p)))


def wgrad_params(src0, dy, dw, *, N, Hs0, Ws0, Hv, Wv, C0, KH, KW, stride, pad, Ho, Wo, Cout, dtype,
                 src1=None, C1=0, mode=SRC_DIRECT, accumulate=0, splits=0):
    p = _lib.WgradParams()
    p.src0, p.src1, p.dy, p.dw = ptr(src0), ptr(src1), ptr(dy), ptr(dw)
    p.N, p.Hs0, p.Ws0, p.Hv, p.Wv, p.C0, p.C1, p.src0_mode = N, Hs0, Ws0, Hv, Wv, C0, C1, mode
    p.KH, p.KW, p.stride, p.pad, p.Ho, p.Wo, p.Cout = KH, KW, stride, pad, Ho, Wo, Cout
    p.accumulate, p.dtype, p.splits = accumulate, dtype, splits
    return p


def wgrad_workspace_bytes(p):
    return int(_lib.load().stp_conv2d_wgrad_workspace_bytes(C.byref(p)))


def conv2d_wgrad(p, workspace, st=None):
    _lib.check(_lib.load().stp_conv2d_wgrad(C.byref(p), ptr(workspace), workspace.numel() * workspace.element_size(),
                                            stream() if st is None else st), "stp_conv2d_wgrad")


def conv2d_wgrad_partial(p, workspace, variant=0):
    _lib.check(_lib.load().stp_conv2d_wgrad_partial(C.byref(p), ptr(workspace), workspace.numel() * workspace.element_size(),
                                                    variant, stream()), "stp_conv2d_wgrad_partial")


def conv2d_wgrad_reduce(p, workspace, variant=0):
    _lib.check(_lib.load().stp_conv2d_wgrad_reduce(C.byref(p), ptr(workspace), variant, stream()), "stp_conv2d_wgrad_reduce")


class WgradGroup(object):
    """Descriptor table of a grouped weight gradient (stp_wgrad_group_*): built from the layers' parameter blocks once their
    device pointers are final; holds the host table, its device copy and the partial-slab workspace."""

    def __init__(self, params, device="cuda"):
        lib = _lib.load()
        self.params = list(params)
        n = len(self.params)
        self.arr = (C.POINTER(_lib.WgradParams) * n)(*[C.pointer(p) for p in self.params])
        tb = int(lib.stp_wgrad_group_table_bytes(self.arr, n))
        wsb = int(lib.stp_wgrad_group_workspace_bytes(self.arr, n))
        if tb <= 0 or wsb <= 0:
            raise _lib.StpError("the layers do not form a weight-gradient group")
        self.host = (C.c_char * tb)()
        _lib.check(lib.stp_wgrad_group_build(self.arr, n, C.addressof(self.host), tb), "stp_wgrad_group_build")
        self.dev = torch.frombuffer(bytearray(bytes(self.host)), dtype=torch.uint8).to(device)
        self.ws = torch.empty(wsb // 4, dtype=torch.float32, device=device)
        self.header = list((C.c_int32 * 16).from_buffer_copy(bytes(self.host)[:64]))   # magic, bm, layers, segments, workgroups, tiles, ..., [14] = pbn

    def partial(self):
        _lib.check(_lib.load().stp_wgrad_group_partial(C.addressof(self.host), self.dev.data_ptr(), self.ws.data_ptr(), self.ws.numel() * 4, stream()),
                   "stp_wgrad_group_partial")

    def reduce(self):
        _lib.check(_lib.load().stp_wgrad_group_reduce(C.addressof(self.host), self.dev.data_ptr(), self.ws.data_ptr(), stream()), "stp_wgrad_group_reduce")

    def run(self):
        self.partial()
        self.reduce()


def wgrad_group_class(p):
    return int(_lib.load().stp_wgrad_group_class(C.byref(p)))


def weight_prepare(master, fwd, bwd, Cout, KH, KW, Cin, KWp, Cinp, CoutB, dtype):
    _lib.call("stp_weight_prepare", ptr(master), ptr(fwd), ptr(bwd), Cout, KH, KW, Cin, KWp, Cinp, CoutB, dtype, stream())


def weight_grad_unpad(padded, grad, Cout, KH, KW, Cin, KWp, Cinp, accumulate=0):
    _lib.call("stp_weight_grad_unpad", ptr(padded), ptr(grad), Cout, KH, KW, Cin, KWp, Cinp, accumulate, stream())


def stem_beta_grad(padded_dw, master, dbeta, Cout, KH, KW, Cin, KWp, Cinp, one_ch):
    _lib.call("stp_stem_beta_grad", ptr(padded_dw), ptr(master), ptr(dbeta), Cout, KH, KW, Cin, KWp, Cinp, one_ch, stream())


def bn_workspace_bytes(Cn):
    return int(_lib.load().stp_bn_workspace_bytes(Cn))


def bn_stats(x, rows, Cn, eps, momentum, mean, rstd, moving_mean, moving_var, workspace):
    _lib.call("stp_bn_stats", ptr(_dev(x)), dt(x), rows, Cn, eps, momentum, ptr(mean), ptr(rstd), ptr(moving_mean),
              ptr(moving_var), ptr(workspace), workspace.numel() * workspace.element_size(), stream())


def bn_apply(x, y, rows, Cn, Cy, mean, rstd, gamma, beta, relu, pad_value=0.0):
    _lib.call("stp_bn_apply", ptr(x), dt(x), ptr(y), dt(y), rows, Cn, Cy, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
              int(relu), float(pad_value), stream())


def bn_inference(x, y, rows, Cn, Cy, mm, mv, eps, gamma, beta, relu, pad_value=0.0):
    _lib.call("stp_bn_inference", ptr(x), dt(x), ptr(y), dt(y), rows, Cn, Cy, ptr(mm), ptr(mv), float(eps), ptr(gamma),
              ptr(beta), int(relu), float(pad_value), stream())


def bn_backward(x, dy, dx, rows, Cn, mean, rstd, gamma, beta, dgamma, dbeta, relu, accumulate_dx, workspace):
    _lib.call("stp_bn_backward", ptr(x), ptr(dy), ptr(dx), dt(x), rows, Cn, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
              ptr(dgamma), ptr(dbeta), int(relu), int(accumulate_dx), ptr(workspace),
              workspace.numel() * workspace.element_size(), stream())


def bn_backward_fused(x, g, dx, rows, Cn, mean, rstd, gamma, partial, tiles, dgamma, dbeta, accumulate_dx, workspace):
    _lib.call("stp_bn_backward_fused", ptr(x), ptr(g), ptr(dx), dt(x), rows, Cn, ptr(mean), ptr(rstd), ptr(gamma), ptr(partial),
              int(tiles), ptr(dgamma), ptr(dbeta), int(accumulate_dx), ptr(workspace),
              workspace.numel() * workspace.element_size(), stream())


def maxpool3x3s2(x, y, idx, N, H, W, Cn):
    _lib.call("stp_maxpool3x3s2", ptr(x), ptr(y), ptr(idx), N, H, W, Cn, dt(x), stream())


def maxpool3x3s2_bwd(idx, dy, dx, N, H, W, Cn, accumulate=0):
    _lib.call("stp_maxpool3x3s2_bwd", ptr(idx), ptr(dy), ptr(dx), N, H, W, Cn, dt(dy), int(accumulate), stream())


def maxpool2x2(x, y, idx, N, H, W, Cn):
    _lib.call("stp_maxpool2x2", ptr(x), ptr(y), ptr(idx), N, H, W, Cn, dt(x), stream())


def maxpool2x2_bwd(idx, dy, dx, N, H, W, Cn, accumulate=0):
    _lib.call("stp_maxpool2x2_bwd", ptr(idx), ptr(dy), ptr(dx), N, H, W, Cn, dt(dy), int(accumulate), stream())


def maxpool_k(x, y, idx, N, H, W, Cn, k):
    _lib.call("stp_maxpool_k", ptr(x), ptr(y), ptr(idx), N, H, W, Cn, k, dt(x), stream())


def maxpool_k_bwd(idx, dy, dx, N, H, W, Cn, k, accumulate=0):
    _lib.call("stp_maxpool_k_bwd", ptr(idx), ptr(dy), ptr(dx), N, H, W, Cn, k, dt(dy), int(accumulate), stream())


def relu_bwd(y, dy, count):
    _lib.call("stp_relu_bwd", ptr(y), ptr(dy), count, dt(dy), stream())


def zero_bytes(t, nbytes):
    _lib.call("stp_zero_bytes", ptr(t), nbytes, stream())


def resize_nearest(x, y, N, H, W, Cn, factor, ldo, coff):
    _lib.call("stp_resize_nearest", ptr(x), ptr(y), N, H, W, Cn, factor, ldo, coff, dt(x), stream())


def resize_nearest_bwd(dy, dx, N, H, W, Cn, factor, ldo, coff, accumulate=0):
    _lib.call("stp_resize_nearest_bwd", ptr(dy), ptr(dx), N, H, W, Cn, factor, ldo, coff, dt(dy), int(accumulate), stream())


def dropout_spatial(x, y, N, HW, Cn, rate, state, salt):
    _lib.call("stp_dropout_spatial", ptr(x), ptr(y), N, HW, Cn, float(rate), ptr(state), int(salt), dt(x), stream())


def softmax_act(z, p, rows, classes, ldz, ldp):
    _lib.call("stp_softmax_act", ptr(z), ptr(p), rows, classes, ldz, ldp, dt(z), stream())


def softmax_act_bwd(p, dp, dz, rows, classes, ldp, ldg):
    _lib.call("stp_softmax_act_bwd", ptr(p), ptr(dp), ptr(dz), rows, classes, ldp, ldg, dt(p), stream())


def prob_cce_dice(probs, target, pixels, classes, ldc, w_cce, w_dice, scalars, dprobs, dl_channels, workspace):
    _lib.call("stp_prob_cce_dice", ptr(probs), ptr(target), pixels, classes, ldc, dt(probs), float(w_cce), float(w_dice), ptr(scalars),
              ptr(dprobs), dl_channels, ptr(workspace), workspace.numel() * workspace.element_size(), stream())


def upsample2x_bwd(dy, dx, N, H, W, Cn, ldy, accumulate=0):
    _lib.call("stp_upsample2x_bwd", ptr(dy), ptr(dx), N, H, W, Cn, ldy, dt(dy), int(accumulate), stream())


def channel_sum(x, rows, Cn, out, accumulate, workspace):
    _lib.call("stp_channel_sum", ptr(x), dt(x), rows, Cn, ptr(out), int(accumulate), ptr(workspace),
              workspace.numel() * workspace.element_size(), stream())


def add_inplace(dst, src, count):
    _lib.call("stp_add_inplace", ptr(dst), ptr(src), count, dt(dst), stream())


# channel squeeze-and-excitation (csrc/se.hip): W1 [C][R], b1 [R], W2 [R][C], b2 [C]; z, s, da2, dz [N][C]; h, da1 [N][R]; all fp32
def se_chunks(N, HW, Cn):
    return int(_lib.load().stp_se_chunks(N, HW, Cn))


def se_workspace_bytes(N, HW, Cn):
    return int(_lib.load().stp_se_workspace_bytes(N, HW, Cn))


def se_squeeze(u, N, HW, Cn, workspace):
    _lib.call("stp_se_squeeze", ptr(_dev(u)), dt(u), N, HW, Cn, ptr(workspace), workspace.numel() * workspace.element_size(), stream())


def se_excite(workspace, N, HW, Cn, R, W1, b1, W2, b2, z, h, s):
    _lib.call("stp_se_excite", ptr(_dev(workspace)), N, HW, Cn, R, ptr(W1), ptr(b1), ptr(W2), ptr(b2), ptr(z), ptr(h), ptr(s), stream())


def se_scale_add(u, shortcut, x, N, HW, Cn, s, stats=None):
    _lib.call("stp_se_scale_add", ptr(_dev(u)), ptr(shortcut), ptr(x), dt(u), N, HW, Cn, ptr(s), ptr(stats), stream())


def se_bwd_reduce(dx, u, N, HW, Cn, workspace):
    _lib.call("stp_se_bwd_reduce", ptr(_dev(dx)), ptr(u), dt(u), N, HW, Cn, ptr(workspace), workspace.numel() * workspace.element_size(),
              stream())


def se_excite_bwd(workspace, N, HW, Cn, R, W1, W2, z, h, s, da2, da1, dz, dW1, db1, dW2, db2):
    _lib.call("stp_se_excite_bwd", ptr(_dev(workspace)), N, HW, Cn, R, ptr(W1), ptr(W2), ptr(z), ptr(h), ptr(s), ptr(da2), ptr(da1), ptr(dz),
              ptr(dW1), ptr(db1), ptr(dW2), ptr(db2), stream())


def se_bwd_apply(dx, du, N, HW, Cn, s, dz):
    _lib.call("stp_se_bwd_apply", ptr(_dev(dx)), ptr(du), dt(dx), N, HW, Cn, ptr(s), ptr(dz), stream())


def loss_workspace_bytes():
    return int(_lib.load().stp_loss_workspace_bytes())


def sigmoid_bce_dice(logits, target, count, w_bce, w_dice, scalars, dlogits, dl_channels, grad_scale, workspace):
    _lib.call("stp_sigmoid_bce_dice", ptr(logits), ptr(target), count, dt(logits), float(w_bce), float(w_dice),
              ptr(scalars), ptr(dlogits), dl_channels, float(grad_scale), ptr(workspace),
              workspace.numel() * workspace.element_size(), stream())


def sigmoid_loss_ex(logits, target, count, weights5, scalars, dlogits, dl_channels, grad_scale, workspace):
    """weights5 = (binary_crossentropy, dice_loss, iou_loss, jaccard_loss, focal_loss) weights."""
    import ctypes
    w = (ctypes.c_float * 5)(*[float(v) for v in weights5])
    _lib.call("stp_sigmoid_loss_ex", ptr(logits), ptr(target), count, dt(logits), ctypes.addressof(w), ptr(scalars), ptr(dlogits),
              dl_channels, float(grad_scale), ptr(workspace), workspace.numel() * workspace.element_size(), stream())


def sigmoid(logits, probs, count):
    _lib.call("stp_sigmoid", ptr(logits), ptr(probs), count, dt(logits), stream())


def adam(param, grad, m, v, count, lr, b1, b2, eps, state, mask=None, gscale=None, clipvalue=0.0):
    _lib.call("stp_adam", ptr(param), ptr(grad), ptr(m), ptr(v), count, ptr(lr), b1, b2, eps, ptr(state), ptr(mask),
              ptr(gscale), float(clipvalue), stream())


def rmsprop(p, g, acc, n, lr, rho, eps, mask=None, gscale=None, clipvalue=0.0):
    _lib.call("stp_rmsprop", ptr(p), ptr(g), ptr(acc), n, ptr(lr), rho, eps, ptr(mask), ptr(gscale), clipvalue, stream())


def nadam(p, g, m, v, n, lr, b1, b2, eps, schedule_decay, state, fstate, mask=None, gscale=None, clipvalue=0.0):
    _lib.call("stp_nadam", ptr(p), ptr(g), ptr(m), ptr(v), n, ptr(lr), b1, b2, eps, schedule_decay, ptr(state), ptr(fstate),
              ptr(mask), ptr(gscale), clipvalue, stream())


def sgd(param, grad, vel, count, lr, momentum, nesterov, mask=None, gscale=None, clipvalue=0.0):
    _lib.call("stp_sgd", ptr(param), ptr(grad), ptr(vel), count, ptr(lr), momentum, int(nesterov), ptr(mask), ptr(gscale),
              float(clipvalue), stream())


def grad_global_scale(grad, count, clipnorm, base, gscale, workspace):
    _lib.call("stp_grad_global_scale", ptr(grad), count, float(clipnorm), float(base), ptr(gscale), ptr(workspace),
              workspace.numel() * workspace.element_size(), stream())


def augment_u8(img, mask, img_out, mask_out, params, N, Hin, Win, Hout, Wout, Cn, field=None):
    # the C entry point takes raw pointers: a destination smaller than N x Hout x Wout (x Cn) would be written past its end
    if img_out.numel() < N * Hout * Wout * Cn or img.numel() < N * Hin * Win * Cn:
        raise ValueError("augment_u8: image buffers are smaller than N x H x W x C (%d < %d or %d < %d)" % (
            img_out.numel(), N * Hout * Wout * Cn, img.numel(), N * Hin * Win * Cn))
    if mask is not None and mask_out is not None and (mask_out.numel() < N * Hout * Wout or mask.numel() < N * Hin * Win):
        raise ValueError("augment_u8: mask buffers are smaller than N x H x W")
    if field is not None:
        if field.numel() < N * Hout * Wout:
            raise ValueError("augment_u8: the displacement field is smaller than N x Hout x Wout")
        _lib.call("stp_augment_field_u8", ptr(img), ptr(mask), ptr(img_out), ptr(mask_out), ptr(params), ptr(field), N, Hin, Win, Hout,
                  Wout, Cn, stream())
        return
    _lib.call("stp_augment_u8", ptr(img), ptr(mask), ptr(img_out), ptr(mask_out), ptr(params), N, Hin, Win, Hout, Wout, Cn,
              stream())


def background_replace_u8(img, mask, bg, out, N, H, W, Cn, erosion):
    if min(img.numel(), bg.numel(), out.numel()) < N * H * W * Cn or mask.numel() < N * H * W:
        raise ValueError("background_replace_u8: buffers are smaller than N x H x W (x C)")
    _lib.call("stp_background_replace_u8", ptr(img), ptr(mask), ptr(bg), ptr(out), N, H, W, Cn, int(erosion), stream())


def field_piecewise(field, grid, N, H, W, rows, cols):
    if field.numel() < N * H * W or grid.numel() < N * rows * cols * 2:
        raise ValueError("field_piecewise: buffers are smaller than N x H x W / N x rows x cols x 2")
    _lib.call("stp_field_piecewise", ptr(field), ptr(grid), N, H, W, rows, cols, stream())


def field_elastic(field, tmp, params, N, H, W):
    if field.numel() < N * H * W or tmp.numel() < N * H * W:
        raise ValueError("field_elastic: buffers are smaller than N x H x W")
    _lib.call("stp_field_elastic", ptr(field), ptr(tmp), ptr(params), N, H, W, stream())


def filter_u8(src, dst, params, N, H, W, Cn):
    _lib.call("stp_filter_u8", ptr(src), ptr(dst), ptr(params), N, H, W, Cn, stream())


def cast_f32_to_bf16(src, dst, count):
    _lib.call("stp_cast_f32_to_bf16", ptr(src), ptr(dst), count, stream())


def cast_bf16_to_f32(src, dst, count, scale=1.0):
    _lib.call("stp_cast_bf16_to_f32", ptr(src), ptr(dst), count, float(scale), stream())


# prediction on the device (csrc/predict.hip): flip 0 none, 1 columns reversed, 2 rows reversed; uint8 images, fp32 probabilities
def flip_u8(src, dst, N, H, W, Cn, flip):
    if min(src.numel(), dst.numel()) < N * H * W * Cn:
        raise ValueError("flip_u8: buffers are smaller than N x H x W x C")
    _lib.call("stp_flip_u8", ptr(_dev(src)), ptr(_dev(dst)), N, H, W, Cn, int(flip), stream())


def predict_accumulate(probs, acc, N, H, W, Cn, flip):
    if min(probs.numel(), acc.numel()) < N * H * W * Cn:
        raise ValueError("predict_accumulate: buffers are smaller than N x H x W x C")
    _lib.call("stp_predict_accumulate", ptr(_dev(probs)), ptr(_dev(acc)), N, H, W, Cn, int(flip), stream())


# dihedral test-time augmentation (csrc/dihedral.hip): op 0..7 = transpose if op & 4, then columns reversed if op & 1, then rows
# reversed if op & 2; src / acc are [N, H, W, C], dst / probs [N, H', W', C] with (H', W') = (W, H) for the transposing ops
def dihedral_u8(src, dst, N, H, W, Cn, op):
    if min(src.numel(), dst.numel()) < N * H * W * Cn:
        raise ValueError("dihedral_u8: buffers are smaller than N x H x W x C")
    _lib.call("stp_dihedral_u8", ptr(_dev(src)), ptr(_dev(dst)), N, H, W, Cn, int(op), stream())


def predict_accumulate_dihedral(probs, acc, N, H, W, Cn, op):
    if min(probs.numel(), acc.numel()) < N * H * W * Cn:
        raise ValueError("predict_accumulate_dihedral: buffers are smaller than N x H x W x C")
    _lib.call("stp_predict_accumulate_dihedral", ptr(_dev(probs)), ptr(_dev(acc)), N, H, W, Cn, int(op), stream())


def predict_finish(acc, H, W, Cn, k, mode, out, h, w, out_ld=None):
    """``acc``: ONE image's [H, W, Cn] sums; ``out``: fp32 (mode 0) or uint8 (1: bytes, 2: labels) whose first element is the map's
    top-left corner - a view into a larger map with ``out_ld`` pixels per row writes a rectangle of it."""
    out_ld = w if out_ld is None else int(out_ld)
    per_px = 1 if mode == 2 else Cn
    room = out.untyped_storage().nbytes() // out.element_size() - out.storage_offset()      # elements from the corner to the storage's end
    if acc.numel() < H * W * Cn or (out_ld >= w and room < ((h - 1) * out_ld + w) * per_px):
        raise ValueError("predict_finish: buffers are smaller than the maps")
    if mode in (0, 1, 2) and out.dtype != (torch.float32 if mode == 0 else torch.uint8):
        raise ValueError("predict_finish: mode %d writes %s" % (mode, "float32" if mode == 0 else "uint8"))
    _lib.call("stp_predict_finish", ptr(_dev(acc)), H, W, Cn, int(k), int(mode), ptr(_dev(out)), h, w, out_ld, stream())


# sliding-window prediction on the device (csrc/window.hip): ``origins`` is a HOST sequence of (y0, x0) pairs; an entry point takes up to
# 64 windows, a longer sequence goes down in slices of 64, in order
WINDOWS_PER_CALL = 64


def _origin_slices(origins):
    flat = [(int(y0), int(x0)) for y0, x0 in origins]
    for s in range(0, len(flat), WINDOWS_PER_CALL):
        part = flat[s:s + WINDOWS_PER_CALL]
        yield s, len(part), (C.c_int32 * (2 * len(part)))(*[v for yx in part for v in yx])


def window_gather_u8(img, h, w, Cn, origins, dst, H, W):
    """``dst`` uint8 [n, H, W, Cn] = the windows of the uint8 image ``img`` [h, w, Cn] at ``origins``, coordinates clipped to the image."""
    if not len(origins) or img.numel() < h * w * Cn or dst.numel() < len(origins) * H * W * Cn:
        raise ValueError("window_gather_u8: no window, or buffers smaller than the image / n x H x W x C")
    if img.dtype != torch.uint8 or dst.dtype != torch.uint8:
        raise ValueError("window_gather_u8: uint8 in, uint8 out")
    flat = _dev(dst).view(-1)
    for s, n, org in _origin_slices(origins):
        _lib.call("stp_window_gather_u8", ptr(_dev(img)), h, w, Cn, org, n, ptr(flat[s * H * W * Cn:]), H, W, stream())


def window_accumulate(acc, H, W, Cn, origins, overlap, canvas, h, w):
    """``canvas`` fp32 [h, w, Cn] += the ramp-weighted sums ``acc`` fp32 [n, H, W, Cn] of the windows at ``origins``, in their order."""
    if not len(origins) or acc.numel() < len(origins) * H * W * Cn or canvas.numel() < h * w * Cn:
        raise ValueError("window_accumulate: no window, or buffers smaller than n x H x W x C / the canvas")
    if acc.dtype != torch.float32 or canvas.dtype != torch.float32:
        raise ValueError("window_accumulate: float32 in, float32 out")
    flat = _dev(acc).view(-1)
    for s, n, org in _origin_slices(origins):
        _lib.call("stp_window_accumulate", ptr(flat[s * H * W * Cn:]), H, W, Cn, org, n, int(overlap), ptr(_dev(canvas)), h, w, stream())


def window_finish(canvas, h, w, Cn, k, sy, sx, mode, out, out_ld=None):
    """``out`` (fp32 for mode 0, uint8 for 1: bytes, 2: labels; ``out_ld`` pixels per row) = ``canvas / (k * sy[y] * sx[x])``, finished as
    ``predict_finish`` finishes a map; ``sy`` / ``sx``: fp32 device tables of the per-axis weight sums."""
    out_ld = w if out_ld is None else int(out_ld)
    per_px = 1 if mode == 2 else Cn
    room = out.untyped_storage().nbytes() // out.element_size() - out.storage_offset()      # elements from the corner to the storage's end
    if canvas.numel() < h * w * Cn or sy.numel() < h or sx.numel() < w or (out_ld >= w and room < ((h - 1) * out_ld + w) * per_px):
        raise ValueError("window_finish: buffers are smaller than the maps")
    if canvas.dtype != torch.float32 or sy.dtype != torch.float32 or sx.dtype != torch.float32:
        raise ValueError("window_finish: a float32 canvas and float32 weight sums")
    if mode in (0, 1, 2) and out.dtype != (torch.float32 if mode == 0 else torch.uint8):
        raise ValueError("window_finish: mode %d writes %s" % (mode, "float32" if mode == 0 else "uint8"))
    _lib.call("stp_window_finish", ptr(_dev(canvas)), h, w, Cn, int(k), ptr(_dev(sy)), ptr(_dev(sx)), int(mode), ptr(_dev(out)), out_ld, stream())


# masks on the device (csrc/mask.hip): ONE image's finished fp32 map [h, w, Cn] -> uint8 {0, 1} masks, their run-length code, sweep counters
def mask_threshold(probs, h, w, Cn, channel, mode, threshold, out, out_ld=None):
    """``out`` uint8 [h, out_ld]: mode 0 ``probs[:, :, channel] > float32(threshold)``, mode 1 ``argmax == channel`` (first largest)."""
    out_ld = w if out_ld is None else int(out_ld)
    room = out.untyped_storage().nbytes() - out.storage_offset()
    if probs.numel() < h * w * Cn or (out_ld >= w and room < (h - 1) * out_ld + w):
        raise ValueError("mask_threshold: buffers are smaller than the maps")
    if probs.dtype != torch.float32 or out.dtype != torch.uint8:
        raise ValueError("mask_threshold: float32 in, uint8 out")
    _lib.call("stp_mask_threshold", ptr(_dev(probs)), h, w, Cn, int(channel), int(mode), float(threshold), ptr(_dev(out)), out_ld, stream())


def mask_morph(src, dst, h, w, r, op):
    """``dst`` = erosion (op 0) / dilation (op 1) of the uint8 mask ``src`` [h, w] by disk(r), zeros outside the image."""
    if min(src.numel(), dst.numel()) < h * w or src.dtype != torch.uint8 or dst.dtype != torch.uint8:
        raise ValueError("mask_morph: two uint8 buffers of h x w")
    _lib.call("stp_mask_morph", ptr(_dev(src)), ptr(_dev(dst)), h, w, int(r), int(op), stream())


def mask_rle_workspace_bytes(h, w):
    return int(_lib.load().stp_mask_rle_workspace_bytes(h, w))


def mask_rle(img, h, w, runs, count, workspace):
    """``runs`` int32 [capacity, 2] = (start, length) of the column-major runs of the uint8 mask ``img`` [h, w], ``count`` int32 [1]."""
    if img.numel() < h * w or img.dtype != torch.uint8 or runs.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() < 1:
        raise ValueError("mask_rle: a uint8 image of h x w, int32 runs and count")
    _lib.call("stp_mask_rle", ptr(_dev(img)), h, w, ptr(_dev(runs)), ptr(_dev(count)), runs.numel() // 2, ptr(_dev(workspace)),
              workspace.numel() * workspace.element_size(), stream())


def threshold_counts_workspace_bytes(T):
    return int(_lib.load().stp_threshold_counts_workspace_bytes(T))


def threshold_counts(probs, target, h, w, Cn, channel, thresholds, counts, totals, workspace):
    """``counts`` int64 [T, 2] = (pixels above thresholds[t], those of them on the target), ``totals`` int64 [2] = (target positives, h * w);
    ``thresholds``: a host sequence, rounded to float32 here."""
    if probs.numel() < h * w * Cn or target.numel() < h * w or probs.dtype != torch.float32 or target.dtype != torch.uint8:
        raise ValueError("threshold_counts: a float32 map of h x w x C and a uint8 target of h x w")
    T = len(thresholds)
    if counts.dtype != torch.int64 or totals.dtype != torch.int64 or counts.numel() < 2 * T or totals.numel() < 2:
        raise ValueError("threshold_counts: int64 counts [T, 2] and totals [2]")
    thr = (C.c_float * max(T, 1))(*[float(t) for t in thresholds])
    _lib.call("stp_threshold_counts", ptr(_dev(probs)), ptr(_dev(target)), h, w, Cn, int(channel), thr, T, ptr(_dev(counts)), ptr(_dev(totals)),
              ptr(_dev(workspace)), workspace.numel() * workspace.element_size(), stream())


# connected components on the device (csrc/components.hip): ONE uint8 mask [h, w] -> its label image, its area-filtered mask, label runs
def _nbytes(t):
    return t.numel() * t.element_size()


def mask_label_workspace_bytes(h, w):
    return int(_lib.load().stp_mask_label_workspace_bytes(h, w))


def mask_label(img, h, w, connectivity, invert, labels, count, workspace):
    """``labels`` int32 [h, w] = scipy.ndimage.label of ``(img != 0) != invert`` (connectivity 1: 4-, 2: 8-neighbourhood), ``count`` int32 [1]."""
    if (img.numel() < h * w or labels.numel() < h * w or img.dtype != torch.uint8 or labels.dtype != torch.int32 or count.dtype != torch.int32
            or count.numel() < 1):
        raise ValueError("mask_label: a uint8 image and int32 labels of h x w, an int32 count")
    _lib.call("stp_mask_label", ptr(_dev(img)), h, w, int(connectivity), int(invert), ptr(_dev(labels)), ptr(_dev(count)),
              ptr(_dev(workspace)), _nbytes(workspace), stream())


def mask_area_filter_workspace_bytes(h, w):
    return int(_lib.load().stp_mask_area_filter_workspace_bytes(h, w))


def mask_area_filter(src, dst, h, w, connectivity, invert, min_size, workspace):
    """``dst`` uint8 {0, 1} = ``src != 0`` without its components of fewer than ``min_size`` pixels (invert 0: remove_small_objects) or with
    its zero components of fewer than ``min_size`` pixels set (invert 1: remove_small_holes); ``dst`` may be ``src``."""
    if min(src.numel(), dst.numel()) < h * w or src.dtype != torch.uint8 or dst.dtype != torch.uint8:
        raise ValueError("mask_area_filter: two uint8 buffers of h x w")
    _lib.call("stp_mask_area_filter", ptr(_dev(src)), ptr(_dev(dst)), h, w, int(connectivity), int(invert), int(min_size),
              ptr(_dev(workspace)), _nbytes(workspace), stream())


def label_rle_workspace_bytes(h, w):
    return int(_lib.load().stp_label_rle_workspace_bytes(h, w))


def label_rle(labels, h, w, runs, count, workspace):
    """``runs`` int32 [capacity, 3] = (value, start, length) of the column-major runs of equal non-zero values of the int32 image ``labels``
    [h, w], ``count`` int32 [1]."""
    if labels.numel() < h * w or labels.dtype != torch.int32 or runs.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() < 1:
        raise ValueError("label_rle: an int32 image of h x w, int32 runs and count")
    _lib.call("stp_label_rle", ptr(_dev(labels)), h, w, ptr(_dev(runs)), ptr(_dev(count)), runs.numel() // 3, ptr(_dev(workspace)),
              _nbytes(workspace), stream())


# object-level matching on the device (csrc/object_match.hip): two int32 label images [h, w] -> true positives per IoU threshold, overlaps
def label_match_workspace_bytes(h, w):
    return int(_lib.load().stp_label_match_workspace_bytes(h, w))


def label_match(pred, truth, h, w, label_cap, iou_num, iou_den, out, workspace):
    """``out`` int64 [T + 3] = (TP_k for the T thresholds ``iou_num[k] / iou_den`` - a host sequence of integers -, pred labels, truth
    labels, out-of-range pixels) of the int32 label images ``pred`` and ``truth`` [h, w] with values 0..label_cap."""
    if pred.numel() < h * w or truth.numel() < h * w or pred.dtype != torch.int32 or truth.dtype != torch.int32:
        raise ValueError("label_match: two int32 label images of h x w")
    T = len(iou_num)
    if out.dtype != torch.int64 or out.numel() < T + 3:
        raise ValueError("label_match: int64 out [T + 3]")
    num = (C.c_int32 * max(T, 1))(*[int(v) for v in iou_num])
    _lib.call("stp_label_match", ptr(_dev(pred)), ptr(_dev(truth)), h, w, int(label_cap), num, T, int(iou_den), ptr(_dev(out)),
              ptr(_dev(workspace)), _nbytes(workspace), stream())


def label_overlaps_workspace_bytes(h, w):
    return int(_lib.load().stp_label_overlaps_workspace_bytes(h, w))


def label_overlaps(pred, truth, h, w, label_cap, triples, count, area_p, area_g, out_of_range, workspace):
    """``triples`` int32 [capacity, 3] = (a, b, pixels with pred = a and truth = b) of the non-empty pairs in no particular order, ``count``
    int32 [1]; ``area_p`` / ``area_g`` int32 [label_cap + 1] = the labels' pixel counts; ``out_of_range`` int64 [1]."""
    if pred.numel() < h * w or truth.numel() < h * w or pred.dtype != torch.int32 or truth.dtype != torch.int32:
        raise ValueError("label_overlaps: two int32 label images of h x w")
    if (triples.dtype != torch.int32 or count.dtype != torch.int32 or count.numel() < 1 or area_p.dtype != torch.int32
            or area_g.dtype != torch.int32 or min(area_p.numel(), area_g.numel()) < label_cap + 1 or out_of_range.dtype != torch.int64
            or out_of_range.numel() < 1):
        raise ValueError("label_overlaps: int32 triples and count, int32 areas [label_cap + 1], an int64 out-of-range count")
    _lib.call("stp_label_overlaps", ptr(_dev(pred)), ptr(_dev(truth)), h, w, int(label_cap), ptr(_dev(triples)), ptr(_dev(count)),
              triples.numel() // 3, ptr(_dev(area_p)), ptr(_dev(area_g)), ptr(_dev(out_of_range)), ptr(_dev(workspace)), _nbytes(workspace),
              stream())


# splitting touching objects on the device (csrc/split.hip): ONE uint8 mask [h, w] -> its squared distance transform, cores, grown labels
def mask_edt_workspace_bytes(h, w):
    return int(_lib.load().stp_mask_edt_workspace_bytes(h, w))


def mask_edt(img, h, w, d2, workspace):
    """``d2`` int32 [h, w] = the exact squared Euclidean distance of every foreground pixel of the uint8 mask ``img`` to its nearest zero
    pixel, 0 off the foreground, 2147483647 everywhere when the mask has no zero."""
    if img.numel() < h * w or d2.numel() < h * w or img.dtype != torch.uint8 or d2.dtype != torch.int32:
        raise ValueError("mask_edt: a uint8 image and an int32 distance image of h x w")
    _lib.call("stp_mask_edt", ptr(_dev(img)), h, w, ptr(_dev(d2)), ptr(_dev(workspace)), _nbytes(workspace), stream())


def edt_threshold(d2, h, w, c2, out):
    """``out`` uint8 [h, w] = ``d2 > c2`` (c2 an integer >= 0): the cores of ``mask_edt``'s image."""
    if d2.numel() < h * w or out.numel() < h * w or d2.dtype != torch.int32 or out.dtype != torch.uint8:
        raise ValueError("edt_threshold: an int32 distance image and a uint8 mask of h x w")
    _lib.call("stp_edt_threshold", ptr(_dev(d2)), h, w, int(c2), ptr(_dev(out)), stream())


def label_grow_workspace_bytes(h, w):
    return int(_lib.load().stp_label_grow_workspace_bytes(h, w))


def label_grow(mask, seeds, h, w, labels, changed, workspace):
    """``labels`` int32 [h, w] = the int32 ``seeds`` (0: none) grown through the uint8 ``mask``: every unlabelled foreground pixel takes
    the label that reaches it first over the 8-neighbourhood, the smaller one on a tie.  One stp_label_grow call makes a bounded number
    of rounds and leaves in ``changed`` (int32 [1]) whether the last still changed a pixel; this wrapper calls again from ``labels``
    until it is clear, reading the word once per call.  Returns the number of calls."""
    if (mask.numel() < h * w or seeds.numel() < h * w or labels.numel() < h * w or mask.dtype != torch.uint8 or seeds.dtype != torch.int32
            or labels.dtype != torch.int32 or changed.dtype != torch.int32 or changed.numel() < 1):
        raise ValueError("label_grow: a uint8 mask, int32 seeds and labels of h x w, an int32 changed word")
    per_call = int(_lib.load().stp_label_grow_rounds())
    src, calls = seeds, 0
    while True:
        _lib.call("stp_label_grow", ptr(_dev(mask)), ptr(_dev(src)), h, w, ptr(_dev(labels)), ptr(_dev(changed)), ptr(_dev(workspace)),
                  _nbytes(workspace), stream())
        calls += 1
        if int(changed[0].item()) == 0:
            return calls
        if calls * per_call >= h * w:          # a round that changes something labels a pixel: there are fewer than h * w of them
            raise _lib.StpError("stp_label_grow still changes pixels after %d rounds on a %d x %d image" % (calls * per_call, h, w))
        src = labels


def label_unclaimed(mask, labels, h, w, out):
    """``out`` uint8 [h, w] = the foreground pixels of ``mask`` whose int32 label is 0."""
    if (mask.numel() < h * w or labels.numel() < h * w or out.numel() < h * w or mask.dtype != torch.uint8 or labels.dtype != torch.int32
            or out.dtype != torch.uint8):
        raise ValueError("label_unclaimed: a uint8 mask, int32 labels and a uint8 output of h x w")
    _lib.call("stp_label_unclaimed", ptr(_dev(mask)), ptr(_dev(labels)), h, w, ptr(_dev(out)), stream())


def label_merge(rest, nc, nr, h, w, labels, total):
    """``labels[i] = rest[i] + nc`` where the int32 image ``rest`` is non-zero, ``total = nc + nr``; ``nc``, ``nr``, ``total``: int32 [1] on
    the device (``total`` is neither of the other two)."""
    if (rest.numel() < h * w or labels.numel() < h * w or rest.dtype != torch.int32 or labels.dtype != torch.int32
            or any(t.dtype != torch.int32 or t.numel() < 1 for t in (nc, nr, total))):
        raise ValueError("label_merge: two int32 label images of h x w, three int32 counts")
    _lib.call("stp_label_merge", ptr(_dev(rest)), ptr(_dev(nc)), ptr(_dev(nr)), h, w, ptr(_dev(labels)), ptr(_dev(total)), stream())


# per-object measurements on the device (csrc/measure.hip): ONE int32 label image [h, w] -> a table per label, the selection by area and
# confidence
def label_measure(labels, probs, h, w, C, channel, label_cap, sums, boxes, out_of_range):
    """``sums`` int64 [label_cap + 1, 4] = (area, sum of y, sum of x, sum of q) and ``boxes`` int32 [label_cap + 1, 4] = the closed box
    (min y, min x, max y, max x; (h, w, -1, -1) without a pixel) per value 0..label_cap of the int32 image ``labels``; q = (int)(clamp(p,
    0, 1) * 65535) of ``probs[..., channel]`` (fp32 [h, w, C]; None: no probabilities, q = 0).  ``out_of_range`` int64 [1] = the pixels
    whose value lies outside 0..label_cap (they count as background)."""
    if labels.numel() < h * w or labels.dtype != torch.int32:
        raise ValueError("label_measure: an int32 label image of h x w")
    if probs is not None and (probs.dtype != torch.float32 or probs.numel() < h * w * max(int(C), 1)):
        raise ValueError("label_measure: float32 probabilities of h x w x C, or None")
    if (sums.dtype != torch.int64 or boxes.dtype != torch.int32 or min(sums.numel(), boxes.numel()) < 4 * (int(label_cap) + 1)
            or out_of_range.dtype != torch.int64 or out_of_range.numel() < 1):
        raise ValueError("label_measure: int64 sums and int32 boxes [label_cap + 1, 4], an int64 out-of-range count")
    _lib.call("stp_label_measure", ptr(_dev(labels)), ptr(_dev(probs)), h, w, int(C), int(channel), int(label_cap), ptr(_dev(sums)),
              ptr(_dev(boxes)), ptr(_dev(out_of_range)), stream())


def label_select_workspace_bytes(label_cap):
    return int(_lib.load().stp_label_select_workspace_bytes(int(label_cap)))


def label_select(labels, h, w, label_cap, sums, boxes, min_area, conf_num, conf_den, out_labels, count, out_sums, out_boxes, workspace):
    """Keeps the labels of ``label_measure``'s table with ``area >= min_area`` (and > 0) and ``sum q * conf_den >= conf_num * 65535 * area``,
    in order, renumbered 1..count: ``out_labels`` int32 [h, w] (may be ``labels``), ``count`` int32 [1], ``out_sums`` / ``out_boxes`` = rows
    0..count of the table in the new numbering (room for label_cap + 1 rows; not the input tables)."""
    if labels.numel() < h * w or out_labels.numel() < h * w or labels.dtype != torch.int32 or out_labels.dtype != torch.int32:
        raise ValueError("label_select: two int32 label images of h x w")
    rows = 4 * (int(label_cap) + 1)
    if (sums.dtype != torch.int64 or out_sums.dtype != torch.int64 or boxes.dtype != torch.int32 or out_boxes.dtype != torch.int32
            or min(sums.numel(), out_sums.numel(), boxes.numel(), out_boxes.numel()) < rows or count.dtype != torch.int32
            or count.numel() < 1):
        raise ValueError("label_select: int64 sums and int32 boxes [label_cap + 1, 4] in and out, an int32 count")
    _lib.call("stp_label_select", ptr(_dev(labels)), h, w, int(label_cap), ptr(_dev(sums)), ptr(_dev(boxes)), int(min_area), int(conf_num),
              int(conf_den), ptr(_dev(out_labels)), ptr(_dev(count)), ptr(_dev(out_sums)), ptr(_dev(out_boxes)), ptr(_dev(workspace)),
              _nbytes(workspace), stream())


# U-Net border weight maps on the device (csrc/border_weight.hip): int32 label images [N, H, W] -> the fp32 weight map, and the one-class
# loss that takes it (csrc/loss_sigmoid.hip)
def border_weight_workspace_bytes(N, H, W):
    return int(_lib.load().stp_border_weight_workspace_bytes(int(N), int(H), int(W)))


def border_weight(labels, N, H, W, w0, sigma, radius, b0, b1, weights, workspace, d1sq=None, d2sq=None):
    """``weights`` float32 [N, H, W] = (b1 on the labelled pixels, b0 elsewhere) + w0 * exp(-(d1 + d2)^2 / (2 sigma^2)) on the background,
    d1 / d2 the distances to the nearest / second-nearest object of the int32 label images ``labels`` inside the (2 radius + 1)^2 window of
    the pixel's own sample (include/stp_hip.h).  ``d1sq`` / ``d2sq``: int32 [N, H, W] or None, the squared distances (-1: none)."""
    n = int(N) * int(H) * int(W)
    if labels.numel() < n or weights.numel() < n or labels.dtype != torch.int32 or weights.dtype != torch.float32:
        raise ValueError("border_weight: int32 labels and float32 weights of N x H x W")
    for d in (d1sq, d2sq):
        if d is not None and (d.dtype != torch.int32 or d.numel() < n):
            raise ValueError("border_weight: d1sq / d2sq are int32 of N x H x W, or None")
    _lib.call("stp_border_weight", ptr(_dev(labels)), int(N), int(H), int(W), float(w0), float(sigma), int(radius), float(b0), float(b1),
              ptr(_dev(weights)), ptr(_dev(d1sq)), ptr(_dev(d2sq)), ptr(_dev(workspace)), _nbytes(workspace), stream())


def sigmoid_bce_dice_weighted(logits, target, count, w_bce, w_dice, scalars, dlogits, dl_channels, grad_scale, workspace, pixel_weights):
    """``sigmoid_bce_dice`` with the cross-entropy weighted per pixel by ``pixel_weights`` (float32 [count], > 0); ``scalars`` float32 [16]:
    [13] weighted_binary_crossentropy, [15] the mean weight, [1] stays the unweighted binary_crossentropy."""
    if pixel_weights is not None and (pixel_weights.dtype != torch.float32 or pixel_weights.numel() < count):
        raise ValueError("sigmoid_bce_dice_weighted: float32 pixel weights, one per element")
    _lib.call("stp_sigmoid_bce_dice_weighted", ptr(logits), ptr(target), count, dt(logits), float(w_bce), float(w_dice), ptr(scalars),
              ptr(dlogits), dl_channels, float(grad_scale), ptr(workspace), workspace.numel() * workspace.element_size(),
              ptr(pixel_weights), stream())
