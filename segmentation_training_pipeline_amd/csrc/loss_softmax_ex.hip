// Multi-class softmax head with the whole loss registry but lovasz_loss: the weighted sum of categorical_crossentropy, dice_loss,
// iou_loss, jaccard_loss and focal_loss (oracle/losses.py) on p = softmax(z) and the one-hot y of the target class t, classes = 2..32:
//   categorical_crossentropy / dice_loss   exactly the forms of softmax_loss_partial_kernel / softmax_loss_grad_kernel (loss_softmax.hip)
//   iou_loss      1 - (I + 1) / U with I = sum p_t and U = pixels + sum p - I + 1: the sums the value pass takes anyway
//   jaccard_loss  per pixel 100 (1 - a / b), a = p_t + 100, b = 101 + sum_c p_c - p_t, mean over pixels - no class loop
//   focal_loss    gamma 2, alpha 0.25, q = clip(p, 1e-7, 1 - 1e-7): -0.25 (1 - q)^2 log q for c == t, -0.75 q^2 log(1 - q) otherwise, both
//                 means over pixels * classes elements; the clip passes no gradient; one v_log_f32 per class in both passes (the oracle's
//                 two constant cross terms, ~2.5e-22 per element, are left out as in loss_multilabel.hip)
// through the softmax: dz_k = p_k (G_k - sum_c G_c p_c), G = the weighted sum of the d / dp.
// Three launches as stp_softmax_cce_dice: value pass (one thread per pixel, the row in registers, 16 partial sums per workgroup, fixed
// order, no atomics) -> one-workgroup finalize in double (12 scalars, the layout of stp_sigmoid_loss_ex) -> gradient pass.  The passes
// are VALU-bound (see softmax_row.h), so the weights - launch-uniform - pick an INSTANCE: the focal class loops and the iou / jaccard
// terms are compiled out when their weights are zero.
//
// Two entry points on ONE body per pass; MASKED is a template parameter of every kernel:
//   stp_softmax_loss_ex      MASKED = false: every pixel counts, with weight 1
//   stp_softmax_loss_masked  MASKED = true: an ignore label and class weights (the arithmetic is fixed in include/stp_hip.h):
//     v_i = [t_i != ignore_label], class of a counted pixel min(t_i, classes - 1), omega_i = v_i w_class, n = sum_i v_i
//     categorical_crossentropy, jaccard_loss, focal_loss   means of omega_i x the per-pixel expression over the n counted pixels
//                   (n * classes elements for focal_loss) - Keras's class_weight / zero sample weight rule
//     dice_loss, iou_loss and the logged dice, iou, iot, binary_accuracy   from sums over the counted pixels; the weights do not enter
//     n and sum omega are columns 9 and 10 of the partial row and scalars 12 and 13.  n differs from batch to batch, so the gradient
//     pass reads it from scalars[12]: no launch argument holds 1 / pixels.
// The mask is a select on the per-pixel terms, never a branch around the row: every lane loads its row (an ignored row may hold
// anything - a select, unlike a product with 0, also drops a NaN) and arrives at the reduction epilogue; the gradient pass STORES the
// zero rows of ignored pixels (the buffer is not cleared between steps).
// The class weight is indexed by a per-lane value: a kernel-argument array indexed that way lives in scratch, so the `classes` weights
// are staged in LDS once per workgroup (128 bytes; 1.f each when class_weights is NULL) - one ds_read per pixel.
// The body is written in the masked form.  In the MASKED = false instances `on` is the constant true and omega the constant 1.f: every
// select folds to its first arm and every product with omega is exact (x * 1.f) and folds away, so they add what they added before
// the two forms met, in that order - and with no ignore label and weights of 1 the masked instances add the same values.
#include "loss_reduce.h"
#include "softmax_row.h"

#define SMX_NSUM 16
#define SMX_GRAD_MAX_BLOCKS 4096

// the workgroup's copy of the class weights; every thread of the workgroup calls this before its first pixel
__device__ __forceinline__ void smx_stage_weights(float* wsh, const float* __restrict__ class_weights, int classes) {
  if (threadIdx.x < STP_MAX_CLASSES) wsh[threadIdx.x] = (class_weights && (int)threadIdx.x < classes) ? class_weights[threadIdx.x] : 1.f;
  __syncthreads();
}

// focal_loss of one pixel, summed over its classes
template <int CM>
__device__ __forceinline__ float smx_focal_pixel(const float (&p)[CM], int t, int classes) {
  int imax;
  const float rest = smx_rest(p, &imax);
  float f = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    if (c < classes) {
      const float q = fminf(fmaxf(p[c], 1e-7f), 1.f - 1e-7f);
      const float omq = fminf(fmaxf(c == imax ? rest : 1.f - p[c], 1e-7f), 1.f - 1e-7f);      // 1 - q
      f += c == t ? -SMX_FOCAL_ALPHA * omq * omq * __logf(q) : -(1.f - SMX_FOCAL_ALPHA) * q * q * __logf(omq);
    }
  }
  return f;
}

// value pass: per-workgroup partials of (v = counted, om = omega; both 1 unless MASKED)
//   0 om cce_pixel  1 v sum_c p  2 v (= y: 1 per pixel)  3 v p_t  4 v [pmax>.5]  5 v [p_t>.5]  6 v count of th == y  7 om jaccard_pixel
//   8 om focal_e   MASKED: 9 v (= n)  10 om   (the rest of the 16 zero)
template <typename T, int CM, bool FOCAL, bool MASKED>
__global__ __launch_bounds__(256) void smx_partial_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target, int64_t pixels,
                                                          int classes, int ldc, bool vec, bool vec4, int ignore_label,
                                                          const float* __restrict__ class_weights, float* __restrict__ partial) {
  // (the LDS array is declared inside the `if constexpr` so that the unmasked instances own none; it has static storage, so the
  //  pointer outlives the block, and it is dereferenced under MASKED only)
  float* wsh = nullptr;
  if constexpr (MASKED) {
    __shared__ float weights[STP_MAX_CLASSES];
    smx_stage_weights(weights, class_weights, classes);
    wsh = weights;
  }
  float a[MASKED ? 11 : 9] = {};
  const int64_t per = (pixels + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < pixels ? i0 + per : pixels;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    float p[CM];
    softmax_row<T, CM>(logits + i * ldc, classes, vec, p, vec4);
    const int tr = target[i];
    const bool on = !MASKED || tr != ignore_label;
    const int t = tr < classes ? tr : classes - 1;
    float om = 1.f;
    if constexpr (MASKED) om = on ? wsh[t] : 0.f;
    float pt, pmax, psum;
    softmax_row_stats(p, t, pt, pmax, psum);
    // the closed forms of softmax_pixel_sums (softmax_row.h), each behind the select
    const float tt = pt > 0.5f ? 1.f : 0.f, tm = pmax > 0.5f ? 1.f : 0.f;
    a[1] += on ? psum : 0.f;
    a[2] += on ? 1.f : 0.f;
    a[3] += on ? pt : 0.f;
    a[4] += on ? tm : 0.f;
    a[5] += on ? tt : 0.f;
    a[6] += on ? (float)classes - (pt > 0.5f ? 0.f : 1.f + tm) : 0.f;
    // the omega-weighted terms: the term itself is selected (an ignored row may hold anything), then om * term joins the sum in one
    // expression - with om = 1 the fma adds exactly the term
    const float ce = on ? -__logf(fminf(fmaxf(pt, 1e-7f), 1.f - 1e-7f)) : 0.f;
    a[0] += om * ce;
    // jaccard: 1 - a / b = (b - a) / b with b - a = 1 + sum_c p_c - 2 p_t (no cancellation against the smooth term)
    const float jq = on ? __fdividef(1.f + psum - 2.f * pt, SMX_JACCARD_SMOOTH + 1.f + psum - pt) : 0.f;
    a[7] += om * SMX_JACCARD_SMOOTH * jq;
    if constexpr (MASKED) {
      a[9] += on ? 1.f : 0.f;
      a[10] += om;
    }
    if constexpr (FOCAL) {
      const float f = smx_focal_pixel(p, t, classes);
      a[8] += om * (on ? f : 0.f);
    }
  }
  loss_block_sums<SMX_NSUM>(a, partial);
}

// the 12 scalars of stp_sigmoid_loss_ex: 0 loss 1 categorical_crossentropy 2 dice_loss 3 dice 4 accuracy 5 sum_p 6 sum_y 7 sum_py 8 iou
// 9 iot 10 jaccard_loss 11 focal_loss; 1..9 as softmax_loss_finalize_kernel defines them.  The means are over the launch's pixels
// (the two reciprocals come with the launch); MASKED: over max(n, 1) counted pixels, and 12 n, 13 sum omega
template <bool MASKED>
__global__ __launch_bounds__(256) void smx_finalize_kernel(const float* partial, int blocks, int classes, double inv_pixels, double inv_elems,
                                                           LossWeights lw, float* scalars) {
  const double* s = loss_finalize_sums<SMX_NSUM>(partial, blocks);
  if (threadIdx.x != 0) return;
  if constexpr (MASKED) {
    const double n = s[9] > 1.0 ? s[9] : 1.0;
    inv_pixels = 1.0 / n;
    inv_elems = 1.0 / (n * classes);
  }
  loss_ex_scalars(s, loss_common_scalars(s, inv_pixels, inv_elems, scalars), lw, inv_pixels, inv_elems, scalars);
  if constexpr (MASKED) {
    scalars[12] = (float)s[9];
    scalars[13] = (float)s[10];
  }
}

// gradient pass: dL/dlogit of the `classes` channels x grad_scale into [pixels][dlc]; the padding channels of every row and (MASKED)
// the rows of ignored pixels exactly 0.  EXT: iou_loss or jaccard_loss carries a weight; FOCAL: focal_loss does.
template <typename T, int CM, bool EXT, bool FOCAL, bool MASKED>
__global__ __launch_bounds__(256) void smx_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target, int64_t pixels,
                                                       int classes, int ldc, bool vec, bool vec4, int ignore_label,
                                                       const float* __restrict__ class_weights, const float* __restrict__ scalars,
                                                       LossWeights lw, float inv_pixels, float inv_elems, float grad_scale,
                                                       T* __restrict__ dl, int dlc, bool vout) {
  float* wsh = nullptr;
  if constexpr (MASKED) {
    __shared__ float weights[STP_MAX_CLASSES];
    smx_stage_weights(weights, class_weights, classes);
    wsh = weights;
    // the counted pixels of THIS batch, as the finalize launch left them (n <= 2^24 is exact in the float)
    const double n = (double)fmaxf(scalars[12], 1.f);
    inv_pixels = (float)(1.0 / n);
    inv_elems = (float)(1.0 / (n * classes));
  }
  const float w_dice = lw.w[1];
  const DiceIouGrad k(scalars);
  const float den = k.den, inv_den2 = k.inv_den2, num = k.num, uden = k.uden, unum = k.unum, inv_uden2 = k.inv_uden2;
  // iou: d / dp_c = -(y_c U - (I + 1)(1 - y_c)) / U^2 -> one value for the target class, one for the others
  const float iou1 = -lw.w[2] * uden * inv_uden2, iou0 = lw.w[2] * unum * inv_uden2;
  const float wf = lw.w[4] * inv_elems;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    float p[CM];
    softmax_row<T, CM>(logits + i * ldc, classes, vec, p, vec4);
    const int tr = target[i];
    const bool on = !MASKED || tr != ignore_label;
    const int t = tr < classes ? tr : classes - 1;
    float om = 1.f;                                            // the class weight alone: an ignored row is zeroed whole at the store below
    if constexpr (MASKED) om = wsh[t];
    const float w_cce = lw.w[0] * om, wfo = wf * om;
    float pt = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) pt = c == t ? p[c] : pt;
    const bool inr = pt >= 1e-7f && pt <= 1.f - 1e-7f;   // the clip passes no gradient outside
    // dice: G_c = d dice_loss / d p_c = -(2 y_c den - num) / den^2 ; dz_k = p_k (G_k - sum_c G_c p_c)
    // sum_c G_c p_c with G_c = (num - 2 y_c den) / den^2: (num sum_c p_c - 2 den p_t) / den^2 - no loop over the classes
    float psum = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) psum += p[c];                                                           // p[c] = 0 beyond classes
    const float gp = (num * psum - 2.f * den * pt) * inv_den2;
    float g[CM];
    // iou and jaccard: E_c = d / dp_c = e1 for the target class, e0 for the rest, ge = sum_c E_c p_c
    float e0 = 0.f, e1 = 0.f, ge = 0.f;
    if constexpr (EXT) {
      // jaccard: d / dp_c = -100 (y_c b - a (1 - y_c)) / b^2 / pixels
      const float ja = pt + SMX_JACCARD_SMOOTH, jb = SMX_JACCARD_SMOOTH + 1.f + psum - pt;
      const float wj = lw.w[3] * om;
      const float jscale = wj * SMX_JACCARD_SMOOTH * __builtin_amdgcn_rcpf(jb * jb) * inv_pixels;
      e0 = iou0 + jscale * ja;
      e1 = iou1 - jscale * jb;
      ge = e0 * (psum - pt) + e1 * pt;
    }
    // focal: with F_c = d focal / dp_c, h_c = p_c F_c and H = sum_c h_c the logits get dz_k = h_k - p_k H.  For a class that is NOT the target
    // F_c grows as 1 / (1 - p_c) and h_k - p_k H cancels to O(1) from terms of that size - so the largest class m (the only one that can
    // have p > 0.5) is kept apart as u_m = h_m (1 - p_m), which has no division, and r = 1 - p_m (smx_rest):
    //   dz_m = u_m - p_m Hrest,   dz_k = h_k - p_k Hrest - u_m (p_k / r) for k != m   (Hrest = sum over c != m of h_c; p_k <= r)
    //   target:  h = 0.25 (2 p (1 - p) log p - (1 - p)^2)           others:  u = -0.75 (2 p^2 (1 - p) log(1 - p) - p^3), h = u / (1 - p)
    // (the per-element weight wfo carries omega)
    int imax = 0;
    float hrest = 0.f, umax = 0.f, rr = 0.f;
    if constexpr (FOCAL) {
      const float rest = smx_rest(p, &imax);
      rr = __builtin_amdgcn_rcpf(fmaxf(rest, 1e-37f));
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        const float pr = p[c];
        const float omp = c == imax ? rest : 1.f - pr;
        const bool in = pr >= 1e-7f && omp >= 1e-7f;             // the clip to [eps, 1 - eps] passes no gradient (false beyond `classes`: p = 0)
        const float lg = __logf(c == t ? pr : omp);
        const float w = (2.f * pr * omp * lg - (c == t ? omp * omp : pr * pr)) * (c == t ? wfo * SMX_FOCAL_ALPHA : -wfo * (1.f - SMX_FOCAL_ALPHA));
        // w = h for the target class, u / p for the others
        const float h = c == t ? w : w * pr * __builtin_amdgcn_rcpf(omp);
        const float u = c == t ? w * omp : w * pr;
        g[c] = in && c != imax ? h : 0.f;
        hrest += g[c];
        umax = in && c == imax ? u : umax;
      }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const float y = c == t ? 1.f : 0.f;
      float v = inr ? w_cce * (p[c] - y) * inv_pixels : 0.f;
      v += w_dice * p[c] * ((-(2.f * y * den - num) * inv_den2) - gp);
      if constexpr (EXT) v += p[c] * ((c == t ? e1 : e0) - ge);
      if constexpr (FOCAL) v += c == imax ? umax - p[c] * hrest : g[c] - p[c] * hrest - umax * (p[c] * rr);
      g[c] = (on && c < classes) ? v * grad_scale : 0.f;
    }
    softmax_grad_row_store<T, CM, true>(dl + i * dlc, g, classes, dlc, vout);
  }
}

template <typename T, int CM, bool MASKED>
static void smx_launch(const T* logits, const uint8_t* target, int64_t pixels, int classes, int ldc, const LossWeights& lw, float* scalars,
                       T* dl, int dlc, float grad_scale, float* ws, int ignore_label, const float* class_weights, hipStream_t s) {
  constexpr int V = Elem<T>::VEC;
  // the widest row access the stride and the base alignment allow: 16 bytes, 8 bytes (16-bit rows of 4 k elements), element by element
  const uintptr_t base = reinterpret_cast<uintptr_t>(logits);
  const bool vec = (ldc % V) == 0 && CM % V == 0 && (base & 15) == 0;
  const bool vec4 = !vec && sizeof(T) == 2 && (ldc % 4) == 0 && (CM % 4) == 0 && (base & 7) == 0;
  const bool focal = lw.w[4] != 0.f, ext = lw.w[2] != 0.f || lw.w[3] != 0.f;
  const int blocks = loss_value_blocks(pixels);
  const double inv_pixels = 1.0 / (double)pixels, inv_elems = 1.0 / ((double)pixels * classes);      // (the MASKED kernels take theirs from n)
  if (focal)
    hipLaunchKernelGGL((smx_partial_kernel<T, CM, true, MASKED>), dim3(blocks), dim3(256), 0, s, logits, target, pixels, classes, ldc, vec, vec4,
                       ignore_label, class_weights, ws);
  else
    hipLaunchKernelGGL((smx_partial_kernel<T, CM, false, MASKED>), dim3(blocks), dim3(256), 0, s, logits, target, pixels, classes, ldc, vec, vec4,
                       ignore_label, class_weights, ws);
  hipLaunchKernelGGL(smx_finalize_kernel<MASKED>, dim3(1), dim3(256), 0, s, ws, blocks, classes, inv_pixels, inv_elems, lw, scalars);
  if (!dl) return;
  const bool vout = (dlc % V) == 0 && (reinterpret_cast<uintptr_t>(dl) & 15) == 0;
  const int g = loss_grad_blocks(pixels, SMX_GRAD_MAX_BLOCKS);
#define SMX_GRAD(EXT, FOCAL)                                                                                                              \
  hipLaunchKernelGGL((smx_grad_kernel<T, CM, EXT, FOCAL, MASKED>), dim3(g), dim3(256), 0, s, logits, target, pixels, classes, ldc, vec, vec4, \
                     ignore_label, class_weights, scalars, lw, (float)inv_pixels, (float)inv_elems, grad_scale, dl, dlc, vout)
  if (focal) {
    if (ext) SMX_GRAD(true, true); else SMX_GRAD(false, true);
  } else {
    if (ext) SMX_GRAD(true, false); else SMX_GRAD(false, false);
  }
#undef SMX_GRAD
}

// both entry points: stp_softmax_loss_ex passes ignore_label -1 and no class weights
template <bool MASKED>
static int smx_entry(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype, const float* weights5,
                     float* scalars, void* dlogits, int32_t dl_channels, float grad_scale, void* workspace, size_t workspace_bytes,
                     int32_t ignore_label, const float* class_weights, void* stream) {
  const int rc = loss_check(dtype, logits && target && weights5 && scalars && workspace && pixels > 0 && classes >= 2 && classes <= STP_MAX_CLASSES &&
                                       ldc >= classes && dl_channels >= classes && ignore_label >= -1 && ignore_label <= 255,
                            workspace_bytes, stp_loss_workspace_bytes());
  if (rc != STP_OK) return rc;
  const LossWeights lw = loss_weights(weights5);
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    loss_by_class_bucket(classes, [&](auto bucket) {
      smx_launch<T, decltype(bucket)::value, MASKED>((const T*)logits, target, pixels, classes, ldc, lw, scalars, (T*)dlogits, dl_channels,
                                                     grad_scale, (float*)workspace, ignore_label, class_weights, (hipStream_t)stream);
    });
  });
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_softmax_loss_ex(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                                   const float* weights5, float* scalars, void* dlogits, int32_t dl_channels, float grad_scale,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return smx_entry<false>(logits, target, pixels, classes, ldc, dtype, weights5, scalars, dlogits, dl_channels, grad_scale, workspace,
                          workspace_bytes, -1, nullptr, stream);
}

extern "C" int stp_softmax_loss_masked(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                                       const float* weights5, float* scalars, void* dlogits, int32_t dl_channels, float grad_scale,
                                       void* workspace, size_t workspace_bytes, int32_t ignore_label, const float* class_weights,
                                       void* stream) {
  return smx_entry<true>(logits, target, pixels, classes, ldc, dtype, weights5, scalars, dlogits, dl_channels, grad_scale, workspace,
                         workspace_bytes, ignore_label, class_weights, stream);
}
