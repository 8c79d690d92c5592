// The losses on PROBABILITIES: the in-tree DeepLabV3+ applies its activation inside the last 1x1 convolution and upsamples the
// probabilities (segmentation_pipeline/impl/deeplab/model.py:485-486).  Reductions: loss_reduce.h.
#include "loss_reduce.h"

#define PL_NSUM 8
#define PL_GRAD_MAX_BLOCKS 16384
#define PL_WORKSPACE_BYTES ((size_t)LOSS_MAX_BLOCKS * PL_NSUM * sizeof(float))

// ------------------------------------------------------------------------------------------
// w_bce * binary_crossentropy + w_dice * dice_loss on PROBABILITIES (1 class), scalars as stp_sigmoid_bce_dice, and the
// gradient w.r.t. the probabilities into column 0 of dprobs [count][dl_channels]:
//   d bce / d p = (p - y) / (p (1 - p)) / count inside the Keras clip [1e-7, 1 - 1e-7], 0 outside;  d dice_loss / d p = -(2 y den - num) / den^2
template <typename T>
__global__ __launch_bounds__(256) void prob_loss_partial_kernel(const T* __restrict__ probs, const uint8_t* __restrict__ target, int64_t count,
                                                                float* partial) {
  float a[PL_NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t per = (count + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < count ? i0 + per : count;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float p = Elem<T>::load(probs + i);
    const float y = target[i] ? 1.f : 0.f;
    const float pc = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
    const float z = logf(pc / (1.f - pc));
    a[0] += fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
    a[1] += p;
    a[2] += y;
    a[3] += p * y;
    const float t = p > 0.5f ? 1.f : 0.f;
    a[4] += t;
    a[5] += t * y;
    a[6] += (t == y) ? 1.f : 0.f;
  }
  loss_block_sums<PL_NSUM>(a, partial);
}
__global__ __launch_bounds__(256) void prob_loss_finalize_kernel(const float* partial, int blocks, double inv_count, float w_bce, float w_dice,
                                                                 float* scalars) {
  const double* s = loss_finalize_sums<PL_NSUM>(partial, blocks);
  if (threadIdx.x != 0) return;
  const LossTerms t = loss_common_scalars(s, inv_count, inv_count, scalars);
  scalars[0] = (float)(w_bce * t.first + w_dice * t.dice_l);
}
template <typename T>
__global__ __launch_bounds__(256) void prob_loss_grad_kernel(const T* __restrict__ probs, const uint8_t* __restrict__ target, int64_t count,
                                                             const float* scalars, float w_bce, float w_dice, float inv_count, T* __restrict__ dp,
                                                             int dlc) {
  const DiceIouGrad k(scalars);
  const float den = k.den, inv_den2 = k.inv_den2, num = k.num;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const float p = Elem<T>::load(probs + i);
    const float y = target[i] ? 1.f : 0.f;
    const bool inr = p >= 1e-7f && p <= 1.f - 1e-7f;
    float g = inr ? w_bce * (p - y) / (p * (1.f - p)) * inv_count : 0.f;
    g += w_dice * (-(2.f * y * den - num) * inv_den2);
    T* o = dp + i * dlc;
    Elem<T>::store(o, g);
    for (int c = 1; c < dlc; ++c) Elem<T>::store(o + c, 0.f);
  }
}

extern "C" int stp_prob_bce_dice(const void* probs, const uint8_t* target, int64_t count, int32_t dtype, float w_bce, float w_dice,
                                 float* scalars, void* dprobs, int32_t dl_channels, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = loss_check(dtype, probs && target && scalars && workspace && count > 0, workspace_bytes, PL_WORKSPACE_BYTES);
  if (rc != STP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = loss_value_blocks(count);
  float* partial = (float*)workspace;
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(prob_loss_partial_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)probs, target, count, partial);
  });
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(prob_loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)count, w_bce, w_dice, scalars);
  STP_LAUNCH_CHECK();
  if (dprobs) {
    if (dl_channels < 1) return STP_E_BADARG;
    const int g = loss_grad_blocks(count, PL_GRAD_MAX_BLOCKS);
    const float inv_count = (float)(1.0 / (double)count);
    loss_by_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(prob_loss_grad_kernel<T>, dim3(g), dim3(256), 0, s, (const T*)probs, target, count, scalars, w_bce, w_dice, inv_count,
                         (T*)dprobs, dl_channels);
    });
    STP_LAUNCH_CHECK();
  }
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// Multi-class loss on PROBABILITIES (the model resizes the softmax output, model.py:485-486): Keras categorical_crossentropy
// (p <- p / sum p, clip to [1e-7, 1 - 1e-7], -log p_target) + w_dice * musket dice over every (pixel, class) element of the
// one-hot target.  probs [pixels][ldc], target = class index per pixel; scalars as stp_softmax_cce_dice; the gradient
// w.r.t. the probabilities goes to dprobs [pixels][dl_channels] (zero padding).  One thread per pixel.
//   d cce / d p_k = -([k == t] / p_t - 1 / S) / pixels  where the clip is inactive on q_t = p_t / S, else 0
template <typename T>
__global__ __launch_bounds__(256) void prob_cce_partial_kernel(const T* __restrict__ probs, const uint8_t* __restrict__ target, int64_t pixels,
                                                               int classes, int ldc, float* partial) {
  float a[PL_NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t per = (pixels + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < pixels ? i0 + per : pixels;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const T* pr = probs + i * ldc;
    const int t = target[i];
    float S = 0.f;
    for (int c = 0; c < classes; ++c) S += Elem<T>::load(pr + c);
    for (int c = 0; c < classes; ++c) {
      const float p = Elem<T>::load(pr + c), y = c == t ? 1.f : 0.f;
      a[1] += p;
      a[3] += p * y;
      const float th = p > 0.5f ? 1.f : 0.f;
      a[4] += th;
      a[5] += th * y;
      a[6] += (th == y) ? 1.f : 0.f;
      if (c == t) a[0] += -logf(fminf(fmaxf(p / S, 1e-7f), 1.f - 1e-7f));
    }
    a[2] += (t < classes) ? 1.f : 0.f;
  }
  loss_block_sums<PL_NSUM>(a, partial);
}
// sum 0 is per PIXEL, sum 6 per (pixel, class) element
__global__ __launch_bounds__(256) void prob_cce_finalize_kernel(const float* partial, int blocks, double inv_pixels, double inv_elems, float w_cce,
                                                                float w_dice, float* scalars) {
  const double* s = loss_finalize_sums<PL_NSUM>(partial, blocks);
  if (threadIdx.x != 0) return;
  const LossTerms t = loss_common_scalars(s, inv_pixels, inv_elems, scalars);
  scalars[0] = (float)(w_cce * t.first + w_dice * t.dice_l);
}
template <typename T>
__global__ __launch_bounds__(256) void prob_cce_grad_kernel(const T* __restrict__ probs, const uint8_t* __restrict__ target, int64_t pixels, int classes,
                                                            int ldc, const float* scalars, float w_cce, float w_dice, float inv_pixels,
                                                            T* __restrict__ dp, int dlc) {
  const DiceIouGrad k(scalars);
  const float den = k.den, inv_den2 = k.inv_den2, num = k.num;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    const T* pr = probs + i * ldc;
    const int t = target[i];
    float S = 0.f;
    for (int c = 0; c < classes; ++c) S += Elem<T>::load(pr + c);
    const float pt = t < classes ? Elem<T>::load(pr + t) : 0.f;
    const float q = pt / S;
    const bool inr = t < classes && q >= 1e-7f && q <= 1.f - 1e-7f;
    T* o = dp + i * dlc;
    for (int c = 0; c < dlc; ++c) {
      float g = 0.f;
      if (c < classes) {
        const float y = c == t ? 1.f : 0.f;
        if (inr) g = -w_cce * (y / pt - 1.f / S) * inv_pixels;
        g += w_dice * (-(2.f * y * den - num) * inv_den2);
      }
      Elem<T>::store(o + c, g);
    }
  }
}

extern "C" int stp_prob_cce_dice(const void* probs, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype, float w_cce,
                                 float w_dice, float* scalars, void* dprobs, int32_t dl_channels, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  // (a gradient row narrower than the classes is refused before anything is launched)
  const int rc = loss_check(dtype, probs && target && scalars && workspace && pixels > 0 && classes >= 2 && classes <= 32 && ldc >= classes &&
                                       !(dprobs && dl_channels < classes),
                            workspace_bytes, PL_WORKSPACE_BYTES);
  if (rc != STP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = loss_value_blocks(pixels, 512);
  float* partial = (float*)workspace;
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(prob_cce_partial_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)probs, target, pixels, classes, ldc, partial);
  });
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(prob_cce_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)pixels, 1.0 / ((double)pixels * classes), w_cce,
                     w_dice, scalars);
  STP_LAUNCH_CHECK();
  if (dprobs) {
    const int g = loss_grad_blocks(pixels, PL_GRAD_MAX_BLOCKS);
    loss_by_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(prob_cce_grad_kernel<T>, dim3(g), dim3(256), 0, s, (const T*)probs, target, pixels, classes, ldc, scalars, w_cce, w_dice,
                         (float)(1.0 / (double)pixels), (T*)dprobs, dl_channels);
    });
    STP_LAUNCH_CHECK();
  }
  return STP_OK;
}
