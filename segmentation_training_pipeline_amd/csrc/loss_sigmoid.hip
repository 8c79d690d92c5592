// The one-class sigmoid head: sigmoid + Keras binary_crossentropy + musket dice (stp_sigmoid_bce_dice), the whole loss registry but
// lovasz_loss (stp_sigmoid_loss_ex), the class convolution's bias gradient and the plain sigmoid.  HBM-bound streaming kernels on the
// two-stage fixed-order reduction of loss_reduce.h.
#include "loss_reduce.h"

#define LOSS_NSUM 8

// ------------------------------------------------------------------------------------------
// pass 1: per-block partial sums of
//   0 bce_i   1 p   2 y   3 p*y   4 [p>.5]   5 [p>.5]*y   6 [(p>.5)==y]   7 unused
// Keras/TF binary_crossentropy on probabilities: clip p to [eps, 1-eps], go back to logits,
// sigmoid_cross_entropy_with_logits.  Returns the loss term; in_range tells whether the clip
// was inactive (gradient flows).
__device__ __forceinline__ float keras_bce(float p, float y, bool* in_range) {
  const float eps = 1e-7f, hi = 1.f - 1e-7f;
  const float pc = fminf(fmaxf(p, eps), hi);
  *in_range = (p >= eps) && (p <= hi);
  const float z = logf(pc / (1.f - pc));
  return fmaxf(z, 0.f) - z * y + log1pf(expf(-fabsf(z)));
}

// The same expression on the hardware transcendentals (v_exp_f32 / v_log_f32, ~1 ulp): the value pass of the headline loss was
// VALU-bound on the library expf / logf / log1pf (five per pixel: 23.6 us for 12 MB at 16 x 512 x 512, whatever the grid).  Each
// term moves by <= 3e-7 absolute; the tests hold the loss to 1e-5 relative.  (The gradient pass only needs the sigmoid.)
__device__ __forceinline__ float keras_bce_fast(float p, float y) {
  const float eps = 1e-7f, hi = 1.f - 1e-7f;
  const float pc = fminf(fmaxf(p, eps), hi);
  const float z = __logf(pc / (1.f - pc));
  return fmaxf(z, 0.f) - z * y + __logf(1.f + __expf(-fabsf(z)));
}

template <typename T>
__global__ __launch_bounds__(256) void loss_partial_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                           int64_t count, float* partial) {
  float a[LOSS_NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto one = [&a](float z, bool tgt) __attribute__((always_inline)) {
    const float y = tgt ? 1.f : 0.f;
    const float p = 1.f / (1.f + __expf(-z));
    a[0] += keras_bce_fast(p, y);
    a[1] += p;
    a[2] += y;
    a[3] += p * y;
    const float t = p > 0.5f ? 1.f : 0.f;
    a[4] += t;
    a[5] += t * y;
    a[6] += (t == y) ? 1.f : 0.f;
  };
  if constexpr (sizeof(T) == 2) {
    // 16-bit logits: 8 pixels per thread and iteration (16 + 8 bytes), two iterations in flight.  One pixel per iteration with a run-time
    // trip count kept ONE 2-byte load in flight per thread: 16 dependent memory round trips = 28 us for 12 MB at 16 x 512 x 512.
    if ((count & 7) == 0 && ((uintptr_t)logits & 15) == 0 && ((uintptr_t)target & 7) == 0) {
      const int64_t groups = count >> 3, per = (groups + gridDim.x - 1) / gridDim.x;
      const int64_t g0 = (int64_t)blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
      auto eight = [&one](const u32x4& zz, const u32x2& tt) __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t tw = e < 2 ? tt.x : tt.y;
          one(h16lo_to_f32(zz[e]), ((tw >> (16 * (e & 1))) & 0xffu) != 0);
          one(h16hi_to_f32(zz[e]), ((tw >> (16 * (e & 1) + 8)) & 0xffu) != 0);
        }
      };
      int64_t g = g0 + threadIdx.x;
      for (; g + 256 < g1; g += 512) {
        const u32x4 z0 = *reinterpret_cast<const u32x4*>(logits + g * 8), z1 = *reinterpret_cast<const u32x4*>(logits + (g + 256) * 8);
        const u32x2 t0 = *reinterpret_cast<const u32x2*>(target + g * 8), t1 = *reinterpret_cast<const u32x2*>(target + (g + 256) * 8);
        eight(z0, t0);
        eight(z1, t1);
      }
      for (; g < g1; g += 256) eight(*reinterpret_cast<const u32x4*>(logits + g * 8), *reinterpret_cast<const u32x2*>(target + g * 8));
    } else {
      const int64_t per = (count + gridDim.x - 1) / gridDim.x;
      const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < count ? i0 + per : count;
      for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) one(Elem<T>::load(logits + i), target[i] != 0);
    }
  } else {
    const int64_t per = (count + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < count ? i0 + per : count;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) one(Elem<T>::load(logits + i), target[i] != 0);
  }
  // loss_block_sums<LOSS_NSUM>(a, partial), spelled out: through the call this kernel - and only this one - takes 89 instead of 80 vector
  // registers in the 16-bit builds, 5 instead of 6 waves per SIMD (same statements, another schedule of the unrolled loop above)
  __shared__ float red[4][LOSS_NSUM];
#pragma unroll
  for (int e = 0; e < LOSS_NSUM; ++e) a[e] = wave_sum(a[e]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int e = 0; e < LOSS_NSUM; ++e) red[threadIdx.x >> 6][e] = a[e];
  __syncthreads();
  if (threadIdx.x < LOSS_NSUM)
    partial[(size_t)blockIdx.x * LOSS_NSUM + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// scalars: 0 loss 1 bce 2 dice_loss 3 dice_metric 4 binary_accuracy 5 sum_p 6 sum_y 7 sum_py
// one workgroup: 8 sums x 32 strided lanes, then a fixed-shape LDS tree (deterministic)
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* partial, int blocks, double inv_count, float w_bce,
                                                            float w_dice, float* scalars) {
  const double* s = loss_finalize_sums<LOSS_NSUM>(partial, blocks);
  if (threadIdx.x != 0) return;
  const LossTerms t = loss_common_scalars(s, inv_count, inv_count, scalars);
  scalars[0] = (float)(w_bce * t.first + w_dice * t.dice_l);
}

// one row of the padded gradient tensor: g in channel 0, zeros behind it - ONE 16-byte store for the usual 8 x bf16 / 4 x fp32 row
// (returns the value as stored: the bias gradient below sums what the weight / data gradients will read)
__device__ __forceinline__ float store_grad_row(float* o, float g, int dlc) {
  if (dlc == 4) { *reinterpret_cast<f32x4*>(o) = f32x4{g, 0.f, 0.f, 0.f}; return g; }
  o[0] = g;
  for (int c = 1; c < dlc; ++c) o[c] = 0.f;
  return g;
}
__device__ __forceinline__ float store_grad_row(bf16_t* o, float g, int dlc) {
  const bf16_t b = f32_to_bf16(g);
  if (dlc == 8) *reinterpret_cast<u32x4*>(o) = u32x4{(uint32_t)b, 0u, 0u, 0u};
  else {
    o[0] = b;
    for (int c = 1; c < dlc; ++c) o[c] = 0;
  }
  return bf16_to_f32(b);
}

// The class convolution's bias gradient = sum of dL/dlogit over all pixels: the gradient kernels leave one partial sum per
// workgroup behind the loss partials (LOSS_GSUM_OFFSET floats into the workspace) and stp_sigmoid_loss_bias_grad adds them up in a
// fixed order - instead of a separate pass over the 8-channel-padded gradient tensor (stp_channel_sum: 46 -> 6 us at 16x512x512).
__device__ __forceinline__ void loss_gsum_block(float acc, float* gsum) {
  float a[1] = {acc};
  loss_block_sums<1, 1, LOSS_WAVES_PAIRWISE>(a, gsum);
}
__global__ __launch_bounds__(256) void loss_bias_grad_kernel(const float* gsum, int blocks, float* dbias, int accumulate) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) a += (double)gsum[b];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) dbias[0] = accumulate ? dbias[0] + (float)sh[0] : (float)sh[0];
}

// pass 2: dL/dlogit, written to channel 0 of a [count][dl_channels] tensor (other channels 0)
template <typename T>
__global__ __launch_bounds__(256) void loss_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                        int64_t count, const float* scalars, float w_bce, float w_dice,
                                                        float inv_count, float grad_scale, T* __restrict__ dl, int dlc,
                                                        float* __restrict__ gsum) {
  const DiceIouGrad k(scalars);
  const float den = k.den, inv_den2 = k.inv_den2, num = k.num;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const float z = Elem<T>::load(logits + i);
    const float y = target[i] ? 1.f : 0.f;
    const float p = 1.f / (1.f + expf(-z));
    const bool inr = (p >= 1e-7f) && (p <= 1.f - 1e-7f);
    // d bce / d z = (p - y) where the probability clip is inactive
    float g = inr ? w_bce * (p - y) * inv_count : 0.f;
    // d dice_loss / d p = -(2 y den - num) / den^2 ;  dp/dz = p (1-p)
    g += w_dice * (-(2.f * y * den - num) * inv_den2) * (p * (1.f - p));
    g *= grad_scale;
    acc += store_grad_row(dl + i * dlc, g, dlc);
  }
  loss_gsum_block(acc, gsum);
}

// sized for the widest partial layout (stp_sigmoid_loss_ex: 16 floats per workgroup)
extern "C" size_t stp_loss_workspace_bytes(void) { return (size_t)(LOSS_GSUM_OFFSET + LOSS_GRAD_MAX_BLOCKS) * sizeof(float); }

extern "C" int stp_sigmoid_loss_bias_grad(const void* workspace, int64_t count, float* dbias, int32_t accumulate, void* stream) {
  if (!workspace || !dbias || count <= 0) return STP_E_BADARG;
  hipLaunchKernelGGL(loss_bias_grad_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace + LOSS_GSUM_OFFSET,
                     loss_grad_blocks(count, LOSS_GRAD_MAX_BLOCKS), dbias, accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_sigmoid_bce_dice(const void* logits, const uint8_t* target, int64_t count, int32_t dtype, float w_bce,
                                    float w_dice, float* scalars, void* dlogits, int32_t dl_channels, float grad_scale,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = loss_check(dtype, logits && target && scalars && workspace && count > 0, workspace_bytes, stp_loss_workspace_bytes());
  if (rc != STP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = loss_value_blocks(count);
  float* partial = (float*)workspace;
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(loss_partial_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)logits, target, count, partial);
  });
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)count, w_bce, w_dice, scalars);
  STP_LAUNCH_CHECK();
  if (dlogits) {
    if (dl_channels < 1) return STP_E_BADARG;
    const int g = loss_grad_blocks(count, LOSS_GRAD_MAX_BLOCKS);
    const float inv_count = (float)(1.0 / (double)count);
    loss_by_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(loss_grad_kernel<T>, dim3(g), dim3(256), 0, s, (const T*)logits, target, count, scalars, w_bce, w_dice, inv_count,
                         grad_scale, (T*)dlogits, dl_channels, partial + LOSS_GSUM_OFFSET);
    });
    STP_LAUNCH_CHECK();
  }
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// The whole musket loss registry for the sigmoid head (reference segmentation.py:15-22): a weighted sum of
//   0 binary_crossentropy  1 dice_loss  2 iou_loss  3 jaccard_loss  4 focal_loss
// iou_loss = 1 - iou_coef (smooth 1, flattened batch); jaccard_loss = jaccard_distance_loss (smooth 100, over the
// class axis = per pixel for one class, mean over pixels); focal_loss = binary focal loss, gamma 2, alpha 0.25,
// Keras epsilon clip, mean over pixels.  Same two-stage fixed-order reduction as above with two more sums:
//   7 jaccard_i   8 focal_i
#define LOSS_NSUM_EX 16
#define JACCARD_SMOOTH 100.f
#define FOCAL_ALPHA 0.25f

__device__ __forceinline__ float focal_term(float p, float y) {
  const float eps = 1e-7f, hi = 1.f - 1e-7f;
  const float pc = fminf(fmaxf(p, eps), hi);
  return y > 0.5f ? -FOCAL_ALPHA * (1.f - pc) * (1.f - pc) * logf(pc) : -(1.f - FOCAL_ALPHA) * pc * pc * logf(1.f - pc);
}

template <typename T>
__global__ __launch_bounds__(256) void loss_ex_partial_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                              int64_t count, float* partial) {
  float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t per = (count + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < count ? i0 + per : count;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float z = Elem<T>::load(logits + i);
    const float y = target[i] ? 1.f : 0.f;
    const float p = 1.f / (1.f + expf(-z));
    bool inr;
    a[0] += keras_bce(p, y, &inr);
    a[1] += p;
    a[2] += y;
    a[3] += p * y;
    const float t = p > 0.5f ? 1.f : 0.f;
    a[4] += t;
    a[5] += t * y;
    a[6] += (t == y) ? 1.f : 0.f;
    const float inter = p * y;
    a[7] += (1.f - (inter + JACCARD_SMOOTH) / (p + y - inter + JACCARD_SMOOTH)) * JACCARD_SMOOTH;
    a[8] += focal_term(p, y);
  }
  loss_block_sums<LOSS_NSUM_EX>(a, partial);
}

// scalars 0..9 as loss_finalize_kernel, 10 jaccard_loss, 11 focal_loss  (iou_loss = 1 - scalars[8])
__global__ __launch_bounds__(256) void loss_ex_finalize_kernel(const float* partial, int blocks, double inv_count, LossWeights lw,
                                                               float* scalars) {
  const double* s = loss_finalize_sums<LOSS_NSUM_EX>(partial, blocks);
  if (threadIdx.x != 0) return;
  loss_ex_scalars(s, loss_common_scalars(s, inv_count, inv_count, scalars), lw, inv_count, inv_count, scalars);
}

template <typename T>
__global__ __launch_bounds__(256) void loss_ex_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                           int64_t count, const float* scalars, LossWeights lw, float inv_count,
                                                           float grad_scale, T* __restrict__ dl, int dlc, float* __restrict__ gsum) {
  const DiceIouGrad k(scalars);
  const float den = k.den, inv_den2 = k.inv_den2, num = k.num, uden = k.uden, unum = k.unum, inv_uden2 = k.inv_uden2;
  float acc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const float z = Elem<T>::load(logits + i);
    const float y = target[i] ? 1.f : 0.f;
    const float p = 1.f / (1.f + expf(-z));
    const bool inr = (p >= 1e-7f) && (p <= 1.f - 1e-7f);
    float g = inr ? lw.w[0] * (p - y) * inv_count : 0.f;
    // gp = d(loss)/dp of the probability-space terms
    float gp = lw.w[1] * (-(2.f * y * den - num) * inv_den2);
    // d iou / dp = (y uden - unum (1 - y)) / uden^2
    gp -= lw.w[2] * (y * uden - unum * (1.f - y)) * inv_uden2;
    {
      const float inter = p * y, jd = p + y - inter + JACCARD_SMOOTH, jn = inter + JACCARD_SMOOTH;
      gp -= lw.w[3] * JACCARD_SMOOTH * (y * jd - jn * (1.f - y)) / (jd * jd) * inv_count;
    }
    if (inr) {
      const float fg = y > 0.5f ? FOCAL_ALPHA * (2.f * (1.f - p) * logf(p) - (1.f - p) * (1.f - p) / p)
                                : -(1.f - FOCAL_ALPHA) * (2.f * p * logf(1.f - p) - p * p / (1.f - p));
      gp += lw.w[4] * fg * inv_count;
    }
    g += gp * (p * (1.f - p));
    g *= grad_scale;
    acc += store_grad_row(dl + i * dlc, g, dlc);
  }
  loss_gsum_block(acc, gsum);
}

extern "C" int stp_sigmoid_loss_ex(const void* logits, const uint8_t* target, int64_t count, int32_t dtype, const float* weights5,
                                   float* scalars, void* dlogits, int32_t dl_channels, float grad_scale, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  const int rc = loss_check(dtype, logits && target && scalars && workspace && weights5 && count > 0, workspace_bytes, stp_loss_workspace_bytes());
  if (rc != STP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const LossWeights lw = loss_weights(weights5);
  const int blocks = loss_value_blocks(count);
  float* partial = (float*)workspace;
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(loss_ex_partial_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)logits, target, count, partial);
  });
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_ex_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)count, lw, scalars);
  STP_LAUNCH_CHECK();
  if (dlogits) {
    if (dl_channels < 1) return STP_E_BADARG;
    const int g = loss_grad_blocks(count, LOSS_GRAD_MAX_BLOCKS);
    const float inv_count = (float)(1.0 / (double)count);
    loss_by_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(loss_ex_grad_kernel<T>, dim3(g), dim3(256), 0, s, (const T*)logits, target, count, scalars, lw, inv_count, grad_scale,
                         (T*)dlogits, dl_channels, partial + LOSS_GSUM_OFFSET);
    });
    STP_LAUNCH_CHECK();
  }
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// stp_sigmoid_bce_dice with a pixel-weight operand (the border weight map of border_weight.hip; include/stp_hip.h has the arithmetic):
// the cross-entropy term is sum w_i bce_i / count, everything else - dice_loss, the logged overlaps, the accuracy and scalars[1], the
// UNWEIGHTED cross-entropy - is the sibling's.  16-wide partial rows with two more sums:
//   7 w_i * bce_i   8 w_i
// The gradient pass leaves no bias-gradient sums: stp_sigmoid_loss_bias_grad does not follow this entry.
template <typename T>
__global__ __launch_bounds__(256) void loss_weighted_partial_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                                    const float* __restrict__ pw, int64_t count, float* partial) {
  float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto one = [&a](float z, bool tgt, float wt) __attribute__((always_inline)) {
    const float y = tgt ? 1.f : 0.f;
    const float p = 1.f / (1.f + __expf(-z));
    const float bce = keras_bce_fast(p, y);
    a[0] += bce;
    a[1] += p;
    a[2] += y;
    a[3] += p * y;
    const float t = p > 0.5f ? 1.f : 0.f;
    a[4] += t;
    a[5] += t * y;
    a[6] += (t == y) ? 1.f : 0.f;
    a[7] += wt * bce;
    a[8] += wt;
  };
  // four pixels per thread and iteration (8 or 16 bytes of logits, 4 of target, 16 of weights) where the operands allow it
  if ((count & 3) == 0 && ((uintptr_t)logits & (4 * sizeof(T) - 1)) == 0 && ((uintptr_t)target & 3) == 0 && ((uintptr_t)pw & 15) == 0) {
    const int64_t groups = count >> 2, per = (groups + gridDim.x - 1) / gridDim.x;
    const int64_t g0 = (int64_t)blockIdx.x * per, g1 = g0 + per < groups ? g0 + per : groups;
    for (int64_t g = g0 + threadIdx.x; g < g1; g += 256) {
      const f32x4 z = load4(logits + g * 4), wt = load4(pw + g * 4);
      const uint32_t tt = *reinterpret_cast<const uint32_t*>(target + g * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) one(z[e], ((tt >> (8 * e)) & 0xffu) != 0, wt[e]);
    }
  } else {
    const int64_t per = (count + gridDim.x - 1) / gridDim.x;
    const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < count ? i0 + per : count;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) one(Elem<T>::load(logits + i), target[i] != 0, pw[i]);
  }
  loss_block_sums<LOSS_NSUM_EX>(a, partial);
}

// scalars 0..9 as loss_finalize_kernel with [0] on the weighted cross-entropy, 13 weighted_binary_crossentropy, 15 the mean weight
__global__ __launch_bounds__(256) void loss_weighted_finalize_kernel(const float* partial, int blocks, double inv_count, float w_bce,
                                                                     float w_dice, float* scalars) {
  const double* s = loss_finalize_sums<LOSS_NSUM_EX>(partial, blocks);
  if (threadIdx.x != 0) return;
  const LossTerms t = loss_common_scalars(s, inv_count, inv_count, scalars);
  const double wbce = s[7] * inv_count;
  scalars[0] = (float)(w_bce * wbce + w_dice * t.dice_l);
  scalars[13] = (float)wbce;
  scalars[15] = (float)(s[8] * inv_count);
}

template <typename T>
__global__ __launch_bounds__(256) void loss_weighted_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                                 const float* __restrict__ pw, int64_t count, const float* scalars,
                                                                 float w_bce, float w_dice, float inv_count, float grad_scale,
                                                                 T* __restrict__ dl, int dlc) {
  const DiceIouGrad k(scalars);
  const float den = k.den, inv_den2 = k.inv_den2, num = k.num;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const float z = Elem<T>::load(logits + i);
    const float y = target[i] ? 1.f : 0.f;
    const float p = 1.f / (1.f + expf(-z));
    const bool inr = (p >= 1e-7f) && (p <= 1.f - 1e-7f);
    // d (w bce) / d z = w (p - y) where the probability clip is inactive
    float g = inr ? w_bce * pw[i] * (p - y) * inv_count : 0.f;
    g += w_dice * (-(2.f * y * den - num) * inv_den2) * (p * (1.f - p));
    g *= grad_scale;
    store_grad_row(dl + i * dlc, g, dlc);
  }
}

extern "C" int stp_sigmoid_bce_dice_weighted(const void* logits, const uint8_t* target, int64_t count, int32_t dtype, float w_bce,
                                             float w_dice, float* scalars, void* dlogits, int32_t dl_channels, float grad_scale,
                                             void* workspace, size_t workspace_bytes, const float* pixel_weights, void* stream) {
  const int rc = loss_check(dtype, logits && target && scalars && workspace && pixel_weights && count > 0, workspace_bytes,
                            stp_loss_workspace_bytes());
  if (rc != STP_OK) return rc;
  if (dlogits && dl_channels < 1) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = loss_value_blocks(count);
  float* partial = (float*)workspace;
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(loss_weighted_partial_kernel<T>, dim3(blocks), dim3(256), 0, s, (const T*)logits, target, pixel_weights, count, partial);
  });
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_weighted_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)count, w_bce, w_dice, scalars);
  STP_LAUNCH_CHECK();
  if (dlogits) {
    const int g = loss_grad_blocks(count, LOSS_GRAD_MAX_BLOCKS);
    const float inv_count = (float)(1.0 / (double)count);
    loss_by_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      hipLaunchKernelGGL(loss_weighted_grad_kernel<T>, dim3(g), dim3(256), 0, s, (const T*)logits, target, pixel_weights, count, scalars, w_bce,
                         w_dice, inv_count, grad_scale, (T*)dlogits, dl_channels);
    });
    STP_LAUNCH_CHECK();
  }
  return STP_OK;
}


template <typename T>
__global__ void sigmoid_kernel(const T* __restrict__ logits, float* __restrict__ probs, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    probs[i] = 1.f / (1.f + expf(-Elem<T>::load(logits + i)));
}

extern "C" int stp_sigmoid(const void* logits, float* probs, int64_t count, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype) || !logits || !probs || count <= 0) return STP_E_BADARG;
  const int g = loss_grad_blocks(count, 4096);
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL(sigmoid_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)logits, probs, count);
  });
  STP_LAUNCH_CHECK();
  return STP_OK;
}
