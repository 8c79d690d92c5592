// Segmentation loss (sigmoid + Keras BCE + musket dice), Keras optimizers over a flat fp32
// arena, weight-layout preparation and wire-format casts.  HBM-bound streaming kernels with
// two-stage fixed-order reductions.
#include "common.h"
#include <cstdlib>

#define LOSS_MAX_BLOCKS 1024
#define LOSS_NSUM 8

// ------------------------------------------------------------------------------------------
// pass 1: per-block partial sums of
//   0 bce_i   1 p   2 y   3 p*y   4 [p>.5]   5 [p>.5]*y   6 [(p>.5)==y]   7 unused
__device__ __forceinline__ float sigmoidf_(float z) { return 1.f / (1.f + __expf(-z)); }

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
  __shared__ double sh[32][LOSS_NSUM];
  const int e = threadIdx.x & 7, lane = threadIdx.x >> 3;
  double a = 0.0;
  {
    int b = lane;
    for (; b + 224 < blocks; b += 256) {      // eight partials in flight; same order of additions
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(b + 32 * u) * LOSS_NSUM + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += (double)v[u];
    }
    for (; b < blocks; b += 32) a += (double)partial[(size_t)b * LOSS_NSUM + e];
  }
  sh[lane][e] = a;
  __syncthreads();
  for (int w = 16; w > 0; w >>= 1) {
    if (lane < w) sh[lane][e] += sh[lane + w][e];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double* s = sh[0];
  const double bce = s[0] * inv_count;
  const double dice_l = 1.0 - (2.0 * s[3] + 1.0) / (s[2] + s[1] + 1.0);
  const double dice_m = (2.0 * s[5] + 1.0) / (s[2] + s[4] + 1.0);
  scalars[0] = (float)(w_bce * bce + w_dice * dice_l);
  scalars[1] = (float)bce;
  scalars[2] = (float)dice_l;
  scalars[3] = (float)dice_m;
  scalars[4] = (float)(s[6] * inv_count);
  scalars[5] = (float)s[1];
  scalars[6] = (float)s[2];
  scalars[7] = (float)s[3];
  scalars[8] = (float)((s[3] + 1.0) / (s[2] + s[1] - s[3] + 1.0));   // iou: musket iou_coef, smooth 1
  scalars[9] = (float)((s[5] + 1.0) / (s[2] + s[4] - s[5] + 1.0));   // iot: the same on predictions thresholded at 0.5
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
#define LOSS_GSUM_OFFSET (LOSS_MAX_BLOCKS * 16)
#define LOSS_GRAD_MAX_BLOCKS 4096
__device__ __forceinline__ void loss_gsum_block(float acc, float* gsum) {
  __shared__ float wred[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) gsum[blockIdx.x] = (wred[0] + wred[1]) + (wred[2] + wred[3]);
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
static int loss_grad_blocks(int64_t count) {
  int64_t g = (count + 255) / 256;
  return (int)(g > LOSS_GRAD_MAX_BLOCKS ? LOSS_GRAD_MAX_BLOCKS : g);
}

// pass 2: dL/dlogit, written to channel 0 of a [count][dl_channels] tensor (other channels 0)
template <typename T>
__global__ __launch_bounds__(256) void loss_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                        int64_t count, const float* scalars, float w_bce, float w_dice,
                                                        float inv_count, float grad_scale, T* __restrict__ dl, int dlc,
                                                        float* __restrict__ gsum) {
  const float sp = scalars[5], sy = scalars[6], spy = scalars[7];
  const float den = sy + sp + 1.f;
  const float inv_den2 = 1.f / (den * den);
  const float num = 2.f * spy + 1.f;
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
                     loss_grad_blocks(count), dbias, accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_sigmoid_bce_dice(const void* logits, const uint8_t* target, int64_t count, int32_t dtype, float w_bce,
                                    float w_dice, float* scalars, void* dlogits, int32_t dl_channels, float grad_scale,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!logits || !target || !scalars || !workspace || count <= 0) return STP_E_BADARG;
  if (workspace_bytes < stp_loss_workspace_bytes()) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int64_t b = count / 1024;
  if (b < 1) b = 1;
  if (b > LOSS_MAX_BLOCKS) b = LOSS_MAX_BLOCKS;
  const int blocks = (int)b;
  float* partial = (float*)workspace;
  if (dtype == STP_H16)
    hipLaunchKernelGGL(loss_partial_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, (const bf16_t*)logits, target, count, partial);
  else if (dtype == STP_F32)
    hipLaunchKernelGGL(loss_partial_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)logits, target, count, partial);
  else
    return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)count, w_bce, w_dice, scalars);
  STP_LAUNCH_CHECK();
  if (dlogits) {
    if (dl_channels < 1) return STP_E_BADARG;
    const int g = loss_grad_blocks(count);
    float* gsum = partial + LOSS_GSUM_OFFSET;
    const float inv_count = (float)(1.0 / (double)count);
    if (dtype == STP_H16)
      hipLaunchKernelGGL(loss_grad_kernel<bf16_t>, dim3(g), dim3(256), 0, s, (const bf16_t*)logits, target, count, scalars,
                         w_bce, w_dice, inv_count, grad_scale, (bf16_t*)dlogits, dl_channels, gsum);
    else
      hipLaunchKernelGGL(loss_grad_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)logits, target, count, scalars,
                         w_bce, w_dice, inv_count, grad_scale, (float*)dlogits, dl_channels, gsum);
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

struct LossWeights { float w[5]; };

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
  __shared__ float red[4][9];
#pragma unroll
  for (int e = 0; e < 9; ++e) a[e] = wave_sum(a[e]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int e = 0; e < 9; ++e) red[threadIdx.x >> 6][e] = a[e];
  __syncthreads();
  if (threadIdx.x < LOSS_NSUM_EX)
    partial[(size_t)blockIdx.x * LOSS_NSUM_EX + threadIdx.x] =
        threadIdx.x < 9 ? red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] : 0.f;
}

// scalars 0..9 as loss_finalize_kernel, 10 jaccard_loss, 11 focal_loss  (iou_loss = 1 - scalars[8])
__global__ __launch_bounds__(256) void loss_ex_finalize_kernel(const float* partial, int blocks, double inv_count, LossWeights lw,
                                                               float* scalars) {
  __shared__ double sh[16][LOSS_NSUM_EX];
  const int e = threadIdx.x & 15, lane = threadIdx.x >> 4;
  double a = 0.0;
  for (int b = lane; b < blocks; b += 16) a += (double)partial[(size_t)b * LOSS_NSUM_EX + e];
  sh[lane][e] = a;
  __syncthreads();
  for (int w = 8; w > 0; w >>= 1) {
    if (lane < w) sh[lane][e] += sh[lane + w][e];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double* s = sh[0];
  const double bce = s[0] * inv_count;
  const double dice_l = 1.0 - (2.0 * s[3] + 1.0) / (s[2] + s[1] + 1.0);
  const double dice_m = (2.0 * s[5] + 1.0) / (s[2] + s[4] + 1.0);
  const double iou = (s[3] + 1.0) / (s[2] + s[1] - s[3] + 1.0);
  const double jac = s[7] * inv_count, focal = s[8] * inv_count;
  scalars[0] = (float)(lw.w[0] * bce + lw.w[1] * dice_l + lw.w[2] * (1.0 - iou) + lw.w[3] * jac + lw.w[4] * focal);
  scalars[1] = (float)bce;
  scalars[2] = (float)dice_l;
  scalars[3] = (float)dice_m;
  scalars[4] = (float)(s[6] * inv_count);
  scalars[5] = (float)s[1];
  scalars[6] = (float)s[2];
  scalars[7] = (float)s[3];
  scalars[8] = (float)iou;
  scalars[9] = (float)((s[5] + 1.0) / (s[2] + s[4] - s[5] + 1.0));
  scalars[10] = (float)jac;
  scalars[11] = (float)focal;
}

template <typename T>
__global__ __launch_bounds__(256) void loss_ex_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                           int64_t count, const float* scalars, LossWeights lw, float inv_count,
                                                           float grad_scale, T* __restrict__ dl, int dlc, float* __restrict__ gsum) {
  const float sp = scalars[5], sy = scalars[6], spy = scalars[7];
  const float den = sy + sp + 1.f;
  const float inv_den2 = 1.f / (den * den);
  const float num = 2.f * spy + 1.f;
  const float uden = sy + sp - spy + 1.f, unum = spy + 1.f;     // iou_coef = unum / uden
  const float inv_uden2 = 1.f / (uden * uden);
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
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!logits || !target || !scalars || !workspace || !weights5 || count <= 0) return STP_E_BADARG;
  if (workspace_bytes < stp_loss_workspace_bytes()) return STP_E_WORKSPACE;
  if (dtype != STP_H16 && dtype != STP_F32) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  LossWeights lw;
  for (int i = 0; i < 5; ++i) lw.w[i] = weights5[i];
  int64_t b = count / 1024;
  if (b < 1) b = 1;
  if (b > LOSS_MAX_BLOCKS) b = LOSS_MAX_BLOCKS;
  const int blocks = (int)b;
  float* partial = (float*)workspace;
  if (dtype == STP_H16)
    hipLaunchKernelGGL(loss_ex_partial_kernel<bf16_t>, dim3(blocks), dim3(256), 0, s, (const bf16_t*)logits, target, count, partial);
  else
    hipLaunchKernelGGL(loss_ex_partial_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)logits, target, count, partial);
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_ex_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)count, lw, scalars);
  STP_LAUNCH_CHECK();
  if (dlogits) {
    if (dl_channels < 1) return STP_E_BADARG;
    const int g = loss_grad_blocks(count);
    float* gsum = partial + LOSS_GSUM_OFFSET;
    const float inv_count = (float)(1.0 / (double)count);
    if (dtype == STP_H16)
      hipLaunchKernelGGL(loss_ex_grad_kernel<bf16_t>, dim3(g), dim3(256), 0, s, (const bf16_t*)logits, target, count, scalars, lw,
                         inv_count, grad_scale, (bf16_t*)dlogits, dl_channels, gsum);
    else
      hipLaunchKernelGGL(loss_ex_grad_kernel<float>, dim3(g), dim3(256), 0, s, (const float*)logits, target, count, scalars, lw,
                         inv_count, grad_scale, (float*)dlogits, dl_channels, gsum);
    STP_LAUNCH_CHECK();
  }
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// Multi-class head: channel softmax + Keras categorical_crossentropy (+ w * musket dice over all class maps).
// One thread per pixel; logits [pixels][ldc] (first `classes` channels), target = class index per pixel.
// The seven sums have the binary kernel's meaning, taken over every (pixel, class) element of the one-hot target;
// sum 0 is the per-pixel cross-entropy.
#include "softmax_row.h"

template <typename T, int CM>
__global__ __launch_bounds__(256) void softmax_loss_partial_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                                   int64_t pixels, int classes, int ldc, float* partial) {
  float a[LOSS_NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t per = (pixels + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < pixels ? i0 + per : pixels;
  const bool vec = (ldc % Elem<T>::VEC) == 0 && CM % Elem<T>::VEC == 0;
  const bool vec4 = !vec && sizeof(T) == 2 && (ldc % 4) == 0 && (CM % 4) == 0 && !(reinterpret_cast<uintptr_t>(logits) & 7);
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
    float p[CM];
    softmax_row<T, CM>(logits + i * ldc, classes, vec, p, vec4);
    const int t = target[i] < classes ? target[i] : classes - 1;
    // the per-class sums of the one-hot target in closed form (the loop over the classes cost ~12 instructions per class and pixel - the
    // kernel is VALU-bound: 137 us per pass for PSPNet's 20 classes against a 38 us memory floor): sum_c y_c = 1, sum_c p_c y_c = p_t, at
    // most ONE class passes the 0.5 threshold (the probabilities sum to 1), so sum_c th_c = [pmax > 0.5], sum_c th_c y_c = [p_t > 0.5] and
    // the count of th_c == y_c is classes - (p_t > 0.5 ? 0 : 1 + [pmax > 0.5]).  The counts are the same integers; sum_c p_c is added per pixel.
    float pt = 0.f, pmax = 0.f, psum = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      pt = c == t ? p[c] : pt;
      pmax = fmaxf(pmax, p[c]);                      // (p[c] = 0 beyond `classes`)
      psum += p[c];
    }
    const float tt = pt > 0.5f ? 1.f : 0.f, tm = pmax > 0.5f ? 1.f : 0.f;
    a[1] += psum;
    a[2] += 1.f;
    a[3] += pt;
    a[4] += tm;
    a[5] += tt;
    a[6] += (float)classes - (pt > 0.5f ? 0.f : 1.f + tm);
    // Keras: p <- p / sum(p) (a no-op on a softmax up to rounding), clip to [eps, 1-eps], -sum(y log p)
    a[0] += -__logf(fminf(fmaxf(pt, 1e-7f), 1.f - 1e-7f));
  }
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

// scalars as in the binary case, with scalars[1] = categorical_crossentropy and scalars[4] the element-wise accuracy
__global__ __launch_bounds__(256) void softmax_loss_finalize_kernel(const float* partial, int blocks, double inv_pixels,
                                                                    double inv_elems, float w_cce, float w_dice, float* scalars) {
  __shared__ double sh[32][LOSS_NSUM];
  const int e = threadIdx.x & 7, lane = threadIdx.x >> 3;
  double a = 0.0;
  {
    int b = lane;
    for (; b + 224 < blocks; b += 256) {      // eight partials in flight (a run-time trip count keeps one); same order of additions
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(size_t)(b + 32 * u) * LOSS_NSUM + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) a += (double)v[u];
    }
    for (; b < blocks; b += 32) a += (double)partial[(size_t)b * LOSS_NSUM + e];
  }
  sh[lane][e] = a;
  __syncthreads();
  for (int w = 16; w > 0; w >>= 1) {
    if (lane < w) sh[lane][e] += sh[lane + w][e];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double* s = sh[0];
  const double cce = s[0] * inv_pixels;
  const double dice_l = 1.0 - (2.0 * s[3] + 1.0) / (s[2] + s[1] + 1.0);
  scalars[0] = (float)(w_cce * cce + w_dice * dice_l);
  scalars[1] = (float)cce;
  scalars[2] = (float)dice_l;
  scalars[3] = (float)((2.0 * s[5] + 1.0) / (s[2] + s[4] + 1.0));
  scalars[4] = (float)(s[6] * inv_elems);
  scalars[5] = (float)s[1];
  scalars[6] = (float)s[2];
  scalars[7] = (float)s[3];
  scalars[8] = (float)((s[3] + 1.0) / (s[2] + s[1] - s[3] + 1.0));
  scalars[9] = (float)((s[5] + 1.0) / (s[2] + s[4] - s[5] + 1.0));
}

template <typename T, int CM>
__global__ __launch_bounds__(256) void softmax_loss_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target,
                                                                int64_t pixels, int classes, int ldc, const float* scalars,
                                                                float w_cce, float w_dice, float inv_pixels, float grad_scale,
                                                                T* __restrict__ dl, int dlc) {
  constexpr int V = Elem<T>::VEC;
  const float sp = scalars[5], sy = scalars[6], spy = scalars[7];
  const float den = sy + sp + 1.f;
  const float inv_den2 = 1.f / (den * den);
  const float num = 2.f * spy + 1.f;
  const bool vec = (ldc % V) == 0 && CM % V == 0, vout = (dlc % V) == 0;
  const bool vec4 = !vec && sizeof(T) == 2 && (ldc % 4) == 0 && (CM % 4) == 0 && !(reinterpret_cast<uintptr_t>(logits) & 7);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    float p[CM];
    softmax_row<T, CM>(logits + i * ldc, classes, vec, p, vec4);
    const int t = target[i] < classes ? target[i] : classes - 1;
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
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const float y = c == t ? 1.f : 0.f;
      float v = inr ? w_cce * (p[c] - y) * inv_pixels : 0.f;
      v += w_dice * p[c] * ((-(2.f * y * den - num) * inv_den2) - gp);
      g[c] = c < classes ? v * grad_scale : 0.f;
    }
    T* o = dl + i * dlc;
    if (vout) {
#pragma unroll
      for (int v = 0; v < 32 / V; ++v) {
        if (v * V >= dlc) break;
        u32x4 r = {0u, 0u, 0u, 0u};
        auto gv = [&](int idx) { return idx < CM ? g[idx % CM] : 0.f; };      // channels past the class bucket are padding
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = pack_bf16x2(gv(v * V + 2 * e), gv(v * V + 2 * e + 1));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) r[e] = __float_as_uint(gv(v * V + e));
        }
        *reinterpret_cast<u32x4*>(o + v * V) = r;
      }
    } else {
#pragma unroll
      for (int c = 0; c < CM; ++c) if (c < classes) Elem<T>::store(o + c, g[c]);
      for (int c = classes; c < dlc; ++c) Elem<T>::store(o + c, 0.f);
    }
  }
}

template <typename T, int CM>
static void launch_softmax_loss(const T* logits, const uint8_t* target, int64_t pixels, int classes, int ldc, float w_cce, float w_dice,
                                float* scalars, T* dl, int dlc, float grad_scale, float* partial, int blocks, hipStream_t s) {
  hipLaunchKernelGGL((softmax_loss_partial_kernel<T, CM>), dim3(blocks), dim3(256), 0, s, logits, target, pixels, classes, ldc, partial);
  hipLaunchKernelGGL(softmax_loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)pixels,
                     1.0 / ((double)pixels * classes), w_cce, w_dice, scalars);
  if (dl) {
    int64_t g = (pixels + 255) / 256;
    if (g > 16384) g = 16384;
    hipLaunchKernelGGL((softmax_loss_grad_kernel<T, CM>), dim3((int)g), dim3(256), 0, s, logits, target, pixels, classes, ldc, scalars, w_cce,
                       w_dice, (float)(1.0 / (double)pixels), grad_scale, dl, dlc);
  }
}

template <typename T>
static void dispatch_softmax_loss(const T* logits, const uint8_t* target, int64_t pixels, int classes, int ldc, float w_cce, float w_dice,
                                  float* scalars, T* dl, int dlc, float grad_scale, float* partial, int blocks, hipStream_t s) {
#define STP_SM(CM) launch_softmax_loss<T, CM>(logits, target, pixels, classes, ldc, w_cce, w_dice, scalars, dl, dlc, grad_scale, partial, blocks, s)
  if (classes <= 4) STP_SM(4);
  else if (classes <= 8) STP_SM(8);
  else if (classes <= 16) STP_SM(16);
  else if (classes <= 24) STP_SM(24);
  else STP_SM(32);
#undef STP_SM
}

extern "C" int stp_softmax_cce_dice(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc,
                                    int32_t dtype, float w_cce, float w_dice, float* scalars, void* dlogits, int32_t dl_channels,
                                    float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!logits || !target || !scalars || !workspace || pixels <= 0 || classes < 2 || classes > STP_MAX_CLASSES || ldc < classes)
    return STP_E_BADARG;
  if (workspace_bytes < stp_loss_workspace_bytes()) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int64_t b = pixels / 1024;
  if (b < 1) b = 1;
  if (b > LOSS_MAX_BLOCKS) b = LOSS_MAX_BLOCKS;
  const int blocks = (int)b;
  float* partial = (float*)workspace;
  if (dlogits && dl_channels < classes) return STP_E_BADARG;
  if (dtype == STP_H16)
    dispatch_softmax_loss<bf16_t>((const bf16_t*)logits, target, pixels, classes, ldc, w_cce, w_dice, scalars, (bf16_t*)dlogits, dl_channels,
                                  grad_scale, partial, blocks, s);
  else if (dtype == STP_F32)
    dispatch_softmax_loss<float>((const float*)logits, target, pixels, classes, ldc, w_cce, w_dice, scalars, (float*)dlogits, dl_channels,
                                 grad_scale, partial, blocks, s);
  else
    return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// Round 6: the same loss on class logits that the network produces at 1 / f of the mask's resolution and resizes bilinearly (PSPNet's
// `final_interpolation`, FPN's last upsampling) - WITHOUT the resized tensor.  The unfused chain writes the f^2-times larger logits,
// reads them twice (value pass, gradient pass), writes their gradient and reads it back in the resize gradient: 1.0 GB and four launches
// for PSPNet's 20 classes at 8 x 768 x 768 (468 us); here both passes interpolate from the low-resolution logits (cache-resident) and the
// gradient pass reduces dL/dlogits straight into the low-resolution gradient.
//   * one thread per (low-resolution cell (n, y0, x0), row jy of the cell): the f output pixels (y0 f + jy, x0 f .. x0 f + f - 1) read the
//     cell's four corners (y0, x0), (y0, x1), (y1, x0), (y1, x1), x1 = min(x0 + 1, W - 1) - the lerp of resize_bilinear_vec_kernel, same
//     order, and the SAME rounding points as the unfused chain: the interpolated logit is rounded to the storage type before the softmax,
//     the per-pixel gradient is rounded to the storage type before it is weighted;
//   * gradient: a thread sums (1 - fx) g and fx g over its f pixels, the f rows of a cell are combined by a DPP butterfly over the cell's f
//     adjacent lanes (fixed order), the cell's four corner sums go to a [cells][4][CM] fp32 table, and a combine launch adds the (up to
//     nine, border clamping included) cell corners that land on a low-resolution pixel in a fixed order - deterministic, no atomics.
// rounds a pair of values to the storage type (one v_cvt_pk per pair)
template <typename T> __device__ __forceinline__ void round_pair_to_storage(float& a, float& b) {
  if constexpr (sizeof(T) == 2) {
    const uint32_t w = pack_bf16x2(a, b);
    a = h16lo_to_f32(w);
    b = h16hi_to_f32(w);
  }
}
// sum over the f = 2^lf adjacent lanes of a cell (every lane of the group gets the sum; groups are lane-aligned)
__device__ __forceinline__ float cell_lanes_sum(float v, int lf) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));             // quad_perm [1,0,3,2]
  if (lf >= 2) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));  // quad_perm [2,3,0,1]
  if (lf >= 3) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true)); // row_half_mirror
  if (lf >= 4) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xf, 0xf, true)); // row_mirror
  return v;
}

struct UpGeo { int H, W, lf; FastDiv divW, divH; };

// Row jy of cell (n, y0, x0): the logits of its f output pixels are L + D fx, fx = jx / f, with L / R the left / right corner columns
// interpolated to the row FIRST (L = v00 + (v10 - v00) fy, R = v01 + (v11 - v01) fy, D = R - L): one multiply-add per class and pixel
// instead of the three of the horizontal-first order of resize_bilinear_vec_kernel (the same number up to the rounding of fp32 sums,
// i.e. the storage rounding that follows lands on the other neighbour for ~1 value in 10^4).  Also the f target bytes of the row.
template <typename T, int CM>
__device__ __forceinline__ void up_row_load(const T* __restrict__ low, const uint8_t* __restrict__ target, uint32_t item, const UpGeo& g, int classes,
                                            int ldc, bool vec, bool vec4, float (&L)[CM], float (&D)[CM], uint32_t& tw0, uint32_t& tw1,
                                            uint32_t& tw2, uint32_t& tw3, float& fy, int& jy, uint32_t& cell) {
  const int f = 1 << g.lf;
  jy = (int)(item & (uint32_t)(f - 1));
  cell = item >> g.lf;
  const uint32_t r = fdiv(cell, g.divW);
  const int x0 = (int)(cell - r * (uint32_t)g.W);
  const uint32_t n = fdiv(r, g.divH);
  const int y0 = (int)(r - n * (uint32_t)g.H);
  const int x1 = min(x0 + 1, g.W - 1), y1 = min(y0 + 1, g.H - 1);
  fy = (float)jy * (1.f / (float)f);
  const T* b = low + (int64_t)n * g.H * g.W * ldc;
  float tmp[CM];
  class_row_load<T, CM>(b + ((int64_t)y0 * g.W + x0) * ldc, classes, vec, L, vec4);
  class_row_load<T, CM>(b + ((int64_t)y1 * g.W + x0) * ldc, classes, vec, tmp, vec4);
#pragma unroll
  for (int c = 0; c < CM; ++c) L[c] = L[c] + (tmp[c] - L[c]) * fy;
  class_row_load<T, CM>(b + ((int64_t)y0 * g.W + x1) * ldc, classes, vec, D, vec4);
  class_row_load<T, CM>(b + ((int64_t)y1 * g.W + x1) * ldc, classes, vec, tmp, vec4);
#pragma unroll
  for (int c = 0; c < CM; ++c) D[c] = (D[c] + (tmp[c] - D[c]) * fy) - L[c];
  const uint8_t* trow = target + (((int64_t)n * g.H + y0) * f + jy) * ((int64_t)g.W * f) + (int64_t)x0 * f;
  tw0 = tw1 = tw2 = tw3 = 0u;
  if (f >= 4) {
    const uint32_t* tq = reinterpret_cast<const uint32_t*>(trow);
    tw0 = tq[0];
    if (f >= 8) tw1 = tq[1];
    if (f >= 16) { tw2 = tq[2]; tw3 = tq[3]; }
  } else {
    tw0 = *reinterpret_cast<const uint16_t*>(trow);
  }
}
// output pixel jx of the row: e[c] = exp(logit_c - max) of the logits rounded to the storage type (0 beyond `classes`), their sum; returns the target class
template <typename T, int CM>
__device__ __forceinline__ int up_pixel_exp(const float (&L)[CM], const float (&D)[CM], uint32_t tw0, uint32_t tw1, uint32_t tw2, uint32_t tw3, int jx,
                                            float inv_f, int classes, float (&e)[CM], float& esum) {
  const float fx = (float)jx * inv_f;
#pragma unroll
  for (int c = 0; c < CM; c += 2) {
    e[c] = L[c] + D[c] * fx;
    e[c + 1] = L[c + 1] + D[c + 1] * fx;
    round_pair_to_storage<T>(e[c], e[c + 1]);
  }
  float m = -3.4e38f;
#pragma unroll
  for (int c = 0; c < CM; ++c) if (c < classes) m = fmaxf(m, e[c]);
  esum = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c) { e[c] = c < classes ? __expf(e[c] - m) : 0.f; esum += e[c]; }
  const uint32_t w = jx < 4 ? tw0 : jx < 8 ? tw1 : jx < 12 ? tw2 : tw3;
  const int t = (int)((w >> ((jx & 3) * 8)) & 255u);
  return t < classes ? t : classes - 1;
}

template <typename T, int CM>
__global__ __launch_bounds__(256) void softmax_up_partial_kernel(const T* __restrict__ low, const uint8_t* __restrict__ target, uint32_t items,
                                                                 const UpGeo g, int classes, int ldc, float* partial) {
  float a[LOSS_NSUM] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int f = 1 << g.lf;
  const float inv_f = 1.f / (float)f;
  const bool vec = (ldc % Elem<T>::VEC) == 0 && CM % Elem<T>::VEC == 0;
  const bool vec4 = !vec && sizeof(T) == 2 && (ldc % 4) == 0 && (CM % 4) == 0 && !(reinterpret_cast<uintptr_t>(low) & 7);
  for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
    float L[CM], D[CM], fy;
    uint32_t tw0, tw1, tw2, tw3, cell;
    int jy;
    up_row_load<T, CM>(low, target, it, g, classes, ldc, vec, vec4, L, D, tw0, tw1, tw2, tw3, fy, jy, cell);
    for (int jx = 0; jx < f; ++jx) {
      float e[CM], esum;
      const int t = up_pixel_exp<T, CM>(L, D, tw0, tw1, tw2, tw3, jx, inv_f, classes, e, esum);
      float et = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) et = c == t ? e[c] : et;
      // the closed forms of softmax_loss_partial_kernel with p_c = e_c / sum: the largest e is exp(0) = 1, so pmax = 1 / sum
      const float inv = 1.f / esum, pt = et * inv, pmax = inv;
      const float tt = pt > 0.5f ? 1.f : 0.f, tm = pmax > 0.5f ? 1.f : 0.f;
      a[1] += esum * inv;
      a[2] += 1.f;
      a[3] += pt;
      a[4] += tm;
      a[5] += tt;
      a[6] += (float)classes - (pt > 0.5f ? 0.f : 1.f + tm);
      a[0] += -__logf(fminf(fmaxf(pt, 1e-7f), 1.f - 1e-7f));
    }
  }
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

template <typename T, int CM>
__global__ __launch_bounds__(256) void softmax_up_grad_kernel(const T* __restrict__ low, const uint8_t* __restrict__ target, uint32_t items,
                                                              const UpGeo g, int classes, int ldc, const float* __restrict__ scalars, float w_cce,
                                                              float w_dice, float inv_pixels, float grad_scale, float* __restrict__ corners) {
  const float sp = scalars[5], sy = scalars[6], spy = scalars[7];
  const float den = sy + sp + 1.f;
  const float inv_den2 = 1.f / (den * den);
  const float num = 2.f * spy + 1.f;
  const int f = 1 << g.lf;
  const float inv_f = 1.f / (float)f;
  const bool vec = (ldc % Elem<T>::VEC) == 0 && CM % Elem<T>::VEC == 0;
  const bool vec4 = !vec && sizeof(T) == 2 && (ldc % 4) == 0 && (CM % 4) == 0 && !(reinterpret_cast<uintptr_t>(low) & 7);
  // (items is a multiple of f and a cell's f lanes are lane-aligned: they enter and leave the loop together)
  for (uint32_t it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
    float L[CM], D[CM], fy;
    uint32_t tw0, tw1, tw2, tw3, cell;
    int jy;
    up_row_load<T, CM>(low, target, it, g, classes, ldc, vec, vec4, L, D, tw0, tw1, tw2, tw3, fy, jy, cell);
    float A[CM], B[CM];                           // sum over the row of (1 - fx) g and fx g
#pragma unroll
    for (int c = 0; c < CM; ++c) A[c] = B[c] = 0.f;
    for (int jx = 0; jx < f; ++jx) {
      float e[CM], esum;
      const int t = up_pixel_exp<T, CM>(L, D, tw0, tw1, tw2, tw3, jx, inv_f, classes, e, esum);
      float et = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) et = c == t ? e[c] : et;
      const float inv = 1.f / esum, pt = et * inv, psum = esum * inv;
      const bool inr = pt >= 1e-7f && pt <= 1.f - 1e-7f;      // the clip passes no gradient outside
      // softmax_loss_grad_kernel's dz_c = w_cce (p_c - y_c) / pixels [inr] + w_dice p_c ((num - 2 y_c den) / den^2 - gp), p_c = e_c / sum:
      // every class gets e_c Kq, the target class the two y terms on top
      const float gp = (num * psum - 2.f * den * pt) * inv_den2;
      const float k1 = inr ? w_cce * inv_pixels : 0.f;
      const float kq = (k1 + w_dice * (num * inv_den2 - gp)) * inv * grad_scale;
      const float corr = -(k1 + pt * w_dice * 2.f * den * inv_den2) * grad_scale;
      const float fx = (float)jx * inv_f, gx = 1.f - fx;
#pragma unroll
      for (int c = 0; c < CM; c += 2) {
        float g0 = e[c] * kq + (c == t ? corr : 0.f), g1 = e[c + 1] * kq + (c + 1 == t ? corr : 0.f);
        round_pair_to_storage<T>(g0, g1);
        A[c] += gx * g0; B[c] += fx * g0;
        A[c + 1] += gx * g1; B[c + 1] += fx * g1;
      }
    }
    // the cell's four corner sums over its f rows; corner k = (row a, column b), k = 2 a + b, is stored by lane k (f >= 4) / k & 1 (f = 2)
    float* out = corners + (size_t)cell * (4 * CM);
    const float wy0 = 1.f - fy, wy1 = fy;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float s[CM];
#pragma unroll
      for (int c = 0; c < CM; ++c) s[c] = cell_lanes_sum(((k & 2) ? wy1 : wy0) * ((k & 1) ? B[c] : A[c]), g.lf);
      if (jy == (k & (f - 1))) {
#pragma unroll
        for (int c = 0; c < CM; c += 4) *reinterpret_cast<f32x4*>(out + k * CM + c) = f32x4{s[c], s[c + 1], s[c + 2], s[c + 3]};
      }
    }
  }
}

// low-resolution gradient = the cell corners that land on each pixel: cell (y0, x0) corner (a, b) -> pixel (min(y0 + a, H - 1), min(x0 + b, W - 1))
template <typename T>
__global__ __launch_bounds__(256) void softmax_up_combine_kernel(const float* __restrict__ corners, int64_t total, int H, int W, int CM, int classes,
                                                                 T* __restrict__ dl, int dlc, const float* __restrict__ dev_scale,
                                                                 float* dev_record) {
  const float m = dev_scale ? dev_scale[0] : 1.f;
  if (dev_record && blockIdx.x == 0 && threadIdx.x == 0) dev_record[0] = m;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % dlc);
    const int64_t pix = i / dlc;
    float sum = 0.f;
    if (c < classes) {
      const int w = (int)(pix % W);
      const int64_t r = pix / W;
      const int h = (int)(r % H);
      const int64_t n = r / H;
      const float* base = corners + n * H * W * (int64_t)(4 * CM) + c;
      // rows of cells whose corner row a lands on h: a = 0: h; a = 1: h - 1, and H - 1 itself when h is the last row (clamped)
      int ys[3], as[3], ny = 0;
      ys[ny] = h; as[ny++] = 0;
      if (h >= 1) { ys[ny] = h - 1; as[ny++] = 1; }
      if (h == H - 1) { ys[ny] = h; as[ny++] = 1; }
      int xs[3], bs[3], nx = 0;
      xs[nx] = w; bs[nx++] = 0;
      if (w >= 1) { xs[nx] = w - 1; bs[nx++] = 1; }
      if (w == W - 1) { xs[nx] = w; bs[nx++] = 1; }
      for (int iy = 0; iy < ny; ++iy)
        for (int ix = 0; ix < nx; ++ix)
          sum += base[(((int64_t)ys[iy] * W + xs[ix]) * 4 + as[iy] * 2 + bs[ix]) * CM];
    }
    Elem<T>::store(dl + i, sum * m);
  }
}

template <typename T, int CM>
static void launch_softmax_up(const T* low, const uint8_t* target, int N, int H, int W, int lf, int classes, int ldc, float w_cce, float w_dice,
                              float* scalars, T* dl, int dlc, float grad_scale, const float* dev_scale, float* dev_record, float* partial,
                              float* corners, hipStream_t s) {
  const int64_t cells = (int64_t)N * H * W, items = cells << lf, pixels = items << lf;
  UpGeo g;
  g.H = H; g.W = W; g.lf = lf; g.divW = make_fastdiv((uint32_t)W); g.divH = make_fastdiv((uint32_t)H);
  // value pass: at most 2048 partial rows (they fit the loss workspace), every thread the same number of rows where the count allows
  // (PSPNet's 589 824 rows: 1152 workgroups x 2 rows, not 1024 x 2.25)
  int64_t b = (items + 255) / 256;
  const int64_t iters = (b + 2047) / 2048;
  b = (b + iters - 1) / iters;
  const int blocks = (int)b;
  static_assert(2048 * LOSS_NSUM <= LOSS_GSUM_OFFSET + LOSS_GRAD_MAX_BLOCKS, "partial rows fit stp_loss_workspace_bytes()");
  hipLaunchKernelGGL((softmax_up_partial_kernel<T, CM>), dim3(blocks), dim3(256), 0, s, low, target, (uint32_t)items, g, classes, ldc, partial);
  hipLaunchKernelGGL(softmax_loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, blocks, 1.0 / (double)pixels,
                     1.0 / ((double)pixels * classes), w_cce, w_dice, scalars);
  if (dl) {
    int64_t gr = (items + 255) / 256;
    if (gr > 16384) gr = 16384;
    hipLaunchKernelGGL((softmax_up_grad_kernel<T, CM>), dim3((int)gr), dim3(256), 0, s, low, target, (uint32_t)items, g, classes, ldc, scalars, w_cce,
                       w_dice, (float)(1.0 / (double)pixels), grad_scale, corners);
    const int64_t total = cells * dlc;
    int64_t g2 = (total + 255) / 256;
    if (g2 > 8192) g2 = 8192;
    hipLaunchKernelGGL(softmax_up_combine_kernel<T>, dim3((int)g2), dim3(256), 0, s, corners, total, H, W, CM, classes, dl, dlc, dev_scale, dev_record);
  }
}

static int up_class_bucket(int classes) { return classes <= 4 ? 4 : classes <= 8 ? 8 : classes <= 16 ? 16 : classes <= 24 ? 24 : 32; }

extern "C" int stp_softmax_cce_dice_up_ok(int32_t factor, int32_t classes, int32_t dtype) {
  const bool on = !(getenv("STP_UP_LOSS") && atoi(getenv("STP_UP_LOSS")) == 0);      // (a plan-time query: read at every call)
  return on && stp_dtype_ok(dtype) && (factor == 2 || factor == 4 || factor == 8 || factor == 16) && classes >= 2 && classes <= STP_MAX_CLASSES;
}
extern "C" size_t stp_softmax_cce_dice_up_corner_bytes(int32_t N, int32_t H, int32_t W, int32_t classes) {
  if (N <= 0 || H <= 0 || W <= 0 || classes < 2 || classes > STP_MAX_CLASSES) return 0;
  return (size_t)N * H * W * 4 * up_class_bucket(classes) * sizeof(float);
}
extern "C" int stp_softmax_cce_dice_up(const void* low, const uint8_t* target, int32_t N, int32_t H, int32_t W, int32_t factor, int32_t classes,
                                       int32_t ldc, int32_t dtype, float w_cce, float w_dice, float* scalars, void* dlow, int32_t dl_channels,
                                       float grad_scale, const float* dev_scale, float* dev_record, void* workspace, size_t workspace_bytes,
                                       void* corners, size_t corner_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!low || !target || !scalars || !workspace || N <= 0 || H <= 0 || W <= 0 || classes < 2 || classes > STP_MAX_CLASSES || ldc < classes)
    return STP_E_BADARG;
  if (factor != 2 && factor != 4 && factor != 8 && factor != 16) return STP_E_BADARG;
  if ((int64_t)N * H * W * factor >= (1ll << 31)) return STP_E_BADARG;      // (work items are indexed in 32 bits)
  if (workspace_bytes < stp_loss_workspace_bytes()) return STP_E_WORKSPACE;
  if (dlow && (dl_channels < classes || !corners)) return STP_E_BADARG;
  if (dlow && corner_bytes < stp_softmax_cce_dice_up_corner_bytes(N, H, W, classes)) return STP_E_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(target) & 3) || (dlow && (reinterpret_cast<uintptr_t>(corners) & 15))) return STP_E_BADARG;
  const int lf = factor == 2 ? 1 : factor == 4 ? 2 : factor == 8 ? 3 : 4;
  hipStream_t s = (hipStream_t)stream;
  float* partial = (float*)workspace;
#define STP_UP(T, CM)                                                                                                                       \
  launch_softmax_up<T, CM>((const T*)low, target, N, H, W, lf, classes, ldc, w_cce, w_dice, scalars, (T*)dlow, dl_channels, grad_scale, \
                           dev_scale, dev_record, partial, (float*)corners, s)
#define STP_UP_T(T)                                                                                                                         \
  switch (up_class_bucket(classes)) {                                                                                                       \
    case 4: STP_UP(T, 4); break;                                                                                                            \
    case 8: STP_UP(T, 8); break;                                                                                                            \
    case 16: STP_UP(T, 16); break;                                                                                                          \
    case 24: STP_UP(T, 24); break;                                                                                                          \
    default: STP_UP(T, 32); break;                                                                                                          \
  }
  if (dtype == STP_H16) { STP_UP_T(bf16_t) }
  else if (dtype == STP_F32) { STP_UP_T(float) }
  else return STP_E_BADARG;
#undef STP_UP_T
#undef STP_UP
  STP_LAUNCH_CHECK();
  return STP_OK;
}

template <typename T>
__global__ void softmax_kernel(const T* __restrict__ logits, float* __restrict__ probs, int64_t pixels, int classes, int ldc) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    float p[STP_MAX_CLASSES];
    softmax_row<T, STP_MAX_CLASSES>(logits + i * ldc, classes, (ldc % Elem<T>::VEC) == 0, p);
#pragma unroll
    for (int c = 0; c < STP_MAX_CLASSES; ++c)
      if (c < classes) probs[i * classes + c] = p[c];
  }
}

extern "C" int stp_softmax(const void* logits, float* probs, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!logits || !probs || pixels <= 0 || classes < 1 || classes > STP_MAX_CLASSES || ldc < classes) return STP_E_BADARG;
  int64_t g = (pixels + 255) / 256;
  if (g > 4096) g = 4096;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == STP_H16) hipLaunchKernelGGL(softmax_kernel<bf16_t>, dim3((int)g), dim3(256), 0, s, (const bf16_t*)logits, probs, pixels, classes, ldc);
  else if (dtype == STP_F32) hipLaunchKernelGGL(softmax_kernel<float>, dim3((int)g), dim3(256), 0, s, (const float*)logits, probs, pixels, classes, ldc);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

template <typename T>
__global__ void sigmoid_kernel(const T* __restrict__ logits, float* __restrict__ probs, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    probs[i] = 1.f / (1.f + expf(-Elem<T>::load(logits + i)));
}

extern "C" int stp_sigmoid(const void* logits, float* probs, int64_t count, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!logits || !probs || count <= 0) return STP_E_BADARG;
  int64_t g = (count + 255) / 256;
  if (g > 4096) g = 4096;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == STP_H16) hipLaunchKernelGGL(sigmoid_kernel<bf16_t>, dim3((int)g), dim3(256), 0, s, (const bf16_t*)logits, probs, count);
  else if (dtype == STP_F32) hipLaunchKernelGGL(sigmoid_kernel<float>, dim3((int)g), dim3(256), 0, s, (const float*)logits, probs, count);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// Optimizers (Keras 2.2.4 formulas).  state[0] = iteration t (int), state[1] = lr_t (float bits)
// gscale[0] <= 0 (or NaN) = "skip this step": stp_grad_global_scale found a non-finite gradient (fp16 overflow under loss scaling).
// Every optimizer kernel - the per-step scalar preparation included - returns without touching parameters, moments or the step
// counter, so one overflowing batch cannot poison P / m / v.
__device__ __forceinline__ bool opt_skip(const float* gscale) { return gscale && !(gscale[0] > 0.f); }

__global__ void adam_prep_kernel(int32_t* state, const float* lr, float beta1, float beta2, const float* gscale) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || opt_skip(gscale)) return;
  const int t = state[0] + 1;
  state[0] = t;
  const double lr_t = (double)lr[0] * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t));
  reinterpret_cast<float*>(state)[1] = (float)lr_t;
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t count, const int32_t* state, float b1,
                                                   float b2, float eps, const uint8_t* __restrict__ mask,
                                                   const float* gscale, float clipvalue) {
  const float lr_t = reinterpret_cast<const float*>(state)[1];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 mv = load4(m + i * 4), vv = load4(v + i * 4), pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float mn = b1 * mv[e] + (1.f - b1) * gv[e];
      const float vn = b2 * vv[e] + (1.f - b2) * gv[e] * gv[e];
      pv[e] = pv[e] - lr_t * mn / (sqrtf(vn) + eps);
      mv[e] = mn;
      vv[e] = vn;
    }
    store4(m + i * 4, mv);
    store4(v + i * 4, vv);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_adam(float* param, const float* grad, float* m, float* v, int64_t count, const float* lr, float beta1,
                        float beta2, float eps, int32_t* state, const uint8_t* mask, const float* gscale, float clipvalue,
                        void* stream) {
  if (!param || !grad || !m || !v || !lr || !state || count <= 0 || (count & 3)) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(64), 0, s, state, lr, beta1, beta2, gscale);
  STP_LAUNCH_CHECK();
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(adam_kernel, dim3((int)g), dim3(256), 0, s, param, grad, m, v, count, state, beta1, beta2, eps, mask,
                     gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// RMSprop (keras/optimizers.py 2.2.4): a <- rho a + (1-rho) g^2 ; p <- p - lr g / (sqrt(a) + eps)
__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ acc,
                                                      int64_t count, const float* lr, float rho, float eps,
                                                      const uint8_t* __restrict__ mask, const float* gscale, float clipvalue) {
  const float l = lr[0];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 av = load4(acc + i * 4), pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float an = rho * av[e] + (1.f - rho) * gv[e] * gv[e];
      pv[e] = pv[e] - l * gv[e] / (sqrtf(an) + eps);
      av[e] = an;
    }
    store4(acc + i * 4, av);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_rmsprop(float* param, const float* grad, float* acc, int64_t count, const float* lr, float rho, float eps,
                           const uint8_t* mask, const float* gscale, float clipvalue, void* stream) {
  if (!param || !grad || !acc || !lr || count <= 0 || (count & 3)) return STP_E_BADARG;
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(rmsprop_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, param, grad, acc, count, lr, rho, eps, mask,
                     gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// Nadam (keras/optimizers.py 2.2.4, schedule_decay form).  state[0] = iteration t, fstate[0] = m_schedule (starts at 1),
// fstate[1..5] = this step's scalars {1/(1-m_schedule_new), 1/(1-m_schedule_next), 1/(1-beta2^t), 1-mu_t, mu_{t+1}}
__global__ void nadam_prep_kernel(int32_t* state, float* fstate, float beta1, float beta2, float schedule_decay, const float* gscale) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || opt_skip(gscale)) return;
  const int t = state[0] + 1;
  state[0] = t;
  const double mu_t = (double)beta1 * (1.0 - 0.5 * pow(0.96, (double)t * (double)schedule_decay));
  const double mu_t1 = (double)beta1 * (1.0 - 0.5 * pow(0.96, (double)(t + 1) * (double)schedule_decay));
  const double ms_new = (double)fstate[0] * mu_t;
  const double ms_next = ms_new * mu_t1;
  fstate[0] = (float)ms_new;
  fstate[1] = (float)(1.0 / (1.0 - ms_new));
  fstate[2] = (float)(1.0 / (1.0 - ms_next));
  fstate[3] = (float)(1.0 / (1.0 - pow((double)beta2, (double)t)));
  fstate[4] = (float)(1.0 - mu_t);
  fstate[5] = (float)mu_t1;
}

__global__ __launch_bounds__(256) void nadam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t count, const float* lr, const float* fstate,
                                                    float b1, float b2, float eps, const uint8_t* __restrict__ mask,
                                                    const float* gscale, float clipvalue) {
  const float l = lr[0];
  const float ig = fstate[1], im = fstate[2], iv = fstate[3], cg = fstate[4], cm = fstate[5];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 mv = load4(m + i * 4), vv = load4(v + i * 4), pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float mn = b1 * mv[e] + (1.f - b1) * gv[e];
      const float vn = b2 * vv[e] + (1.f - b2) * gv[e] * gv[e];
      const float mbar = cg * (gv[e] * ig) + cm * (mn * im);
      pv[e] = pv[e] - l * mbar / (sqrtf(vn * iv) + eps);
      mv[e] = mn;
      vv[e] = vn;
    }
    store4(m + i * 4, mv);
    store4(v + i * 4, vv);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_nadam(float* param, const float* grad, float* m, float* v, int64_t count, const float* lr, float beta1,
                         float beta2, float eps, float schedule_decay, int32_t* state, float* fstate, const uint8_t* mask,
                         const float* gscale, float clipvalue, void* stream) {
  if (!param || !grad || !m || !v || !lr || !state || !fstate || count <= 0 || (count & 3)) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nadam_prep_kernel, dim3(1), dim3(64), 0, s, state, fstate, beta1, beta2, schedule_decay, gscale);
  STP_LAUNCH_CHECK();
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(nadam_kernel, dim3((int)g), dim3(256), 0, s, param, grad, m, v, count, lr, fstate, beta1, beta2, eps, mask,
                     gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ vel,
                                                  int64_t count, const float* lr, float mu, int nesterov,
                                                  const uint8_t* __restrict__ mask, const float* gscale, float clipvalue) {
  const float l = lr[0];
  if (opt_skip(gscale)) return;
  const float gs = gscale ? gscale[0] : 1.f;
  const int64_t n4 = count >> 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    f32x4 gv = load4(g + i * 4) * gs;
    if (clipvalue > 0.f)
#pragma unroll
      for (int e = 0; e < 4; ++e) gv[e] = fminf(fmaxf(gv[e], -clipvalue), clipvalue);
    f32x4 vv = vel ? load4(vel + i * 4) : f32x4{0.f, 0.f, 0.f, 0.f}, pv = load4(p + i * 4);
    uint32_t mk = mask ? *reinterpret_cast<const uint32_t*>(mask + i * 4) : 0x01010101u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!((mk >> (8 * e)) & 0xff)) continue;
      const float vn = mu * vv[e] - l * gv[e];
      pv[e] = nesterov ? pv[e] + mu * vn - l * gv[e] : pv[e] + vn;
      vv[e] = vn;
    }
    if (vel) store4(vel + i * 4, vv);
    store4(p + i * 4, pv);
  }
}

extern "C" int stp_sgd(float* param, const float* grad, float* vel, int64_t count, const float* lr, float momentum,
                       int32_t nesterov, const uint8_t* mask, const float* gscale, float clipvalue, void* stream) {
  if (!param || !grad || !lr || count <= 0 || (count & 3)) return STP_E_BADARG;
  int64_t g = ((count >> 2) + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(sgd_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, param, grad, vel, count, lr, momentum,
                     nesterov, mask, gscale, clipvalue);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ||grad||^2 partials -> gscale = min(1, clipnorm/||base*g||) * base   (base = 1/world_size)
__global__ __launch_bounds__(256) void sqsum_partial_kernel(const float* __restrict__ g, int64_t count, float* partial) {
  float a = 0.f;
  const int64_t per = (count + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < count ? i0 + per : count;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) a += g[i] * g[i];
  __shared__ float red[4];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void gscale_finalize_kernel(const float* partial, int blocks, float clipnorm, float base,
                                                              float* gscale) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) a += (double)partial[b];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double norm = sqrt(sh[0]) * (double)base;  // norm of the (mean) gradient the optimizer will see
  if (!(sh[0] >= 0.0 && sh[0] < 1e300 * 1e300) || !(norm == norm)) {   // inf / NaN somewhere in the arena: the step is skipped (opt_skip)
    gscale[0] = -1.f;
    gscale[1] += 1.f;                              // skipped steps so far (host: HipSegModel.skipped_steps)
    return;
  }
  double k = 1.0;
  if (clipnorm > 0.f && norm > (double)clipnorm) k = (double)clipnorm / norm;
  gscale[0] = (float)(k * (double)base);
}

extern "C" int stp_grad_global_scale(const float* grad, int64_t count, float clipnorm, float base, float* gscale,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (!grad || !gscale || !workspace || count <= 0) return STP_E_BADARG;
  if (workspace_bytes < 1024 * sizeof(float)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int64_t b = count / 4096;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  hipLaunchKernelGGL(sqsum_partial_kernel, dim3((int)b), dim3(256), 0, s, grad, count, (float*)workspace);
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gscale_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (int)b, clipnorm, base, gscale);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ---- dynamic loss scaling (fp16 storage).  dls = float[8] on the device: [0] multiplier m of the NEXT backward pass (a power of two, on
// top of the static scale the loss kernels apply), [1] clean steps since the last change, [2] growth interval (steps), [3] smallest m,
// [4] m of the gradients now in the arena (written by stp_scale_by_device when the backward pass is seeded), [5] largest m.  Everything happens on the device, inside the
// captured step: stp_scale_by_device multiplies the loss gradient by m right after the loss kernel seeded it; the _dls form of
// stp_grad_global_scale folds 1/m into gscale, halves m when the step is skipped (non-finite gradient) and doubles it after
// `interval` clean steps - the schedule of torch.cuda.amp.GradScaler / Keras' LossScaleOptimizer.
template <typename T>
__global__ __launch_bounds__(256) void scale_by_device_kernel(T* __restrict__ x, int64_t count, const float* __restrict__ scalar, float* record) {
  const float m = scalar[0];
  if (record && blockIdx.x == 0 && threadIdx.x == 0) record[0] = m;      // (the multiplier this backward pass runs under: dls[4])
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256)
    Elem<T>::store(x + i, Elem<T>::load(x + i) * m);
}
extern "C" int stp_scale_by_device(void* x, int64_t count, int32_t dtype, const float* scalar, float* record, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;
  if (!x || !scalar || count <= 0) return STP_E_BADARG;
  int64_t g = (count + 255) / 256;
  if (g > 8192) g = 8192;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == STP_H16) hipLaunchKernelGGL(scale_by_device_kernel<bf16_t>, dim3((int)g), dim3(256), 0, s, (bf16_t*)x, count, scalar, record);
  else if (dtype == STP_F32) hipLaunchKernelGGL(scale_by_device_kernel<float>, dim3((int)g), dim3(256), 0, s, (float*)x, count, scalar, record);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

__global__ __launch_bounds__(256) void gscale_finalize_dls_kernel(const float* partial, int blocks, float clipnorm, float base,
                                                                  float* gscale, float* dls) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) a += (double)partial[b];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float m = dls[0];
  // the gradients in the arena were produced under dls[4] (recorded by stp_scale_by_device when their backward pass was seeded);
  // dls[0] is the multiplier of the NEXT pass - equal only while every step is one backward pass followed by one optimizer launch
  const double eff = (double)base / (double)dls[4];  // what turns an arena value into the gradient the optimizer sees
  const double norm = sqrt(sh[0]) * eff;
  if (!(sh[0] >= 0.0 && sh[0] < 1e300 * 1e300) || !(norm == norm)) {   // overflow: skip the step, halve the multiplier
    gscale[0] = -1.f;
    gscale[1] += 1.f;
    dls[0] = fmaxf(m * 0.5f, dls[3]);
    dls[1] = 0.f;
    return;
  }
  double k = 1.0;
  if (clipnorm > 0.f && norm > (double)clipnorm) k = (double)clipnorm / norm;
  gscale[0] = (float)(k * eff);
  const float clean = dls[1] + 1.f;
  if (clean >= dls[2]) { dls[0] = fminf(m * 2.f, dls[5]); dls[1] = 0.f; }
  else dls[1] = clean;
}

extern "C" int stp_grad_global_scale_dls(const float* grad, int64_t count, float clipnorm, float base, float* gscale, float* dls,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  if (!grad || !gscale || !dls || !workspace || count <= 0) return STP_E_BADARG;
  if (workspace_bytes < 1024 * sizeof(float)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  int64_t b = count / 4096;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  hipLaunchKernelGGL(sqsum_partial_kernel, dim3((int)b), dim3(256), 0, s, grad, count, (float*)workspace);
  STP_LAUNCH_CHECK();
  hipLaunchKernelGGL(gscale_finalize_dls_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, (int)b, clipnorm, base, gscale, dls);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// weight compute copies.  master [Cout][KH][KW][Cin] fp32.
//   fwd [rows_f][KH][KWp][Cinp]  (rows_f = Cout rounded up to 16; zero padded)
//   bwd [rows_b][KH][KW][CoutB]  bwd[ci][kh][kw][co] = master[co][KH-1-kh][KW-1-kw][ci]
//                                (rows_b = Cin rounded up to 16, CoutB >= Cout; zero padded)
template <typename T>
__global__ __launch_bounds__(256) void weight_prepare_kernel(const float* __restrict__ w, T* __restrict__ fwd, T* __restrict__ bwd,
                                                             int Cout, int KH, int KW, int Cin, int KWp, int Cinp, int CoutB,
                                                             int rows_f, int rows_b) {
  const int64_t nf = fwd ? (int64_t)rows_f * KH * KWp * Cinp : 0;
  const int64_t nb = bwd ? (int64_t)rows_b * KH * KW * CoutB : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nf + nb; i += (int64_t)gridDim.x * 256) {
    if (i < nf) {
      int64_t r = i;
      const int ci = (int)(r % Cinp); r /= Cinp;
      const int kw = (int)(r % KWp); r /= KWp;
      const int kh = (int)(r % KH);
      const int co = (int)(r / KH);
      float v = 0.f;
      if (co < Cout && kw < KW && ci < Cin) v = w[(((int64_t)co * KH + kh) * KW + kw) * Cin + ci];
      Elem<T>::store(fwd + i, v);
    } else {
      int64_t r = i - nf;
      const int co = (int)(r % CoutB); r /= CoutB;
      const int kw = (int)(r % KW); r /= KW;
      const int kh = (int)(r % KH);
      const int ci = (int)(r / KH);
      float v = 0.f;
      if (co < Cout && ci < Cin) v = w[(((int64_t)co * KH + (KH - 1 - kh)) * KW + (KW - 1 - kw)) * Cin + ci];
      Elem<T>::store(bwd + (i - nf), v);
    }
  }
}

extern "C" int stp_weight_prepare(const float* master, void* fwd, void* bwd, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin,
                                  int32_t KWp, int32_t Cinp, int32_t CoutB, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!master || (!fwd && !bwd) || KWp < KW || Cinp < Cin || CoutB < Cout) return STP_E_BADARG;
  const int rows_f = round_up(Cout, 16), rows_b = round_up(Cin, 16);
  const int64_t total = (fwd ? (int64_t)rows_f * KH * KWp * Cinp : 0) + (bwd ? (int64_t)rows_b * KH * KW * CoutB : 0);
  int64_t g = (total + 255) / 256;
  if (g > 2048) g = 2048;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == STP_H16)
    hipLaunchKernelGGL(weight_prepare_kernel<bf16_t>, dim3((int)g), dim3(256), 0, s, master, (bf16_t*)fwd, (bf16_t*)bwd, Cout, KH,
                       KW, Cin, KWp, Cinp, CoutB, rows_f, rows_b);
  else if (dtype == STP_F32)
    hipLaunchKernelGGL(weight_prepare_kernel<float>, dim3((int)g), dim3(256), 0, s, master, (float*)fwd, (float*)bwd, Cout, KH, KW,
                       Cin, KWp, Cinp, CoutB, rows_f, rows_b);
  else
    return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// All layers in one launch: desc[l] describes layer l, `start` is the running element count (fwd then bwd
// elements of every layer); a thread finds its layer by binary search.  Same arithmetic as the
// per-layer kernel above, 1 launch instead of ~50 per step.
struct WeightPrepDesc {
  const float* master;
  void* fwd;
  void* bwd;
  int64_t start;      // first global element index of this layer
  int32_t Cout, KH, KW, Cin, KWp, Cinp, CoutB, rows_f, rows_b, pad_;
};

// grid.y = layer; the workgroups of a layer stride over its (tap, 32-cout, 32-cin) units.  A unit is read once
// from the fp32 master (cin fastest: coalesced), held in LDS, and written twice: the forward copy in the same
// orientation and the data-gradient copy transposed (cout fastest) with the taps flipped - both coalesced.
// Padding (Cinp > Cin, KWp > KW, row padding to 16, CoutB > Cout) is written as zeros.
// 16-bit layers without padding (Cin a multiple of 64, Cout of 32: every layer that matters by bytes): a unit is (tap, 32 cout,
// 64 cin) - 16-byte loads of the fp32 master, 16-byte stores of BOTH copies (8 consecutive cin of a cout row forward, 8 consecutive
// cout of a cin row transposed).  Same rounding per element as the generic path below: bit-identical copies.
template <typename T>
__device__ __forceinline__ void weight_prepare_fast_layer(const WeightPrepDesc& d, float (*tile)[65]) {
  const int CT = d.Cout >> 5, IT = d.Cin >> 6, taps = d.KH * d.KW;
  const int units = taps * CT * IT;
  const int tid = threadIdx.x;
  T* fwd = reinterpret_cast<T*>(d.fwd);
  T* bwd = reinterpret_cast<T*>(d.bwd);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int it = u % IT, ct = (u / IT) % CT, tap = u / (IT * CT);
    const int kh = tap / d.KW, kw = tap - kh * d.KW;
    const int co0 = ct * 32, ci0 = it * 64;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int r = p * 16 + (tid >> 4), c4 = (tid & 15) * 4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(d.master + (((int64_t)(co0 + r) * d.KH + kh) * d.KW + kw) * d.Cin + ci0 + c4);
      tile[r][c4] = v.x; tile[r][c4 + 1] = v.y; tile[r][c4 + 2] = v.z; tile[r][c4 + 3] = v.w;
    }
    __syncthreads();
    if (fwd) {
      const int r = tid >> 3, c8 = (tid & 7) * 8;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(tile[r][c8 + 2 * e], tile[r][c8 + 2 * e + 1]);
      *reinterpret_cast<u32x4*>(fwd + (((int64_t)(co0 + r) * d.KH + kh) * d.KW + kw) * d.Cin + ci0 + c8) = o;
    }
    if (bwd) {
      const int ci = tid >> 2, c8 = (tid & 3) * 8;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = pack_bf16x2(tile[c8 + 2 * e][ci], tile[c8 + 2 * e + 1][ci]);
      *reinterpret_cast<u32x4*>(bwd + (((int64_t)(ci0 + ci) * d.KH + (d.KH - 1 - kh)) * d.KW + (d.KW - 1 - kw)) * d.Cout + co0 + c8) = o;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void weight_prepare_batched_kernel(const WeightPrepDesc* __restrict__ desc, int nlayers, int64_t total) {
  __shared__ float tile[32][65];
  const WeightPrepDesc d = desc[blockIdx.y];
  if constexpr (sizeof(T) == 2) {
    if (!(d.Cin & 63) && !(d.Cout & 31) && d.Cinp == d.Cin && d.KWp == d.KW && d.CoutB == d.Cout && d.rows_f == d.Cout && d.rows_b == d.Cin &&
        !(reinterpret_cast<uintptr_t>(d.master) & 15) && !(reinterpret_cast<uintptr_t>(d.fwd) & 15) && !(reinterpret_cast<uintptr_t>(d.bwd) & 15)) {
      weight_prepare_fast_layer<T>(d, tile);
      return;
    }
  }
  const int co_ext = d.bwd ? (d.rows_f > d.CoutB ? d.rows_f : d.CoutB) : d.rows_f;
  const int ci_ext = d.bwd ? (d.Cinp > d.rows_b ? d.Cinp : d.rows_b) : d.Cinp;
  const int CT = (co_ext + 31) >> 5, IT = (ci_ext + 31) >> 5, taps = d.KH * d.KWp;
  const int units = taps * CT * IT;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  T* fwd = reinterpret_cast<T*>(d.fwd);
  T* bwd = reinterpret_cast<T*>(d.bwd);
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int it = u % IT;
    const int ct = (u / IT) % CT;
    const int tap = u / (IT * CT);
    const int kh = tap / d.KWp, kw = tap - kh * d.KWp;
    const int co0 = ct * 32, ci0 = it * 32;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int co = co0 + ty + 8 * p, ci = ci0 + tx;
      float v = 0.f;
      if (co < d.Cout && kw < d.KW && ci < d.Cin) v = d.master[(((int64_t)co * d.KH + kh) * d.KW + kw) * d.Cin + ci];
      tile[ty + 8 * p][tx] = v;
      if (fwd && co < d.rows_f && ci < d.Cinp) Elem<T>::store(fwd + (((int64_t)co * d.KH + kh) * d.KWp + kw) * d.Cinp + ci, v);
    }
    __syncthreads();
    if (bwd && kw < d.KW) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int ci = ci0 + ty + 8 * p, co = co0 + tx;
        if (ci < d.rows_b && co < d.CoutB)
          Elem<T>::store(bwd + (((int64_t)ci * d.KH + (d.KH - 1 - kh)) * d.KW + (d.KW - 1 - kw)) * d.CoutB + co, tile[tx][ty + 8 * p]);
      }
    }
    __syncthreads();
  }
}

extern "C" size_t stp_weight_prepare_desc_bytes(void) { return sizeof(WeightPrepDesc); }

// Fills one host-side descriptor (the caller uploads the array to the device); returns the element count.
extern "C" int64_t stp_weight_prepare_desc_fill(void* desc_host, int32_t index, int64_t start, const float* master, void* fwd,
                                                void* bwd, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin, int32_t KWp,
                                                int32_t Cinp, int32_t CoutB) {
  WeightPrepDesc* d = reinterpret_cast<WeightPrepDesc*>(desc_host) + index;
  d->master = master; d->fwd = fwd; d->bwd = bwd; d->start = start;
  d->Cout = Cout; d->KH = KH; d->KW = KW; d->Cin = Cin; d->KWp = KWp; d->Cinp = Cinp; d->CoutB = CoutB;
  d->rows_f = round_up(Cout, 16); d->rows_b = round_up(Cin, 16); d->pad_ = 0;
  return (fwd ? (int64_t)d->rows_f * KH * KWp * Cinp : 0) + (bwd ? (int64_t)d->rows_b * KH * KW * CoutB : 0);
}

extern "C" int stp_weight_prepare_batched(const void* desc_dev, int32_t nlayers, int64_t total, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!desc_dev || nlayers <= 0 || total <= 0) return STP_E_BADARG;
  // grid.x workgroups per layer: the big layers (9.4 MB, 2304 units) grid-stride over them, the surplus workgroups of the small
  // layers exit at once (64 -> 256: the launch lasts as long as its largest layer, 130 -> see DESIGN)
  hipStream_t s = (hipStream_t)stream;
  static const int per_layer = getenv("STP_PREP_BLOCKS") ? atoi(getenv("STP_PREP_BLOCKS")) : 512;
  if (dtype == STP_H16)
    hipLaunchKernelGGL(weight_prepare_batched_kernel<bf16_t>, dim3(per_layer, nlayers), dim3(256), 0, s, (const WeightPrepDesc*)desc_dev, nlayers, total);
  else if (dtype == STP_F32)
    hipLaunchKernelGGL(weight_prepare_batched_kernel<float>, dim3(per_layer, nlayers), dim3(256), 0, s, (const WeightPrepDesc*)desc_dev, nlayers, total);
  else
    return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// Class-collapsed weights of a 3x3 convolution over a NEAREST-2x upsampled source (stp_conv_params.weight_up): for output parity
// (py, px) the taps that read the same low-resolution pixel are summed - rows (py, ty): (0,0) {0}, (0,1) {1,2}, (1,0) {0,1}, (1,1) {2}.
// out[row][c = py*2+px][t = ty*2+tx][ci], row < round_up(Cout, 16) (zero rows behind Cout); sums in fp32, one rounding.
struct UpcollapseDesc {     // 32 bytes (the host packs it as two pointers + four int32)
  const float* master;
  void* out;
  int32_t Cout, rows, C0, Ctot;
};

template <typename T>
__device__ __forceinline__ void weight_upcollapse_layer(const UpcollapseDesc& d, int64_t first, int64_t stride) {
  T* out = reinterpret_cast<T*>(d.out);
  if constexpr (sizeof(T) == 2) {
    // 8 consecutive input channels per thread (C0 and Ctot multiples of 8, 16-byte aligned rows): 16-byte loads and stores, 32-bit
    // index arithmetic; same fp32 sums in the same order, one rounding: bit-identical to the element-wise loop below
    if (!(d.C0 & 7) && !(d.Ctot & 7) && !(reinterpret_cast<uintptr_t>(d.master) & 15) && !(reinterpret_cast<uintptr_t>(d.out) & 15) &&
        (int64_t)d.rows * 16 * d.C0 < (1ll << 31)) {
      const uint32_t c8n = (uint32_t)d.C0 >> 3, n8 = (uint32_t)d.rows * 16u * c8n;
      for (uint32_t i = (uint32_t)first; i < n8; i += (uint32_t)stride) {
        const uint32_t q = i / c8n, ci = (i - q * c8n) * 8u, ct = q & 15u, co = q >> 4;
        const int py = ct >> 3, px = (ct >> 2) & 1, ty = (ct >> 1) & 1, tx = ct & 1;
        const int kh0 = (py == 0) ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), kh1 = (py == 0) ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
        const int kw0 = (px == 0) ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kw1 = (px == 0) ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
        f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = v0;
        if ((int)co < d.Cout)
          for (int kh = kh0; kh <= kh1; ++kh)
            for (int kw = kw0; kw <= kw1; ++kw) {
              const float* src = d.master + (((int64_t)co * 3 + kh) * 3 + kw) * d.Ctot + ci;
              v0 += *reinterpret_cast<const f32x4*>(src);
              v1 += *reinterpret_cast<const f32x4*>(src + 4);
            }
        *reinterpret_cast<u32x4*>(out + (size_t)i * 8) = u32x4{pack_bf16x2(v0.x, v0.y), pack_bf16x2(v0.z, v0.w), pack_bf16x2(v1.x, v1.y), pack_bf16x2(v1.z, v1.w)};
      }
      return;
    }
  }
  const int64_t n = (int64_t)d.rows * 16 * d.C0;
  for (int64_t i = first; i < n; i += stride) {
    const int ci = (int)(i % d.C0);
    const int ct = (int)((i / d.C0) & 15);
    const int co = (int)(i / ((int64_t)16 * d.C0));
    const int py = ct >> 3, px = (ct >> 2) & 1, ty = (ct >> 1) & 1, tx = ct & 1;
    const int kh0 = (py == 0) ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), kh1 = (py == 0) ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
    const int kw0 = (px == 0) ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kw1 = (px == 0) ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
    float v = 0.f;
    if (co < d.Cout)
      for (int kh = kh0; kh <= kh1; ++kh)
        for (int kw = kw0; kw <= kw1; ++kw) v += d.master[(((int64_t)co * 3 + kh) * 3 + kw) * d.Ctot + ci];
    Elem<T>::store(out + i, v);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void weight_upcollapse_kernel(UpcollapseDesc d) {
  weight_upcollapse_layer<T>(d, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}
// grid.y = layer (descriptor table on the device): ONE launch per step for all decoder stages
template <typename T>
__global__ __launch_bounds__(256) void weight_upcollapse_batched_kernel(const UpcollapseDesc* __restrict__ desc) {
  weight_upcollapse_layer<T>(desc[blockIdx.y], (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}

extern "C" int stp_weight_prepare_upcollapse(const float* master, void* weight_up, int32_t Cout, int32_t C0, int32_t C1, int32_t dtype,
                                             void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!master || !weight_up || Cout <= 0 || C0 <= 0 || C1 < 0) return STP_E_BADARG;
  UpcollapseDesc d;
  d.master = master; d.out = weight_up; d.Cout = Cout; d.rows = round_up(Cout, 16); d.C0 = C0; d.Ctot = C0 + C1;
  int64_t g = ((int64_t)d.rows * 16 * C0 + 255) / 256;
  if (g > 2048) g = 2048;
  if (dtype == STP_H16) hipLaunchKernelGGL(weight_upcollapse_kernel<bf16_t>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, d);
  else if (dtype == STP_F32) hipLaunchKernelGGL(weight_upcollapse_kernel<float>, dim3((int)g), dim3(256), 0, (hipStream_t)stream, d);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" size_t stp_weight_prepare_upcollapse_desc_bytes(void) { return sizeof(UpcollapseDesc); }

// desc_dev: `nlayers` descriptors {const float* master; void* out; int32 Cout, rows (= Cout rounded up to 16), C0, C0 + C1} on the device
extern "C" int stp_weight_prepare_upcollapse_batched(const void* desc_dev, int32_t nlayers, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!desc_dev || nlayers <= 0) return STP_E_BADARG;
  const dim3 grid(256, nlayers);
  if (dtype == STP_H16) hipLaunchKernelGGL(weight_upcollapse_batched_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else if (dtype == STP_F32) hipLaunchKernelGGL(weight_upcollapse_batched_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// The data gradient w.r.t. the LOW-RESOLUTION source of such a convolution is a plain 4x4 / stride 2 / pad 1 convolution of dY:
// dX_lo[i] takes dY rows 2i-1 .. 2i+2 through the row-tap sums {2}, {1,2}, {0,1}, {0} of the 3x3 kernel (columns alike) - 16
// instead of 36 taps per low-resolution pixel, and neither the high-resolution gradient nor its 2x2 fold exist.  out = the weight
// matrix of that convolution, [round_up(C0, 16)][4][4][CoutB] (rows = input channels of the forward layer, zero padding).
// Descriptor: UpcollapseDesc with `rows` holding CoutB.
template <typename T>
__global__ __launch_bounds__(256) void weight_upcollapse_bwd_batched_kernel(const UpcollapseDesc* __restrict__ desc) {
  const UpcollapseDesc d = desc[blockIdx.y];
  const int CoutB = d.rows, rows = (d.C0 + 15) / 16 * 16;
  T* out = reinterpret_cast<T*>(d.out);
  const int64_t n = (int64_t)rows * 16 * CoutB;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int co = (int)(i % CoutB);
    const int rs = (int)((i / CoutB) & 15);
    const int ci = (int)(i / ((int64_t)16 * CoutB));
    const int r = rs >> 2, c = rs & 3;
    const int kh0 = r == 0 ? 2 : r == 1 ? 1 : 0, kh1 = r == 0 ? 2 : r == 1 ? 2 : r == 2 ? 1 : 0;
    const int kw0 = c == 0 ? 2 : c == 1 ? 1 : 0, kw1 = c == 0 ? 2 : c == 1 ? 2 : c == 2 ? 1 : 0;
    float v = 0.f;
    if (co < d.Cout && ci < d.C0)
      for (int kh = kh0; kh <= kh1; ++kh)
        for (int kw = kw0; kw <= kw1; ++kw) v += d.master[(((int64_t)co * 3 + kh) * 3 + kw) * d.Ctot + ci];
    Elem<T>::store(out + i, v);
  }
}

// desc_dev: nlayers records {const float* master; void* out; int32 Cout, CoutB, C0, C0 + C1} (32 bytes each) on the device
extern "C" int stp_weight_prepare_upcollapse_bwd_batched(const void* desc_dev, int32_t nlayers, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!desc_dev || nlayers <= 0) return STP_E_BADARG;
  const dim3 grid(256, nlayers);
  if (dtype == STP_H16) hipLaunchKernelGGL(weight_upcollapse_bwd_batched_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else if (dtype == STP_F32) hipLaunchKernelGGL(weight_upcollapse_bwd_batched_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const UpcollapseDesc*)desc_dev);
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// padded gradient [CoutP][KH][KWp][Cinp] -> master layout [Cout][KH][KW][Cin]
__global__ void weight_grad_unpad_kernel(const float* __restrict__ padded, float* __restrict__ grad, int Cout, int KH, int KW,
                                         int Cin, int KWp, int Cinp, int accumulate) {
  const int64_t n = (int64_t)Cout * KH * KW * Cin;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    int64_t r = i;
    const int ci = (int)(r % Cin); r /= Cin;
    const int kw = (int)(r % KW); r /= KW;
    const int kh = (int)(r % KH);
    const int co = (int)(r / KH);
    const float v = padded[(((int64_t)co * KH + kh) * KWp + kw) * Cinp + ci];
    grad[i] = accumulate ? grad[i] + v : v;
  }
}

extern "C" int stp_weight_grad_unpad(const float* padded, float* grad, int32_t Cout, int32_t KH, int32_t KW, int32_t Cin,
                                     int32_t KWp, int32_t Cinp, int32_t accumulate, void* stream) {
  if (!padded || !grad) return STP_E_BADARG;
  int64_t g = ((int64_t)Cout * KH * KW * Cin + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(weight_grad_unpad_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, padded, grad, Cout, KH, KW, Cin,
                     KWp, Cinp, accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// Gradient of the beta of the input BatchNormalization (bn_data, scale=False) without a stem
// data-gradient pass.  The stem input carries a constant-one 4th channel, so the padded stem
// weight gradient holds S[co][kh][kw] = sum over valid taps of dY in channel slot `one_ch`;
//   dbeta[c] = sum_{co,kh,kw} W[co][kh][kw][c] * S[co][kh][kw].
__global__ void stem_beta_grad_kernel(const float* __restrict__ padded_dw, const float* __restrict__ w, float* __restrict__ dbeta,
                                      int Cout, int KH, int KW, int Cin, int KWp, int Cinp, int one_ch) {
  const int c = blockIdx.x;
  float a = 0.f;
  const int n = Cout * KH * KW;
  for (int i = threadIdx.x; i < n; i += 256) {
    int r = i;
    const int kw = r % KW; r /= KW;
    const int kh = r % KH;
    const int co = r / KH;
    a += w[(((int64_t)co * KH + kh) * KW + kw) * Cin + c] * padded_dw[(((int64_t)co * KH + kh) * KWp + kw) * Cinp + one_ch];
  }
  // 4 waves (the kernel is the tail of the backward pass: 3136 products per channel, latency-bound at 64 threads)
  __shared__ float red[4];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) dbeta[c] = ((red[0] + red[1]) + red[2]) + red[3];
}

extern "C" int stp_stem_beta_grad(const float* padded_dw, const float* master, float* dbeta, int32_t Cout, int32_t KH,
                                  int32_t KW, int32_t Cin, int32_t KWp, int32_t Cinp, int32_t one_ch, void* stream) {
  if (!padded_dw || !master || !dbeta || one_ch >= Cinp) return STP_E_BADARG;
  hipLaunchKernelGGL(stem_beta_grad_kernel, dim3(Cin), dim3(256), 0, (hipStream_t)stream, padded_dw, master, dbeta, Cout, KH, KW,
                     Cin, KWp, Cinp, one_ch);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
__global__ void cast_f32_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = f32_to_bf16(src[i]);
}
__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, int64_t count, float scale) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) dst[i] = bf16_to_f32(src[i]) * scale;
}
extern "C" int stp_cast_f32_to_bf16(const float* src, void* dst, int64_t count, void* stream) {
  if (!src || !dst || count <= 0) return STP_E_BADARG;
  int64_t g = (count + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, src, (bf16_t*)dst, count);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
extern "C" int stp_cast_bf16_to_f32(const void* src, float* dst, int64_t count, float scale, void* stream) {
  if (!src || !dst || count <= 0) return STP_E_BADARG;
  int64_t g = (count + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3((int)g), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, dst, count, scale);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_abi_version(void) { return 1; }
extern "C" int stp_storage_dtype(void) { return STP_H16; }
