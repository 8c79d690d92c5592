// The two-stage fixed-order reduction every loss head runs, once: value pass -> per-workgroup partials -> one-workgroup finalize in
// double -> scalars -> gradient pass.  The ORDER OF ADDITIONS is what keeps graph replay bit-identical, and it is defined here only:
//   wave      wave_sum (xor butterfly, 32 .. 1)
//   workgroup the four wave values left to right, r0 + r1 + r2 + r3 (LOSS_WAVES_LTR), or pairwise, (r0 + r1) + (r2 + r3)
//             (LOSS_WAVES_PAIRWISE: the multi-label value pass and every bias-gradient sum) - float addition is not associative, a
//             kernel keeps the order it was written with
//   finalize  sum e = tid % NSUM, lane = tid / NSUM adds partial[b][e] for b = lane, lane + 256 / NSUM, ... in that order into a double,
//             then a halving LDS tree over the lanes
// Included by every loss translation unit (loss_sigmoid / loss_softmax / loss_softmax_ex / loss_multilabel / loss_prob .hip).
// The build contracts within a source expression (-ffp-contract=on): an expression that moves here moves whole.
#pragma once
#include "common.h"
#include <type_traits>

#define LOSS_MAX_BLOCKS 1024         // value-pass workgroups; stp_loss_workspace_bytes() covers 1024 x 16 partial floats
// the workspace of stp_loss_workspace_bytes(): the partial rows, then one bias-gradient partial per gradient workgroup of the one-class
// sigmoid heads (stp_sigmoid_loss_bias_grad)
#define LOSS_GSUM_OFFSET (LOSS_MAX_BLOCKS * 16)
#define LOSS_GRAD_MAX_BLOCKS 4096
#define LOSS_WAVES_LTR 0
#define LOSS_WAVES_PAIRWISE 1

struct LossWeights { float w[5]; };  // the registry order: crossentropy, dice_loss, iou_loss, jaccard_loss, focal_loss

// ---- workgroup epilogue (256 threads): the per-thread sums a[0 .. NUSED) -> partial[block][0 .. NSUM), zeros from NUSED on.
// NLDS = columns of the LDS table where a kernel keeps more than it uses.  One kernel keeps a copy of these statements:
// loss_partial_kernel (loss_sigmoid.hip, the headline's value pass) compiles to 9 more vector registers through this call (80 -> 89,
// 6 -> 5 waves per SIMD in the bf16 build) - a fix to the statements below goes there too.
template <int NSUM, int NUSED, int ORDER = LOSS_WAVES_LTR, int NLDS = NUSED>
__device__ __forceinline__ void loss_block_sums(float (&a)[NUSED], float* partial) {
  static_assert(NUSED <= NSUM && NUSED <= NLDS, "more sums than the partial row holds");
  __shared__ float red[4][NLDS];
#pragma unroll
  for (int e = 0; e < NUSED; ++e) a[e] = wave_sum(a[e]);
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int e = 0; e < NUSED; ++e) red[threadIdx.x >> 6][e] = a[e];
  __syncthreads();
  if (threadIdx.x < NSUM) {
    const bool used = NUSED == NSUM || threadIdx.x < NUSED;
    if constexpr (ORDER == LOSS_WAVES_PAIRWISE)
      partial[(size_t)blockIdx.x * NSUM + threadIdx.x] =
          used ? (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]) : 0.f;
    else
      partial[(size_t)blockIdx.x * NSUM + threadIdx.x] =
          used ? red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x] : 0.f;
  }
}

// ---- finalize reduction (one workgroup of 256): returns s[0 .. NSUM), the sums over `blocks` partial rows, valid in every thread.
// 64 / NSUM loads in flight per thread (a run-time trip count keeps one); the additions run in the order of the plain loop.
template <int NSUM>
__device__ __forceinline__ const double* loss_finalize_sums(const float* partial, int blocks) {
  static_assert(NSUM == 8 || NSUM == 16, "partial rows are 8 or 16 floats");
  constexpr int LANES = 256 / NSUM, FLIGHT = 64 / NSUM;
  __shared__ double sh[LANES][NSUM];
  const int e = threadIdx.x % NSUM, lane = threadIdx.x / NSUM;
  double a = 0.0;
  {
    int b = lane;
    for (; b + LANES * (FLIGHT - 1) < blocks; b += LANES * FLIGHT) {
      float v[FLIGHT];
#pragma unroll
      for (int u = 0; u < FLIGHT; ++u) v[u] = partial[(size_t)(b + LANES * u) * NSUM + e];
#pragma unroll
      for (int u = 0; u < FLIGHT; ++u) a += (double)v[u];
    }
    for (; b < blocks; b += LANES) a += (double)partial[(size_t)b * NSUM + e];
  }
  sh[lane][e] = a;
  __syncthreads();
  for (int w = LANES / 2; w > 0; w >>= 1) {
    if (lane < w) sh[lane][e] += sh[lane + w][e];
    __syncthreads();
  }
  return sh[0];
}

// ---- scalars[1 .. 9], the same in every family, from the sums
//   s: 0 first term (crossentropy) per element  1 p  2 y  3 p*y  4 [p>.5]  5 [p>.5]*y  6 [(p>.5)==y]
//   scalars: 1 first term  2 dice_loss  3 dice (thresholded)  4 accuracy  5 sum_p  6 sum_y  7 sum_py  8 iou (musket iou_coef, smooth 1)
//            9 iot (the same on predictions thresholded at 0.5)
// inv_first / inv_acc: the reciprocal counts of the first term and of the accuracy.  scalars[0] (and [10], [11]) stay with the family: the
// plain families add TWO weighted terms - s[7], s[8] are not sums in their 8-wide rows, and 0 * NaN is not 0.
struct LossTerms { double first, dice_l, iou; };
__device__ __forceinline__ LossTerms loss_common_scalars(const double* s, double inv_first, double inv_acc, float* scalars) {
  LossTerms t;
  t.first = s[0] * inv_first;
  t.dice_l = 1.0 - (2.0 * s[3] + 1.0) / (s[2] + s[1] + 1.0);
  t.iou = (s[3] + 1.0) / (s[2] + s[1] - s[3] + 1.0);
  scalars[1] = (float)t.first;
  scalars[2] = (float)t.dice_l;
  scalars[3] = (float)((2.0 * s[5] + 1.0) / (s[2] + s[4] + 1.0));
  scalars[4] = (float)(s[6] * inv_acc);
  scalars[5] = (float)s[1];
  scalars[6] = (float)s[2];
  scalars[7] = (float)s[3];
  scalars[8] = (float)t.iou;
  scalars[9] = (float)((s[5] + 1.0) / (s[2] + s[4] - s[5] + 1.0));
  return t;
}
// scalars[0], [10], [11] of the families with the whole registry (16-wide rows: s[7] jaccard per pixel, s[8] focal per element)
__device__ __forceinline__ void loss_ex_scalars(const double* s, const LossTerms& t, const LossWeights& lw, double inv_jaccard, double inv_focal,
                                                float* scalars) {
  const double jac = s[7] * inv_jaccard, focal = s[8] * inv_focal;
  scalars[0] = (float)(lw.w[0] * t.first + lw.w[1] * t.dice_l + lw.w[2] * (1.0 - t.iou) + lw.w[3] * jac + lw.w[4] * focal);
  scalars[10] = (float)jac;
  scalars[11] = (float)focal;
}

// ---- gradient-pass preamble: the constants of d dice_loss / dp = -(2 y den - num) / den^2 and d iou / dp = (y uden - unum (1 - y)) / uden^2
struct DiceIouGrad {
  float den, num, inv_den2, uden, unum, inv_uden2;
  __device__ __forceinline__ explicit DiceIouGrad(const float* scalars) {
    const float sp = scalars[5], sy = scalars[6], spy = scalars[7];
    den = sy + sp + 1.f;
    inv_den2 = 1.f / (den * den);
    num = 2.f * spy + 1.f;
    uden = sy + sp - spy + 1.f;      // iou_coef = unum / uden
    unum = spy + 1.f;
    inv_uden2 = 1.f / (uden * uden);
  }
};

// ---- host side
static inline int loss_value_blocks(int64_t count, int per_block = 1024) {
  const int64_t b = count / per_block;
  return (int)(b < 1 ? 1 : b > LOSS_MAX_BLOCKS ? LOSS_MAX_BLOCKS : b);
}
// one thread per item up to `cap` workgroups (2048 multi-label / 4096 sigmoid, extended softmax / 16384 softmax, probabilities), a grid stride beyond
static inline int loss_grad_blocks(int64_t count, int cap) {
  const int64_t g = (count + 255) / 256;
  return (int)(g > cap ? cap : g);
}
static inline LossWeights loss_weights(const float* weights5) {
  LossWeights lw;
  for (int i = 0; i < 5; ++i) lw.w[i] = weights5[i];
  return lw;
}
// the argument checks every entry point starts with: the dtype first (the other build's 16-bit code, or garbage), then the entry's own
// conditions, then the workspace
static inline int loss_check(int32_t dtype, bool args_ok, size_t workspace_bytes, size_t workspace_need) {
  if (!stp_dtype_ok(dtype) || !args_ok) return STP_E_BADARG;
  return workspace_bytes < workspace_need ? STP_E_WORKSPACE : STP_OK;
}
// f(T{}) with T = the storage type of a checked dtype: loss_by_dtype(dtype, [&](auto tag) { using T = decltype(tag); ... })
template <typename F> static inline void loss_by_dtype(int32_t dtype, F&& f) {
  if (dtype == STP_H16) f(bf16_t{});
  else f(float{});
}
// the compile-time bound of the unrolled class loops
static inline int loss_class_bucket(int classes) { return classes <= 4 ? 4 : classes <= 8 ? 8 : classes <= 16 ? 16 : classes <= 24 ? 24 : 32; }
// f(std::integral_constant<int, CM>) for the bucket of `classes`
template <typename F> static inline void loss_by_class_bucket(int classes, F&& f) {
  switch (loss_class_bucket(classes)) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 24: f(std::integral_constant<int, 24>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}
