// Multi-label sigmoid head: C = 2..8 independent sigmoid channels per pixel (classes: C, activation: sigmoid), the Keras / musket
// losses applied element by element over the whole [pixels][C] tensor (oracle/losses.py on an [N,H,W,C] target):
//   binary_crossentropy  mean over pixels*C elements (Keras TF form, 1e-7 clip)
//   dice_loss / iou      ONE soft dice / iou over the flattened tensor, smooth 1 (musket's definition, not a mean over classes)
//   jaccard_loss         per pixel over the class axis, smooth 100, mean over pixels
//   focal_loss           gamma 2, alpha 0.25, positive and negative terms each a mean over elements
// The target is one byte per pixel, bit c = class c.  Same two-stage fixed-order reduction as stp_sigmoid_loss_ex (one thread per
// pixel, the class loop unrolled to CM = 4 or 8 and predicated, rows read in 16- / 8-byte chunks where the stride allows): value pass
// -> per-workgroup partials -> finalize (12 scalars) -> gradient pass, which leaves one partial sum PER CLASS per workgroup for
// stp_sigmoid_multilabel_bias_grad.  Plain global (not buffer) loads and stores: no register-soffset store hazard (tests/test_isa_multilabel.py).
#include "loss_reduce.h"

#define ML_MAX_CLASSES 8
#define ML_NSUM 16
// gradient-pass workgroups: their 8 per-class sums reuse the value pass's partial area (1024 x 16 floats = 2048 x 8), which the
// finalize launch has consumed before the gradient pass starts (same stream)
#define ML_GRAD_MAX_BLOCKS 2048
#define ML_JACCARD_SMOOTH 100.f
#define ML_FOCAL_ALPHA 0.25f
// Keras clips the probability to [eps, 1 - eps] and goes back to logits: zc = log(pc / (1 - pc)) = clamp(z, -ZMAX, ZMAX) with
// ZMAX = log((1 - eps) / eps), and exp(-|zc|) = max(exp(-|z|), EMIN) with EMIN = eps / (1 - eps)
#define ML_ZMAX 16.11809555f
#define ML_EMIN 1.0000001e-7f

// one row of logits -> p[0 .. CM), zeros beyond `classes`.  CB = bytes per load (16, 8, or 0 = element by element); the host picks a
// CB that divides the row stride and the base alignment, and CB / sizeof(T) <= CM, so every chunk that holds a used channel lies in the row.
template <typename T, int CM, int CB>
__device__ __forceinline__ void ml_row_load(const T* __restrict__ z, int classes, float (&p)[CM]) {
  if constexpr (CB == 0) {
#pragma unroll
    for (int c = 0; c < CM; ++c) p[c] = c < classes ? Elem<T>::load(z + c) : 0.f;
  } else {
    constexpr int E = CB / (int)sizeof(T), NW = CB / 4;
    static_assert(E <= CM && CM % E == 0, "chunk wider than the class bucket");
#pragma unroll
    for (int v = 0; v < CM / E; ++v) {
      uint32_t w[NW];
      if (v * E < classes) {
        if constexpr (NW == 4) {
          const u32x4 r = *reinterpret_cast<const u32x4*>(z + v * E);
          w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
        } else {
          const u32x2 r = *reinterpret_cast<const u32x2*>(z + v * E);
          w[0] = r.x; w[1] = r.y;
        }
      } else {
#pragma unroll
        for (int k = 0; k < NW; ++k) w[k] = 0u;
      }
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        if constexpr (sizeof(T) == 2) {
          p[v * E + 2 * k] = h16lo_to_f32(w[k]);
          p[v * E + 2 * k + 1] = h16hi_to_f32(w[k]);
        } else {
          p[v * E + k] = __uint_as_float(w[k]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) p[c] = c < classes ? p[c] : 0.f;
  }
}

// sigmoid on one v_exp_f32 + one v_rcp_f32 (no IEEE division sequence); e = exp(-|z|) is returned for the softplus below
__device__ __forceinline__ float ml_sigmoid(float z, float* e_out) {
  const float e = __expf(-fabsf(z));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  *e_out = e;
  return z >= 0.f ? r : e * r;
}

// value pass: per-workgroup partials of
//   0 bce_e  1 p  2 y  3 p*y  4 [p>.5]  5 [p>.5]*y  6 [(p>.5)==y]  7 jaccard_pixel  8 focal_e   (9..15 zero)
template <typename T, int CM, int CB>
__global__ __launch_bounds__(256) void ml_partial_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target, int64_t pixels,
                                                         int classes, int ldc, float* __restrict__ partial) {
  float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto pixel = [&](float (&z)[CM], uint32_t bits) __attribute__((always_inline)) {
    float inter = 0.f, tot = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < classes) {
        float e;
        const float y = ((bits >> c) & 1u) ? 1.f : 0.f, pr = ml_sigmoid(z[c], &e);
        // Keras binary_crossentropy on the clipped probability with three hardware transcendentals per element (exp, rcp, log: the
        // pass is VALU-bound otherwise): zc = clamp(z) (see ML_ZMAX), L = log(1 + exp(-|zc|)), log(pc) = min(zc, 0) - L and
        // log(1 - pc) = -max(zc, 0) - L
        const float pc = fminf(fmaxf(pr, 1e-7f), 1.f - 1e-7f);
        const float zc = fminf(fmaxf(z[c], -ML_ZMAX), ML_ZMAX);
        const float L = __logf(1.f + fmaxf(e, ML_EMIN));
        a[0] += fmaxf(zc, 0.f) - zc * y + L;
        a[1] += pr;
        a[2] += y;
        a[3] += pr * y;
        const float t = pr > 0.5f ? 1.f : 0.f;
        a[4] += t;
        a[5] += t * y;
        a[6] += (t == y) ? 1.f : 0.f;
        a[8] += y > 0.5f ? -ML_FOCAL_ALPHA * (1.f - pc) * (1.f - pc) * (fminf(zc, 0.f) - L)
                         : (1.f - ML_FOCAL_ALPHA) * pc * pc * (fmaxf(zc, 0.f) + L);
        inter += pr * y;
        tot += pr + y;
      }
    }
    a[7] += (1.f - __fdividef(inter + ML_JACCARD_SMOOTH, tot - inter + ML_JACCARD_SMOOTH)) * ML_JACCARD_SMOOTH;
  };
  const int64_t per = (pixels + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * per, i1 = i0 + per < pixels ? i0 + per : pixels;
  int64_t i = i0 + threadIdx.x;
  for (; i + 256 < i1; i += 512) {          // two rows in flight per thread
    float p0[CM], p1[CM];
    ml_row_load<T, CM, CB>(logits + i * ldc, classes, p0);
    ml_row_load<T, CM, CB>(logits + (i + 256) * ldc, classes, p1);
    const uint32_t b0 = target[i], b1 = target[i + 256];
    pixel(p0, b0);
    pixel(p1, b1);
  }
  for (; i < i1; i += 256) {
    float p0[CM];
    ml_row_load<T, CM, CB>(logits + i * ldc, classes, p0);
    pixel(p0, target[i]);
  }
  loss_block_sums<ML_NSUM, 9, LOSS_WAVES_PAIRWISE>(a, partial);
}

// the 12 scalars of stp_sigmoid_loss_ex: 0 loss 1 bce 2 dice_loss 3 dice 4 binary_accuracy 5 sum_p 6 sum_y 7 sum_py 8 iou 9 iot
// 10 jaccard_loss 11 focal_loss - element means over pixels * classes, jaccard over pixels
__global__ __launch_bounds__(256) void ml_finalize_kernel(const float* partial, int blocks, double inv_elems, double inv_pixels, LossWeights lw,
                                                          float* scalars) {
  const double* s = loss_finalize_sums<ML_NSUM>(partial, blocks);
  if (threadIdx.x != 0) return;
  loss_ex_scalars(s, loss_common_scalars(s, inv_elems, inv_elems, scalars), lw, inv_pixels, inv_elems, scalars);
}

// gradient pass: dL/dlogit of the `classes` channels x grad_scale into [pixels][dlc] (padding channels 0); one partial sum per class of the
// STORED values per workgroup -> gsum[block][8].  VEC_OUT: dlc is a multiple of 16 bytes (the plan's padded gradient rows) - 16-byte stores.
template <typename T, int CM, int CB, bool VEC_OUT>
__global__ __launch_bounds__(256) void ml_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target, int64_t pixels,
                                                      int classes, int ldc, const float* __restrict__ scalars, LossWeights lw, float inv_elems,
                                                      float inv_pixels, float grad_scale, T* __restrict__ dl, int dlc, float* __restrict__ gsum) {
  constexpr int V = Elem<T>::VEC;
  const DiceIouGrad k(scalars);
  const float den = k.den, inv_den2 = k.inv_den2, num = k.num, uden = k.uden, unum = k.unum, inv_uden2 = k.inv_uden2;
  const bool focal = lw.w[4] != 0.f;
  float acc[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) acc[c] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    float p[CM];
    ml_row_load<T, CM, CB>(logits + i * ldc, classes, p);
    const uint32_t bits = target[i];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      float e;
      p[c] = ml_sigmoid(p[c], &e);
    }
    float inter = 0.f, tot = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const float y = ((bits >> c) & 1u) ? 1.f : 0.f;
      inter += c < classes ? p[c] * y : 0.f;
      tot += c < classes ? p[c] + y : 0.f;
    }
    const float jd = tot - inter + ML_JACCARD_SMOOTH, jn = inter + ML_JACCARD_SMOOTH;
    const float jscale = lw.w[3] * ML_JACCARD_SMOOTH * __builtin_amdgcn_rcpf(jd * jd) * inv_pixels;
    float g[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      const float y = ((bits >> c) & 1u) ? 1.f : 0.f, pr = p[c];
      const bool inr = (pr >= 1e-7f) && (pr <= 1.f - 1e-7f);
      float v = inr ? lw.w[0] * (pr - y) * inv_elems : 0.f;
      // gp = d(loss)/dp of the probability-space terms (dice, iou, jaccard, focal)
      float gp = lw.w[1] * (-(2.f * y * den - num) * inv_den2);
      gp -= lw.w[2] * (y * uden - unum * (1.f - y)) * inv_uden2;
      gp -= jscale * (y * jd - jn * (1.f - y));
      if (focal && inr) {
        const float fg = y > 0.5f ? ML_FOCAL_ALPHA * (2.f * (1.f - pr) * __logf(pr) - (1.f - pr) * (1.f - pr) * __builtin_amdgcn_rcpf(pr))
                                  : -(1.f - ML_FOCAL_ALPHA) * (2.f * pr * __logf(1.f - pr) - pr * pr * __builtin_amdgcn_rcpf(1.f - pr));
        gp += lw.w[4] * fg * inv_elems;
      }
      v += gp * (pr * (1.f - pr));
      g[c] = c < classes ? v * grad_scale : 0.f;
    }
    // round to the storage type once: the stored value is what the bias gradient sums (the weight / data gradients read it)
    if constexpr (sizeof(T) == 2) {
#pragma unroll
      for (int c = 0; c < CM; c += 2) {
        const uint32_t w = pack_bf16x2(g[c], g[c + 1]);
        g[c] = h16lo_to_f32(w);
        g[c + 1] = h16hi_to_f32(w);
      }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) acc[c] += g[c];
    T* o = dl + i * dlc;
    if constexpr (VEC_OUT) {
      // 16-byte rows up to 16 channels (the padded 8 / 16 of the plan), zero vectors beyond the class bucket
#pragma unroll
      for (int v = 0; v < 16 / V; ++v) {
        if (v * V >= dlc) break;
        u32x4 r = {0u, 0u, 0u, 0u};
        if (v * V < CM) {
          if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int c = v * V + 2 * e;
              r[e] = c < CM ? pack_bf16x2(g[c < CM ? c : 0], g[c < CM ? c + 1 : 0]) : 0u;   // (CM is even)
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int c = v * V + e;
              r[e] = c < CM ? __float_as_uint(g[c < CM ? c : 0]) : 0u;
            }
          }
        }
        *reinterpret_cast<u32x4*>(o + v * V) = r;
      }
      for (int c = 16; c < dlc; c += V) *reinterpret_cast<u32x4*>(o + c) = u32x4{0u, 0u, 0u, 0u};
    } else {
#pragma unroll
      for (int c = 0; c < CM; ++c) if (c < classes) Elem<T>::store(o + c, g[c]);
      for (int c = classes; c < dlc; ++c) Elem<T>::store(o + c, 0.f);
    }
  }
  loss_block_sums<ML_MAX_CLASSES, CM, LOSS_WAVES_PAIRWISE, ML_MAX_CLASSES>(acc, gsum);
}

// dbias[c] (+)= sum over the gradient workgroups of gsum[block][c]: 8 classes x 32 strided lanes, then a fixed-shape LDS tree
__global__ __launch_bounds__(256) void ml_bias_grad_kernel(const float* gsum, int blocks, int classes, float* dbias, int accumulate) {
  const double* s = loss_finalize_sums<ML_MAX_CLASSES>(gsum, blocks);
  const int c = threadIdx.x & 7;
  if (threadIdx.x < (unsigned)classes) dbias[c] = accumulate ? dbias[c] + (float)s[c] : (float)s[c];
}

template <typename T, int CM, int CB>
static void ml_launch(const T* logits, const uint8_t* target, int64_t pixels, int classes, int ldc, const LossWeights& lw, float* scalars,
                      T* dl, int dlc, bool vec_out, float grad_scale, float* ws, hipStream_t s) {
  const int blocks = loss_value_blocks(pixels);
  hipLaunchKernelGGL((ml_partial_kernel<T, CM, CB>), dim3(blocks), dim3(256), 0, s, logits, target, pixels, classes, ldc, ws);
  hipLaunchKernelGGL(ml_finalize_kernel, dim3(1), dim3(256), 0, s, ws, blocks, 1.0 / ((double)pixels * classes), 1.0 / (double)pixels, lw,
                     scalars);
  if (!dl) return;
  const int g = loss_grad_blocks(pixels, ML_GRAD_MAX_BLOCKS);
  const float inv_elems = (float)(1.0 / ((double)pixels * classes)), inv_pixels = (float)(1.0 / (double)pixels);
  if (vec_out)
    hipLaunchKernelGGL((ml_grad_kernel<T, CM, CB, true>), dim3(g), dim3(256), 0, s, logits, target, pixels, classes, ldc, scalars, lw,
                       inv_elems, inv_pixels, grad_scale, dl, dlc, ws);
  else
    hipLaunchKernelGGL((ml_grad_kernel<T, CM, CB, false>), dim3(g), dim3(256), 0, s, logits, target, pixels, classes, ldc, scalars, lw,
                       inv_elems, inv_pixels, grad_scale, dl, dlc, ws);
}

// picks the class bucket and the widest row load the stride and the base alignment allow
template <typename T>
static void ml_dispatch(const T* logits, const uint8_t* target, int64_t pixels, int classes, int ldc, const LossWeights& lw, float* scalars,
                        T* dl, int dlc, float grad_scale, float* ws, hipStream_t s) {
  const size_t row = (size_t)ldc * sizeof(T);
  const uintptr_t base = reinterpret_cast<uintptr_t>(logits);
  const bool vec_out = dl && ((size_t)dlc * sizeof(T)) % 16 == 0 && (reinterpret_cast<uintptr_t>(dl) & 15) == 0;
#define ML_GO(CM, CB) ml_launch<T, CM, CB>(logits, target, pixels, classes, ldc, lw, scalars, dl, dlc, vec_out, grad_scale, ws, s)
  if (classes <= 4) {
    if (sizeof(T) == 4 && row % 16 == 0 && (base & 15) == 0) ML_GO(4, sizeof(T) == 4 ? 16 : 8);    // (16 bytes = 8 x 16-bit > CM)
    else if (row % 8 == 0 && (base & 7) == 0) ML_GO(4, 8);
    else ML_GO(4, 0);
  } else {
    if (row % 16 == 0 && (base & 15) == 0) ML_GO(8, 16);
    else if (row % 8 == 0 && (base & 7) == 0) ML_GO(8, 8);
    else ML_GO(8, 0);
  }
#undef ML_GO
}

extern "C" int stp_sigmoid_multilabel_loss(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc,
                                           int32_t dtype, const float* weights5, float* scalars, void* dlogits, int32_t dl_channels,
                                           float grad_scale, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = loss_check(dtype, logits && target && weights5 && scalars && workspace && pixels > 0 && classes >= 2 && classes <= ML_MAX_CLASSES &&
                                       ldc >= classes && dl_channels >= classes,
                            workspace_bytes, stp_loss_workspace_bytes());
  if (rc != STP_OK) return rc;
  const LossWeights lw = loss_weights(weights5);
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    ml_dispatch<T>((const T*)logits, target, pixels, classes, ldc, lw, scalars, (T*)dlogits, dl_channels, grad_scale, (float*)workspace,
                   (hipStream_t)stream);
  });
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_sigmoid_multilabel_bias_grad(const void* workspace, int64_t pixels, int32_t classes, float* dbias, int32_t accumulate,
                                                void* stream) {
  if (!workspace || !dbias || pixels <= 0 || classes < 2 || classes > ML_MAX_CLASSES) return STP_E_BADARG;
  hipLaunchKernelGGL(ml_bias_grad_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, loss_grad_blocks(pixels, ML_GRAD_MAX_BLOCKS), classes,
                     dbias, accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
