// Pooling: the stem's 3x3 / stride-2 max pooling (forward, gradient, gradient completing a BatchNormalization backward, and the
// forward fused with the BatchNormalization apply before it), 2x2 and k x k max pooling, average pooling and PSPNet's pooling pyramid.
#include "stream_ops.h"
#include <algorithm>
#include <cstdlib>

// ------------------------------------------------------------------------------------------
// ZeroPadding2D(1) + MaxPooling2D(3, 2, valid).  idx[n,ho,wo,c] = kh*3+kw of the first maximum
// (padded taps take part with value 0, as in the Keras graph).
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx,
                                                          int N, int H, int W, int C, int Ho, int Wo) {
  const int cg = C / V;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Wo * cg) return;
  const int wo = t / cg, c = (t - wo * cg) * V;
  for (int rr = 0; rr < POOL_ROWS; ++rr) {
  const int orow = blockIdx.y * POOL_ROWS + rr;
  if (orow >= N * Ho) break;
  const int n = orow / Ho, ho = orow - n * Ho;
  float best[V];
  uint8_t bi[V];
  // all nine taps are fetched BEFORE the first comparison (clamped addresses, out-of-image taps replaced by 0 afterwards): one
  // memory round trip per thread instead of nine dependent ones (the predicated form waited for every tap before the next)
  float v[9][V];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int h = min(max(2 * ho - 1 + kh, 0), H - 1), w = min(max(2 * wo - 1 + kw, 0), W - 1);
      ldv<T, V>(x + (((size_t)n * H + h) * W + w) * C + c, v[kh * 3 + kw]);
    }
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int h = 2 * ho - 1 + kh, w = 2 * wo - 1 + kw;
      const bool in = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;      // padded taps take part with value 0
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float tv = in ? v[kh * 3 + kw][e] : 0.f;
        if ((kh | kw) == 0 || tv > best[e]) { best[e] = tv; bi[e] = (uint8_t)(kh * 3 + kw); }
      }
    }
  const size_t o = (((size_t)n * Ho + ho) * Wo + wo) * C + c;
  stv<T, V>(y + o, best);
  if (idx) {
    if constexpr (V == 8) *reinterpret_cast<uint2*>(idx + o) = *reinterpret_cast<const uint2*>(bi);
    else *reinterpret_cast<uint32_t*>(idx + o) = *reinterpret_cast<const uint32_t*>(bi);
  }
  }
}

// BatchNormalization apply (+ activation) FUSED with the max-pooling that follows it (round 5: the stem's bn0 -> relu0 -> pooling0).
// The thread of pooled pixel (ho, wo) fetches the nine taps of the PRE-normalisation tensor, normalises them with the arithmetic and
// the rounding of stp_bn_apply (the maximum is taken over the values AS STORED), writes the pooled value + index, and stores the
// normalised tensor for the 2 x 2 block of input pixels (2ho, 2wo) .. (2ho + 1, 2wo + 1) - its taps (1..2, 1..2): every input pixel
// of an even-sized map belongs to exactly one block.  One read of the 134 MB tensor instead of two (apply: read + write, pool: read).
__global__ __launch_bounds__(256) void bn_apply_maxpool_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ yb, bf16_t* __restrict__ y,
                                                               uint8_t* __restrict__ idx, int N, int H, int W, int C, int Ho, int Wo,
                                                               const float* mean, const float* rstd, const float* gamma, const float* beta, int relu) {
  const int cg = C >> 3;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Wo * cg) return;
  const int wo = t / cg, c = (t - wo * cg) * 8;
  float sc[8], sh[8];
  {
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(mean + c), m1 = *reinterpret_cast<const f32x4*>(mean + c + 4);
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(rstd + c), r1 = *reinterpret_cast<const f32x4*>(rstd + c + 4);
    f32x4 g0 = {1.f, 1.f, 1.f, 1.f}, g1 = g0, b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (gamma) { g0 = *reinterpret_cast<const f32x4*>(gamma + c); g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4); }
    if (beta) { b0 = *reinterpret_cast<const f32x4*>(beta + c); b1 = *reinterpret_cast<const f32x4*>(beta + c + 4); }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float r = e < 4 ? r0[e & 3] : r1[e & 3], k = gamma ? r * (e < 4 ? g0[e & 3] : g1[e & 3]) : r;
      sc[e] = k;
      sh[e] = (e < 4 ? b0[e & 3] : b1[e & 3]) - (e < 4 ? m0[e & 3] : m1[e & 3]) * k;
    }
  }
  for (int rr = 0; rr < POOL_ROWS; ++rr) {
    const int orow = blockIdx.y * POOL_ROWS + rr;
    if (orow >= N * Ho) break;
    const int n = orow / Ho, ho = orow - n * Ho;
    u32x4 v[9];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int h = min(max(2 * ho - 1 + kh, 0), H - 1), w = min(max(2 * wo - 1 + kw, 0), W - 1);
        v[kh * 3 + kw] = *reinterpret_cast<const u32x4*>(x + (((size_t)n * H + h) * W + w) * C + c);
      }
    float best[8];
    uint8_t bi[8];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const int h = 2 * ho - 1 + kh, w = 2 * wo - 1 + kw;
        const bool in = (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;      // padded taps take part with value 0
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float lo = bn_act(bn_affine(h16lo_to_f32(v[kh * 3 + kw][e]), sc[2 * e], sh[2 * e]), relu);
          const float hi = bn_act(bn_affine(h16hi_to_f32(v[kh * 3 + kw][e]), sc[2 * e + 1], sh[2 * e + 1]), relu);
          o[e] = pack_bf16x2(lo, hi);
          const float tl = in ? h16lo_to_f32(o[e]) : 0.f, th = in ? h16hi_to_f32(o[e]) : 0.f;      // the values as stored
          if ((kh | kw) == 0 || tl > best[2 * e]) { best[2 * e] = tl; bi[2 * e] = (uint8_t)(kh * 3 + kw); }
          if ((kh | kw) == 0 || th > best[2 * e + 1]) { best[2 * e + 1] = th; bi[2 * e + 1] = (uint8_t)(kh * 3 + kw); }
        }
        if (kh >= 1 && kw >= 1 && in) *reinterpret_cast<u32x4*>(yb + (((size_t)n * H + h) * W + w) * C + c) = o;   // this thread's 2 x 2 block
      }
    const size_t oo = (((size_t)n * Ho + ho) * Wo + wo) * C + c;
    *reinterpret_cast<u32x4*>(y + oo) = u32x4{pack_bf16x2(best[0], best[1]), pack_bf16x2(best[2], best[3]), pack_bf16x2(best[4], best[5]),
                                             pack_bf16x2(best[6], best[7])};
    if (idx) *reinterpret_cast<uint2*>(idx + oo) = *reinterpret_cast<const uint2*>(bi);
  }
}
// H, W even, C % 8 == 0, 16-bit storage.  x = the tensor BEFORE the BatchNormalization, yb = the normalised (+ activated) tensor
// [N,H,W,C] (stp_bn_apply's output, bit for bit), y / idx = stp_maxpool3x3s2's outputs for it.
extern "C" int stp_bn_apply_maxpool3x3s2(const void* x, void* yb, void* y, uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype,
                                         const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t relu, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (dtype != STP_H16 || !x || !yb || !y || !mean || !rstd || N <= 0 || (C & 7) || (H & 1) || (W & 1)) return STP_E_BADARG;
  const int Ho = H / 2, Wo = W / 2;
  if ((int64_t)N * Ho > 65535 * POOL_ROWS) return STP_E_BADARG;  // gridDim.y
  const dim3 grid(ceil_div(Wo * (C / 8), 256), ceil_div(N * Ho, POOL_ROWS));
  hipLaunchKernelGGL(bn_apply_maxpool_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (bf16_t*)yb, (bf16_t*)y, idx, N, H, W, C, Ho, Wo,
                     mean, rstd, gamma, beta, relu);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// One workgroup row per input row (blockIdx.y = n*H + h): 32-bit index arithmetic only, V channels per thread
// (16 bytes of bf16), each input pixel gathers from the <= 4 windows that contain it.
template <typename T, int V, bool BNB>
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const uint8_t* __restrict__ idx, const T* __restrict__ dy,
                                                          T* __restrict__ dx, int N, int H, int W, int C, int Ho, int Wo,
                                                          int accumulate, BnBack bnb, float* __restrict__ partial) {
  const int cg = C / V;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool on = t < W * cg;
  if (!BNB && !on) return;
  const int w = on ? t / cg : 0, c = on ? (t - w * cg) * V : 0;
  constexpr int ROWS = BNB ? BNB_ROWS : POOL_ROWS;
  float sg[V], sq[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { sg[e] = 0.f; sq[e] = 0.f; }
  for (int rr = 0; rr < ROWS; ++rr) {
    const int row = blockIdx.y * ROWS + rr;
    if (row >= N * H || !on) break;
    const int n = row / H, h = row - n * H;
    float g[V];
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = 0.f;
    const size_t oo = (((size_t)n * H + h) * W + w) * C + c;
    // windows (ho,wo) with 2*ho-1+kh == h  ->  kh = h+1-2*ho in [0,2]: an even row has ONE (kh = 1), an odd row TWO (kh = 0
    // of ho = (h+1)/2 and kh = 2 of ho = (h-1)/2); the same along w.  The <= 4 (index, gradient) pairs are fetched up front
    // with clamped addresses - one memory round trip - and the invalid ones masked afterwards.
    int hos[2], khs[2], wos[2], kws[2];
    bool hv[2], wv[2];
    if (h & 1) { hos[0] = (h + 1) >> 1; khs[0] = 0; hos[1] = (h - 1) >> 1; khs[1] = 2; hv[0] = hos[0] < Ho; hv[1] = true; }
    else { hos[0] = h >> 1; khs[0] = 1; hos[1] = 0; khs[1] = 1; hv[0] = hos[0] < Ho; hv[1] = false; }
    if (w & 1) { wos[0] = (w + 1) >> 1; kws[0] = 0; wos[1] = (w - 1) >> 1; kws[1] = 2; wv[0] = wos[0] < Wo; wv[1] = true; }
    else { wos[0] = w >> 1; kws[0] = 1; wos[1] = 0; kws[1] = 1; wv[0] = wos[0] < Wo; wv[1] = false; }
    uint8_t id[4][V];
    float d[4][V];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const size_t o = (((size_t)n * Ho + min(hos[a], Ho - 1)) * Wo + min(wos[b], Wo - 1)) * C + c;
        if constexpr (V == 8) *reinterpret_cast<uint2*>(id[a * 2 + b]) = *reinterpret_cast<const uint2*>(idx + o);
        else *reinterpret_cast<uint32_t*>(id[a * 2 + b]) = *reinterpret_cast<const uint32_t*>(idx + o);
        ldv<T, V>(dy + o, d[a * 2 + b]);
      }
    // (summation order = the former kh-major / kw-minor walk: kh 0 before kh 2, kw 0 before kw 2)
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const bool ok = hv[a] && wv[b];
        const uint8_t me = (uint8_t)(khs[a] * 3 + kws[b]);
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (ok && id[a * 2 + b][e] == me) g[e] += d[a * 2 + b][e];
      }
    if (accumulate) {
      float o[V];
      ldv<T, V>(dx + oo, o);
#pragma unroll
      for (int e = 0; e < V; ++e) g[e] += o[e];
    }
    if constexpr (BNB) bnb_mask_store<T, V>(g, oo, c, bnb, dx, sg, sq);
    else stv<T, V>(dx + oo, g);
  }
  if constexpr (BNB) bnb_reduce<V>(sg, sq, cg, C, partial);
}

extern "C" int stp_maxpool3x3s2(const void* x, void* y, uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C,
                                int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !y || (C & 3) || N <= 0) return STP_E_BADARG;
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  if ((int64_t)N * Ho > 65535) return STP_E_BADARG;  // gridDim.y
  hipStream_t s = (hipStream_t)stream;
  const bool v8 = dtype == STP_H16 && (C & 7) == 0;
  const dim3 grid(ceil_div(Wo * (C / (v8 ? 8 : 4)), 256), ceil_div(N * Ho, POOL_ROWS));
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((maxpool_fwd_kernel<T, V>), grid, dim3(256), 0, s, (const T*)x, (T*)y, idx, N, H, W, C, Ho, Wo);
  });
}

static int maxpool_bwd_launch(const uint8_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype,
                              int32_t accumulate, const BnBack* bnb, float* partial, hipStream_t s) {
  if (!idx || !dy || !dx || (C & 3) || N <= 0) return STP_E_BADARG;
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  if ((int64_t)N * H > 65535) return STP_E_BADARG;  // gridDim.y
  const bool v8 = dtype == STP_H16 && (C & 7) == 0;
  const int vec = v8 ? 8 : 4;
  if (bnb) {
    if (!bnb_channels_ok(C, vec) || !partial) return STP_E_BADARG;
    return launch_tv(dtype, v8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((maxpool_bwd_kernel<T, V, true>), bnb_grid(N, H, W, C, V), dim3(256), bnb_lds(V), s, idx, (const T*)dy, (T*)dx, N, H, W, C, Ho,
                         Wo, accumulate, *bnb, partial);
    });
  }
  const dim3 grid(ceil_div(W * (C / vec), 256), ceil_div(N * H, POOL_ROWS));
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((maxpool_bwd_kernel<T, V, false>), grid, dim3(256), 0, s, idx, (const T*)dy, (T*)dx, N, H, W, C, Ho, Wo, accumulate, bnback_none(),
                       nullptr);
  });
}

extern "C" int stp_maxpool3x3s2_bwd(const uint8_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                    int32_t dtype, int32_t accumulate, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  return maxpool_bwd_launch(idx, dy, dx, N, H, W, C, dtype, accumulate, nullptr, nullptr, (hipStream_t)stream);
}

// Same tile count rule as stp_upsample2x_bwd_bn_tiles (H, W = the pool INPUT size): workgroups of the launch, 0 = unsupported C.
extern "C" int stp_maxpool3x3s2_bwd_bn_tiles(int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  return bnb_tiles(N, H, W, C, (dtype == STP_H16 && (C & 7) == 0) ? 8 : 4);
}

extern "C" int stp_maxpool3x3s2_bwd_bn(const uint8_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                       int32_t dtype, int32_t accumulate, const void* bn_x, const float* mean, const float* rstd,
                                       const float* gamma, const float* beta, int32_t relu, float* partial, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  BnBack b;
  if (!bnback_fill(&b, bn_x, mean, rstd, gamma, beta, relu, partial)) return STP_E_BADARG;
  return maxpool_bwd_launch(idx, dy, dx, N, H, W, C, dtype, accumulate, &b, partial, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// MaxPooling2D(2, 2) without padding (keras.applications VGG blocks).  idx[n,ho,wo,c] = 2*dy+dx of the first maximum;
// every input pixel belongs to exactly one window, so the gradient is a masked copy.  H and W even.
template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, uint8_t* __restrict__ idx,
                                                           int N, int H, int W, int C) {
  const int cg = C / V, Ho = H >> 1, Wo = W >> 1;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Wo * cg) return;
  const int wo = t / cg, c = (t - wo * cg) * V;
  for (int rr = 0; rr < POOL_ROWS; ++rr) {
  const int orow = blockIdx.y * POOL_ROWS + rr;
  if (orow >= N * Ho) break;
  const int n = orow / Ho, ho = orow - n * Ho;
  float best[V];
  uint8_t bi[V];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float v[V];
    ldv<T, V>(x + (((size_t)n * H + 2 * ho + (k >> 1)) * W + 2 * wo + (k & 1)) * C + c, v);
#pragma unroll
    for (int e = 0; e < V; ++e)
      if (k == 0 || v[e] > best[e]) { best[e] = v[e]; bi[e] = (uint8_t)k; }
  }
  const size_t o = (((size_t)n * Ho + ho) * Wo + wo) * C + c;
  stv<T, V>(y + o, best);
  if (idx) {
    if constexpr (V == 8) *reinterpret_cast<uint2*>(idx + o) = *reinterpret_cast<const uint2*>(bi);
    else *reinterpret_cast<uint32_t*>(idx + o) = *reinterpret_cast<const uint32_t*>(bi);
  }
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const uint8_t* __restrict__ idx, const T* __restrict__ dy, T* __restrict__ dx,
                                                           int N, int H, int W, int C, int accumulate) {
  const int cg = C / V, Ho = H >> 1, Wo = W >> 1;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W * cg) return;
  const int w = t / cg, c = (t - w * cg) * V;
  const int n = blockIdx.y / H, h = blockIdx.y - n * H;
  const size_t o = (((size_t)n * Ho + (h >> 1)) * Wo + (w >> 1)) * C + c;
  uint8_t id[V];
  if constexpr (V == 8) *reinterpret_cast<uint2*>(id) = *reinterpret_cast<const uint2*>(idx + o);
  else *reinterpret_cast<uint32_t*>(id) = *reinterpret_cast<const uint32_t*>(idx + o);
  float d[V], g[V];
  ldv<T, V>(dy + o, d);
  const uint8_t me = (uint8_t)(((h & 1) << 1) | (w & 1));
#pragma unroll
  for (int e = 0; e < V; ++e) g[e] = id[e] == me ? d[e] : 0.f;
  T* out = dx + (((size_t)n * H + h) * W + w) * C + c;
  if (accumulate) {
    float a[V];
    ldv<T, V>(out, a);
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] += a[e];
  }
  stv<T, V>(out, g);
}

extern "C" int stp_maxpool2x2(const void* x, void* y, uint8_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype,
                              void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !y || (C & 3) || N <= 0 || (H & 1) || (W & 1) || (int64_t)N * (H >> 1) > 65535) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const bool v8 = dtype == STP_H16 && (C & 7) == 0;
  const dim3 grid(ceil_div((W >> 1) * (C / (v8 ? 8 : 4)), 256), N * (H >> 1));
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((maxpool2_fwd_kernel<T, V>), grid, dim3(256), 0, s, (const T*)x, (T*)y, idx, N, H, W, C);
  });
}

extern "C" int stp_maxpool2x2_bwd(const uint8_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C,
                                  int32_t dtype, int32_t accumulate, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!idx || !dy || !dx || (C & 3) || N <= 0 || (H & 1) || (W & 1) || (int64_t)N * H > 65535) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const bool v8 = dtype == STP_H16 && (C & 7) == 0;
  const dim3 grid(ceil_div(W * (C / (v8 ? 8 : 4)), 256), N * H);
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((maxpool2_bwd_kernel<T, V>), grid, dim3(256), 0, s, idx, (const T*)dy, (T*)dx, N, H, W, C, accumulate);
  });
}

// ------------------------------------------------------------------------------------------
// AveragePooling2D(pool = strides = k) with H % k == W % k == 0 (PSPNet's pyramid pooling levels) and its gradient
// (every input pixel belongs to exactly one window: dx = dy / k^2).
template <typename T>
__global__ __launch_bounds__(256) void avgpool_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int k) {
  const int Ho = H / k, Wo = W / k;
  const int64_t total = (int64_t)N * Ho * Wo * C;
  const float inv = 1.f / (float)(k * k);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int wo = (int)((i / C) % Wo);
    const int ho = (int)((i / ((int64_t)C * Wo)) % Ho);
    const int n = (int)(i / ((int64_t)C * Wo * Ho));
    const T* b = x + (((int64_t)n * H + (int64_t)ho * k) * W + (int64_t)wo * k) * C + c;
    float acc = 0.f;
    for (int dy = 0; dy < k; ++dy)
      for (int dx = 0; dx < k; ++dx) acc += Elem<T>::load(b + ((int64_t)dy * W + dx) * C);
    Elem<T>::store(y + i, acc * inv);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C, int k,
                                                          int accumulate) {
  const int Ho = H / k, Wo = W / k;
  const int64_t total = (int64_t)N * H * W * C;
  const float inv = 1.f / (float)(k * k);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int w = (int)((i / C) % W);
    const int h = (int)((i / ((int64_t)C * W)) % H);
    const int n = (int)(i / ((int64_t)C * W * H));
    float g = Elem<T>::load(dy + (((int64_t)n * Ho + h / k) * Wo + w / k) * C + c) * inv;
    if (accumulate) g += Elem<T>::load(dx + i);
    Elem<T>::store(dx + i, g);
  }
}

// Large windows (PSPNet: 96x96 .. 16x16 pixels per output): one workgroup per (window, channel chunk).  VL vector lanes x
// PL pixel lanes stride over the window with 16-byte loads; the pixel lanes are combined through LDS in a fixed order.
template <typename T, int V>
__global__ __launch_bounds__(256) void avgpool_win_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C, int k, int VL,
                                                          int rps, float* __restrict__ part) {
  extern __shared__ float red[];  // [PL][VL*V]
  const int PL = 256 / VL;
  const int vl = threadIdx.x % VL, pl = threadIdx.x / VL;
  const int Ho = H / k, Wo = W / k;
  int b = blockIdx.x;
  const int wo = b % Wo; b /= Wo;
  const int ho = b % Ho;
  const int n = b / Ho;
  const int c = (blockIdx.y * VL + vl) * V;
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  if (c < C && pl < PL) {
    const T* base = x + (((int64_t)n * H + (int64_t)ho * k) * W + (int64_t)wo * k) * C + c;
    const int r0 = blockIdx.z * rps, r1 = min(k, r0 + rps);      // window rows of this split (all of them without a workspace)
    for (int p = r0 * k + pl; p < r1 * k; p += PL) {
      const int dy = p / k, dx = p - dy * k;
      float v[V];
      ldv<T, V>(base + ((int64_t)dy * W + dx) * C, v);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += v[e];
    }
  }
  if (pl < PL) {
#pragma unroll
    for (int e = 0; e < V; ++e) red[(pl * VL + vl) * V + e] = acc[e];
  }
  __syncthreads();
  const int t = threadIdx.x, cc = blockIdx.y * VL * V + t;
  if (t < VL * V && cc < C) {
    float sum = 0.f;
    for (int l = 0; l < PL; ++l) sum += red[l * VL * V + t];
    if (part) part[((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * C + cc] = sum;
    else Elem<T>::store(y + (((int64_t)n * Ho + ho) * Wo + wo) * C + cc, sum / (float)(k * k));
  }
}

template <typename T, int V>
__global__ __launch_bounds__(256) void avgpool_bwd_vec_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H, int W, int C, int k,
                                                              int accumulate) {
  const int cg = C / V;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W * cg) return;
  const int w = t / cg, c = (t - w * cg) * V;
  const int n = blockIdx.y / H, h = blockIdx.y - n * H;
  const float inv = 1.f / (float)(k * k);
  float g[V], o[V];
  ldv<T, V>(dy + (((int64_t)n * (H / k) + h / k) * (W / k) + w / k) * C + c, g);
  T* d = dx + (((int64_t)n * H + h) * W + w) * C + c;
#pragma unroll
  for (int e = 0; e < V; ++e) o[e] = g[e] * inv;
  if (accumulate) {
    ldv<T, V>(d, g);
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] += g[e];
  }
  stv<T, V>(d, o);
}

// the argument checks of stp_avgpool and stp_avgpool_bwd (a, b: the two tensors)
static inline bool avgpool_args_ok(const void* a, const void* b, int N, int H, int W, int C, int k, int dtype) {
  return stp_dtype_ok(dtype) && a && b && N > 0 && C > 0 && k >= 1 && !(H % k) && !(W % k);      // (the other build's 16-bit code, or garbage)
}

extern "C" size_t stp_avgpool_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k) {
  if (N <= 0 || C <= 0 || k < 1 || H % k || W % k) return 0;
  return split_bytes_either_width((int64_t)N * (H / k) * (W / k), C, k);
}

extern "C" int stp_avgpool(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t dtype, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (!avgpool_args_ok(x, y, N, H, W, C, k, dtype)) return STP_E_BADARG;
  const int V = vec_for(dtype, C, 0, 0);
  if (V > 1 && k * k >= 32) {
    const int cg = C / V, VL = pool_vl(cg);
    const int64_t nwin = (int64_t)N * (H / k) * (W / k);
    const SplitPlan sp = split_plan_fit(split_plan(nwin, C, cg, VL, k), k, workspace, workspace_bytes);
    const int rps = sp.rps, S = sp.S;
    float* part = S > 1 ? (float*)workspace : nullptr;
    const dim3 grid((unsigned)nwin, ceil_div(cg, VL), S);
    const size_t lds = (size_t)(256 / VL) * VL * V * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const int rc = launch_tv(dtype, V == 8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((avgpool_win_kernel<T, V>), grid, dim3(256), lds, s, (const T*)x, (T*)y, H, W, C, k, VL, rps, part);
    });
    if (rc || S <= 1) return rc;
    return split_combine_launch(part, S, nwin * C, 1.f / (float)(k * k), y, dtype, 0, s);
  }
  const int g = grid_for((int64_t)N * (H / k) * (W / k) * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(avgpool_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, N, H, W, C, k);
  });
}

extern "C" int stp_avgpool_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t dtype,
                               int32_t accumulate, void* stream) {
  if (!avgpool_args_ok(dy, dx, N, H, W, C, k, dtype)) return STP_E_BADARG;
  const int V = vec_for(dtype, C, 0, 0);
  if (V > 1 && (int64_t)N * H <= 65535) {
    const dim3 grid(ceil_div(W * (C / V), 256), N * H);
    hipStream_t s = (hipStream_t)stream;
    return launch_tv(dtype, V == 8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((avgpool_bwd_vec_kernel<T, V>), grid, dim3(256), 0, s, (const T*)dy, (T*)dx, H, W, C, k, accumulate);
    });
  }
  const int g = grid_for((int64_t)N * H * W * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(avgpool_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (T*)dx, N, H, W, C, k, accumulate);
  });
}

// ---- PSPNet's pyramid pooling in ONE pass over the feature map (round 6).  AveragePooling2D at the four pyramid levels (windows 96 / 48 / 32 /
// 16 pixels at 8 x 96 x 96 x 512) read the same 75 MB four times (4 x 20 us) and their gradients rewrite its gradient four times (108 us).
// Every coarser window is a union of windows of the finest level, so: the fp32 sums of the FINEST windows (avgpool_win_kernel with its
// partial-sum table), then one small launch that forms every level's mean from those sums in a fixed order (one rounding per output, as
// the separate launches); backward: one pass over the feature gradient that adds the <= 4 levels' dY / k^2 of its pixel.
struct PoolPyr { void* y[4]; int k[4]; int64_t first[5]; int64_t nwin; int levels; };
template <typename T>
__global__ __launch_bounds__(256) void avgpool_pyramid_combine_kernel(const float* __restrict__ part, int S, PoolPyr p, int H, int W, int C) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.first[p.levels]) return;
  int L = 0;
#pragma unroll
  for (int q = 1; q < 4; ++q) if (q < p.levels && i >= p.first[q]) L = q;
  const int64_t j = i - p.first[L];
  const int k0 = p.k[0], k = p.k[L], r = k / k0, Ho = H / k, Wo = W / k, H0 = H / k0, W0 = W / k0;
  const int c = (int)(j % C);
  int64_t b = j / C;
  const int wo = (int)(b % Wo); b /= Wo;
  const int ho = (int)(b % Ho);
  const int64_t n = b / Ho;
  float sum = 0.f;
  for (int a = 0; a < r; ++a)
    for (int d = 0; d < r; ++d) {
      const int64_t win = (n * H0 + (int64_t)ho * r + a) * W0 + (int64_t)wo * r + d;
      for (int q = 0; q < S; ++q) sum += part[((int64_t)q * p.nwin + win) * C + c];
    }
  Elem<T>::store((T*)p.y[L] + j, sum / (float)(k * k));
}

struct PoolPyrB { const void* dy[4]; int k[4]; float inv[4]; int levels; };
template <typename T, int V>
__global__ __launch_bounds__(256) void avgpool_pyramid_bwd_kernel(PoolPyrB p, T* __restrict__ dx, int H, int W, int C, int accumulate) {
  const int cg = C / V;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W * cg) return;
  const int w = t / cg, c = (t - w * cg) * V;
  const int n = blockIdx.y / H, h = blockIdx.y - n * H;
  float o[V], g[V];
#pragma unroll
  for (int e = 0; e < V; ++e) o[e] = 0.f;
#pragma unroll
  for (int L = 0; L < 4; ++L) {
    if (L < p.levels) {
      const int k = p.k[L];
      ldv<T, V>((const T*)p.dy[L] + (((int64_t)n * (H / k) + h / k) * (W / k) + w / k) * C + c, g);
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] += g[e] * p.inv[L];
    }
  }
  T* d = dx + (((int64_t)n * H + h) * W + w) * C + c;
  if (accumulate) {
    ldv<T, V>(d, g);
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] += g[e];
  }
  stv<T, V>(d, o);
}

static int pool_pyramid_levels(const int* k) {
  int levels = 0;
  while (levels < 4 && k[levels] > 0) ++levels;
  return levels;
}
static bool pool_pyramid_ok(int N, int H, int W, int C, const int* k, int levels, int dtype) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || levels < 1 || levels > 4 || (dtype != STP_H16 && dtype != STP_F32)) return false;
  if (vec_for(dtype, C, 0, 0) <= 1 || (int64_t)N * H > 65535) return false;
  for (int i = 0; i < levels; ++i)
    if (k[i] < 1 || H % k[i] || W % k[i] || k[i] % k[0]) return false;
  return k[0] * k[0] >= 32;      // (the window kernel serves the finest level)
}
// 1 if the four AveragePooling2D(k_i) of one tensor can run as a pyramid: k0 = the finest window, every other k a multiple of it (k = 0: level unused)
extern "C" int stp_avgpool_pyramid_ok(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k0, int32_t k1, int32_t k2, int32_t k3, int32_t dtype) {
  const bool on = !(getenv("STP_POOL_PYRAMID") && atoi(getenv("STP_POOL_PYRAMID")) == 0);      // (a plan-time query: read at every call)
  const int k[4] = {k0, k1, k2, k3};
  return on && stp_dtype_ok(dtype) && pool_pyramid_ok(N, H, W, C, k, pool_pyramid_levels(k), dtype) ? 1 : 0;
}
// the split of the finest level's window launch (the table of fp32 sums is always written, also with one split)
static SplitPlan pool_pyramid_split(int N, int H, int W, int C, int k0, int dtype) {
  const int V = vec_for(dtype, C, 0, 0), cg = C / V;
  return split_plan((int64_t)N * (H / k0) * (W / k0), C, cg, pool_vl(cg), k0);
}
extern "C" size_t stp_avgpool_pyramid_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t k0, int32_t dtype) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || k0 < 1 || H % k0 || W % k0 || (dtype != STP_H16 && dtype != STP_F32) || vec_for(dtype, C, 0, 0) <= 1) return 0;
  return pool_pyramid_split(N, H, W, C, k0, dtype).bytes;
}
extern "C" int stp_avgpool_pyramid(const void* x, void* y0, void* y1, void* y2, void* y3, int32_t k0, int32_t k1, int32_t k2, int32_t k3, int32_t N,
                                   int32_t H, int32_t W, int32_t C, int32_t dtype, void* workspace, size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  const int k[4] = {k0, k1, k2, k3};
  void* y[4] = {y0, y1, y2, y3};
  PoolPyr p;
  p.levels = pool_pyramid_levels(k);
  if (!x || !workspace || !pool_pyramid_ok(N, H, W, C, k, p.levels, dtype)) return STP_E_BADARG;
  if (workspace_bytes < stp_avgpool_pyramid_workspace_bytes(N, H, W, C, k0, dtype)) return STP_E_WORKSPACE;
  p.first[0] = 0;
  for (int i = 0; i < 4; ++i) {
    const bool on = i < p.levels;
    if (on && !y[i]) return STP_E_BADARG;
    p.y[i] = on ? y[i] : nullptr;
    p.k[i] = on ? k[i] : 0;
    p.first[i + 1] = p.first[i] + (on ? (int64_t)N * (H / k[i]) * (W / k[i]) * C : 0);
  }
  const int V = vec_for(dtype, C, 0, 0), cg = C / V, VL = pool_vl(cg);
  p.nwin = (int64_t)N * (H / k0) * (W / k0);
  const SplitPlan sp = pool_pyramid_split(N, H, W, C, k0, dtype);
  const int rps = sp.rps, S = sp.S;
  float* part = (float*)workspace;
  const dim3 grid((unsigned)p.nwin, ceil_div(cg, VL), S);
  const size_t lds = (size_t)(256 / VL) * VL * V * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch_tv(dtype, V == 8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((avgpool_win_kernel<T, V>), grid, dim3(256), lds, s, (const T*)x, (T*)nullptr, H, W, C, k0, VL, rps, part);
  });
  if (rc) return rc;
  const unsigned g = (unsigned)ceil_div(p.first[p.levels], (int64_t)256);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(avgpool_pyramid_combine_kernel<T>, dim3(g), dim3(256), 0, s, part, S, p, H, W, C);
  });
}
extern "C" int stp_avgpool_pyramid_bwd(const void* dy0, const void* dy1, const void* dy2, const void* dy3, int32_t k0, int32_t k1, int32_t k2, int32_t k3,
                                       void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t accumulate, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  const int k[4] = {k0, k1, k2, k3};
  const void* dy[4] = {dy0, dy1, dy2, dy3};
  PoolPyrB p;
  p.levels = pool_pyramid_levels(k);
  if (!dx || !pool_pyramid_ok(N, H, W, C, k, p.levels, dtype)) return STP_E_BADARG;
  for (int i = 0; i < 4; ++i) {
    const bool on = i < p.levels;
    if (on && !dy[i]) return STP_E_BADARG;
    p.dy[i] = on ? dy[i] : nullptr;
    p.k[i] = on ? k[i] : 1;
    p.inv[i] = on ? 1.f / (float)(k[i] * k[i]) : 0.f;
  }
  const int V = vec_for(dtype, C, 0, 0);
  const dim3 grid(ceil_div(W * (C / V), 256), N * H);
  hipStream_t s = (hipStream_t)stream;
  return launch_tv(dtype, V == 8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((avgpool_pyramid_bwd_kernel<T, V>), grid, dim3(256), 0, s, p, (T*)dx, H, W, C, accumulate);
  });
}

// ------------------------------------------------------------------------------------------
// MaxPooling2D(pool_size = strides = k) for any k (PSPNet `psp_pooling_type: max`, schemas/segmentation.raml:233-236): one thread
// per (output pixel, channel), channels fastest (coalesced); idx = position kh * k + kw of the FIRST maximum (int32, k up to the
// whole map); the gradient goes to that position only (windows do not overlap: one thread per input element, no atomics)
template <typename T>
__global__ __launch_bounds__(256) void maxpool_k_kernel(const T* __restrict__ x, T* __restrict__ y, int32_t* __restrict__ idx, int N, int H, int W,
                                                        int C, int k) {
  const int Ho = H / k, Wo = W / k;
  const int64_t total = (int64_t)N * Ho * Wo * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int xo = (int)(p % Wo), yo = (int)((p / Wo) % Ho), n = (int)(p / ((int64_t)Wo * Ho));
    const T* b = x + (((int64_t)n * H + yo * k) * W + xo * k) * C + c;
    // the running maximum starts from the window's first element, not from a finite floor: a window of -inf (or of fp32 values below
    // the floor) pools to its own maximum with idx 0, as MaxPooling2D does
    float best = 0.f;
    int bi = 0;
    for (int a = 0; a < k; ++a)
      for (int q = 0; q < k; ++q) {
        const float v = Elem<T>::load(b + ((int64_t)a * W + q) * C);
        if ((a | q) == 0 || v > best) { best = v; bi = a * k + q; }
      }
    Elem<T>::store(y + i, best);
    if (idx) idx[i] = bi;
  }
}
template <typename T>
__global__ __launch_bounds__(256) void maxpool_k_bwd_kernel(const int32_t* __restrict__ idx, const T* __restrict__ dy, T* __restrict__ dx, int N,
                                                            int H, int W, int C, int k, int accumulate) {
  const int Ho = H / k, Wo = W / k;
  const int64_t total = (int64_t)N * H * W * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int xi = (int)(p % W), yi = (int)((p / W) % H), n = (int)(p / ((int64_t)W * H));
    const int64_t o = (((int64_t)n * Ho + yi / k) * Wo + xi / k) * C + c;
    float g = (idx[o] == (yi % k) * k + (xi % k)) ? Elem<T>::load(dy + o) : 0.f;
    if (accumulate) g += Elem<T>::load(dx + i);
    Elem<T>::store(dx + i, g);
  }
}
extern "C" int stp_maxpool_k(const void* x, void* y, int32_t* idx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k, int32_t dtype,
                             void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || k < 1 || H % k || W % k) return STP_E_BADARG;
  const int g = grid_for((int64_t)N * (H / k) * (W / k) * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(maxpool_k_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, idx, N, H, W, C, k);
  });
}
extern "C" int stp_maxpool_k_bwd(const int32_t* idx, const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t k,
                                 int32_t dtype, int32_t accumulate, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!idx || !dy || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || k < 1 || H % k || W % k) return STP_E_BADARG;
  const int g = grid_for((int64_t)N * H * W * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(maxpool_k_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, idx, (const T*)dy, (T*)dx, N, H, W, C, k, accumulate);
  });
}
