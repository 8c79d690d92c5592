// The 2x changes of resolution whose gradients can complete a BatchNormalization backward: the 2x scatter of a stride-2 shortcut's
// gradient and the gradient of UpSampling2D(2), each with its _bn form, and FPN's upsample-and-add.
#include "stream_ops.h"

// ------------------------------------------------------------------------------------------
// Data gradient of a 1x1 / stride-2 convolution (the projection shortcut of a bottleneck ResNet's first unit), second half: the GEMM
// t = W^T dY runs at LOW resolution ([N, Ho, Wo, C], a plain 1x1 / stride-1 launch); this pass puts t[n, a, b] at (2a, 2b) of the
// [N, H, W, C] gradient - zeros elsewhere, or on top of what the tensor's other consumers wrote (accumulate) - and, when it completes the
// gradient of a BatchNormalization(+activation) output, masks it and reduces the backward sums (bnb_mask_store / bnb_reduce, as the
// max-pool gather of pool.hip).  The zero-inserted form it replaces ran the GEMM over all four parity classes of the high-resolution grid:
// 229 us for 256 <- 512 channels at 4 x 256 x 256 (FPN/ResNet50), 3.4 x its memory floor.
template <typename T, int V, bool BNB>
__global__ __launch_bounds__(256) void scatter2x_bwd_kernel(const T* __restrict__ t, T* __restrict__ dx, int N, int H, int W, int C, int Ho, int Wo,
                                                            int accumulate, BnBack bnb, float* __restrict__ partial) {
  const int cg = C / V;
  const int tt = blockIdx.x * 256 + threadIdx.x;
  const bool on = tt < W * cg;
  if (!BNB && !on) return;
  const int w = on ? tt / cg : 0, c = on ? (tt - w * cg) * V : 0;
  constexpr int ROWS = BNB ? BNB_ROWS : POOL_ROWS;
  constexpr int RB = 4;                                 // rows requested together: one memory round trip per RB rows, not per row
  static_assert(ROWS % RB == 0, "row batches");
  float sg[V], sq[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { sg[e] = 0.f; sq[e] = 0.f; }
  BnBackCh kc[V / 4];
  if constexpr (BNB) {
#pragma unroll
    for (int q = 0; q < V / 4; ++q) kc[q] = bnback_load(bnb, c + 4 * q);
  }
  const bool wev = !(w & 1) && (w >> 1) < Wo;
  for (int r0 = 0; r0 < ROWS; r0 += RB) {
    float g[RB][V], o[RB][V], xv[RB][V];
    bool live[RB];
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      const int row = blockIdx.y * ROWS + r0 + j;
      live[j] = on && row < N * H;
      const int n = live[j] ? row / H : 0, h = live[j] ? row - n * H : 0;
      const size_t oo = (((size_t)n * H + h) * W + w) * C + c;
      const bool hit = live[j] && wev && !(h & 1) && (h >> 1) < Ho;
      if (!BNB && accumulate && !hit) live[j] = false;   // nothing to add there, nothing to mask: the position keeps what it holds
#pragma unroll
      for (int e = 0; e < V; ++e) g[j][e] = o[j][e] = xv[j][e] = 0.f;
      if (hit) ldv<T, V>(t + (((size_t)n * Ho + (h >> 1)) * Wo + (w >> 1)) * C + c, g[j]);
      if (live[j] && accumulate) ldv<T, V>(dx + oo, o[j]);
      if (BNB && live[j]) ldv<T, V>(reinterpret_cast<const T*>(bnb.x) + oo, xv[j]);
    }
#pragma unroll
    for (int j = 0; j < RB; ++j) {
      if (!live[j]) continue;
      const int row = blockIdx.y * ROWS + r0 + j;
      const int n = row / H, h = row - n * H;
      const size_t oo = (((size_t)n * H + h) * W + w) * C + c;
#pragma unroll
      for (int e = 0; e < V; ++e) g[j][e] += o[j][e];
      if constexpr (BNB) {
#pragma unroll
        for (int q = 0; q < V / 4; ++q) {
          const f32x4 st = stored4(f32x4{g[j][4 * q], g[j][4 * q + 1], g[j][4 * q + 2], g[j][4 * q + 3]}, (const T*)nullptr);
          f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
          const f32x4 m = bnback_apply(kc[q], bnb.relu, f32x4{xv[j][4 * q], xv[j][4 * q + 1], xv[j][4 * q + 2], xv[j][4 * q + 3]}, st, s4, q4);
#pragma unroll
          for (int e = 0; e < 4; ++e) { g[j][4 * q + e] = m[e]; sg[4 * q + e] += s4[e]; sq[4 * q + e] += q4[e]; }
        }
      }
      stv<T, V>(dx + oo, g[j]);
    }
  }
  if constexpr (BNB) bnb_reduce<V>(sg, sq, cg, C, partial);
}

static int scatter2x_bwd_launch(const void* t, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t accumulate,
                                const BnBack* bnb, float* partial, hipStream_t s) {
  if (!t || !dx || (C & 3) || N <= 0 || H <= 0 || W <= 0) return STP_E_BADARG;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  if ((int64_t)N * H > 65535 * (int64_t)(bnb ? BNB_ROWS : POOL_ROWS)) return STP_E_BADARG;      // gridDim.y
  const bool v8 = dtype == STP_H16 && (C & 7) == 0;
  const int vec = v8 ? 8 : 4;
  if (bnb) {
    if (!bnb_channels_ok(C, vec) || !partial) return STP_E_BADARG;
    return launch_tv(dtype, v8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((scatter2x_bwd_kernel<T, V, true>), bnb_grid(N, H, W, C, V), dim3(256), bnb_lds(V), s, (const T*)t, (T*)dx, N, H, W, C, Ho, Wo,
                         accumulate, *bnb, partial);
    });
  }
  const dim3 grid(ceil_div(W * (C / vec), 256), ceil_div(N * H, POOL_ROWS));
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((scatter2x_bwd_kernel<T, V, false>), grid, dim3(256), 0, s, (const T*)t, (T*)dx, N, H, W, C, Ho, Wo, accumulate, bnback_none(),
                       nullptr);
  });
}

// t: [N, (H - 1) / 2 + 1, (W - 1) / 2 + 1, C]; dx: [N, H, W, C].  accumulate != 0: dx += the scattered t (odd positions untouched).
extern "C" int stp_scatter2x_bwd(const void* t, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t accumulate, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  return scatter2x_bwd_launch(t, dx, N, H, W, C, dtype, accumulate, nullptr, nullptr, (hipStream_t)stream);
}

// columns of the [2][C][tiles] partial table of stp_scatter2x_bwd_bn (H, W = the HIGH-resolution size); 0 = unsupported C
extern "C" int stp_scatter2x_bwd_bn_tiles(int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  return bnb_tiles(N, H, W, C, (dtype == STP_H16 && (C & 7) == 0) ? 8 : 4);
}

// ... and the completed gradient masked with the activation of the BatchNormalization whose output the tensor is (bn_x: its input),
// stored in place of dY, sum g / sum g * xhat reduced into partial[2][C][tiles] for stp_bn_backward_fused
extern "C" int stp_scatter2x_bwd_bn(const void* t, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, int32_t accumulate,
                                    const void* bn_x, const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t relu,
                                    float* partial, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  BnBack b;
  if (!bnback_fill(&b, bn_x, mean, rstd, gamma, beta, relu, partial)) return STP_E_BADARG;
  return scatter2x_bwd_launch(t, dx, N, H, W, C, dtype, accumulate, &b, partial, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// gradient of UpSampling2D(2): dy is [N,2H,2W,ldy] (first C channels used), dx [N,H,W,C].
// BNB: dx is the gradient of a BatchNormalization(+activation) output that this launch completes - the value is masked with the
// activation re-derived from the BN input x and the workgroup writes its partial sums of g and g * xhat ([2][C][workgroups],
// the layout stp_bn_backward_fused reduces), exactly as the convolution epilogues do (stp_conv_params.bnb_x).
template <typename T, int V, bool BNB>
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W,
                                                             int C, int ldy, int accumulate, BnBack bnb, float* __restrict__ partial) {
  const int cg = C / V;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const bool on = t < W * cg;
  if (!BNB && !on) return;
  const int w = on ? t / cg : 0, c = on ? (t - w * cg) * V : 0;
  constexpr int ROWS = BNB ? BNB_ROWS : 1;
  float sg[V], sq[V];
#pragma unroll
  for (int e = 0; e < V; ++e) { sg[e] = 0.f; sq[e] = 0.f; }
  for (int rr = 0; rr < ROWS; ++rr) {
    const int row = blockIdx.y * ROWS + rr;
    if (row >= N * H || !on) break;
    const int n = row / H, h = row - n * H;
    const size_t o = (((size_t)n * H + h) * W + w) * C + c;
    const T* b = dy + (((size_t)n * 2 * H + 2 * h) * 2 * W + 2 * w) * ldy + c;
    float g[V], a1[V], a2[V], a3[V];
    ldv<T, V>(b, g);
    ldv<T, V>(b + ldy, a1);
    ldv<T, V>(b + (size_t)2 * W * ldy, a2);
    ldv<T, V>(b + (size_t)2 * W * ldy + ldy, a3);
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] = ((g[e] + a1[e]) + a2[e]) + a3[e];
    if (accumulate) {
      float p[V];
      ldv<T, V>(dx + o, p);
#pragma unroll
      for (int e = 0; e < V; ++e) g[e] += p[e];
    }
    if constexpr (BNB) bnb_mask_store<T, V>(g, o, c, bnb, dx, sg, sq);
    else stv<T, V>(dx + o, g);
  }
  if constexpr (BNB) bnb_reduce<V>(sg, sq, cg, C, partial);
}

static int upsample2x_bwd_launch(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldy, int32_t dtype,
                                 int32_t accumulate, const BnBack* bnb, float* partial, hipStream_t s) {
  if (!dy || !dx || (C & 3) || (ldy & 3) || ldy < C || (int64_t)N * H > 65535) return STP_E_BADARG;
  const bool v8 = dtype == STP_H16 && (C & 7) == 0 && (ldy & 7) == 0;
  const int vec = v8 ? 8 : 4;
  if (bnb) {
    if (!bnb_channels_ok(C, vec) || !partial) return STP_E_BADARG;
    return launch_tv(dtype, v8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((upsample2x_bwd_kernel<T, V, true>), bnb_grid(N, H, W, C, V), dim3(256), bnb_lds(V), s, (const T*)dy, (T*)dx, N, H, W, C, ldy,
                         accumulate, *bnb, partial);
    });
  }
  const dim3 grid(ceil_div(W * (C / vec), 256), N * H);
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((upsample2x_bwd_kernel<T, V, false>), grid, dim3(256), 0, s, (const T*)dy, (T*)dx, N, H, W, C, ldy, accumulate, bnback_none(),
                       nullptr);
  });
}

extern "C" int stp_upsample2x_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldy,
                                  int32_t dtype, int32_t accumulate, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  return upsample2x_bwd_launch(dy, dx, N, H, W, C, ldy, dtype, accumulate, nullptr, nullptr, (hipStream_t)stream);
}

// number of workgroups (= partial-sum tiles per channel) of stp_upsample2x_bwd_bn
extern "C" int stp_upsample2x_bwd_bn_tiles(int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldy, int32_t dtype) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  const bool v8 = dtype == STP_H16 && (C & 7) == 0 && (ldy & 7) == 0;
  return bnb_tiles(N, H, W, C, v8 ? 8 : 4);          // 0: not supported for this channel count
}

extern "C" int stp_upsample2x_bwd_bn(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t ldy, int32_t dtype,
                                     int32_t accumulate, const void* bn_x, const float* mean, const float* rstd, const float* gamma,
                                     const float* beta, int32_t relu, float* partial, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  BnBack b;
  if (!bnback_fill(&b, bn_x, mean, rstd, gamma, beta, relu, partial)) return STP_E_BADARG;
  return upsample2x_bwd_launch(dy, dx, N, H, W, C, ldy, dtype, accumulate, &b, partial, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// FPN's top-down step: x[n,2h+i,2w+j,c] += m[n,h,w,c]: Add()([lateral, UpSampling2D(2)(m)]) in place on the lateral tensor.
template <typename T, int V>
__global__ __launch_bounds__(256) void upsample2x_add_kernel(T* __restrict__ x, const T* __restrict__ m, int N, int H, int W, int C) {
  const int cg = C / V;                       // H, W: size of x (even)
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= W * cg) return;
  const int w = t / cg, c = (t - w * cg) * V;
  const int n = blockIdx.y / H, h = blockIdx.y - n * H;
  float a[V], b[V];
  T* px = x + (((size_t)n * H + h) * W + w) * C + c;
  ldv<T, V>(px, a);
  ldv<T, V>(m + (((size_t)n * (H >> 1) + (h >> 1)) * (W >> 1) + (w >> 1)) * C + c, b);
#pragma unroll
  for (int e = 0; e < V; ++e) a[e] += b[e];
  stv<T, V>(px, a);
}

extern "C" int stp_upsample2x_add(void* x, const void* m, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !m || (C & 3) || N <= 0 || (H & 1) || (W & 1) || (int64_t)N * H > 65535) return STP_E_BADARG;
  hipStream_t s = (hipStream_t)stream;
  const bool v8 = dtype == STP_H16 && (C & 7) == 0;
  const dim3 grid(ceil_div(W * (C / (v8 ? 8 : 4)), 256), N * H);
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((upsample2x_add_kernel<T, V>), grid, dim3(256), 0, s, (T*)x, (const T*)m, N, H, W, C);
  });
}
