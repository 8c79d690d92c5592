// Changes of resolution and their gradients: the 2x scatter of a stride-2 shortcut's gradient and the gradient of UpSampling2D(2)
// (both can complete a BatchNormalization backward), FPN's upsample-and-add, bilinear resize by an integer factor with its family of
// gradient kernels, the sum of resized pyramid levels (PSPNet head) and nearest resize.
#include "stream_ops.h"
#include "launch.h"
#include <algorithm>
#include <cstdlib>

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
// FPN pieces.  (a) x[n,2h+i,2w+j,c] += m[n,h,w,c]: Add()([lateral, UpSampling2D(2)(m)]) in place on the lateral tensor.
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

// (b) tf.image.resize_bilinear(align_corners=False) of TF 1.x (what Keras 2.2.4 K.resize_images(interpolation='bilinear')
// calls) by an integer factor f: src = dst / f, x0 = floor(src), x1 = min(x0 + 1, in - 1), no half-pixel offset.
// The output may be a channel slice of a wider tensor (ldo / coff: Concatenate of the resized pyramid levels); f = 1 copies.
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C,
                                                              int f, int ldo, int coff) {
  const int Ho = H * f, Wo = W * f;
  const int64_t total = (int64_t)N * Ho * Wo * C;
  const float inv = 1.f / (float)f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int xo = (int)((i / C) % Wo);
    const int yo = (int)((i / ((int64_t)C * Wo)) % Ho);
    const int n = (int)(i / ((int64_t)C * Wo * Ho));
    const int x0 = xo / f, y0 = yo / f;
    const float fx = (float)(xo - x0 * f) * inv, fy = (float)(yo - y0 * f) * inv;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const T* b = x + (int64_t)n * H * W * C + c;
    const float v00 = Elem<T>::load(b + ((int64_t)y0 * W + x0) * C), v01 = Elem<T>::load(b + ((int64_t)y0 * W + x1) * C);
    const float v10 = Elem<T>::load(b + ((int64_t)y1 * W + x0) * C), v11 = Elem<T>::load(b + ((int64_t)y1 * W + x1) * C);
    const float top = v00 + (v01 - v00) * fx, bot = v10 + (v11 - v10) * fx;      // TF's lerp order
    Elem<T>::store(y + (((int64_t)n * Ho + yo) * Wo + xo) * ldo + coff + c, top + (bot - top) * fy);
  }
}

// gradient: dx[n,h,w,c] (+)= sum over the outputs that read this input pixel, in a fixed order (deterministic gather)
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W,
                                                                  int C, int f, int ldo, int coff, int accumulate) {
  const int Ho = H * f, Wo = W * f;
  const int64_t total = (int64_t)N * H * W * C;
  const float inv = 1.f / (float)f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int w = (int)((i / C) % W);
    const int h = (int)((i / ((int64_t)C * W)) % H);
    const int n = (int)(i / ((int64_t)C * W * H));
    const T* b = dy + (int64_t)n * Ho * Wo * ldo + coff + c;
    float acc = 0.f;
    // rows yo with y0 == h contribute (1 - fy) [all of it when h is the last row: y1 clamps to h]; rows with y0 == h - 1 contribute fy
    for (int yo = max((h - 1) * f, 0); yo < (h + 1) * f; ++yo) {
      const int y0 = yo / f;
      const float fy = (float)(yo - y0 * f) * inv;
      float wy = 0.f;
      if (y0 == h) wy += 1.f - fy;
      if (min(y0 + 1, H - 1) == h) wy += fy;
      if (wy == 0.f) continue;
      for (int xo = max((w - 1) * f, 0); xo < (w + 1) * f; ++xo) {
        const int x0 = xo / f;
        const float fx = (float)(xo - x0 * f) * inv;
        float wx = 0.f;
        if (x0 == w) wx += 1.f - fx;
        if (min(x0 + 1, W - 1) == w) wx += fx;
        if (wx != 0.f) acc += wy * wx * Elem<T>::load(b + ((int64_t)yo * Wo + xo) * ldo);
      }
    }
    if (accumulate) acc += Elem<T>::load(dx + i);
    Elem<T>::store(dx + i, acc);
  }
}

// 16-byte channel groups: one thread per (output pixel, channel group), the same lerp order as the scalar kernel
template <typename T, int V>
__global__ __launch_bounds__(256) void resize_bilinear_vec_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int C, int f,
                                                                  int ldo, int coff) {
  const int cg = C / V, Ho = H * f, Wo = W * f;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= Wo * cg) return;
  const int xo = t / cg, c = (t - xo * cg) * V;
  const int n = blockIdx.y / Ho, yo = blockIdx.y - n * Ho;
  const float inv = 1.f / (float)f;
  const int x0 = xo / f, y0 = yo / f;
  const float fx = (float)(xo - x0 * f) * inv, fy = (float)(yo - y0 * f) * inv;
  const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
  const T* b = x + (int64_t)n * H * W * C + c;
  float v00[V], v01[V], v10[V], v11[V], o[V];
  ldv<T, V>(b + ((int64_t)y0 * W + x0) * C, v00);
  ldv<T, V>(b + ((int64_t)y0 * W + x1) * C, v01);
  ldv<T, V>(b + ((int64_t)y1 * W + x0) * C, v10);
  ldv<T, V>(b + ((int64_t)y1 * W + x1) * C, v11);
#pragma unroll
  for (int e = 0; e < V; ++e) {
    const float top = v00[e] + (v01[e] - v00[e]) * fx, bot = v10[e] + (v11[e] - v10[e]) * fx;
    o[e] = top + (bot - top) * fy;
  }
  stv<T, V>(y + (((int64_t)n * Ho + yo) * Wo + xo) * ldo + coff + c, o);
}

// gradient, ROW-PAIR TILE form for wide channel slices (round 6: FPN's pyramid levels resized x2 / x4 / x8 into the 512-channel
// concatenation - 67 MB of dY per level; the gather kernel below re-reads every output pixel four times from L2 with a division per tap:
// 84 us per level).  One workgroup = (image, two input rows, WS input columns, CC channels):
//   phase 1 (vertical): the <= 3 f - 1 output rows that touch the two input rows are streamed ONCE; a thread owns <= K (column, 16-byte
//            channel group) items of the tile's <= (WS + 1) f - 1 output columns and keeps two fp32 sums per element (one per input row,
//            row weights are workgroup-uniform) - K independent 16-byte loads per row, no barrier in the loop;
//   phase 2 (horizontal): the sums go to LDS once, then every (input row, input column, 4 channels) item adds its <= 2 f - 1 columns
//            with the column weights, in a fixed order - deterministic.
// Every dY byte is read (3 f - 1) / (2 f) x ((WS + 1) f - 1) / (WS f) ~ 1.6 times (from L2 where neighbouring workgroups overlap).
#define RBT_K 3
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_tile_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H, int W, int C, int f,
                                                                       int ldo, int coff, int accumulate, int WS, int CC) {
  extern __shared__ __attribute__((aligned(16))) float rbt_smem[];      // [2][cols][CC]
  const int HP = (H + 1) >> 1;
  const int n = blockIdx.y / HP, h0 = (blockIdx.y - n * HP) * 2, h1 = h0 + 1;
  const int w0 = blockIdx.x * WS, w1 = min(w0 + WS, W);
  const int c0 = blockIdx.z * CC;
  const int Ho = H * f, Wo = W * f;
  const int xlo = max((w0 - 1) * f + 1, 0), xhi = min(w1 * f, Wo), cols = xhi - xlo;
  const int ylo = max((h0 - 1) * f + 1, 0), yhi = min((h1 + 1) * f, Ho);
  const int cgc = CC >> 3, items = cols * cgc;
  const float inv = 1.f / (float)f;
  float a0[RBT_K][8], a1[RBT_K][8];
  int64_t off[RBT_K];
#pragma unroll
  for (int k = 0; k < RBT_K; ++k) {
#pragma unroll
    for (int e = 0; e < 8; ++e) a0[k][e] = a1[k][e] = 0.f;
    const int it = threadIdx.x + k * 256;
    const int col = it / cgc, cv = it - col * cgc;
    off[k] = it < items ? (int64_t)(xlo + col) * ldo + coff + c0 + cv * 8 : -1;
  }
  const T* base = dy + (int64_t)n * Ho * Wo * ldo;
#pragma unroll 2
  for (int yo = ylo; yo < yhi; ++yo) {
    const int y0 = yo / f, y1 = min(y0 + 1, H - 1);
    const float fy = (float)(yo - y0 * f) * inv;
    const float wa = (y0 == h0 ? 1.f - fy : 0.f) + (y1 == h0 ? fy : 0.f), wb = (y0 == h1 ? 1.f - fy : 0.f) + (y1 == h1 ? fy : 0.f);
    const T* row = base + (int64_t)yo * Wo * ldo;
    u32x4 v[RBT_K];
#pragma unroll
    for (int k = 0; k < RBT_K; ++k)
      if (off[k] >= 0) v[k] = *reinterpret_cast<const u32x4*>(row + off[k]);
#pragma unroll
    for (int k = 0; k < RBT_K; ++k) {
      if (off[k] < 0) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float lo = h16lo_to_f32(v[k][e]), hi = h16hi_to_f32(v[k][e]);
        a0[k][2 * e] += wa * lo; a0[k][2 * e + 1] += wa * hi;
        a1[k][2 * e] += wb * lo; a1[k][2 * e + 1] += wb * hi;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < RBT_K; ++k) {
    const int it = threadIdx.x + k * 256;
    if (it >= items) continue;
    float* d0 = rbt_smem + (size_t)it * 8, *d1 = d0 + (size_t)cols * CC;      // item order = [col][channel group]: the [cols][CC] image
    *reinterpret_cast<f32x4*>(d0) = f32x4{a0[k][0], a0[k][1], a0[k][2], a0[k][3]};
    *reinterpret_cast<f32x4*>(d0 + 4) = f32x4{a0[k][4], a0[k][5], a0[k][6], a0[k][7]};
    *reinterpret_cast<f32x4*>(d1) = f32x4{a1[k][0], a1[k][1], a1[k][2], a1[k][3]};
    *reinterpret_cast<f32x4*>(d1 + 4) = f32x4{a1[k][4], a1[k][5], a1[k][6], a1[k][7]};
  }
  __syncthreads();
  const int c4n = CC >> 2, per_row = (w1 - w0) * c4n;
  for (int idx = threadIdx.x; idx < 2 * per_row; idx += 256) {
    const int r = idx >= per_row ? 1 : 0, rem = idx - r * per_row;
    const int wl = rem / c4n, c4 = rem - wl * c4n, w = w0 + wl;
    const int h = r ? h1 : h0;
    if (h >= H) continue;
    const float* src = rbt_smem + (size_t)r * cols * CC + c4 * 4;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    const int x_lo = max((w - 1) * f + 1, 0), x_hi = min((w + 1) * f, Wo);
    for (int xo = x_lo; xo < x_hi; ++xo) {
      const int x0 = xo / f, x1 = min(x0 + 1, W - 1);
      const float fx = (float)(xo - x0 * f) * inv;
      const float wx = (x0 == w ? 1.f - fx : 0.f) + (x1 == w ? fx : 0.f);
      const f32x4 t = *reinterpret_cast<const f32x4*>(src + (size_t)(xo - xlo) * CC);
      sum.x += wx * t.x; sum.y += wx * t.y; sum.z += wx * t.z; sum.w += wx * t.w;
    }
    T* d = dx + (((int64_t)n * H + h) * W + w) * C + c0 + c4 * 4;
    if (accumulate) {
      const f32x4 o = load4(d);
      sum.x += o.x; sum.y += o.y; sum.z += o.z; sum.w += o.w;
    }
    store4(d, sum);
  }
}

// gradient, one workgroup per (input pixel, channel chunk): the (2f)^2 outputs that may read the pixel are spread over TL tap
// lanes (VL vector lanes each), tap-lane partials are combined through LDS in a fixed order - deterministic, and parallel
// even when a whole 96x96 map is the gradient of a single pooled pixel (PSPNet level 1)
template <typename T, int V>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_blk_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H, int W, int C,
                                                                      int f, int ldo, int coff, int accumulate, int VL, int rps,
                                                                      float* __restrict__ part, int TLp, int PPB, int npix) {
  // 256 threads = PPB input pixels x TLp tap lanes x VL vector lanes (few taps and few channels - the x4 resize of 3-class
  // logits - would leave most of a one-pixel workgroup idle)
  extern __shared__ float red[];  // [PPB][TLp][VL*V]
  const int vl = threadIdx.x % VL, q = threadIdx.x / VL;
  const int pl = q / TLp, tl = q - pl * TLp;
  const int Ho = H * f, Wo = W * f;
  const int pix = blockIdx.x * PPB + pl;
  const bool pon = pl < PPB && pix < npix;
  int b = pon ? pix : 0;
  const int w = b % W; b /= W;
  const int h = b % H;
  const int n = b / H;
  const int c = (blockIdx.y * VL + vl) * V;
  const float inv = 1.f / (float)f;
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  if (c < C && pon) {
    const T* src = dy + (int64_t)n * Ho * Wo * ldo + coff + c;
    const int span = 2 * f;
    const int r0 = blockIdx.z * rps, r1 = min(span, r0 + rps);   // tap rows of this split
    for (int t = r0 * span + tl; t < r1 * span; t += TLp) {
      const int ty = t / span, tx = t - ty * span;
      const int yo = (h - 1) * f + ty, xo = (w - 1) * f + tx;
      if (yo < 0 || xo < 0) continue;
      const int y0 = yo / f, x0 = xo / f;
      const float fy = (float)(yo - y0 * f) * inv, fx = (float)(xo - x0 * f) * inv;
      float wy = 0.f, wx = 0.f;
      if (y0 == h) wy += 1.f - fy;
      if (min(y0 + 1, H - 1) == h) wy += fy;
      if (x0 == w) wx += 1.f - fx;
      if (min(x0 + 1, W - 1) == w) wx += fx;
      const float wgt = wy * wx;
      if (wgt == 0.f) continue;
      float v[V];
      ldv<T, V>(src + ((int64_t)yo * Wo + xo) * ldo, v);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += wgt * v[e];
    }
  }
  if (pl < PPB) {
#pragma unroll
    for (int e = 0; e < V; ++e) red[((pl * TLp + tl) * VL + vl) * V + e] = acc[e];
  }
  __syncthreads();
  const int CW = VL * V;                               // channels of this workgroup's chunk
  for (int t = threadIdx.x; t < PPB * CW; t += 256) {
    const int p2 = t / CW, ch = t - p2 * CW;
    const int cc = blockIdx.y * CW + ch, px = blockIdx.x * PPB + p2;
    if (cc >= C || px >= npix) continue;
    float sum = 0.f;
    for (int l = 0; l < TLp; ++l) sum += red[(p2 * TLp + l) * CW + ch];
    if (part) {
      part[((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * C + cc] = sum;      // (splits: PPB == 1)
    } else {
      T* d = dx + (int64_t)px * C + cc;
      if (accumulate) sum += Elem<T>::load(d);
      Elem<T>::store(d, sum);
    }
  }
}

// gradient, ROW-STREAMING form for the resize of CLASS LOGITS (few channels, x4 / x8: PSPNet's final_interpolation, FPN's last_upsample -
// round 5): one workgroup per input row (n, h).  The <= 2f output rows that touch it are streamed whole through a double-buffered LDS
// row (coalesced 16-byte loads; the row of the next iteration sits in registers while this one is reduced); a thread owns up to two
// (w, 16-byte channel group) items and takes the 2f taps of its item from the staged row in a fixed order - deterministic.  The gather
// kernel below gives such shapes ONE input pixel per workgroup (256 tap lanes, an LDS reduction per 48 output bytes): 224 us for PSPNet's
// x8 gradient (226 MB), 128 us for FPN's x4.
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_rows_kernel(const T* __restrict__ dy, T* __restrict__ dx, int H, int W, int C, int f,
                                                                       int ldo, int coff, int accumulate, int nvec) {
  extern __shared__ __attribute__((aligned(16))) char rb_smem[];
  constexpr int EV = 16 / (int)sizeof(T);
  const int n = blockIdx.x / H, h = blockIdx.x - n * H;
  const int Ho = H * f, Wo = W * f;
  const int rowV = Wo * ldo / EV, rowB = rowV * 16;                   // vectors / bytes of one output row (host: ldo % EV == 0)
  const int yo0 = max((h - 1) * f, 0), yo1 = min((h + 1) * f, Ho);    // output rows that may read input row h
  const float inv = 1.f / (float)f;
  const int cgv = C / EV, nitem = W * cgv;
  float acc[2][EV];
  int iw[2], ic[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
#pragma unroll
    for (int e = 0; e < EV; ++e) acc[k][e] = 0.f;
    const int it = threadIdx.x + k * 256;
    iw[k] = it < nitem ? it / cgv : -1;
    ic[k] = it < nitem ? (it - (it / cgv) * cgv) * EV : 0;
  }
  constexpr int MAXV = 10;                                            // 16-byte vectors of a row per thread (host: nvec <= MAXV)
  u32x4 pre[MAXV];
  auto fetch = [&](int yo) {
    const char* src = reinterpret_cast<const char*>(dy + ((int64_t)(n * Ho + yo) * Wo) * ldo);
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
      const int o = threadIdx.x + v * 256;
      if (v < nvec && o < rowV) pre[v] = *reinterpret_cast<const u32x4*>(src + (size_t)o * 16);
    }
  };
  auto park = [&](int buf) {
#pragma unroll
    for (int v = 0; v < MAXV; ++v) {
      const int o = threadIdx.x + v * 256;
      if (v < nvec && o < rowV) *reinterpret_cast<u32x4*>(rb_smem + buf * rowB + o * 16) = pre[v];
    }
  };
  fetch(yo0);
  int buf = 0;
  for (int yo = yo0; yo < yo1; ++yo) {
    park(buf);
    __syncthreads();                        // row yo is staged; the buffer of row yo - 1 is free
    if (yo + 1 < yo1) fetch(yo + 1);
    const int y0 = yo / f;
    const float fy = (float)(yo - y0 * f) * inv;
    float wy = 0.f;
    if (y0 == h) wy += 1.f - fy;
    if (min(y0 + 1, H - 1) == h) wy += fy;
    if (wy != 0.f) {
      const T* row = reinterpret_cast<const T*>(rb_smem + buf * rowB) + coff;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int w = iw[k];
        if (w < 0) continue;
        float r[EV];
#pragma unroll
        for (int e = 0; e < EV; ++e) r[e] = 0.f;
        for (int tx = 0; tx < 2 * f; ++tx) {
          const int xo = (w - 1) * f + tx;
          if (xo < 0) continue;
          const int x0 = xo / f;
          const float fx = (float)(xo - x0 * f) * inv;
          float wx = 0.f;
          if (x0 == w) wx += 1.f - fx;
          if (min(x0 + 1, W - 1) == w) wx += fx;
          float v[EV];
          ldv<T, EV>(row + xo * ldo + ic[k], v);
#pragma unroll
          for (int e = 0; e < EV; ++e) r[e] += wx * v[e];
        }
#pragma unroll
        for (int e = 0; e < EV; ++e) acc[k][e] += wy * r[e];
      }
    }
    buf ^= 1;
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (iw[k] < 0) continue;
    T* d = dx + ((int64_t)(n * H + h) * W + iw[k]) * C + ic[k];
    if (accumulate) {
      float a[EV];
      ldv<T, EV>(d, a);
#pragma unroll
      for (int e = 0; e < EV; ++e) acc[k][e] += a[e];
    }
    stv<T, EV>(d, acc[k]);
  }
}

// gradient, TINY input maps resized by a large factor (PSPNet's pyramid levels: 1 x 1 ... 6 x 6 maps of 512 channels, factors 96 ... 16,
// written into a slice of the concatenation - round 5): the reduction is separable.  Pass 1, one workgroup per OUTPUT row (n, yo): a
// thread owns one 16-byte channel group and every G-th pixel of the row (a wave reads one pixel's whole channel slice: 1 KB contiguous),
// keeps W <= 8 column accumulators, the G pixel groups meet through LDS in a fixed order -> part[n][yo][w][c] (fp32).  Pass 2: input
// row h sums its <= 2f rows of `part` with the row weights.  Every byte of dY is read once, coalesced; the gather kernel below took 51-80 us
// per level for 75 MB (one scattered 16-byte load per tap, an LDS reduction per input pixel).
#define RBT_MAXW 8
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_tiny_rows_kernel(const T* __restrict__ dy, float* __restrict__ part, int H, int W, int C, int f,
                                                                            int ldo, int coff) {
  extern __shared__ float rbt_red[];                    // [G - 1][W][C]
  constexpr int EV = 16 / (int)sizeof(T);
  const int cgv = C / EV, G = 256 / cgv;                // pixel groups of the workgroup (host: 256 % cgv == 0)
  const int cv = threadIdx.x % cgv, g = threadIdx.x / cgv;
  const int Wo = W * f;
  const int64_t row = blockIdx.x;                       // n * Ho + yo
  const T* src = dy + row * Wo * ldo + coff + cv * EV;
  const float inv = 1.f / (float)f;
  float acc[RBT_MAXW][EV];
#pragma unroll
  for (int w = 0; w < RBT_MAXW; ++w)
#pragma unroll
    for (int e = 0; e < EV; ++e) acc[w][e] = 0.f;
  // four pixels per iteration, their loads issued before the first use (a run-time trip count keeps ONE load in flight otherwise: §3.5a)
  for (int xb = g; xb < Wo; xb += 4 * G) {
    float v[4][EV];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int xo = xb + u * G;
      if (xo < Wo) ldv<T, EV>(src + (int64_t)xo * ldo, v[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int xo = xb + u * G;
      if (xo >= Wo) break;
      const int x0 = xo / f;
      const float fx = (float)(xo - x0 * f) * inv;
      const int x1 = min(x0 + 1, W - 1);
#pragma unroll
      for (int w = 0; w < RBT_MAXW; ++w) {
        float wx = 0.f;
        if (x0 == w) wx += 1.f - fx;
        if (x1 == w) wx += fx;
        if (wx != 0.f) {
#pragma unroll
          for (int e = 0; e < EV; ++e) acc[w][e] += wx * v[u][e];
        }
      }
    }
  }
  if (g > 0) {
#pragma unroll
    for (int w = 0; w < RBT_MAXW; ++w)
      if (w < W)
#pragma unroll
        for (int e = 0; e < EV; ++e) rbt_red[((size_t)(g - 1) * W + w) * C + cv * EV + e] = acc[w][e];
  }
  __syncthreads();
  if (g == 0) {
#pragma unroll
    for (int w = 0; w < RBT_MAXW; ++w) {
      if (w >= W) break;
#pragma unroll
      for (int e = 0; e < EV; ++e) {
        float sum = acc[w][e];
        for (int q = 1; q < G; ++q) sum += rbt_red[((size_t)(q - 1) * W + w) * C + cv * EV + e];
        part[(row * W + w) * C + cv * EV + e] = sum;
      }
    }
  }
}
// pass 2: one WAVE per (n, h, w, 4 channels): its 64 lanes take the <= 2f rows of `part` in slices (all loads in flight), a fixed butterfly
// sums them (an output summed its rows one load at a time in the first version: 192 dependent-latency steps for PSPNet's level 1)
template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_bwd_tiny_cols_kernel(const float* __restrict__ part, T* __restrict__ dx, int N, int H, int W, int C,
                                                                            int f, int accumulate) {
  const int Ho = H * f, c4n = C >> 2;
  const int64_t nvec = (int64_t)N * H * W * c4n;
  const int lane = threadIdx.x & 63;
  const int64_t ov = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (ov >= nvec) return;                                 // (wave-uniform)
  const int c4 = (int)(ov % c4n);
  const int w = (int)((ov / c4n) % W), h = (int)((ov / ((int64_t)c4n * W)) % H), n = (int)(ov / ((int64_t)c4n * W * H));
  const float inv = 1.f / (float)f;
  const int yo0 = max((h - 1) * f, 0), yo1 = min((h + 1) * f, Ho);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int yo = yo0 + lane; yo < yo1; yo += 64) {
    const int y0 = yo / f;
    const float fy = (float)(yo - y0 * f) * inv;
    float wy = 0.f;
    if (y0 == h) wy += 1.f - fy;
    if (min(y0 + 1, H - 1) == h) wy += fy;
    const f32x4 v = *reinterpret_cast<const f32x4*>(part + (((int64_t)n * Ho + yo) * W + w) * C + c4 * 4);
    acc += wy * v;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = wave_sum(acc[e]);
  if (lane == 0) {
    T* d = dx + (((int64_t)n * H + h) * W + w) * C + c4 * 4;
    float o[4] = {acc[0], acc[1], acc[2], acc[3]};
    if (accumulate) {
      float a[4];
      ldv<T, 4>(d, a);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] += a[e];
    }
    stv<T, 4>(d, o);
  }
}
// eligibility + workspace of the two-pass form
static bool resize_bwd_tiny_ok(int N, int H, int W, int C, int factor, int ldo, int coff, int dtype) {
  static const bool on = !(getenv("STP_RESIZE_BWD_TINY") && atoi(getenv("STP_RESIZE_BWD_TINY")) == 0);
  const int ev = dtype == STP_H16 ? 8 : 4;
  if (!on || factor < 8 || W > RBT_MAXW || H > 16 || (C % ev) || (ldo % ev) || (coff % ev)) return false;
  const int cgv = C / ev;
  return cgv >= 1 && cgv <= 256 && (256 % cgv) == 0 && (size_t)(256 / cgv - 1) * W * C * sizeof(float) <= 64 * 1024 && (int64_t)N * H * factor < (1ll << 31);
}

// factor 1 (the level of a concatenation that keeps its resolution: PSPNet's feature map, FPN's stride-4 branch): the gradient is the
// channel slice [coff, coff + C) of dY copied (or added) back - 16-byte vectors, four in flight.  The generic gather kernel ran its 2 x 2
// tap loops with integer divisions and 2-byte loads on it: 244 us for 151 MB (PSPNet 768 x 768 batch 8), 236 us for FPN's (round 5).
template <typename T, int V>
__global__ __launch_bounds__(256) void slice_copy_kernel(const T* __restrict__ dy, T* __restrict__ dx, int64_t pixels, int C, int ldo, int coff, int accumulate) {
  const int cg = C / V;
  const int64_t total = pixels * cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t p = i / cg;
    const int c = (int)(i - p * cg) * V;
    float v[V];
    ldv<T, V>(dy + p * ldo + coff + c, v);
    if (accumulate) {
      float a[V];
      ldv<T, V>(dx + p * C + c, a);
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] += a[e];
    }
    stv<T, V>(dx + p * C + c, v);
  }
}

extern "C" int stp_resize_bilinear(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo,
                                   int32_t coff, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || factor < 1 || ldo < coff + C || coff < 0) return STP_E_BADARG;
  if (dtype != STP_H16 && dtype != STP_F32) return STP_E_BADARG;
  const int V = vec_for(dtype, C, ldo, coff);
  if (V > 1 && (int64_t)N * H * factor <= 65535) {
    const dim3 grid(ceil_div(W * factor * (C / V), 256), N * H * factor);
    hipStream_t s = (hipStream_t)stream;
    return launch_tv(dtype, V == 8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((resize_bilinear_vec_kernel<T, V>), grid, dim3(256), 0, s, (const T*)x, (T*)y, H, W, C, factor, ldo, coff);
    });
  }
  const int g = grid_for((int64_t)N * H * factor * W * factor * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(resize_bilinear_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, N, H, W, C, factor, ldo, coff);
  });
}

// ---- PSPNet head (round 6): Conv2D(1x1) over Concatenate([feature, resized pyramid levels]) = Conv2D(1x1) over the feature with ITS columns
// of the kernel + the sum over the levels of resize(Conv2D(1x1) of the TINY level map with the level's columns) - a 1x1 convolution is a
// per-pixel linear map, so it commutes with the (per-channel, linear) bilinear resize.  The 2560-channel concatenation (377 MB at 8 x 96 x
// 96), its gradient and 80 % of the convolution's FLOP disappear.  This kernel is the sum of the resized level terms: up to four sources
// [N][h_i][w_i][C], h_i * f_i = Ho, one fp32 sum, ONE rounding; same lerp order as resize_bilinear_vec_kernel (TF 1.x, align_corners False).
struct UpSum4 { const void* x[4]; int h[4], w[4], f[4], col0[4]; FastDiv df[4], dcg; int n, cols; };
// One workgroup per OUTPUT ROW (n, yo): the two source rows every level contributes to this row (sum of the widths <= 12 columns x 2 rows x C
// channels, 16-bit: 24 KB for 512 channels) are staged in LDS once, then a thread walks (pixel, 16-byte channel group) items of the row.
// (First form: one thread per output vector with sixteen 16-byte loads from the tiny maps in flight - 128 registers, three waves per SIMD,
//  69-74 us for 75 MB = latency x occupancy, not bytes.)  Same lerp order as resize_bilinear_vec_kernel: along x first (top, bottom), then y.
template <typename T, int V>
__global__ __launch_bounds__(256) void upsample_sum_kernel(const UpSum4 a, T* __restrict__ y, int Ho, int Wo, int C) {
  extern __shared__ __attribute__((aligned(16))) char ups_rows[];          // [2][cols][C] of T
  T* rows = reinterpret_cast<T*>(ups_rows);
  const int cg = C / V;
  const int n = blockIdx.x / Ho, yo = blockIdx.x - n * Ho;                 // (workgroup-uniform)
  float fy[4];
  for (int i = 0; i < a.n; ++i) {
    const int H = a.h[i], W = a.w[i], f = a.f[i];
    const int y0 = (int)fdiv((uint32_t)yo, a.df[i]), y1 = min(y0 + 1, H - 1);
    fy[i] = (float)(yo - y0 * f) * (1.f / (float)f);
    const T* b = reinterpret_cast<const T*>(a.x[i]) + (int64_t)n * H * W * C;
    for (int t = threadIdx.x; t < 2 * W * cg; t += 256) {
      const int r = t / (W * cg), rem = t - r * (W * cg);                    // rem = w * cg + channel group: contiguous in the source row
      float v[V];
      ldv<T, V>(b + ((int64_t)(r ? y1 : y0) * W) * C + (int64_t)rem * V, v);
      stv<T, V>(rows + ((size_t)(r * a.cols + a.col0[i]) * C) + (size_t)rem * V, v);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < Wo * cg; t += 256) {
    const int xo = (int)fdiv((uint32_t)t, a.dcg), c = (t - xo * cg) * V;
    float o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i >= a.n) break;
      const int f = a.f[i];
      const int x0 = (int)fdiv((uint32_t)xo, a.df[i]), x1 = min(x0 + 1, a.w[i] - 1);
      const float fx = (float)(xo - x0 * f) * (1.f / (float)f);
      const T* r0 = rows + (size_t)a.col0[i] * C + c;
      const T* r1 = r0 + (size_t)a.cols * C;
      float v00[V], v01[V], v10[V], v11[V];
      ldv<T, V>(r0 + (size_t)x0 * C, v00);
      ldv<T, V>(r0 + (size_t)x1 * C, v01);
      ldv<T, V>(r1 + (size_t)x0 * C, v10);
      ldv<T, V>(r1 + (size_t)x1 * C, v11);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float top = v00[e] + (v01[e] - v00[e]) * fx, bot = v10[e] + (v11[e] - v10[e]) * fx;
        o[e] += top + (bot - top) * fy[i];
      }
    }
    stv<T, V>(y + (((int64_t)n * Ho + yo) * Wo + xo) * C + c, o);
  }
}

extern "C" int stp_upsample_sum(const void* x0, const void* x1, const void* x2, const void* x3, int32_t h0, int32_t h1, int32_t h2, int32_t h3,
                                void* y, int32_t N, int32_t Ho, int32_t Wo, int32_t C, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype) || !y || N <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || Ho != Wo) return STP_E_BADARG;
  const void* xs[4] = {x0, x1, x2, x3};
  const int hs[4] = {h0, h1, h2, h3};
  UpSum4 a;
  a.n = 0; a.cols = 0;
  for (int i = 0; i < 4; ++i) {
    if (!xs[i]) break;
    if (hs[i] <= 0 || Ho % hs[i]) return STP_E_BADARG;
    a.x[a.n] = xs[i]; a.h[a.n] = a.w[a.n] = hs[i]; a.f[a.n] = Ho / hs[i]; a.df[a.n] = make_fastdiv((uint32_t)(Ho / hs[i]));
    a.col0[a.n] = a.cols; a.cols += hs[i];
    ++a.n;
  }
  for (int i = a.n; i < 4; ++i) { a.x[i] = nullptr; a.h[i] = a.w[i] = a.f[i] = 1; a.col0[i] = 0; a.df[i] = make_fastdiv(1u); }
  const int V = dtype == STP_H16 ? (C % 8 == 0 ? 8 : C % 4 == 0 ? 4 : 0) : (C % 4 == 0 ? 4 : 0);
  const size_t lds = (size_t)2 * a.cols * C * (dtype == STP_H16 ? 2 : 4);
  if (!a.n || !V || (int64_t)N * Ho >= (1ll << 31) || lds > 64 * 1024) return STP_E_BADARG;      // (PSPNet: 12 columns x 512 channels = 24 KB)
  a.dcg = make_fastdiv((uint32_t)(C / V));
  const dim3 grid((unsigned)(N * Ho));
  hipStream_t s = (hipStream_t)stream;
  return launch_tv(dtype, dtype == STP_H16 && V == 8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((upsample_sum_kernel<T, V>), grid, dim3(256), lds, s, a, (T*)y, Ho, Wo, C);
  });
}

extern "C" size_t stp_resize_bilinear_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || factor < 2) return 0;
  const int64_t npix = (int64_t)N * H * W;
  const int span = 2 * factor;
  size_t need = 0;
  // the two-pass form for tiny maps (part[N][H * factor][W][C] fp32); sized for either 16-bit or fp32 vectors, any slice alignment
  if (factor >= 8 && W <= RBT_MAXW && H <= 16) need = (size_t)N * H * factor * W * C * sizeof(float);
  for (int V = 4; V <= 8; V += 4) {
    const int cg = ceil_div(C, V);
    const int rps = split_rows(npix * ceil_div(cg, pool_vl(cg)), span, span);
    if (rps < span) need = std::max(need, (size_t)ceil_div(span, rps) * npix * C * sizeof(float));
  }
  return need;
}

extern "C" int stp_resize_bilinear_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor,
                                       int32_t ldo, int32_t coff, int32_t dtype, int32_t accumulate, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!dy || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || factor < 1 || ldo < coff + C || coff < 0) return STP_E_BADARG;
  if (dtype != STP_H16 && dtype != STP_F32) return STP_E_BADARG;
  const int V = vec_for(dtype, C, ldo, coff);
  if (V > 1 && factor == 1) {      // a channel slice copied (or added) back
    const int64_t pixels = (int64_t)N * H * W;
    const int g = grid_for_amortised(pixels * (C / V), 4);
    hipStream_t s = (hipStream_t)stream;
    return launch_tv(dtype, V == 8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((slice_copy_kernel<T, V>), dim3(g), dim3(256), 0, s, (const T*)dy, (T*)dx, pixels, C, ldo, coff, accumulate);
    });
  }
  if (resize_bwd_tiny_ok(N, H, W, C, factor, ldo, coff, dtype) && workspace &&
      workspace_bytes >= (size_t)N * H * factor * W * C * sizeof(float) && !(reinterpret_cast<uintptr_t>(dy) & 15)) {
    // tiny map, large factor (pyramid levels): separable two-pass reduction, every byte of dY read once
    const int ev = dtype == STP_H16 ? 8 : 4, cgv = C / ev, G = 256 / cgv;
    const size_t lds = (size_t)(G - 1) * W * C * sizeof(float);
    float* part = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)(N * H * factor));
    const int rc = launch_t(dtype, [&](auto tv) {
      using T = typename decltype(tv)::T;
      hipLaunchKernelGGL(resize_bilinear_bwd_tiny_rows_kernel<T>, grid, dim3(256), lds, s, (const T*)dy, part, H, W, C, factor, ldo, coff);
    });
    if (rc) return rc;
    const int g2 = (int)(((int64_t)N * H * W * (C / 4) + 3) / 4);
    return launch_t(dtype, [&](auto tv) {
      using T = typename decltype(tv)::T;
      hipLaunchKernelGGL(resize_bilinear_bwd_tiny_cols_kernel<T>, dim3(g2), dim3(256), 0, s, part, (T*)dx, N, H, W, C, factor, accumulate);
    });
  }
  {
    // class logits (few channels, whole output rows fit an LDS buffer): the row-streaming kernel.  STP_RESIZE_BWD_ROWS=0: the gather kernel.
    static const bool rows_on = !(getenv("STP_RESIZE_BWD_ROWS") && atoi(getenv("STP_RESIZE_BWD_ROWS")) == 0);
    const int esz = dtype == STP_H16 ? 2 : 4, ev = 16 / esz;
    const int64_t rowB = (int64_t)W * factor * ldo * esz;
    const int nvec = (int)((rowB / 16 + 255) / 256);
    if (rows_on && factor >= 2 && !(C % ev) && !(ldo % ev) && !(coff % ev) && (int64_t)W * (C / ev) <= 512 && rowB <= 40960 && nvec <= 10 &&
        !(reinterpret_cast<uintptr_t>(dy) & 15) && !(reinterpret_cast<uintptr_t>(dx) & 15) && (int64_t)N * H < (1ll << 31)) {
      const dim3 grid((unsigned)(N * H));
      hipStream_t s = (hipStream_t)stream;
      return launch_t(dtype, [&](auto tv) {
        using T = typename decltype(tv)::T;
        hipLaunchKernelGGL(resize_bilinear_bwd_rows_kernel<T>, grid, dim3(256), (size_t)(2 * rowB), s, (const T*)dy, (T*)dx, H, W, C, factor, ldo, coff,
                           accumulate, nvec);
      });
    }
  }
  {
    // wide 16-bit channel slices (FPN's pyramid levels): the row-pair tile kernel.  STP_RESIZE_BWD_TILE=0: the gather kernel.
    static const bool tile_on = !(getenv("STP_RESIZE_BWD_TILE") && atoi(getenv("STP_RESIZE_BWD_TILE")) == 0);
    const int WS = factor >= 64 ? 1 : 64 / (factor > 0 ? factor : 1), CC = C < 64 ? C : 64;
    const int cols = (WS + 1) * factor - 1;
    const size_t lds = (size_t)2 * cols * CC * sizeof(float);
    if (tile_on && V == 8 && factor >= 2 && C >= 32 && C % CC == 0 && cols * (CC / 8) <= 256 * RBT_K && lds <= 96 * 1024 &&
        (int64_t)N * ((H + 1) / 2) <= 65535 && C / CC <= 65535 && !(reinterpret_cast<uintptr_t>(dy) & 15) && !(reinterpret_cast<uintptr_t>(dx) & 7)) {
      const dim3 grid((unsigned)ceil_div(W, WS), (unsigned)(N * ((H + 1) / 2)), (unsigned)(C / CC));
      // (cols * (CC / 8) <= 256 * RBT_K bounds lds by 48 KB today; a larger RBT_K gets its grant from the helper)
      return stp_launch_lds(resize_bilinear_bwd_tile_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t*)dy, (bf16_t*)dx, H, W, C,
                            factor, ldo, coff, accumulate, WS, CC);
    }
  }
  if (V > 1 && factor >= 2) {
    const int cg = C / V, span = 2 * factor;
    const int64_t npix = (int64_t)N * H * W;
    // few taps per pixel: wide channel chunks keep the tap lanes busy; many taps: 128-byte chunks and more workgroups
    const int VL = span * span >= 256 ? pool_vl(cg) : (cg < 32 ? cg : 32);
    int rps = VL == pool_vl(cg) ? split_rows(npix * ceil_div(cg, VL), span, span) : span;
    int S = ceil_div(span, rps);
    if (S > 1 && (!workspace || workspace_bytes < (size_t)S * npix * C * sizeof(float))) { rps = span; S = 1; }
    float* part = S > 1 ? (float*)workspace : nullptr;
    // tap lanes per pixel: the largest power of two that the taps can keep busy; the rest of the workgroup takes more pixels
    int TLp = 1;
    while (TLp * 2 <= 256 / VL && TLp * 2 <= span * span) TLp *= 2;
    int PPB = (256 / VL) / TLp;
    if (S > 1 || PPB < 1) { PPB = 1; TLp = 256 / VL; }
    const dim3 grid((unsigned)ceil_div(npix, PPB), ceil_div(cg, VL), S);
    const size_t lds = (size_t)(256 / VL) * VL * V * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    const int rc = launch_tv(dtype, V == 8, [&](auto tv) {
      using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
      hipLaunchKernelGGL((resize_bilinear_bwd_blk_kernel<T, V>), grid, dim3(256), lds, s, (const T*)dy, (T*)dx, H, W, C, factor, ldo, coff, accumulate, VL,
                         rps, part, TLp, PPB, (int)npix);
    });
    if (rc || S <= 1) return rc;
    return split_combine_launch(part, S, npix * C, 1.f, dx, dtype, accumulate, s);
  }
  const int g = grid_for((int64_t)N * H * W * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(resize_bilinear_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (T*)dx, N, H, W, C, factor, ldo, coff,
                       accumulate);
  });
}

// ------------------------------------------------------------------------------------------
// ResizeImage(factor, interpolation='nearest') = UpSampling2D(factor): y[n, yo, xo, coff + c] = x[n, yo / f, xo / f, c]; the
// gradient sums the f x f outputs of an input pixel in row-major order (segmentation_models' FPN `interpolation: nearest`, PSPNet
// `final_interpolation: nearest`, schemas/segmentation.raml:196-199, 245-248)
template <typename T>
__global__ __launch_bounds__(256) void resize_nearest_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int f,
                                                             int ldo, int coff) {
  const int Ho = H * f, Wo = W * f;
  const int64_t total = (int64_t)N * Ho * Wo * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int xo = (int)(p % Wo), yo = (int)((p / Wo) % Ho), n = (int)(p / ((int64_t)Wo * Ho));
    y[p * ldo + coff + c] = x[(((int64_t)n * H + yo / f) * W + xo / f) * C + c];
  }
}
template <typename T>
__global__ __launch_bounds__(256) void resize_nearest_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C,
                                                                 int f, int ldo, int coff, int accumulate) {
  const int Wo = W * f, Ho = H * f;
  const int64_t total = (int64_t)N * H * W * C;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int xi = (int)(p % W), yi = (int)((p / W) % H), n = (int)(p / ((int64_t)W * H));
    float s = 0.f;
    for (int a = 0; a < f; ++a)
      for (int b = 0; b < f; ++b) s += Elem<T>::load(dy + (((int64_t)n * Ho + yi * f + a) * Wo + xi * f + b) * ldo + coff + c);
    if (accumulate) s += Elem<T>::load(dx + i);
    Elem<T>::store(dx + i, s);
  }
}
extern "C" int stp_resize_nearest(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo, int32_t coff,
                                  int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || factor < 1 || ldo < coff + C || coff < 0) return STP_E_BADARG;
  const int g = grid_for((int64_t)N * H * factor * W * factor * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(resize_nearest_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, N, H, W, C, factor, ldo, coff);
  });
}
extern "C" int stp_resize_nearest_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo,
                                      int32_t coff, int32_t dtype, int32_t accumulate, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!dy || !dx || N <= 0 || H <= 0 || W <= 0 || C <= 0 || factor < 1 || ldo < coff + C || coff < 0) return STP_E_BADARG;
  const int g = grid_for((int64_t)N * H * W * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(resize_nearest_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (T*)dx, N, H, W, C, factor, ldo, coff,
                       accumulate);
  });
}
