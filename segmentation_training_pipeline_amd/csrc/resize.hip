// Changes of resolution by an integer factor, forward: bilinear resize (TF 1.x, align_corners False) into a channel slice, the sum of
// resized pyramid levels (PSPNet head), nearest resize with its gradient.  The gradient of the bilinear resize is resize_bwd.hip;
// the 2x gradients that complete a BatchNormalization backward are upsample2x.hip.
#include "stream_ops.h"

// tf.image.resize_bilinear(align_corners=False) of TF 1.x (what Keras 2.2.4 K.resize_images(interpolation='bilinear')
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

extern "C" int stp_resize_bilinear(const void* x, void* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo,
                                   int32_t coff, int32_t dtype, void* stream) {
  if (!resize_args_ok(x, y, N, H, W, C, factor, ldo, coff, dtype)) return STP_E_BADARG;
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
  if (!resize_args_ok(x, y, N, H, W, C, factor, ldo, coff, dtype)) return STP_E_BADARG;
  const int g = grid_for((int64_t)N * H * factor * W * factor * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(resize_nearest_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)x, (T*)y, N, H, W, C, factor, ldo, coff);
  });
}
extern "C" int stp_resize_nearest_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor, int32_t ldo,
                                      int32_t coff, int32_t dtype, int32_t accumulate, void* stream) {
  if (!resize_args_ok(dy, dx, N, H, W, C, factor, ldo, coff, dtype)) return STP_E_BADARG;
  const int g = grid_for((int64_t)N * H * W * C);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(resize_nearest_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)dy, (T*)dx, N, H, W, C, factor, ldo, coff,
                       accumulate);
  });
}
