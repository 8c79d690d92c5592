// Small elementwise and per-channel passes: zero fill, the tap-sum head (a 3x3 class head as a 1x1 convolution + tap sum), the
// gradient of a ReLU fused into a convolution, the fp32 column-slice copy, per-channel sums (bias gradient) and dst += src.
#include "stream_ops.h"

__global__ __launch_bounds__(256) void zero_kernel(uint4* p, int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = uint4{0u, 0u, 0u, 0u};
}
extern "C" int stp_zero_bytes(void* p, int64_t bytes, void* stream) {
  if (!p || bytes <= 0 || (bytes & 15) || ((uintptr_t)p & 15)) return STP_E_BADARG;
  hipLaunchKernelGGL(zero_kernel, dim3(grid_for(bytes >> 4)), dim3(256), 0, (hipStream_t)stream, (uint4*)p, bytes >> 4);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// Conv2D(3x3, padding 1) with FEW output channels over MANY input channels (the class heads of FPN and PSPNet: 512 -> 3 / 20) as a 1x1
// convolution into 9 x Cout TAP CHANNELS + a tap sum.  Channel mixing is pointwise, so W_t . shift_t(x) = shift_t(W_t . x): the 3x3 kernel
// [Cout][3][3][Cin] IS the matrix [9 Cout][Cin] of a 1x1 convolution z = W x (row o * 9 + t: no copy, the master parameter's own bytes) and
//   y[n, h, w, o] = bias[o] + sum_t z[n, h + t / 3 - 1, w + t % 3 - 1, o * 9 + t]        (taps outside the image: zero, as the padding)
// The per-tap kernel read the 512-channel input nine times from L2 for 3 useful output channels (340 us forward, 308 us data gradient,
// 183 us weight gradient on FPN/ResNet50 1024 x 1024 batch 4); the 1x1 form reads it once per pass and everything else is 27 channels wide.
// Backward: dz[n, h, w, o * 9 + t] = dy[n, h - (t / 3 - 1), w - (t % 3 - 1), o], then the 1x1 convolution's ordinary gradients - its weight
// gradient is the 3x3 kernel's gradient in place.
template <typename T>
__global__ __launch_bounds__(256) void tapsum_fwd_kernel(const T* __restrict__ z, T* __restrict__ y, const float* __restrict__ bias, int N, int H, int W,
                                                         int Cout, int Zc, int Cy) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * H * W * Cout) return;
  const int o = (int)(idx % Cout);
  const long long p = idx / Cout;
  const int w = (int)(p % W), h = (int)((p / W) % H), n = (int)(p / ((long long)W * H));
  float acc = bias ? bias[o] : 0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int hh = h + t / 3 - 1, ww = w + t % 3 - 1;
    if ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) acc += Elem<T>::load(z + (((size_t)n * H + hh) * W + ww) * Zc + o * 9 + t);
  }
  Elem<T>::store(y + (size_t)p * Cy + o, acc);
}
template <typename T>
__global__ __launch_bounds__(256) void tapsum_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dz, int N, int H, int W, int Cout, int Cdy, int Cdz) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)N * H * W * Cdz) return;
  const int j = (int)(idx % Cdz);
  const long long p = idx / Cdz;
  const int w = (int)(p % W), h = (int)((p / W) % H), n = (int)(p / ((long long)W * H));
  float v = 0.f;
  if (j < 9 * Cout) {
    const int o = j / 9, t = j - o * 9;
    const int hh = h - (t / 3 - 1), ww = w - (t % 3 - 1);
    if ((unsigned)hh < (unsigned)H && (unsigned)ww < (unsigned)W) v = Elem<T>::load(dy + (((size_t)n * H + hh) * W + ww) * Cdy + o);
  }
  Elem<T>::store(dz + (size_t)idx, v);                      // (the padded tap channels j >= 9 Cout: zero)
}

// z: [N, H, W, Zc] with the tap channel (o, t) at o * 9 + t (Zc >= 9 Cout); y: [N, H, W, Cy] (channels >= Cout untouched); bias: [Cout] or NULL
extern "C" int stp_tapsum_fwd(const void* z, void* y, const float* bias, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t Zc, int32_t Cy,
                              int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!z || !y || N <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Zc < 9 * Cout || Cy < Cout) return STP_E_BADARG;
  const long long total = (long long)N * H * W * Cout;
  if (total > 0x7fffffffll * 128) return STP_E_BADARG;
  const dim3 grid((unsigned)((total + 255) / 256));
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(tapsum_fwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)z, (T*)y, bias, N, H, W, Cout, Zc, Cy);
  });
}
// dy: [N, H, W, Cdy] (the first Cout channels are read); dz: [N, H, W, Cdz], written whole (Cdz >= 9 Cout)
extern "C" int stp_tapsum_bwd(const void* dy, void* dz, int32_t N, int32_t H, int32_t W, int32_t Cout, int32_t Cdy, int32_t Cdz, int32_t dtype,
                              void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!dy || !dz || N <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Cdz < 9 * Cout || Cdy < Cout) return STP_E_BADARG;
  const long long total = (long long)N * H * W * Cdz;
  if (total > 0x7fffffffll * 128) return STP_E_BADARG;
  const dim3 grid((unsigned)((total + 255) / 256));
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(tapsum_bwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)dy, (T*)dz, N, H, W, Cout, Cdy, Cdz);
  });
}

// dY <- dY * [y > 0] in place: the gradient of a ReLU fused into a convolution epilogue (VGG: Conv2D(activation='relu'))
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ y, T* __restrict__ dy, int64_t count4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count4; i += (int64_t)gridDim.x * 256) {
    const f32x4 a = ld4<T>(y + i * 4);
    f32x4 g = ld4<T>(dy + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) g[e] = a[e] > 0.f ? g[e] : 0.f;
    store4(dy + i * 4, g);
  }
}

extern "C" int stp_relu_bwd(const void* y, void* dy, int64_t count, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!y || !dy || count <= 0 || (count & 3)) return STP_E_BADARG;
  const int g = grid_for(count >> 2);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(relu_bwd_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (const T*)y, (T*)dy, count >> 2);
  });
}

// fp32 column slice of a row-major matrix: dst[r][0 .. cols) (+)= src[r][0 .. cols) with separate row pitches - the 1x1 convolutions
// that multiply by a COLUMN RANGE of a shared kernel (stp_upsample_sum above) read their range as a dense matrix and hand their weight
// gradient back into it.  cols, both pitches and both pointers multiples of 4 floats.
__global__ __launch_bounds__(256) void copy_cols_f32_kernel(float* __restrict__ dst, int ldd, const float* __restrict__ src, int lds, int rows,
                                                            int cols4, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)rows * cols4) return;
  const int r = (int)(i / cols4), c = (int)(i - (int64_t)r * cols4) * 4;
  f32x4 v = *reinterpret_cast<const f32x4*>(src + (int64_t)r * lds + c);
  float* d = dst + (int64_t)r * ldd + c;
  if (accumulate) v += *reinterpret_cast<const f32x4*>(d);
  *reinterpret_cast<f32x4*>(d) = v;
}
extern "C" int stp_copy_cols_f32(float* dst, int32_t ld_dst, const float* src, int32_t ld_src, int32_t rows, int32_t cols, int32_t accumulate, void* stream) {
  if (!dst || !src || rows <= 0 || cols <= 0 || (cols & 3) || (ld_dst & 3) || (ld_src & 3) || ld_dst < cols || ld_src < cols ||
      (reinterpret_cast<uintptr_t>(dst) & 15) || (reinterpret_cast<uintptr_t>(src) & 15))
    return STP_E_BADARG;
  hipLaunchKernelGGL(copy_cols_f32_kernel, dim3(ceil_div((int64_t)rows * (cols / 4), 256)), dim3(256), 0, (hipStream_t)stream, dst, ld_dst, src, ld_src,
                     rows, cols / 4, accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// per-channel sums of a [rows][C] tensor (bias gradient) and dst += src
__global__ __launch_bounds__(256) void colsum_finalize_kernel(const float* partial, int blocks, int C, float* out,
                                                              int accumulate) {
  const int c = blockIdx.x * 4 + (threadIdx.x & 3);
  const Sum2 t = reduce_partials(partial, blocks, C, c, false);
  if ((threadIdx.x >> 2) != 0 || c >= C) return;
  out[c] = accumulate ? out[c] + (float)t.s : (float)t.s;
}

extern "C" int stp_channel_sum(const void* x, int32_t dtype, int64_t rows, int32_t C, float* out, int32_t accumulate,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !out || !workspace || rows <= 0 || C <= 0 || (C & 3)) return STP_E_BADARG;
  if (workspace_bytes < stp_bn_workspace_bytes(C)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = bn_blocks(rows);
  float* partial = (float*)workspace;
  if (const int rc = bn_partial_launch(x, dtype, rows, C, blocks, partial, s)) return rc;
  hipLaunchKernelGGL(colsum_finalize_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, s, partial, blocks, C, out, accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void add_inplace_kernel(T* __restrict__ dst, const T* __restrict__ src, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256)
    store4(dst + i * 4, ld4<T>(dst + i * 4) + ld4<T>(src + i * 4));
}

extern "C" int stp_add_inplace(void* dst, const void* src, int64_t count, int32_t dtype, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!dst || !src || count <= 0 || (count & 3)) return STP_E_BADARG;
  const int g = grid_for(count >> 2);
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(add_inplace_kernel<T>, dim3(g), dim3(256), 0, (hipStream_t)stream, (T*)dst, (const T*)src, count >> 2);
  });
}
