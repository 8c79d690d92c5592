// Prediction on the device (segmentation_pipeline/segmentation.py: predict_on_batch_device and the methods over it): the flipped
// input of flip test-time augmentation, the running sum of the models' un-flipped probability maps, and the finished map - the mean,
// gathered back to the image's own size, as fp32, as the bytes of a PNG or as a label map.  Three streaming kernels on uint8 and
// fp32 (nothing here depends on the build's 16-bit storage format), no atomics, int64 element indices.
//
// Every value is produced by the operation numpy would use on the host - one fp32 add per model and flip in a fixed order, one
// correctly rounded fp32 division, one fp32 multiplication by 255 and a truncation - so the device path equals the host path
// (predict_on_batch, _scale_back, astype(uint8), argmax) bit for bit.
//
// Access width: a thread owns VEC consecutive elements of one DESTINATION row and moves them with one 16-byte access where every row
// starts on a 16-byte boundary (base pointer aligned, row pitch a multiple of 16 bytes); otherwise one element per thread.  The source
// side of a column flip and of the nearest gather is read element by element (its 16 bytes are not contiguous).
#include "common.h"

template <typename T, int VEC> struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline int stream_grid(int64_t items) {
  int64_t g = (items + 255) / 256;
  return (int)(g > 16384 ? 16384 : g);
}

// dst[n][y][x][c] (+)= src[n][y'][x'][c];  flip 0: (y', x') = (y, x), 1: (y, W - 1 - x), 2: (H - 1 - y, x).  rows = N * H.
// COLUMNS = (flip == 1) is a template parameter so that the other two keep their one 16-byte load per thread.
template <typename T, int VEC, bool ACCUMULATE, bool COLUMNS>
__global__ __launch_bounds__(256) void flip_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t rows, int H, int W, int C, int flip) {
  typedef Pack<T, VEC> P;
  const int rowlen = W * C, vpr = rowlen / VEC;      // (VEC divides rowlen: the launcher's condition)
  const int64_t total = rows * vpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / vpr;
    const int e0 = (int)(i - r * vpr) * VEC;
    const int y = (int)(r % H);
    const int64_t sr = flip == 2 ? r - y + (H - 1 - y) : r;
    const T* srow = src + sr * rowlen;
    T* dptr = dst + r * rowlen + e0;
    P v;
    if (!COLUMNS) {
      v = *reinterpret_cast<const P*>(srow + e0);
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int e = e0 + j, x = e / C, c = e - x * C;
        v.v[j] = srow[(W - 1 - x) * C + c];
      }
    }
    if (ACCUMULATE) {
      const P a = *reinterpret_cast<const P*>(dptr);
#pragma unroll
      for (int j = 0; j < VEC; ++j) v.v[j] = (T)__fadd_rn((float)a.v[j], (float)v.v[j]);
    }
    *reinterpret_cast<P*>(dptr) = v;
  }
}

template <typename T, bool ACCUMULATE>
static int launch_flip(const T* src, T* dst, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flip, void* stream) {
  if (!src || !dst || src == dst || N <= 0 || H <= 0 || W <= 0 || C <= 0 || flip < 0 || flip > 2) return STP_E_BADARG;
  if ((int64_t)W * C > 0x7fffffff) return STP_E_BADARG;
  constexpr int VEC = 16 / (int)sizeof(T);
  const int64_t rows = (int64_t)N * H;
  const int rowlen = W * C;
  const bool vec = rowlen % VEC == 0 && aligned16(src) && aligned16(dst);
  const dim3 grid(stream_grid(vec ? rows * (rowlen / VEC) : rows * rowlen));
  void (*kernel)(const T*, T*, int64_t, int, int, int, int) =
      vec ? (flip == 1 ? flip_kernel<T, VEC, ACCUMULATE, true> : flip_kernel<T, VEC, ACCUMULATE, false>)
          : (flip == 1 ? flip_kernel<T, 1, ACCUMULATE, true> : flip_kernel<T, 1, ACCUMULATE, false>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, src, dst, rows, H, W, C, flip);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_flip_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flip, void* stream) {
  return launch_flip<uint8_t, false>(src, dst, N, H, W, C, flip, stream);
}

extern "C" int stp_predict_accumulate(const float* probs, float* acc, int32_t N, int32_t H, int32_t W, int32_t C, int32_t flip, void* stream) {
  return launch_flip<float, true>(probs, acc, N, H, W, C, flip, stream);
}

// One image: out row y, pixel x <- acc[(y * H / h), (x * W / w)] / k (integer division of the coordinates: PipelineConfig._scale_back).
// MODE 0: fp32 [h][w][C];  1: uint8 [h][w][C] = (uint8)(value * 255.f);  2: uint8 [h][w] = first index of the largest of the C values
// (a NaN is never larger), or value > 0.5f for C == 1.  A destination row holds w * C elements (mode 2: w), rows are out_ld pixels apart.
template <int MODE> struct FinishOut { typedef uint8_t type; };
template <> struct FinishOut<0> { typedef float type; };

template <int MODE>
__device__ __forceinline__ typename FinishOut<MODE>::type finish_one(const float* __restrict__ srow, int e, int W, int C, int w, float kf) {
  if (MODE == 2) {
    const float* px = srow + (int64_t)((int64_t)e * W / w) * C;
    const float v0 = __fdiv_rn(px[0], kf);
    if (C == 1) return v0 > 0.5f;
    float best = v0;
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = __fdiv_rn(px[c], kf);
      if (v > best) best = v, arg = c;
    }
    return (typename FinishOut<MODE>::type)arg;
  }
  const int x = e / C, c = e - x * C;
  const float v = __fdiv_rn(srow[(int64_t)((int64_t)x * W / w) * C + c], kf);
  if (MODE == 0) return v;
  return (typename FinishOut<MODE>::type)(uint8_t)(int)__fmul_rn(v, 255.f);
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void predict_finish_kernel(const float* __restrict__ acc, int H, int W, int C, float kf,
                                                             typename FinishOut<MODE>::type* __restrict__ out, int h, int w, int64_t pitch) {
  typedef typename FinishOut<MODE>::type T;
  typedef Pack<T, VEC> P;
  const int rowlen = MODE == 2 ? w : w * C, vpr = (rowlen + VEC - 1) / VEC;
  const int64_t total = (int64_t)h * vpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int y = (int)(i / vpr);
    const int e0 = (int)(i - (int64_t)y * vpr) * VEC;
    const float* srow = acc + (int64_t)((int64_t)y * H / h) * W * C;
    T* dptr = out + (int64_t)y * pitch + e0;
    if (e0 + VEC <= rowlen) {
      P v;
#pragma unroll
      for (int j = 0; j < VEC; ++j) v.v[j] = finish_one<MODE>(srow, e0 + j, W, C, w, kf);
      *reinterpret_cast<P*>(dptr) = v;
    } else {      // the row's tail: fewer than VEC elements left
      for (int j = 0; e0 + j < rowlen; ++j) dptr[j] = finish_one<MODE>(srow, e0 + j, W, C, w, kf);
    }
  }
}

template <int MODE>
static void launch_finish(const float* acc, int H, int W, int C, float kf, void* out, int h, int w, int64_t pitch, hipStream_t st) {
  typedef typename FinishOut<MODE>::type T;
  constexpr int VEC = 16 / (int)sizeof(T);
  const int rowlen = MODE == 2 ? w : w * C;
  if (aligned16(out) && pitch % VEC == 0) {
    hipLaunchKernelGGL((predict_finish_kernel<MODE, VEC>), dim3(stream_grid((int64_t)h * ((rowlen + VEC - 1) / VEC))), dim3(256), 0, st, acc, H, W, C,
                       kf, (T*)out, h, w, pitch);
  } else {
    hipLaunchKernelGGL((predict_finish_kernel<MODE, 1>), dim3(stream_grid((int64_t)h * rowlen)), dim3(256), 0, st, acc, H, W, C, kf, (T*)out, h, w,
                       pitch);
  }
}

extern "C" int stp_predict_finish(const float* acc, int32_t H, int32_t W, int32_t C, int32_t k, int32_t mode, void* out, int32_t h, int32_t w,
                                  int32_t out_ld, void* stream) {
  if (!acc || !out || (const void*)acc == out || H <= 0 || W <= 0 || C <= 0 || k <= 0 || mode < 0 || mode > 2 || h <= 0 || w <= 0 || out_ld < w)
    return STP_E_BADARG;
  if (mode == 2 && C > 32) return STP_E_BADARG;
  if ((int64_t)w * C > 0x7fffffff || (int64_t)W * C > 0x7fffffff) return STP_E_BADARG;
  const int64_t pitch = mode == 2 ? (int64_t)out_ld : (int64_t)out_ld * C;      // destination elements between rows
  const float kf = (float)k;
  if (mode == 0) launch_finish<0>(acc, H, W, C, kf, out, h, w, pitch, (hipStream_t)stream);
  else if (mode == 1) launch_finish<1>(acc, H, W, C, kf, out, h, w, pitch, (hipStream_t)stream);
  else launch_finish<2>(acc, H, W, C, kf, out, h, w, pitch, (hipStream_t)stream);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
