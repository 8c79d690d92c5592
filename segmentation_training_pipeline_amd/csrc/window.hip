// Sliding-window prediction on the device (segmentation_pipeline/segmentation.py: _predict_windows_device): an image larger than the
// network shape is predicted at its own pixel scale in overlapping H x W windows that are cross-faded where they overlap.  Three
// streaming kernels around the unchanged inference plan: the gather of one batch of windows out of the image, the weighted sum of the
// batch's probability sums into the full-size canvas, and the finished map.  uint8 and fp32 only (nothing here depends on the build's
// 16-bit storage format), no atomics, int64 element indices.
//
// Geometry: a window at origin (y0, x0) weights its pixel (ly, lx) with ry[ly] * rx[lx], r[i] = min(i + 1, L - i, overlap + 1) - a
// linear ramp over the `overlap` border pixels, integers throughout.  The canvas is accumulated in GATHER form: a thread owns canvas
// elements and walks the batch's windows in index order, so no two threads write one element, nothing is atomic and the order of the
// fp32 additions is the window order - the order of the host statement (tests/_window_reference.py), whose result the three kernels
// reproduce bit for bit: one fp32 multiplication and one fp32 addition per window, one correctly rounded division at the end.
//
// Access width, as in predict.hip: a thread owns VEC consecutive elements of one DESTINATION row and moves them with one 16-byte access
// where every row starts on a 16-byte boundary; otherwise one element per thread.  Sources (the image under a window's clipped
// coordinates, a window's sums under a canvas pixel) start anywhere and are read element by element.
#include "common.h"

#define STP_WINDOW_MAX 64

template <typename T, int VEC> struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

// the batch's window origins, (y0, x0) per window: copied from the host into the kernel's arguments
struct Origins {
  int32_t yx[STP_WINDOW_MAX][2];
};

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline int stream_grid(int64_t items) {
  int64_t g = (items + 255) / 256;
  return (int)(g > 16384 ? 16384 : g);
}

// origins -> Origins after the checks every entry makes: n in 1..64, 0 <= y0 < h, 0 <= x0 < w
static bool load_origins(const int32_t* origins, int32_t n, int32_t h, int32_t w, Origins* o) {
  if (!origins || n < 1 || n > STP_WINDOW_MAX) return false;
  for (int i = 0; i < n; ++i) {
    const int32_t y0 = origins[2 * i], x0 = origins[2 * i + 1];
    if (y0 < 0 || y0 >= h || x0 < 0 || x0 >= w) return false;
    o->yx[i][0] = y0, o->yx[i][1] = x0;
  }
  for (int i = n; i < STP_WINDOW_MAX; ++i) o->yx[i][0] = o->yx[i][1] = 0;
  return true;
}

// dst[i][y][x][c] = img[min(y0_i + y, h - 1)][min(x0_i + x, w - 1)][c];  blockIdx.y = the window i (uniform: its origin is a scalar load
// from the kernel's arguments).
template <int VEC>
__global__ __launch_bounds__(256) void window_gather_kernel(const uint8_t* __restrict__ img, int h, int w, int C, Origins org,
                                                            uint8_t* __restrict__ dst, int H, int W) {
  typedef Pack<uint8_t, VEC> P;
  const int rowlen = W * C, vpr = rowlen / VEC;      // (VEC divides rowlen: the launcher's condition)
  const int i = blockIdx.y;
  const int y0 = org.yx[i][0], x0 = org.yx[i][1];
  const int64_t total = (int64_t)H * vpr;
  uint8_t* win = dst + (int64_t)i * H * rowlen;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int y = (int)(t / vpr);
    const int e0 = (int)(t - (int64_t)y * vpr) * VEC;
    const uint8_t* srow = img + (int64_t)min(y0 + y, h - 1) * w * C;
    P v;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int e = e0 + j, x = e / C, c = e - x * C;
      v.v[j] = srow[(int64_t)min(x0 + x, w - 1) * C + c];
    }
    *reinterpret_cast<P*>(win + (int64_t)y * rowlen + e0) = v;
  }
}

extern "C" int stp_window_gather_u8(const uint8_t* img, int32_t h, int32_t w, int32_t C, const int32_t* origins, int32_t n, uint8_t* dst,
                                    int32_t H, int32_t W, void* stream) {
  if (!img || !dst || img == dst || h <= 0 || w <= 0 || C <= 0 || H <= 0 || W <= 0) return STP_E_BADARG;
  if ((int64_t)W * C > 0x7fffffff || (int64_t)w * C > 0x7fffffff) return STP_E_BADARG;
  Origins org;
  if (!load_origins(origins, n, h, w, &org)) return STP_E_BADARG;
  const int rowlen = W * C;
  if (rowlen % 16 == 0 && aligned16(dst)) {
    hipLaunchKernelGGL(window_gather_kernel<16>, dim3(stream_grid((int64_t)H * (rowlen / 16)), n), dim3(256), 0, (hipStream_t)stream, img, h, w, C,
                       org, dst, H, W);
  } else {
    hipLaunchKernelGGL(window_gather_kernel<1>, dim3(stream_grid((int64_t)H * rowlen), n), dim3(256), 0, (hipStream_t)stream, img, h, w, C, org, dst,
                       H, W);
  }
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// the ramp of one axis: window pixel l of L, min(l + 1, L - l, overlap + 1)
__device__ __forceinline__ int ramp(int l, int L, int overlap) { return min(min(l + 1, L - l), overlap + 1); }

// canvas[y][x][c] += sum over the windows i that hold (y, x), in index order, of (float)(ry * rx) * acc[i][y - y0][x - x0][c];
// rows ybeg .. ybeg + rows - 1 of the canvas (the rows the batch's windows span).
template <int VEC>
__global__ __launch_bounds__(256) void window_accumulate_kernel(const float* __restrict__ acc, int H, int W, int C, Origins org, int n, int overlap,
                                                                float* __restrict__ canvas, int w, int ybeg, int rows) {
  typedef Pack<float, VEC> P;
  const int rowlen = w * C, vpr = rowlen / VEC;      // (VEC divides rowlen: the launcher's condition)
  const int64_t total = (int64_t)rows * vpr;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int r = (int)(t / vpr);
    const int e0 = (int)(t - (int64_t)r * vpr) * VEC;
    const int y = ybeg + r;
    float* cptr = canvas + (int64_t)y * rowlen + e0;
    int xs[VEC], cs[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) xs[j] = (e0 + j) / C, cs[j] = (e0 + j) - xs[j] * C;
    P v;
    bool touched = false;
    for (int i = 0; i < n; ++i) {
      const int ly = y - org.yx[i][0], x0 = org.yx[i][1];
      if (ly < 0 || ly >= H || xs[VEC - 1] < x0 || xs[0] >= x0 + W) continue;      // this window holds none of the thread's pixels
      if (!touched) v = *reinterpret_cast<const P*>(cptr), touched = true;
      const int ry = ramp(ly, H, overlap);
      const float* arow = acc + ((int64_t)i * H + ly) * W * C;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int lx = xs[j] - x0;
        if (lx >= 0 && lx < W) {
          const float wgt = (float)(ry * ramp(lx, W, overlap));
          v.v[j] = __fadd_rn(v.v[j], __fmul_rn(wgt, arow[(int64_t)lx * C + cs[j]]));
        }
      }
    }
    if (touched) *reinterpret_cast<P*>(cptr) = v;
  }
}

extern "C" int stp_window_accumulate(const float* acc, int32_t H, int32_t W, int32_t C, const int32_t* origins, int32_t n, int32_t overlap,
                                     float* canvas, int32_t h, int32_t w, void* stream) {
  if (!acc || !canvas || acc == canvas || H <= 0 || W <= 0 || C <= 0 || h <= 0 || w <= 0) return STP_E_BADARG;
  if (overlap < 0 || 2 * (int64_t)overlap > (H < W ? H : W) || overlap >= 4096) return STP_E_BADARG;      // (overlap + 1)^2 is an exact fp32 integer
  if ((int64_t)W * C > 0x7fffffff || (int64_t)w * C > 0x7fffffff) return STP_E_BADARG;
  Origins org;
  if (!load_origins(origins, n, h, w, &org)) return STP_E_BADARG;
  int ybeg = h, yend = 0;                            // the canvas rows the batch's windows span
  for (int i = 0; i < n; ++i) {
    const int y0 = org.yx[i][0], y1 = (int64_t)y0 + H < h ? y0 + H : h;
    ybeg = y0 < ybeg ? y0 : ybeg;
    yend = y1 > yend ? y1 : yend;
  }
  const int rows = yend - ybeg, rowlen = w * C;
  if (rowlen % 4 == 0 && aligned16(canvas)) {
    hipLaunchKernelGGL(window_accumulate_kernel<4>, dim3(stream_grid((int64_t)rows * (rowlen / 4))), dim3(256), 0, (hipStream_t)stream, acc, H, W, C,
                       org, n, overlap, canvas, w, ybeg, rows);
  } else {
    hipLaunchKernelGGL(window_accumulate_kernel<1>, dim3(stream_grid((int64_t)rows * rowlen)), dim3(256), 0, (hipStream_t)stream, acc, H, W, C, org,
                       n, overlap, canvas, w, ybeg, rows);
  }
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// value = canvas[y][x][c] / (k * sy[y] * sx[x]).  MODE 0: fp32 [h][w][C];  1: uint8 [h][w][C] = (uint8)(value * 255.f);  2: uint8 [h][w] =
// first index of the largest of the C values (a NaN is never larger), or value > 0.5f for C == 1.  A destination row holds w * C elements
// (mode 2: w), rows are `pitch` elements apart.
template <int MODE> struct WindowOut { typedef uint8_t type; };
template <> struct WindowOut<0> { typedef float type; };

template <int MODE>
__device__ __forceinline__ typename WindowOut<MODE>::type window_finish_one(const float* __restrict__ crow, int e, int C, float ky,
                                                                           const float* __restrict__ sx) {
  typedef typename WindowOut<MODE>::type T;
  if (MODE == 2) {
    const float* px = crow + (int64_t)e * C;
    const float den = __fmul_rn(ky, sx[e]);
    const float v0 = __fdiv_rn(px[0], den);
    if (C == 1) return v0 > 0.5f;
    float best = v0;
    int arg = 0;
    for (int c = 1; c < C; ++c) {
      const float v = __fdiv_rn(px[c], den);
      if (v > best) best = v, arg = c;
    }
    return (T)arg;
  }
  const int x = e / C;
  const float v = __fdiv_rn(crow[e], __fmul_rn(ky, sx[x]));
  if (MODE == 0) return v;
  return (T)(uint8_t)(int)__fmul_rn(v, 255.f);
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void window_finish_kernel(const float* __restrict__ canvas, int h, int w, int C, float kf,
                                                            const float* __restrict__ sy, const float* __restrict__ sx,
                                                            typename WindowOut<MODE>::type* __restrict__ out, int64_t pitch) {
  typedef typename WindowOut<MODE>::type T;
  typedef Pack<T, VEC> P;
  const int rowlen = MODE == 2 ? w : w * C, vpr = (rowlen + VEC - 1) / VEC;
  const int64_t total = (int64_t)h * vpr;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int y = (int)(t / vpr);
    const int e0 = (int)(t - (int64_t)y * vpr) * VEC;
    const float* crow = canvas + (int64_t)y * w * C;
    const float ky = __fmul_rn(kf, sy[y]);           // (k * sy[y] * sx[x] is an exact integer below 2^24 in any order: the caller's check)
    T* dptr = out + (int64_t)y * pitch + e0;
    if (e0 + VEC <= rowlen) {
      P v;
#pragma unroll
      for (int j = 0; j < VEC; ++j) v.v[j] = window_finish_one<MODE>(crow, e0 + j, C, ky, sx);
      *reinterpret_cast<P*>(dptr) = v;
    } else {      // the row's tail: fewer than VEC elements left
      for (int j = 0; e0 + j < rowlen; ++j) dptr[j] = window_finish_one<MODE>(crow, e0 + j, C, ky, sx);
    }
  }
}

template <int MODE>
static void launch_window_finish(const float* canvas, int h, int w, int C, float kf, const float* sy, const float* sx, void* out, int64_t pitch,
                                 hipStream_t st) {
  typedef typename WindowOut<MODE>::type T;
  constexpr int VEC = 16 / (int)sizeof(T);
  const int rowlen = MODE == 2 ? w : w * C;
  if (aligned16(out) && pitch % VEC == 0) {
    hipLaunchKernelGGL((window_finish_kernel<MODE, VEC>), dim3(stream_grid((int64_t)h * ((rowlen + VEC - 1) / VEC))), dim3(256), 0, st, canvas, h, w,
                       C, kf, sy, sx, (T*)out, pitch);
  } else {
    hipLaunchKernelGGL((window_finish_kernel<MODE, 1>), dim3(stream_grid((int64_t)h * rowlen)), dim3(256), 0, st, canvas, h, w, C, kf, sy, sx,
                       (T*)out, pitch);
  }
}

extern "C" int stp_window_finish(const float* canvas, int32_t h, int32_t w, int32_t C, int32_t k, const float* sy, const float* sx, int32_t mode,
                                 void* out, int32_t out_ld, void* stream) {
  if (!canvas || !sy || !sx || !out || (const void*)canvas == out || h <= 0 || w <= 0 || C <= 0 || k <= 0 || mode < 0 || mode > 2 || out_ld < w)
    return STP_E_BADARG;
  if (mode == 2 && C > 32) return STP_E_BADARG;
  if ((int64_t)w * C > 0x7fffffff) return STP_E_BADARG;
  const int64_t pitch = mode == 2 ? (int64_t)out_ld : (int64_t)out_ld * C;      // destination elements between rows
  const float kf = (float)k;
  if (mode == 0) launch_window_finish<0>(canvas, h, w, C, kf, sy, sx, out, pitch, (hipStream_t)stream);
  else if (mode == 1) launch_window_finish<1>(canvas, h, w, C, kf, sy, sx, out, pitch, (hipStream_t)stream);
  else launch_window_finish<2>(canvas, h, w, C, kf, sy, sx, out, pitch, (hipStream_t)stream);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
