// Dihedral (D4) test-time augmentation on the device (segmentation_pipeline/segmentation.py: ttflips="d4"): the eight symmetries of
// the square applied to the uint8 input batch, and the running sum of the un-transformed probability maps.  uint8 and fp32 only
// (nothing here depends on the build's 16-bit storage format), no atomics, int64 element indices; every value is moved as it is or
// added with one __fadd_rn, so the device path equals the numpy statement (tests/_dihedral_reference.py) bit for bit.
//
// op 0..7 (include/stp_hip.h):  g_op(x) = transpose if op & 4, then columns reversed if op & 1, then rows reversed if op & 2.
// Both entry points are one gather, dst[n][i][j][:] (+)= src[n][sy][sx][:], with the destination Hd x Wd and the source Hs x Ws:
//   no transpose:  (Hs, Ws) = (Hd, Wd),  sy = RS ? Hs - 1 - i : i,  sx = CS ? Ws - 1 - j : j
//   transpose:     (Hs, Ws) = (Wd, Hd),  sy = RS ? Hs - 1 - j : j,  sx = CS ? Ws - 1 - i : i
// stp_predict_accumulate_dihedral (inv_op) has RS = op & 2, CS = op & 1.  stp_dihedral_u8 (g_op) has the same without a transpose;
// with one, the reversals act on the destination's axes, which are the source's other axes: RS = op & 1, CS = op & 2.
//
// Access width is predict.hip's rule: a thread owns VEC consecutive elements of one destination row and moves them with one 16-byte
// access where every row starts on a 16-byte boundary (base pointers aligned, row pitches a multiple of 16 bytes); otherwise one
// element per thread.
//
// The ops without a transpose, and the transposing ones on pixels of 256 bytes or more (C >= 64 floats), are a direct gather: a
// destination row's source is a row (read with 16-byte loads where the columns are not reversed) or a sequence of whole pixels, each a
// contiguous run that covers two cache lines or more (16-byte loads where the vector divides the pixel).
//
// The transposing ops on smaller pixels (1..7 bytes of input, 4..128 bytes of a map) move a tile of TP x TP pixels through LDS, so that
// both sides of global memory see contiguous runs of TP pixels: a block copies nj source rows of ni pixels into LDS as they lie (16-byte
// loads), then writes ni destination rows of nj pixels (16-byte stores), reading LDS down its columns.  TP is 64 pixels below 4 bytes per
// pixel, 32 below 16, 16 below 128, 8 below 256: every run is 64 bytes or more (64 only for C = 1 bytes) and a tile is at most 35 KB of
// LDS.  (Measured, DESIGN.md 3.34: the direct gather of 80-byte pixels, whose runs straddle the 128-byte lines, took 101 us where the
// tiles take 78 us and a flip of the same bytes 74 us.)
// The LDS row pitch is the row rounded up to 128 bytes (one sweep of the 32 banks) PLUS ONE PIXEL: the lanes of a column read, which
// walk (source row, channel), then fall on consecutive addresses modulo 128 bytes - consecutive banks instead of one.  The LDS
// accesses of a 16-byte chunk go element by element (lanes 4 dwords apart: a 4-way conflict; LDS time is not what bounds the kernel).
// Tiles that hang over the image's edge copy and write only their ni x nj part.
#include "common.h"

template <typename T, int VEC> struct alignas(sizeof(T) * VEC) Pack {
  T v[VEC];
};

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// MODE 0: no transpose, columns not reversed - VEC elements of a source row;  1: VEC divides C - VEC elements inside one source pixel;
// 2: element by element.  rows = N * Hd.
template <typename T, int VEC, bool ACCUMULATE, int MODE>
__global__ __launch_bounds__(256) void dihedral_gather_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t rows, int Hd, int Wd, int C,
                                                              int transpose, int rs, int cs) {
  typedef Pack<T, VEC> P;
  const int rowlen = Wd * C, vpr = rowlen / VEC;      // (VEC divides rowlen: the launcher's condition)
  const int Hs = transpose ? Wd : Hd, Ws = transpose ? Hd : Wd;
  const int64_t total = rows * vpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / vpr;
    const int e0 = (int)(i - r * vpr) * VEC;
    const int y = (int)(r % Hd);
    const T* simg = src + (r / Hd) * ((int64_t)Hd * rowlen);
    T* dptr = dst + r * rowlen + e0;
    P v;
    if (MODE == 0) {
      v = *reinterpret_cast<const P*>(simg + (int64_t)(rs ? Hd - 1 - y : y) * rowlen + e0);
    } else {
      int x = e0 / C, c = e0 - x * C;
#pragma unroll
      for (int j = 0; j < (MODE == 1 ? 1 : VEC); ++j) {
        const int a = transpose ? x : y, b = transpose ? y : x;
        const T* p = simg + ((int64_t)(rs ? Hs - 1 - a : a) * Ws + (cs ? Ws - 1 - b : b)) * C + c;
        if (MODE == 1) {
          v = *reinterpret_cast<const P*>(p);
        } else {
          v.v[j] = *p;
          if (++c == C) c = 0, ++x;
        }
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

// The transposing ops through LDS.  A block takes destination tiles [i0, i0 + ni) x [j0, j0 + nj) of image n; pitch is the LDS row
// pitch in elements.  VEC > 1: every source and destination row starts on a 16-byte boundary and is a whole number of 16-byte chunks,
// and so is every tile's run in it (TP * C * sizeof(T) is a multiple of 16, so a ragged tile's run is one too; its reversed run
// starts at column 0).
template <typename T, int VEC, bool ACCUMULATE>
__global__ __launch_bounds__(256) void dihedral_tile_kernel(const T* __restrict__ src, T* __restrict__ dst, int64_t tiles, int Hd, int Wd, int C,
                                                            int TP, int pitch, int rs, int cs) {
  extern __shared__ __align__(16) unsigned char lds_bytes[];
  T* lds = reinterpret_cast<T*>(lds_bytes);
  typedef Pack<T, VEC> P;
  const int Hs = Wd, Ws = Hd;
  const int tiles_j = (Wd + TP - 1) / TP, tiles_i = (Hd + TP - 1) / TP;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t q = tile / tiles_j;
    const int j0 = (int)(tile - q * tiles_j) * TP, i0 = (int)(q % tiles_i) * TP;
    const int64_t n = q / tiles_i;
    const int ni = min(TP, Hd - i0), nj = min(TP, Wd - j0);
    // source rows sy(j0 + dj), dj < nj, columns xlo .. xlo + ni - 1 -> lds[dj][0 .. ni * C) as they lie
    const int xlo = cs ? Ws - i0 - ni : i0;
    const int scpr = ni * C / VEC;
    for (int t = threadIdx.x; t < nj * scpr; t += 256) {
      const int dj = t / scpr, e0 = (t - dj * scpr) * VEC;
      const int sy = rs ? Hs - 1 - (j0 + dj) : j0 + dj;
      const T* g = src + ((n * Hs + sy) * Ws + xlo) * C + e0;
      T* l = lds + dj * pitch + e0;
      const P v = *reinterpret_cast<const P*>(g);
#pragma unroll
      for (int j = 0; j < VEC; ++j) l[j] = v.v[j];
    }
    __syncthreads();
    // destination rows i0 + di, di < ni, columns j0 .. j0 + nj - 1 <- lds[dj][pixel di (reversed: ni - 1 - di)]
    const int dcpr = nj * C / VEC;
    for (int t = threadIdx.x; t < ni * dcpr; t += 256) {
      const int di = t / dcpr, e0 = (t - di * dcpr) * VEC;
      T* g = dst + ((n * Hd + i0 + di) * Wd + j0) * C + e0;
      int dj = e0 / C, c = e0 - dj * C;
      const T* l = lds + (cs ? ni - 1 - di : di) * C;
      P v;
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        v.v[j] = l[dj * pitch + c];
        if (++c == C) c = 0, ++dj;
      }
      if (ACCUMULATE) {
        const P a = *reinterpret_cast<const P*>(g);
#pragma unroll
        for (int j = 0; j < VEC; ++j) v.v[j] = (T)__fadd_rn((float)a.v[j], (float)v.v[j]);
      }
      *reinterpret_cast<P*>(g) = v;
    }
    __syncthreads();      // (the next tile overwrites the LDS rows)
  }
}

static inline int capped_grid(int64_t blocks) { return (int)(blocks > 65536 ? 65536 : blocks); }

// dst [N][Hd][Wd][C] (+)= the gather of src described at the top.
template <typename T, bool ACCUMULATE>
static void launch_dihedral(const T* src, T* dst, int64_t N, int Hd, int Wd, int C, bool transpose, int rs, int cs, hipStream_t st) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const int Ws = transpose ? Hd : Wd;
  const int64_t rows = N * Hd;
  const int rowlen = Wd * C, pixel_bytes = C * (int)sizeof(T);
  const bool vec = rowlen % VEC == 0 && aligned16(src) && aligned16(dst);
  if (!transpose || pixel_bytes >= 256) {
    const int mode = (!transpose && !cs) ? 0 : (vec && C % VEC == 0 ? 1 : 2);
    void (*kernel)(const T*, T*, int64_t, int, int, int, int, int, int) =
        vec ? (mode == 0   ? dihedral_gather_kernel<T, VEC, ACCUMULATE, 0>
               : mode == 1 ? dihedral_gather_kernel<T, VEC, ACCUMULATE, 1>
                           : dihedral_gather_kernel<T, VEC, ACCUMULATE, 2>)
            : (mode == 0 ? dihedral_gather_kernel<T, 1, ACCUMULATE, 0> : dihedral_gather_kernel<T, 1, ACCUMULATE, 2>);
    const int64_t items = vec ? rows * (rowlen / VEC) : rows * rowlen;
    hipLaunchKernelGGL(kernel, dim3(capped_grid((items + 255) / 256)), dim3(256), 0, st, src, dst, rows, Hd, Wd, C, (int)transpose, rs, cs);
    return;
  }
  const int TP = pixel_bytes < 4 ? 64 : (pixel_bytes < 16 ? 32 : (pixel_bytes < 128 ? 16 : 8));
  const int pitch = (TP * pixel_bytes + 127) / 128 * 128 / (int)sizeof(T) + C;      // elements: whole bank sweeps plus one pixel
  const int64_t tiles = N * ((Hd + TP - 1) / TP) * ((Wd + TP - 1) / TP);
  const size_t lds = (size_t)TP * pitch * sizeof(T);
  const bool vec2 = vec && ((int64_t)Ws * C) % VEC == 0 && (TP * C) % VEC == 0;
  void (*kernel)(const T*, T*, int64_t, int, int, int, int, int, int, int) =
      vec2 ? dihedral_tile_kernel<T, VEC, ACCUMULATE> : dihedral_tile_kernel<T, 1, ACCUMULATE>;
  hipLaunchKernelGGL(kernel, dim3(capped_grid(tiles)), dim3(256), lds, st, src, dst, tiles, Hd, Wd, C, TP, pitch, rs, cs);
}

static inline bool dihedral_args_ok(const void* a, const void* b, int32_t N, int32_t H, int32_t W, int32_t C, int32_t op) {
  if (!a || !b || a == b || N <= 0 || H <= 0 || W <= 0 || C <= 0 || op < 0 || op > 7) return false;
  return (int64_t)W * C <= 0x7fffffff && (int64_t)H * C <= 0x7fffffff;
}

extern "C" int stp_dihedral_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t C, int32_t op, void* stream) {
  if (!dihedral_args_ok(src, dst, N, H, W, C, op)) return STP_E_BADARG;
  const bool t = (op & 4) != 0;      // the destination is [N][W][H][C] then, and its reversals are the source's other axes'
  launch_dihedral<uint8_t, false>(src, dst, N, t ? W : H, t ? H : W, C, t, t ? (op & 1) : (op >> 1 & 1), t ? (op >> 1 & 1) : (op & 1),
                                  (hipStream_t)stream);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_predict_accumulate_dihedral(const float* probs, float* acc, int32_t N, int32_t H, int32_t W, int32_t C, int32_t op,
                                               void* stream) {
  if (!dihedral_args_ok(probs, acc, N, H, W, C, op)) return STP_E_BADARG;
  launch_dihedral<float, true>(probs, acc, N, H, W, C, (op & 4) != 0, op >> 1 & 1, op & 1, (hipStream_t)stream);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
