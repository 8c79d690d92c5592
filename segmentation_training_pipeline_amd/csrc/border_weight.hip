// U-Net border weight maps (include/stp_hip.h has the arithmetic): per pixel the squared distances to the nearest and to the
// second-nearest object inside a (2R + 1)^2 window of its own sample, then w = class balance + w0 exp(-(d1 + d2)^2 / 2 sigma^2) on the
// background.  Separable and exact, two launches over the whole batch:
//   bw_rows_kernel  a workgroup owns 256 pixels of one row and holds them with an R-pixel halo in LDS; a pixel walks |dx| = 0 .. R
//                   outwards (left before right) and keeps the first labelled pixel (dxA, labelA) and the first one with another label
//                   (dxB).  8 bytes per pixel in the workspace: labelA, dxA | dxB << 8 (BW_NONE = no such pixel).
//   bw_cols_kernel  a workgroup owns 64 columns x BW_TILE_ROWS rows of ONE sample and holds the candidates of those columns with an
//                   R-row halo in LDS (6 bytes per cell, (32 + 2 * 32) x 64 cells = 36 KiB at the largest radius: four workgroups per
//                   CU).  Rows outside the sample are staged as BW_NONE, so the scans need no clipping and never see the neighbouring
//                   sample.  A pixel scans dy = -R .. R twice: (D1^2, L1) from the A candidates, then per row dxA if labelA != L1, else
//                   dxB.  A wave reads 64 consecutive cells of one LDS row: no bank conflict.
// int32 and fp32 only: both builds export the same code.  No atomics, no workgroup reads what another writes within a launch.
#include "common.h"
#include <math.h>

#define BW_THREADS 256
#define BW_MAX_RADIUS 32
#define BW_NONE 255u                  // a byte distance: no such pixel within the radius
#define BW_TILE_COLS 64
#define BW_TILE_ROWS 32
#define BW_BIG 0x7fffffff

__global__ __launch_bounds__(BW_THREADS) void bw_rows_kernel(const int* __restrict__ labels, int W, int segs, int R, int2* __restrict__ cand) {
  __shared__ int lab[BW_THREADS + 2 * BW_MAX_RADIUS];
  const int seg = (int)(blockIdx.x % (unsigned)segs);
  const int64_t row = blockIdx.x / (unsigned)segs;          // 0 .. N * H
  const int x0 = seg * BW_THREADS;
  const int* src = labels + row * W;
  for (int i = threadIdx.x; i < BW_THREADS + 2 * R; i += BW_THREADS) {
    const int x = x0 - R + i;
    lab[i] = (x >= 0 && x < W) ? src[x] : 0;
  }
  __syncthreads();
  const int x = x0 + (int)threadIdx.x;
  if (x >= W) return;
  const int c = R + (int)threadIdx.x;
  unsigned dA = BW_NONE, dB = BW_NONE;
  int lA = 0;
  for (int dx = 0; dx <= R; ++dx) {
    const int l = lab[c - dx], r = lab[c + dx];
    if (l > 0) {
      if (dA == BW_NONE) { dA = (unsigned)dx; lA = l; }
      else if (l != lA && dB == BW_NONE) dB = (unsigned)dx;
    }
    if (dx && r > 0) {
      if (dA == BW_NONE) { dA = (unsigned)dx; lA = r; }
      else if (r != lA && dB == BW_NONE) dB = (unsigned)dx;
    }
    if (dB != BW_NONE) break;
  }
  cand[row * W + x] = make_int2(lA, (int)(dA | (dB << 8)));
}

__global__ __launch_bounds__(BW_THREADS) void bw_cols_kernel(const int2* __restrict__ cand, int H, int W, int tiles_x, int tiles_y, int R,
                                                             float w0, float inv_2s2, float b0, float b1, float* __restrict__ weights,
                                                             int* __restrict__ d1sq, int* __restrict__ d2sq) {
  extern __shared__ __attribute__((aligned(16))) char bw_smem[];
  const int rows = BW_TILE_ROWS + 2 * R;
  int* lA = reinterpret_cast<int*>(bw_smem);                                        // [rows][64]
  uint16_t* pk = reinterpret_cast<uint16_t*>(bw_smem + (size_t)rows * BW_TILE_COLS * sizeof(int));   // [rows][64]: dxA | dxB << 8
  const int tx = (int)(blockIdx.x % (unsigned)tiles_x);
  const int ty = (int)((blockIdx.x / (unsigned)tiles_x) % (unsigned)tiles_y);
  const int64_t n = blockIdx.x / ((unsigned)tiles_x * (unsigned)tiles_y);
  const int x0 = tx * BW_TILE_COLS, y0 = ty * BW_TILE_ROWS;
  const int64_t base = n * H * (int64_t)W;
  for (int i = threadIdx.x; i < rows * BW_TILE_COLS; i += BW_THREADS) {
    const int r = i / BW_TILE_COLS, c = i % BW_TILE_COLS;
    const int y = y0 - R + r, x = x0 + c;
    int2 v = make_int2(0, (int)(BW_NONE | (BW_NONE << 8)));
    if (y >= 0 && y < H && x < W) v = cand[base + (int64_t)y * W + x];
    lA[i] = v.x;
    pk[i] = (uint16_t)v.y;
  }
  __syncthreads();
  const int c = threadIdx.x & (BW_TILE_COLS - 1), g = threadIdx.x / BW_TILE_COLS;
  const int x = x0 + c;
  if (x >= W) return;
  for (int k = 0; k < BW_TILE_ROWS / (BW_THREADS / BW_TILE_COLS); ++k) {
    const int ly = g + k * (BW_THREADS / BW_TILE_COLS);       // row of the tile
    const int y = y0 + ly;
    if (y >= H) break;
    const int centre = (ly + R) * BW_TILE_COLS + c;
    int best1 = BW_BIG, l1 = 0;
    for (int dy = -R; dy <= R; ++dy) {
      const int i = centre + dy * BW_TILE_COLS;
      const unsigned a = pk[i] & 255u;
      if (a != BW_NONE) {
        const int v = dy * dy + (int)(a * a);
        if (v < best1) { best1 = v; l1 = lA[i]; }
      }
    }
    int best2 = BW_BIG;
    if (best1 != BW_BIG) {
      for (int dy = -R; dy <= R; ++dy) {
        const int i = centre + dy * BW_TILE_COLS;
        const unsigned p = pk[i], a = p & 255u, b = p >> 8;
        const unsigned d = (a != BW_NONE && lA[i] != l1) ? a : b;
        if (d != BW_NONE) best2 = min(best2, dy * dy + (int)(d * d));
      }
    }
    const bool fg = (pk[centre] & 255u) == 0u;               // a labelled pixel is its own nearest pixel of the row
    float term = 0.f;
    if (!fg && best2 != BW_BIG) {
      const float s = sqrtf((float)best1) + sqrtf((float)best2);
      term = w0 * expf(-(s * s) * inv_2s2);
    }
    const int64_t o = base + (int64_t)y * W + x;
    weights[o] = (fg ? b1 : b0) + term;
    if (d1sq) d1sq[o] = best1 == BW_BIG ? -1 : best1;
    if (d2sq) d2sq[o] = best2 == BW_BIG ? -1 : best2;
  }
}

static inline bool bw_sizes_ok(int32_t N, int32_t H, int32_t W) {
  return N >= 1 && H >= 1 && W >= 1 && (int64_t)N * H * W < ((int64_t)1 << 31);
}
static inline size_t bw_workspace_bytes(int64_t pixels) { return (size_t)((pixels * 8 + 15) / 16 * 16); }

extern "C" size_t stp_border_weight_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  return bw_sizes_ok(N, H, W) ? bw_workspace_bytes((int64_t)N * H * W) : 0;
}

extern "C" int stp_border_weight(const int32_t* labels, int32_t N, int32_t H, int32_t W, float w0, float sigma, int32_t radius, float b0, float b1,
                                 float* weights, int32_t* d1sq, int32_t* d2sq, void* workspace, size_t workspace_bytes, void* stream) {
  if (!labels || !weights || !workspace || !bw_sizes_ok(N, H, W) || radius < 1 || radius > BW_MAX_RADIUS) return STP_E_BADARG;
  if (!isfinite(w0) || !isfinite(sigma) || !isfinite(b0) || !isfinite(b1) || w0 < 0.f || sigma <= 0.f || b0 <= 0.f || b1 <= 0.f) return STP_E_BADARG;
  const float inv_2s2 = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
  if (!isfinite(inv_2s2)) return STP_E_BADARG;                // a sigma whose 1 / 2 sigma^2 leaves fp32
  const int64_t pixels = (int64_t)N * H * W;
  if (((uintptr_t)workspace & 7) != 0 || workspace_bytes < bw_workspace_bytes(pixels)) return STP_E_WORKSPACE;
  const int64_t segs = (W + BW_THREADS - 1) / BW_THREADS, row_blocks = (int64_t)N * H * segs;
  const int64_t tiles_x = (W + BW_TILE_COLS - 1) / BW_TILE_COLS, tiles_y = (H + BW_TILE_ROWS - 1) / BW_TILE_ROWS;
  const int64_t col_blocks = (int64_t)N * tiles_x * tiles_y;
  if (row_blocks >= ((int64_t)1 << 31) || col_blocks >= ((int64_t)1 << 31)) return STP_E_BADARG;      // (N * H * W < 2^31 already bounds both)
  hipStream_t st = (hipStream_t)stream;
  int2* cand = (int2*)workspace;
  hipLaunchKernelGGL(bw_rows_kernel, dim3((unsigned)row_blocks), dim3(BW_THREADS), 0, st, labels, W, (int)segs, radius, cand);
  STP_LAUNCH_CHECK();
  const size_t lds = (size_t)(BW_TILE_ROWS + 2 * radius) * BW_TILE_COLS * (sizeof(int) + sizeof(uint16_t));
  hipLaunchKernelGGL(bw_cols_kernel, dim3((unsigned)col_blocks), dim3(BW_THREADS), lds, st, cand, H, W, (int)tiles_x, (int)tiles_y, radius, w0,
                     inv_2s2, b0, b1, weights, d1sq, d2sq);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
