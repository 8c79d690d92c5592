// Gradient of the bilinear resize by an integer factor (resize.hip): seven forms - a slice copy, a separable two-pass reduction for tiny
// maps, a row-streaming and a row-pair tile kernel, the workgroup-per-pixel kernel in one pass or split over a workspace, a scalar
// gather - and THE statement of which one runs (resize_bwd_plan), asked by the launch, by the workspace query and by
// stp_resize_bilinear_bwd_form.
#include "stream_ops.h"
#include "launch.h"
#include <algorithm>
#include <cstdlib>

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

// ------------------------------------------------------------------------------------------
// THE decision: which form serves a call, and its launch geometry.  resize_bwd_plan walks the forms in a fixed order and the first
// that accepts wins; stp_resize_bilinear_bwd launches what the plan says, stp_resize_bilinear_bwd_form reports it, and the workspace
// query asks the same size functions (resize_bwd_tiny_shape / resize_bwd_tiny_bytes, split_bytes_either_width).
struct ResizeBwdPlan {
  int form;                      // STP_RESIZE_BWD_*
  int V;                         // channels per vector (vec_for): slice copy, block
  dim3 grid;                     // of the form's first launch
  size_t lds;
  int g2;                        // tiny: workgroups of the column pass
  int nvec;                      // rows: 16-byte vectors of an output row per thread
  int WS, CC;                    // tile: input columns and channels per workgroup
  int VL, rps, S, TLp, PPB;      // block: vector lanes, tap rows per split, splits, tap lanes per pixel, pixels per workgroup
};

// STP_RESIZE_BWD_TINY / _ROWS / _TILE = 0 switch a form off (A/B runs); each is read once per process
static bool resize_bwd_switch(const char* name) { return !(getenv(name) && atoi(getenv(name)) == 0); }

// the two-pass form: the shapes it is for, its workspace part[N][H * factor][W][C] (fp32), and the full eligibility
static bool resize_bwd_tiny_shape(int H, int W, int factor) { return factor >= 8 && W <= RBT_MAXW && H <= 16; }
static size_t resize_bwd_tiny_bytes(int N, int H, int W, int C, int factor) { return (size_t)N * H * factor * W * C * sizeof(float); }
static bool resize_bwd_tiny_ok(int N, int H, int W, int C, int factor, int ldo, int coff, int dtype) {
  static const bool on = resize_bwd_switch("STP_RESIZE_BWD_TINY");
  const int ev = dtype == STP_H16 ? 8 : 4;
  if (!on || !resize_bwd_tiny_shape(H, W, factor) || (C % ev) || (ldo % ev) || (coff % ev)) return false;
  const int cgv = C / ev;
  return cgv >= 1 && cgv <= 256 && (256 % cgv) == 0 && (size_t)(256 / cgv - 1) * W * C * sizeof(float) <= 64 * 1024 && (int64_t)N * H * factor < (1ll << 31);
}

static ResizeBwdPlan resize_bwd_plan(int N, int H, int W, int C, int factor, int ldo, int coff, int dtype, const void* dy, const void* dx,
                                     const void* workspace, size_t workspace_bytes) {
  ResizeBwdPlan p = {};
  const uintptr_t ady = reinterpret_cast<uintptr_t>(dy), adx = reinterpret_cast<uintptr_t>(dx);
  const int64_t npix = (int64_t)N * H * W;
  const int V = p.V = vec_for(dtype, C, ldo, coff);
  if (V > 1 && factor == 1) {      // a channel slice copied (or added) back
    p.form = STP_RESIZE_BWD_SLICE_COPY;
    p.grid = dim3(grid_for_amortised(npix * (C / V), 4));
    return p;
  }
  if (resize_bwd_tiny_ok(N, H, W, C, factor, ldo, coff, dtype) && workspace && workspace_bytes >= resize_bwd_tiny_bytes(N, H, W, C, factor) &&
      !(ady & 15)) {
    // tiny map, large factor (pyramid levels): separable two-pass reduction, every byte of dY read once
    const int ev = dtype == STP_H16 ? 8 : 4, cgv = C / ev, G = 256 / cgv;
    p.form = STP_RESIZE_BWD_TINY;
    p.grid = dim3((unsigned)(N * H * factor));
    p.lds = (size_t)(G - 1) * W * C * sizeof(float);
    p.g2 = (int)((npix * (C / 4) + 3) / 4);
    return p;
  }
  {
    // class logits (few channels, whole output rows fit an LDS buffer): the row-streaming kernel.  STP_RESIZE_BWD_ROWS=0: the gather kernel.
    static const bool rows_on = resize_bwd_switch("STP_RESIZE_BWD_ROWS");
    const int esz = dtype == STP_H16 ? 2 : 4, ev = 16 / esz;
    const int64_t rowB = (int64_t)W * factor * ldo * esz;
    const int nvec = (int)((rowB / 16 + 255) / 256);
    if (rows_on && factor >= 2 && !(C % ev) && !(ldo % ev) && !(coff % ev) && (int64_t)W * (C / ev) <= 512 && rowB <= 40960 && nvec <= 10 &&
        !(ady & 15) && !(adx & 15) && (int64_t)N * H < (1ll << 31)) {
      p.form = STP_RESIZE_BWD_ROWS;
      p.grid = dim3((unsigned)(N * H));
      p.lds = (size_t)(2 * rowB);
      p.nvec = nvec;
      return p;
    }
  }
  {
    // wide 16-bit channel slices (FPN's pyramid levels): the row-pair tile kernel.  STP_RESIZE_BWD_TILE=0: the gather kernel.
    static const bool tile_on = resize_bwd_switch("STP_RESIZE_BWD_TILE");
    const int WS = factor >= 64 ? 1 : 64 / (factor > 0 ? factor : 1), CC = C < 64 ? C : 64;
    const int cols = (WS + 1) * factor - 1;
    const size_t lds = (size_t)2 * cols * CC * sizeof(float);
    if (tile_on && V == 8 && factor >= 2 && C >= 32 && C % CC == 0 && cols * (CC / 8) <= 256 * RBT_K && lds <= 96 * 1024 &&
        (int64_t)N * ((H + 1) / 2) <= 65535 && C / CC <= 65535 && !(ady & 15) && !(adx & 7)) {
      p.form = STP_RESIZE_BWD_TILE;
      p.grid = dim3((unsigned)ceil_div(W, WS), (unsigned)(N * ((H + 1) / 2)), (unsigned)(C / CC));
      p.lds = lds;      // (cols * (CC / 8) <= 256 * RBT_K bounds it by 48 KB today; a larger RBT_K gets its grant from stp_launch_lds)
      p.WS = WS; p.CC = CC;
      return p;
    }
  }
  if (V > 1 && factor >= 2) {
    const int cg = C / V, span = 2 * factor;
    // few taps per pixel: wide channel chunks keep the tap lanes busy; many taps: 128-byte chunks and more workgroups
    const int VL = span * span >= 256 ? pool_vl(cg) : (cg < 32 ? cg : 32);
    SplitPlan sp = {span, 1, 0};
    if (VL == pool_vl(cg)) sp = split_plan_fit(split_plan(npix, C, cg, VL, span), span, workspace, workspace_bytes);
    // tap lanes per pixel: the largest power of two that the taps can keep busy; the rest of the workgroup takes more pixels
    int TLp = 1;
    while (TLp * 2 <= 256 / VL && TLp * 2 <= span * span) TLp *= 2;
    int PPB = (256 / VL) / TLp;
    if (sp.S > 1 || PPB < 1) { PPB = 1; TLp = 256 / VL; }
    p.form = sp.S > 1 ? STP_RESIZE_BWD_BLOCK_SPLIT : STP_RESIZE_BWD_BLOCK;
    p.grid = dim3((unsigned)ceil_div(npix, PPB), ceil_div(cg, VL), sp.S);
    p.lds = (size_t)(256 / VL) * VL * V * sizeof(float);
    p.VL = VL; p.rps = sp.rps; p.S = sp.S; p.TLp = TLp; p.PPB = PPB;
    return p;
  }
  p.form = STP_RESIZE_BWD_GATHER;
  p.grid = dim3(grid_for(npix * C));
  return p;
}

// fp32 workspace that lets every form run: the query knows neither dtype nor slice, so it sizes the tiny form's table for every shape
// the form is for, and the block form's split for either vector width
extern "C" size_t stp_resize_bilinear_bwd_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || factor < 2) return 0;
  const size_t tiny = resize_bwd_tiny_shape(H, W, factor) ? resize_bwd_tiny_bytes(N, H, W, C, factor) : 0;
  return std::max(tiny, split_bytes_either_width((int64_t)N * H * W, C, 2 * factor));
}

extern "C" int stp_resize_bilinear_bwd_form(const void* dy, const void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor,
                                            int32_t ldo, int32_t coff, int32_t dtype, const void* workspace, size_t workspace_bytes) {
  if (!resize_args_ok(dy, dx, N, H, W, C, factor, ldo, coff, dtype)) return STP_E_BADARG;
  return resize_bwd_plan(N, H, W, C, factor, ldo, coff, dtype, dy, dx, workspace, workspace_bytes).form;
}

extern "C" int stp_resize_bilinear_bwd(const void* dy, void* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t factor,
                                       int32_t ldo, int32_t coff, int32_t dtype, int32_t accumulate, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (!resize_args_ok(dy, dx, N, H, W, C, factor, ldo, coff, dtype)) return STP_E_BADARG;
  const ResizeBwdPlan p = resize_bwd_plan(N, H, W, C, factor, ldo, coff, dtype, dy, dx, workspace, workspace_bytes);
  const int64_t npix = (int64_t)N * H * W;
  hipStream_t s = (hipStream_t)stream;
  switch (p.form) {
    case STP_RESIZE_BWD_SLICE_COPY:
      return launch_tv(dtype, p.V == 8, [&](auto tv) {
        using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
        hipLaunchKernelGGL((slice_copy_kernel<T, V>), p.grid, dim3(256), 0, s, (const T*)dy, (T*)dx, npix, C, ldo, coff, accumulate);
      });
    case STP_RESIZE_BWD_TINY: {
      float* part = (float*)workspace;
      const int rc = launch_t(dtype, [&](auto tv) {
        using T = typename decltype(tv)::T;
        hipLaunchKernelGGL(resize_bilinear_bwd_tiny_rows_kernel<T>, p.grid, dim3(256), p.lds, s, (const T*)dy, part, H, W, C, factor, ldo, coff);
      });
      if (rc) return rc;
      return launch_t(dtype, [&](auto tv) {
        using T = typename decltype(tv)::T;
        hipLaunchKernelGGL(resize_bilinear_bwd_tiny_cols_kernel<T>, dim3(p.g2), dim3(256), 0, s, part, (T*)dx, N, H, W, C, factor, accumulate);
      });
    }
    case STP_RESIZE_BWD_ROWS:
      return launch_t(dtype, [&](auto tv) {
        using T = typename decltype(tv)::T;
        hipLaunchKernelGGL(resize_bilinear_bwd_rows_kernel<T>, p.grid, dim3(256), p.lds, s, (const T*)dy, (T*)dx, H, W, C, factor, ldo, coff, accumulate,
                           p.nvec);
      });
    case STP_RESIZE_BWD_TILE:
      return stp_launch_lds(resize_bilinear_bwd_tile_kernel<bf16_t>, p.grid, dim3(256), p.lds, s, (const bf16_t*)dy, (bf16_t*)dx, H, W, C, factor, ldo,
                            coff, accumulate, p.WS, p.CC);
    case STP_RESIZE_BWD_BLOCK:
    case STP_RESIZE_BWD_BLOCK_SPLIT: {
      float* part = p.S > 1 ? (float*)workspace : nullptr;
      const int rc = launch_tv(dtype, p.V == 8, [&](auto tv) {
        using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
        hipLaunchKernelGGL((resize_bilinear_bwd_blk_kernel<T, V>), p.grid, dim3(256), p.lds, s, (const T*)dy, (T*)dx, H, W, C, factor, ldo, coff,
                           accumulate, p.VL, p.rps, part, p.TLp, p.PPB, (int)npix);
      });
      if (rc || p.S <= 1) return rc;
      return split_combine_launch(part, p.S, npix * C, 1.f, dx, dtype, accumulate, s);
    }
    default:
      return launch_t(dtype, [&](auto tv) {
        using T = typename decltype(tv)::T;
        hipLaunchKernelGGL(resize_bilinear_bwd_kernel<T>, p.grid, dim3(256), 0, s, (const T*)dy, (T*)dx, N, H, W, C, factor, ldo, coff, accumulate);
      });
  }
}
