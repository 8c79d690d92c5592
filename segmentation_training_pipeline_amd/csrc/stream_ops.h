// Shared pieces of the HBM-bound streaming units bn.hip, pool.hip, upsample2x.hip, resize.hip, resize_bwd.hip and elementwise.hip: the
// vector load / store helpers, the per-channel partial-sum kernel and its fixed-order reduction, the grid rules, the one statement of the
// storage-type / vector-width dispatch, the one statement of a tap reduction split over a workspace (SplitPlan), and both sides (device tail, host launch pieces) of the gradient passes that complete a BatchNormalization
// backward.  Everything here is a template, __forceinline__ or static inline: a unit that includes it gets only what it uses.
#pragma once
#include "common.h"

#define BN_MAX_BLOCKS 1024
#ifndef POOL_ROWS
#define POOL_ROWS 4  // image rows per workgroup of the max-pool kernels (one row per workgroup = 8-32 K tiny workgroups: dispatch-bound)
#endif

// ------------------------------------------------------------------------------------------
// Host dispatch on storage type and vector width - THE statement of the rule: 16-bit storage whose channel counts (and whatever
// else the call site needs, e.g. a row pitch) are multiples of 8 takes <bf16_t, 8> (one 16-byte vector), other 16-bit storage
// <bf16_t, 4>, fp32 <float, 4>.  The caller computes `v8` (true only for 16-bit storage) and passes a generic lambda holding ONE launch:
//   return launch_tv(dtype, v8, [&](auto tv) {
//     using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
//     hipLaunchKernelGGL((kernel<T, V>), grid, dim3(256), 0, s, (const T*)x, (T*)y, ...);
//   });
// Returns STP_E_BADARG for a dtype that is neither (nothing is launched), STP_E_LAUNCH if the launch failed, else STP_OK.
template <typename T_, int V_> struct ElemVec { using T = T_; static constexpr int V = V_; };
template <typename F> static inline int launch_tv(int dtype, bool v8, F&& launch) {
  if (v8) launch(ElemVec<bf16_t, 8>{});
  else if (dtype == STP_H16) launch(ElemVec<bf16_t, 4>{});
  else if (dtype == STP_F32) launch(ElemVec<float, 4>{});
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}
// ... and for the kernels that only choose the storage type (V is not meaningful there)
template <typename F> static inline int launch_t(int dtype, F&& launch) {
  if (dtype == STP_H16) launch(ElemVec<bf16_t, 1>{});
  else if (dtype == STP_F32) launch(ElemVec<float, 1>{});
  else return STP_E_BADARG;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

template <typename T> __device__ __forceinline__ f32x4 ld4(const T* p);
template <> __device__ __forceinline__ f32x4 ld4<float>(const float* p) { return load4(p); }
template <> __device__ __forceinline__ f32x4 ld4<bf16_t>(const bf16_t* p) { return load4(p); }

// V consecutive channels <-> float[V]; V*sizeof(T) is 8 or 16 bytes
template <typename T, int V> __device__ __forceinline__ void ldv(const T* p, float (&o)[V]) {
  if constexpr (V == 4) {
    const f32x4 v = ld4<T>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else {  // 8 bf16 = one 16-byte load
    const u32x4 r = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) { o[2 * e] = h16lo_to_f32(r[e]); o[2 * e + 1] = h16hi_to_f32(r[e]); }
  }
}
template <typename T, int V> __device__ __forceinline__ void stv(T* p, const float (&o)[V]) {
  if constexpr (V == 4) {
    store4(p, f32x4{o[0], o[1], o[2], o[3]});
  } else {
    u32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = pack_bf16x2(o[2 * e], o[2 * e + 1]);
    *reinterpret_cast<u32x4*>(p) = r;
  }
}

// ------------------------------------------------------------------------------------------
// statistics: partial[block][0][c] = sum x, partial[block][1][c] = sum x^2 over the block's rows
// Each thread owns V consecutive channels (16 bytes for bf16 V=8 / fp32 V=4) and strides over rows with 4
// independent loads in flight; row lanes are then combined through LDS in a fixed order.
template <typename T, int V>
__global__ __launch_bounds__(256) void bn_partial_kernel(const T* __restrict__ x, int64_t rows, int C, float* partial) {
  extern __shared__ float red[];  // [256][2V]
  const int cg = C / V;
  const int colsPerPass = cg < 256 ? cg : 256;
  const int rowLanes = 256 / colsPerPass;
  const int tcol = threadIdx.x % colsPerPass, trow = threadIdx.x / colsPerPass;
  const int64_t rowsPerBlock = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rowsPerBlock;
  const int64_t r1 = r0 + rowsPerBlock < rows ? r0 + rowsPerBlock : rows;
  for (int c0 = 0; c0 < cg; c0 += colsPerPass) {
    const int c = c0 + tcol;
    float s[V], q[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = q[e] = 0.f;
    if (c < cg && trow < rowLanes) {
      const T* base = x + (size_t)c * V;
      int64_t r = r0 + trow;
      for (; r + 3 * (int64_t)rowLanes < r1; r += 4 * (int64_t)rowLanes) {
        float v0[V], v1[V], v2[V], v3[V];
        ldv<T, V>(base + r * C, v0);
        ldv<T, V>(base + (r + rowLanes) * C, v1);
        ldv<T, V>(base + (r + 2 * (int64_t)rowLanes) * C, v2);
        ldv<T, V>(base + (r + 3 * (int64_t)rowLanes) * C, v3);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          s[e] += (v0[e] + v1[e]) + (v2[e] + v3[e]);
          q[e] += (v0[e] * v0[e] + v1[e] * v1[e]) + (v2[e] * v2[e] + v3[e] * v3[e]);
        }
      }
      for (; r < r1; r += rowLanes) {
        float v0[V];
        ldv<T, V>(base + r * C, v0);
#pragma unroll
        for (int e = 0; e < V; ++e) { s[e] += v0[e]; q[e] += v0[e] * v0[e]; }
      }
    }
    const int slot = (trow * colsPerPass + tcol) * 2 * V;
#pragma unroll
    for (int e = 0; e < V; ++e) { red[slot + e] = s[e]; red[slot + V + e] = q[e]; }
    __syncthreads();
    if (trow == 0 && c < cg) {
      float a[2 * V];
#pragma unroll
      for (int e = 0; e < 2 * V; ++e) a[e] = 0.f;
      for (int t = 0; t < rowLanes; ++t)
#pragma unroll
        for (int e = 0; e < 2 * V; ++e) a[e] += red[(t * colsPerPass + tcol) * 2 * V + e];
      float* p = partial + (size_t)blockIdx.x * 2 * C;
#pragma unroll
      for (int e = 0; e < V; ++e) { p[c * V + e] = a[e]; p[C + c * V + e] = a[V + e]; }
    }
    __syncthreads();
  }
}

// Sums partial[b][which][c] over b for 4 consecutive channels per workgroup: 64 strided lanes per
// channel (independent loads in flight), then a fixed-shape LDS tree -> deterministic.
// Returns the totals (valid on lane 0 of each channel column) for `which` = 0 and 1.
struct Sum2 { double s, q; };
__device__ __forceinline__ Sum2 reduce_partials(const float* partial, int blocks, int C, int c, bool want_q) {
  __shared__ double sh[2][64][4];
  const int cc = threadIdx.x & 3, lane = threadIdx.x >> 2;
  double s = 0.0, q = 0.0;
  if (c < C)
    for (int b = lane; b < blocks; b += 64) {
      s += (double)partial[(size_t)b * 2 * C + c];
      if (want_q) q += (double)partial[(size_t)b * 2 * C + C + c];
    }
  sh[0][lane][cc] = s;
  sh[1][lane][cc] = q;
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) {
    if (lane < w) {
      sh[0][lane][cc] += sh[0][lane + w][cc];
      sh[1][lane][cc] += sh[1][lane + w][cc];
    }
    __syncthreads();
  }
  Sum2 r;
  r.s = sh[0][0][cc];
  r.q = sh[1][0][cc];
  return r;
}

static inline int bn_blocks(int64_t rows) {
  int64_t b = rows / 64;
  if (b < 1) b = 1;
  if (b > BN_MAX_BLOCKS) b = BN_MAX_BLOCKS;
  return (int)b;
}
// bn_partial_kernel over x[rows][C] (C % 4 == 0) with `blocks` workgroups: stp_bn_stats and stp_channel_sum
static inline int bn_partial_launch(const void* x, int dtype, int64_t rows, int C, int blocks, float* partial, hipStream_t s) {
  return launch_tv(dtype, dtype == STP_H16 && (C & 7) == 0, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((bn_partial_kernel<T, V>), dim3(blocks), dim3(256), 256 * 2 * V * sizeof(float), s, (const T*)x, rows, C, partial);
  });
}

// a grid whose stride (grid x 256) is a multiple of `groups`, close to (and not above) `want` blocks; 0 if none
static inline int grid_multiple_of(int want, int groups);
static inline int grid_fixed_channels(int want, int groups) {   // prefer a grid that keeps every thread on one channel group
  const int g = grid_multiple_of(want, groups);
  return g > 0 ? g : want;
}
static inline int grid_multiple_of(int want, int groups) {
  // grid * 256 % groups == 0  <=>  grid % (groups / gcd(groups, 256)) == 0
  int a = groups, b = 256;
  while (b) { const int t = a % b; a = b; b = t; }
  const int q = groups / a;
  const int g = want / q * q;
  return g >= 1 ? g : 0;
}

static inline int grid_for(int64_t items) {
  int64_t b = (items + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}
// elementwise BatchNormalization passes with per-thread channel constants: at least `per_thread` vectors per thread once every CU
// has two workgroups, so the constant set-up is amortised (a thread with one vector spends most of its life fetching constants)
static inline int grid_for_amortised(int64_t items, int per_thread) {
  int64_t b = (items + 255) / 256;
  const int64_t lean = (items + 256 * (int64_t)per_thread - 1) / (256 * (int64_t)per_thread);
  if (b > 512) b = lean > 512 ? lean : 512;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

// vector width shared by the pooling / resize kernels: 16-byte (bf16 x8, fp32 x4) or 8-byte (bf16 x4) channel groups
static inline int vec_for(int dtype, int a, int b, int c) {
  const int m = a | b | c;
  if (dtype == STP_H16 && !(m & 7)) return 8;
  return (m & 3) ? 1 : 4;
}

// the argument checks that open the bilinear / nearest resize entry points and their gradients (a, b: the two tensors; the dtype test
// refuses the other build's 16-bit code, or garbage)
static inline bool resize_args_ok(const void* a, const void* b, int N, int H, int W, int C, int factor, int ldo, int coff, int dtype) {
  return stp_dtype_ok(dtype) && a && b && N > 0 && H > 0 && W > 0 && C > 0 && factor >= 1 && ldo >= coff + C && coff >= 0;
}

static inline int pool_vl(int cg) { return cg < 8 ? cg : 8; }   // 8 vector lanes = 128 contiguous bytes per pixel and workgroup

// second stage of a split reduction: dst[i] (+)= scale * sum_s part[s][i], s in ascending order
template <typename T>
__global__ __launch_bounds__(256) void split_combine_kernel(const float* __restrict__ part, int S, int64_t n, float scale, T* __restrict__ dst,
                                                            int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float sum = 0.f;
  for (int q = 0; q < S; ++q) sum += part[(int64_t)q * n + i];
  sum *= scale;
  if (accumulate) sum += Elem<T>::load(dst + i);
  Elem<T>::store(dst + i, sum);
}
static inline int split_combine_launch(const float* part, int S, int64_t n, float scale, void* dst, int dtype, int accumulate, hipStream_t s) {
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL(split_combine_kernel<T>, dim3((unsigned)ceil_div(n, (int64_t)256)), dim3(256), 0, s, part, S, n, scale, (T*)dst, accumulate);
  });
}

// rows-per-split of a reduction over `rows` x `cols` taps done by `blocks` workgroups: split until >= 1024 workgroups exist
static inline int split_rows(int64_t blocks, int rows, int cols) {
  if (blocks >= 1024 || (int64_t)rows * cols < 1024) return rows;
  const int want = (int)ceil_div((int64_t)1024, blocks);
  const int rps = (int)ceil_div(rows, want < rows ? want : rows);
  return rps < 1 ? 1 : rps;
}

// THE statement of the split of a rows x rows tap reduction (an average-pooling window, the (2f)^2 taps of a resize gradient) over a
// workspace: `items` outputs (windows, input pixels) of C channels in cg vector groups, VL of them per workgroup -> rows per split,
// splits, and the bytes of the fp32 table part[S][items][C] that the splits write and split_combine_launch sums.
struct SplitPlan { int rps, S; size_t bytes; };
static inline SplitPlan split_plan(int64_t items, int C, int cg, int VL, int rows) {
  SplitPlan p;
  p.rps = split_rows(items * ceil_div(cg, VL), rows, rows);
  p.S = ceil_div(rows, p.rps);
  p.bytes = (size_t)p.S * items * C * sizeof(float);
  return p;
}
// no workspace, or one too small for the table: one pass that writes the destination itself
static inline SplitPlan split_plan_fit(SplitPlan p, int rows, const void* workspace, size_t workspace_bytes) {
  if (p.S > 1 && (!workspace || workspace_bytes < p.bytes)) { p.rps = rows; p.S = 1; p.bytes = 0; }
  return p;
}
// what a *_workspace_bytes query that does not know the dtype answers: the larger table of either vector width the launch may pick
// (channel counts that neither width divides are counted in rounded-up groups); 0 where neither splits
static inline size_t split_bytes_either_width(int64_t items, int C, int rows) {
  size_t need = 0;
  for (int V = 4; V <= 8; V += 4) {
    const int cg = ceil_div(C, V);
    const SplitPlan p = split_plan(items, C, cg, pool_vl(cg), rows);
    if (p.S > 1) need = need > p.bytes ? need : p.bytes;
  }
  return need;
}

// ------------------------------------------------------------------------------------------
// Shared tail of the gradient kernels that COMPLETE the gradient of a BatchNormalization(+activation) output (the 2x2 fold of
// UpSampling2D, the max-pool gather): the thread's V values are masked with the activation re-derived from the BN input x,
// stored, and the workgroup reduces sum(g) / sum(g * xhat) per channel into partial[2][C][workgroups] - the layout
// stp_bn_backward_fused consumes, exactly what the convolution epilogues write (stp_conv_params.bnb_x).
// Thread layout of the callers: t = blockIdx.x * 256 + threadIdx.x = pixel * cg + channel group, cg = C / V dividing 256.
__device__ __forceinline__ f32x4 stored4(f32x4 v, const float*) { return v; }   // the value as the destination dtype holds it
__device__ __forceinline__ f32x4 stored4(f32x4 v, const bf16_t*) {
  const uint32_t a = pack_bf16x2(v.x, v.y), b = pack_bf16x2(v.z, v.w);
  return f32x4{h16lo_to_f32(a), h16hi_to_f32(a), h16lo_to_f32(b), h16hi_to_f32(b)};
}

#define BNB_ROWS 8   // image rows per workgroup of the *_bn gradient kernels: fewer, larger partial-sum tiles


template <typename T, int V>
__device__ __forceinline__ void bnb_mask_store(float (&g)[V], size_t o, int c, const BnBack& bnb, T* __restrict__ dx, float (&sg)[V],
                                               float (&sq)[V]) {
  float xv[V];
  ldv<T, V>(reinterpret_cast<const T*>(bnb.x) + o, xv);
#pragma unroll
  for (int q = 0; q < V / 4; ++q) {
    const BnBackCh k = bnback_load(bnb, c + 4 * q);
    const f32x4 st = stored4(f32x4{g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]}, (const T*)nullptr);
    f32x4 s4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
    const f32x4 m = bnback_apply(k, bnb.relu, f32x4{xv[4 * q], xv[4 * q + 1], xv[4 * q + 2], xv[4 * q + 3]}, st, s4, q4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { g[4 * q + e] = m[e]; sg[4 * q + e] += s4[e]; sq[4 * q + e] += q4[e]; }
  }
  stv<T, V>(dx + o, g);
}

// threads t and t + cg own the same channels: fixed-order combine over the workgroup's 256 / cg pixel columns
template <int V>
__device__ __forceinline__ void bnb_reduce(const float (&sg)[V], const float (&sq)[V], int cg, int C, float* __restrict__ partial) {
  extern __shared__ float red[];  // [256][2V]
#pragma unroll
  for (int e = 0; e < V; ++e) { red[threadIdx.x * 2 * V + e] = sg[e]; red[threadIdx.x * 2 * V + V + e] = sq[e]; }
  __syncthreads();
  const int cl = cg < 256 ? cg : 256;               // channel groups present in this workgroup
  for (int idx = threadIdx.x; idx < cl * V; idx += 256) {
    const int gq = idx / V, e = idx - gq * V;
    const int cg0 = (blockIdx.x * 256 + gq) % cg;   // channel group of local thread gq
    float s = 0.f, q2 = 0.f;
    for (int l = gq; l < 256; l += cl) { s += red[l * 2 * V + e]; q2 += red[l * 2 * V + V + e]; }
    const size_t nblk = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int ch = cg0 * V + e;
    partial[(size_t)ch * nblk + blk] = s;
    partial[((size_t)C + ch) * nblk + blk] = q2;
  }
}

// Host side of those passes (stp_maxpool3x3s2_bwd, stp_scatter2x_bwd, stp_upsample2x_bwd and their _bn forms).  Each launcher keeps
// its own argument checks and its own grid for the plain form; what the _bn forms share is stated here once.
static inline BnBack bnback_none() {      // the plain form's (unused) kernel argument
  BnBack b;
  b.x = nullptr; b.mean = b.rstd = b.gamma = b.beta = nullptr; b.relu = 0;
  return b;
}
// the seven arguments of a _bn entry point -> *b; false if one that must be there is missing
static inline bool bnback_fill(BnBack* b, const void* bn_x, const float* mean, const float* rstd, const float* gamma, const float* beta, int relu,
                               const float* partial) {
  if (!bn_x || !mean || !rstd || !partial) return false;
  b->x = (const char*)bn_x; b->mean = mean; b->rstd = rstd; b->gamma = gamma; b->beta = beta; b->relu = relu;
  return true;
}
// each workgroup must hold whole pixels of all its channel groups
static inline bool bnb_channels_ok(int C, int V) { return 256 % (C / V) == 0; }
static inline size_t bnb_lds(int V) { return 256 * 2 * V * sizeof(float); }
// the launch grid; its workgroups are the columns ("tiles") of the [2][C][tiles] partial table
static inline dim3 bnb_grid(int N, int H, int W, int C, int V) { return dim3(ceil_div(W * (C / V), 256), ceil_div(N * H, BNB_ROWS)); }
// what the *_bn_tiles queries answer: the tile count, 0 = this channel count is not supported
static inline int bnb_tiles(int N, int H, int W, int C, int V) {
  if (C <= 0 || (C & 3) || !bnb_channels_ok(C, V)) return 0;
  const dim3 g = bnb_grid(N, H, W, C, V);
  return (int)(g.x * g.y);
}
