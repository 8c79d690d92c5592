// BatchNormalization (training / inference phase): statistics, apply, backward, and the fused finalize + apply forms.
// All are HBM-bound streaming kernels: 16-byte vector access, channel constants staged in LDS,
// two-stage fixed-order reductions (per-block partials -> finalize) so results are
// deterministic run to run.  (The statistics kernel for 16-bit / fp32 tensors, bn_partial_kernel, lives in stream_ops.h:
// stp_channel_sum of elementwise.hip launches it too.)
#include "stream_ops.h"
#include <cstdlib>

// ------------------------------------------------------------------------------------------
// statistics of the raw image (uint8) - partial[block][0][c] = sum x, partial[block][1][c] = sum x^2 as bn_partial_kernel writes them
// raw image input: uint8, any channel count (C = 3); one thread per (row-lane, channel)
__global__ __launch_bounds__(256) void bn_partial_u8_kernel(const uint8_t* __restrict__ x, int64_t rows, int C, float* partial) {
  __shared__ float rs[256 * 2];
  const int rowLanes = 256 / C;
  const int tcol = threadIdx.x % C, trow = threadIdx.x / C;
  const int64_t rowsPerBlock = (rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * rowsPerBlock;
  const int64_t r1 = r0 + rowsPerBlock < rows ? r0 + rowsPerBlock : rows;
  float s = 0.f, q = 0.f;
  if (trow < rowLanes)
    for (int64_t r = r0 + trow; r < r1; r += rowLanes) {
      const float v = (float)x[r * C + tcol];
      s += v;
      q += v * v;
    }
  rs[threadIdx.x * 2] = s;
  rs[threadIdx.x * 2 + 1] = q;
  __syncthreads();
  if (trow == 0 && threadIdx.x < C) {
    float a = 0.f, b = 0.f;
    for (int t = 0; t < rowLanes; ++t) { a += rs[(t * C + tcol) * 2]; b += rs[(t * C + tcol) * 2 + 1]; }
    partial[(size_t)blockIdx.x * 2 * C + tcol] = a;
    partial[(size_t)blockIdx.x * 2 * C + C + tcol] = b;
  }
}

// The same statistics for 1..8 interleaved uint8 channels (the raw image), vectorised: a thread takes 16 rows = C 16-byte loads
// per iteration, so byte k of the group belongs to channel k % C at compile time; sums are exact integers (order-free, hence
// deterministic), converted once per workgroup.  rows per workgroup are a multiple of 16; the ragged end goes byte by byte.
template <int C>
__global__ __launch_bounds__(256) void bn_partial_u8v_kernel(const uint8_t* __restrict__ x, int64_t rows, float* partial) {
  __shared__ unsigned long long red[4][2 * C];
  const int64_t rowsPerBlock = ((rows + gridDim.x - 1) / gridDim.x + 15) & ~(int64_t)15;
  const int64_t r0 = (int64_t)blockIdx.x * rowsPerBlock;
  const int64_t r1 = r0 + rowsPerBlock < rows ? r0 + rowsPerBlock : rows;
  const int64_t rv = r0 + ((r1 > r0 ? r1 - r0 : 0) & ~(int64_t)15);            // end of the whole 16-row groups
  uint32_t sm[C], sq[C];
#pragma unroll
  for (int c = 0; c < C; ++c) sm[c] = sq[c] = 0u;
  for (int64_t r = r0 + (int64_t)threadIdx.x * 16; r < rv; r += 256 * 16) {
    uint4 v[C];
    const uint4* p = reinterpret_cast<const uint4*>(x + r * C);
#pragma unroll
    for (int j = 0; j < C; ++j) v[j] = p[j];
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const uint32_t w[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t b = (w[k >> 2] >> (8 * (k & 3))) & 0xffu;
        sm[(j * 16 + k) % C] += b;
        sq[(j * 16 + k) % C] += b * b;
      }
    }
  }
  for (int64_t i = rv * C + threadIdx.x; i < r1 * C; i += 256) {                 // (fewer than 16 rows)
    const uint32_t b = x[i];
    const int ch = (int)(i % C);
#pragma unroll
    for (int c = 0; c < C; ++c)
      if (c == ch) { sm[c] += b; sq[c] += b * b; }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    unsigned long long a = sm[c], b = sq[c];
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][c] = a; red[threadIdx.x >> 6][C + c] = b; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * C)
    partial[(size_t)blockIdx.x * 2 * C + threadIdx.x] =
        (float)(double)(red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// launch: grid = ceil(C/4), block = 256
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* partial, int blocks, int C, double inv_rows, double unbias,
                                                          float eps, float momentum, float* mean, float* rstd, float* mm,
                                                          float* mv) {
  const int c = blockIdx.x * 4 + (threadIdx.x & 3);
  const Sum2 t = reduce_partials(partial, blocks, C, c, true);
  if ((threadIdx.x >> 2) != 0 || c >= C) return;
  const double m = t.s * inv_rows;
  double var = t.q * inv_rows - m * m;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (mm) mm[c] = mm[c] * momentum + (float)m * (1.f - momentum);
  if (mv) mv[c] = mv[c] * momentum + (float)(var * unbias) * (1.f - momentum);
}

extern "C" size_t stp_bn_workspace_bytes(int32_t C) { return (size_t)BN_MAX_BLOCKS * 2 * C * sizeof(float); }

extern "C" int stp_bn_stats(const void* x, int32_t xdtype, int64_t rows, int32_t C, float eps, float momentum,
                            float* mean, float* rstd, float* moving_mean, float* moving_var, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!x || !mean || !rstd || !workspace || rows <= 0 || C <= 0) return STP_E_BADARG;
  if (workspace_bytes < stp_bn_workspace_bytes(C)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = bn_blocks(rows);
  float* partial = (float*)workspace;
  if (xdtype == STP_U8) {
    if (C > 256) return STP_E_BADARG;
    const bool vec = ((uintptr_t)x & 15) == 0;
#define STP_U8V(CC) hipLaunchKernelGGL(bn_partial_u8v_kernel<CC>, dim3(blocks), dim3(256), 0, s, (const uint8_t*)x, rows, partial)
    switch (vec ? C : 0) {
      case 1: STP_U8V(1); break;
      case 2: STP_U8V(2); break;
      case 3: STP_U8V(3); break;
      case 4: STP_U8V(4); break;
      case 5: STP_U8V(5); break;
      case 6: STP_U8V(6); break;
      case 7: STP_U8V(7); break;
      case 8: STP_U8V(8); break;
      default: hipLaunchKernelGGL(bn_partial_u8_kernel, dim3(blocks), dim3(256), 0, s, (const uint8_t*)x, rows, C, partial);
    }
#undef STP_U8V
  } else {
    if (C & 3) return STP_E_BADARG;
    if (const int rc = bn_partial_launch(x, xdtype, rows, C, blocks, partial, s)) return rc;
  }
  STP_LAUNCH_CHECK();
  const double unbias = rows > 1 ? (double)rows / (double)(rows - 1) : 1.0;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, s, partial, blocks, C, 1.0 / (double)rows,
                     unbias, eps, momentum, mean, rstd, moving_mean, moving_var);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// Sum of the [2][tiles] partial columns of one channel by 256 threads (one workgroup per channel), fp64, fixed order: up to four
// columns per thread with all loads issued first, a DPP row reduction on the two halves of the doubles (no LDS round trips: the
// ds_bpermute butterfly this replaces was 24 dependent LDS operations of a 5 us launch), the four row totals of a wave by
// v_readlane, the four waves through LDS (one barrier).  Valid in thread 0.
__device__ __forceinline__ double bnf_row_shr_add(double v, int ctl_id) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  int lo = (int)(u & 0xffffffffull), hi = (int)(u >> 32);
  int mlo, mhi;
  switch (ctl_id) {      // bound_ctrl: lanes shifted in from outside the row read 0.0
    case 1: mlo = __builtin_amdgcn_update_dpp(0, lo, 0x111, 0xf, 0xf, true); mhi = __builtin_amdgcn_update_dpp(0, hi, 0x111, 0xf, 0xf, true); break;
    case 2: mlo = __builtin_amdgcn_update_dpp(0, lo, 0x112, 0xf, 0xf, true); mhi = __builtin_amdgcn_update_dpp(0, hi, 0x112, 0xf, 0xf, true); break;
    case 4: mlo = __builtin_amdgcn_update_dpp(0, lo, 0x114, 0xf, 0xf, true); mhi = __builtin_amdgcn_update_dpp(0, hi, 0x114, 0xf, 0xf, true); break;
    default: mlo = __builtin_amdgcn_update_dpp(0, lo, 0x118, 0xf, 0xf, true); mhi = __builtin_amdgcn_update_dpp(0, hi, 0x118, 0xf, 0xf, true); break;
  }
  return v + __builtin_bit_cast(double, ((unsigned long long)(unsigned)mhi << 32) | (unsigned long long)(unsigned)mlo);
}
__device__ __forceinline__ double bnf_readlane_f64(double v, int lane) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffull), lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ void bnf_channel_sums(const float* __restrict__ ps, const float* __restrict__ pq, int tiles, double (*sh)[4], double& S, double& Q) {
  double s = 0.0, q = 0.0;
  if (tiles <= 1024) {
    float a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = (int)threadIdx.x + 256 * u;
      a[u] = b[u] = 0.f;
      if (t < tiles) { a[u] = ps[t]; b[u] = pq[t]; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if ((int)threadIdx.x + 256 * u < tiles) { s += (double)a[u]; q += (double)b[u]; }
  } else {
    for (int t = threadIdx.x; t < tiles; t += 256) { s += (double)ps[t]; q += (double)pq[t]; }
  }
  s = bnf_row_shr_add(s, 1); q = bnf_row_shr_add(q, 1);
  s = bnf_row_shr_add(s, 2); q = bnf_row_shr_add(q, 2);
  s = bnf_row_shr_add(s, 4); q = bnf_row_shr_add(q, 4);
  s = bnf_row_shr_add(s, 8); q = bnf_row_shr_add(q, 8);      // lane 15 of every 16-lane row: the row's total
  const double ws = (bnf_readlane_f64(s, 15) + bnf_readlane_f64(s, 31)) + (bnf_readlane_f64(s, 47) + bnf_readlane_f64(s, 63));
  const double wq = (bnf_readlane_f64(q, 15) + bnf_readlane_f64(q, 31)) + (bnf_readlane_f64(q, 47) + bnf_readlane_f64(q, 63));
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = ws; sh[1][threadIdx.x >> 6] = wq; }
  __syncthreads();
  S = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
  Q = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
}

// Finalize for statistics produced by a convolution epilogue: partial is [2][C][tiles] (tile contiguous).
// One wave per channel: coalesced strided walk + wave reduction, fixed order.
__global__ __launch_bounds__(256) void bn_finalize_tiles_kernel(const float* __restrict__ partial, int tiles, int C, double inv_rows,
                                                                double unbias, float eps, float momentum, float* mean, float* rstd,
                                                                float* mm, float* mv) {
  __shared__ double sh[2][4];
  const int c = blockIdx.x;
  double S, Q;
  bnf_channel_sums(partial + (size_t)c * tiles, partial + ((size_t)C + c) * tiles, tiles, sh, S, Q);
  if (threadIdx.x != 0) return;
  const double m = S * inv_rows;
  double var = Q * inv_rows - m * m;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  rstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (mm) mm[c] = mm[c] * momentum + (float)m * (1.f - momentum);
  if (mv) mv[c] = mv[c] * momentum + (float)(var * unbias) * (1.f - momentum);
}

extern "C" int stp_bn_finalize(const float* partial, int32_t tiles, int64_t rows, int32_t C, float eps, float momentum, float* mean,
                               float* rstd, float* moving_mean, float* moving_var, void* stream) {
  if (!partial || !mean || !rstd || tiles <= 0 || rows <= 0 || C <= 0) return STP_E_BADARG;
  const double unbias = rows > 1 ? (double)rows / (double)(rows - 1) : 1.0;
  hipLaunchKernelGGL(bn_finalize_tiles_kernel, dim3(C), dim3(256), 0, (hipStream_t)stream, partial, tiles, C, 1.0 / (double)rows,
                     unbias, eps, momentum, mean, rstd, moving_mean, moving_var);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------
// apply: y = relu?(x*scale + shift); scale/shift staged in LDS once per block
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void bn_apply_kernel(const TX* __restrict__ x, TY* __restrict__ y, int64_t rows, int C,
                                                       const float* mean, const float* rstd, const float* gamma,
                                                       const float* beta, const float* mvar, float eps, int relu,
                                                       const long long* slots = nullptr, int nslots = 0, double inv_rows = 0.0,
                                                       double unbias = 0.0, float momentum = 0.f, float* mean_out = nullptr,
                                                       float* rstd_out = nullptr, float* mm = nullptr, float* mv = nullptr) {
  extern __shared__ float ss[];  // scale[C], shift[C]
  for (int c = threadIdx.x; c < C; c += 256) {
    float m, r;
    if (slots) {
      // batch statistics straight from the producing convolution's fixed-point slots (every workgroup derives the same
      // numbers; workgroup 0 publishes them for the backward pass and updates the moving statistics)
      const double md = slot_sum(slots, nslots, c) * inv_rows;
      double var = slot_sum(slots, nslots, C + c) * inv_rows - md * md;
      if (var < 0.0) var = 0.0;
      m = (float)md;
      r = (float)(1.0 / sqrt(var + (double)eps));
      if (blockIdx.x == 0) {
        mean_out[c] = m;
        rstd_out[c] = r;
        if (mm) mm[c] = mm[c] * momentum + m * (1.f - momentum);
        if (mv) mv[c] = mv[c] * momentum + (float)(var * unbias) * (1.f - momentum);
      }
    } else {
      m = mean[c];
      r = rstd ? rstd[c] : rsqrtf(mvar[c] + eps);
    }
    const float sc = gamma ? r * gamma[c] : r;
    ss[c] = sc;
    ss[C + c] = (beta ? beta[c] : 0.f) - m * sc;
  }
  __syncthreads();
  const int cg = C >> 2;
  const int64_t total = rows * cg;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % cg) * 4;
    f32x4 v = ld4<TX>(x + i * 4);
    v.x = bn_affine(v.x, ss[c], ss[C + c]);
    v.y = bn_affine(v.y, ss[c + 1], ss[C + c + 1]);
    v.z = bn_affine(v.z, ss[c + 2], ss[C + c + 2]);
    v.w = bn_affine(v.w, ss[c + 3], ss[C + c + 3]);
    if (relu) { v.x = bn_act(v.x, relu); v.y = bn_act(v.y, relu); v.z = bn_act(v.z, relu); v.w = bn_act(v.w, relu); }
    store4(y + i * 4, v);
  }
}

// bf16 fast path: a thread owns 8 CONSECUTIVE channels (one 16-byte vector per row) for the whole launch - the grid stride is a
// multiple of the C/8 channel groups, so scale / shift live in 16 registers instead of being re-read from LDS per element
// (rocprofv3: the LDS-table kernel spent 27 % of its time in LDS with 64 % bank conflicts) - and walks rows with 4 vectors in flight.
__global__ __launch_bounds__(256) void bn_apply_v8_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int64_t rows, int C,
                                                          const float* mean, const float* rstd, const float* gamma, const float* beta,
                                                          int relu) {
  // the thread fetches the constants of ITS 8 channels itself (eight 16-byte loads that hit L2, issued with the first data vectors):
  // no LDS table, no barrier - on the 4-17 MB tensors a thread handles a few vectors and the table prologue was most of its life
  const int cg = C >> 3;
  const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;   // stride % cg == 0 (host)
  const int c = (int)(t0 % cg) * 8;
  float sc[8], sh[8];
  {
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(mean + c), m1 = *reinterpret_cast<const f32x4*>(mean + c + 4);
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(rstd + c), r1 = *reinterpret_cast<const f32x4*>(rstd + c + 4);
    f32x4 g0 = {1.f, 1.f, 1.f, 1.f}, g1 = g0, b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
    if (gamma) { g0 = *reinterpret_cast<const f32x4*>(gamma + c); g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4); }
    if (beta) { b0 = *reinterpret_cast<const f32x4*>(beta + c); b1 = *reinterpret_cast<const f32x4*>(beta + c + 4); }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float r = e < 4 ? r0[e & 3] : r1[e & 3], k = gamma ? r * (e < 4 ? g0[e & 3] : g1[e & 3]) : r;
      sc[e] = k;
      sh[e] = (e < 4 ? b0[e & 3] : b1[e & 3]) - (e < 4 ? m0[e & 3] : m1[e & 3]) * k;
    }
  }
  const int64_t total = rows * cg;
  auto one = [&](const u32x4 r) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = bn_act(bn_affine(h16lo_to_f32(r[e]), sc[2 * e], sh[2 * e]), relu);
      const float hi = bn_act(bn_affine(h16hi_to_f32(r[e]), sc[2 * e + 1], sh[2 * e + 1]), relu);
      o[e] = pack_bf16x2(lo, hi);
    }
    return o;
  };
  int64_t i = t0;
  for (; i + 3 * stride < total; i += 4 * stride) {
    const u32x4 r0 = *reinterpret_cast<const u32x4*>(x + i * 8), r1 = *reinterpret_cast<const u32x4*>(x + (i + stride) * 8);
    const u32x4 r2 = *reinterpret_cast<const u32x4*>(x + (i + 2 * stride) * 8), r3 = *reinterpret_cast<const u32x4*>(x + (i + 3 * stride) * 8);
    *reinterpret_cast<u32x4*>(y + i * 8) = one(r0);
    *reinterpret_cast<u32x4*>(y + (i + stride) * 8) = one(r1);
    *reinterpret_cast<u32x4*>(y + (i + 2 * stride) * 8) = one(r2);
    *reinterpret_cast<u32x4*>(y + (i + 3 * stride) * 8) = one(r3);
  }
  for (; i < total; i += stride) *reinterpret_cast<u32x4*>(y + i * 8) = one(*reinterpret_cast<const u32x4*>(x + i * 8));
}

// uint8 [rows][C <= CY] -> TY [rows][CY] (CY = 4, or 8 for images of 4..7 channels); padded channels get pad_value
template <typename TY, int CY>
__global__ __launch_bounds__(256) void bn_apply_u8_kernel(const uint8_t* __restrict__ x, TY* __restrict__ y, int64_t rows,
                                                          int C, const float* mean, const float* rstd, const float* gamma,
                                                          const float* beta, const float* mvar, float eps, int relu,
                                                          float pad_value) {
  float sc[CY], sh[CY];
#pragma unroll
  for (int c = 0; c < CY; ++c) {
    if (c < C) {
      const float r = rstd ? rstd[c] : rsqrtf(mvar[c] + eps);
      sc[c] = gamma ? r * gamma[c] : r;
      sh[c] = (beta ? beta[c] : 0.f) - mean[c] * sc[c];
    } else { sc[c] = 0.f; sh[c] = pad_value; }
  }
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < rows; r += (int64_t)gridDim.x * 256) {
#pragma unroll
    for (int h = 0; h < CY / 4; ++h) {
      f32x4 v;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = h * 4 + e;
        float t = c < C ? bn_affine((float)x[r * C + c], sc[c], sh[c]) : pad_value;
        if (relu && c < C) t = bn_act(t, relu);
        v[e] = t;
      }
      store4(y + r * CY + h * 4, v);
    }
  }
}

static int bn_apply_dispatch(const void* x, int xdt, void* y, int ydt, int64_t rows, int C, int Cy, const float* mean,
                             const float* rstd, const float* gamma, const float* beta, const float* mvar, float eps,
                             int relu, float pad_value, hipStream_t s) {
  if (!x || !y || !mean || rows <= 0) return STP_E_BADARG;
  if (xdt == STP_U8) {
    if ((Cy != 4 && Cy != 8) || C > Cy) return STP_E_BADARG;
    const int g = grid_for(rows);
#define STP_APPLY_U8(TY_, CY_) \
    hipLaunchKernelGGL((bn_apply_u8_kernel<TY_, CY_>), dim3(g), dim3(256), 0, s, (const uint8_t*)x, (TY_*)y, rows, C, mean, rstd, gamma, beta, mvar, eps, \
                       relu, pad_value)
    if (ydt == STP_H16) { if (Cy == 4) STP_APPLY_U8(bf16_t, 4); else STP_APPLY_U8(bf16_t, 8); }
    else if (ydt == STP_F32) { if (Cy == 4) STP_APPLY_U8(float, 4); else STP_APPLY_U8(float, 8); }
    else return STP_E_BADARG;
#undef STP_APPLY_U8
    STP_LAUNCH_CHECK();
    return STP_OK;
  }
  if ((C & 3) || Cy != C || xdt != ydt) return STP_E_BADARG;
  if (xdt == STP_H16 && (C & 7) == 0 && rstd && !mvar) {
    const int gv = grid_multiple_of(grid_for_amortised(rows * (C >> 3), 8), C >> 3);   // 8 vectors per thread once the CUs are covered
    if (gv > 0) {
      hipLaunchKernelGGL(bn_apply_v8_kernel, dim3(gv), dim3(256), 0, s, (const bf16_t*)x, (bf16_t*)y, rows, C, mean, rstd, gamma, beta, relu);
      STP_LAUNCH_CHECK();
      return STP_OK;
    }
  }
  const size_t lds = 2 * (size_t)C * sizeof(float);
  const int g = grid_for(rows * (C >> 2));
  return launch_t(xdt, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL((bn_apply_kernel<T, T>), dim3(g), dim3(256), lds, s, (const T*)x, (T*)y, rows, C, mean, rstd, gamma, beta, mvar, eps, relu);
  });
}

extern "C" int stp_bn_apply(const void* x, int32_t xdtype, void* y, int32_t ydtype, int64_t rows, int32_t C, int32_t Cy,
                            const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t relu,
                            float pad_value, void* stream) {
  if (!rstd) return STP_E_BADARG;
  return bn_apply_dispatch(x, xdtype, y, ydtype, rows, C, Cy, mean, rstd, gamma, beta, nullptr, 0.f, relu, pad_value,
                           (hipStream_t)stream);
}

extern "C" int stp_bn_apply_slots(const void* x, void* y, int32_t dtype, int64_t rows, int32_t C, const int64_t* slots, int32_t nslots,
                                  float eps, float momentum, float* mean, float* rstd, float* moving_mean, float* moving_var,
                                  const float* gamma, const float* beta, int32_t relu, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !y || !slots || !mean || !rstd || rows <= 0 || C <= 0 || (C & 3) || nslots < 1 || (nslots & (nslots - 1))) return STP_E_BADARG;
  const size_t lds = 2 * (size_t)C * sizeof(float);
  const int g = grid_for(rows * (C >> 2));
  const double inv_rows = 1.0 / (double)rows, unbias = rows > 1 ? (double)rows / (double)(rows - 1) : 1.0;
  hipStream_t s = (hipStream_t)stream;
  return launch_t(dtype, [&](auto tv) {
    using T = typename decltype(tv)::T;
    hipLaunchKernelGGL((bn_apply_kernel<T, T>), dim3(g), dim3(256), lds, s, (const T*)x, (T*)y, rows, C, (const float*)nullptr,
                       (const float*)nullptr, gamma, beta, (const float*)nullptr, eps, relu, (const long long*)slots, nslots, inv_rows, unbias,
                       momentum, mean, rstd, moving_mean, moving_var);
  });
}

extern "C" int stp_bn_inference(const void* x, int32_t xdtype, void* y, int32_t ydtype, int64_t rows, int32_t C, int32_t Cy,
                                const float* moving_mean, const float* moving_var, float eps, const float* gamma,
                                const float* beta, int32_t relu, float pad_value, void* stream) {
  if (!moving_var) return STP_E_BADARG;
  return bn_apply_dispatch(x, xdtype, y, ydtype, rows, C, Cy, moving_mean, nullptr, gamma, beta, moving_var, eps, relu,
                           pad_value, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// backward.  g = dy * [relu ? (x*scale+shift > 0) : 1];  partial sums of g and g*xhat
template <typename T, int V>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const T* __restrict__ x, const T* __restrict__ dy, int64_t rows,
                                                             int C, const float* mean, const float* rstd,
                                                             const float* gamma, const float* beta, int relu,
                                                             float* partial) {
  extern __shared__ float red[];
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
      float mu[V], rs[V], sc[V], sh[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        mu[e] = mean[c * V + e];
        rs[e] = rstd[c * V + e];
        sc[e] = gamma ? rs[e] * gamma[c * V + e] : rs[e];
        sh[e] = (beta ? beta[c * V + e] : 0.f) - mu[e] * sc[e];
      }
      const size_t cb = (size_t)c * V;
      int64_t r = r0 + trow;
      for (; r + (int64_t)rowLanes < r1; r += 2 * (int64_t)rowLanes) {
        float x0[V], g0[V], x1[V], g1[V];
        ldv<T, V>(x + r * C + cb, x0);
        ldv<T, V>(dy + r * C + cb, g0);
        ldv<T, V>(x + (r + rowLanes) * C + cb, x1);
        ldv<T, V>(dy + (r + rowLanes) * C + cb, g1);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if (!bn_act_on(bn_affine(x0[e], sc[e], sh[e]), relu)) g0[e] = 0.f;
          if (!bn_act_on(bn_affine(x1[e], sc[e], sh[e]), relu)) g1[e] = 0.f;
          s[e] += g0[e] + g1[e];
          q[e] += g0[e] * ((x0[e] - mu[e]) * rs[e]) + g1[e] * ((x1[e] - mu[e]) * rs[e]);
        }
      }
      for (; r < r1; r += rowLanes) {
        float x0[V], g0[V];
        ldv<T, V>(x + r * C + cb, x0);
        ldv<T, V>(dy + r * C + cb, g0);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if (!bn_act_on(bn_affine(x0[e], sc[e], sh[e]), relu)) g0[e] = 0.f;
          s[e] += g0[e];
          q[e] += g0[e] * ((x0[e] - mu[e]) * rs[e]);
        }
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

// sums[0][c] = dbeta, sums[1][c] = dgamma (raw sums, also written to the grad buffers)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* partial, int blocks, int C, float* sums,
                                                              float* dgamma, float* dbeta) {
  const int c = blockIdx.x * 4 + (threadIdx.x & 3);
  const Sum2 t = reduce_partials(partial, blocks, C, c, true);
  if ((threadIdx.x >> 2) != 0 || c >= C) return;
  sums[c] = (float)t.s;
  sums[C + c] = (float)t.q;
  if (dbeta) dbeta[c] = (float)t.s;
  if (dgamma) dgamma[c] = (float)t.q;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* dx,
                                                           int64_t rows, int C, const float* mean, const float* rstd,
                                                           const float* gamma, const float* beta, const float* sums,
                                                           float inv_rows, int relu, int accumulate, const long long* slots = nullptr,
                                                           int nslots = 0, float* dgamma = nullptr, float* dbeta = nullptr, const T* dadd = nullptr) {
  // accumulate: dx = result + dadd (dadd == nullptr: in place, dadd = dx; otherwise the addend lives in ANOTHER buffer and stays intact -
  // a residual gradient that a pending grouped weight gradient still reads as its dY)
  if (!dadd) dadd = dx;
  extern __shared__ float ss[];  // mean, rstd, scale, shift, k1 = dbeta/M, k2 = dgamma/M   [6][C]
  if (!slots && V == 8 && ((int64_t)gridDim.x * 256) % (C / V) == 0) {
    // The thread keeps its 8 channels for the whole launch and fetches their constants ITSELF (twelve 16-byte loads that hit L2, one
    // latency, issued together with the first data vectors): no LDS table, no barrier.  The table prologue - C x 6 values through
    // LDS per workgroup, then 48 conflicting LDS reads per thread - was most of the launch on the 4-17 MB tensors of stages 2-4,
    // where a thread handles one or two vectors (rocprofv3: 22 us for an 8 MB tensor; launch_table: 0.7-1.1 TB/s).
    const int cg8 = C / 8;
    const int c = (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % cg8) * 8;
    float mu[8], rs[8], sc[8], sh[8], k1[8], k2[8];
    {
      const f32x4 m0 = *reinterpret_cast<const f32x4*>(mean + c), m1 = *reinterpret_cast<const f32x4*>(mean + c + 4);
      const f32x4 r0 = *reinterpret_cast<const f32x4*>(rstd + c), r1 = *reinterpret_cast<const f32x4*>(rstd + c + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(sums + c), s1 = *reinterpret_cast<const f32x4*>(sums + c + 4);
      const f32x4 q0 = *reinterpret_cast<const f32x4*>(sums + C + c), q1 = *reinterpret_cast<const f32x4*>(sums + C + c + 4);
      f32x4 g0 = {1.f, 1.f, 1.f, 1.f}, g1 = g0, b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
      if (gamma) { g0 = *reinterpret_cast<const f32x4*>(gamma + c); g1 = *reinterpret_cast<const f32x4*>(gamma + c + 4); }
      if (beta) { b0 = *reinterpret_cast<const f32x4*>(beta + c); b1 = *reinterpret_cast<const f32x4*>(beta + c + 4); }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float m = e < 4 ? m0[e & 3] : m1[e & 3], r = e < 4 ? r0[e & 3] : r1[e & 3];
        const float k = gamma ? r * (e < 4 ? g0[e & 3] : g1[e & 3]) : r;
        mu[e] = m; rs[e] = r; sc[e] = k;
        sh[e] = (e < 4 ? b0[e & 3] : b1[e & 3]) - m * k;
        k1[e] = (e < 4 ? s0[e & 3] : s1[e & 3]) * inv_rows;
        k2[e] = (e < 4 ? q0[e & 3] : q1[e & 3]) * inv_rows;
      }
    }
    const int64_t total8 = rows * cg8, stride8 = (int64_t)gridDim.x * 256;
    auto one8 = [&](int64_t i, const float (&xv)[V], float (&g)[V], const float (&d)[V]) {
      float o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (!bn_act_on(bn_affine(xv[e], sc[e], sh[e]), relu)) g[e] = 0.f;
        const float xh = (xv[e] - mu[e]) * rs[e];
        o[e] = sc[e] * (g[e] - k1[e] - xh * k2[e]);
        if (accumulate) o[e] += d[e];
      }
      stv<T, V>(dx + i * V, o);
    };
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + stride8 < total8; i += 2 * stride8) {          // two rows in flight per thread
      float x0[V], g0[V], d0[V], x1[V], g1[V], d1[V];
      ldv<T, V>(x + i * V, x0);
      ldv<T, V>(x + (i + stride8) * V, x1);
      ldv<T, V>(dy + i * V, g0);
      ldv<T, V>(dy + (i + stride8) * V, g1);
      if (accumulate) { ldv<T, V>(dadd + i * V, d0); ldv<T, V>(dadd + (i + stride8) * V, d1); }
      one8(i, x0, g0, d0);
      one8(i + stride8, x1, g1, d1);
    }
    for (; i < total8; i += stride8) {
      float x0[V], g0[V], d0[V];
      ldv<T, V>(x + i * V, x0);
      ldv<T, V>(dy + i * V, g0);
      if (accumulate) ldv<T, V>(dadd + i * V, d0);
      one8(i, x0, g0, d0);
    }
    return;
  }
  for (int c = threadIdx.x; c < C; c += 256) {
    const float r = rstd[c], sc = gamma ? r * gamma[c] : r;
    ss[c] = mean[c];
    ss[C + c] = r;
    ss[2 * C + c] = sc;
    ss[3 * C + c] = (beta ? beta[c] : 0.f) - mean[c] * sc;
    float sb, sg;
    if (slots) {    // sums from the data-gradient convolution's fixed-point slots; workgroup 0 publishes the parameter gradients
      sb = (float)slot_sum(slots, nslots, c);
      sg = (float)slot_sum(slots, nslots, C + c);
      if (blockIdx.x == 0) {
        if (dbeta) dbeta[c] = sb;
        if (dgamma) dgamma[c] = sg;
      }
    } else {
      sb = sums[c];
      sg = sums[C + c];
    }
    ss[4 * C + c] = sb * inv_rows;
    ss[5 * C + c] = sg * inv_rows;
  }
  __syncthreads();
  const int cg = C / V;
  const int64_t total = rows * cg;
  const int64_t stride = (int64_t)gridDim.x * 256;
  if (stride % cg == 0) {
    // the thread keeps its V channels for the whole launch: the six per-channel constants live in registers instead of being
    // re-read from LDS per element (rocprofv3: 44 % LDS time, 62 % bank conflicts in the table-driven loop below)
    const int c = (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % cg) * V;
    float mu[V], rs[V], sc[V], sh[V], k1[V], k2[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      mu[e] = ss[c + e]; rs[e] = ss[C + c + e]; sc[e] = ss[2 * C + c + e]; sh[e] = ss[3 * C + c + e];
      k1[e] = ss[4 * C + c + e]; k2[e] = ss[5 * C + c + e];
    }
    auto one = [&](int64_t i, const float (&xv)[V], float (&g)[V], const float (&d)[V]) {
      float o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (!bn_act_on(bn_affine(xv[e], sc[e], sh[e]), relu)) g[e] = 0.f;
        const float xh = (xv[e] - mu[e]) * rs[e];
        o[e] = sc[e] * (g[e] - k1[e] - xh * k2[e]);
        if (accumulate) o[e] += d[e];
      }
      stv<T, V>(dx + i * V, o);
    };
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + stride < total; i += 2 * stride) {          // two rows in flight per thread
      float x0[V], g0[V], d0[V], x1[V], g1[V], d1[V];
      ldv<T, V>(x + i * V, x0);
      ldv<T, V>(x + (i + stride) * V, x1);
      ldv<T, V>(dy + i * V, g0);
      ldv<T, V>(dy + (i + stride) * V, g1);
      if (accumulate) { ldv<T, V>(dadd + i * V, d0); ldv<T, V>(dadd + (i + stride) * V, d1); }
      one(i, x0, g0, d0);
      one(i + stride, x1, g1, d1);
    }
    for (; i < total; i += stride) {
      float x0[V], g0[V], d0[V];
      ldv<T, V>(x + i * V, x0);
      ldv<T, V>(dy + i * V, g0);
      if (accumulate) ldv<T, V>(dadd + i * V, d0);
      one(i, x0, g0, d0);
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int c = (int)(i % cg) * V;
    float xv[V], g[V], o[V];
    ldv<T, V>(x + i * V, xv);
    ldv<T, V>(dy + i * V, g);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      if (!bn_act_on(bn_affine(xv[e], ss[2 * C + c + e], ss[3 * C + c + e]), relu)) g[e] = 0.f;
      const float xh = (xv[e] - ss[c + e]) * ss[C + c + e];
      o[e] = ss[2 * C + c + e] * (g[e] - ss[4 * C + c + e] - xh * ss[5 * C + c + e]);
    }
    if (accumulate) {
      float d[V];
      ldv<T, V>(dadd + i * V, d);
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] += d[e];
    }
    stv<T, V>(dx + i * V, o);
  }
}

// the one launch of bn_bwd_apply_kernel: sums from `sums` (stp_bn_backward, stp_bn_backward_fused_add) or from `slots`
// (stp_bn_backward_slots, which also publishes dgamma / dbeta); dadd: see the kernel
static int bn_bwd_apply_launch(const void* x, const void* dy, void* dx, int dtype, int64_t rows, int C, const float* mean, const float* rstd,
                               const float* gamma, const float* beta, const float* sums, int relu, int accumulate, const long long* slots, int nslots,
                               float* dgamma, float* dbeta, const void* dadd, hipStream_t s) {
  const bool v8 = dtype == STP_H16 && (C & 7) == 0;
  const size_t lds2 = 6 * (size_t)C * sizeof(float);
  const int g = grid_fixed_channels(grid_for_amortised(rows * (C / (v8 ? 8 : 4)), 8), C / (v8 ? 8 : 4));
  const float inv_rows = (float)(1.0 / (double)rows);
  return launch_tv(dtype, v8, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, V>), dim3(g), dim3(256), lds2, s, (const T*)x, (const T*)dy, (T*)dx, rows, C, mean, rstd, gamma, beta,
                       sums, inv_rows, relu, accumulate, slots, nslots, dgamma, dbeta, (const T*)dadd);
  });
}

extern "C" int stp_bn_backward(const void* x, const void* dy, void* dx, int32_t dtype, int64_t rows, int32_t C,
                               const float* mean, const float* rstd, const float* gamma, const float* beta, float* dgamma,
                               float* dbeta, int32_t relu, int32_t accumulate_dx, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !dy || !dx || !mean || !rstd || !workspace || rows <= 0 || C <= 0 || (C & 3)) return STP_E_BADARG;
  if (workspace_bytes < stp_bn_workspace_bytes(C)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int blocks = bn_blocks(rows) > BN_MAX_BLOCKS - 1 ? BN_MAX_BLOCKS - 1 : bn_blocks(rows);
  float* partial = (float*)workspace;
  float* sums = partial + (size_t)(BN_MAX_BLOCKS - 1) * 2 * C;  // last slab holds the finalized sums
  const int rc = launch_tv(dtype, dtype == STP_H16 && (C & 7) == 0, [&](auto tv) {
    using T = typename decltype(tv)::T; constexpr int V = decltype(tv)::V;
    hipLaunchKernelGGL((bn_bwd_partial_kernel<T, V>), dim3(blocks), dim3(256), 256 * 2 * V * sizeof(float), s, (const T*)x, (const T*)dy, rows, C,
                       mean, rstd, gamma, beta, relu, partial);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(ceil_div(C, 4)), dim3(256), 0, s, partial, blocks, C, sums, dgamma, dbeta);
  STP_LAUNCH_CHECK();
  return bn_bwd_apply_launch(x, dy, dx, dtype, rows, C, mean, rstd, gamma, beta, sums, relu, accumulate_dx, nullptr, 0, nullptr, nullptr, nullptr, s);
}

// ------------------------------------------------------------------------------------------
// FUSED finalize + apply (round 3).  The finalize launches (one workgroup per channel, ~5 us each: 86 per U-Net/ResNet34 step, pure
// launch latency on the critical chain conv -> finalize -> apply -> conv) disappear where the partial table is small: a workgroup
// of the apply pass owns a SLAB of 64 channels (128 bytes of every row: whole cache lines) x a chunk of rows, and first reduces the
// [2][64][tiles] partial sums of its own slab - fp64, fixed order, the same for every workgroup of the slab, so all of them
// normalise with bit-identical constants; the chunk-0 workgroup of a slab also publishes mean / rstd / moving statistics
// (dgamma / dbeta in the backward form).  Each workgroup re-reads 512 x tiles bytes that sit in L2 - eligible while that is <= 64 KB.
#define BNF_SLAB 64
static bool bn_fused_ok(int dtype, int64_t rows, int C, int tiles) {
  static const bool on = !(getenv("STP_BN_FUSE_FINALIZE") && atoi(getenv("STP_BN_FUSE_FINALIZE")) == 0);
  // measured per shape (U-Net/ResNet34 bs16, eager launches, profiles/r03j_bn_fused_vs_separate.txt): 32 columns (stage 4) 8.1 vs 6.7 + 7.0 us
  // forward and 7.7 vs 11.4 backward, 128 columns (stage 3) 10.4 vs 13.7 and 10.9 vs 12.5, 256 columns (stage 2: 128 KB of partial sums
  // per workgroup, twice its own rows) 14.7 vs 16.0 and 17.8 vs 15.8 - the fused form stops at 128 columns
  // (STP_BN_FUSE_MAXCOLS: A/B switch for the column limit; round 4 re-measured 256 columns with the rows prefetched before the sums)
  static const int maxcols = getenv("STP_BN_FUSE_MAXCOLS") ? atoi(getenv("STP_BN_FUSE_MAXCOLS")) : 128;
  return on && dtype == STP_H16 && (C % BNF_SLAB) == 0 && tiles >= 1 && tiles <= maxcols && rows >= 64;
}
static int bn_fused_chunks(int64_t rows, int C) {
  // ~8 rows per thread once the CUs are covered (a thread owns 8 channels of a row: 32 rows per workgroup pass)
  const int slabs = C / BNF_SLAB;
  int64_t want = (rows + 255) / 256;              // 8 passes of 32 rows
  const int64_t lo = (2 * 256 + slabs - 1) / slabs;
  if (want < lo) want = lo;
  const int64_t hi = (rows + 31) / 32;
  if (want > hi) want = hi;
  return (int)(want < 1 ? 1 : want);
}

// sum of partial[stat][c][0..tiles) for the 64 channels of the slab: 4 lanes per channel, fp64, fixed order; result in lanes j == 0
__device__ __forceinline__ void bnf_slab_sums(const float* __restrict__ partial, int tiles, int C, int c0, double& s, double& q) {
  const int cl = threadIdx.x >> 2, j = threadIdx.x & 3;
  const float* ps = partial + (size_t)(c0 + cl) * tiles;
  const float* pq = partial + ((size_t)C + c0 + cl) * tiles;
  s = 0.0; q = 0.0;
  if ((tiles & 3) == 0 && tiles > 128 && tiles <= 256) {
    // two batches of the 128-column form below (same order of additions as the generic loop: t ascending per lane)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 a[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = 4 * j + 16 * (u + 8 * h);
        a[u] = b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t < tiles) { a[u] = *reinterpret_cast<const f32x4*>(ps + t); b[u] = *reinterpret_cast<const f32x4*>(pq + t); }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (4 * j + 16 * (u + 8 * h) < tiles) {
          s += ((double)a[u].x + (double)a[u].y) + ((double)a[u].z + (double)a[u].w);
          q += ((double)b[u].x + (double)b[u].y) + ((double)b[u].z + (double)b[u].w);
        }
    }
  } else if ((tiles & 3) == 0 && tiles <= 128) {
    // (the fused kernels' case.)  All loads first - as a loop with a run-time trip count every one of the up to 8 iterations exposed
    // a memory round trip at the start of EVERY workgroup of the apply pass; then the sums in the same order
    f32x4 a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int t = 4 * j + 16 * u;
      a[u] = b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < tiles) { a[u] = *reinterpret_cast<const f32x4*>(ps + t); b[u] = *reinterpret_cast<const f32x4*>(pq + t); }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (4 * j + 16 * u < tiles) {
        s += ((double)a[u].x + (double)a[u].y) + ((double)a[u].z + (double)a[u].w);
        q += ((double)b[u].x + (double)b[u].y) + ((double)b[u].z + (double)b[u].w);
      }
  } else if ((tiles & 3) == 0) {
    for (int t = 4 * j; t < tiles; t += 16) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(ps + t), b = *reinterpret_cast<const f32x4*>(pq + t);
      s += ((double)a.x + (double)a.y) + ((double)a.z + (double)a.w);
      q += ((double)b.x + (double)b.y) + ((double)b.z + (double)b.w);
    }
  } else {
    for (int t = j; t < tiles; t += 4) { s += (double)ps[t]; q += (double)pq[t]; }
  }
  s += __shfl_xor(s, 1, 64); q += __shfl_xor(q, 1, 64);
  s += __shfl_xor(s, 2, 64); q += __shfl_xor(q, 2, 64);
}

__global__ __launch_bounds__(256) void bn_finalize_apply_kernel(const float* __restrict__ partial, int tiles, const bf16_t* __restrict__ x,
                                                                bf16_t* __restrict__ y, int64_t rows, int C, int chunks, double inv_rows,
                                                                double unbias, float eps, float momentum, float* mean, float* rstd,
                                                                float* mm, float* mv, const float* gamma, const float* beta, int relu) {
  __shared__ float tab[2][BNF_SLAB];
  const int slab = blockIdx.x / chunks, chunk = blockIdx.x - slab * chunks, c0 = slab * BNF_SLAB;
  const int cg = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  const int64_t per = (rows + chunks - 1) / chunks, ra = (int64_t)chunk * per, rb = ra + per < rows ? ra + per : rows;
  const size_t col = (size_t)c0 + cg * 8;
  // The first four rows of this thread are requested BEFORE the partial sums are reduced (round 4): they do not depend on the
  // statistics, and with ~8 rows per thread the launch is two dependent memory round trips long (sums, then rows) - this makes it one.
  int64_t r = ra + r0;
  const bool pre = r + 96 < rb;
  u32x4 p0 = {0u, 0u, 0u, 0u}, p1 = p0, p2 = p0, p3 = p0;
  if (pre) {
    p0 = *reinterpret_cast<const u32x4*>(x + (size_t)r * C + col); p1 = *reinterpret_cast<const u32x4*>(x + (size_t)(r + 32) * C + col);
    p2 = *reinterpret_cast<const u32x4*>(x + (size_t)(r + 64) * C + col); p3 = *reinterpret_cast<const u32x4*>(x + (size_t)(r + 96) * C + col);
  }
  {
    const int cc = c0 + (threadIdx.x >> 2);
    const float gam = gamma ? gamma[cc] : 1.f, bet = beta ? beta[cc] : 0.f;     // (requested with the rows: independent of the sums)
    double s, q;
    bnf_slab_sums(partial, tiles, C, c0, s, q);
    if ((threadIdx.x & 3) == 0) {
      const int c = cc;
      const double m = s * inv_rows;
      double var = q * inv_rows - m * m;
      if (var < 0.0) var = 0.0;
      const float mf = (float)m, rf = (float)(1.0 / sqrt(var + (double)eps));
      const float k = gamma ? rf * gam : rf;
      tab[0][threadIdx.x >> 2] = k;
      tab[1][threadIdx.x >> 2] = bet - mf * k;
      if (chunk == 0) {
        mean[c] = mf;
        rstd[c] = rf;
        if (mm) mm[c] = mm[c] * momentum + mf * (1.f - momentum);
        if (mv) mv[c] = mv[c] * momentum + (float)(var * unbias) * (1.f - momentum);
      }
    }
  }
  __syncthreads();
  float sc[8], sh[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { sc[e] = tab[0][cg * 8 + e]; sh[e] = tab[1][cg * 8 + e]; }
  auto one = [&](const u32x4 rr) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float lo = bn_act(bn_affine(h16lo_to_f32(rr[e]), sc[2 * e], sh[2 * e]), relu);
      const float hi = bn_act(bn_affine(h16hi_to_f32(rr[e]), sc[2 * e + 1], sh[2 * e + 1]), relu);
      o[e] = pack_bf16x2(lo, hi);
    }
    return o;
  };
  if (pre) {
    *reinterpret_cast<u32x4*>(y + (size_t)r * C + col) = one(p0);
    *reinterpret_cast<u32x4*>(y + (size_t)(r + 32) * C + col) = one(p1);
    *reinterpret_cast<u32x4*>(y + (size_t)(r + 64) * C + col) = one(p2);
    *reinterpret_cast<u32x4*>(y + (size_t)(r + 96) * C + col) = one(p3);
    r += 128;
  }
  for (; r + 96 < rb; r += 128) {       // four rows in flight per thread
    const u32x4 v0 = *reinterpret_cast<const u32x4*>(x + (size_t)r * C + col), v1 = *reinterpret_cast<const u32x4*>(x + (size_t)(r + 32) * C + col);
    const u32x4 v2 = *reinterpret_cast<const u32x4*>(x + (size_t)(r + 64) * C + col), v3 = *reinterpret_cast<const u32x4*>(x + (size_t)(r + 96) * C + col);
    *reinterpret_cast<u32x4*>(y + (size_t)r * C + col) = one(v0);
    *reinterpret_cast<u32x4*>(y + (size_t)(r + 32) * C + col) = one(v1);
    *reinterpret_cast<u32x4*>(y + (size_t)(r + 64) * C + col) = one(v2);
    *reinterpret_cast<u32x4*>(y + (size_t)(r + 96) * C + col) = one(v3);
  }
  for (; r < rb; r += 32) *reinterpret_cast<u32x4*>(y + (size_t)r * C + col) = one(*reinterpret_cast<const u32x4*>(x + (size_t)r * C + col));
}

extern "C" int stp_bn_finalize_apply_ok(int32_t dtype, int64_t rows, int32_t C, int32_t tiles) { return bn_fused_ok(dtype, rows, C, tiles) ? 1 : 0; }

extern "C" int stp_bn_finalize_apply(const float* partial, int32_t tiles, const void* x, void* y, int32_t dtype, int64_t rows, int32_t C,
                                     float eps, float momentum, float* mean, float* rstd, float* moving_mean, float* moving_var,
                                     const float* gamma, const float* beta, int32_t relu, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;
  if (!partial || !x || !y || !mean || !rstd || rows <= 0 || C <= 0 || !bn_fused_ok(dtype, rows, C, tiles)) return STP_E_BADARG;
  const int chunks = bn_fused_chunks(rows, C);
  const double unbias = rows > 1 ? (double)rows / (double)(rows - 1) : 1.0;
  hipLaunchKernelGGL(bn_finalize_apply_kernel, dim3((C / BNF_SLAB) * chunks), dim3(256), 0, (hipStream_t)stream, partial, tiles, (const bf16_t*)x,
                     (bf16_t*)y, rows, C, chunks, 1.0 / (double)rows, unbias, eps, momentum, mean, rstd, moving_mean, moving_var, gamma, beta, relu);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// backward form: dx = scale * (g - sum(g)/M - xhat * sum(g xhat)/M) (+ dadd); g already carries the activation mask
__global__ __launch_bounds__(256) void bn_bwd_finalize_apply_kernel(const float* __restrict__ partial, int tiles, const bf16_t* __restrict__ x,
                                                                    const bf16_t* __restrict__ g, bf16_t* dx, const bf16_t* dadd, int64_t rows, int C,
                                                                    int chunks, float inv_rows, const float* __restrict__ mean,
                                                                    const float* __restrict__ rstd, const float* __restrict__ gamma, float* dgamma,
                                                                    float* dbeta) {
  __shared__ float tab[5][BNF_SLAB];      // sum g / M, sum g xhat / M, mean, rstd, rstd * gamma
  const int slab = blockIdx.x / chunks, chunk = blockIdx.x - slab * chunks, c0 = slab * BNF_SLAB;
  const int cg = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  const int64_t per = (rows + chunks - 1) / chunks, ra = (int64_t)chunk * per, rb = ra + per < rows ? ra + per : rows;
  const size_t col = (size_t)c0 + cg * 8;
  // (the first FOUR rows of x / g / dadd are requested before the partial sums are reduced: see bn_finalize_apply_kernel; a thread
  //  owns ~8 rows, so the launch is two batches of loads deep instead of four)
  int64_t r = ra + r0;
  const bool pre = r + 96 < rb;
  const u32x4 z4 = {0u, 0u, 0u, 0u};
  u32x4 px[4] = {z4, z4, z4, z4}, pg[4] = {z4, z4, z4, z4}, pd[4] = {z4, z4, z4, z4};
  if (pre) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t o = (size_t)(r + 32 * k) * C + col;
      px[k] = *reinterpret_cast<const u32x4*>(x + o);
      pg[k] = *reinterpret_cast<const u32x4*>(g + o);
      if (dadd) pd[k] = *reinterpret_cast<const u32x4*>(dadd + o);
    }
  }
  {
    const int cl = threadIdx.x >> 2, c = c0 + cl;
    // per-channel constants requested with the rows (independent of the sums); scale = rstd * gamma goes through the table as well -
    // read from global memory after the barrier, the 8 gamma values of a thread were 8 dependent round trips in every workgroup
    const float mc = mean[c], rc = rstd[c], gc = gamma ? gamma[c] : 1.f;
    double s, q;
    bnf_slab_sums(partial, tiles, C, c0, s, q);
    if ((threadIdx.x & 3) == 0) {
      const float sf = (float)s, qf = (float)q;
      tab[0][cl] = sf * inv_rows;
      tab[1][cl] = qf * inv_rows;
      tab[2][cl] = mc;
      tab[3][cl] = rc;
      tab[4][cl] = gamma ? rc * gc : rc;
      if (chunk == 0) {
        if (dbeta) dbeta[c] = sf;
        if (dgamma) dgamma[c] = qf;
      }
    }
  }
  __syncthreads();
  float k1[8], k2[8], mu[8], rs[8], sc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    k1[e] = tab[0][cg * 8 + e]; k2[e] = tab[1][cg * 8 + e]; mu[e] = tab[2][cg * 8 + e]; rs[e] = tab[3][cg * 8 + e];
    sc[e] = tab[4][cg * 8 + e];
  }
  // same arithmetic per element as before (fp32, same order): dx = scale * (g - k1 - xhat * k2) (+ dadd)
  auto one = [&](size_t off, const u32x4 xr, const u32x4 gr, const u32x4 dr) {
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xl = h16lo_to_f32(xr[e]), xh_ = h16hi_to_f32(xr[e]);
      const float gl = h16lo_to_f32(gr[e]), gh = h16hi_to_f32(gr[e]);
      const float xhl = (xl - mu[2 * e]) * rs[2 * e], xhh = (xh_ - mu[2 * e + 1]) * rs[2 * e + 1];
      float ol = sc[2 * e] * (gl - k1[2 * e] - xhl * k2[2 * e]), oh = sc[2 * e + 1] * (gh - k1[2 * e + 1] - xhh * k2[2 * e + 1]);
      if (dadd) { ol += h16lo_to_f32(dr[e]); oh += h16hi_to_f32(dr[e]); }
      o[e] = pack_bf16x2(ol, oh);
    }
    *reinterpret_cast<u32x4*>(dx + off) = o;
  };
  if (pre) {
#pragma unroll
    for (int k = 0; k < 4; ++k) one((size_t)(r + 32 * k) * C + col, px[k], pg[k], pd[k]);
    r += 128;
  }
  for (; r + 96 < rb; r += 128) {          // four rows in flight per thread
    u32x4 vx[4], vg[4], vd[4] = {z4, z4, z4, z4};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t o = (size_t)(r + 32 * k) * C + col;
      vx[k] = *reinterpret_cast<const u32x4*>(x + o);
      vg[k] = *reinterpret_cast<const u32x4*>(g + o);
      if (dadd) vd[k] = *reinterpret_cast<const u32x4*>(dadd + o);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) one((size_t)(r + 32 * k) * C + col, vx[k], vg[k], vd[k]);
  }
  for (; r < rb; r += 32) {
    const size_t o = (size_t)r * C + col;
    const u32x4 vx = *reinterpret_cast<const u32x4*>(x + o), vg = *reinterpret_cast<const u32x4*>(g + o);
    const u32x4 vd = dadd ? *reinterpret_cast<const u32x4*>(dadd + o) : z4;
    one(o, vx, vg, vd);
  }
}

static int bn_bwd_fused_launch(const void* x, const void* g, void* dx, const void* dadd, int64_t rows, int C, const float* mean, const float* rstd,
                               const float* gamma, const float* partial, int tiles, float* dgamma, float* dbeta, int accumulate_dx, hipStream_t s) {
  const int chunks = bn_fused_chunks(rows, C);
  hipLaunchKernelGGL(bn_bwd_finalize_apply_kernel, dim3((C / BNF_SLAB) * chunks), dim3(256), 0, s, partial, tiles, (const bf16_t*)x, (const bf16_t*)g,
                     (bf16_t*)dx, accumulate_dx ? (const bf16_t*)dadd : (const bf16_t*)nullptr, rows, C, chunks, (float)(1.0 / (double)rows), mean, rstd,
                     gamma, dgamma, dbeta);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// [2][C][tiles] epilogue partials -> sums (same contract as bn_bwd_finalize_kernel); one workgroup per channel
__global__ __launch_bounds__(256) void bn_bwd_finalize_tiles_kernel(const float* __restrict__ partial, int tiles, int C, float* sums,
                                                                    float* dgamma, float* dbeta) {
  __shared__ double sh[2][4];
  const int c = blockIdx.x;
  double S, Q;
  bnf_channel_sums(partial + (size_t)c * tiles, partial + ((size_t)C + c) * tiles, tiles, sh, S, Q);
  if (threadIdx.x != 0) return;
  sums[c] = (float)S;
  sums[C + c] = (float)Q;
  if (dbeta) dbeta[c] = (float)S;
  if (dgamma) dgamma[c] = (float)Q;
}

extern "C" int stp_bn_backward_slots(const void* x, const void* g, void* dx, int32_t dtype, int64_t rows, int32_t C, const float* mean,
                                     const float* rstd, const float* gamma, const int64_t* slots, int32_t nslots, float* dgamma,
                                     float* dbeta, int32_t accumulate_dx, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !g || !dx || !mean || !rstd || !slots || rows <= 0 || C <= 0 || (C & 3) || nslots < 1 || (nslots & (nslots - 1))) return STP_E_BADARG;
  return bn_bwd_apply_launch(x, g, dx, dtype, rows, C, mean, rstd, gamma, nullptr, nullptr, 0, accumulate_dx, (const long long*)slots, nslots, dgamma,
                             dbeta, nullptr, (hipStream_t)stream);
}

extern "C" int stp_bn_backward_fused_add(const void* x, const void* g, void* dx, const void* dadd, int32_t dtype, int64_t rows, int32_t C,
                                     const float* mean, const float* rstd, const float* gamma, const float* partial,
                                     int32_t tiles, float* dgamma, float* dbeta, int32_t accumulate_dx, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!x || !g || !dx || (accumulate_dx && !dadd) || !mean || !rstd || !partial || !workspace || rows <= 0 || C <= 0 || (C & 3) || tiles <= 0) return STP_E_BADARG;
  if (workspace_bytes < stp_bn_workspace_bytes(C)) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (bn_fused_ok(dtype, rows, C, tiles))      // one launch: every workgroup reduces the partial sums of its own 64-channel slab
    return bn_bwd_fused_launch(x, g, dx, dadd, rows, C, mean, rstd, gamma, partial, tiles, dgamma, dbeta, accumulate_dx, s);
  float* sums = (float*)workspace + (size_t)(BN_MAX_BLOCKS - 1) * 2 * C;
  hipLaunchKernelGGL(bn_bwd_finalize_tiles_kernel, dim3(C), dim3(256), 0, s, partial, tiles, C, sums, dgamma, dbeta);
  STP_LAUNCH_CHECK();
  // the ReLU mask is already folded into g
  return bn_bwd_apply_launch(x, g, dx, dtype, rows, C, mean, rstd, gamma, nullptr, sums, 0, accumulate_dx, nullptr, 0, nullptr, nullptr, dadd, s);
}

extern "C" int stp_bn_backward_fused(const void* x, const void* g, void* dx, int32_t dtype, int64_t rows, int32_t C,
                                     const float* mean, const float* rstd, const float* gamma, const float* partial,
                                     int32_t tiles, float* dgamma, float* dbeta, int32_t accumulate_dx, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return stp_bn_backward_fused_add(x, g, dx, dx, dtype, rows, C, mean, rstd, gamma, partial, tiles, dgamma, dbeta, accumulate_dx, workspace,
                                   workspace_bytes, stream);
}
