// Convolution weight gradient as a pixel-reduction GEMM on MFMA (gfx950).
//
//   dW[co][k] = sum_p dY[p][co] * V[p][k]      p = (n,ho,wo),  k = (kh*KW + kw)*Ctot + c
//
// Both operands live in HBM with the reduction index (pixels) as the SLOW dimension and
// channels contiguous (NHWC), the opposite of what an MFMA fragment wants (8 consecutive
// reduction elements per lane).  Tiles are therefore staged pixel-major in LDS and
//   * bf16: fetched with ds_read_b64_tr_b16, the gfx950 transpose read: a 16-lane group reads a
//     [4 pixels][16 channels] block and lane i receives channel i of the 4 pixels;
//   * fp32: v_mfma_f32_16x16x4_f32 takes ONE element per lane, so plain ds_read_b32 suffices.
// Only the (lane, slot) -> pixel assignment has to agree between the A and B fragments; it is
// chosen so that a 32-lane access touches 8 consecutive pixel rows, which together with a
// 32-byte-unit XOR swizzle makes the transpose reads bank-conflict free.
// The im2col operand V is gathered on the fly exactly as in conv_igemm.hip (nearest-2x /
// zero-insert / concat folded in).  Pixels are partitioned over `splits` slabs (split-K) that
// a second kernel sums in fixed order: deterministic, no atomics.
//
// This unit: the GEMM kernels (register-staged and LDS-DMA ring), the reduces of plain [splits][Cout][K] slabs, the single-layer
// planner and every stp_conv2d_wgrad* / stp_wgrad_reduce_* entry point.  The row-of-taps kernels are in conv_wgrad_row.hip, the
// all-taps kernels in conv_wgrad_taps9.hip, the grouped launch in conv_wgrad_group.hip; conv_wgrad.h holds what they share.
#include "conv_wgrad.h"
#include <cstdlib>


// One pixel-step of MFMAs for this wave (transpose reads for bf16, scalar reads for fp32).
template <typename T, int BM, int BN, int WM, int WN>
__device__ __forceinline__ void wgrad_compute(const char* sa, int wm, int wn, int lr, int lg,
                                              f32x4 (&acc)[BM / WM / 16][BN / WN / 16]) {
  constexpr int SZ = (int)sizeof(T);
  constexpr int PK = 128 / SZ;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int ROWA = BM * SZ, ROWB = BN * SZ;
    const char* sb = sa + PK * ROWA;
    const int ca = (wm * (BM / WM)) * SZ, cb = (wn * (BN / WN)) * SZ;  // wave column origin, bytes
    if constexpr (sizeof(T) == 2) {
      // 64 pixels per step = 2 MFMA k-steps of 32 pixels.  Lane group g owns pixels
      // {4g..4g+3} and {16+4g..16+4g+3} of the 32: two transpose reads of a [4][16] block.
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        u32x4 fa[TM], fb[TN];
        const int prow = c * 32 + lg * 4 + (lr >> 2);
        const int qb = (lr & 3) * 8;  // this lane's 8-byte quad inside the 32-byte block
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int byte = ca + i * 32 + qb;
          s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(sa + tile_addr<ROWA>(prow, byte)));
          s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(sa + tile_addr<ROWA>(prow + 16, byte)));
          u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          fa[i] = u32x4{l2.x, l2.y, h2.x, h2.y};
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int byte = cb + j * 32 + qb;
          s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(sb + tile_addr<ROWB>(prow, byte)));
          s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
              (__attribute__((address_space(3))) s16x4*)(sb + tile_addr<ROWB>(prow + 16, byte)));
          u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          fb[j] = u32x4{l2.x, l2.y, h2.x, h2.y};
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = mfma16_16x16x32(fa[i], fb[j], acc[i][j]);
      }
    } else {
      // fp32: 32 pixels per step = 8 MFMA k-steps of 4 pixels; lane group g owns pixel 4s+g.
#pragma unroll
      for (int s = 0; s < PK / 4; ++s) {
        const int prow = s * 4 + lg;
        float fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
          fa[i] = *reinterpret_cast<const float*>(sa + tile_addr<ROWA>(prow, ca + (i * 16 + lr) * 4));
#pragma unroll
        for (int j = 0; j < TN; ++j)
          fb[j] = *reinterpret_cast<const float*>(sb + tile_addr<ROWB>(prow, cb + (j * 16 + lr) * 4));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
      }
    }
  }

template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void wgrad_write_slab(const WgradArgs& a, int split, int cout0, int k0, int wm, int wn, int lr, int lg,
                                                 f32x4 (&acc)[BM / WM / 16][BN / WN / 16]) {
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  float* out = a.out + (size_t)split * a.Cout * a.K;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int kc = k0 + wn * (BN / WN) + j * 16 + lr;
      const int co = cout0 + wm * (BM / WM) + i * 16 + lg * 4;
      if (kc >= a.K) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (co + r < a.Cout) out[(size_t)(co + r) * a.K + kc] = acc[i][j][r];
    }
  }
}

template <typename T, int BM, int BN, int WM, int WN, bool C4>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a) {
  static_assert(WM * WN == 4, "4 waves");
  constexpr int SZ = (int)sizeof(T);
  constexpr int VEC = Elem<T>::VEC;
  constexpr int PK = 128 / SZ;  // pixels per step: 64 bf16 / 32 fp32
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int ROWA = BM * SZ, ROWB = BN * SZ;
  constexpr int VPRA = BM / VEC, VPRB = BN / VEC;       // 16-byte vectors per pixel row
  constexpr int NVA = (PK * VPRA + 255) / 256, NVB = (PK * VPRB + 255) / 256;  // vectors per thread
  constexpr int STAGE = PK * (ROWA + ROWB);

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int tiles = a.ntile_m * a.ntile_n;
  const int bid = a.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;  // the tiles of one split (same pixels) share an XCD's L2
  const int split = bid / tiles;
  const int t = bid - split * tiles;
  const int tile_m = t % a.ntile_m, tile_n = t / a.ntile_m;
  const int cout0 = tile_m * BM, k0 = tile_n * BN;
  const int step0 = split * a.steps_per_split;
  const int step1 = min(step0 + a.steps_per_split, a.nsteps);

  // ---- fixed per-thread column metadata ---------------------------------------------------
  const int colA = (tid % VPRA) * VEC;  // cout offset within tile
  const int colB = (tid % VPRB) * VEC;  // k offset within tile
  const int rowA0 = tid / VPRA, rowB0 = tid / VPRB;
  const bool coA_ok = (cout0 + colA) < a.Cout;
  const int kB = k0 + colB;
  const bool kB_ok = kB < a.K;
  int kh, kw, ci, cs, mode, Hs, Ws;
  const char* base;
  if constexpr (C4) {
    const uint32_t pos = (uint32_t)kB >> 2;
    kh = (int)fdiv(pos, a.divKW);
    kw = (int)pos - kh * a.KW;
    ci = 0; cs = 4; mode = 0; Hs = a.Hs0; Ws = a.Ws0; base = a.src0;
  } else {
    const uint32_t pos = fdiv((uint32_t)kB, a.divC);
    ci = kB - (int)pos * a.Ctot;
    kh = (int)fdiv(pos, a.divKW);
    kw = (int)pos - kh * a.KW;
    const bool first = ci < a.C0;
    base = first ? a.src0 : a.src1;
    cs = first ? a.C0 : a.C1;
    mode = first ? a.mode : 0;
    Hs = first ? a.Hs0 : a.Hv;
    Ws = first ? a.Ws0 : a.Wv;
    if (!first) ci -= a.C0;
  }

  u32x4 ra[NVA], rb[NVB];

  auto load_tile = [&](int step) {
    const int p0 = step * PK;
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
      const int row = rowA0 + i * (256 / VPRA);
      const int p = p0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (coA_ok && row < PK && p < a.P)
        v = *reinterpret_cast<const u32x4*>(a.dy + ((size_t)p * a.Cout + cout0 + colA) * SZ);
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int row = rowB0 + i * (256 / VPRB);
      const int p = p0 + row;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (kB_ok && row < PK && p < a.P) {
        const uint32_t n = fdiv((uint32_t)p, a.divHoWo);
        const uint32_t rem = (uint32_t)p - n * (uint32_t)a.HoWo;
        const uint32_t ho = fdiv(rem, a.divWo);
        const uint32_t wo = rem - ho * (uint32_t)a.Wo;
        const int hv = (int)ho * a.stride - a.pad + kh;
        const int wv = (int)wo * a.stride - a.pad + kw;
        if constexpr (C4) {
          if ((unsigned)hv < (unsigned)a.Hv) {
            const char* rowp = base + ((size_t)((int)n * Hs + hv) * Ws) * (4 * SZ);
            if ((unsigned)wv < (unsigned)a.Wv) {
              u32x2 q = *reinterpret_cast<const u32x2*>(rowp + (size_t)wv * (4 * SZ));
              v.x = q.x; v.y = q.y;
            }
            if ((unsigned)(wv + 1) < (unsigned)a.Wv) {
              u32x2 q = *reinterpret_cast<const u32x2*>(rowp + (size_t)(wv + 1) * (4 * SZ));
              v.z = q.x; v.w = q.y;
            }
          }
        } else {
          bool ok = (unsigned)hv < (unsigned)a.Hv && (unsigned)wv < (unsigned)a.Wv;
          if (mode == STP_SRC_ZEROINS2X) ok = ok && (((hv | wv) & 1) == 0);
          const int hs = mode ? (hv >> 1) : hv, ws = mode ? (wv >> 1) : wv;
          if (ok) v = *reinterpret_cast<const u32x4*>(base + (((size_t)((int)n * Hs + hs) * Ws + ws) * cs + ci) * SZ);
        }
      }
      rb[i] = v;
    }
  };

  auto store_tile = [&](int buf) {
    char* sa = smem + buf * STAGE;
    char* sb = sa + PK * ROWA;
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
      const int row = rowA0 + i * (256 / VPRA);
      if (row < PK) *reinterpret_cast<u32x4*>(sa + tile_addr<ROWA>(row, colA * SZ)) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int row = rowB0 + i * (256 / VPRB);
      if (row < PK) *reinterpret_cast<u32x4*>(sb + tile_addr<ROWB>(row, colB * SZ)) = rb[i];
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int lr = lane & 15, lg = lane >> 4;
  auto compute = [&](int buf) { wgrad_compute<T, BM, BN, WM, WN>(smem + buf * STAGE, wm, wn, lr, lg, acc); };

  if (step0 < step1) {
    load_tile(step0);
    store_tile(0);
    __syncthreads();
    for (int st = step0; st < step1; ++st) {
      const int cur = (st - step0) & 1;
      if (st + 1 < step1) load_tile(st + 1);
      compute(cur);
      if (st + 1 < step1) store_tile(cur ^ 1);
      __syncthreads();
    }
  }

  wgrad_write_slab<BM, BN, WM, WN>(a, split, cout0, k0, wm, wn, lr, lg, acc);
}


// ------------------------------------------------------------------------------------------------
// Direct-to-LDS variant: every 16-byte vector of both tiles is fetched with `buffer_load_dwordx4 ... lds`
// (32-bit offsets, out-of-range -> 0 for padding / tails), STAGES-deep ring with counted vmcnt.  The LDS
// image of an LDS-DMA is lane-linear, so the 32-byte-unit XOR swizzle is applied to the SOURCE column:
// a thread owns a fixed PHYSICAL 16-byte slot and fetches the logical column that lives there (the
// swizzle key only depends on row&7 and every pass advances the row by a multiple of 8).
//
// ROWU ("uniform rows"): when Wo % PK == 0, or PK % Wo == 0 and Ho*Wo % PK == 0 (every power-of-two feature map), the
// PK pixels of a step are (ho0 + r / Wo, wo0 + r % Wo) of ONE image with wave-uniform (n, ho0, wo0): the two
// divisions per gathered row become per-thread constants plus scalar arithmetic - the address VALU work was
// what bounded this kernel (scratch/whatif_bench.py: loads-only took 80% of the full time).
template <typename T, int BM, int BN, int WM, int WN, int STAGES, bool ROWU>
__global__ __launch_bounds__(256) void conv_wgrad_dma_kernel(const WgradArgs a) {
  static_assert(WM * WN == 4 && STAGES >= 2, "config");
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int SZ = (int)sizeof(T);
  constexpr int PK = 128 / SZ;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int ROWA = BM * SZ, ROWB = BN * SZ;
  constexpr int VPRA = ROWA / 16, VPRB = ROWB / 16;
  constexpr int RPA = 256 / VPRA, RPB = 256 / VPRB;            // rows per pass
  constexpr int NVA = (PK + RPA - 1) / RPA, NVB = (PK + RPB - 1) / RPB;
  static_assert((NVA == 1 || RPA % 8 == 0) && (NVB == 1 || RPB % 8 == 0), "swizzle key must not change between passes");
  constexpr int STAGE = PK * (ROWA + ROWB);
  constexpr int L = NVA + NVB;
  constexpr int DUMP = STAGES * STAGE;  // 4 KiB sink for the lane groups that have no row in a pass

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  const int tiles = a.ntile_m * a.ntile_n;
  const int bid = a.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;  // the tiles of one split (same pixels) share an XCD's L2
  const int split = bid / tiles;
  const int t = bid - split * tiles;
  const int tile_m = t % a.ntile_m, tile_n = t / a.ntile_m;
  const int cout0 = tile_m * BM, k0 = tile_n * BN;
  const int step0 = split * a.steps_per_split;
  const int step1 = min(step0 + a.steps_per_split, a.nsteps);

  const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.bytesdy, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)a.src0, 0, a.bytes0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.src1 ? a.src1 : a.src0), 0, a.src1 ? a.bytes1 : 0u, 0x00020000);

  // fixed per-thread columns (logical column stored at this thread's physical slot)
  const int rowA0 = tid / VPRA, rowB0 = tid / VPRB;
  const int colA = (tile_addr<ROWA>(rowA0, (tid % VPRA) * 16) - rowA0 * ROWA) / SZ;
  const int colB = (tile_addr<ROWB>(rowB0, (tid % VPRB) * 16) - rowB0 * ROWB) / SZ;
  const bool coA_ok = (cout0 + colA) < a.Cout;
  const int kB = k0 + colB;
  const bool kB_ok = kB < a.K;
  const uint32_t pos = fdiv((uint32_t)kB, a.divC);
  int ci = kB - (int)pos * a.Ctot;
  const int kh = (int)fdiv(pos, a.divKW);
  const int kw = (int)pos - kh * a.KW;
  const bool first = ci < a.C0;
  if (!first) ci -= a.C0;
  const int cs = first ? a.C0 : a.C1;
  const int sh = (first && a.mode) ? 1 : 0;
  const bool zins = first && a.mode == STP_SRC_ZEROINS2X;
  const int Hs = first ? a.Hs0 : a.Hv, Ws = first ? a.Ws0 : a.Wv;

  // ROWU: per-thread constants of its rows
  int hc[NVB], wc[NVB];
  uint32_t rowa[NVA];
  const uint32_t pixb = (uint32_t)cs * SZ, imgb = (uint32_t)Hs * (uint32_t)Ws * pixb, cib = (uint32_t)ci * SZ;
  if constexpr (ROWU) {
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int row = rowB0 + i * RPB;
      const int dho = a.Wo >= PK ? 0 : row / a.Wo;
      const int dwo = a.Wo >= PK ? row : row - dho * a.Wo;
      hc[i] = dho * a.stride - a.pad + kh;
      wc[i] = dwo * a.stride - a.pad + kw;
    }
#pragma unroll
    for (int i = 0; i < NVA; ++i) rowa[i] = ((uint32_t)(rowA0 + i * RPA) * (uint32_t)a.Cout + (uint32_t)(cout0 + colA)) * SZ;
  }

  auto issue_tile = [&](int step, int buf) {
    const int p0 = step * PK;
    char* sa = smem + buf * STAGE;
    char* sb = sa + PK * ROWA;
    if constexpr (ROWU) {
      // wave-uniform decomposition of the step's first pixel (P % PK == 0 here: no ragged tail)
      const uint32_t n = fdiv((uint32_t)p0, a.divHoWo);
      const uint32_t rem = (uint32_t)p0 - n * (uint32_t)a.HoWo;
      const uint32_t ho0 = fdiv(rem, a.divWo);
      const uint32_t wo0 = rem - ho0 * (uint32_t)a.Wo;
      const int hs = (int)ho0 * a.stride, wsb = (int)wo0 * a.stride;
      const uint32_t abase = (uint32_t)p0 * (uint32_t)a.Cout * SZ;
      const uint32_t nb = n * imgb + cib;
#pragma unroll
      for (int i = 0; i < NVA; ++i) {
        const bool act = (i * 256 + wave * 64) / VPRA < PK;
        const bool rok = NVA * RPA == PK || (rowA0 + i * RPA) < PK;
        char* dst = act ? sa + (i * 256 + wave * 64) * 16 : smem + DUMP + wave * 1024;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsd, (__attribute__((address_space(3))) void*)dst, 16,
                                                 (coA_ok && rok) ? abase + rowa[i] : STP_OOB, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < NVB; ++i) {
        const bool act = (i * 256 + wave * 64) / VPRB < PK;
        const bool rok = NVB * RPB == PK || (rowB0 + i * RPB) < PK;
        const int hv = hs + hc[i], wv = wsb + wc[i];
        bool ok = kB_ok && rok && (unsigned)hv < (unsigned)a.Hv && (unsigned)wv < (unsigned)a.Wv;
        if (zins) ok = ok && (((hv | wv) & 1) == 0);
        const uint32_t off = nb + ((uint32_t)(hv >> sh) * (uint32_t)Ws + (uint32_t)(wv >> sh)) * pixb;
        char* dst = act ? sb + (i * 256 + wave * 64) * 16 : smem + DUMP + wave * 1024;
        if (first) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (__attribute__((address_space(3))) void*)dst, 16, ok ? off : STP_OOB, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (__attribute__((address_space(3))) void*)dst, 16, ok ? off : STP_OOB, 0, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int i = 0; i < NVA; ++i) {
      const int row = rowA0 + i * RPA;
      const int p = p0 + row;
      const bool act = (i * 256 + wave * 64) / VPRA < PK;   // wave-uniform: does this pass have rows for this wave?
      const uint32_t off = (coA_ok && row < PK && p < a.P) ? ((uint32_t)p * (uint32_t)a.Cout + (uint32_t)(cout0 + colA)) * SZ : STP_OOB;
      char* dst = act ? sa + (i * 256 + wave * 64) * 16 : smem + DUMP + wave * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsd, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int row = rowB0 + i * RPB;
      const int p = p0 + row;
      const bool act = (i * 256 + wave * 64) / VPRB < PK;
      uint32_t off = STP_OOB;
      if (kB_ok && row < PK && p < a.P) {
        const uint32_t n = fdiv((uint32_t)p, a.divHoWo);
        const uint32_t rem = (uint32_t)p - n * (uint32_t)a.HoWo;
        const uint32_t ho = fdiv(rem, a.divWo);
        const uint32_t wo = rem - ho * (uint32_t)a.Wo;
        const int hv = (int)ho * a.stride - a.pad + kh;
        const int wv = (int)wo * a.stride - a.pad + kw;
        bool ok = (unsigned)hv < (unsigned)a.Hv && (unsigned)wv < (unsigned)a.Wv;
        if (zins) ok = ok && (((hv | wv) & 1) == 0);
        if (ok) off = ((n * (uint32_t)Hs + (uint32_t)(hv >> sh)) * (uint32_t)Ws + (uint32_t)(wv >> sh)) * (uint32_t)cs * SZ + (uint32_t)ci * SZ;
      }
      char* dst = act ? sb + (i * 256 + wave * 64) * 16 : smem + DUMP + wave * 1024;
      if (first) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
      else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (__attribute__((address_space(3))) void*)dst, 16, off, 0, 0, 0);
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int lr = lane & 15, lg = lane >> 4;

  const int nst = step1 - step0;
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nst) issue_tile(step0 + s, s);
  int buf = 0, nbuf = STAGES - 1;
  for (int st = 0; st < nst; ++st) {
    const int ahead = nst - 1 - st;
    if (STAGES >= 3 && ahead >= STAGES - 2) wait_vmcnt<(STAGES >= 3 ? (STAGES - 2) : 0) * L>();
    else if (STAGES >= 4 && ahead == 1) wait_vmcnt<L>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
#if !defined(STP_EXP) || STP_EXP != 2  // what-if builds (scratch/exp_build.sh): 1 = no MFMA work, 2 = no loads in the loop
    if (st + STAGES - 1 < nst) issue_tile(step0 + st + STAGES - 1, nbuf);
#endif
#if !defined(STP_EXP) || STP_EXP != 1
    wgrad_compute<T, BM, BN, WM, WN>(smem + buf * STAGE, wm, wn, lr, lg, acc);
#endif
    buf = (buf + 1 == STAGES) ? 0 : buf + 1;
    nbuf = (nbuf + 1 == STAGES) ? 0 : nbuf + 1;
  }
  wgrad_write_slab<BM, BN, WM, WN>(a, split, cout0, k0, wm, wn, lr, lg, acc);
#endif
}

// dw[i] (+)= sum_k slabs[k][i], 4 floats per thread (count is a multiple of 4: Cout*K with K % 4 == 0)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dw, int64_t count,
                                                           int splits, int accumulate) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= count) return;
  f32x4 s = *reinterpret_cast<const f32x4*>(slabs + i);
  int k = 1;
  for (; k + 3 < splits; k += 4) {      // four slab loads in flight; same order of additions
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(slabs + (size_t)k * count + i), a1 = *reinterpret_cast<const f32x4*>(slabs + (size_t)(k + 1) * count + i);
    const f32x4 a2 = *reinterpret_cast<const f32x4*>(slabs + (size_t)(k + 2) * count + i), a3 = *reinterpret_cast<const f32x4*>(slabs + (size_t)(k + 3) * count + i);
    s += a0; s += a1; s += a2; s += a3;
  }
  for (; k < splits; ++k) s += *reinterpret_cast<const f32x4*>(slabs + (size_t)k * count + i);
  if (accumulate) s += *reinterpret_cast<const f32x4*>(dw + i);
  *reinterpret_cast<f32x4*>(dw + i) = s;
}

// Many slabs, few elements (small-channel layers: up to 1024 slabs of a few thousand floats): 16 lanes walk
// the slabs in parallel for each group of 4 elements, then a fixed-shape LDS tree combines them.
__global__ __launch_bounds__(256) void wgrad_reduce_wide_kernel(const float* __restrict__ slabs, float* __restrict__ dw, int64_t count,
                                                                int splits, int accumulate) {
  __shared__ f32x4 sh[16][16];
  const int ev = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int64_t i = ((int64_t)blockIdx.x * 16 + ev) * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i < count) {
    // eight loads in flight per lane (the loop is latency-bound otherwise: 13.5 us for 10-20 MB of slabs); same order of additions
    int k = sl;
    for (; k + 112 < splits; k += 128) {
      f32x4 a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = *reinterpret_cast<const f32x4*>(slabs + (size_t)(k + 16 * u) * count + i);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += a[u];
    }
    for (; k < splits; k += 16) s += *reinterpret_cast<const f32x4*>(slabs + (size_t)k * count + i);
  }
  sh[sl][ev] = s;
  __syncthreads();
  for (int w = 8; w > 0; w >>= 1) {
    if (sl < w) sh[sl][ev] += sh[sl + w][ev];
    __syncthreads();
  }
  if (sl == 0 && i < count) {
    f32x4 r = sh[0][ev];
    if (accumulate) r += *reinterpret_cast<const f32x4*>(dw + i);
    *reinterpret_cast<f32x4*>(dw + i) = r;
  }
}

// ---- batched reduce of lone weight gradients (round 6) ---------------------------------------------------------------------------------
// The bottleneck ResNets' 1x1 layers never neighbour a layer of their own class, so each ran partial launch + reduce launch: 59 reduces per
// step on FPN/ResNet50, 30 on PSPNet/ResNet101 at ~9 us each (profiles/r06a_floor_config{3,4}.txt: 576 / 260 us = 3.7 % / 2.9 % of the
// step) for 1 - 16 MB of slabs - launch latency, not bytes.  The weight gradient feeds nothing but the optimizer: a layer whose slabs are
// the plain [splits][Cout * K] form keeps them in a workspace OF ITS OWN and its reduce joins a table; one launch (grid y = layer) reduces
// up to STP_WGRAD_REDUCE_BATCH layers.  Same 16-lane walk + fixed-shape tree as wgrad_reduce_wide_kernel: deterministic.
struct WgReduceDesc {
  const float* slabs;
  float* dw;
  int64_t count;
  int32_t splits, accumulate;
};

__global__ __launch_bounds__(256) void wgrad_reduce_batched_kernel(const WgReduceDesc* __restrict__ D) {
  const WgReduceDesc d = D[blockIdx.y];
  if ((int64_t)blockIdx.x * 64 >= d.count) return;                      // (workgroup-uniform: the grid is sized for the largest layer)
  __shared__ f32x4 sh[16][16];
  const int ev = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int64_t i = ((int64_t)blockIdx.x * 16 + ev) * 4;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (i < d.count) {
    int k = sl;
    for (; k + 112 < d.splits; k += 128) {      // eight loads in flight per lane; same order of additions as the one-by-one loop
      f32x4 a[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) a[u] = *reinterpret_cast<const f32x4*>(d.slabs + (size_t)(k + 16 * u) * d.count + i);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += a[u];
    }
    for (; k < d.splits; k += 16) s += *reinterpret_cast<const f32x4*>(d.slabs + (size_t)k * d.count + i);
  }
  sh[sl][ev] = s;
  __syncthreads();
  for (int w = 8; w > 0; w >>= 1) {
    if (sl < w) sh[sl][ev] += sh[sl + w][ev];
    __syncthreads();
  }
  if (sl == 0 && i < d.count) {
    f32x4 r = sh[0][ev];
    if (d.accumulate) r += *reinterpret_cast<const f32x4*>(d.dw + i);
    *reinterpret_cast<f32x4*>(d.dw + i) = r;
  }
}

// ---- host side: the single-layer planner and entry points --------------------------------------------------------------------------
WgradPath wgrad_path(const stp_wgrad_params* p, int variant) {
  if (!p) return WG_PATH_GEMM;      // (wgrad_fill refuses it)
  if (variant == 0 && p->splits == 0 && stp_wgrad_sc_eligible(p)) return WG_PATH_SC;
  if (variant == 4 || (variant == 0 && wgrad_row_auto(p))) return WG_PATH_ROW;
  return WG_PATH_GEMM;
}

// The split count of a plan whose tile, ntile_m, ntile_n and nsteps are set.  asked > 0: the caller's count; otherwise
// fill the machine EXACTLY once: workgroup slots = CUs x co-resident workgroups (LDS-limited: 2 for the 128-row tiles,
// 3 for the 64-row tiles; `target` > 0 replaces the slots), splits = floor(slots / tiles).  One workgroup more than the slots costs a
// whole extra round (scratch/wgrad_split_sweep.py: 128->128 @64x64, 9 tiles: 57 splits = 513 workgroups 49 us, 56 splits = 504
// workgroups 33 us); every split also costs a slab write + read of Cout*K floats, so fewer is better at equal fill.
void wgrad_choose_splits(WgradPlan& w, int asked, int target) {
  int splits = asked;
  if (splits <= 0) {
    const int slots = target > 0 ? target : stp_cu_count() * (w.bm == 64 ? 3 : 2);
    splits = slots / (w.ntile_m * w.ntile_n);
    if (splits < 1) splits = 1;
    const int max_by_steps = w.nsteps / 8 > 0 ? w.nsteps / 8 : 1;  // keep >= 8 steps per split
    if (splits > max_by_steps) splits = max_by_steps;
    if (splits > 512) splits = 512;   // (the stem: 2 tiles x 384 splits = 768 workgroups, 113 -> 88 us)
  }
  if (splits > w.nsteps) splits = w.nsteps;
  if (splits < 1) splits = 1;
  w.steps_per_split = ceil_div(w.nsteps, splits);
  w.splits = ceil_div(w.nsteps, w.steps_per_split);
}

static WgradPlan plan_wgrad(const stp_wgrad_params* p) {
  WgradPlan w;
  if (p->splits == 0 && stp_wgrad_sc_eligible(p)) {
    w.tile = WG_TILE_SC; w.bm = w.bn = 0; w.ntile_m = w.ntile_n = 1;
    w.splits = stp_wgrad_sc_slabs(p); w.steps_per_split = 0; w.nsteps = 0;
    return w;
  }
  const int K = p->KH * p->KW * (p->C0 + p->C1);
  const int pk = p->dtype == STP_H16 ? 64 : 32;
  const int64_t P = (int64_t)p->N * p->Ho * p->Wo;
  if (p->Cout <= 16) { w.tile = 4; w.bm = 16; w.bn = 256; }
  else if (p->Cout <= 32) { w.tile = 3; w.bm = 32; w.bn = 256; }
  else if (p->Cout <= 64) { w.tile = 2; w.bm = 64; w.bn = 128; }
  else { w.tile = 1; w.bm = 128; w.bn = 128; }
  w.ntile_m = ceil_div(p->Cout, w.bm);
  w.ntile_n = ceil_div(K, w.bn);
  w.nsteps = ceil_div(P, pk);
  int target = 0;
  if (p->splits <= 0) {
    static const int env = getenv("STP_WGRAD_BLOCKS") ? atoi(getenv("STP_WGRAD_BLOCKS")) : 0;
    target = env;
  }
  wgrad_choose_splits(w, p->splits, target);
  return w;
}

static WgradPlan plan_wgrad_gemm(const stp_wgrad_params* p) {
  stp_wgrad_params q = *p;
  if (q.splits == 0 && stp_wgrad_sc_eligible(p)) q.splits = -1;  // any non-zero value bypasses the small-channel plan...
  WgradPlan w = plan_wgrad(&q);
  return w;
}

// enough for either kernel family (the automatic choice and the forced GEMM variants)
extern "C" size_t stp_conv2d_wgrad_workspace_bytes(const stp_wgrad_params* p) {
  if (!p) return 0;
  const WgradPlan w = plan_wgrad(p), g = plan_wgrad_gemm(p);
  size_t bytes = wgrad_slab_bytes(p, w.splits > g.splits ? w.splits : g.splits);
  if (wgrad_row_eligible(p)) {
    const size_t rb = wgrad_row_slab_bytes(plan_wgrad_row(p));
    if (rb > bytes) bytes = rb;
  }
  return bytes;
}

template <typename T, int BM, int BN, int WM, int WN, bool C4>
static int launch_wgrad(WgradArgs& a, int splits, hipStream_t s) {
  constexpr int PK = 128 / (int)sizeof(T);
  return launch_wg(conv_wgrad_kernel<T, BM, BN, WM, WN, C4>, a, (size_t)2 * PK * (BM + BN) * sizeof(T), splits, s);
}

template <typename T, int BM, int BN, int WM, int WN, int STAGES>
static int launch_wgrad_dma(WgradArgs& a, int splits, hipStream_t s) {
  constexpr int PK = 128 / (int)sizeof(T);
  const size_t lds = (size_t)STAGES * PK * (BM + BN) * sizeof(T) + 4096;
  if (a.rowu) return launch_wg(conv_wgrad_dma_kernel<T, BM, BN, WM, WN, STAGES, true>, a, lds, splits, s);
  return launch_wg(conv_wgrad_dma_kernel<T, BM, BN, WM, WN, STAGES, false>, a, lds, splits, s);
}

// The GEMM tile number of a plan (plan_wgrad) -> the instance: f(GemmTile<BM, BN, WM, WN>{}).
template <int BM_, int BN_, int WM_, int WN_> struct GemmTile { static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_; };
template <typename F> static int gemm_tile(int tile, F&& f) {
  switch (tile) {
    case 1: return f(GemmTile<128, 128, 2, 2>{});
    case 2: return f(GemmTile<64, 128, 1, 4>{});
    case 3: return f(GemmTile<32, 256, 1, 4>{});
    case 4: return f(GemmTile<16, 256, 1, 4>{});
    default: return STP_E_BADARG;
  }
}

// variant: 0 = auto, 1 = legacy register-staged, 2/3 = DMA ring with that many stages
template <typename T, bool C4>
static int launch_wgrad_tile(WgradArgs& a, const WgradPlan& w, bool dma_ok, int variant, hipStream_t s) {
  constexpr bool f32 = sizeof(T) == 4;
  int v = 1;      // the 4-channel stem form has the register-staged kernel only
  if constexpr (!C4) {
    v = variant;
    // (STP_WGRAD_DMA_STAGES=3: the 3-stage ring for the automatic choice - experiments on the lone 1x1 layers of the bottleneck ResNets,
    //  whose 18-step workgroups wait for every 64-pixel step's LDS-DMA with only one other step in flight)
    static const int dma_auto = (getenv("STP_WGRAD_DMA_STAGES") && atoi(getenv("STP_WGRAD_DMA_STAGES")) == 3) ? 3 : 2;
    if (v == 0) v = dma_ok ? dma_auto : 1;
    if (v >= 2 && (!dma_ok || (f32 && w.tile >= 3))) v = 1;  // fp32 256-column tiles: swizzle key varies per pass
  }
  return gemm_tile(w.tile, [&](auto t) -> int {
    using G = decltype(t);
    if (v == 1) return launch_wgrad<T, G::BM, G::BN, G::WM, G::WN, C4>(a, w.splits, s);
    if constexpr (!C4 && !(f32 && G::BN == 256)) {      // (no fp32 DMA instance for the 256-column tiles: v is 1 there)
      if (v == 2) return launch_wgrad_dma<T, G::BM, G::BN, G::WM, G::WN, 2>(a, w.splits, s);
      if (v == 3) return launch_wgrad_dma<T, G::BM, G::BN, G::WM, G::WN, 3>(a, w.splits, s);
    }
    return STP_E_BADARG;
  });
}

int wgrad_fill(const stp_wgrad_params* p, void* workspace, size_t workspace_bytes, WgradArgs& a, WgradPlan& w, bool* c4_out, bool* dma_out) {
  if (!p || !p->src0 || !p->dy || !p->dw || !workspace) return STP_E_BADARG;
  if (p->dtype != STP_F32 && p->dtype != STP_H16) return STP_E_BADARG;
  const int vec = p->dtype == STP_H16 ? 8 : 4;
  const int sz = p->dtype == STP_H16 ? 2 : 4;
  const bool c4 = (p->dtype == STP_H16) && p->C0 == 4 && p->C1 == 0;
  if (c4) {
    if ((p->KW & 1) || p->src0_mode != STP_SRC_DIRECT) return STP_E_BADARG;
  } else if ((p->C0 % vec) || (p->C1 % vec)) {
    return STP_E_BADARG;
  }
  if (p->Cout % vec) return STP_E_BADARG;
  if (p->C1 > 0 && !p->src1) return STP_E_BADARG;
  if (stp_conv2d_wgrad_workspace_bytes(p) > workspace_bytes) return STP_E_WORKSPACE;
  w = plan_wgrad_gemm(p);
  if (wgrad_slab_bytes(p, w.splits) > workspace_bytes) return STP_E_WORKSPACE;
  a.src0 = (const char*)p->src0; a.src1 = (const char*)p->src1; a.dy = (const char*)p->dy; a.out = (float*)workspace;
  a.N = p->N; a.Hs0 = p->Hs0; a.Ws0 = p->Ws0; a.Hv = p->Hv; a.Wv = p->Wv; a.C0 = p->C0; a.C1 = p->C1;
  a.Ctot = p->C0 + p->C1; a.mode = p->src0_mode;
  a.KH = p->KH; a.KW = p->KW; a.stride = p->stride; a.pad = p->pad; a.Ho = p->Ho; a.Wo = p->Wo; a.Cout = p->Cout;
  a.K = p->KH * p->KW * a.Ctot;
  const int64_t P = (int64_t)p->N * p->Ho * p->Wo;
  if (P >= (1ll << 31)) return STP_E_BADARG;
  a.P = (int)P; a.HoWo = p->Ho * p->Wo;
  a.ntile_m = w.ntile_m; a.ntile_n = w.ntile_n; a.steps_per_split = w.steps_per_split; a.nsteps = w.nsteps;
  // measured per layer (scratch/launch_table.py with and without): the XCD-contiguous order gains 5-10% when one
  // Cout tile covers the layer (Cout <= 128), is neutral for Cout = 512 and loses 35% for Cout = 256
  a.xcd = w.ntile_m == 1;
  {
    const int pk = 128 / sz;
    a.rowu = (p->Wo % pk == 0) || (pk % p->Wo == 0 && a.HoWo % pk == 0);
  }
  a.divC = make_fastdiv((uint32_t)a.Ctot); a.divKW = make_fastdiv((uint32_t)a.KW);
  a.divHoWo = make_fastdiv((uint32_t)a.HoWo); a.divWo = make_fastdiv((uint32_t)a.Wo);
  const int64_t lim = 1ll << 31;
  const int64_t b0 = (int64_t)p->N * p->Hs0 * p->Ws0 * p->C0 * sz, b1 = (int64_t)p->N * p->Hv * p->Wv * p->C1 * sz;
  const int64_t bd = P * p->Cout * sz;
  a.bytes0 = (uint32_t)(b0 < lim ? b0 : 0); a.bytes1 = (uint32_t)(b1 < lim ? b1 : 0); a.bytesdy = (uint32_t)(bd < lim ? bd : 0);
  *c4_out = c4;
  *dma_out = !c4 && b0 < lim && b1 < lim && bd < lim;
  a.pbn.x = nullptr; a.pbn.mean = p->src_bn_mean; a.pbn.rstd = p->src_bn_rstd; a.pbn.gamma = p->src_bn_gamma; a.pbn.beta = p->src_bn_beta;
  a.pbn.relu = p->src_bn_relu;
  return STP_OK;
}

extern "C" int stp_conv2d_wgrad_kernel_id(const stp_wgrad_params* p) {
  if (!p) return 0;
  const WgradPath path = wgrad_path(p, 0);
  return path == WG_PATH_SC ? 1 : path == WG_PATH_ROW ? (p->Cout <= 64 ? 3 : 2) : 0;
}

// Phase 1: per-split partial sums into the workspace slabs.  `variant` as in launch_wgrad_tile.
extern "C" int stp_conv2d_wgrad_partial(const stp_wgrad_params* p, void* workspace, size_t workspace_bytes, int32_t variant,
                                        void* stream) {
  const WgradPath path = wgrad_path(p, variant);
  if (path == WG_PATH_SC) {
    if (!workspace || stp_conv2d_wgrad_workspace_bytes(p) > workspace_bytes) return STP_E_WORKSPACE;
    return stp_wgrad_sc_partial(p, workspace, stream);
  }
  if (p && p->src_bn_mean && path != WG_PATH_ROW) return STP_E_BADARG;   // fused producer BatchNormalization: small-channel and
  WgradArgs a;                                                           // row-of-taps kernels only
  WgradPlan w;
  bool c4, dma;
  const int rc = wgrad_fill(p, workspace, workspace_bytes, a, w, &c4, &dma);
  if (rc != STP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (path == WG_PATH_ROW) {
    if (!wgrad_row_eligible(p) || !dma) return STP_E_BADARG;
    return wgrad_row_partial(p, a, s);
  }
  if (p->dtype == STP_H16)
    return c4 ? launch_wgrad_tile<bf16_t, true>(a, w, dma, variant, s) : launch_wgrad_tile<bf16_t, false>(a, w, dma, variant, s);
  return launch_wgrad_tile<float, false>(a, w, dma, variant, s);
}

// Phase 2: dw (+)= sum over slabs, fixed order.  `variant` must be the one given to the partial launch (wgrad_path then answers the same).
extern "C" int stp_conv2d_wgrad_reduce(const stp_wgrad_params* p, const void* workspace, int32_t variant, void* stream) {
  if (!p || !p->dw || !workspace) return STP_E_BADARG;
  if (wgrad_path(p, variant) == WG_PATH_ROW) {
    if (!wgrad_row_eligible(p)) return STP_E_BADARG;
    return wgrad_row_reduce(p, workspace, (hipStream_t)stream);
  }
  const WgradPlan w = variant == 0 ? plan_wgrad(p) : plan_wgrad_gemm(p);
  const int64_t count = (int64_t)p->Cout * p->KH * p->KW * (p->C0 + p->C1);
  if ((w.splits >= 64 && count <= (1 << 16)) || (w.splits >= 32 && count <= (1 << 19)))
    hipLaunchKernelGGL(wgrad_reduce_wide_kernel, dim3(ceil_div(count, 64)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)workspace, p->dw, count, w.splits, p->accumulate);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(ceil_div(count, 1024)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace,
                       p->dw, count, w.splits, p->accumulate);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" size_t stp_wgrad_reduce_desc_bytes() { return sizeof(WgReduceDesc); }

// Fills descriptor `index` of a host table for the layer `p` whose partial launch (stp_conv2d_wgrad_partial, variant 0) wrote `workspace`.
// Returns the element count of the layer (> 0), or 0 when its slabs are not the plain [splits][Cout * KH * KW * C] form (row-of-taps
// kernels: fragment-major slabs) - such a layer keeps its own stp_conv2d_wgrad_reduce launch.
extern "C" int64_t stp_wgrad_reduce_desc_fill(void* host_table, int32_t index, const stp_wgrad_params* p, const void* workspace) {
  if (!host_table || index < 0 || !p || !p->dw || !workspace) return 0;
  if (wgrad_path(p, 0) == WG_PATH_ROW) return 0;
  const WgradPlan w = plan_wgrad(p);
  const int64_t count = (int64_t)p->Cout * p->KH * p->KW * (p->C0 + p->C1);
  if (w.splits < 1 || count <= 0 || (count & 3)) return 0;
  WgReduceDesc& d = reinterpret_cast<WgReduceDesc*>(host_table)[index];
  d.slabs = (const float*)workspace; d.dw = p->dw; d.count = count; d.splits = w.splits; d.accumulate = p->accumulate;
  return count;
}

extern "C" int stp_wgrad_reduce_batched(const void* table_dev, int32_t n, int64_t max_count, void* stream) {
  if (!table_dev || n <= 0 || max_count <= 0) return STP_E_BADARG;
  hipLaunchKernelGGL(wgrad_reduce_batched_kernel, dim3(ceil_div(max_count, 64), n), dim3(256), 0, (hipStream_t)stream, (const WgReduceDesc*)table_dev);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_conv2d_wgrad(const stp_wgrad_params* p, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = stp_conv2d_wgrad_partial(p, workspace, workspace_bytes, 0, stream);
  if (rc != STP_OK) return rc;
  return stp_conv2d_wgrad_reduce(p, workspace, 0, stream);
}
