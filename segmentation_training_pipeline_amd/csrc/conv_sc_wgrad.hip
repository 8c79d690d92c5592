// Small-channel family (conv_sc.h): the weight gradient, conv_sc_wgrad_* / stp_wgrad_sc_* (its lean form is in conv_sc_lean.hip).
#include "conv_sc.h"

// =================================================================================================
// Small-channel weight gradient:  dW[co][tap*CIN + ci] = sum_pixels dY[p][co] * X[p + tap][ci]
// Persistent workgroups walk 8x32 tiles; per tile the X halo tile and the dY tile are staged in LDS.
// The reduction index (pixels) is the slow dimension of both tiles, so bf16 fragments come from the
// transpose read ds_read_b64_tr_b16 ([4 pixels][16 channels] per 16-lane group); fp32 uses one element
// per lane.  A 32-pixel MFMA chunk is one tile row.  The 9 taps are split over the 4 waves (wave w owns
// taps w, w+4, w+8), so no cross-wave reduction is needed and accumulators stay in registers across
// tiles.  Each workgroup writes one fp32 slab; the generic fixed-order reduce kernel sums them.
// =================================================================================================
typedef short s16x4_t __attribute__((ext_vector_type(4)));


// STREAMING form of conv_sc_wgrad_kernel below (the one stp_wgrad_sc_partial launches; the register-staged form stays for A/B runs,
// STP_SC_STREAM=0): the X halo tile and the dY tile of the NEXT tile are written into the other half of a double buffer by LDS-DMA
// (out-of-image pixels = out-of-range offset = zeros) while the current tile is multiplied; the fused producer BatchNormalization
// normalises the staged halo vectors in LDS (same fma / activation / rounding).  Same MFMA order: bit-identical slabs.
template <typename T, int CIN, int COUT>
__global__ __launch_bounds__(256) void conv_sc_wgrad_stream_kernel(const ScWgArgs a) {
  constexpr int SZ = (int)sizeof(T);
  constexpr int VEC = Elem<T>::VEC;
  constexpr int TMo = (COUT + 15) / 16, TNi = CIN / 16;
  constexpr int PIXB = CIN * SZ, DYB = COUT * SZ;
  constexpr int HALO_BYTES = SC_HH * SC_HW * PIXB;
  static_assert(CIN % 16 == 0 && COUT % VEC == 0, "channel granularity");

  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][halo tile | dY tile], each padded to whole 1 KB wave pieces
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int sh = a.up ? 1 : 0;

  static_assert(256 % (CIN / VEC) == 0, "a thread stages the same channel vector in every pass");
  const bool pbn = a.pbn.mean != nullptr;
  ScStageBn<T> sbn;
  if (pbn) sbn.load(a.pbn, (tid % (CIN / VEC)) * VEC);

  f32x4 acc[3][TMo][TNi];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int i = 0; i < TMo; ++i)
#pragma unroll
      for (int j = 0; j < TNi; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // ---- staging: LDS-DMA into a double buffer; the tile of the NEXT iteration streams in while this one is multiplied --------
  const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((void*)a.src, 0, a.src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.dy_bytes, 0x00020000);
  constexpr int VPPX = CIN / VEC, VPPD = COUT / VEC;
  constexpr int NVX = SC_HH * SC_HW * VPPX, NPX = (NVX + 255) / 256;      // halo vectors / passes
  constexpr int NVD = SC_TH * SC_TW * VPPD, NPD = (NVD + 255) / 256;      // dY vectors / passes
  constexpr int XBUF = NPX * 4096, DBUF = NPD * 4096, BUF = XBUF + DBUF;  // whole 1 KB wave pieces
  int hyx[NPX], pyx[NPD];
#pragma unroll
  for (int p = 0; p < NPX; ++p) {
    const int v = p * 256 + tid, pix = v / VPPX;
    const int hy = pix / SC_HW, hx = pix - hy * SC_HW;
    hyx[p] = v < NVX ? (hy << 16 | hx) : -1;
  }
#pragma unroll
  for (int p = 0; p < NPD; ++p) {
    const int v = p * 256 + tid, pix = v / VPPD;
    pyx[p] = v < NVD ? ((pix / SC_TW) << 16 | (pix % SC_TW)) : -1;
  }
  const uint32_t cvx = (uint32_t)(tid % VPPX) * 16u, cvd = (uint32_t)(tid % VPPD) * 16u;
  auto decode = [&](int tile, int& n, int& y0, int& x0) {
    int b = tile;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y;
    n = b / a.tiles_y;
    y0 = ty * SC_TH; x0 = tx * SC_TW;
  };
  auto issue_tile = [&](int tile, int bsel) -> uint32_t {
    int n, y0, x0;
    decode(tile, n, y0, x0);
    uint32_t inside = 0;
    char* xb = smem + bsel * BUF;
#pragma unroll
    for (int p = 0; p < NPX; ++p) {
      const int gy = y0 - 1 + (hyx[p] >> 16), gx = x0 - 1 + (hyx[p] & 0xffff);
      const bool ok = hyx[p] >= 0 && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
      const uint32_t off = ok ? (uint32_t)((n * a.Hs + (gy >> sh)) * a.Ws + (gx >> sh)) * (uint32_t)PIXB + cvx : 0x80000000u;
      inside |= ok ? (1u << p) : 0u;
      if (p * 256 + wave * 64 < NVX)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (__attribute__((address_space(3))) void*)(xb + p * 4096 + wave * 1024), 16, off, 0, 0, 0);
    }
#pragma unroll
    for (int p = 0; p < NPD; ++p) {
      const int gy = y0 + (pyx[p] >> 16), gx = x0 + (pyx[p] & 0xffff);
      const bool ok = pyx[p] >= 0 && gy < a.H && gx < a.W;
      const uint32_t off = ok ? (uint32_t)((n * a.H + gy) * a.W + gx) * (uint32_t)DYB + cvd : 0x80000000u;
      if (p * 256 + wave * 64 < NVD)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsd, (__attribute__((address_space(3))) void*)(xb + XBUF + p * 4096 + wave * 1024), 16, off, 0, 0, 0);
    }
    return inside;
  };

  int cur = 0;
  uint32_t inside_cur = (int)blockIdx.x < a.ntiles ? issue_tile((int)blockIdx.x, 0) : 0u;
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    char* halo = smem + cur * BUF;
    char* dyt = halo + XBUF;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // own pieces of this tile have landed
    if (pbn) {
#pragma unroll
      for (int p = 0; p < NPX; ++p)
        if (inside_cur & (1u << p)) {                      // padding applies to the NORMALISED tensor
          u32x4* vp = reinterpret_cast<u32x4*>(halo + (p * 256 + tid) * 16);
          *vp = sbn.apply(*vp, a.pbn.relu);
        }
    }
    lds_barrier();                                          // tile visible; every wave has left the previous tile's buffer
    if (tile + (int)gridDim.x < a.ntiles) inside_cur = issue_tile(tile + (int)gridDim.x, cur ^ 1);
    cur ^= 1;

#pragma unroll 1
    for (int row = 0; row < SC_TH; ++row) {  // one 32-pixel chunk = one tile row
      if constexpr (sizeof(T) == 2) {
        // lane group g owns pixels x = 4g..4g+3 (lo) and 16+4g..16+4g+3 (hi); lane i of a group addresses pixel (i>>2), quad (i&3)
        const int xl = lg * 4 + (lr >> 2), qb = (lr & 3) * 8;
        u32x4 fa[TMo];
#pragma unroll
        for (int i = 0; i < TMo; ++i) {
          const char* p = dyt + ((row * SC_TW + xl) * COUT + i * 16) * SZ + qb;
          const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
          const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p + 16 * DYB));
          const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          fa[i] = u32x4{l2.x, l2.y, h2.x, h2.y};
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int tap = wave + 4 * t;
          if (tap < 9) {
            const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
            for (int j = 0; j < TNi; ++j) {
              const char* p = halo + (((row + kh) * SC_HW + xl + kw) * CIN + j * 16) * SZ + qb;
              const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
              const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p + 16 * PIXB));
              const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
              const u32x4 fb = u32x4{l2.x, l2.y, h2.x, h2.y};
#pragma unroll
              for (int i = 0; i < TMo; ++i)
                acc[t][i][j] = mfma16_16x16x32(fa[i], fb, acc[t][i][j]);
            }
          }
        }
      } else {
        // fp32: 8 k-steps of 4 pixels; lane group g owns pixel 4s + g
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int x = s * 4 + lg;
          float fa[TMo];
#pragma unroll
          for (int i = 0; i < TMo; ++i) fa[i] = *reinterpret_cast<const float*>(dyt + ((row * SC_TW + x) * COUT + i * 16 + lr) * SZ);
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            const int tap = wave + 4 * t;
            if (tap < 9) {
              const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
              for (int j = 0; j < TNi; ++j) {
                const float fb = *reinterpret_cast<const float*>(halo + (((row + kh) * SC_HW + x + kw) * CIN + j * 16 + lr) * SZ);
#pragma unroll
                for (int i = 0; i < TMo; ++i) acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb, acc[t][i][j], 0, 0, 0);
              }
            }
          }
        }
      }
    }
  }

  // ---- slab: C layout row (co) = lg*4 + r, col (ci) = lr ------------------------------------------
  float* out = a.slabs + (size_t)blockIdx.x * a.Cout * (9 * a.ctot);
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int tap = wave + 4 * t;
    if (tap >= 9) continue;
#pragma unroll
    for (int i = 0; i < TMo; ++i)
#pragma unroll
      for (int j = 0; j < TNi; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = i * 16 + lg * 4 + r;
          if (co < a.Cout) out[(size_t)co * (9 * a.ctot) + tap * a.ctot + a.coff + j * 16 + lr] = acc[t][i][j][r];
        }
  }
}


template <typename T, int CIN, int COUT>
__global__ __launch_bounds__(256) void conv_sc_wgrad_kernel(const ScWgArgs a) {
  constexpr int SZ = (int)sizeof(T);
  constexpr int VEC = Elem<T>::VEC;
  constexpr int TMo = (COUT + 15) / 16, TNi = CIN / 16;
  constexpr int PIXB = CIN * SZ, DYB = COUT * SZ;
  constexpr int HALO_BYTES = SC_HH * SC_HW * PIXB;
  static_assert(CIN % 16 == 0 && COUT % VEC == 0, "channel granularity");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* halo = smem;
  char* dyt = smem + HALO_BYTES;  // [SC_TH][SC_TW][COUT]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int sh = a.up ? 1 : 0;

  static_assert(256 % (CIN / VEC) == 0, "a thread stages the same channel vector in every pass");
  const bool pbn = a.pbn.mean != nullptr;
  ScStageBn<T> sbn;
  if (pbn) sbn.load(a.pbn, (tid % (CIN / VEC)) * VEC);

  f32x4 acc[3][TMo][TNi];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int i = 0; i < TMo; ++i)
#pragma unroll
      for (int j = 0; j < TNi; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    int b = tile;
    const int tx = b % a.tiles_x; b /= a.tiles_x;
    const int ty = b % a.tiles_y;
    const int n = b / a.tiles_y;
    const int y0 = ty * SC_TH, x0 = tx * SC_TW;
    __syncthreads();  // previous tile fully consumed
    const char* img = a.src + (size_t)n * a.Hs * a.Ws * PIXB;
    for (int v = tid; v < SC_HH * SC_HW * (CIN / VEC); v += 256) {
      const int pix = v / (CIN / VEC), cv = v - pix * (CIN / VEC);
      const int hy = pix / SC_HW, hx = pix - hy * SC_HW;
      const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
      u32x4 val = {0u, 0u, 0u, 0u};
      if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) {
        val = *reinterpret_cast<const u32x4*>(img + ((size_t)(gy >> sh) * a.Ws + (gx >> sh)) * PIXB + cv * 16);
        if (pbn) val = sbn.apply(val, a.pbn.relu);
      }
      *reinterpret_cast<u32x4*>(halo + v * 16) = val;
    }
    const char* dimg = a.dy + (size_t)n * a.H * a.W * DYB;
    for (int v = tid; v < SC_TH * SC_TW * (COUT / VEC); v += 256) {
      const int pix = v / (COUT / VEC), cv = v - pix * (COUT / VEC);
      const int py = pix / SC_TW, px = pix - py * SC_TW;
      const int gy = y0 + py, gx = x0 + px;
      u32x4 val = {0u, 0u, 0u, 0u};
      if (gy < a.H && gx < a.W) val = *reinterpret_cast<const u32x4*>(dimg + ((size_t)gy * a.W + gx) * DYB + cv * 16);
      *reinterpret_cast<u32x4*>(dyt + v * 16) = val;
    }
    __syncthreads();

#pragma unroll 1
    for (int row = 0; row < SC_TH; ++row) {  // one 32-pixel chunk = one tile row
      if constexpr (sizeof(T) == 2) {
        // lane group g owns pixels x = 4g..4g+3 (lo) and 16+4g..16+4g+3 (hi); lane i of a group addresses pixel (i>>2), quad (i&3)
        const int xl = lg * 4 + (lr >> 2), qb = (lr & 3) * 8;
        u32x4 fa[TMo];
#pragma unroll
        for (int i = 0; i < TMo; ++i) {
          const char* p = dyt + ((row * SC_TW + xl) * COUT + i * 16) * SZ + qb;
          const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
          const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p + 16 * DYB));
          const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          fa[i] = u32x4{l2.x, l2.y, h2.x, h2.y};
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const int tap = wave + 4 * t;
          if (tap < 9) {
            const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
            for (int j = 0; j < TNi; ++j) {
              const char* p = halo + (((row + kh) * SC_HW + xl + kw) * CIN + j * 16) * SZ + qb;
              const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
              const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p + 16 * PIXB));
              const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
              const u32x4 fb = u32x4{l2.x, l2.y, h2.x, h2.y};
#pragma unroll
              for (int i = 0; i < TMo; ++i)
                acc[t][i][j] = mfma16_16x16x32(fa[i], fb, acc[t][i][j]);
            }
          }
        }
      } else {
        // fp32: 8 k-steps of 4 pixels; lane group g owns pixel 4s + g
#pragma unroll
        for (int s = 0; s < 8; ++s) {
          const int x = s * 4 + lg;
          float fa[TMo];
#pragma unroll
          for (int i = 0; i < TMo; ++i) fa[i] = *reinterpret_cast<const float*>(dyt + ((row * SC_TW + x) * COUT + i * 16 + lr) * SZ);
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            const int tap = wave + 4 * t;
            if (tap < 9) {
              const int kh = tap / 3, kw = tap - kh * 3;
#pragma unroll
              for (int j = 0; j < TNi; ++j) {
                const float fb = *reinterpret_cast<const float*>(halo + (((row + kh) * SC_HW + x + kw) * CIN + j * 16 + lr) * SZ);
#pragma unroll
                for (int i = 0; i < TMo; ++i) acc[t][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb, acc[t][i][j], 0, 0, 0);
              }
            }
          }
        }
      }
    }
  }

  // ---- slab: C layout row (co) = lg*4 + r, col (ci) = lr ------------------------------------------
  float* out = a.slabs + (size_t)blockIdx.x * a.Cout * (9 * a.ctot);
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const int tap = wave + 4 * t;
    if (tap >= 9) continue;
#pragma unroll
    for (int i = 0; i < TMo; ++i)
#pragma unroll
      for (int j = 0; j < TNi; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = i * 16 + lg * 4 + r;
          if (co < a.Cout) out[(size_t)co * (9 * a.ctot) + tap * a.ctot + a.coff + j * 16 + lr] = acc[t][i][j][r];
        }
  }
}

#define SC_WG_MAX_BLOCKS 1024

// the stem's weight gradient (7x7 / stride 2, 4 padded input channels -> 64) through conv_stem_wgrad_lean_kernel (conv_sc_lean.hip)
static bool wgrad_stem_shape(const stp_wgrad_params* p) {
  return p->dtype == STP_H16 && p->C0 == 4 && p->C1 == 0 && p->KH == 7 && p->KW == 8 && p->stride == 2 && p->pad == 3 && p->Cout == 64 &&
         p->src0_mode == STP_SRC_DIRECT && p->Hs0 == p->Hv && p->Ws0 == p->Wv && p->Ho == (p->Hv - 1) / 2 + 1 && p->Wo == (p->Wv - 1) / 2 + 1 &&
         !p->src_bn_mean && stem_wg_lean_serves(p->N, p->Hv, p->Wv, p->Ho, p->Wo);
}

extern "C" int stp_wgrad_sc_eligible(const stp_wgrad_params* p) {
  if (!p || !stp_dtype_ok(p->dtype)) return 0;
  if (wgrad_stem_shape(p)) return 1;
  const int vec = p->dtype == STP_H16 ? 8 : 4;
  const bool c0ok = p->C0 == 16 || p->C0 == 32 || (p->C0 == 64 && vec == 8);
  const bool c1ok = p->C1 == 0 || p->C1 == 16 || p->C1 == 32 || (p->C1 == 64 && vec == 8);   // (shape-only: no pointers here)
  return p->KH == 3 && p->KW == 3 && p->stride == 1 && p->pad == 1 && c0ok && c1ok &&
         (p->Cout == 8 || p->Cout == 16 || p->Cout == 32 || (p->Cout == 4 && vec == 4)) && (p->Cout % vec) == 0 &&
         p->Ho == p->Hv && p->Wo == p->Wv &&
         (p->src0_mode == STP_SRC_DIRECT || (p->src0_mode == STP_SRC_NEAREST2X && p->Hv == 2 * p->Hs0 && p->Wv == 2 * p->Ws0));
}

// number of slabs (= workgroups) the small-channel weight gradient writes
extern "C" int stp_wgrad_sc_slabs(const stp_wgrad_params* p) {
  if (wgrad_stem_shape(p)) return stem_wg_lean_blocks(p->N, p->Ho, p->Wo);
  const int64_t tiles = (int64_t)p->N * ceil_div(p->Hv, SC_TH) * ceil_div(p->Wv, SC_TW);
  static const int max_blocks = getenv("STP_SC_WG_BLOCKS") ? atoi(getenv("STP_SC_WG_BLOCKS")) : SC_WG_MAX_BLOCKS;
  // one workgroup per slot the double-buffered staging leaves on a CU (round 4: 1024 workgroups of an 80 KB kernel were two rounds of
  // 512, each with its own prologue, slab and share of the reduce kernel's input)
  const int vec = p->dtype == STP_H16 ? 8 : 4, cin = p->C0 > p->C1 ? p->C0 : p->C1;
  const int64_t npx = ((int64_t)SC_HH * SC_HW * (cin / vec) + 255) / 256, npd = ((int64_t)SC_TH * SC_TW * ((p->Cout + vec - 1) / vec) + 255) / 256;
  const int64_t lds = 2 * (npx + npd) * 4096;
  int per_cu = (int)((160 * 1024) / (lds > 0 ? lds : 1));
  per_cu = per_cu < 1 ? 1 : per_cu > 4 ? 4 : per_cu;
  int64_t blocks = (int64_t)stp_cu_count() * per_cu;
  if (blocks > max_blocks) blocks = max_blocks;
  return (int)(tiles < blocks ? tiles : blocks);
}

template <typename T, int CIN, int COUT>
static int launch_sc_wg(const ScWgArgs& a, int blocks, hipStream_t s) {
  if (sc_stream_on() && a.src_bytes && a.dy_bytes) {
    constexpr int VEC = Elem<T>::VEC;
    constexpr int NPX = (SC_HH * SC_HW * (CIN / VEC) + 255) / 256, NPD = (SC_TH * SC_TW * (COUT / VEC) + 255) / 256;
    const size_t lds = (size_t)2 * (NPX + NPD) * 4096;
    return stp_launch_lds(conv_sc_wgrad_stream_kernel<T, CIN, COUT>, dim3(blocks), dim3(256), lds, s, a);
  }
  const size_t lds = (size_t)SC_HH * SC_HW * CIN * sizeof(T) + (size_t)SC_TH * SC_TW * COUT * sizeof(T) + 64;
  hipLaunchKernelGGL((conv_sc_wgrad_kernel<T, CIN, COUT>), dim3(blocks), dim3(256), lds, s, a);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

template <typename T>
static int sc_wg_dispatch(const ScWgArgs& a, int cin, int cout, int blocks, hipStream_t s) {
  {
    const int r = sc_wg_lean_launch(a, cin, cout, Elem<T>::DTYPE, blocks, s);      // the lean kernel (conv_sc_lean.hip) where it serves the configuration
    if (r != 1) return r;
  }
  const int key = cin * 64 + cout;
  if constexpr (sizeof(T) == 2) {
    switch (key) {
      case 16 * 64 + 8: return launch_sc_wg<T, 16, 8>(a, blocks, s);
      case 16 * 64 + 16: return launch_sc_wg<T, 16, 16>(a, blocks, s);
      case 16 * 64 + 32: return launch_sc_wg<T, 16, 32>(a, blocks, s);
      case 32 * 64 + 8: return launch_sc_wg<T, 32, 8>(a, blocks, s);
      case 32 * 64 + 16: return launch_sc_wg<T, 32, 16>(a, blocks, s);
      case 32 * 64 + 32: return launch_sc_wg<T, 32, 32>(a, blocks, s);
      case 64 * 64 + 8: return launch_sc_wg<T, 64, 8>(a, blocks, s);
      case 64 * 64 + 16: return launch_sc_wg<T, 64, 16>(a, blocks, s);
      case 64 * 64 + 32: return launch_sc_wg<T, 64, 32>(a, blocks, s);
      default: return STP_E_BADARG;
    }
  } else {
    switch (key) {
      case 16 * 64 + 4: return launch_sc_wg<T, 16, 4>(a, blocks, s);
      case 16 * 64 + 8: return launch_sc_wg<T, 16, 8>(a, blocks, s);
      case 16 * 64 + 16: return launch_sc_wg<T, 16, 16>(a, blocks, s);
      case 16 * 64 + 32: return launch_sc_wg<T, 16, 32>(a, blocks, s);
      case 32 * 64 + 4: return launch_sc_wg<T, 32, 4>(a, blocks, s);
      case 32 * 64 + 8: return launch_sc_wg<T, 32, 8>(a, blocks, s);
      case 32 * 64 + 16: return launch_sc_wg<T, 32, 16>(a, blocks, s);
      case 32 * 64 + 32: return launch_sc_wg<T, 32, 32>(a, blocks, s);
      default: return STP_E_BADARG;
    }
  }
}

// One launch per source of the concatenated input; both write disjoint column ranges of the same slabs.
extern "C" int stp_wgrad_sc_partial(const stp_wgrad_params* p, void* workspace, void* stream) {
  if (!stp_wgrad_sc_eligible(p) || !p->src0 || !p->dy || !workspace || (p->C1 > 0 && !p->src1)) return STP_E_BADARG;
  if (wgrad_stem_shape(p)) return stem_wg_lean_launch(p->src0, p->dy, (float*)workspace, p->N, p->Hv, p->Wv, p->Ho, p->Wo, (hipStream_t)stream);
  ScWgArgs a;
  a.dy = (const char*)p->dy; a.slabs = (float*)workspace;
  a.N = p->N; a.H = p->Hv; a.W = p->Wv; a.Cout = p->Cout;
  a.tiles_x = ceil_div(a.W, SC_TW); a.tiles_y = ceil_div(a.H, SC_TH); a.ntiles = a.N * a.tiles_x * a.tiles_y;
  a.ctot = p->C0 + p->C1;
  a.pbn.x = nullptr; a.pbn.mean = p->src_bn_mean; a.pbn.rstd = p->src_bn_rstd; a.pbn.gamma = p->src_bn_gamma; a.pbn.beta = p->src_bn_beta;
  a.pbn.relu = p->src_bn_relu;
  if (a.pbn.mean && (!a.pbn.rstd || p->C1 > 0)) return STP_E_BADARG;
  const int blocks = stp_wgrad_sc_slabs(p);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t szb = p->dtype == STP_H16 ? 2 : 4, lim = 0x80000000ull;
  const uint64_t dyb = (uint64_t)p->N * p->Hv * p->Wv * p->Cout * szb, b0 = (uint64_t)p->N * p->Hs0 * p->Ws0 * p->C0 * szb;
  const uint64_t b1 = (uint64_t)p->N * p->Hv * p->Wv * p->C1 * szb;
  a.dy_bytes = dyb < lim ? (uint32_t)dyb : 0u;      // (0 = beyond 32-bit LDS-DMA offsets: the register-staged kernel runs)
  a.src_bytes = b0 < lim ? (uint32_t)b0 : 0u;
  a.src = (const char*)p->src0; a.Hs = p->Hs0; a.Ws = p->Ws0; a.up = p->src0_mode == STP_SRC_NEAREST2X; a.coff = 0;
  int rc = p->dtype == STP_H16 ? sc_wg_dispatch<bf16_t>(a, p->C0, p->Cout, blocks, s) : sc_wg_dispatch<float>(a, p->C0, p->Cout, blocks, s);
  if (rc != STP_OK || p->C1 == 0) return rc;
  a.pbn.mean = nullptr;
  a.src = (const char*)p->src1; a.Hs = p->Hv; a.Ws = p->Wv; a.up = 0; a.coff = p->C0;
  a.src_bytes = b1 < lim ? (uint32_t)b1 : 0u;
  return p->dtype == STP_H16 ? sc_wg_dispatch<bf16_t>(a, p->C1, p->Cout, blocks, s) : sc_wg_dispatch<float>(a, p->C1, p->Cout, blocks, s);
}
