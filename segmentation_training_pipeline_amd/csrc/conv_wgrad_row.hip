// Weight gradient of the 3x3 / stride 1 layers, row-of-taps tiles (conv_wgrad.hip has the family's head comment, conv_wgrad.h what the
// units share): the body, its single-layer and grouped kernels, their two reduces, eligibility, plan and the four launchers.
#include "conv_wgrad.h"
#include <cstdlib>

// ------------------------------------------------------------------------------------------------
// ROW-OF-TAPS variant (bf16, 3x3 / stride 1 / pad 1, source channel counts multiples of 64, uniform-row feature maps).
// The DMA kernel (conv_wgrad_dma_kernel, conv_wgrad.hip) is bound by the L2 -> LDS path (what-if build: loads only = 80 % of the launch; 64 FLOP per staged
// byte): every k-tile re-stages dY, and the im2col columns of the three taps of a kernel row are three copies of the same
// pixels shifted by one.  Here a workgroup's k-tile is ONE KERNEL ROW of a 64-channel input block - 192 columns
// (kw = 0..2) x (ci 0..63) - and the operand tile of a 64-pixel step is the step's input pixels WITH THEIR HALO: rows x
// (seg + 2) pixels of 128 bytes (seg = min(64, Wo) pixels of `rows` image rows).  The B fragment of tap kw is the same LDS
// block read one pixel row further: 28 KB staged per 2 x 128 x 192 x 64 FLOP = 112 FLOP per byte, 7 LDS-DMA instructions
// per thread per 48 MFMAs (8 per 32 above).  LDS rows keep the 32-byte-unit XOR swizzle of tile_addr<> (a transpose read
// touches 8 consecutive pixel rows from any start: conflict-free for every kw).
//   tile: BM output channels x 192 columns of kernel row kh, input-channel block cib   (tile_n = kh * (C0 / 64) + cib)
//   dW column of (kw, ci): (kh * 3 + kw) * Ctot + cib * 64 + ci.  Two concatenated sources (each a multiple of 64 channels, the first optionally
//   nearest-2x upsampled: the decoder's UpSampling2D + Concatenate) are handled per 64-channel block: a block lies in one source.
// PBN (fused producer BatchNormalization of src0) is a compile-time parameter of the body: 20 VGPRs the plain launches do not carry.
// which instances run on v_mfma_f32_32x32x16 (STP_ROW_M32=0: a what-if build on the 16 x 16 x 32 form everywhere)
#ifndef STP_ROW_M32
#define STP_ROW_M32 0
#endif
template <int BM, int WM, int WN> struct RowM32 { static constexpr bool value = STP_ROW_M32 && BM == 128 && WM == 2 && WN == 2; };

// element e (float4) of a tile's fragment-major slab -> first of its 4 output channels (relative to the tile) and its column (0..191)
template <int BM, int WM, int WN>
__device__ __forceinline__ void row_slab_decode(int e, int& co, int& col) {
  const int lane = e & 63;
  int q = e >> 6;
  if constexpr (RowM32<BM, WM, WN>::value) {
    constexpr int TM = BM / WM / 32, TN = 192 / WN / 32;
    const int qq = q & 3; q >>= 2;
    const int ij = q % (TM * TN), wave = q / (TM * TN);
    const int i = ij / TN, j = ij - i * TN, wm = wave / WN, wn = wave % WN;
    co = wm * (BM / WM) + i * 32 + 8 * qq + 4 * (lane >> 5);
    col = wn * (192 / WN) + j * 32 + (lane & 31);
  } else {
    constexpr int TM = BM / WM / 16, TN = 192 / WN / 16;
    const int ij = q % (TM * TN), wave = q / (TM * TN);
    const int i = ij / TN, j = ij - i * TN, wm = wave / WN, wn = wave % WN;
    co = wm * (BM / WM) + i * 16 + (lane >> 4) * 4;
    col = wn * (192 / WN) + j * 16 + (lane & 15);
  }
}

// (t, step0, step1, out_tile): the tile of the layer (tile_m fastest), the range of 64-pixel steps summed and the fragment-major
// partial slab [wave][i][j][lane] float4 that receives the sums - the single-layer kernel derives them from the block id, the
// grouped kernel (below) from its work list.
template <int BM, int WM, int WN, int STAGES, bool PBN>
__device__ __forceinline__ void conv_wgrad_row_body(const WgradArgs& a, const int t, const int step0, const int step1, f32x4* const out_tile) {
  static_assert(WM * WN == 4, "4 waves");
#if defined(__HIP_DEVICE_COMPILE__)
  typedef bf16_t T;
  constexpr int SZ = 2, PK = 64, BN = 192;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  constexpr int ROWA = BM * SZ, ROWB = 128;                    // LDS row bytes: dY pixel / halo pixel (64 input channels)
  constexpr int VPRA = ROWA / 16, RPA = 256 / VPRA, NVA = PK / RPA;
  constexpr int HROWS = 72, NVB = 3;                           // halo rows: rows x (seg + 2) <= 72; passes of 32 rows, the third has 8
  constexpr int STAGE = PK * ROWA + HROWS * ROWB;
  constexpr int L = NVA + NVB;                                 // LDS-DMA instructions per stage: wave 0 (waves 1-3 skip the third halo pass)
  static_assert(NVA * RPA == PK && (NVA == 1 || RPA % 8 == 0), "A passes");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int lr = lane & 15, lg = lane >> 4;

  const int tile_m = t % a.ntile_m, tile_n = t / a.ntile_m;
  const int ncib = a.Ctot >> 6;
  const int kh = tile_n / ncib, cib = tile_n - kh * ncib;       // cib: 64-channel block of the CONCATENATED input
  const bool first = cib * 64 < a.C0;                            // wave-uniform: which source holds this block
  const int cs = first ? a.C0 : a.C1, cb_src = first ? cib : cib - (a.C0 >> 6);
  const int sh = (first && a.mode == STP_SRC_NEAREST2X) ? 1 : 0;  // UpSampling2D(2) folded into the gather: source pixel = (h >> 1, w >> 1)
  const int Hs = first ? a.Hs0 : a.Hv, Ws = first ? a.Ws0 : a.Wv;
  const int cout0 = tile_m * BM;

  const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.bytesdy, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)(first ? a.src0 : a.src1), 0, first ? a.bytes0 : a.bytes1, 0x00020000);

  // geometry of a step: `rows` image rows of `seg` pixels (wave-uniform)
  const int seg = a.Wo >= PK ? PK : a.Wo, rows = PK / seg, hw = seg + 2;

  // ---- LDS-DMA constants.  A (dY): as in the DMA kernel.  B: halo row h = pass * 32 + tid / 8, physical slot tid & 7 -------
  const int rowA0 = tid / VPRA;
  const int colA = (tile_addr<ROWA>(rowA0, (tid % VPRA) * 16) - rowA0 * ROWA) / SZ;
  const bool coA_ok = (cout0 + colA) < a.Cout;
  uint32_t rowa[NVA];
#pragma unroll
  for (int i = 0; i < NVA; ++i) rowa[i] = ((uint32_t)(rowA0 + i * RPA) * (uint32_t)a.Cout + (uint32_t)(cout0 + colA)) * SZ;
  const int hb0 = tid >> 3;
  const uint32_t colB = (uint32_t)(tile_addr<ROWB>(hb0, (tid & 7) * 16) - hb0 * ROWB);   // logical byte column held by this slot
  int hr[NVB], hx[NVB];          // image row / column of the halo pixel relative to the step's first pixel (-1 = unused row)
#pragma unroll
  for (int i = 0; i < NVB; ++i) {
    const int h = hb0 + i * 32;
    const int r = h / hw;
    hr[i] = r < rows ? r + kh - 1 : -0x4000;
    hx[i] = h - r * hw - 1;
  }
  const uint32_t pixb = (uint32_t)cs * SZ, imgb = (uint32_t)Hs * (uint32_t)Ws * pixb, cbyte = (uint32_t)cb_src * 128u + colB;
  // fused PRODUCER BatchNormalization (+activation): the thread that DMA'd a 16-byte vector of the halo tile normalises it in LDS
  // once it has landed (own data: its vmcnt orders the read-modify-write, the step's barrier publishes it) - same fma, activation
  // and bf16 rounding as stp_bn_apply, so the operand equals the tensor that launch would have stored; padding stays zero
  const bool pbn = PBN && a.pbn.mean != nullptr;
  f32x2 psc[4], psh[4];
  if (pbn) {
    const int c0 = cb_src * 64 + (int)(colB >> 1);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float r = a.pbn.rstd[c0 + e], k = a.pbn.gamma ? r * a.pbn.gamma[c0 + e] : r;
      psc[e >> 1][e & 1] = k;
      psh[e >> 1][e & 1] = (a.pbn.beta ? a.pbn.beta[c0 + e] : 0.f) - a.pbn.mean[c0 + e] * k;
    }
  }
  auto transform_tile = [&](int step, int buf) {
    char* sb = smem + buf * STAGE + PK * ROWA;
    const int p0 = step * PK;
    const uint32_t n = fdiv((uint32_t)p0, a.divHoWo);
    const uint32_t rem = (uint32_t)p0 - n * (uint32_t)a.HoWo;
    const uint32_t ho0 = fdiv(rem, a.divWo);
    const uint32_t wo0 = rem - ho0 * (uint32_t)a.Wo;
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      if (i * 32 + wave * 8 >= HROWS) continue;                 // wave-uniform
      const int hv = (int)ho0 + hr[i], wv = (int)wo0 + hx[i];
      if (!((unsigned)hv < (unsigned)a.Hv && (unsigned)wv < (unsigned)a.Wv)) continue;
      u32x4* vp = reinterpret_cast<u32x4*>(sb + (i * 256 + tid) * 16);
      const u32x4 v = *vp;
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        f32x2 t = {h16lo_to_f32(v[e]), h16hi_to_f32(v[e])};
        t = __builtin_elementwise_fma(t, psc[e], psh[e]);
        o[e] = pack_bf16x2(bn_act(t.x, a.pbn.relu), bn_act(t.y, a.pbn.relu));
      }
      *vp = o;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  };

  auto issue_tile = [&](int step, int buf) {
    const int p0 = step * PK;
    char* sa = smem + buf * STAGE;
    char* sb = sa + PK * ROWA;
    const uint32_t n = fdiv((uint32_t)p0, a.divHoWo);
    const uint32_t rem = (uint32_t)p0 - n * (uint32_t)a.HoWo;
    const uint32_t ho0 = fdiv(rem, a.divWo);
    const uint32_t wo0 = rem - ho0 * (uint32_t)a.Wo;
    const uint32_t abase = (uint32_t)p0 * (uint32_t)a.Cout * SZ;
    const uint32_t nb = n * imgb + cbyte;
#pragma unroll
    for (int i = 0; i < NVA; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsd, (__attribute__((address_space(3))) void*)(sa + (i * 256 + wave * 64) * 16), 16,
                                               coA_ok ? abase + rowa[i] : STP_OOB, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NVB; ++i) {
      const int hv = (int)ho0 + hr[i], wv = (int)wo0 + hx[i];
      const bool ok = (unsigned)hv < (unsigned)a.Hv && (unsigned)wv < (unsigned)a.Wv;
      const uint32_t off = nb + ((uint32_t)(hv >> sh) * (uint32_t)Ws + (uint32_t)(wv >> sh)) * pixb;
      if (i * 32 + wave * 8 < HROWS)     // wave-uniform: rows 72.. of the third pass do not exist
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (__attribute__((address_space(3))) void*)(sb + (i * 256 + wave * 64) * 16), 16,
                                                 ok ? off : STP_OOB, 0, 0, 0);
    }
  };

  // ---- fragment addresses.  Pixel q of the step = image row q / seg, column q % seg -> halo row (q / seg) * hw + q % seg + kw.
  // A 16-lane group reads 4 consecutive pixels (seg >= 16: they share an image row); lane: pixel (lr >> 2), quad (lr & 3).
  const int qb = (lr & 3) * 8;
  int prowA[4], hrowB[4];      // [chunk * 2 + half]: dY row / halo row (kw = 0) of this lane's pixel
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = e * 16 + lg * 4 + (lr >> 2);
    prowA[e] = q;
    const int r = q / seg;
    hrowB[e] = r * hw + (q - r * seg);
  }
  int kwB[TN], cbB[TN];        // tap and byte column (64-channel block) of this wave's column blocks
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int col = wn * (BN / WN) + j * 16;
    kwB[j] = col >> 6;
    cbB[j] = (col & 63) * SZ + qb;
  }
  const int ca = (wm * (BM / WM)) * SZ + qb;

  // M32 (128-channel class, 2 x 2 waves of 64 x 96): v_mfma_f32_32x32x16 - half the MFMA instructions per step for the same
  // transpose reads (the operand bytes of a wave tile do not depend on the MFMA shape), which frees issue slots for the reads.
  // Operand layout of the 32 x 32 x 16 form: lane group g = lane >> 4 holds rows / columns 16 (g & 1) .. +15 and k = 8 (g >> 1) .. +7;
  // a k-step = 16 pixels: pixel 16 kk + 8 (g >> 1) + {0..3} from the first transpose read, + {4..7} from the second - the same map
  // for both operands, which is all the contraction needs.
  constexpr bool M32 = RowM32<BM, WM, WN>::value;
  constexpr int TM32 = M32 ? BM / WM / 32 : 1, TN32 = M32 ? BN / WN / 32 : 1;
  int prowA32[8], hrowB32[8], kwB32[TN32], cbB32[TN32];
  int ca32 = 0;
  if constexpr (M32) {
    const int hh = lg & 1, kh2 = lg >> 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {      // e = kk * 2 + half
      const int q = (e >> 1) * 16 + kh2 * 8 + (e & 1) * 4 + (lr >> 2);
      prowA32[e] = q;
      const int r = q / seg;
      hrowB32[e] = r * hw + (q - r * seg);
    }
#pragma unroll
    for (int j = 0; j < TN32; ++j) {
      const int col = wn * (BN / WN) + j * 32 + hh * 16;
      kwB32[j] = col >> 6;
      cbB32[j] = (col & 63) * SZ + qb;
    }
    ca32 = (wm * (BM / WM) + hh * 16) * SZ + qb;
  }

  f32x4 acc[M32 ? 1 : TM][M32 ? 1 : TN];
  f32x16 acc32[TM32][TN32];
  if constexpr (M32) {
#pragma unroll
    for (int i = 0; i < TM32; ++i)
#pragma unroll
      for (int j = 0; j < TN32; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc32[i][j][e] = 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  auto compute = [&](const char* sa) {
    const char* sb = sa + PK * ROWA;
    if constexpr (M32) {
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        u32x4 fa[TM32], fb[TN32];
#pragma unroll
        for (int i = 0; i < TM32; ++i) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sa + tile_addr<ROWA>(prowA32[2 * kk], ca32 + i * 64)));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sa + tile_addr<ROWA>(prowA32[2 * kk + 1], ca32 + i * 64)));
          const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          fa[i] = u32x4{l2.x, l2.y, h2.x, h2.y};
        }
#pragma unroll
        for (int j = 0; j < TN32; ++j) {
          const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sb + tile_addr<ROWB>(hrowB32[2 * kk] + kwB32[j], cbB32[j])));
          const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sb + tile_addr<ROWB>(hrowB32[2 * kk + 1] + kwB32[j], cbB32[j])));
          const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
          fb[j] = u32x4{l2.x, l2.y, h2.x, h2.y};
        }
#pragma unroll
        for (int i = 0; i < TM32; ++i)
#pragma unroll
          for (int j = 0; j < TN32; ++j)
            acc32[i][j] = mfma16_32x32x16(fa[i], fb[j], acc32[i][j]);
      }
      return;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      u32x4 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sa + tile_addr<ROWA>(prowA[2 * c], ca + i * 32)));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sa + tile_addr<ROWA>(prowA[2 * c + 1], ca + i * 32)));
        const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
        fa[i] = u32x4{l2.x, l2.y, h2.x, h2.y};
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sb + tile_addr<ROWB>(hrowB[2 * c] + kwB[j], cbB[j])));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(sb + tile_addr<ROWB>(hrowB[2 * c + 1] + kwB[j], cbB[j])));
        const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
        fb[j] = u32x4{l2.x, l2.y, h2.x, h2.y};
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = mfma16_16x16x32(fa[i], fb[j], acc[i][j]);
    }
  };

  // STAGES-deep ring, one barrier per step: tile st+STAGES-1 is issued after the barrier of step st (every wave has left
  // compute(st-1), the last reader of that slot); the wait leaves the STAGES-2 younger tiles in flight
  const int nst = step1 - step0;
#pragma unroll
  for (int q = 0; q < STAGES - 1; ++q)
    if (q < nst) issue_tile(step0 + q, q);
  int buf = 0, nbuf = STAGES - 1;
  for (int st = 0; st < nst; ++st) {
    const int ahead = nst - 1 - st;      // tiles after this one
    if (STAGES >= 3 && ahead >= STAGES - 2) {
      if (wave == 0) wait_vmcnt<(STAGES - 2) * L>(); else wait_vmcnt<(STAGES - 2) * (L - 1)>();
    } else {
      wait_vmcnt<0>();
    }
    if (pbn) transform_tile(step0 + st, buf);
    __builtin_amdgcn_s_barrier();
#if !defined(STP_EXP) || STP_EXP != 2
    if (st + STAGES - 1 < nst) issue_tile(step0 + st + STAGES - 1, nbuf);
#endif
#if !defined(STP_EXP) || STP_EXP != 1
    compute(smem + buf * STAGE);
#endif
    buf = (buf + 1 == STAGES) ? 0 : buf + 1;
    nbuf = (nbuf + 1 == STAGES) ? 0 : nbuf + 1;
  }

  // ---- slab, FRAGMENT-MAJOR: [split][tile][wave][i][j][lane] float4 (the lane's 4 output channels of one column) - every store is
  // a 16-byte lane-contiguous vector (1 KB per wave instruction) instead of 4-byte stores K floats apart (measured: the scattered
  // slab write was a third of the launch); wgrad_reduce_row_kernel sums the splits in this order and scatters into dW once
  f32x4* out = out_tile + (size_t)wave * (TM * TN * 64) + lane;
  if constexpr (M32) {      // [wave][i][j][q][lane]: the lane's rows 8 q + 4 (lane >> 5) + {0..3} of column lane & 31 (row_slab_decode)
#pragma unroll
    for (int i = 0; i < TM32; ++i)
#pragma unroll
      for (int j = 0; j < TN32; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          out[((i * TN32 + j) * 4 + q) * 64] = f32x4{acc32[i][j][4 * q], acc32[i][j][4 * q + 1], acc32[i][j][4 * q + 2], acc32[i][j][4 * q + 3]};
  } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) out[(i * TN + j) * 64] = acc[i][j];
  }
#endif
}

// single layer: block = (split, tile), the tiles of one split (same pixels) next to each other
template <int BM, int WM, int WN, int STAGES, bool PBN>
__device__ __forceinline__ void conv_wgrad_row_single(const WgradArgs& a) {
  const int tiles = a.ntile_m * a.ntile_n;
  const int bid = a.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
  const int split = bid / tiles;
  const int t = bid - split * tiles;
  const int step0 = split * a.steps_per_split;
  const int step1 = min(step0 + a.steps_per_split, a.nsteps);
  conv_wgrad_row_body<BM, WM, WN, STAGES, PBN>(a, t, step0, step1, reinterpret_cast<f32x4*>(a.out) + (size_t)(split * tiles + t) * (BM * 192 / 4));
}
template <int BM, int WM, int WN, int STAGES>
__global__ __launch_bounds__(256) void conv_wgrad_row_kernel(const WgradArgs a) { conv_wgrad_row_single<BM, WM, WN, STAGES, false>(a); }
template <int BM, int WM, int WN, int STAGES>
__global__ __launch_bounds__(256) void conv_wgrad_row_pbn_kernel(const WgradArgs a) { conv_wgrad_row_single<BM, WM, WN, STAGES, true>(a); }


// PBN: the instance for groups in which some layer reads the tensor BEFORE a BatchNormalization(+activation) and normalises its halo
// tile in LDS (per layer: WgradArgs::pbn.mean != nullptr) - the stp_bn_apply launch of that BatchNormalization is gone (graph.py)
template <int BM, int WM, int WN, int STAGES, bool PBN>
__device__ __forceinline__ void conv_wgrad_row_group_body(const char* __restrict__ table, f32x4* __restrict__ slabs) {
  const WgGroupHeader* const hd = reinterpret_cast<const WgGroupHeader*>(table);
  const WgLayer* const layers = reinterpret_cast<const WgLayer*>(table + hd->off_layers);
  const WgSeg* const segs = reinterpret_cast<const WgSeg*>(table + hd->off_segs);
  const int* const first = reinterpret_cast<const int*>(table + hd->off_first);
  // consecutive block ids round-robin over the XCDs: give every XCD one contiguous run of the line (the tiles of a layer read
  // the same dY / x pixels at the same time: they meet in one L2)
  // hd->xcd: 0 = identity (line neighbours on different XCDs), 1 = one contiguous run of the line per XCD, G >= 2 = runs of G line
  // neighbours per XCD, the runs dealt round-robin (G workgroups share their operands in one L2, no more: 64 workgroups fetching the
  // same lines at the same time from ONE L2 measured slower for the 512-channel layers)
  int w = blockIdx.x;
  if (hd->xcd == 1) {
    w = xcd_remap(blockIdx.x, gridDim.x);
  } else if (hd->xcd >= 2) {
    const int G = hd->xcd, nmain = (int)gridDim.x / (8 * G) * (8 * G);
    if ((int)blockIdx.x < nmain) {
      const int x = blockIdx.x & 7, j = blockIdx.x >> 3;
      w = ((j / G) * 8 + x) * G + (j % G);
    }
  }
  const int s0 = __builtin_amdgcn_readfirstlane(first[w]), s1 = __builtin_amdgcn_readfirstlane(first[w + 1]);
  for (int s = s0; s < s1; ++s) {
    // The descriptors are read through the CONSTANT address space: invariant scalar loads the compiler may hoist out of the step
    // loop and keep in SGPRs, as it does for kernel arguments.  Through a global pointer every `memory`-clobbering s_waitcnt of the
    // loop forced a reload (s_load + lgkmcnt(0) in every step, which also drains the fragment reads: -17 % on the first build).
    WgSeg sg;
    load_constant(sg, segs + s);
    WgradArgs a;
    load_constant(a, &layers[sg.layer].a);
    if (s != s0) __syncthreads();        // the previous segment's last fragment reads precede this segment's first LDS-DMA
    conv_wgrad_row_body<BM, WM, WN, STAGES, PBN>(a, sg.tile, sg.step0, sg.step1, slabs + (size_t)sg.slot * (BM * 192 / 4));
  }
}
template <int BM, int WM, int WN, int STAGES>
__global__ __launch_bounds__(256) void conv_wgrad_row_group_kernel(const char* __restrict__ table, f32x4* __restrict__ slabs) {
  conv_wgrad_row_group_body<BM, WM, WN, STAGES, false>(table, slabs);
}
template <int BM, int WM, int WN, int STAGES>
__global__ __launch_bounds__(256) void conv_wgrad_row_group_pbn_kernel(const char* __restrict__ table, f32x4* __restrict__ slabs) {
  conv_wgrad_row_group_body<BM, WM, WN, STAGES, true>(table, slabs);
}

// sum of a tile's partial slabs in line order, scattered into dW (the element decode of wgrad_reduce_row_kernel).  SL lanes walk the
// slab list of an element in parallel (fixed assignment, fixed-shape LDS tree: deterministic) - stage-1 tiles have 40+ slabs.
template <int BM, int WM, int WN, int SL>
__global__ __launch_bounds__(256) void wgrad_group_reduce_kernel(const char* __restrict__ table, const f32x4* __restrict__ slabs) {
  constexpr int PER = BM * 192 / 4, EPB = 256 / SL, BPT = PER / EPB;
  static_assert(PER % EPB == 0, "whole blocks per tile");
  __shared__ f32x4 sh[SL][EPB];
  const WgGroupHeader* const hd = reinterpret_cast<const WgGroupHeader*>(table);
  const WgLayer* const layers = reinterpret_cast<const WgLayer*>(table + hd->off_layers);
  const int* const slot_list = reinterpret_cast<const int*>(table + hd->off_slots);
  const WgTile tl = reinterpret_cast<const WgTile*>(table + hd->off_tiles)[blockIdx.x / BPT];
  const int ev = threadIdx.x % EPB, sl = threadIdx.x / EPB;
  const int e = (blockIdx.x % BPT) * EPB + ev;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  {
    // (four slab loads in flight per lane; same order of additions)
    int k = sl;
    for (; k + 3 * SL < tl.nslots; k += 4 * SL) {
      const f32x4 a0 = slabs[(size_t)slot_list[tl.list0 + k] * PER + e], a1 = slabs[(size_t)slot_list[tl.list0 + k + SL] * PER + e];
      const f32x4 a2 = slabs[(size_t)slot_list[tl.list0 + k + 2 * SL] * PER + e], a3 = slabs[(size_t)slot_list[tl.list0 + k + 3 * SL] * PER + e];
      s += a0; s += a1; s += a2; s += a3;
    }
    for (; k < tl.nslots; k += SL) s += slabs[(size_t)slot_list[tl.list0 + k] * PER + e];
  }
  if (SL > 1) {
    sh[sl][ev] = s;
    __syncthreads();
#pragma unroll
    for (int w = SL / 2; w > 0; w >>= 1) {
      if (sl < w) sh[sl][ev] += sh[sl + w][ev];
      __syncthreads();
    }
    s = sh[0][ev];
    if (sl != 0) return;
  }
  const WgLayer& L = layers[tl.layer];
  int col, co;
  row_slab_decode<BM, WM, WN>(e, co, col);
  const int tile_m = tl.t % L.a.ntile_m, tile_n = tl.t / L.a.ntile_m;
  const int ncib = L.a.Ctot >> 6, kh = tile_n / ncib, cib = tile_n - kh * ncib;
  const int kc = (kh * 3 + (col >> 6)) * L.a.Ctot + cib * 64 + (col & 63);
  co += tile_m * BM;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (co + r < L.a.Cout) {
      float* d = L.dw + (size_t)(co + r) * L.a.K + kc;
      *d = L.accumulate ? *d + s[r] : s[r];
    }
}

// Reduction of the row-of-taps kernel's fragment-major slabs: element e = ((tile * 4 + wave) * TM*TN + i*TN + j) * 64 + lane.
// SL lanes walk the splits of an element in parallel (fixed assignment, fixed-shape LDS tree: deterministic), then the 4 floats
// go to dW[co + r][(kh*3 + kw) * C0 + cib*64 + ci].
template <int BM, int WM, int WN, int SL>
__global__ __launch_bounds__(256) void wgrad_reduce_row_kernel(const f32x4* __restrict__ slabs, float* __restrict__ dw, int64_t per_split,
                                                               int splits, int accumulate, int ntile_m, int C0, int Cout, int K) {
  constexpr int EPB = 256 / SL;
  __shared__ f32x4 sh[SL][EPB];
  const int ev = threadIdx.x % EPB, sl = threadIdx.x / EPB;
  const int64_t e = (int64_t)blockIdx.x * EPB + ev;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (e < per_split)
    for (int k = sl; k < splits; k += SL) s += slabs[(size_t)k * per_split + e];
  if (SL > 1) {
    sh[sl][ev] = s;
    __syncthreads();
#pragma unroll
    for (int w = SL / 2; w > 0; w >>= 1) {
      if (sl < w) sh[sl][ev] += sh[sl + w][ev];
      __syncthreads();
    }
    s = sh[0][ev];
  }
  if (sl != 0 || e >= per_split) return;
  constexpr int PERT = BM * 192 / 4;                       // float4 elements per tile
  const int t = (int)(e / PERT);
  int col, co;
  row_slab_decode<BM, WM, WN>((int)(e - (int64_t)t * PERT), co, col);
  const int tile_m = t % ntile_m, tile_n = t / ntile_m;
  const int ncib = C0 >> 6, kh = tile_n / ncib, cib = tile_n - kh * ncib;
  const int kc = (kh * 3 + (col >> 6)) * C0 + cib * 64 + (col & 63);
  co += tile_m * BM;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (co + r < Cout) {
      float* d = dw + (size_t)(co + r) * K + kc;
      *d = accumulate ? *d + s[r] : s[r];
    }
}

// ---- row-of-taps kernel (conv_wgrad_row_kernel): eligibility and plan ------------------------------------------------------
bool wgrad_row_eligible(const stp_wgrad_params* p) {
  if (!p || p->dtype != STP_H16 || p->KH != 3 || p->KW != 3 || p->stride != 1 || p->pad != 1 || (p->C0 & 63) || (p->C1 & 63) ||
      p->Ho != p->Hv || p->Wo != p->Wv || (p->Cout & 7))
    return false;
  if (p->src_bn_mean && (!p->src_bn_rstd || p->C1 != 0 || p->src0_mode != STP_SRC_DIRECT)) return false;
  if (p->src0_mode == STP_SRC_DIRECT ? (p->Hs0 != p->Hv || p->Ws0 != p->Wv)
                                     : (p->src0_mode != STP_SRC_NEAREST2X || p->Hv != 2 * p->Hs0 || p->Wv != 2 * p->Ws0))
    return false;
  const int hw = p->Ho * p->Wo;
  return (p->Wo % 64 == 0) || (p->Wo >= 16 && 64 % p->Wo == 0 && hw % 64 == 0);
}
bool wgrad_row_auto(const stp_wgrad_params* p) {
  static const bool on = !(getenv("STP_WGRAD_ROW") && atoi(getenv("STP_WGRAD_ROW")) == 0);
  return on && p->splits == 0 && wgrad_row_eligible(p);
}
WgradPlan plan_wgrad_row(const stp_wgrad_params* p) {
  WgradPlan w;
  w.bm = p->Cout <= 64 ? 64 : 128; w.bn = 192;
  w.tile = w.bm == 64 ? WG_TILE_ROW64 : WG_TILE_ROW128;
  w.ntile_m = ceil_div(p->Cout, w.bm);
  w.ntile_n = 3 * ((p->C0 + p->C1) / 64);
  const int64_t P = (int64_t)p->N * p->Ho * p->Wo;
  w.nsteps = (int)(P / 64);
  int target = 0;
  if (p->splits <= 0) {
    static const int env = getenv("STP_WGRAD_ROW_BLOCKS") ? atoi(getenv("STP_WGRAD_ROW_BLOCKS")) : 0;
    target = env;
  }
  wgrad_choose_splits(w, p->splits, target);      // co-resident workgroups (LDS: 40 / 56 KB each)
  return w;
}

// ---- launchers: single layer (`a` as wgrad_fill left it), then the group (the header is the validated host copy of the table) -----
int wgrad_row_partial(const stp_wgrad_params* p, WgradArgs& a, hipStream_t s) {
  const WgradPlan w = plan_wgrad_row(p);
  a.ntile_m = w.ntile_m; a.ntile_n = w.ntile_n; a.steps_per_split = w.steps_per_split; a.nsteps = w.nsteps;
  a.xcd = w.ntile_m == 1;
  static const int stages = getenv("STP_WGRAD_ROW_STAGES") ? atoi(getenv("STP_WGRAD_ROW_STAGES")) : 3;
  const size_t lds = (size_t)(stages == 2 ? 2 : 3) * (64 * w.bm * 2 + 72 * 128);    // 25 / 17 KB per stage
  if (stages == 2 && a.pbn.mean) return STP_E_BADARG;       // (the 2-stage what-if build has no fused producer BatchNormalization)
  return row_class<false>(w.bm, [&](auto c) -> int {
    using C = decltype(c);
    if (stages == 2) return launch_wg(conv_wgrad_row_kernel<C::BM, C::WM, C::WN, 2>, a, lds, w.splits, s);
    if (a.pbn.mean) return launch_wg(conv_wgrad_row_pbn_kernel<C::BM, C::WM, C::WN, 3>, a, lds, w.splits, s);   // its own instances
    return launch_wg(conv_wgrad_row_kernel<C::BM, C::WM, C::WN, 3>, a, lds, w.splits, s);
  });
}

int wgrad_row_reduce(const stp_wgrad_params* p, const void* workspace, hipStream_t s) {
  const WgradPlan r = plan_wgrad_row(p);
  const int64_t per_split = (int64_t)r.ntile_m * r.ntile_n * r.bm * 192 / 4;   // float4 elements
  const int K = 9 * (p->C0 + p->C1);
  const int sl = r.splits >= 32 ? 16 : r.splits >= 8 ? 4 : 1;
  const dim3 grid(ceil_div(per_split, 256 / sl));
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, (const f32x4*)workspace, p->dw, per_split, r.splits, p->accumulate, r.ntile_m,
                       p->C0 + p->C1, p->Cout, K);
  };
  const int rc = row_class<false>(r.bm, [&](auto c) -> int {
    using C = decltype(c);
    if (sl == 16) launch(wgrad_reduce_row_kernel<C::BM, C::WM, C::WN, 16>);
    else if (sl == 4) launch(wgrad_reduce_row_kernel<C::BM, C::WM, C::WN, 4>);
    else launch(wgrad_reduce_row_kernel<C::BM, C::WM, C::WN, 1>);
    return STP_OK;
  });
  if (rc != STP_OK) return rc;
  STP_LAUNCH_CHECK();
  return STP_OK;
}

int wgrad_row_group_partial(const WgGroupHeader* hd, const void* dev_table, void* workspace, hipStream_t s) {
  const size_t lds = (size_t)3 * (64 * hd->bm * 2 + 72 * 128);
  return row_class(hd->bm, [&](auto c) -> int {
    using C = decltype(c);
    return stp_launch_lds(hd->pbn ? conv_wgrad_row_group_pbn_kernel<C::BM, C::WM, C::WN, 3> : conv_wgrad_row_group_kernel<C::BM, C::WM, C::WN, 3>,
                          dim3(hd->n_wg), dim3(256), lds, s, (const char*)dev_table, (f32x4*)workspace);
  });
}

int wgrad_row_group_reduce(const WgGroupHeader* hd, const void* dev_table, const void* workspace, hipStream_t s) {
  const int sl = hd->reduce_lanes == 4 ? 4 : 1;
  const dim3 grid(hd->n_tiles * (hd->bm * 192 / 4 / (256 / sl)));
  auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, (const char*)dev_table, (const f32x4*)workspace); };
  const int rc = row_class(hd->bm, [&](auto c) -> int {
    using C = decltype(c);
    if (sl == 4) launch(wgrad_group_reduce_kernel<C::BM, C::WM, C::WN, 4>);
    else launch(wgrad_group_reduce_kernel<C::BM, C::WM, C::WN, 1>);
    return STP_OK;
  });
  if (rc != STP_OK) return rc;
  STP_LAUNCH_CHECK();
  return STP_OK;
}
