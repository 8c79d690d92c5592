// Weight gradient of the 3x3 / stride 1 layers, all-taps tiles of the grouped launch (conv_wgrad.hip has the family's head comment,
// conv_wgrad.h what the units share): the body, the grouped kernel, its reduce and their two launchers.
#include "conv_wgrad.h"

// ------------------------------------------------------------------------------------------------
// ALL-TAPS tile (round 4): BM output channels x 576 columns = the NINE taps of one 64-channel input block.
// The row-of-taps tile (conv_wgrad_row.hip; BM x 192: one kernel row) re-stages dY for each of the three kernel rows and the same input pixels
// three times with a one-row shift: 25 KB through L2 -> LDS per 3.1 MFLOP, and the 24-96 tiles over a pixel range each fetch their
// own copy (profiles/r03final_pmc_traffic.json: 4.85x the algorithmic bytes reach the fabric; the kernel waits on memory 42 % of
// its time).  Here a step stages dY once (64 pixels x BM channels) and ONE halo of the input block - (rows + 2) image rows of
// (seg + 2) pixels - for all nine taps: 43.5 KB (seg = 64) / 33 KB (seg = 16, 32) per 9.4 MFLOP = 1.7-2.3x fewer staged bytes per
// FLOP, and a third of the tiles per pixel range.
//   * 512 threads = 8 waves as 2 (output channels: BM / 2 each) x 4 (the four 16-channel quarters of the input block): a wave's
//     columns are (tap 0..8) x (its 16 channels) - the swizzle slot of its B reads is then a LANE CONSTANT and the tap is
//       kw -> one of 3 address registers per pixel group (the halo row shifts by one),  kh -> an INSTRUCTION IMMEDIATE:
//     the halo row pitch is padded to a multiple of 8 rows (hwp = 24 / 40 / 72 for seg = 16 / 32 / 64), so kh * hwp never moves the
//     swizzle key ((row >> 1) & 3).  12 + 4 * TM address registers serve all 36 + 4 * TM transpose reads of a step.
//   * SEG (pixels of an image row per step: min(64, Wo)) is a template parameter: pitch, immediates and the pixel -> halo row map
//     are compile-time.
//   * accumulators TM x 9 tiles of 16 x 16 (144 registers at BM = 128), one workgroup per CU, 3-stage LDS-DMA ring
//     (3 x 48 KB at BM = 128 / seg = 64), one barrier per step; every wave issues the same NVA + NPASS LDS-DMA instructions per step
//     (rows past the halo are fetched out of bounds = zeros), so the counted vmcnt is a compile-time constant.
//   * partial slab per segment: fragment-major [wave][i][tap][lane] float4, summed in line order by wgrad_group9_reduce_kernel.
// Eligibility = the row-of-taps rules (3x3 / s1 / p1, 64-channel blocks, uniform-row maps), no fused producer BatchNormalization.
template <int SEG> struct Taps9Geo {
  static constexpr int ROWS = 64 / SEG, HW = SEG + 2, HWP = (HW + 7) / 8 * 8, HR = (ROWS + 2) * HWP;
  static constexpr int NPASS = (HR + 63) / 64, LROWS = NPASS * 64;
};

template <int BM, int SEG, int STAGES, bool M32>
__device__ __forceinline__ void conv_wgrad_taps9_body(const WgradArgs& a, const int t, const int step0, const int step1, f32x4* const out_tile) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef Taps9Geo<SEG> G;
  constexpr int SZ = 2, PK = 64;
  constexpr int TM = BM / 2 / 16, TN = 9;
  constexpr int ROWA = BM * SZ, ROWB = 128;
  constexpr int VPRA = ROWA / 16, RPA = 512 / VPRA, NVA = (PK + RPA - 1) / RPA;
  constexpr int ABYTES = (PK * ROWA > NVA * 512 * 16) ? PK * ROWA : NVA * 512 * 16;     // (BM = 32: the single pass covers 128 rows)
  constexpr int STAGE = ABYTES + G::LROWS * ROWB;
  constexpr int L = NVA + G::NPASS;                               // LDS-DMA instructions per thread per step (every wave)
  static_assert(BM == 128 || BM == 64 || BM == 32, "output-channel tile");
  static_assert(!M32 || BM == 128, "the 32 x 32 x 16 form: 4 x 2 waves of 32 channels x (9 taps x 32 input channels)");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // The thread index passes through an opaque asm: the lane constants below (fragment and LDS-DMA addresses) depend only on it and
  // on SEG, so the compiler would hoist those of ALL THREE bodies of conv_wgrad_taps9_group_kernel out of its segment loop and keep
  // them alive across it - ~50 registers that the BM = 128 instance does not have (42 spills).  Recomputed per segment instead.
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int lr = lane & 15, lg = lane >> 4;

  const int tile_m = t % a.ntile_m, cib = t / a.ntile_m;         // cib: 64-channel block of the CONCATENATED input
  const bool first = cib * 64 < a.C0;                            // wave-uniform: which source holds this block
  const int cs = first ? a.C0 : a.C1, cb_src = first ? cib : cib - (a.C0 >> 6);
  const int sh = (first && a.mode == STP_SRC_NEAREST2X) ? 1 : 0;
  const int Hs = first ? a.Hs0 : a.Hv, Ws = first ? a.Ws0 : a.Wv;
  const int cout0 = tile_m * BM;

  const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)a.dy, 0, a.bytesdy, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)(first ? a.src0 : a.src1), 0, first ? a.bytes0 : a.bytes1, 0x00020000);

  // ---- LDS-DMA constants.  A (dY): pass i = pixel rows i * RPA + tid / VPRA.  B: LDS halo row h = pass * 64 + tid / 8 -> image row
  // h / HWP - 1, column h % HWP - 1 relative to the step's first pixel (pad columns and rows past the halo: out of bounds)
  const int rowA0 = tid / VPRA;
  const int colA = (tile_addr<ROWA>(rowA0, (tid % VPRA) * 16) - rowA0 * ROWA) / SZ;
  const bool coA_ok = (cout0 + colA) < a.Cout;
  uint32_t rowa[NVA];
#pragma unroll
  for (int i = 0; i < NVA; ++i)
    rowa[i] = (rowA0 + i * RPA) < PK ? ((uint32_t)(rowA0 + i * RPA) * (uint32_t)a.Cout + (uint32_t)(cout0 + colA)) * SZ : STP_OOB;
  const int hb0 = tid >> 3;
  const uint32_t colB = (uint32_t)(tile_addr<ROWB>(hb0, (tid & 7) * 16) - hb0 * ROWB);    // logical byte column held by this slot (hb0 + 64 p: same key)
  // (image row / column of halo row pass * 64 + hb0 relative to the step's first pixel: recomputed per piece from hb0 - compile-time
  //  divisor, ~6 VALU - instead of 2 x NPASS registers: the BM = 128 instance sits at the 256-register limit)
  const uint32_t pixb = (uint32_t)cs * SZ, imgb = (uint32_t)Hs * (uint32_t)Ws * pixb, cbyte = (uint32_t)cb_src * 128u + colB;

  // a tile = L pieces (LDS-DMA instructions): pieces 0 .. NVA-1 = dY, NVA .. L-1 = halo passes.  The step's scalar geometry
  // (image, first row / column, byte bases) is computed once (tile_geo), a piece adds its lane constants.
  struct TileGeo { uint32_t ho0, wo0, abase, nb; };
  auto tile_geo = [&](int step) {
    const int p0 = step * PK;
    const uint32_t n = fdiv((uint32_t)p0, a.divHoWo);
    const uint32_t rem = (uint32_t)p0 - n * (uint32_t)a.HoWo;
    TileGeo tg;
    tg.ho0 = fdiv(rem, a.divWo);
    tg.wo0 = rem - tg.ho0 * (uint32_t)a.Wo;
    tg.abase = (uint32_t)p0 * (uint32_t)a.Cout * SZ;
    tg.nb = n * imgb + cbyte;
    return tg;
  };
  auto issue_piece = [&](const TileGeo& tg, int buf, int piece) __attribute__((always_inline)) {
    char* sa = smem + buf * STAGE;
    if (piece < NVA) {
      const int i = piece;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsd, (__attribute__((address_space(3))) void*)(sa + (i * 512 + wave * 64) * 16), 16,
                                               (coA_ok && rowa[i] != STP_OOB) ? tg.abase + rowa[i] : STP_OOB, 0, 0, 0);
    } else {
      const int i = piece - NVA;
      const int h = hb0 + i * 64;
      const int r = h / G::HWP, c = h - r * G::HWP;
      const int hv = (int)tg.ho0 + r - 1, wv = (int)tg.wo0 + c - 1;
      const bool ok = r < G::ROWS + 2 && c < G::HW && (unsigned)hv < (unsigned)a.Hv && (unsigned)wv < (unsigned)a.Wv;
      const uint32_t off = tg.nb + ((uint32_t)(hv >> sh) * (uint32_t)Ws + (uint32_t)(wv >> sh)) * pixb;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (__attribute__((address_space(3))) void*)(sa + ABYTES + (i * 512 + wave * 64) * 16), 16,
                                               ok ? off : STP_OOB, 0, 0, 0);
    }
  };
  auto issue_tile = [&](int step, int buf) {
    const TileGeo tg = tile_geo(step);
#pragma unroll
    for (int pc = 0; pc < L; ++pc) issue_piece(tg, buf, pc);
  };

  // The transpose reads are INLINE ASM with hand-counted lgkmcnt waits (see the 16 x 16 x 32 path below for why).
  auto tr_read = [&](uint32_t addr, auto off) __attribute__((always_inline)) {
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(decltype(off)::value));
    return v;
  };
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;      // LDS byte address of the ring (the asm reads take addresses)

  if constexpr (M32) {
    // ---- v_mfma_f32_32x32x16 form (BM = 128): 8 waves = 4 (32 output channels) x 2 (32 of the block's 64 input channels); a wave's
    // tile = 32 channels x (9 taps x 32 channels) = 9 accumulators of 32 x 32.  The 16 x 16 x 32 form tops out at 80 % of the MFMA
    // peak (MI355X_MICROARCH.md: ~5 vs ~8 cycles per CU for half the FLOP), and the all-taps loop is MFMA-issue bound
    // (profiles/r04h_pmc_sq.json: issue stalls 46 % of the wave cycles, MFMA pipe busy 44 %).
    // Operand layout: lane group g = lane >> 4 holds rows / columns 16 (g & 1) .. +15 and k = 8 (g >> 1) .. +7 of a 16-pixel k-step:
    // pixels 16 kk + 8 (g >> 1) + {0..3} from the first transpose read, + {4..7} from the second.  kk and the kernel row are
    // instruction immediates (16 pixels = 16 LDS rows, a kernel row = HWP rows: multiples of 8 rows, same swizzle key); the channel
    // block (g & 1) and the tap column kw sit in the 2 + 6 address registers.
    const int wm4 = wave >> 1, wn2 = wave & 1;
    const int hh = lg & 1, kh2 = lg >> 1;
    const int qb32 = (lr & 3) * 8;
    uint32_t a32[2], b32[2][3];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int q0 = kh2 * 8 + half * 4 + (lr >> 2);
      a32[half] = (uint32_t)tile_addr<ROWA>(q0, (wm4 * 32 + hh * 16) * SZ + qb32);
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) b32[half][kw] = (uint32_t)(ABYTES + tile_addr<ROWB>(q0 + kw, (wn2 * 32 + hh * 16) * SZ + qb32));
    }
    f32x16 acc32[9];
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc32[j][e] = 0.f;
    auto read_a32 = [&](uint32_t st, auto kkc, u32x4& fa) __attribute__((always_inline)) {
      constexpr int OFF = decltype(kkc)::value * 16 * ROWA;
      const u32x2 l2 = tr_read(st + a32[0], std::integral_constant<int, OFF>{});
      const u32x2 h2 = tr_read(st + a32[1], std::integral_constant<int, OFF>{});
      fa = u32x4{l2.x, l2.y, h2.x, h2.y};
    };
    auto read_b32 = [&](uint32_t st, auto kkc, auto khc, u32x4 (&fb)[3]) __attribute__((always_inline)) {
      constexpr int Q = decltype(kkc)::value * 16;
      constexpr int OFF = ((Q / SEG) * G::HWP + (Q % SEG) + decltype(khc)::value * G::HWP) * ROWB;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const u32x2 l2 = tr_read(st + b32[0][kw], std::integral_constant<int, OFF>{});
        const u32x2 h2 = tr_read(st + b32[1][kw], std::integral_constant<int, OFF>{});
        fb[kw] = u32x4{l2.x, l2.y, h2.x, h2.y};
      }
    };
    auto wait32 = [&](auto young, u32x4& fa, u32x4 (&fb)[3]) __attribute__((always_inline)) {
      asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(fa), "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]) : "n"(decltype(young)::value));
    };
    static_assert(L <= 6, "one LDS-DMA piece per two MFMA groups");
    // 12 groups (k-step kk = 0..3) x (kernel row kh = 0..2) of 3 MFMAs; the fragments of group g + 1 (and the A fragment of the next
    // k-step) are requested before the MFMAs of group g; an LDS-DMA piece of the next tile follows every second group.
    auto compute32 = [&](uint32_t st, bool next, int nstep, int nb_) {
      u32x4 fa[2], fb[2][3];
      TileGeo tg = {0u, 0u, 0u, 0u};
      if (next) tg = tile_geo(nstep);
      read_a32(st, std::integral_constant<int, 0>{}, fa[0]);
      read_b32(st, std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{}, fb[0]);
#define STP_T9M_GROUP(G_, KK_, KH_, KKN_, KHN_)                                                                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                                            \
      if (KH_ == 0 && KK_ < 3) read_a32(st, std::integral_constant<int, (KK_ + 1) & 3>{}, fa[(KK_ + 1) & 1]);                       \
      if (G_ + 1 < 12) read_b32(st, std::integral_constant<int, KKN_>{}, std::integral_constant<int, KHN_>{}, fb[(G_ + 1) & 1]);    \
      wait32(std::integral_constant<int, (G_ + 1 < 12 ? 6 : 0) + ((KH_ == 0 && KK_ < 3) ? 2 : 0)>{}, fa[KK_ & 1], fb[G_ & 1]);      \
      __builtin_amdgcn_sched_barrier(0);                                                                                            \
      _Pragma("unroll") for (int kw = 0; kw < 3; ++kw)                                                                              \
        acc32[KH_ * 3 + kw] = mfma16_32x32x16(fa[KK_ & 1], fb[G_ & 1][kw], acc32[KH_ * 3 + kw]);                                    \
      __builtin_amdgcn_sched_barrier(0);                                                                                            \
      if ((G_ & 1) == 0 && G_ / 2 < L && next) issue_piece(tg, nb_, G_ / 2);
      STP_T9M_GROUP(0, 0, 0, 0, 1)
      STP_T9M_GROUP(1, 0, 1, 0, 2)
      STP_T9M_GROUP(2, 0, 2, 1, 0)
      STP_T9M_GROUP(3, 1, 0, 1, 1)
      STP_T9M_GROUP(4, 1, 1, 1, 2)
      STP_T9M_GROUP(5, 1, 2, 2, 0)
      STP_T9M_GROUP(6, 2, 0, 2, 1)
      STP_T9M_GROUP(7, 2, 1, 2, 2)
      STP_T9M_GROUP(8, 2, 2, 3, 0)
      STP_T9M_GROUP(9, 3, 0, 3, 1)
      STP_T9M_GROUP(10, 3, 1, 3, 2)
      STP_T9M_GROUP(11, 3, 2, 0, 0)
#undef STP_T9M_GROUP
      __builtin_amdgcn_sched_barrier(0);
    };
    const int nst = step1 - step0;
#pragma unroll
    for (int q = 0; q < STAGES - 1; ++q)
      if (q < nst) issue_tile(step0 + q, q);
    int buf = 0, nbuf = STAGES - 1;
    for (int st = 0; st < nst; ++st) {
      const int ahead = nst - 1 - st;
      if (STAGES >= 3 && ahead >= STAGES - 2) wait_vmcnt<(STAGES - 2) * L>();
      else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      compute32(lds0 + (uint32_t)(buf * STAGE), st + STAGES - 1 < nst, step0 + st + STAGES - 1, nbuf);
      buf = (buf + 1 == STAGES) ? 0 : buf + 1;
      nbuf = (nbuf + 1 == STAGES) ? 0 : nbuf + 1;
    }
    // slab: [wave][tap][q][lane] float4 = rows 8 q + 4 (lane >> 5) + {0..3} (output channels) of column lane & 31 (taps9_slab_decode)
    f32x4* out = out_tile + (size_t)wave * (9 * 4 * 64) + lane;
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        out[(j * 4 + q) * 64] = f32x4{acc32[j][4 * q], acc32[j][4 * q + 1], acc32[j][4 * q + 2], acc32[j][4 * q + 3]};
    return;
  }

  // ---- fragment addresses (bytes from the stage base).  Pixel q of the step (row q / SEG, column q % SEG); a 16-lane group reads 4
  // consecutive pixels: lane -> pixel (lr >> 2), 8-byte quad (lr & 3) of the 32-byte channel block.
  const int qb = (lr & 3) * 8;
  // A: the 32-byte channel block i of a wave sits in byte bits 5.. of the row, the swizzle key XORs the same bits: block i = block 0
  // XOR (i * 32) - one address register per pixel group (4 instead of 4 x TM)
  int aaddr[4], baddr[4][3];           // [pixel group e = chunk * 2 + half] / [e][kw]
  static_assert(ROWA >= 64 && ((BM / 2) * SZ) % (TM * 32) == 0, "the wave's channel blocks occupy an aligned bit field of the row");
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = e * 16 + lg * 4 + (lr >> 2);
    aaddr[e] = tile_addr<ROWA>(q, (wm * (BM / 2)) * SZ + qb);
    const int r = q / SEG, c = q - r * SEG;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) baddr[e][kw] = ABYTES + tile_addr<ROWB>(r * G::HWP + c + kw, wn * 32 + qb);
  }

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // A step = 2 chunks of 32 pixels x 3 kernel rows = 6 groups of 3 taps x TM MFMAs.  The B fragments of group g + 1 are requested
  // BEFORE the MFMAs of group g (two sets of 12 registers, pinned by sched_barrier: left alone, the scheduler hoists every read of
  // the step to its top - 52 fragment registers on top of 144 accumulators + 28 addresses = 36 spills at BM = 128).
  // The transpose reads are INLINE ASM with hand-counted lgkmcnt waits: through the builtin, the compiler's wait-count pass puts
  // `s_waitcnt vmcnt(0)` in front of the first LDS read after every LDS-DMA instruction (it cannot tell that the ring slot being
  // filled is not the one being read) - with the pieces of the next tile issued between the MFMA groups that drained the whole DMA
  // queue six times per step (first build: 5600 cycles per step for 2304 cycles of MFMA work).  The step's barrier + counted vmcnt
  // order the slot that IS read.
  auto read_a = [&](uint32_t st, int c, u32x4 (&fa)[TM]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const u32x2 l2 = tr_read(st + (uint32_t)(aaddr[2 * c] ^ (i * 32)), std::integral_constant<int, 0>{});
      const u32x2 h2 = tr_read(st + (uint32_t)(aaddr[2 * c + 1] ^ (i * 32)), std::integral_constant<int, 0>{});
      fa[i] = u32x4{l2.x, l2.y, h2.x, h2.y};
    }
  };
  // (kernel row kh = a compile-time byte offset: a multiple of 8 LDS rows, same swizzle key)
  auto read_b = [&](uint32_t st, int c, auto khc, u32x4 (&fb)[3]) __attribute__((always_inline)) {
    constexpr int OFF = decltype(khc)::value * G::HWP * ROWB;
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const u32x2 l2 = tr_read(st + (uint32_t)baddr[2 * c][kw], std::integral_constant<int, OFF>{});
      const u32x2 h2 = tr_read(st + (uint32_t)baddr[2 * c + 1][kw], std::integral_constant<int, OFF>{});
      fb[kw] = u32x4{l2.x, l2.y, h2.x, h2.y};
    }
  };
  // everything but the `young` most recent LDS reads has returned; the fragments are operands of the asm, so no MFMA that consumes
  // them can be scheduled above the wait
  auto wait_frags = [&](auto young, u32x4 (&fa)[TM], u32x4 (&fb)[3]) __attribute__((always_inline)) {
    if constexpr (TM == 4)
      asm volatile("s_waitcnt lgkmcnt(%7)" : "+v"(fa[0]), "+v"(fa[1]), "+v"(fa[2]), "+v"(fa[3]), "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]) : "n"(decltype(young)::value));
    else if constexpr (TM == 2)
      asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(fa[0]), "+v"(fa[1]), "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]) : "n"(decltype(young)::value));
    else
      asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(fa[0]), "+v"(fb[0]), "+v"(fb[1]), "+v"(fb[2]) : "n"(decltype(young)::value));
  };
  static_assert(L <= 6, "one LDS-DMA piece per MFMA group");
  // A step = 2 chunks of 32 pixels x 3 kernel rows = 6 groups of 3 taps x TM MFMAs.  The B fragments of group g + 1 are requested
  // BEFORE the MFMAs of group g (two sets of 12 registers).  `next`: the pieces of tile `nstep` go into ring slot `nb_` BETWEEN the
  // MFMA groups, one per group (an LDS-DMA instruction costs ~60 issue cycles among MFMAs, 100-180 in a burst that opens the step).
  // Steps are software-pipelined ACROSS the step barrier (-DSTP_T9_NOPIPE: the what-if build without): the barrier of step st + 1 sits in front of the
  // LAST MFMA group of step st - every wave has waited for its own pieces of tile st + 1 and for every fragment read of the current
  // slot - and the first fragments of step st + 1 are requested before / right behind those MFMAs.  With the barrier at the top of the
  // step every wave sat through the first read round trip of every step with the MFMA pipe empty (~400 of ~3700 cycles per step).
  constexpr int P5 = L < 5 ? L : 5;                          // pieces of the next-but-one tile issued before the last group
#if defined(STP_T9_NOPIPE)
  constexpr bool PIPE = false;
#else
  constexpr bool PIPE = true;
#endif
  u32x4 fa[TM], fb[2][3];
  auto compute = [&](uint32_t st, uint32_t st_nx, bool more, bool next, int nstep, int nb_) {
    TileGeo tg = {0u, 0u, 0u, 0u};
    if (next) tg = tile_geo(nstep);
#define STP_T9_MFMAS(G_, KH_)                                                                                    \
    _Pragma("unroll") for (int kw = 0; kw < 3; ++kw)                                                             \
      _Pragma("unroll") for (int i = 0; i < TM; ++i)                                                             \
        acc[i][KH_ * 3 + kw] = mfma16_16x16x32(fa[i], fb[G_ & 1][kw], acc[i][KH_ * 3 + kw]);
#define STP_T9_GROUP(G_, C_, KH_, CN_, KHN_)                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    read_b(st, CN_, std::integral_constant<int, KHN_>{}, fb[(G_ + 1) & 1]);                                      \
    wait_frags(std::integral_constant<int, 6>{}, fa, fb[G_ & 1]);                                                \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    STP_T9_MFMAS(G_, KH_)                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                                           \
    if (G_ < L && next) issue_piece(tg, nb_, G_);                                                                \
    if (G_ == 2) {   /* the A fragments of the second chunk, behind the last MFMAs that read the first */        \
      __builtin_amdgcn_sched_barrier(0);                                                                         \
      read_a(st, 1, fa);                                                                                         \
    }
    // (fa = A fragments of chunk 0 and fb[0] = group 0 of THIS step are in flight: requested by the prologue / the previous step)
    // (group 2 -> 3: the 2 * TM reads of read_a(1) are OLDER than the 6 of read_b(group 4), so "all but the youngest 6" covers them)
    STP_T9_GROUP(0, 0, 0, 0, 1)
    STP_T9_GROUP(1, 0, 1, 0, 2)
    STP_T9_GROUP(2, 0, 2, 1, 0)
    STP_T9_GROUP(3, 1, 0, 1, 1)
    STP_T9_GROUP(4, 1, 1, 1, 2)
    // ---- group 5 (its B fragments were requested in group 4) + the hand-over to the next step
    __builtin_amdgcn_sched_barrier(0);
    wait_frags(std::integral_constant<int, 0>{}, fa, fb[1]);        // every LDS read of this wave has returned (the current slot is done with)
    if (PIPE && more) {
      if (next) wait_vmcnt<P5>(); else wait_vmcnt<0>();              // own pieces of tile st + 1 have landed (the P5 youngest: tile st + 2)
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      read_b(st_nx, 0, std::integral_constant<int, 0>{}, fb[0]);
    }
    __builtin_amdgcn_sched_barrier(0);
    STP_T9_MFMAS(5, 2)
    __builtin_amdgcn_sched_barrier(0);
    if (5 < L && next) issue_piece(tg, nb_, 5);
    if (PIPE && more) {
      __builtin_amdgcn_sched_barrier(0);
      read_a(st_nx, 0, fa);
    }
#undef STP_T9_GROUP
#undef STP_T9_MFMAS
    __builtin_amdgcn_sched_barrier(0);
  };

  const int nst = step1 - step0;
#pragma unroll
  for (int q = 0; q < STAGES - 1; ++q)
    if (q < nst) issue_tile(step0 + q, q);
  static_assert(STAGES == 3, "the pipelined hand-over assumes the 3-slot ring");
  if (nst > 1) wait_vmcnt<L>(); else wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  read_a(lds0, 0, fa);
  read_b(lds0, 0, std::integral_constant<int, 0>{}, fb[0]);
  int buf = 0, nbuf = STAGES - 1;
  for (int st = 0; st < nst; ++st) {
    const int nx = (buf + 1 == STAGES) ? 0 : buf + 1;
    if (!PIPE && st > 0) {                                   // (what-if build: barrier and first reads at the top of every step)
      if (st + 1 < nst) wait_vmcnt<L>(); else wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();
      read_a(lds0 + (uint32_t)(buf * STAGE), 0, fa);
      read_b(lds0 + (uint32_t)(buf * STAGE), 0, std::integral_constant<int, 0>{}, fb[0]);
    }
    compute(lds0 + (uint32_t)(buf * STAGE), lds0 + (uint32_t)(nx * STAGE), st + 1 < nst, st + STAGES - 1 < nst, step0 + st + STAGES - 1, nbuf);
    buf = nx;
    nbuf = (nbuf + 1 == STAGES) ? 0 : nbuf + 1;
  }

  // ---- slab, fragment-major: [wave][i][tap][lane] float4 = the lane's 4 output channels of one column (taps9_slab_decode)
  f32x4* out = out_tile + (size_t)wave * (TM * TN * 64) + lane;
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) out[(i * TN + j) * 64] = acc[i][j];
#endif
}

// element e (float4) of an all-taps tile's slab -> first of its 4 output channels (relative to the tile), tap and input channel (0..63)
template <int BM, bool M32> __device__ __forceinline__ void taps9_slab_decode(int e, int& co, int& tap, int& ci) {
  const int lane = e & 63;
  if constexpr (M32) {
    const int t2 = e >> 6, q = t2 & 3, t3 = t2 >> 2;
    tap = t3 % 9;
    const int wave = t3 / 9;
    co = (wave >> 1) * 32 + 8 * q + 4 * (lane >> 5);
    ci = (wave & 1) * 32 + (lane & 31);
  } else {
    constexpr int TM = BM / 2 / 16;
    const int q = e >> 6;
    const int ij = q % (TM * 9), wave = q / (TM * 9);
    const int i = ij / 9;
    tap = ij - i * 9;
    co = (wave >> 2) * (BM / 2) + i * 16 + (lane >> 4) * 4;
    ci = (wave & 3) * 16 + (lane & 15);
  }
}

template <int BM, int STAGES, bool M32 = false>
__global__ __launch_bounds__(512) void conv_wgrad_taps9_group_kernel(const char* __restrict__ table, f32x4* __restrict__ slabs) {
  const WgGroupHeader* const hd = reinterpret_cast<const WgGroupHeader*>(table);
  const WgLayer* const layers = reinterpret_cast<const WgLayer*>(table + hd->off_layers);
  const WgSeg* const segs = reinterpret_cast<const WgSeg*>(table + hd->off_segs);
  const int* const first = reinterpret_cast<const int*>(table + hd->off_first);
  const int w = hd->xcd == 1 ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
  const int s0 = __builtin_amdgcn_readfirstlane(first[w]), s1 = __builtin_amdgcn_readfirstlane(first[w + 1]);
  for (int s = s0; s < s1; ++s) {
    WgSeg sg;
    load_constant(sg, segs + s);
    WgradArgs a;
    load_constant(a, &layers[sg.layer].a);
    if (s != s0) __syncthreads();        // the previous segment's last fragment reads precede this segment's first LDS-DMA
    f32x4* const out = slabs + (size_t)sg.slot * (BM * 576 / 4);
    // a group mixes feature-map widths (decoder + encoder stages): the segment's layer picks the body (wave-uniform)
    if (a.Wo >= 64) conv_wgrad_taps9_body<BM, 64, STAGES, M32>(a, sg.tile, sg.step0, sg.step1, out);
    else if (a.Wo == 32) conv_wgrad_taps9_body<BM, 32, STAGES, M32>(a, sg.tile, sg.step0, sg.step1, out);
    else conv_wgrad_taps9_body<BM, 16, STAGES, M32>(a, sg.tile, sg.step0, sg.step1, out);
  }
}

template <int BM, int SL, bool M32 = false>
__global__ __launch_bounds__(256) void wgrad_group9_reduce_kernel(const char* __restrict__ table, const f32x4* __restrict__ slabs) {
  constexpr int PER = BM * 576 / 4, EPB = 256 / SL, BPT = PER / EPB;
  static_assert(PER % EPB == 0, "whole blocks per tile");
  __shared__ f32x4 shm[SL][EPB];
  const WgGroupHeader* const hd = reinterpret_cast<const WgGroupHeader*>(table);
  const WgLayer* const layers = reinterpret_cast<const WgLayer*>(table + hd->off_layers);
  const int* const slot_list = reinterpret_cast<const int*>(table + hd->off_slots);
  const WgTile tl = reinterpret_cast<const WgTile*>(table + hd->off_tiles)[blockIdx.x / BPT];
  const int ev = threadIdx.x % EPB, sl = threadIdx.x / EPB;
  const int e = (blockIdx.x % BPT) * EPB + ev;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  {
    int k = sl;
    for (; k + 3 * SL < tl.nslots; k += 4 * SL) {
      const f32x4 a0 = slabs[(size_t)slot_list[tl.list0 + k] * PER + e], a1 = slabs[(size_t)slot_list[tl.list0 + k + SL] * PER + e];
      const f32x4 a2 = slabs[(size_t)slot_list[tl.list0 + k + 2 * SL] * PER + e], a3 = slabs[(size_t)slot_list[tl.list0 + k + 3 * SL] * PER + e];
      s += a0; s += a1; s += a2; s += a3;
    }
    for (; k < tl.nslots; k += SL) s += slabs[(size_t)slot_list[tl.list0 + k] * PER + e];
  }
  if (SL > 1) {
    shm[sl][ev] = s;
    __syncthreads();
#pragma unroll
    for (int w = SL / 2; w > 0; w >>= 1) {
      if (sl < w) shm[sl][ev] += shm[sl + w][ev];
      __syncthreads();
    }
    s = shm[0][ev];
    if (sl != 0) return;
  }
  const WgLayer& L = layers[tl.layer];
  int co, tap, ci;
  taps9_slab_decode<BM, M32>(e, co, tap, ci);
  const int tile_m = tl.t % L.a.ntile_m, cib = tl.t / L.a.ntile_m;
  const int kc = tap * L.a.Ctot + cib * 64 + ci;
  co += tile_m * BM;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (co + r < L.a.Cout) {
      float* d = L.dw + (size_t)(co + r) * L.a.K + kc;
      *d = L.accumulate ? *d + s[r] : s[r];
    }
}

// ---- launchers of the group (the header is the validated host copy of the table; m32: header taps9 == 2, the 128 class only) ------
int wgrad_taps9_group_partial(const WgGroupHeader* hd, const void* dev_table, void* workspace, hipStream_t s) {
  // 3 stages x (dY tile + 256 halo rows of 128 bytes - the seg = 64 geometry, the largest)
  const size_t lds9 = (size_t)3 * ((hd->bm == 128 ? 16384 : 8192) + 256 * 128);
  static_assert((size_t)3 * (8192 + 256 * 128) > STP_LDS_DEFAULT, "every launch of these kernels needs the grant");
  auto launch9 = [&](auto kern) { return stp_launch_lds(kern, dim3(hd->n_wg), dim3(512), lds9, s, (const char*)dev_table, (f32x4*)workspace); };
  return row_class(hd->bm, [&](auto c) -> int {
    constexpr int BM = decltype(c)::BM;
    if constexpr (BM == 128) {
      if (hd->taps9 == 2) return launch9(conv_wgrad_taps9_group_kernel<128, 3, true>);
    }
    return launch9(conv_wgrad_taps9_group_kernel<BM, 3>);
  });
}

int wgrad_taps9_group_reduce(const WgGroupHeader* hd, const void* dev_table, const void* workspace, hipStream_t s) {
  const int sl = hd->reduce_lanes == 4 ? 4 : 1;
  const dim3 grid9(hd->n_tiles * (hd->bm * 576 / 4 / (256 / sl)));
  auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, grid9, dim3(256), 0, s, (const char*)dev_table, (const f32x4*)workspace); };
  const int rc = row_class(hd->bm, [&](auto c) -> int {
    constexpr int BM = decltype(c)::BM;
    if constexpr (BM == 128) {
      if (hd->taps9 == 2) {
        if (sl == 4) launch(wgrad_group9_reduce_kernel<128, 4, true>);
        else launch(wgrad_group9_reduce_kernel<128, 1, true>);
        return STP_OK;
      }
    }
    if (sl == 4) launch(wgrad_group9_reduce_kernel<BM, 4>);
    else launch(wgrad_group9_reduce_kernel<BM, 1>);
    return STP_OK;
  });
  if (rc != STP_OK) return rc;
  STP_LAUNCH_CHECK();
  return STP_OK;
}
