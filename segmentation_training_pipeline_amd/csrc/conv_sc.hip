// "Small-channel" 3x3 / stride-1 / pad-1 convolution for the full-resolution decoder tail and the head
// (Cin <= 32, Cout <= 32): these layers are HBM-bound (AI 8..96 FLOP/B), and the generic
// implicit-GEMM gather re-reads every input pixel 9 times through the vector-memory path.
//
// Here a workgroup owns an 8 x 32 output tile: the (8+2) x (32+2) x Cin input halo tile is staged ONCE in
// LDS (coalesced 16-byte vectors, padding and nearest-2x upsampling resolved while staging), the whole
// weight matrix lives in registers as MFMA A fragments, and every B fragment is a single ds_read_b128
// from the halo tile at (pixel + tap offset): no im2col copy exists anywhere.  Per 16 output pixels:
// ceil(9*Cin/32) LDS reads and as many MFMAs per 16 output channels.  With ~11-22 KB of LDS per
// workgroup 7+ workgroups share a CU, which is what hides the load latency of this streaming kernel.
//
//   C[cout][pixel] = sum_k W[cout][k] * halo[pixel + tap(k)][ch(k)],   k = tap*Cin + ch, tap = kh*3 + kw
// The k -> (lane group, vector slot) assignment is the same for A and B (all a contraction needs).
// Used for forward and (with the flipped/transposed weight copy) for the data gradient.
#include "conv_sc_epilogue.h"

template <typename T, int CIN, int TM>
__global__ __launch_bounds__(256) void conv_sc_kernel(const ScArgs a) {
  constexpr int SZ = (int)sizeof(T);
  constexpr int VEC = Elem<T>::VEC;
  constexpr int KC = 4 * VEC;                    // k values per MFMA chunk (32 bf16 / 16 fp32)
  constexpr int K = 9 * CIN;
  constexpr int NCH = (K + KC - 1) / KC;
  constexpr int VPP = CIN / VEC;                 // 16-byte vectors per pixel
  constexpr int PIXB = CIN * SZ;                 // bytes per pixel in the halo tile
  static_assert(CIN % VEC == 0, "CIN must be a multiple of the 16-byte vector");

  extern __shared__ __attribute__((aligned(16))) char halo[];  // [SC_HH][SC_HW][CIN]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;

  int b = blockIdx.x;
  const int bq = (int)fdiv((uint32_t)b, a.divTx);
  const int tx = b - bq * a.tiles_x;
  const int n = (int)fdiv((uint32_t)bq, a.divTy);
  const int ty = bq - n * a.tiles_y;
  const int y0 = ty * SC_TH, x0 = tx * SC_TW;

  // ---- stage the halo tile -----------------------------------------------------------------
  const int sh = a.up ? 1 : 0;
  const char* img = a.src + (size_t)n * a.Hs * a.Ws * PIXB;
  static_assert(256 % VPP == 0, "a thread stages the same channel vector in every pass");
  const bool pbn = a.pbn.mean != nullptr;
  ScStageBn<T> sbn;
  if (pbn) sbn.load(a.pbn, (tid % VPP) * VEC);
  for (int v = tid; v < SC_HH * SC_HW * VPP; v += 256) {
    const int pix = v / VPP, cv = v - pix * VPP;
    const int hy = pix / SC_HW, hx = pix - hy * SC_HW;
    const int gy = y0 - 1 + hy, gx = x0 - 1 + hx;
    u32x4 val = {0u, 0u, 0u, 0u};
    if ((unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W) {
      val = *reinterpret_cast<const u32x4*>(img + ((size_t)(gy >> sh) * a.Ws + (gx >> sh)) * PIXB + cv * 16);
      if (pbn) val = sbn.apply(val, a.pbn.relu);
    }
    *reinterpret_cast<u32x4*>(halo + v * 16) = val;
  }

  // ---- weights -> registers (A fragments), per-lane tap offsets of the B fragments -----------
  u32x4 fa[TM][NCH];
  int boff[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k0 = c * KC + lg * VEC;
    const int tap = k0 / CIN, ch = k0 - tap * CIN;
    const int kh = tap / 3, kw = tap - kh * 3;
    boff[c] = (k0 < K) ? ((kh * SC_HW + kw) * CIN + ch) * SZ : -1;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      u32x4 w = {0u, 0u, 0u, 0u};
      if (k0 < K) w = *reinterpret_cast<const u32x4*>(a.weight + ((size_t)(i * 16 + lr) * K + k0) * SZ);
      fa[i][c] = w;
    }
  }
  __syncthreads();
  float* red = reinterpret_cast<float*>(halo + SC_HH * SC_HW * PIXB);  // [4][TM*16][2] behind the halo tile
  // (A variant that looped over 16-channel passes of the same halo tile to cut registers - 5 instead of 3 waves/SIMD for
  //  Cout = 32 - measured slower: the weights then load after the barrier instead of under the halo staging.)

  // ---- MFMAs: wave w owns tile rows 2w, 2w+1; 4 fragments of 16 pixels -------------------------
  f32x4 acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int py = wave * 2 + (f >> 1), px = (f & 1) * 16 + lr;
    const char* pbase = halo + (py * SC_HW + px) * PIXB;
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      u32x4 fb = {0u, 0u, 0u, 0u};
      if (boff[c] >= 0) fb = *reinterpret_cast<const u32x4*>(pbase + boff[c]);
#pragma unroll
      for (int i = 0; i < TM; ++i) ScMma<T>::run(fa[i][c], fb, acc[i][f]);
    }
  }

  // ---- epilogue -----------------------------------------------------------------------------------
  ScEpilogue<T, TM> ep;
  ep.load_constants(a, lg);
  ep.prefetch(a, n, y0, x0, wave, lr, lg);
  ep.finish(a, acc, red, n, y0, x0, (int)blockIdx.x, (int)gridDim.x, tid, wave, lr, lg);
}

// =================================================================================================
// STREAMING form of the kernel above (the one stp_conv2d_sc launches; the single-shot form stays for A/B runs, STP_SC_STREAM=0).
// The single-shot workgroup loads its halo tile through registers (2-6 dependent global-load round trips, the trip count is
// not a compile-time constant), synchronises, computes, stores and retires: measured 85-150 us on the 16x512x512 layers whose
// tensors take 30-55 us at HBM speed.  Here workgroups are PERSISTENT (a few per CU), the weights' A fragments and the fused
// BatchNormalization constants are fetched once per workgroup, and the halo tile of the NEXT tile is written straight into the
// other half of a double buffer by LDS-DMA (buffer_load ... lds, 16 bytes per lane, out-of-image pixels = out-of-range offset =
// zeros) while the current tile is multiplied and stored.  Per tile:
//   vmcnt(0) (own pieces of this tile, issued one tile ago) | producer BatchNormalization of the own pieces, in LDS | barrier |
//   epilogue operand prefetch | LDS-DMA of the next tile | MFMAs | epilogue (vmcnt leaves the DMA in flight) | stores
// Tiles are walked XCD by XCD: workgroup b (XCD b & 7) owns every (gridDim/8)-th tile of the b&7-th eighth of the tile list, so
// the halo rows shared by neighbouring tiles meet in one L2.  Same MFMA order, same epilogue arithmetic: results are bit-identical
// to the single-shot kernel.
// =================================================================================================
// (second launch bound = waves per SIMD = workgroups per CU the register allocation must leave room for)
template <typename T, int CIN, int TM>
__global__ __launch_bounds__(256, (TM == 1 ? (sizeof(T) == 2 && CIN <= 16 ? SC_WPE_SMALL : 3) : 2)) void conv_sc_stream_kernel(const ScArgs a) {
  constexpr int SZ = (int)sizeof(T);
  constexpr int VEC = Elem<T>::VEC;
  constexpr int KC = 4 * VEC;
  constexpr int K = 9 * CIN;
  constexpr int NCH = (K + KC - 1) / KC;
  constexpr int VPP = CIN / VEC;
  constexpr int PIXB = CIN * SZ;
  constexpr int NV = SC_HH * SC_HW * VPP;          // 16-byte vectors of a halo tile
  constexpr int NPASS = (NV + 255) / 256;          // LDS-DMA instructions per thread per tile
  constexpr int BUF = NPASS * 4096;                // one half of the double buffer (whole 1 KB wave pieces)
  static_assert(CIN % VEC == 0 && 256 % VPP == 0, "a thread stages the same channel vector in every pass");

  // LDS: [2][BUF] halo tiles | statistics scratch [4][TM*16][2] | BN-backward table [4][32] | producer-BN table [2][32]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* red = reinterpret_cast<float*>(smem + 2 * BUF);
  float* ktab = red + 4 * TM * 16 * 2;
  float* ptab = ktab + 128;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int sh = a.up ? 1 : 0;

  // ---- tiles of this workgroup ------------------------------------------------------------------
  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  int t_first, t_step, t_end;
  if ((gridDim.x & 7) == 0) {
    const int q = ntiles >> 3, r = ntiles & 7, x = blockIdx.x & 7;
    const int start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    t_first = start + (int)(blockIdx.x >> 3); t_step = (int)(gridDim.x >> 3); t_end = start + q + (x < r ? 1 : 0);
  } else {
    t_first = (int)blockIdx.x; t_step = (int)gridDim.x; t_end = ntiles;
  }
  if (t_first >= t_end) return;

  // ---- per-thread constants of the staging: halo coordinates of the vector of every pass ------------
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.src, 0, a.src_bytes, 0x00020000);
  int hyx[NPASS];            // hy << 16 | hx ; -1 past the tile
  const int cvb = (tid % VPP) * 16;
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int v = p * 256 + tid, pix = v / VPP;
    const int hy = pix / SC_HW, hx = pix - hy * SC_HW;
    hyx[p] = v < NV ? (hy << 16 | hx) : -1;
  }
  const bool pbn = a.pbn.mean != nullptr;

  auto decode = [&](int tile, int& n, int& y0, int& x0) {
    const int bq = (int)fdiv((uint32_t)tile, a.divTx);
    const int tx = tile - bq * a.tiles_x;
    n = (int)fdiv((uint32_t)bq, a.divTy);
    const int ty = bq - n * a.tiles_y;
    y0 = ty * SC_TH; x0 = tx * SC_TW;
  };
  // LDS-DMA of a tile into buffer half b; returns the mask of passes whose vector lies inside the image
  // (EVERY wave issues NPASS instructions for EVERY tile slot - a piece that lies past the tile, or a tile past the end of the list
  //  (live == false), is requested out of range: zeros into the buffer's slack / the idle half, no memory traffic.  With a
  //  conditional issue the compiler cannot count the instructions that follow the epilogue's operand prefetch and waits for
  //  (nearly) all of them, i.e. for the NEXT tile, in every tile's epilogue.)
  auto issue_tile = [&](int tile, int b, bool live) -> uint32_t {
    int n, y0, x0;
    decode(tile, n, y0, x0);
    uint32_t inside = 0;
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int gy = y0 - 1 + (hyx[p] >> 16), gx = x0 - 1 + (hyx[p] & 0xffff);
      const bool ok = live && hyx[p] >= 0 && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
      const uint32_t off = ok ? (uint32_t)((n * a.Hs + (gy >> sh)) * a.Ws + (gx >> sh)) * (uint32_t)PIXB + (uint32_t)cvb : 0x80000000u;
      inside |= ok ? (1u << p) : 0u;
#if !defined(STP_EXP) || STP_EXP != 12   // (what-if builds of scratch/sc_exp_build.sh: 11 = no output stores, 12 = no halo loads, 13 = no LDS reads / MFMAs)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(smem + b * BUF + p * 4096 + wave * 1024), 16, off, 0, 0, 0);
#endif
    }
    return inside;
  };

  uint32_t inside_cur = issue_tile(t_first, 0, true);

  // ---- once per workgroup: weights -> registers (A fragments), lane addresses of the B fragments, constant tables -> LDS ----
  u32x4 fa[TM][NCH];
  uint32_t bl[NCH];            // LDS address of fragment chunk c for tile row 2*wave, column lr (buffer half 0); ~0 = chunk past K
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const int k0 = c * KC + lg * VEC;
    const int tap = k0 / CIN, ch = k0 - tap * CIN;
    const int kh = tap / 3, kw = tap - kh * 3;
    bl[c] = (k0 < K) ? (uint32_t)((((wave * 2 + kh) * SC_HW + kw + lr) * CIN + ch) * SZ) : 0xffffffffu;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      u32x4 w = {0u, 0u, 0u, 0u};
      if (k0 < K) w = *reinterpret_cast<const u32x4*>(a.weight + ((size_t)(i * 16 + lr) * K + k0) * SZ);
      fa[i][c] = w;
    }
  }
  // (asm read path) the same addresses with the lane groups past K parked on address 0; last_ok: this lane's slot of the last chunk is below K
  uint32_t bla[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) bla[c] = (uint32_t)(uintptr_t)smem + (bl[c] == 0xffffffffu ? 0u : bl[c]);
  const bool last_ok = (NCH - 1) * KC + lg * VEC < K;
  ScEpilogue<T, TM, true> ep;
  ep.fill_table(a, ktab, tid);
  if (pbn && tid < CIN) {
    const float r = a.pbn.rstd[tid], sc = a.pbn.gamma ? r * a.pbn.gamma[tid] : r;
    ptab[tid] = sc;
    ptab[32 + tid] = (a.pbn.beta ? a.pbn.beta[tid] : 0.f) - a.pbn.mean[tid] * sc;
  }
  lds_barrier();               // the tables are visible

  auto body = [&](int tile, auto curc) {
    constexpr int CUR = decltype(curc)::value;
    int n, y0, x0;
    decode(tile, n, y0, x0);
    // this tile's pieces (own) have landed; the previous tile's stores are out.  (The builtin, not inline asm: the compiler's
    // wait-count bookkeeping restarts from zero here instead of carrying the prologue's pending loads around the loop.)
    ScStageBn<T> sbn;
    if (pbn) sbn.load_tab(ptab, ptab + 32, (tid % VPP) * VEC);      // (table reads: requested before the wait)
    __builtin_amdgcn_s_waitcnt(0x0f70);                   // vmcnt(0)
    asm volatile("" ::: "memory");
    if (pbn) {
      // padding applies to the NORMALISED tensor: out-of-image vectors stay zero.  Reads in batches of three (one LDS round trip per
      // batch instead of one per vector).
#pragma unroll
      for (int p0 = 0; p0 < NPASS; p0 += 3) {
        u32x4 v[3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (p0 + q < NPASS) v[q] = *reinterpret_cast<const u32x4*>(smem + CUR * BUF + ((p0 + q) * 256 + tid) * 16);
#pragma unroll
        for (int q = 0; q < 3; ++q)
          if (p0 + q < NPASS && (inside_cur & (1u << (p0 + q))))
            *reinterpret_cast<u32x4*>(smem + CUR * BUF + ((p0 + q) * 256 + tid) * 16) = sbn.apply(v[q], a.pbn.relu);
      }
    }
    lds_barrier();
    ep.prefetch(a, n, y0, x0, wave, lr, lg);
    const int next = tile + t_step;
    inside_cur = issue_tile(next < t_end ? next : tile, CUR ^ 1, next < t_end);

    f32x4 acc[TM][4];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int f = 0; f < 4; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};
#if !defined(STP_SC_PLAIN_READS)
    if constexpr (SZ == 2) {
      // SC_RING reads are kept IN FLIGHT ahead of the MFMAs that consume them (a ring of register quads, refilled after every
      // MFMA) and released one by one with counted waits.  As plain C++ the compiler kept one or two reads in flight (register budget of 4 waves per SIMD)
      // and paired every ds_read_b128 with an lgkmcnt(0): 12-36 exposed LDS round trips per tile in every wave, the largest item
      // of the per-tile serial chain (what-if without the reads / MFMAs: -25..-40 %).  Inline asm, so the order is ours; a counted
      // wait only ever over-waits when the compiler adds LDS / scalar-memory operations of its own (they are older or younger than
      // the whole group it releases).  The fragment's tile row / column half and the buffer half are instruction offsets.
      constexpr bool PART = (K % KC) != 0;                 // last chunk: lane groups past K read address 0 and are zeroed below
      constexpr int R = 4 * NCH;                            // reads of a tile, fragment-major: k = f * NCH + c
      constexpr int D = SC_RING < R ? SC_RING : R;          // reads in flight (a ring of D register quads)
      u32x4 ring[D];
      (void)bla; (void)last_ok;
      auto issue = [&ring, &bla](auto kc) {
        constexpr int k = decltype(kc)::value, F = k / NCH, c = k % NCH;
        constexpr int OFF = CUR * BUF + ((F >> 1) * SC_HW + (F & 1) * 16) * PIXB;
        static_assert(OFF + 2 * SC_HW * PIXB < 65536, "ds_read offset field");
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ring[k % D]) : "v"(bla[c]), "n"(OFF));
      };
      sc_unroll<D>(issue);
      sc_unroll<R>([&ring, &fa, &acc, &issue, last_ok](auto kc) {
        constexpr int k = decltype(kc)::value, F = k / NCH, c = k % NCH;
        constexpr int young = (R - 1 - k) < (D - 1) ? (R - 1 - k) : (D - 1);      // reads issued after read k at this point
        asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(ring[k % D]) : "n"(young));
        u32x4 v = ring[k % D];
        if (PART && c == NCH - 1 && !last_ok) v = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < TM; ++i) ScMma<T>::run(fa[i][c], v, acc[i][F]);
        if constexpr (k + D < R) issue(std::integral_constant<int, k + D>{});
      });
    } else
#endif
    {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        u32x4 fb = {0u, 0u, 0u, 0u};
        // the fragment's tile row / column half and the buffer half are instruction offsets
#if !defined(STP_EXP) || STP_EXP != 13
        if (bl[c] != 0xffffffffu) fb = *reinterpret_cast<const u32x4*>(smem + bl[c] + (CUR * BUF + ((f >> 1) * SC_HW + (f & 1) * 16) * PIXB));
#pragma unroll
        for (int i = 0; i < TM; ++i) ScMma<T>::run(fa[i][c], fb, acc[i][f]);
#else
        if (a.N < 0) acc[0][f][0] += __uint_as_float(fa[0][c][0] + bl[c]);
#endif
      }
    }
    }
    ep.finish(a, acc, red, n, y0, x0, tile, ntiles, tid, wave, lr, lg);
  };

  ep.reset_stats();
  for (int tile = t_first; tile < t_end; tile += 2 * t_step) {
    body(tile, std::integral_constant<int, 0>{});
    if (tile + t_step < t_end) body(tile + t_step, std::integral_constant<int, 1>{});
  }
  ep.flush_stats(a, red, (int)blockIdx.x, (int)gridDim.x, tid, wave, lr, lg);
}

template <typename T, int CIN, int TM>
static int launch_sc(const ScArgs& a, hipStream_t s) {
  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  if (sc_stream_on()) {
    constexpr int NV = SC_HH * SC_HW * (CIN / Elem<T>::VEC), NPASS = (NV + 255) / 256;
    const size_t lds = (size_t)2 * NPASS * 4096 + (4 * TM * 16 * 2 + 128 + 64) * sizeof(float);
    const int blocks = sc_stream_blocks(Elem<T>::DTYPE, CIN, TM * 16, ntiles);      // a multiple of 8 on this machine: XCD-contiguous tile walk
    return stp_launch_lds(conv_sc_stream_kernel<T, CIN, TM>, dim3(blocks), dim3(256), lds, s, a);
  }
  const size_t lds = (size_t)SC_HH * SC_HW * CIN * sizeof(T) + 4 * TM * 16 * 2 * sizeof(float);
  hipLaunchKernelGGL((conv_sc_kernel<T, CIN, TM>), dim3(ntiles), dim3(256), lds, s, a);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// columns of the [stat][channel][column] partial sums this kernel writes for p (one per tile; one per workgroup in streaming form)
extern "C" int stp_conv2d_sc_stats_tiles(const stp_conv_params* p) {
  const int ntiles = p->N * ceil_div(p->Hv, SC_TH) * ceil_div(p->Wv, SC_TW);
  if (!sc_stream_on() || p->stats_slots) return ntiles;
  return sc_stream_blocks(p->dtype, p->C0, p->Cout <= 16 ? 16 : 32, ntiles);
}

template <typename T>
static int dispatch_sc(const ScArgs& a, int cin, hipStream_t s) {
  const int tm = a.Cout <= 16 ? 1 : 2;
  switch (cin * 4 + tm) {
    case 4 * 4 + 1: if constexpr (sizeof(T) == 4) return launch_sc<T, 4, 1>(a, s); else return STP_E_BADARG;
    case 4 * 4 + 2: if constexpr (sizeof(T) == 4) return launch_sc<T, 4, 2>(a, s); else return STP_E_BADARG;
    case 8 * 4 + 1: return launch_sc<T, 8, 1>(a, s);
    case 8 * 4 + 2: return launch_sc<T, 8, 2>(a, s);
    case 16 * 4 + 1: return launch_sc<T, 16, 1>(a, s);
    case 16 * 4 + 2: return launch_sc<T, 16, 2>(a, s);
    case 32 * 4 + 1: return launch_sc<T, 32, 1>(a, s);
    case 32 * 4 + 2: return launch_sc<T, 32, 2>(a, s);
    default: return STP_E_BADARG;
  }
}

// Is this convolution served by the small-channel kernel?  (stp_conv2d consults this before the GEMM path.)
extern "C" int stp_conv2d_sc_eligible(const stp_conv_params* p) {
  if (!p || !stp_dtype_ok(p->dtype)) return 0;
  const int vec = p->dtype == STP_H16 ? 8 : 4;
  const int cin = p->C0;
  // fp32 holds half as many k per 16-byte vector: cap Cin at 16 there so the A fragments stay in registers
  const bool cin_ok = p->dtype == STP_F32 ? (cin == 4 || cin == 8 || cin == 16) : (cin == 8 || cin == 16 || cin == 32);
  return p->KH == 3 && p->KW == 3 && p->stride == 1 && p->pad == 1 && p->C1 == 0 && cin_ok && (cin % vec) == 0 && p->Cout <= 32 &&
         p->Cd0 == p->Cout && !p->residual && p->Ho == p->Hv && p->Wo == p->Wv &&
         (p->src0_mode == STP_SRC_DIRECT || (p->src0_mode == STP_SRC_NEAREST2X && p->Hv == 2 * p->Hs0 && p->Wv == 2 * p->Ws0));
}

extern "C" int stp_conv2d_sc(const stp_conv_params* p, void* stream) {
  if (!stp_conv2d_sc_eligible(p) || !p->src0 || !p->weight || !p->dst0) return STP_E_BADARG;
  ScArgs a;
  a.src = (const char*)p->src0; a.weight = (const char*)p->weight; a.bias = p->bias; a.dst = (char*)p->dst0;
  a.N = p->N; a.H = p->Hv; a.W = p->Wv; a.Hs = p->Hs0; a.Ws = p->Ws0; a.Cout = p->Cout;
  a.up = p->src0_mode == STP_SRC_NEAREST2X; a.accumulate = p->accumulate0; a.relu = p->relu;
  {
    const uint64_t sb = (uint64_t)p->N * p->Hs0 * p->Ws0 * p->C0 * (p->dtype == STP_H16 ? 2 : 4);
    if (sb >= 0x80000000ull) return STP_E_BADARG;   // 32-bit LDS-DMA offsets
    a.src_bytes = (uint32_t)sb;
  }
  a.tiles_x = ceil_div(a.W, SC_TW); a.tiles_y = ceil_div(a.H, SC_TH);
  a.divTx = make_fastdiv((uint32_t)a.tiles_x); a.divTy = make_fastdiv((uint32_t)a.tiles_y);
  a.stats = p->stats_partial;
  a.stat_slots = p->stats_slots;
  if (a.stats && (p->Cout & 3)) return STP_E_BADARG;
  if (a.stat_slots && (!a.stats || (a.stat_slots & (a.stat_slots - 1)) || a.stat_slots > 64)) return STP_E_BADARG;
  a.bnb.x = (const char*)p->bnb_x; a.bnb.mean = p->bnb_mean; a.bnb.rstd = p->bnb_rstd; a.bnb.gamma = p->bnb_gamma;
  a.bnb.beta = p->bnb_beta; a.bnb.relu = p->bnb_relu;
  a.sum2 = p->dst_sum2x2;
  a.pbn.x = nullptr; a.pbn.mean = p->src_bn_mean; a.pbn.rstd = p->src_bn_rstd; a.pbn.gamma = p->src_bn_gamma; a.pbn.beta = p->src_bn_beta;
  a.pbn.relu = p->src_bn_relu;
  if (a.pbn.mean && !a.pbn.rstd) return STP_E_BADARG;
  if (a.bnb.x && (!a.stats || !a.bnb.mean || !a.bnb.rstd || p->relu)) return STP_E_BADARG;
  if (a.sum2 && ((p->Cout & 3) || (a.H & 1) || (a.W & 1) || p->bias || p->relu || (a.stats && !a.bnb.x))) return STP_E_BADARG;
  const_cast<stp_conv_params*>(p)->stats_tiles = stp_conv2d_sc_stats_tiles(p);
  hipStream_t s = (hipStream_t)stream;
  {
    const int r = sc_lean_launch(a, p->C0, p->dtype, s);      // the lean kernel (conv_sc_lean.hip) where it serves the configuration
    if (r != 1) return r;
  }
  return p->dtype == STP_H16 ? dispatch_sc<bf16_t>(a, p->C0, s) : dispatch_sc<float>(a, p->C0, s);
}
