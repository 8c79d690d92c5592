// Small-channel family (conv_sc.h): the wide-output data gradient, conv_scw_stream_kernel / stp_conv2d_scw*.
#include "conv_sc.h"

// =================================================================================================
// WIDE-OUTPUT form: data gradient of the first full-resolution decoder convolution,
//   conv3x3(concat(UpSampling2D(2)(x), skip)) -> 32 channels   (U-Net decoder_stage3_conv1 at 16 x 256 x 256)
// i.e. a 3x3 convolution of dY (32 channels) into 128 channels that belong to TWO tensors: the first Cd0 are the gradient of the
// upsampled tensor - its 2x2 blocks are summed here (dst_sum2x2) and land on the low-resolution gradient directly, optionally
// with the fused BatchNormalization-backward sums - the rest the gradient of the skip tensor.  The generic per-tap kernel spent
// 216 us on it (K = 32 per tap: a ring stage per MFMA step) and wrote a full-resolution gradient of the upsampled tensor that
// stp_upsample2x_bwd read back; the layer moves 67 MB in and 168 MB out, ~45 us at HBM speed.
// Same streaming scheme as conv_sc_stream_kernel (persistent workgroups, 8 x 32 tiles, the next tile's dY halo written into the
// other half of a double buffer by LDS-DMA); what differs is the split: the 4 waves share every B fragment (pixels) and own 32
// OUTPUT CHANNELS each (A fragments = 32 x 288 weights = 72 registers), a tile is walked in two passes of 4 rows (accumulators:
// 2 x 8 fragments).  Waves below Cd0 / 32 take the summed epilogue, the others store the skip gradient.
// =================================================================================================
struct ScwArgs {
  const char* src;      // dY [N,H,W,32]
  const char* weight;   // [128][9*32]  (the data-gradient weight copy: rows = input channels of the forward convolution)
  char* dst_up;         // [N,H/2,W/2,C0]
  char* dst_sk;         // [N,H,W,C1]
  int N, H, W, C0, C1, acc_up, acc_sk;
  int tiles_x, tiles_y;
  FastDiv divTx, divTy;
  float* stats;         // [2][C0][workgroups] (fused BatchNormalization-backward sums of the first C0 channels)
  BnBack bnb;
  uint32_t src_bytes, x_bytes;   // sizes of src and bnb.x (buffer descriptors of the LDS-DMA)
  uint32_t up_bytes, sk_bytes;   // sizes of dst_up and dst_sk (buffer descriptors of the stores)
};

template <typename T>
__global__ __launch_bounds__(256, 2) void conv_scw_stream_kernel(const ScwArgs a) {
  constexpr int CIN = 32, SZ = (int)sizeof(T), K = 9 * CIN, NCH = 9, VPP = 4, PIXB = CIN * SZ;
  constexpr int NV = SC_HH * SC_HW * VPP, NPASS = (NV + 255) / 256, BUF = NPASS * 4096;
  static_assert(SZ == 2, "16-bit storage");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* ktab = reinterpret_cast<float*>(smem + 2 * BUF);     // [4][128]: scale, shift, mean, rstd of the first C0 channels
  // [2][XBUF]: the BatchNormalization input of the tile's 4 x 16 low-resolution pixels ([pixel][C0]), staged by LDS-DMA with the
  // halo tile - a tile ahead of its use (fetched where it is used, each pass of the summed epilogue stalled on an HBM round trip:
  // 135 vs 86 us without the fused sums)
  constexpr int XBUF = 3 * 4096;
  char* const xlds = smem + 2 * BUF + 2048;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  // this wave's two 16-channel groups.  With as many summed as skip channels (the U-Net shape) every wave takes one group of each:
  // the summed epilogue carries the BatchNormalization-backward arithmetic, and two waves doing all of it while the other two
  // wait at the tile barrier cost 40 us of 125
  const int cbi[2] = {a.C0 == 64 ? wave * 16 : wave * 32, a.C0 == 64 ? 64 + wave * 16 : wave * 32 + 16};
  const bool upi[2] = {cbi[0] < a.C0, cbi[1] < a.C0};          // (wave-uniform) summed epilogue / skip epilogue

  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  int t_first, t_step, t_end;
  if ((gridDim.x & 7) == 0) {
    const int q = ntiles >> 3, r = ntiles & 7, x = blockIdx.x & 7;
    const int start = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    t_first = start + (int)(blockIdx.x >> 3); t_step = (int)(gridDim.x >> 3); t_end = start + q + (x < r ? 1 : 0);
  } else {
    t_first = (int)blockIdx.x; t_step = (int)gridDim.x; t_end = ntiles;
  }
  if (t_first >= t_end) {    // (no tile: its statistics column must still be defined)
    if (a.stats && tid < a.C0) {
      a.stats[(size_t)tid * gridDim.x + blockIdx.x] = 0.f;
      a.stats[((size_t)a.C0 + tid) * gridDim.x + blockIdx.x] = 0.f;
    }
    return;
  }

  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)a.src, 0, a.src_bytes, 0x00020000);
  const int H2 = a.H >> 1, W2 = a.W >> 1;
  const bool bnb = a.bnb.x != nullptr;
  const bool xrs_on = bnb;
  const __amdgpu_buffer_rsrc_t xrs = __builtin_amdgcn_make_buffer_rsrc((void*)(bnb ? a.bnb.x : a.src), 0, bnb ? a.x_bytes : 0u, 0x00020000);
  int hyx[NPASS];
  const int cvb = (tid % VPP) * 16;
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int v = p * 256 + tid, pix = v / VPP;
    const int hy = pix / SC_HW, hx = pix - hy * SC_HW;
    hyx[p] = v < NV ? (hy << 16 | hx) : -1;
  }
  int xq[3];                 // vector p * 256 + tid of the x tile: low-res row << 16 | column << 8 | 16-byte vector of the pixel; -1 past it
  {
    const int vpp = a.C0 >> 3;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const int v = p * 256 + tid, px = v / vpp;
      xq[p] = (xrs_on && px < 64) ? ((px >> 4) << 16 | (px & 15) << 8 | (v - px * vpp)) : -1;
    }
  }
  auto decode = [&](int tile, int& n, int& y0, int& x0) {
    const int bq = (int)fdiv((uint32_t)tile, a.divTx);
    const int tx = tile - bq * a.tiles_x;
    n = (int)fdiv((uint32_t)bq, a.divTy);
    const int ty = bq - n * a.tiles_y;
    y0 = ty * SC_TH; x0 = tx * SC_TW;
  };
  // (instruction count matters here: the waves of these streaming kernels spend as long in address arithmetic as in MFMAs.  A tile
  //  whose halo lies inside the image - all but the border tiles - takes its LDS-DMA offsets as (per-thread constant) + (tile base))
  uint32_t hrel[NPASS];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) hrel[p] = hyx[p] >= 0 ? (uint32_t)(((hyx[p] >> 16) * a.W + (hyx[p] & 0xffff)) * PIXB + cvb) : 0x80000000u;
  auto issue_tile = [&](int tile, int b) {
    int n, y0, x0;
    decode(tile, n, y0, x0);
    const bool inner = y0 >= 1 && x0 >= 1 && y0 + SC_TH + 1 <= a.H && x0 + SC_TW + 1 <= a.W;      // (uniform)
    const uint32_t tbase = (uint32_t)(((n * a.H + y0 - 1) * a.W + x0 - 1) * PIXB);
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      uint32_t off;
      if (inner) {
        off = hyx[p] >= 0 ? tbase + hrel[p] : 0x80000000u;
      } else {
        const int gy = y0 - 1 + (hyx[p] >> 16), gx = x0 - 1 + (hyx[p] & 0xffff);
        const bool ok = hyx[p] >= 0 && (unsigned)gy < (unsigned)a.H && (unsigned)gx < (unsigned)a.W;
        off = ok ? (uint32_t)((n * a.H + gy) * a.W + gx) * (uint32_t)PIXB + (uint32_t)cvb : 0x80000000u;
      }
#if !defined(STP_EXP) || STP_EXP != 32   // (what-if builds, scratch/sc_exp_build.sh: 31 = no output stores, 32 = no halo loads, 33 = no LDS reads / MFMAs)
      if (p * 256 + wave * 64 < NV)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(smem + b * BUF + p * 4096 + wave * 1024), 16, off, 0, 0, 0);
#endif
    }
    if (xrs_on) {
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        const int ly = (y0 >> 1) + (xq[p] >> 16), lx = (x0 >> 1) + ((xq[p] >> 8) & 0xff);
        const bool ok = xq[p] >= 0 && ly < H2 && lx < W2;
        const uint32_t off = ok ? (uint32_t)(((n * H2 + ly) * W2 + lx) * a.C0 + (xq[p] & 0xff) * 8) * 2u : 0x80000000u;
        if (p * 256 + wave * 64 < 8 * a.C0)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void*)(xlds + b * XBUF + p * 4096 + wave * 1024), 16, off, 0, 0, 0);
      }
    }
  };
  issue_tile(t_first, 0);

  // once per workgroup: this wave's weights -> registers; chunk c of K = tap c (32 channels: lane group lg holds channels 8 lg ..)
  u32x4 fa[2][NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i)
      fa[i][c] = *reinterpret_cast<const u32x4*>(a.weight + ((size_t)(cbi[i] + lr) * K + c * CIN + lg * 8) * SZ);
  const uint32_t lbase = (uint32_t)((lr * CIN + lg * 8) * SZ);     // lane part of every B-fragment address
  if (bnb && tid < 128) {
    float sc = 0.f, sh = 0.f, mu = 0.f, rsd = 0.f;
    if (tid < a.C0) {
      mu = a.bnb.mean[tid]; rsd = a.bnb.rstd[tid];
      sc = a.bnb.gamma ? rsd * a.bnb.gamma[tid] : rsd;
      sh = (a.bnb.beta ? a.bnb.beta[tid] : 0.f) - mu * sc;
    }
    ktab[tid] = sc; ktab[128 + tid] = sh; ktab[256 + tid] = mu; ktab[384 + tid] = rsd;
  }
  f32x2 ssp[2], qqp[2];        // fused sums of the lane's two channels (see the summed epilogue)
#pragma unroll
  for (int i = 0; i < 2; ++i) { ssp[i] = f32x2{0.f, 0.f}; qqp[i] = f32x2{0.f, 0.f}; }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the first tile's own pieces have landed
  lds_barrier();               // ... everybody's; the table is visible
  const __amdgpu_buffer_rsrc_t rup = __builtin_amdgcn_make_buffer_rsrc((void*)a.dst_up, 0, a.up_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsk = __builtin_amdgcn_make_buffer_rsrc((void*)a.dst_sk, 0, a.sk_bytes, 0x00020000);
  // per-lane byte offsets inside an output row segment (see the epilogues): summed half = low-resolution pixel lr / 2, channels
  // cbi + 4 lg + 2 (lr & 1); skip half = pixel lr, channels cbi - C0 + 4 lg
  uint32_t lup[2], lsk[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    lup[i] = (uint32_t)((lr >> 1) * a.C0 + cbi[i] + lg * 4 + 2 * (lr & 1)) * 2u;
    lsk[i] = (uint32_t)(lr * a.C1 + (cbi[i] - a.C0) + lg * 4) * 2u;
  }

  auto body = [&](int tile, auto curc) {
    constexpr int CUR = decltype(curc)::value;
    int n, y0, x0;
    decode(tile, n, y0, x0);
    // (this tile's halo is complete and visible, and every wave has left the other half: the wait + barrier at the end of the
    //  previous tile - there the wait sits BEFORE the last pass's stores, so it drains the stores of a pass ago instead of the
    //  ones just issued: at the top of the tile it exposed a store round trip per tile)
    const int next = tile + t_step;
    const bool full = y0 + SC_TH <= a.H && x0 + SC_TW <= a.W;      // (uniform) no pixel of the tile lies outside the image
    if (next < t_end) issue_tile(next, CUR ^ 1);

#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x4 acc[2][8];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int f = 0; f < 8; ++f) acc[i][f] = f32x4{0.f, 0.f, 0.f, 0.f};
      // a B fragment = 16 pixels of halo row r shifted by kw: it serves the taps (kh, kw) of the output rows r - kh, so each of the
      // 6 x 3 x 2 fragments of a pass is read ONCE and used by up to three output rows (36 LDS reads for 72 fragment uses).
      // Software pipeline, three reads ahead: left alone the compiler keeps ONE fragment register (ds_read -> lgkmcnt(0) -> 2-6
      // MFMAs: 36 exposed LDS latencies a pass); the scheduling barriers pin read s + 3 in front of the MFMAs of read s
      auto bfrag = [&](int sidx) -> u32x4 {
        const int r = sidx / 6, kw = (sidx >> 1) % 3, h2 = sidx & 1;
        return *reinterpret_cast<const u32x4*>(smem + lbase + (CUR * BUF + ((h * 4 + r) * SC_HW + h2 * 16 + kw) * PIXB));
      };
      u32x4 fbq[4];
#if defined(STP_EXP) && STP_EXP == 33
      if (a.N < 0) acc[0][0][0] += __uint_as_float(fa[0][h][0] + fa[1][h][1] + lbase);
#else
      fbq[0] = bfrag(0); fbq[1] = bfrag(1); fbq[2] = bfrag(2);
#pragma unroll
      for (int sidx = 0; sidx < 36; ++sidx) {
#if !defined(STP_EXP) || STP_EXP != 34
        __builtin_amdgcn_sched_barrier(0);
#endif
        if (sidx + 3 < 36) fbq[(sidx + 3) & 3] = bfrag(sidx + 3);
        const int r = sidx / 6, kw = (sidx >> 1) % 3, h2 = sidx & 1;
        const u32x4 fb = fbq[sidx & 3];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
          const int orow = r - kh;
          if (orow < 0 || orow > 3) continue;
          acc[0][orow * 2 + h2] = mfma16_16x16x32(fa[0][kh * 3 + kw], fb, acc[0][orow * 2 + h2]);
          acc[1][orow * 2 + h2] = mfma16_16x16x32(fa[1][kh * 3 + kw], fb, acc[1][orow * 2 + h2]);
        }
      }
#if !defined(STP_EXP) || STP_EXP != 34
      __builtin_amdgcn_sched_barrier(0);
#endif
#endif
      if (h == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next tile's own pieces have landed (issued two passes ago)
      auto epilogue = [&](auto fullc) {
        constexpr bool FULL = decltype(fullc)::value;      // no pixel of the tile lies outside the image: no per-lane bounds work
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        if (upi[i]) {
          // gradient of UpSampling2D(2): fragments f and f + 2 are the two rows of an output row, lanes lr and lr ^ 1 its columns.
          // After the quad_perm add both lanes of a pair hold the 4 channel sums: the even lane finishes channels 0, 1, the odd lane
          // channels 2, 3 (half the per-lane arithmetic of the fused BatchNormalization backward, 4-byte accesses, no idle lanes)
          const int par = lr & 1;
          const int co = cbi[i] + lg * 4 + 2 * par;
#pragma unroll
          for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
              asm volatile("" ::: "memory");       // (keeps the table / x reads of the iterations from being hoisted together: registers)
              const int gy = y0 + h * 4 + q * 2, gx = x0 + h2 * 16 + lr;
              f32x4 v = acc[i][q * 4 + h2] + acc[i][q * 4 + h2 + 2];
#pragma unroll
              for (int e = 0; e < 4; ++e)
                v[e] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[e]), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
              f32x2 v2 = par ? f32x2{v[2], v[3]} : f32x2{v[0], v[1]};
              // buffer addressing: (per-lane constant voffset) + (scalar soffset of the output row / column half) - no per-store VALU
              const uint32_t so = (uint32_t)(((n * H2 + (y0 >> 1) + h * 2 + q) * W2 + (x0 >> 1) + h2 * 8) * a.C0) * 2u;
              const uint32_t vo = (FULL || (gy < a.H && gx < a.W)) ? lup[i] : 0x80000000u;
              if (a.acc_up) {
                const uint32_t w0 = __builtin_amdgcn_raw_buffer_load_b32(rup, vo, so, 0);
                v2 += f32x2{h16lo_to_f32(w0), h16hi_to_f32(w0)};
              }
              uint32_t w = pack_bf16x2(v2.x, v2.y);
              if (bnb && (FULL || vo != 0x80000000u)) {
                const f32x2 ksc = *reinterpret_cast<const f32x2*>(ktab + co), ksh = *reinterpret_cast<const f32x2*>(ktab + 128 + co);
                const f32x2 kmu = *reinterpret_cast<const f32x2*>(ktab + 256 + co), krs = *reinterpret_cast<const f32x2*>(ktab + 384 + co);
                const uint32_t xw = *reinterpret_cast<const uint32_t*>(xlds + CUR * XBUF + (((h * 2 + q) * 16 + h2 * 8 + (lr >> 1)) * a.C0 + co) * 2);
                const f32x2 xv = {h16lo_to_f32(xw), h16hi_to_f32(xw)}, dy = {h16lo_to_f32(w), h16hi_to_f32(w)};     // dY as stored
                f32x2 g;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                  g[e] = bn_act_on(bn_affine(xv[e], ksc[e], ksh[e]), a.bnb.relu) ? dy[e] : 0.f;
                  ssp[i][e] += g[e];
                  qqp[i][e] += g[e] * ((xv[e] - kmu[e]) * krs[e]);
                }
                w = pack_bf16x2(g.x, g.y);
              }
#if defined(STP_EXP) && STP_EXP == 31
              if (a.N < 0)
#endif
              __builtin_amdgcn_raw_buffer_store_b32(w, rup, vo, so, 0);
            }
        } else {
#pragma unroll
          for (int f = 0; f < 8; ++f) {
            const int gy = y0 + h * 4 + (f >> 1), gx = x0 + (f & 1) * 16 + lr;
            const uint32_t so = (uint32_t)(((n * a.H + y0 + h * 4 + (f >> 1)) * a.W + x0 + (f & 1) * 16) * a.C1) * 2u;
            const uint32_t vo = (FULL || (gy < a.H && gx < a.W)) ? lsk[i] : 0x80000000u;
            f32x4 v = acc[i][f];
            if (a.acc_sk) {
              const u32x2 w0 = __builtin_amdgcn_raw_buffer_load_b64(rsk, vo, so, 0);
              v += f32x4{h16lo_to_f32(w0.x), h16hi_to_f32(w0.x), h16lo_to_f32(w0.y), h16hi_to_f32(w0.y)};
            }
#if defined(STP_EXP) && STP_EXP == 31
            if (a.N < 0)
#endif
            __builtin_amdgcn_raw_buffer_store_b64(u32x2{pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)}, rsk, vo, so, 0);
          }
        }
      }
      };
      if (full) epilogue(std::integral_constant<bool, true>{}); else epilogue(std::integral_constant<bool, false>{});
    }
    lds_barrier();        // the next tile is visible to everybody, and everybody has left this one
  };

  for (int tile = t_first; tile < t_end; tile += 2 * t_step) {
    body(tile, std::integral_constant<int, 0>{});
    if (tile + t_step < t_end) body(tile + t_step, std::integral_constant<int, 1>{});
  }
  // fused sums: one column per workgroup; a 16-channel group belongs to one wave outright (no cross-wave step).  Even lanes hold
  // the sums of channels 0, 1 of their 4-channel block, odd lanes of channels 2, 3: row_shr 2, 4, 8 leave them in lanes 14 and 15
  if (a.stats) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (!upi[i]) continue;
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        float sv = ssp[i][e], qv = qqp[i][e];
#pragma unroll
        for (int sh = 0; sh < 3; ++sh) {
          sv += __builtin_bit_cast(float, sh == 0 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sv), 0x112, 0xf, 0xf, true)
                                          : sh == 1 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sv), 0x114, 0xf, 0xf, true)
                                                    : __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, sv), 0x118, 0xf, 0xf, true));
          qv += __builtin_bit_cast(float, sh == 0 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, qv), 0x112, 0xf, 0xf, true)
                                          : sh == 1 ? __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, qv), 0x114, 0xf, 0xf, true)
                                                    : __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, qv), 0x118, 0xf, 0xf, true));
        }
        if (lr >= 14) {
          const int ch = cbi[i] + lg * 4 + 2 * (lr & 1) + e;
          a.stats[(size_t)ch * gridDim.x + blockIdx.x] = sv;
          a.stats[((size_t)a.C0 + ch) * gridDim.x + blockIdx.x] = qv;
        }
      }
    }
  }
}

static int scw_blocks(int ntiles) {
  const int64_t b = (int64_t)stp_cu_count() * 2;
  return (int)(b < ntiles ? b : ntiles);
}

// Is this convolution the two-destination data gradient served by conv_scw_stream_kernel?  (stp_conv2d consults this first.)
extern "C" int stp_conv2d_scw_eligible(const stp_conv_params* p) {
  static const bool on = !(getenv("STP_SCW") && atoi(getenv("STP_SCW")) == 0);
  if (!on || !p || p->dtype != STP_H16) return 0;
  return p->KH == 3 && p->KW == 3 && p->stride == 1 && p->pad == 1 && p->C0 == 32 && p->C1 == 0 && p->Cout == 128 && p->dst1 != nullptr &&
         p->Cd0 > 0 && p->Cd0 < 128 && (p->Cd0 % 32) == 0 && p->dst_sum2x2 == 1 && p->src0_mode == STP_SRC_DIRECT && p->Hs0 == p->Hv &&
         p->Ws0 == p->Wv && p->Ho == p->Hv && p->Wo == p->Wv && !(p->Ho & 1) && !(p->Wo & 1) && !p->bias && !p->relu && !p->residual &&
         !p->src_bn_mean && !p->stats_slots && !p->fold_src && !p->weight_up;
}
extern "C" int stp_conv2d_scw_stats_tiles(const stp_conv_params* p) {
  return scw_blocks(p->N * ceil_div(p->Hv, SC_TH) * ceil_div(p->Wv, SC_TW));
}

extern "C" int stp_conv2d_scw(const stp_conv_params* p, void* stream) {
  if (!stp_conv2d_scw_eligible(p) || !p->src0 || !p->weight || !p->dst0) return STP_E_BADARG;
  ScwArgs a;
  a.src = (const char*)p->src0; a.weight = (const char*)p->weight; a.dst_up = (char*)p->dst0; a.dst_sk = (char*)p->dst1;
  a.N = p->N; a.H = p->Hv; a.W = p->Wv; a.C0 = p->Cd0; a.C1 = p->Cout - p->Cd0; a.acc_up = p->accumulate0; a.acc_sk = p->accumulate1;
  {
    const uint64_t sb = (uint64_t)p->N * p->Hs0 * p->Ws0 * p->C0 * 2;
    if (sb >= 0x80000000ull) return STP_E_BADARG;   // 32-bit LDS-DMA offsets
    a.src_bytes = (uint32_t)sb;
    a.x_bytes = (uint32_t)((uint64_t)p->N * (p->Hv / 2) * (p->Wv / 2) * p->Cd0 * 2);    // (a quarter of the pixels, < 128 channels: smaller)
    a.up_bytes = a.x_bytes;
    const uint64_t kb = (uint64_t)p->N * p->Hv * p->Wv * (p->Cout - p->Cd0) * 2;
    if (kb >= 0x80000000ull) return STP_E_BADARG;
    a.sk_bytes = (uint32_t)kb;
  }
  a.tiles_x = ceil_div(a.W, SC_TW); a.tiles_y = ceil_div(a.H, SC_TH);
  a.divTx = make_fastdiv((uint32_t)a.tiles_x); a.divTy = make_fastdiv((uint32_t)a.tiles_y);
  a.stats = p->stats_partial;
  a.bnb.x = (const char*)p->bnb_x; a.bnb.mean = p->bnb_mean; a.bnb.rstd = p->bnb_rstd; a.bnb.gamma = p->bnb_gamma;
  a.bnb.beta = p->bnb_beta; a.bnb.relu = p->bnb_relu;
  if (a.bnb.x && (!a.stats || !a.bnb.mean || !a.bnb.rstd)) return STP_E_BADARG;
  if (a.stats && !a.bnb.x) return STP_E_BADARG;      // the only sums this kernel fuses are the BatchNormalization-backward ones
  const int ntiles = a.N * a.tiles_x * a.tiles_y;
  const int blocks = scw_blocks(ntiles);
  const_cast<stp_conv_params*>(p)->stats_tiles = blocks;
  constexpr int NPASS = (SC_HH * SC_HW * 4 + 255) / 256;
  constexpr size_t lds = (size_t)2 * NPASS * 4096 + 512 * sizeof(float) + 2 * 3 * 4096;
  static_assert(lds > STP_LDS_DEFAULT, "every launch of this kernel needs the grant");
  return stp_launch_lds(conv_scw_stream_kernel<bf16_t>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, a);
}
