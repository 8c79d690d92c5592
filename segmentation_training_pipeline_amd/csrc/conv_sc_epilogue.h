// Device templates of the small-channel kernels that more than one translation unit uses: the stored-value rounding (sc_stored), the
// MFMA step per storage type (ScMma), and the epilogue of the generic forward kernels (ScEpilogue with its ScRaw4 operands).
// Users: conv_sc.hip (all of it), conv_sc_stem.hip (sc_stored, ScMma).
#pragma once
#include "conv_sc.h"

__device__ __forceinline__ f32x4 sc_stored(f32x4 v, const float*) { return v; }
__device__ __forceinline__ f32x4 sc_stored(f32x4 v, const bf16_t*) {
  const uint32_t a = pack_bf16x2(v.x, v.y), b = pack_bf16x2(v.z, v.w);
  return f32x4{h16lo_to_f32(a), h16hi_to_f32(a), h16lo_to_f32(b), h16hi_to_f32(b)};
}

template <typename T> struct ScMma;
template <> struct ScMma<bf16_t> {
  __device__ static __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
    c = mfma16_16x16x32(a, b, c);
  }
};
template <> struct ScMma<float> {
  __device__ static __forceinline__ void run(const u32x4& a, const u32x4& b, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
  }
};

// 4 channels as fetched (8 bytes of bf16 stay packed until they are used: prefetched epilogue operands cost half the registers)
template <typename T> struct ScRaw4;
template <> struct ScRaw4<float> {
  f32x4 v;
  __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const f32x4*>(p); }
  __device__ __forceinline__ f32x4 get() const { return v; }
};
template <> struct ScRaw4<bf16_t> {
  u32x2 v;
  __device__ __forceinline__ void load(const bf16_t* p) { v = *reinterpret_cast<const u32x2*>(p); }
  __device__ __forceinline__ f32x4 get() const {
    return f32x4{h16lo_to_f32(v.x), h16hi_to_f32(v.x), h16lo_to_f32(v.y), h16hi_to_f32(v.y)};
  }
};


// Epilogue of the small-channel kernels, shared by the single-shot and the streaming form.  prefetch() issues the global
// operands of the fused BatchNormalization backward (the BN input x of every output this lane owns: clamped addresses, no
// control flow between the loads, one latency) - the streaming kernel calls it BEFORE it starts the next tile's LDS-DMA, so
// the vmcnt wait that releases these registers does not also wait for that tile; finish() does the arithmetic and the stores.
// LDSK: the per-channel constants of the fused BatchNormalization backward live in an LDS table [4][32] (scale, shift, mean,
// rstd; filled once per persistent workgroup) and are read where they are used instead of occupying 16 registers per 16 channels.
template <typename T, int TM, bool LDSK = false>
struct ScEpilogue {
  ScRaw4<T> xpre[TM][4];
  BnBackCh bks[LDSK ? 1 : TM];
  const float* ktab;
  // LDSK (persistent workgroup): the fused sums run over ALL tiles of the workgroup in these registers and are reduced once
  // (flush_stats) into column `workgroup` of [stat][channel][workgroups]; the slot form still adds per tile
  f32x4 ssp[LDSK ? TM : 1], qqp[LDSK ? TM : 1];
  // LDSK: the bias of the lane's channels, fetched ONCE per persistent workgroup (fill_table) - as a global load in finish() it was a
  // memory round trip (and a vmcnt(0), which also waits for the next tile's LDS-DMA) per tile
  f32x4 biasr[LDSK ? TM : 1];
  __device__ __forceinline__ void reset_stats() {
#pragma unroll
    for (int i = 0; i < (LDSK ? TM : 1); ++i) { ssp[i] = f32x4{0.f, 0.f, 0.f, 0.f}; qqp[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }

  __device__ __forceinline__ void load_constants(const ScArgs& a, int lg) {
    if (a.bnb.x) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        if (i * 16 + lg * 4 < a.Cout) bks[i] = bnback_load(a.bnb, i * 16 + lg * 4);
    }
  }
  // (all 256 threads) fill the LDS table; the caller's next barrier publishes it
  __device__ __forceinline__ void fill_table(const ScArgs& a, float* tab, int tid) {
    ktab = tab;
    if constexpr (LDSK) {
      const int lg = (tid & 63) >> 4;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = i * 16 + lg * 4 + r;
          biasr[i][r] = (a.bias && co < a.Cout) ? a.bias[co] : 0.f;
        }
    }
    if (a.bnb.x && tid < 32) {
      float sc = 0.f, sh = 0.f, mu = 0.f, rs = 0.f;
      if (tid < a.Cout) {
        mu = a.bnb.mean[tid]; rs = a.bnb.rstd[tid];
        sc = a.bnb.gamma ? rs * a.bnb.gamma[tid] : rs;
        sh = (a.bnb.beta ? a.bnb.beta[tid] : 0.f) - mu * sc;
      }
      tab[tid] = sc; tab[32 + tid] = sh; tab[64 + tid] = mu; tab[96 + tid] = rs;
    }
  }
  __device__ __forceinline__ BnBackCh bk(int i, int lg) const {
    if constexpr (LDSK) {
      // Inline asm: a ds_read the compiler knows about, issued while the next tile's LDS-DMA is in flight, gets an s_waitcnt vmcnt(0)
      // in front of it (the wait-count pass assumes the two may alias) - that put the whole DMA latency into every tile's epilogue.
      BnBackCh k;
      const uint32_t ad = (uint32_t)(uintptr_t)ktab + (uint32_t)(i * 16 + lg * 4) * 4u;
      asm volatile("ds_read_b128 %0, %1" : "=v"(k.sc) : "v"(ad));
      asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(k.sh) : "v"(ad));
      asm volatile("ds_read_b128 %0, %1 offset:256" : "=v"(k.mu) : "v"(ad));
      asm volatile("ds_read_b128 %0, %1 offset:384" : "=v"(k.rs) : "v"(ad));
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(k.sc), "+v"(k.sh), "+v"(k.mu), "+v"(k.rs));
      return k;
    } else {
      return bks[i];
    }
  }

  __device__ __forceinline__ void prefetch(const ScArgs& a, int n, int y0, int x0, int wave, int lr, int lg) {
    if (!a.bnb.x) return;
    if (a.sum2) {
      const int H2 = a.H >> 1, W2 = a.W >> 1;
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int gy = y0 + wave * 2, gx = x0 + h2 * 16 + lr;
        const size_t pm = ((size_t)n * H2 + (gy >> 1)) * W2 + (gx >> 1);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int co = i * 16 + lg * 4;
          const bool ok = !(lr & 1) && gy < a.H && gx < a.W && co < a.Cout;
          xpre[i][h2].load(reinterpret_cast<const T*>(a.bnb.x) + (ok ? pm * a.Cout + co : (size_t)0));
        }
      }
    } else {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int gy = y0 + wave * 2 + (f >> 1), gx = x0 + (f & 1) * 16 + lr;
        const size_t pm = ((size_t)n * a.H + gy) * a.W + gx;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int co = i * 16 + lg * 4;
          const bool ok = gy < a.H && gx < a.W && co + 3 < a.Cout;
          xpre[i][f].load(reinterpret_cast<const T*>(a.bnb.x) + (ok ? pm * a.Cout + co : (size_t)0));
        }
      }
    }
  }

  // tile / ntiles: column of this tile in the [stat][channel][tile] partial sums
  __device__ __forceinline__ void finish(const ScArgs& a, f32x4 (&acc)[TM][4], float* red, int n, int y0, int x0, int tile, int ntiles, int tid,
                                         int wave, int lr, int lg) {
    T* out = reinterpret_cast<T*>(a.dst);
    f32x4 ss[TM], qq[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) { ss[i] = f32x4{0.f, 0.f, 0.f, 0.f}; qq[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (a.sum2) {
      // gradient of UpSampling2D(2): the wave's two tile rows are one output row (fragments f and f+2, same lane), lanes
      // lr and lr^1 one output column (quad_perm DPP); even lanes own the low-resolution pixel
      const int H2 = a.H >> 1, W2 = a.W >> 1;
#pragma unroll
      for (int h2 = 0; h2 < 2; ++h2) {
        const int gy = y0 + wave * 2, gx = x0 + h2 * 16 + lr;
        const bool own = !(lr & 1) && gy < a.H && gx < a.W;
        const size_t pm = ((size_t)n * H2 + (gy >> 1)) * W2 + (gx >> 1);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int co = i * 16 + lg * 4;
          f32x4 v = acc[i][h2] + acc[i][h2 + 2];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            v[e] += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v[e]), 0xB1, 0xf, 0xf, true));  // quad_perm [1,0,3,2]
          if (!own || co >= a.Cout) continue;
          T* d = out + pm * a.Cout + co;
          if (a.accumulate) v += load4(d);
          if (a.bnb.x) v = bnback_apply(bk(i, lg), a.bnb.relu, xpre[i][h2].get(), sc_stored(v, (const T*)nullptr), ss[i], qq[i]);
#if defined(STP_EXP) && STP_EXP == 11
          if (a.N < 0)
#endif
          store4(d, v);
        }
      }
    } else {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const int gy = y0 + wave * 2 + (f >> 1), gx = x0 + (f & 1) * 16 + lr;
        if (gy >= a.H || gx >= a.W) continue;
        const size_t pm = ((size_t)n * a.H + gy) * a.W + gx;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int co = i * 16 + lg * 4;
          if (co >= a.Cout) continue;
          f32x4 v = acc[i][f];
          if (co + 3 < a.Cout) {
            if (a.bias) {
              if constexpr (LDSK) v += biasr[i]; else v += *reinterpret_cast<const f32x4*>(a.bias + co);
            }
            T* d = out + pm * a.Cout + co;
            if (a.accumulate) v += load4(d);
            if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if (a.bnb.x) v = bnback_apply(bk(i, lg), a.bnb.relu, xpre[i][f].get(), sc_stored(v, (const T*)nullptr), ss[i], qq[i]);
#if defined(STP_EXP) && STP_EXP == 11
            if (a.N < 0)
#endif
            store4(d, v);
            if (a.stats && !a.bnb.x) {
              const f32x4 sv = sc_stored(v, (const T*)nullptr);
              ss[i] += sv;
              qq[i] += sv * sv;
            }
          } else {
            for (int r = 0; r < 4 && co + r < a.Cout; ++r) {
              float x = v[r];
              if (a.bias) {
                if constexpr (LDSK) x += biasr[i][r]; else x += a.bias[co + r];
              }
              T* d = out + pm * a.Cout + co + r;
              if (a.accumulate) x += Elem<T>::load(d);
              if (a.relu) x = fmaxf(x, 0.f);
#if defined(STP_EXP) && STP_EXP == 11
              if (a.N < 0)
#endif
              Elem<T>::store(d, x);
            }
          }
        }
      }
    }
    if constexpr (LDSK) {
      if (a.stats && !a.stat_slots) {     // keep summing; flush_stats() reduces once per workgroup
#pragma unroll
        for (int i = 0; i < TM; ++i) { ssp[i] += ss[i]; qqp[i] += qq[i]; }
        return;
      }
    }
    reduce_stats(a, ss, qq, red, tile, ntiles, tid, wave, lr, lg);
  }

  __device__ __forceinline__ void flush_stats(const ScArgs& a, float* red, int column, int columns, int tid, int wave, int lr, int lg) {
    if constexpr (LDSK) {
      if (a.stats && !a.stat_slots) reduce_stats(a, ssp, qqp, red, column, columns, tid, wave, lr, lg);
    }
  }

  template <int NS>
  __device__ __forceinline__ void reduce_stats(const ScArgs& a, f32x4 (&ss)[NS], f32x4 (&qq)[NS], float* red, int tile, int ntiles, int tid,
                                               int wave, int lr, int lg) {
    if (a.stats) {
      // butterfly over the 16 pixel lanes, then the 4 waves (same channels, different rows) through LDS
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float sv = row_sum16_to_lane15(ss[i][e]), qv = row_sum16_to_lane15(qq[i][e]);
          if (lr == 15) {
            const int cl = i * 16 + lg * 4 + e;
            red[(wave * TM * 16 + cl) * 2] = sv;
            red[(wave * TM * 16 + cl) * 2 + 1] = qv;
          }
        }
      lds_barrier();
      if (tid < TM * 16 && tid < a.Cout) {
        float sv = 0.f, qv = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) { sv += red[(w * TM * 16 + tid) * 2]; qv += red[(w * TM * 16 + tid) * 2 + 1]; }
        if (a.stat_slots) {
          long long* sl = reinterpret_cast<long long*>(a.stats);
          slot_add(sl, a.stat_slots, tid, tile, sv);
          slot_add(sl, a.stat_slots, a.Cout + tid, tile, qv);
        } else {
          a.stats[(size_t)tid * ntiles + tile] = sv;                     // [stat][channel][tile]
          a.stats[((size_t)a.Cout + tid) * ntiles + tile] = qv;
        }
      }
    }
  }
};
