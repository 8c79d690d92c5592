// Class rows of the multi-class (softmax) head held in registers: the row load, the per-pixel sums of the value passes and the padded
// gradient row store, shared by the loss kernels of loss_softmax.hip and loss_softmax_ex.hip and the confusion kernels of class_confusion.hip.
#pragma once
#include "common.h"

#define STP_MAX_CLASSES 32

// Rows are held in registers: the class loops are unrolled to a compile-time bound CM (4, 8, 16, 24 or 32 >= classes) and
// predicated, rows whose stride allows it are read / written as 16-byte vectors.
template <typename T, int CM>
__device__ __forceinline__ void class_row_load(const T* z, int classes, bool vec, float (&p)[CM], bool vec4 = false) {
  constexpr int V = Elem<T>::VEC;
  if (vec) {
#pragma unroll
    for (int v = 0; v < CM / V; ++v) {
      if (v * V < classes) {
        const u32x4 r = *reinterpret_cast<const u32x4*>(z + v * V);
        if constexpr (sizeof(T) == 2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { p[v * V + 2 * e] = h16lo_to_f32(r[e]); p[v * V + 2 * e + 1] = h16hi_to_f32(r[e]); }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) p[v * V + e] = __uint_as_float(r[e]);
        }
      }
    }
  } else if (sizeof(T) == 2 && vec4) {
    // 16-bit rows whose stride is a multiple of 4 elements only (PSPNet's 20 classes: 40-byte rows): 8-byte loads instead of 20 scalar ones
#pragma unroll
    for (int v = 0; v < CM / 4; ++v) {
      if (v * 4 < classes) {
        const u32x2 r = *reinterpret_cast<const u32x2*>(z + v * 4);
        p[v * 4] = h16lo_to_f32(r.x); p[v * 4 + 1] = h16hi_to_f32(r.x); p[v * 4 + 2] = h16lo_to_f32(r.y); p[v * 4 + 3] = h16hi_to_f32(r.y);
      }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c) p[c] = c < classes ? p[c] : 0.f;
  } else {
#pragma unroll
    for (int c = 0; c < CM; ++c) p[c] = c < classes ? Elem<T>::load(z + c) : 0.f;
  }
}
// The row access a KERNEL picks for class_row_load from the stride alone (the entry points that promise no base alignment): 16-byte
// vectors when the stride and the class bucket are whole vectors, else 8-byte loads for 16-bit rows of 4 k elements on an 8-byte base.
// (stp_softmax_loss_ex / _masked decide on the host, where the base's 16-byte alignment is tested too: smx_launch.)
struct RowAccess { bool vec, vec4; };
template <typename T, int CM>
__device__ __forceinline__ RowAccess row_access(const T* base, int ldc) {
  RowAccess r;
  r.vec = (ldc % Elem<T>::VEC) == 0 && CM % Elem<T>::VEC == 0;
  r.vec4 = !r.vec && sizeof(T) == 2 && (ldc % 4) == 0 && (CM % 4) == 0 && !(reinterpret_cast<uintptr_t>(base) & 7);
  return r;
}
// logits in p[0 .. classes) -> probabilities (p[c] = 0 beyond `classes`)
template <int CM>
__device__ __forceinline__ void softmax_probs(float (&p)[CM], int classes) {
  float m = -3.4e38f;
#pragma unroll
  for (int c = 0; c < CM; ++c) if (c < classes) m = fmaxf(m, p[c]);
  float sum = 0.f;
#pragma unroll
  // (v_exp_f32 behind __expf: the library expf is ~20 instructions per class and pixel in a kernel that is VALU-bound - 95 + 128 us for
  //  PSPNet's 20 classes at 8 x 768 x 768 against a 38 us memory floor per pass; each probability moves by <= 3e-7 relative, the tests hold
  //  the loss to 1e-5 and the logits' gradient to the format's rounding)
  for (int c = 0; c < CM; ++c) { p[c] = c < classes ? __expf(p[c] - m) : 0.f; sum += p[c]; }
  const float inv = 1.f / sum;
#pragma unroll
  for (int c = 0; c < CM; ++c) p[c] *= inv;
}
template <typename T, int CM>
__device__ __forceinline__ void softmax_row(const T* z, int classes, bool vec, float (&p)[CM], bool vec4 = false) {
  class_row_load<T, CM>(z, classes, vec, p, vec4);
  softmax_probs<CM>(p, classes);
}

// The per-class sums of the one-hot target in closed form (a loop over the classes cost ~12 instructions per class and pixel - the value
// passes are VALU-bound: 137 us per pass for PSPNet's 20 classes against a 38 us memory floor): sum_c y_c = 1, sum_c p_c y_c = p_t, at most
// ONE class passes the 0.5 threshold (the probabilities sum to 1), so sum_c th_c = [pmax > 0.5], sum_c th_c y_c = [p_t > 0.5] and the count
// of th_c == y_c is classes - (p_t > 0.5 ? 0 : 1 + [pmax > 0.5]).  The counts are the same integers; sum_c p_c is added per pixel.
// softmax_row_stats: p_t, max_c p_c and sum_c p_c of a row of probabilities.
template <int CM>
__device__ __forceinline__ void softmax_row_stats(const float (&p)[CM], int t, float& pt, float& pmax, float& psum) {
  pt = 0.f; pmax = 0.f; psum = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    pt = c == t ? p[c] : pt;
    pmax = fmaxf(pmax, p[c]);                      // (p[c] = 0 beyond `classes`)
    psum += p[c];
  }
}
// one pixel into the sums 0 cce_pixel  2 y (= 1 per pixel)  3 p_t  4 [pmax>.5]  5 [p_t>.5]  6 count of th == y.  Sum 1 (+= sum_c p_c) stays
// with the caller: the fused form adds a product there, which contracts to one fma only while it is one expression.
template <int N>
__device__ __forceinline__ void softmax_pixel_sums(float (&a)[N], float pt, float pmax, int classes) {
  const float tt = pt > 0.5f ? 1.f : 0.f, tm = pmax > 0.5f ? 1.f : 0.f;
  a[2] += 1.f;
  a[3] += pt;
  a[4] += tm;
  a[5] += tt;
  a[6] += (float)classes - (pt > 0.5f ? 0.f : 1.f + tm);
  // Keras: p <- p / sum(p) (a no-op on a softmax up to rounding), clip to [eps, 1-eps], -sum(y log p)
  a[0] += -__logf(fminf(fmaxf(pt, 1e-7f), 1.f - 1e-7f));
}

// One row of the padded gradient tensor: g[0 .. classes) into o[0 .. dlc), zeros behind.  vout: dlc is a multiple of 16 bytes and the
// rows are 16-byte aligned - whole vectors (up to the 32 channels of the widest class bucket unrolled, zero vectors beyond).  WIDE: also
// rows wider than any class bucket (stp_softmax_loss_ex).  No plan makes such rows (gradient rows are the class count padded to 16
// bytes, <= 32 channels), but the loop is not free: with it stp_softmax_cce_dice's gradient kernel takes 2 - 15 more vector registers
// and loses a wave per SIMD at 24 classes, so that kernel compiles it out and leaves channels from 32 on as it always did.
template <typename T, int CM, bool WIDE>
__device__ __forceinline__ void softmax_grad_row_store(T* o, const float (&g)[CM], int classes, int dlc, bool vout) {
  constexpr int V = Elem<T>::VEC;
  if (vout) {
#pragma unroll
    for (int v = 0; v < 32 / V; ++v) {
      if (v * V >= dlc) break;
      u32x4 r = {0u, 0u, 0u, 0u};
      auto gv = [&](int idx) { return idx < CM ? g[idx % CM] : 0.f; };      // channels past the class bucket are padding
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = pack_bf16x2(gv(v * V + 2 * e), gv(v * V + 2 * e + 1));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = __float_as_uint(gv(v * V + e));
      }
      *reinterpret_cast<u32x4*>(o + v * V) = r;
    }
    if constexpr (WIDE)
      for (int c = 32; c < dlc; c += V) *reinterpret_cast<u32x4*>(o + c) = u32x4{0u, 0u, 0u, 0u};
  } else {
#pragma unroll
    for (int c = 0; c < CM; ++c) if (c < classes) Elem<T>::store(o + c, g[c]);
    for (int c = classes; c < dlc; ++c) Elem<T>::store(o + c, 0.f);
  }
}

// ---- class rows held at 1 / f of the mask's resolution (f = 2^lf; stp_softmax_cce_dice_up, stp_class_confusion_up): one work item per
// (low-resolution cell (n, y0, x0), row jy of the cell) - its f output pixels (y0 f + jy, x0 f + jx) share the cell's four corner rows
// (y0, x0), (y0, x1), (y1, x0), (y1, x1), x1 = min(x0 + 1, W - 1), y1 likewise.  Integer arithmetic only: each kernel interpolates in
// its own order.
struct UpGeo { int H, W, lf; FastDiv divW, divH; };
static inline UpGeo make_upgeo(int H, int W, int lf) {
  UpGeo g;
  g.H = H; g.W = W; g.lf = lf; g.divW = make_fastdiv((uint32_t)W); g.divH = make_fastdiv((uint32_t)H);
  return g;
}
struct UpCell {
  int jy, y0, x0, x1, y1;
  uint32_t cell, n;
};
// (f = 1 << g.lf, which every caller holds already)
__device__ __forceinline__ UpCell up_cell_decode(uint32_t item, const UpGeo& g, int f) {
  UpCell u;
  u.jy = (int)(item & (uint32_t)(f - 1));
  u.cell = item >> g.lf;
  const uint32_t r = fdiv(u.cell, g.divW);
  u.x0 = (int)(u.cell - r * (uint32_t)g.W);
  u.n = fdiv(r, g.divH);
  u.y0 = (int)(r - u.n * (uint32_t)g.H);
  u.x1 = min(u.x0 + 1, g.W - 1);
  u.y1 = min(u.y0 + 1, g.H - 1);
  return u;
}
// the f target bytes of the item's row
__device__ __forceinline__ const uint8_t* up_cell_target_row(const uint8_t* target, const UpCell& u, const UpGeo& g, int f) {
  return target + (((int64_t)u.n * g.H + u.y0) * f + u.jy) * ((int64_t)g.W * f) + (int64_t)u.x0 * f;
}

// ---- the extended terms (loss_softmax_ex.hip)
#define SMX_JACCARD_SMOOTH 100.f
#define SMX_FOCAL_ALPHA 0.25f

// 1 - p_c without cancellation: at most one probability of a row exceeds 0.5 - for the largest one (index *imax) 1 - p is the sum of
// the OTHERS (returned), for every other class 1 - p_c >= 0.5 is exact enough as written.  A confidently wrong pixel (a class that is not
// the target at p -> 1) is where focal_loss is largest: log(1 - p) and 1 / (1 - p) of a rounded 1.f - p lose 1e-7 / (1 - p) there.
template <int CM>
__device__ __forceinline__ float smx_rest(const float (&p)[CM], int* imax) {
  float pmax = p[0], rest = 0.f;
  int im = 0;
#pragma unroll
  for (int c = 1; c < CM; ++c) {
    const bool gt = p[c] > pmax;
    pmax = gt ? p[c] : pmax;
    im = gt ? c : im;
  }
#pragma unroll
  for (int c = 0; c < CM; ++c) rest += c == im ? 0.f : p[c];                 // (p[c] = 0 beyond `classes`)
  *imax = im;
  return rest;
}
