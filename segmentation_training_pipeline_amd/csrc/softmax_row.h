// Class rows of the multi-class (softmax) head held in registers: shared by the loss kernels of loss_optim.hip and loss_softmax_ex.hip.
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
