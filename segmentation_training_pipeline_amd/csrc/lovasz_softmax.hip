// lovasz_softmax of the loss registry: the Lovasz-Softmax of Berman et al. on the multi-class softmax head, batch form (per_image=False,
// classes='present'); include/stp_hip.h fixes the arithmetic (stp_lovasz_softmax).  For every class c, over the counted pixels of the batch:
//   e_ic = y_ic ? 1 - p_ic : p_ic;  sort descending (ties: ascending pixel);  loss_c = sum_r e_(r) g_r  with the closed-form g_r of
//   lovasz.hip (positive at rank r: 1 / (G + c0_r); negative: (G - c1_r) / ((G + c0_r - 1) (G + c0_r)));  mean over the present classes.
// The gradient treats g as a constant: d_ic = -+ g_rank(i,c) / P, dz_ik = p_ik (d_ik - sum_c p_ic d_ic).
//
// Device path (nothing allocates or synchronises; every launch captures into a hipGraph):
//   1. key pass      one softmax per pixel row -> `classes` (key, value) pairs: key = class << 30 | (bits(1.f) - bits(e)) - e lies in [0, 1],
//                    so its bits are < 2^30 and ascending keys are descending errors inside a class; an ignored pixel's keys take the
//                    sentinel class `classes` and sort behind everything; value = pixel << 1 | y.  The counted pixels n are counted here
//                    (one integer atomicAdd per workgroup): every class segment of the sorted array has exactly n elements, segment c
//                    starts at c n.
//   2. sort          ONE chip-wide stable radix sort over 30 + ceil(log2(classes + 1)) bits (rocPRIM through hipCUB, double-buffered pairs
//                    and temporary storage from the caller's workspace).
//   3. scan          (a) a grid of (chunk, class) workgroups counts the positives of its chunk of STP_LOVASZ_SOFTMAX_CHUNK ranks;
//                    (b) the same grid sums the counts before its chunk (integers) and of the whole class (G_c), scans the chunk, leaves
//                    sum e g in one partial per workgroup and scatters -+ g into the fp32 coefficient buffer (zero-filled first; it lives
//                    in the pair buffer the sort left free).  The buffer is held as [classes][pixels] planes: the workgroups that run
//                    together belong to one class, so their scattered 4-byte writes fall into one plane (19 MB at 8 x 768 x 768) that
//                    stays in cache until its lines are whole - measured 1.61 ms against 2.36 ms for [pixels][classes] rows at 20
//                    classes - and the gradient pass reads a plane with consecutive lanes on consecutive words.
//                    The launch boundary is the only synchronisation.
//   4. finalize      one workgroup: per class the partials in a fixed order in double, P = classes with G_c > 0, scalars[14] and [0].
//   5. gradient pass per counted pixel row: softmax again, the pixel's coefficients, P from the device, dlogits += weight grad_scale dz
//                    (the add happens in the storage type, as stp_lovasz_hinge does it).
#include <hipcub/hipcub.hpp>

#include "loss_reduce.h"
#include "softmax_row.h"

namespace {

#define LVS_T 1024
#define LVS_CHUNK STP_LOVASZ_SOFTMAX_CHUNK
#define LVS_ERR_BITS 30
#define LVS_ONE 0x3F800000u        // bits of 1.f: < 2^30
#define LVS_META_WORDS 64          // [0] counted pixels n  [1] present classes P  [2 + c] positives G_c
static_assert(LVS_CHUNK % LVS_T == 0, "a chunk is a whole number of workgroup-wide steps");
static_assert(2 + STP_MAX_CLASSES <= LVS_META_WORDS, "the class table fits the meta words");

__global__ __launch_bounds__(256) void lvs_zero_kernel(uint4* p, int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = uint4{0u, 0u, 0u, 0u};
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the workgroup (NW waves), valid in every thread; `sh` may be reused after the call
template <int NW>
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t* sh) {
  v = wave_sum_u32(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < NW; ++i) s += sh[i];
  __syncthreads();
  return s;
}

template <typename T, int CM>
__global__ __launch_bounds__(256) void lvs_keys_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target, int64_t pixels, int classes,
                                                       int ldc, int ignore_label, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                       uint32_t* meta) {
  __shared__ uint32_t sh[4];
  const RowAccess ra = row_access<T, CM>(logits, ldc);
  uint32_t counted = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    const int ts = target[i];
    const bool on = ts != ignore_label;
    float p[CM];
    softmax_row<T, CM>(logits + i * ldc, classes, ra.vec, p, ra.vec4);
    const int t = ts < classes ? ts : classes - 1;
    uint64_t* k = keys + i * classes;
    uint32_t* v = vals + i * classes;
    const uint64_t cls_off = on ? 0u : (uint64_t)classes;        // an ignored pixel: the sentinel class in every key
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      if (c < classes) {
        const uint32_t y = (on && c == t) ? 1u : 0u;
        float e = y ? 1.f - p[c] : p[c];
        e = e > 0.f ? fminf(e, 1.f) : 0.f;                       // [+0, 1]: the bits are ordered and < 2^30 (NaN, -0 -> 0)
        k[c] = ((on ? (uint64_t)c : cls_off) << LVS_ERR_BITS) | (uint64_t)(LVS_ONE - __float_as_uint(e));
        v[c] = ((uint32_t)i << 1) | y;
      }
    }
    counted += on ? 1u : 0u;
  }
  counted = block_sum_u32<4>(counted, sh);
  if (threadIdx.x == 0 && counted) atomicAdd(meta, counted);
}

// (a) positives of chunk blockIdx.x of class blockIdx.y (0 for a chunk past the n counted pixels)
__global__ __launch_bounds__(LVS_T) void lvs_count_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ meta, int nchunks,
                                                          uint32_t* __restrict__ pos_partial) {
  __shared__ uint32_t sh[LVS_T / 64];
  const int64_t n = meta[0], r0 = (int64_t)blockIdx.x * LVS_CHUNK;
  const int c = blockIdx.y;
  uint32_t s = 0;
  if (r0 < n) {
    const uint32_t* v = vals + (int64_t)c * n + r0;
    const int m = (int)(n - r0 < LVS_CHUNK ? n - r0 : LVS_CHUNK);
    for (int j = threadIdx.x; j < m; j += LVS_T) s += v[j] & 1u;
  }
  s = block_sum_u32<LVS_T / 64>(s, sh);
  if (threadIdx.x == 0) pos_partial[(size_t)c * nchunks + blockIdx.x] = s;
}

// (b) the chunk's ranks: g_r from the integer counts, sum e g into loss_partial[class][chunk], -+ g into coef[class][pixel] (coef may be NULL)
__global__ __launch_bounds__(LVS_T) void lvs_scan_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ meta, const uint32_t* __restrict__ pos_partial, int nchunks,
                                                         int classes, int64_t pixels, float* __restrict__ coef, float* __restrict__ loss_partial) {
  __shared__ uint32_t sh[LVS_T / 64];
  __shared__ float fsum[LVS_T / 64];
  const int64_t n = meta[0], r0 = (int64_t)blockIdx.x * LVS_CHUNK;
  if (r0 >= n) return;                                           // (uniform: the chunk lies past the class segment)
  const int c = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int nvalid = (int)((n + LVS_CHUNK - 1) / LVS_CHUNK);
  uint32_t before = 0, all = 0;
  for (int j = t; j < nvalid; j += LVS_T) {
    const uint32_t v = pos_partial[(size_t)c * nchunks + j];
    all += v;
    before += j < chunk ? v : 0u;
  }
  before = block_sum_u32<LVS_T / 64>(before, sh);
  const uint32_t G = block_sum_u32<LVS_T / 64>(all, sh);
  if (G == 0) {                                                  // (uniform) the class is absent: no term, no gradient
    if (t == 0) loss_partial[(size_t)c * nchunks + chunk] = 0.f;
    return;
  }
  const float Gf = (float)G;
  const uint64_t* k = keys + (int64_t)c * n;
  const uint32_t* v = vals + (int64_t)c * n;
  uint32_t carry = before;
  float acc = 0.f;
  for (int it = 0; it < LVS_CHUNK / LVS_T; ++it) {
    const int64_t r = r0 + it * LVS_T + t;
    const bool live = r < n;
    const uint32_t val = live ? v[r] : 0u;
    const uint32_t y = val & 1u;
    uint32_t s = y;                                              // inclusive scan of y: wave scan + wave totals
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(s, o, 64);
      if (lane >= o) s += u;
    }
    if (lane == 63) sh[w] = s;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < LVS_T / 64; ++i) {
      base += i < w ? sh[i] : 0u;
      tot += sh[i];
    }
    __syncthreads();
    const uint32_t c1 = carry + base + s;                        // positives among ranks 0..r
    carry += tot;
    if (live) {
      const float c0 = (float)((uint32_t)(r + 1) - c1);          // negatives among ranks 0..r
      const float den = Gf + c0;
      const float gr = y ? 1.f / den : (Gf - (float)c1) / ((den - 1.f) * den);
      const float e = __uint_as_float(LVS_ONE - (uint32_t)(k[r] & ((1u << LVS_ERR_BITS) - 1u)));
      acc += e * gr;
      const int64_t pix = val >> 1;
      if (coef && pix < pixels) coef[(int64_t)c * pixels + pix] = y ? -gr : gr;
    }
  }
  acc = wave_sum(acc);                                           // fixed-order workgroup sum
  if (lane == 0) fsum[w] = acc;
  __syncthreads();
  if (t == 0) {
    float s = 0.f;
    for (int i = 0; i < LVS_T / 64; ++i) s += fsum[i];
    loss_partial[(size_t)c * nchunks + chunk] = s;
  }
}

// scalars[14] = lovasz_softmax, scalars[0] += weight * lovasz_softmax; meta[1] = P, meta[2 + c] = G_c
__global__ __launch_bounds__(256) void lvs_finalize_kernel(const uint32_t* __restrict__ pos_partial, const float* __restrict__ loss_partial, int nchunks,
                                                           int classes, float weight, uint32_t* meta, float* scalars) {
  __shared__ double shd[256];
  __shared__ uint32_t shg[256];
  const int t = threadIdx.x;
  const int64_t n = meta[0];
  const int nvalid = (int)((n + LVS_CHUNK - 1) / LVS_CHUNK);
  double total = 0.0;
  uint32_t present = 0;
  for (int c = 0; c < classes; ++c) {
    double a = 0.0;
    uint32_t g = 0;
    for (int j = t; j < nvalid; j += 256) {
      g += pos_partial[(size_t)c * nchunks + j];
      a += (double)loss_partial[(size_t)c * nchunks + j];
    }
    shd[t] = a;
    shg[t] = g;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (t < h) {
        shd[t] += shd[t + h];
        shg[t] += shg[t + h];
      }
      __syncthreads();
    }
    if (t == 0) {
      meta[2 + c] = shg[0];
      if (shg[0] > 0) {
        total += shd[0];
        ++present;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const float l = present ? (float)(total / (double)present) : 0.f;
    meta[1] = present;
    scalars[14] = l;
    scalars[0] = __fadd_rn(scalars[0], __fmul_rn(weight, l));      // (two roundings: the sum grows by exactly weight * scalars[14])
  }
}

template <typename T, int CM>
__global__ __launch_bounds__(256) void lvs_grad_kernel(const T* __restrict__ logits, const uint8_t* __restrict__ target, int64_t pixels, int classes,
                                                       int ldc, int ignore_label, const float* __restrict__ coef, const uint32_t* __restrict__ meta,
                                                       float scale, T* __restrict__ dl, int dlc) {
  const uint32_t present = meta[1];
  if (present == 0) return;                                       // nothing counted: the gradient stays as it is
  const float ks = scale / (float)present;
  const RowAccess ra = row_access<T, CM>(logits, ldc);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * 256) {
    if ((int)target[i] == ignore_label) continue;                 // the row of an ignored pixel stays exactly 0
    float p[CM];
    softmax_row<T, CM>(logits + i * ldc, classes, ra.vec, p, ra.vec4);
    float dd[CM], sum = 0.f;
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      dd[c] = c < classes ? coef[(int64_t)c * pixels + i] : 0.f;      // (a class plane: consecutive lanes, consecutive words)
      sum += p[c] * dd[c];
    }
    T* o = dl + i * dlc;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < classes) Elem<T>::store(o + c, Elem<T>::load(o + c) + ks * (p[c] * (dd[c] - sum)));
  }
}

struct LvsLayout { size_t keys0, keys1, vals0, vals1, pos_partial, loss_partial, meta, temp, temp_bytes, total; int nchunks, end_bit; };

static int lvs_end_bit(int classes) {
  int b = 0;
  while ((1 << b) < classes + 1) ++b;      // the classes and the sentinel
  return LVS_ERR_BITS + b;
}

static int lvs_layout(int64_t pixels, int classes, LvsLayout* L) {
  const int64_t count = pixels * classes;
  L->end_bit = lvs_end_bit(classes);
  L->nchunks = (int)((pixels + LVS_CHUNK - 1) / LVS_CHUNK);
  size_t temp = 0;
  hipcub::DoubleBuffer<uint64_t> dk((uint64_t*)nullptr, (uint64_t*)nullptr);
  hipcub::DoubleBuffer<uint32_t> dv((uint32_t*)nullptr, (uint32_t*)nullptr);
  if (hipcub::DeviceRadixSort::SortPairs(nullptr, temp, dk, dv, (int)count, 0, L->end_bit, (hipStream_t)0) != hipSuccess) return STP_E_LAUNCH;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t o = 0;
  L->keys0 = o; o += up((size_t)count * 8);
  L->keys1 = o; o += up((size_t)count * 8);
  L->vals0 = o; o += up((size_t)count * 4);
  L->vals1 = o; o += up((size_t)count * 4);
  L->pos_partial = o; o += up((size_t)classes * L->nchunks * 4);
  L->loss_partial = o; o += up((size_t)classes * L->nchunks * 4);
  L->meta = o; o += up(LVS_META_WORDS * 4);
  L->temp = o; L->temp_bytes = temp; o += up(temp);
  L->total = o;
  return STP_OK;
}

static bool lvs_shape_ok(int64_t pixels, int classes) {
  return pixels > 0 && classes >= 2 && classes <= STP_MAX_CLASSES && pixels * classes < ((int64_t)1 << 31);
}

}  // namespace

extern "C" size_t stp_lovasz_softmax_workspace_bytes(int64_t pixels, int32_t classes) {
  LvsLayout L;
  if (!lvs_shape_ok(pixels, classes) || lvs_layout(pixels, classes, &L) != STP_OK) return 0;
  return L.total;
}

extern "C" int stp_lovasz_softmax(const void* logits, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                                  float weight, float* scalars, void* dlogits, int32_t dl_channels, float grad_scale, int32_t ignore_label,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!logits || !target || !scalars || !workspace || !lvs_shape_ok(pixels, classes) || ldc < classes || (dlogits && dl_channels < classes) ||
      ignore_label < -1 || ignore_label > 255 || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return STP_E_BADARG;
  LvsLayout L;
  if (lvs_layout(pixels, classes, &L) != STP_OK) return STP_E_LAUNCH;
  if (workspace_bytes < L.total) return STP_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int64_t count = pixels * classes;
  uint32_t* meta = (uint32_t*)(ws + L.meta);
  uint32_t* pos_partial = (uint32_t*)(ws + L.pos_partial);
  float* loss_partial = (float*)(ws + L.loss_partial);
  hipcub::DoubleBuffer<uint64_t> dk((uint64_t*)(ws + L.keys0), (uint64_t*)(ws + L.keys1));
  hipcub::DoubleBuffer<uint32_t> dv((uint32_t*)(ws + L.vals0), (uint32_t*)(ws + L.vals1));
  hipLaunchKernelGGL(lvs_zero_kernel, dim3(1), dim3(256), 0, s, (uint4*)meta, (int64_t)(LVS_META_WORDS * 4 / 16));
  const int gk = loss_grad_blocks(pixels, 8192);
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    loss_by_class_bucket(classes, [&](auto bucket) {
      constexpr int CM = decltype(bucket)::value;
      hipLaunchKernelGGL((lvs_keys_kernel<T, CM>), dim3(gk), dim3(256), 0, s, (const T*)logits, target, pixels, classes, ldc, ignore_label,
                         dk.Current(), dv.Current(), meta);
    });
  });
  STP_LAUNCH_CHECK();
  size_t temp = L.temp_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(ws + L.temp, temp, dk, dv, (int)count, 0, L.end_bit, s) != hipSuccess) return STP_E_LAUNCH;
  const uint64_t* keys = dk.Current();
  const uint32_t* vals = dv.Current();
  // the key buffer the sort left free (8 bytes per pair) holds the 4-byte coefficients
  float* coef = dlogits ? (float*)dk.Alternate() : nullptr;
  if (coef) {
    const int64_t n16 = (count * 4 + 15) / 16;
    hipLaunchKernelGGL(lvs_zero_kernel, dim3(loss_grad_blocks(n16, 8192)), dim3(256), 0, s, (uint4*)coef, n16);
  }
  const dim3 grid((unsigned)L.nchunks, (unsigned)classes);
  hipLaunchKernelGGL(lvs_count_kernel, grid, dim3(LVS_T), 0, s, vals, meta, L.nchunks, pos_partial);
  hipLaunchKernelGGL(lvs_scan_kernel, grid, dim3(LVS_T), 0, s, keys, vals, meta, pos_partial, L.nchunks, classes, pixels, coef, loss_partial);
  hipLaunchKernelGGL(lvs_finalize_kernel, dim3(1), dim3(256), 0, s, pos_partial, loss_partial, L.nchunks, classes, weight, meta, scalars);
  STP_LAUNCH_CHECK();
  if (dlogits) {
    const int gg = loss_grad_blocks(pixels, 8192);
    loss_by_dtype(dtype, [&](auto tag) {
      using T = decltype(tag);
      loss_by_class_bucket(classes, [&](auto bucket) {
        constexpr int CM = decltype(bucket)::value;
        hipLaunchKernelGGL((lvs_grad_kernel<T, CM>), dim3(gg), dim3(256), 0, s, (const T*)logits, target, pixels, classes, ldc, ignore_label, coef,
                           meta, weight * grad_scale, (T*)dlogits, dl_channels);
      });
    });
    STP_LAUNCH_CHECK();
  }
  return STP_OK;
}
