// The multi-class head's confusion matrix: counts[t][p] = pixels of target class t whose predicted class is p, the predicted class being
// the FIRST index of the row maximum of the stored values (K.argmax / numpy.argmax; logits or DeepLab's probabilities alike).
// categorical_accuracy and the per-class / mean IoU of an epoch are ratios of sums of these integers (backend.confusion_metrics).
//   stp_class_confusion     rows [pixels][ldc] at the mask's resolution
//   stp_class_confusion_ignore  the same with an ignore label: pixels whose target holds it are not counted
//   stp_class_confusion_up  logits held at 1 / f of it (where stp_softmax_cce_dice_up removed the resized tensor from the step): every output
//                           pixel is interpolated with the expression of resize_bilinear_kernel (resize.hip) and rounded to the storage
//                           type as that kernel's store rounds it - the counts are those of stp_resize_bilinear + stp_class_confusion.
// One thread per pixel; a workgroup (1024 threads, so that few tables leave the chip) keeps the classes^2 table in LDS.  Masks are
// piecewise constant: the 64 pixels of a wave mostly share one (target, predicted) key, so a wave first peels off up to CONF_PEEL distinct
// keys with one LDS add of a popcount each, and only lanes whose key is still unserved add on their own.  Workgroup tables go to the
// workspace, a finalize launch sums them: integer sums, so neither form depends on an order and graph replay is bit-identical.
#include "loss_reduce.h"
#include "softmax_row.h"
#include "wave_count.h"      // wave_count(): the peel of up to WAVE_COUNT_PEEL (the CONF_PEEL of the comment above) keys

#define CONF_THREADS 1024
#define CONF_MAX_BLOCKS 512          // two workgroups per CU; stp_class_confusion_workspace_bytes() covers 512 tables

template <int CM>
__device__ __forceinline__ int first_argmax(const float (&p)[CM], int classes) {
  float best = p[0];
  int idx = 0;
#pragma unroll
  for (int c = 1; c < CM; ++c) {
    const bool up = c < classes && p[c] > best;      // (false for NaN on either side: the index stays in [0, classes))
    best = up ? p[c] : best;
    idx = up ? c : idx;
  }
  return idx;
}

// the workgroup's table (THREADS = its size): zeroed before the first pixel, written to its slot of the workspace after the last
template <int THREADS> __device__ __forceinline__ void conf_table_clear(int* table, int entries) {
  for (int e = threadIdx.x; e < entries; e += THREADS) table[e] = 0;
  __syncthreads();
}
template <int THREADS> __device__ __forceinline__ void conf_table_store(const int* table, int entries, int* partial) {
  __syncthreads();
  for (int e = threadIdx.x; e < entries; e += THREADS) partial[(size_t)blockIdx.x * entries + e] = table[e];
}

// IGNORE (stp_class_confusion_ignore): a pixel whose stored target equals ignore_label keeps key -1 - its row is not loaded, it joins no
// key group of the ballot peel and adds nothing, so the table's total is the number of counted pixels.  The other instance never
// looks at the argument.
template <typename T, int CM, bool IGNORE>
__global__ __launch_bounds__(CONF_THREADS) void class_confusion_kernel(const T* __restrict__ rows, const uint8_t* __restrict__ target,
                                                                       int64_t pixels, int classes, int ldc, int ignore_label,
                                                                       int* __restrict__ partial) {
  __shared__ int table[STP_MAX_CLASSES * STP_MAX_CLASSES];
  conf_table_clear<CONF_THREADS>(table, classes * classes);
  const RowAccess ra = row_access<T, CM>(rows, ldc);
  // (the trip count is the same in every lane of a wave: wave_count is called by all 64)
  for (int64_t base = (int64_t)blockIdx.x * CONF_THREADS; base < pixels; base += (int64_t)gridDim.x * CONF_THREADS) {
    const int64_t i = base + threadIdx.x;
    int key = -1;
    if (i < pixels) {
      const int tr = target[i];
      if (!IGNORE || tr != ignore_label) {
        float p[CM];
        class_row_load<T, CM>(rows + i * ldc, classes, ra.vec, p, ra.vec4);
        const int t = tr < classes ? tr : classes - 1;
        key = t * classes + first_argmax<CM>(p, classes);
      }
    }
    wave_count(table, key);
  }
  conf_table_store<CONF_THREADS>(table, classes * classes, partial);
}

template <typename T> __device__ __forceinline__ float round_to_storage(float v) {
  if constexpr (sizeof(T) == 2) return bf16_to_f32(f32_to_bf16(v));      // (Elem<T>::store and load)
  else return v;
}

// one thread per (low-resolution cell (n, y0, x0), row jy of the cell): its f output pixels (y0 f + jy, x0 f + jx) share the four corner rows
template <typename T, int CM>
__global__ __launch_bounds__(256) void class_confusion_up_kernel(const T* __restrict__ low, const uint8_t* __restrict__ target, uint32_t items,
                                                                 const UpGeo g, int classes, int ldc, int* __restrict__ partial) {
  __shared__ int table[STP_MAX_CLASSES * STP_MAX_CLASSES];
  conf_table_clear<256>(table, classes * classes);
  const int f = 1 << g.lf;
  const float inv = 1.f / (float)f;
  const RowAccess ra = row_access<T, CM>(low, ldc);
  for (uint32_t base = blockIdx.x * 256u; base < items; base += gridDim.x * 256u) {
    const uint32_t it = base + threadIdx.x;
    const bool on = it < items;
    float v00[CM], v01[CM], v10[CM], v11[CM];
    const uint8_t* trow = target;
    float fy = 0.f;
    if (on) {
      const UpCell u = up_cell_decode(it, g, f);
      fy = (float)u.jy * inv;
      const T* b = low + (int64_t)u.n * g.H * g.W * ldc;
      class_row_load<T, CM>(b + ((int64_t)u.y0 * g.W + u.x0) * ldc, classes, ra.vec, v00, ra.vec4);
      class_row_load<T, CM>(b + ((int64_t)u.y0 * g.W + u.x1) * ldc, classes, ra.vec, v01, ra.vec4);
      class_row_load<T, CM>(b + ((int64_t)u.y1 * g.W + u.x0) * ldc, classes, ra.vec, v10, ra.vec4);
      class_row_load<T, CM>(b + ((int64_t)u.y1 * g.W + u.x1) * ldc, classes, ra.vec, v11, ra.vec4);
      trow = up_cell_target_row(target, u, g, f);
    }
    for (int jx = 0; jx < f; ++jx) {
      int key = -1;
      if (on) {
        const float fx = (float)jx * inv;
        float p[CM];
#pragma unroll
        for (int c = 0; c < CM; ++c) {
          // resize_bilinear_kernel's statements (TF's lerp order); each one source expression, as the build contracts within one
          const float top = v00[c] + (v01[c] - v00[c]) * fx, bot = v10[c] + (v11[c] - v10[c]) * fx;
          p[c] = round_to_storage<T>(top + (bot - top) * fy);
        }
        const int t = trow[jx] < classes ? trow[jx] : classes - 1;
        key = t * classes + first_argmax<CM>(p, classes);
      }
      wave_count(table, key);
    }
  }
  conf_table_store<256>(table, classes * classes, partial);
}

// counts[e] = sum over the workgroup tables; thread (slice = tid / 16, e = tid % 16) of workgroup b adds tables slice, slice + 16, ... of
// entry 16 b + e, the 16 slices meet in LDS
__global__ __launch_bounds__(256) void class_confusion_finalize_kernel(const int* __restrict__ partial, int blocks, int entries,
                                                                       int* __restrict__ counts) {
  __shared__ int sh[16][16];
  const int e = blockIdx.x * 16 + (threadIdx.x & 15), slice = threadIdx.x >> 4;
  int a = 0;
  if (e < entries) {
#pragma unroll 8
    for (int b = slice; b < blocks; b += 16) a += partial[(size_t)b * entries + e];
  }
  sh[slice][threadIdx.x & 15] = a;
  __syncthreads();
  if (threadIdx.x < 16 && e < entries) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += sh[k][threadIdx.x];
    counts[e] = s;
  }
}

static inline size_t conf_workspace_bytes(int classes) { return (size_t)CONF_MAX_BLOCKS * classes * classes * sizeof(int); }

extern "C" size_t stp_class_confusion_workspace_bytes(int32_t classes) {
  if (classes < 2 || classes > STP_MAX_CLASSES) return 0;
  return conf_workspace_bytes(classes);
}

static inline void conf_finalize(const int* partial, int blocks, int classes, int32_t* counts, hipStream_t s) {
  const int entries = classes * classes;
  hipLaunchKernelGGL(class_confusion_finalize_kernel, dim3((entries + 15) / 16), dim3(256), 0, s, partial, blocks, entries, counts);
}

// both full-resolution entry points: stp_class_confusion passes ignore_label -1
template <bool IGNORE>
static int conf_entry(const void* rows, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype, int32_t* counts,
                      void* workspace, size_t workspace_bytes, int32_t ignore_label, void* stream) {
  const int rc = loss_check(dtype, rows && target && counts && workspace && pixels > 0 && pixels < (1ll << 31) && classes >= 2 &&
                                       classes <= STP_MAX_CLASSES && ldc >= classes && ignore_label >= -1 && ignore_label <= 255,
                            workspace_bytes, classes >= 2 && classes <= STP_MAX_CLASSES ? conf_workspace_bytes(classes) : 0);
  if (rc != STP_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int64_t want = (pixels + CONF_THREADS - 1) / CONF_THREADS;
  const int blocks = (int)(want > CONF_MAX_BLOCKS ? CONF_MAX_BLOCKS : want);
  int* partial = (int*)workspace;
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    loss_by_class_bucket(classes, [&](auto bucket) {
      constexpr int CM = decltype(bucket)::value;
      hipLaunchKernelGGL((class_confusion_kernel<T, CM, IGNORE>), dim3(blocks), dim3(CONF_THREADS), 0, s, (const T*)rows, target, pixels, classes, ldc,
                         ignore_label, partial);
    });
  });
  conf_finalize(partial, blocks, classes, counts, s);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_class_confusion(const void* rows, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                                   int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  return conf_entry<false>(rows, target, pixels, classes, ldc, dtype, counts, workspace, workspace_bytes, -1, stream);
}

extern "C" int stp_class_confusion_ignore(const void* rows, const uint8_t* target, int64_t pixels, int32_t classes, int32_t ldc, int32_t dtype,
                                          int32_t* counts, void* workspace, size_t workspace_bytes, int32_t ignore_label, void* stream) {
  return conf_entry<true>(rows, target, pixels, classes, ldc, dtype, counts, workspace, workspace_bytes, ignore_label, stream);
}

extern "C" int stp_class_confusion_up_ok(int32_t factor, int32_t classes, int32_t dtype) {
  return stp_dtype_ok(dtype) && (factor == 2 || factor == 4 || factor == 8 || factor == 16) && classes >= 2 && classes <= STP_MAX_CLASSES;
}

extern "C" int stp_class_confusion_up(const void* low, const uint8_t* target, int32_t N, int32_t H, int32_t W, int32_t factor, int32_t classes,
                                      int32_t ldc, int32_t dtype, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  if (!stp_dtype_ok(dtype)) return STP_E_BADARG;      // (the other build's 16-bit code, or garbage)
  if (!low || !target || !counts || !workspace || N <= 0 || H <= 0 || W <= 0 || classes < 2 || classes > STP_MAX_CLASSES || ldc < classes)
    return STP_E_BADARG;
  if (factor != 2 && factor != 4 && factor != 8 && factor != 16) return STP_E_BADARG;
  // pixels < 2^31 (the work items, pixels / factor, are indexed in 32 bits); factor by factor, so that no product leaves 64 bits
  const int64_t lim = 1ll << 31, cells_nh = (int64_t)N * H;
  if (cells_nh >= lim || cells_nh * W >= lim || cells_nh * W * factor * factor >= lim) return STP_E_BADARG;
  if (workspace_bytes < conf_workspace_bytes(classes)) return STP_E_WORKSPACE;
  const int lf = factor == 2 ? 1 : factor == 4 ? 2 : factor == 8 ? 3 : 4;
  hipStream_t s = (hipStream_t)stream;
  const UpGeo g = make_upgeo(H, W, lf);
  const int64_t items = ((int64_t)N * H * W) << lf;
  const int blocks = loss_grad_blocks(items, CONF_MAX_BLOCKS);
  int* partial = (int*)workspace;
  loss_by_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    loss_by_class_bucket(classes, [&](auto bucket) {
      constexpr int CM = decltype(bucket)::value;
      hipLaunchKernelGGL((class_confusion_up_kernel<T, CM>), dim3(blocks), dim3(256), 0, s, (const T*)low, target, (uint32_t)items, g, classes, ldc, partial);
    });
  });
  conf_finalize(partial, blocks, classes, counts, s);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
