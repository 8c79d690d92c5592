// Object-level matching of two label images on the device (segmentation_pipeline/segmentation.py: score_objects, find_object_threshold,
// object_overlaps): the counters behind the per-object scores of the Airbus ship and DSB-2018 competitions - a predicted object is a true
// positive at t when its IoU with a ground-truth object exceeds t.  int32 and int64 only; every result is exact integer work, equals its
// host statement (tests/_object_match_reference.py) and is the same from run to run: all that workgroups exchange are integer sums.
// h * w < 2^31 (a pixel count is an int32); slot and pixel indices are int64.
//
// No workgroup waits for another: what a launch needs from other workgroups was written by an earlier launch on the same stream.
//   om_clear_kernel     zeroes the workspace (both area arrays, the table) and the counters
//   om_count_kernel     a wave owns 64 consecutive pixels of a row.  A stretch of lanes with one value adds its length once, from its
//                       first lane: into area_p[pred], into area_g[truth] and - both non-zero - into the pair's slot of an open-addressing
//                       table keyed by (pred << 32) | truth (0: empty).  The slot is claimed with a 64-bit atomicCAS, whose RETURN value
//                       decides (empty or this key: add the length; another key: the next slot) - no plain read of the table exists in
//                       this launch.  The table has a power of two >= 2 * h * w slots and at most h * w distinct keys (every pair owns a
//                       pixel): the load stays <= 1/2, so a probe sequence meets an empty slot and ends.
//   om_finalize_kernel  (stp_label_match) one thread per slot: I, U = A_p + A_g - I and the number m of thresholds the pair exceeds (they
//                       ascend, so those are the first m); a workgroup's histogram of m in LDS, its suffix sums added to out[k].  The
//                       first label_cap threads also count the labels with a non-zero area.
//   om_emit_kernel      (stp_label_overlaps) one thread per slot: a wave reserves room for its occupied slots with one atomicAdd and
//                       writes their (a, b, I); the first label_cap + 1 threads copy the areas out.
#include "common.h"

#define OM_THREADS 256
#define OM_MAX_T 64
#define OM_MAX_DEN 1000

struct OmThresholds {
  int num[OM_MAX_T];
};

typedef unsigned long long om_u64;

__global__ __launch_bounds__(OM_THREADS) void om_clear_kernel(om_u64* __restrict__ ws, int64_t words, int64_t* __restrict__ out, int n_out,
                                                              int* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * OM_THREADS + threadIdx.x;
  if (i < words) ws[i] = 0ull;
  if (out && i < n_out) out[i] = 0;
  if (count && i == 0) *count = 0;
}

// the lanes of a wave hold consecutive pixels: `first` = this lane starts a stretch of equal keys, `len` = that stretch's length
__device__ __forceinline__ void om_stretch(long long key, int lane, bool& first, int& len) {
  const long long prev = __shfl_up(key, 1);
  first = lane == 0 || prev != key;
  const om_u64 firsts = __ballot(first);
  const om_u64 next = lane == 63 ? 0ull : firsts >> (lane + 1);
  len = next ? __ffsll((long long)next) : 64 - lane;
}

__global__ __launch_bounds__(OM_THREADS) void om_count_kernel(const int* __restrict__ pred, const int* __restrict__ truth, int h, int w, int segs,
                                                              int label_cap, int* __restrict__ area_p, int* __restrict__ area_g, om_u64* keys,
                                                              int* counts, int64_t slots, int shift, om_u64* __restrict__ out_of_range) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (OM_THREADS / 64) + (threadIdx.x >> 6);
  if (item >= (int64_t)h * segs) return;      // (the same in every lane of a wave: the ballots are called by all 64)
  const int y = (int)(item / segs), seg = (int)(item - (int64_t)y * segs);
  const int x = seg * 64 + lane;
  int p = 0, g = 0;
  bool outside = false;
  if (x < w) {
    const int64_t i = (int64_t)y * w + x;
    p = pred[i];
    g = truth[i];
    if ((unsigned)p > (unsigned)label_cap) p = 0, outside = true;      // (a negative value too) background, and never an index
    if ((unsigned)g > (unsigned)label_cap) g = 0, outside = true;
  }
  const om_u64 outs = __ballot(outside);
  if (outs && lane == 0) atomicAdd(out_of_range, (om_u64)__popcll(outs));
  bool first;
  int len;
  om_stretch(p, lane, first, len);
  if (first && p > 0) atomicAdd(area_p + p, len);
  om_stretch(g, lane, first, len);
  if (first && g > 0) atomicAdd(area_g + g, len);
  const om_u64 key = (p > 0 && g > 0) ? ((om_u64)(unsigned)p << 32) | (om_u64)(unsigned)g : 0ull;
  om_stretch((long long)key, lane, first, len);
  if (first && key) {
    int64_t s = (int64_t)((key * 0x9E3779B97F4A7C15ull) >> shift);      // the top log2(slots) bits of the product
    for (int64_t probe = 0; probe < slots; ++probe) {                   // (ends long before: at most half of the slots are taken)
      const om_u64 old = atomicCAS(keys + s, 0ull, key);
      if (old == 0ull || old == key) {
        atomicAdd(counts + s, len);
        break;
      }
      s = (s + 1) & (slots - 1);
    }
  }
}

__global__ __launch_bounds__(OM_THREADS) void om_finalize_kernel(const om_u64* __restrict__ keys, const int* __restrict__ counts, int64_t slots,
                                                                 const int* __restrict__ area_p, const int* __restrict__ area_g, int label_cap,
                                                                 OmThresholds thr, int T, int den, om_u64* __restrict__ out) {
  __shared__ int hist[OM_MAX_T + 1];
  const int64_t i = (int64_t)blockIdx.x * OM_THREADS + threadIdx.x;
  if (threadIdx.x <= OM_MAX_T) hist[threadIdx.x] = 0;
  __syncthreads();
  const om_u64 key = i < slots ? keys[i] : 0ull;
  if (key) {
    const int a = (int)(key >> 32), b = (int)(key & 0xffffffffull);
    const int64_t I = counts[i];
    const int64_t U = (int64_t)area_p[a] + (int64_t)area_g[b] - I;
    int m = 0;
    while (m < T && I * den > (int64_t)thr.num[m] * U) ++m;      // iou > t_k for k < m (the thresholds ascend)
    if (m) atomicAdd(&hist[m], 1);
  }
  const bool label = i >= 1 && i <= label_cap;      // (slots >= 2 h w > label_cap: some thread sees every label)
  const int n_pred = __syncthreads_count(label && area_p[i] > 0);
  const int n_truth = __syncthreads_count(label && area_g[i] > 0);      // (this barrier also orders the LDS adds before the reads below)
  if (threadIdx.x < T) {
    int tp = 0;
    for (int m = threadIdx.x + 1; m <= T; ++m) tp += hist[m];
    if (tp) atomicAdd(out + threadIdx.x, (om_u64)tp);
  }
  if (threadIdx.x == 0) {
    if (n_pred) atomicAdd(out + T, (om_u64)n_pred);
    if (n_truth) atomicAdd(out + T + 1, (om_u64)n_truth);
  }
}

__global__ __launch_bounds__(OM_THREADS) void om_emit_kernel(const om_u64* __restrict__ keys, const int* __restrict__ counts, int64_t slots,
                                                             const int* __restrict__ area_p, const int* __restrict__ area_g, int label_cap,
                                                             int* __restrict__ triples, int64_t capacity, int* count,
                                                             int* __restrict__ area_p_out, int* __restrict__ area_g_out) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * OM_THREADS + threadIdx.x;
  if (i <= label_cap) {
    area_p_out[i] = area_p[i];
    area_g_out[i] = area_g[i];
  }
  const om_u64 key = i < slots ? keys[i] : 0ull;
  const om_u64 taken = __ballot(key != 0ull);
  if (!taken) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(count, __popcll(taken));
  base = __shfl(base, 0);
  if (key) {
    const int64_t k = (int64_t)base + __popcll(taken & ((1ull << lane) - 1ull));
    if (k < capacity) {
      triples[3 * k] = (int)(key >> 32);
      triples[3 * k + 1] = (int)(key & 0xffffffffull);
      triples[3 * k + 2] = counts[i];
    }
  }
}

static inline bool om_size_ok(int32_t h, int32_t w) { return h > 0 && w > 0 && (int64_t)h * w < (1ll << 31); }
static inline int om_log2_slots(int64_t n) {      // the smallest power of two >= 2 n, at least 2
  int l = 1;
  while ((1ll << l) < 2 * n) ++l;
  return l;
}
static inline int64_t om_area_bytes(int64_t n) { return (2 * (n + 1) * 4 + 15) / 16 * 16; }      // two int32 arrays of n + 1 entries
static inline size_t om_workspace_bytes(int64_t n) { return (size_t)(om_area_bytes(n) + (1ll << om_log2_slots(n)) * 12); }

struct OmPlan {
  int64_t n, slots;
  int log2_slots;
  int *area_p, *area_g, *counts;
  om_u64* keys;
};

static OmPlan om_plan(int32_t h, int32_t w, void* workspace) {
  OmPlan p;
  p.n = (int64_t)h * w;
  p.log2_slots = om_log2_slots(p.n);
  p.slots = 1ll << p.log2_slots;
  p.area_p = (int*)workspace;
  p.area_g = p.area_p + p.n + 1;
  p.keys = (om_u64*)((char*)workspace + om_area_bytes(p.n));
  p.counts = (int*)(p.keys + p.slots);
  return p;
}

static inline unsigned om_blocks(int64_t threads) { return (unsigned)((threads + OM_THREADS - 1) / OM_THREADS); }      // (<= 2^24)

// the two launches both entries share: the areas and the pair table of (pred, truth)
static void om_clear_and_count(const OmPlan& p, const int32_t* pred, const int32_t* truth, int h, int w, int label_cap, void* workspace,
                               int64_t* out, int n_out, int* count, om_u64* out_of_range, hipStream_t st) {
  const int64_t words = (int64_t)(om_workspace_bytes(p.n) / 8);
  hipLaunchKernelGGL(om_clear_kernel, dim3(om_blocks(words)), dim3(OM_THREADS), 0, st, (om_u64*)workspace, words, out, n_out, count);
  const int segs = (w + 63) / 64;
  const int64_t items = (int64_t)h * segs;
  hipLaunchKernelGGL(om_count_kernel, dim3((unsigned)((items + 3) / 4)), dim3(OM_THREADS), 0, st, pred, truth, h, w, segs, label_cap, p.area_p,
                     p.area_g, p.keys, p.counts, p.slots, 64 - p.log2_slots, out_of_range);
}

static inline bool om_common_ok(const void* pred, const void* truth, int32_t h, int32_t w, int32_t label_cap, const void* workspace) {
  return pred && truth && workspace && om_size_ok(h, w) && label_cap >= 0 && (int64_t)label_cap <= (int64_t)h * w;
}

extern "C" size_t stp_label_match_workspace_bytes(int32_t h, int32_t w) {
  if (!om_size_ok(h, w)) return 0;
  return om_workspace_bytes((int64_t)h * w);
}

extern "C" int stp_label_match(const int32_t* pred, const int32_t* truth, int32_t h, int32_t w, int32_t label_cap, const int32_t* iou_num,
                               int32_t T, int32_t iou_den, int64_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!om_common_ok(pred, truth, h, w, label_cap, workspace) || !iou_num || !out) return STP_E_BADARG;
  if (T < 1 || T > OM_MAX_T || iou_den < 1 || iou_den > OM_MAX_DEN) return STP_E_BADARG;
  OmThresholds thr;
  for (int k = 0; k < OM_MAX_T; ++k) thr.num[k] = 0;
  for (int k = 0; k < T; ++k) {
    const int64_t num = iou_num[k];
    if (2 * num < iou_den || num > iou_den || (k > 0 && num <= iou_num[k - 1])) return STP_E_BADARG;
    thr.num[k] = (int)num;
  }
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || (reinterpret_cast<uintptr_t>(out) & 7u) != 0) return STP_E_BADARG;
  const OmPlan p = om_plan(h, w, workspace);
  if (workspace_bytes < om_workspace_bytes(p.n)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  om_clear_and_count(p, pred, truth, h, w, label_cap, workspace, out, T + 3, nullptr, (om_u64*)out + T + 2, st);
  hipLaunchKernelGGL(om_finalize_kernel, dim3(om_blocks(p.slots)), dim3(OM_THREADS), 0, st, p.keys, p.counts, p.slots, p.area_p, p.area_g,
                     label_cap, thr, T, iou_den, (om_u64*)out);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" size_t stp_label_overlaps_workspace_bytes(int32_t h, int32_t w) {
  if (!om_size_ok(h, w)) return 0;
  return om_workspace_bytes((int64_t)h * w);
}

extern "C" int stp_label_overlaps(const int32_t* pred, const int32_t* truth, int32_t h, int32_t w, int32_t label_cap, int32_t* triples,
                                  int32_t* count, int64_t capacity, int32_t* area_p, int32_t* area_g, int64_t* out_of_range, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (!om_common_ok(pred, truth, h, w, label_cap, workspace) || !triples || !count || !area_p || !area_g || !out_of_range) return STP_E_BADARG;
  if (capacity < (int64_t)h * w) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || (reinterpret_cast<uintptr_t>(out_of_range) & 7u) != 0) return STP_E_BADARG;
  const OmPlan p = om_plan(h, w, workspace);
  if (workspace_bytes < om_workspace_bytes(p.n)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  om_clear_and_count(p, pred, truth, h, w, label_cap, workspace, out_of_range, 1, count, (om_u64*)out_of_range, st);
  hipLaunchKernelGGL(om_emit_kernel, dim3(om_blocks(p.slots)), dim3(OM_THREADS), 0, st, p.keys, p.counts, p.slots, p.area_p, p.area_g, label_cap,
                     triples, capacity, count, area_p, area_g);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
