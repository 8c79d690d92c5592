// Per-object measurements of a label image on the device (segmentation_pipeline/segmentation.py: predict_instances_ex, score_instances_ex,
// find_confidence, measure_labels): per label its area, the sums of y, of x and of the fixed-point probability, and its bounding box; then
// the selection of the objects that are large and confident enough, renumbered in order.  int32, int64 and fp32 only; the one float
// operation is q = (int)(clamp(p, 0, 1) * 65535.0f) - one multiply, one truncation, nothing a compiler could fuse.  Everything after it is
// exact integer work, equals its host statement (tests/_measure_reference.py) and is the same from run to run: all that workgroups
// exchange are integer sums, minima and maxima.  h, w <= 32767 (a pixel count is an int32); sums and pixel indices are int64.
//
// No workgroup waits for another: what a launch needs from other workgroups was written by an earlier launch on the same stream.
//   ms_clear_kernel    (stp_label_measure) rows 0..label_cap of the table: zero sums, the empty box (h, w, -1, -1); the counter
//   ms_measure_kernel  a wave owns 64 consecutive pixels of a row, MS_ITEMS of them in turn.  A stretch of lanes with one label
//                      (om_stretch's ballot) contributes once, from its first lane: its length, y * length, the closed-form sum of its x,
//                      its sum of q - the wave's inclusive prefix sum of q at its last lane minus the value just before its first, both
//                      read with a shuffle - and y, its first and its last x.  The stretches of one label meet in a table of MS_SLOTS
//                      labels in LDS (a slot is claimed with atomicCAS, whose return value decides; MS_PROBES slots are tried, then the
//                      stretch goes to global memory directly); after the barrier one thread per taken slot adds it to the global row.
//                      One object that fills the image then costs 8 global atomics per workgroup and not per stretch.
//   ms_flag_kernel     (stp_label_select) the workgroup's number of kept labels
//   ms_scan_kernel     one workgroup, the blocks in order: the kept labels before each block; *count
//   ms_map_kernel      the keep flags again, their fixed-order exclusive scan (rle_block_scan) -> map[old] = new or 0; the kept rows are
//                      copied to their new place; row 0 of the outputs
//   ms_relabel_kernel  out_labels[i] = map[labels[i]], 0 for a value outside 0..label_cap; a pixel is read and written by one thread
#include "common.h"
#include "rle_scan.h"

#define MS_THREADS 256
#define MS_WAVES (MS_THREADS / 64)
#define MS_ITEMS 8        // 64-pixel segments a wave takes in turn: a workgroup covers MS_WAVES * MS_ITEMS * 64 = 2048 pixels
#define MS_SLOTS 128      // labels a workgroup combines in LDS (a power of two)
#define MS_SLOT_BITS 7
#define MS_PROBES 4
#define MS_CONF_ONE 65535
#define MS_MAX_DEN 10000
#ifndef MS_COMBINE
#define MS_COMBINE 1      // 0: every stretch goes to global memory (the form the LDS table was measured against)
#endif

static_assert(MS_THREADS == RLE_THREADS, "ms_flag_kernel and ms_map_kernel number the blocks of labels alike");

typedef unsigned long long ms_u64;

__global__ __launch_bounds__(MS_THREADS) void ms_clear_kernel(int64_t* __restrict__ sums, int* __restrict__ boxes, int label_cap, int h, int w,
                                                              int64_t* __restrict__ out_of_range) {
  const int64_t k = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (k == 0) *out_of_range = 0;
  if (k > label_cap) return;
  for (int c = 0; c < 4; ++c) sums[4 * k + c] = 0;
  boxes[4 * k] = h;
  boxes[4 * k + 1] = w;
  boxes[4 * k + 2] = -1;
  boxes[4 * k + 3] = -1;
}

// the lanes of a wave hold consecutive pixels: `first` = this lane starts a stretch of equal labels, `len` = what is left of the stretch
__device__ __forceinline__ void ms_stretch(int key, int lane, bool& first, int& len) {
  const int prev = __shfl_up(key, 1);
  first = lane == 0 || prev != key;
  const ms_u64 firsts = __ballot(first);
  const ms_u64 next = lane == 63 ? 0ull : firsts >> (lane + 1);
  len = next ? __ffsll((long long)next) : 64 - lane;
}

__device__ __forceinline__ int ms_quantise(float p) {
  const float c = p > 0.f ? (p < 1.f ? p : 1.f) : 0.f;      // (a NaN compares false: 0)
  return (int)(c * 65535.0f);
}

__device__ __forceinline__ void ms_global_add(ms_u64* sums, int* boxes, int k, ms_u64 area, ms_u64 sy, ms_u64 sx, ms_u64 sq, int y0, int x0,
                                              int y1, int x1) {
  ms_u64* s = sums + 4 * (int64_t)k;
  int* b = boxes + 4 * (int64_t)k;
  atomicAdd(s, area);
  if (sy) atomicAdd(s + 1, sy);
  if (sx) atomicAdd(s + 2, sx);
  if (sq) atomicAdd(s + 3, sq);
  atomicMin(b, y0);
  atomicMin(b + 1, x0);
  atomicMax(b + 2, y1);
  atomicMax(b + 3, x1);
}

__global__ __launch_bounds__(MS_THREADS) void ms_measure_kernel(const int* __restrict__ labels, const float* __restrict__ probs, int h, int w,
                                                                int C, int channel, int segs, int label_cap, ms_u64* sums, int* boxes,
                                                                ms_u64* out_of_range) {
#if MS_COMBINE
  __shared__ int keys[MS_SLOTS];
  __shared__ ms_u64 acc[MS_SLOTS][4];
  __shared__ int box[MS_SLOTS][4];
  if (threadIdx.x < MS_SLOTS) {
    const int s = threadIdx.x;
    keys[s] = 0;
    acc[s][0] = acc[s][1] = acc[s][2] = acc[s][3] = 0ull;
    box[s][0] = h;
    box[s][1] = w;
    box[s][2] = -1;
    box[s][3] = -1;
  }
  __syncthreads();
#endif
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t items = (int64_t)h * segs;
  const int64_t base = (int64_t)blockIdx.x * (MS_WAVES * MS_ITEMS);
  for (int j = 0; j < MS_ITEMS; ++j) {
    const int64_t item = base + j * MS_WAVES + wave;
    if (item < items) {      // (the same in every lane of a wave: the ballots and shuffles are called by all 64)
      const int y = (int)(item / segs), seg = (int)(item - (int64_t)y * segs);
      const int x = seg * 64 + lane;
      int k = 0, q = 0;
      bool outside = false;
      if (x < w) {
        const int64_t i = (int64_t)y * w + x;
        k = labels[i];
        if ((unsigned)k > (unsigned)label_cap) k = 0, outside = true;      // (a negative value too) background, and never an index
        if (probs && k > 0) q = ms_quantise(probs[i * C + channel]);
      }
      const ms_u64 outs = __ballot(outside);
      if (outs && lane == 0) atomicAdd(out_of_range, (ms_u64)__popcll(outs));
      bool first;
      int len;
      ms_stretch(k, lane, first, len);
      int incl = q;      // the inclusive prefix sum over the wave: at most 64 * 65535
      for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off);
        if (lane >= off) incl += up;
      }
      const int at_end = __shfl(incl, lane + len - 1);
      const int before = __shfl_up(incl, 1);
      if (first && k > 0) {
        const ms_u64 area = (ms_u64)len;
        const ms_u64 sy = (ms_u64)y * area;
        const ms_u64 sx = area * (ms_u64)x + (ms_u64)(len * (len - 1) / 2);
        const ms_u64 sq = (ms_u64)(at_end - (lane ? before : 0));
        const int x1 = x + len - 1;
#if MS_COMBINE
        int s = (int)(((unsigned)k * 0x9E3779B1u) >> (32 - MS_SLOT_BITS));
        bool placed = false;
        for (int probe = 0; probe < MS_PROBES && !placed; ++probe) {
          const int old = atomicCAS(&keys[s], 0, k);
          if (old == 0 || old == k) {
            atomicAdd(&acc[s][0], area);
            atomicAdd(&acc[s][1], sy);
            atomicAdd(&acc[s][2], sx);
            atomicAdd(&acc[s][3], sq);
            atomicMin(&box[s][0], y);
            atomicMin(&box[s][1], x);
            atomicMax(&box[s][2], y);
            atomicMax(&box[s][3], x1);
            placed = true;
          }
          s = (s + 1) & (MS_SLOTS - 1);
        }
        if (!placed) ms_global_add(sums, boxes, k, area, sy, sx, sq, y, x, y, x1);
#else
        ms_global_add(sums, boxes, k, area, sy, sx, sq, y, x, y, x1);
#endif
      }
    }
  }
#if MS_COMBINE
  __syncthreads();
  if (threadIdx.x < MS_SLOTS) {
    const int s = threadIdx.x;
    const int k = keys[s];
    if (k > 0) ms_global_add(sums, boxes, k, acc[s][0], acc[s][1], acc[s][2], acc[s][3], box[s][0], box[s][1], box[s][2], box[s][3]);
  }
#endif
}

// keep label k: area > 0, area >= min_area and sum q * den >= num * 65535 * area (area < 2^31: both products stay below 2^61)
__device__ __forceinline__ bool ms_keep(const int64_t* __restrict__ sums, int64_t k, int label_cap, int64_t min_area, int num, int den) {
  if (k < 1 || k > label_cap) return false;
  const int64_t area = sums[4 * k], sq = sums[4 * k + 3];
  return area > 0 && area >= min_area && sq * den >= (int64_t)num * MS_CONF_ONE * area;
}

__global__ __launch_bounds__(MS_THREADS) void ms_flag_kernel(const int64_t* __restrict__ sums, int label_cap, int64_t min_area, int num, int den,
                                                             int* __restrict__ block_kept) {
  const int64_t k = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  const int kept = __syncthreads_count(ms_keep(sums, k, label_cap, min_area, num, den));
  if (threadIdx.x == 0) block_kept[blockIdx.x] = kept;
}

// one workgroup, the blocks in order: block_kept[b] becomes the number of kept labels before block b; *count
__global__ __launch_bounds__(RLE_THREADS) void ms_scan_kernel(int* block_kept, int blocks, int* __restrict__ count) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  int run = 0;
  for (int b0 = 0; b0 < blocks; b0 += RLE_THREADS) {
    const int b = b0 + threadIdx.x;
    const int a = b < blocks ? block_kept[b] : 0;
    int es, em, ts, tm;
    rle_block_scan(a, -1, sa, sm, es, em, ts, tm);
    if (b < blocks) block_kept[b] = run + es;
    run += ts;
  }
  if (threadIdx.x == 0) *count = run;
}

__global__ __launch_bounds__(RLE_THREADS) void ms_map_kernel(const int64_t* __restrict__ sums, const int* __restrict__ boxes, int label_cap,
                                                             int h, int w, int64_t min_area, int num, int den,
                                                             const int* __restrict__ kept_before, int* __restrict__ map,
                                                             int64_t* __restrict__ out_sums, int* __restrict__ out_boxes) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  const int64_t k = (int64_t)blockIdx.x * RLE_THREADS + threadIdx.x;
  const bool keep = ms_keep(sums, k, label_cap, min_area, num, den);
  int es, em, ts, tm;
  rle_block_scan(keep ? 1 : 0, -1, sa, sm, es, em, ts, tm);
  if (k > label_cap) return;
  const int64_t to = keep ? (int64_t)kept_before[blockIdx.x] + es + 1 : 0;
  map[k] = (int)to;
  if (keep) {
    for (int c = 0; c < 4; ++c) {
      out_sums[4 * to + c] = sums[4 * k + c];
      out_boxes[4 * to + c] = boxes[4 * k + c];
    }
  }
  if (k == 0) {
    for (int c = 0; c < 4; ++c) out_sums[c] = 0;
    out_boxes[0] = h;
    out_boxes[1] = w;
    out_boxes[2] = -1;
    out_boxes[3] = -1;
  }
}

__global__ __launch_bounds__(MS_THREADS) void ms_relabel_kernel(const int* labels, int64_t n, int label_cap, const int* __restrict__ map,
                                                                int* out_labels) {
  const int64_t i = (int64_t)blockIdx.x * MS_THREADS + threadIdx.x;
  if (i >= n) return;
  const int k = labels[i];
  out_labels[i] = (unsigned)k > (unsigned)label_cap ? 0 : map[k];
}

static inline bool ms_size_ok(int32_t h, int32_t w) { return h > 0 && w > 0 && h <= 32767 && w <= 32767; }      // (h * w < 2^30)
static inline bool ms_cap_ok(int32_t h, int32_t w, int32_t label_cap) { return label_cap >= 0 && (int64_t)label_cap <= (int64_t)h * w; }
static inline bool ms_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
static inline unsigned ms_blocks(int64_t threads) { return (unsigned)((threads + MS_THREADS - 1) / MS_THREADS); }      // (<= 2^22)
static inline int64_t ms_map_bytes(int64_t label_cap) { return ((label_cap + 1) * 4 + 7) / 8 * 8; }
static inline size_t ms_select_bytes(int64_t label_cap) {      // map[label_cap + 1], then one int32 per block of 256 labels
  return (size_t)(ms_map_bytes(label_cap) + ((int64_t)ms_blocks(label_cap + 1) * 4 + 7) / 8 * 8);
}

extern "C" int stp_label_measure(const int32_t* labels, const float* probs, int32_t h, int32_t w, int32_t C, int32_t channel,
                                 int32_t label_cap, int64_t* sums, int32_t* boxes, int64_t* out_of_range, void* stream) {
  if (!labels || !sums || !boxes || !out_of_range || !ms_size_ok(h, w) || !ms_cap_ok(h, w, label_cap)) return STP_E_BADARG;
  if (probs && (C < 1 || channel < 0 || channel >= C)) return STP_E_BADARG;
  if (!ms_aligned8(sums) || !ms_aligned8(out_of_range)) return STP_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ms_clear_kernel, dim3(ms_blocks((int64_t)label_cap + 1)), dim3(MS_THREADS), 0, st, sums, boxes, label_cap, h, w,
                     out_of_range);
  const int segs = (w + 63) / 64;
  const int64_t items = (int64_t)h * segs;
  const int per_block = MS_WAVES * MS_ITEMS;
  hipLaunchKernelGGL(ms_measure_kernel, dim3((unsigned)((items + per_block - 1) / per_block)), dim3(MS_THREADS), 0, st, labels, probs, h, w,
                     probs ? C : 1, probs ? channel : 0, segs, label_cap, (ms_u64*)sums, boxes, (ms_u64*)out_of_range);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" size_t stp_label_select_workspace_bytes(int32_t label_cap) {
  if (label_cap < 0) return 0;
  return ms_select_bytes(label_cap);
}

extern "C" int stp_label_select(const int32_t* labels, int32_t h, int32_t w, int32_t label_cap, const int64_t* sums, const int32_t* boxes,
                                int64_t min_area, int32_t conf_num, int32_t conf_den, int32_t* out_labels, int32_t* count,
                                int64_t* out_sums, int32_t* out_boxes, void* workspace, size_t workspace_bytes, void* stream) {
  if (!labels || !sums || !boxes || !out_labels || !count || !out_sums || !out_boxes || !workspace) return STP_E_BADARG;
  if (!ms_size_ok(h, w) || !ms_cap_ok(h, w, label_cap) || min_area < 0) return STP_E_BADARG;
  if (conf_den < 1 || conf_den > MS_MAX_DEN || conf_num < 0 || conf_num > conf_den) return STP_E_BADARG;
  if ((const void*)out_sums == (const void*)sums || (const void*)out_boxes == (const void*)boxes) return STP_E_BADARG;
  if (!ms_aligned8(workspace) || !ms_aligned8(sums) || !ms_aligned8(out_sums)) return STP_E_BADARG;
  if (workspace_bytes < ms_select_bytes(label_cap)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int* map = (int*)workspace;
  int* block_kept = (int*)((char*)workspace + ms_map_bytes(label_cap));
  const unsigned blocks = ms_blocks((int64_t)label_cap + 1);
  hipLaunchKernelGGL(ms_flag_kernel, dim3(blocks), dim3(MS_THREADS), 0, st, sums, label_cap, min_area, conf_num, conf_den, block_kept);
  hipLaunchKernelGGL(ms_scan_kernel, dim3(1), dim3(RLE_THREADS), 0, st, block_kept, (int)blocks, count);
  hipLaunchKernelGGL(ms_map_kernel, dim3(blocks), dim3(RLE_THREADS), 0, st, sums, boxes, label_cap, h, w, min_area, conf_num, conf_den,
                     block_kept, map, out_sums, out_boxes);
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(ms_relabel_kernel, dim3(ms_blocks(n)), dim3(MS_THREADS), 0, st, labels, n, label_cap, map, out_labels);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
