// Connected components on the device (segmentation_pipeline/segmentation.py: predict_masks_ex's min_size / area_threshold / components): the
// objects of ONE uint8 mask [h, w] - their numbers (scipy.ndimage.label), the mask without its small objects or with its small holes
// filled (skimage's remove_small_objects / remove_small_holes), and the run-length code of a label image, one triple per run
// (impl/rle.py: multi_rle_encode).  uint8, int32 and int64 only; every result is exact integer work and equals its host statement
// (tests/_components_reference.py) bit for bit.  h * w < 2^31, so a pixel index is an int32; indices that are scaled are int64.
//
// No workgroup waits for another: what a launch needs from other workgroups was written by an earlier launch on the same stream.  The one
// exchange inside a launch is the union-find of cc_merge_kernel (DESIGN.md 3.25 has the argument):
//   * parent[i] <= i always (-1: not foreground, which never changes); a root is parent[i] == i
//   * find only descends; union attaches the larger root to the smaller with an int32 atomicMin and, when the value the atomic RETURNS
//     shows the node was no longer a root, goes on from that value - max(a, b) strictly decreases, so every loop ends on any input and
//     under any interleaving
//   * every parent read of that launch is an agent-scope atomic load (the XCDs' L2s and the CUs' L1s are not coherent); a stale value
//     would still be an ancestor of the same component, and no decision rests on a read - only on the atomic's return value
//
//   stp_mask_label        init (row runs of 64-pixel segments from one ballot), merge, flatten + roots per workgroup, one fixed-order
//                         scan, rank of the roots, relabel: 6 launches
//   stp_mask_area_filter  init, merge, flatten + int32 atomicAdd of workgroup- and wave-pre-summed counts into area[root], select: 4 launches
//                         (one binarising launch when min_size <= 1: no component has fewer than 1 pixel)
//   stp_label_rle         64 x 64 tiles transposed through LDS into the flat column-major array, run ends and the last run start
//                         counted per workgroup of 1024 pixels, the fixed-order scan of mask.hip, a compacting write: 4 launches
#include "common.h"
#include "rle_scan.h"

#define CC_THREADS 256
#define LRLE_PER_THREAD 4
#define LRLE_BLOCK (RLE_THREADS * LRLE_PER_THREAD)

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of i's tree: only descends (parent[i] <= i), ends at a cell that names itself
__device__ __forceinline__ int cc_find(const int* parent, int i) {
  int p;
  while ((p = cc_load(parent + i)) != i) i = p;
  return i;
}

// joins the trees of a and b.  a > b are roots as far as this thread has seen; atomicMin(parent[a], b) returns a when a still was one -
// done - and otherwise the parent a had meanwhile: that tree and b's still have to meet (the link a -> old may just have been replaced
// by a -> b), so the loop goes on with (old, b), old < a.
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  for (;;) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

// A wave owns 64 consecutive pixels of a row.  Foreground = (img != 0) != invert; a foreground pixel's parent is the first pixel of its
// run inside the segment (the position after the last 0 bit below the lane), everything else is -1.  `area` (may be NULL) is zeroed.
__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const uint8_t* __restrict__ img, int h, int w, int segs, int invert,
                                                             int* __restrict__ parent, int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (CC_THREADS / 64) + (threadIdx.x >> 6);
  if (item >= (int64_t)h * segs) return;      // (the same in every lane of a wave: the ballot is called by all 64)
  const int y = (int)(item / segs), seg = (int)(item - (int64_t)y * segs);
  const int x = seg * 64 + lane;
  const int64_t i = (int64_t)y * w + x;
  bool fg = false;
  if (x < w) fg = (img[i] != 0) != (invert != 0);
  const unsigned long long b = __ballot(fg);
  if (x < w) {
    const unsigned long long below = ~b & ((1ull << lane) - 1ull);
    const int start = below ? 64 - __clzll((long long)below) : 0;
    parent[i] = fg ? (int)(i - lane + start) : -1;
    if (area) area[i] = 0;
  }
}

// One thread per foreground pixel and the unions the runs of cc_init_kernel leave open: left across a segment border, up, and (connectivity
// 2) the two upper diagonals - each only where no other link already implies it (L, U, UL: the left, upper, upper-left neighbour is
// foreground):  up is implied by L && UL (the left pixel's own up link and the two row links);  up-left by L or U;  up-right by U.
__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(int* parent, int h, int w, int connectivity) {
  const int64_t n = (int64_t)h * w;
  const int64_t i64 = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i64 >= n) return;
  const int i = (int)i64;
  if (cc_load(parent + i) < 0) return;
  const int y = i / w, x = i - y * w;
  const bool L = x > 0 && cc_load(parent + i - 1) >= 0;
  if (L && (x & 63) == 0) cc_union(parent, i, i - 1);
  if (y == 0) return;
  const bool U = cc_load(parent + i - w) >= 0;
  const bool UL = x > 0 && cc_load(parent + i - w - 1) >= 0;
  if (U && !(L && UL)) cc_union(parent, i, i - w);
  if (connectivity == 2) {
    if (UL && !L && !U) cc_union(parent, i, i - w - 1);
    if (!U && x + 1 < w && cc_load(parent + i - w + 1) >= 0) cc_union(parent, i, i - w + 1);
  }
}

// A later launch: the trees are final, every pixel is pointed at its root (a cell read here holds its old parent or its root - both
// ancestors - and a root's cell never changes).  block_roots[b] = the roots among the workgroup's 256 pixels.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_count_kernel(int* parent, int64_t n, int* __restrict__ block_roots) {
  const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  int is_root = 0;
  if (i < n && cc_load(parent + i) >= 0) {
    const int root = cc_find(parent, (int)i);
    parent[i] = root;
    is_root = root == (int)i;
  }
  const int roots = __syncthreads_count(is_root);
  if (threadIdx.x == 0) block_roots[blockIdx.x] = roots;
}

// one workgroup, the blocks in order: roots_before[b] = the roots of the blocks before b; *count = all of them
__global__ __launch_bounds__(RLE_THREADS) void cc_scan_kernel(const int* __restrict__ block_roots, int blocks, int* __restrict__ roots_before,
                                                              int* __restrict__ count) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  int run_sum = 0;
  for (int b0 = 0; b0 < blocks; b0 += RLE_THREADS) {
    const int b = b0 + threadIdx.x;
    int es, em, ts, tm;
    rle_block_scan(b < blocks ? block_roots[b] : 0, -1, sa, sm, es, em, ts, tm);
    if (b < blocks) roots_before[b] = run_sum + es;
    run_sum += ts;
  }
  if (threadIdx.x == 0) *count = run_sum;
}

// a root's label is the number of roots at or before it in row-major order; only the roots' cells of `labels` are written here
__global__ __launch_bounds__(RLE_THREADS) void cc_rank_kernel(const int* __restrict__ parent, int64_t n, const int* __restrict__ roots_before,
                                                              int* __restrict__ labels) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  const int64_t i = (int64_t)blockIdx.x * RLE_THREADS + threadIdx.x;
  const int is_root = i < n && parent[i] == (int)i;
  int es, em, ts, tm;
  rle_block_scan(is_root, -1, sa, sm, es, em, ts, tm);
  if (is_root) labels[i] = roots_before[blockIdx.x] + es + 1;
}

// every other pixel: 0 off the foreground, else its root's label (the roots' cells are read, never written, in this launch)
__global__ __launch_bounds__(CC_THREADS) void cc_relabel_kernel(const int* __restrict__ parent, int64_t n, int* labels) {
  const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= n) return;
  const int p = parent[i];
  if (p < 0) labels[i] = 0;
  else if (p != (int)i) labels[i] = labels[p];
}

// Flatten, and area[root] += 1 per pixel, pre-summed twice (integer adds: the sums do not depend on their order or grouping).  The
// workgroup's 1024 consecutive pixels count those of ONE root - the smallest root among them, which for the large component that would
// otherwise meet in one cell from every wave is that component's - and add them once.  The rest goes by waves: the lanes are consecutive
// pixels, a stretch of lanes with one root adds its length once, from its first lane.
#define CC_AREA_THREADS 1024
__global__ __launch_bounds__(CC_AREA_THREADS) void cc_flatten_area_kernel(int* parent, int64_t n, int* __restrict__ area) {
  __shared__ int wave_min[CC_AREA_THREADS / 64];
  const int64_t i = (int64_t)blockIdx.x * CC_AREA_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int root = -1;
  if (i < n && cc_load(parent + i) >= 0) {
    root = cc_find(parent, (int)i);
    parent[i] = root;
  }
  int m = root >= 0 ? root : 0x7fffffff;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = min(m, __shfl_xor(m, off));
  if (lane == 0) wave_min[threadIdx.x >> 6] = m;
  __syncthreads();
  int common = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < CC_AREA_THREADS / 64; ++k) common = min(common, wave_min[k]);
  const int members = __syncthreads_count(root == common);
  if (threadIdx.x == 0 && members > 0) atomicAdd(area + common, members);
  const int key = root == common ? -1 : root;      // what is left for the waves
  const int prev = __shfl_up(key, 1);
  const bool first = lane == 0 || prev != key;
  const unsigned long long firsts = __ballot(first);
  if (first && key >= 0) {
    const unsigned long long next = lane == 63 ? 0ull : firsts >> (lane + 1);
    atomicAdd(area + key, next ? __ffsll((long long)next) : 64 - lane);
  }
}

// invert 0: the foreground pixels of components with area >= min_size;  invert 1 (foreground = the zeros): the ones, and the zeros of
// components with area < min_size.  `src` is not read again: parent >= 0 says what it held.
__global__ __launch_bounds__(CC_THREADS) void cc_select_kernel(const int* __restrict__ parent, const int* __restrict__ area, int64_t n,
                                                               int invert, int64_t min_size, uint8_t* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= n) return;
  const int p = parent[i];
  uint8_t v;
  if (p < 0) v = invert ? 1 : 0;
  else {
    const bool small = (int64_t)area[p] < min_size;
    v = invert ? small : !small;
  }
  dst[i] = v;
}

// min_size <= 1 removes / fills nothing: dst = (src != 0); a thread reads and writes its own pixel, so src == dst is fine
__global__ __launch_bounds__(CC_THREADS) void cc_binarise_kernel(const uint8_t* src, int64_t n, uint8_t* dst) {
  const int64_t i = (int64_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i < n) dst[i] = src[i] != 0;
}

static inline int64_t cc_blocks(int64_t n) { return (n + CC_THREADS - 1) / CC_THREADS; }
static inline int64_t round16(int64_t v) { return (v + 15) / 16 * 16; }
static inline bool cc_size_ok(int32_t h, int32_t w) { return h > 0 && w > 0 && (int64_t)h * w < (1ll << 31); }
static inline size_t label_workspace_bytes(int64_t n) { return (size_t)(n * 4 + round16(cc_blocks(n) * 2 * (int64_t)sizeof(int))); }
static inline size_t area_workspace_bytes(int64_t n) { return (size_t)(n * 8); }

// the two launches every entry shares: parent[] of the final trees (not yet flattened)
static void cc_build_forest(const uint8_t* img, int h, int w, int connectivity, int invert, int* parent, int* area, hipStream_t st) {
  const int segs = (w + 63) / 64;
  const int64_t items = (int64_t)h * segs;      // (< 2^31 / 64 + h)
  hipLaunchKernelGGL(cc_init_kernel, dim3((unsigned)((items + 3) / 4)), dim3(CC_THREADS), 0, st, img, h, w, segs, invert, parent, area);
  hipLaunchKernelGGL(cc_merge_kernel, dim3((unsigned)cc_blocks((int64_t)h * w)), dim3(CC_THREADS), 0, st, parent, h, w, connectivity);
}

extern "C" size_t stp_mask_label_workspace_bytes(int32_t h, int32_t w) {
  if (!cc_size_ok(h, w)) return 0;
  return label_workspace_bytes((int64_t)h * w);
}

extern "C" int stp_mask_label(const uint8_t* img, int32_t h, int32_t w, int32_t connectivity, int32_t invert, int32_t* labels, int32_t* count,
                              void* workspace, size_t workspace_bytes, void* stream) {
  if (!img || !labels || !count || !workspace || !cc_size_ok(h, w) || connectivity < 1 || connectivity > 2) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  if (workspace_bytes < label_workspace_bytes(n)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)cc_blocks(n);      // (< 2^23: every grid here is far below 2^31 - 1 workgroups)
  int* parent = (int*)workspace;
  int *block_roots = parent + n, *roots_before = block_roots + blocks;
  cc_build_forest(img, h, w, connectivity, invert != 0, parent, nullptr, st);
  hipLaunchKernelGGL(cc_flatten_count_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, parent, n, block_roots);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(RLE_THREADS), 0, st, block_roots, blocks, roots_before, count);
  hipLaunchKernelGGL(cc_rank_kernel, dim3(blocks), dim3(RLE_THREADS), 0, st, parent, n, roots_before, labels);
  hipLaunchKernelGGL(cc_relabel_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, parent, n, labels);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" size_t stp_mask_area_filter_workspace_bytes(int32_t h, int32_t w) {
  if (!cc_size_ok(h, w)) return 0;
  return area_workspace_bytes((int64_t)h * w);
}

extern "C" int stp_mask_area_filter(const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t connectivity, int32_t invert,
                                    int64_t min_size, void* workspace, size_t workspace_bytes, void* stream) {
  if (!src || !dst || !workspace || !cc_size_ok(h, w) || connectivity < 1 || connectivity > 2 || min_size < 0) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  if (workspace_bytes < area_workspace_bytes(n)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int blocks = (int)cc_blocks(n);
  if (min_size <= 1) {
    hipLaunchKernelGGL(cc_binarise_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, src, n, dst);
  } else {
    int* parent = (int*)workspace;
    int* area = parent + n;
    cc_build_forest(src, h, w, connectivity, invert != 0, parent, area, st);      // (the only launch that reads src: the first)
    hipLaunchKernelGGL(cc_flatten_area_kernel, dim3((unsigned)((n + CC_AREA_THREADS - 1) / CC_AREA_THREADS)), dim3(CC_AREA_THREADS), 0, st, parent,
                       n, area);
    hipLaunchKernelGGL(cc_select_kernel, dim3(blocks), dim3(CC_THREADS), 0, st, parent, area, n, invert != 0, min_size, dst);
  }
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------------ run-length code of a label image
// T[x * h + y] = labels[y][x]: the flat column-major array itself
__global__ __launch_bounds__(256) void lrle_transpose_kernel(const int* __restrict__ labels, int h, int w, int tiles_x, int* __restrict__ T) {
  __shared__ int tile[64][65];      // (rows 65 dwords apart: a wave reads one column of 64 rows from 64 banks)
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int64_t y0 = (int64_t)ty * 64, x0 = (int64_t)tx * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 4
  for (int rr = wave; rr < 64; rr += 4) {
    const int64_t y = y0 + rr, x = x0 + lane;
    tile[rr][lane] = (y < h && x < w) ? labels[y * w + x] : 0;
  }
  __syncthreads();
  for (int c = wave; c < 64; c += 4) {
    const int64_t x = x0 + c, y = y0 + lane;
    if (x < w && y < h) T[x * h + y] = tile[lane][c];
  }
}

// the thread's LRLE_PER_THREAD consecutive values of T from `base`, and as bit masks which of them start / end a run: a non-zero value
// that differs from its flat predecessor / successor (0 past either end of the array)
__device__ __forceinline__ void lrle_edges(const int* __restrict__ T, int64_t n, int64_t base, int (&v)[LRLE_PER_THREAD], unsigned& starts,
                                           unsigned& ends) {
  starts = ends = 0u;
  int prev = (base > 0 && base - 1 < n) ? T[base - 1] : 0;
  int cur = base < n ? T[base] : 0;
#pragma unroll
  for (int e = 0; e < LRLE_PER_THREAD; ++e) {
    const int next = base + e + 1 < n ? T[base + e + 1] : 0;
    v[e] = cur;
    if (cur != 0) {
      if (cur != prev) starts |= 1u << e;
      if (cur != next) ends |= 1u << e;
    }
    prev = cur;
    cur = next;
  }
}

// per workgroup of 1024 values: how many runs end in it, and the position of its last run start (-1: none)
__global__ __launch_bounds__(RLE_THREADS) void lrle_count_kernel(const int* __restrict__ T, int64_t n, int* __restrict__ block_ends,
                                                                 int* __restrict__ block_last) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  const int64_t base = ((int64_t)blockIdx.x * RLE_THREADS + threadIdx.x) * LRLE_PER_THREAD;
  int v[LRLE_PER_THREAD];
  unsigned starts, ends;
  lrle_edges(T, n, base, v, starts, ends);
  const int last = starts ? (int)(base + 31 - __clz((int)starts)) : -1;
  int es, em, ts, tm;
  rle_block_scan(__popc(ends), last, sa, sm, es, em, ts, tm);
  if (threadIdx.x == 0) {
    block_ends[blockIdx.x] = ts;
    block_last[blockIdx.x] = tm;
  }
}

// the k-th end closes the k-th start; a run's start is the last start at or before its end - in this thread's values, or carried
__global__ __launch_bounds__(RLE_THREADS) void lrle_write_kernel(const int* __restrict__ T, int64_t n, const int* __restrict__ ends_before,
                                                                 const int* __restrict__ carry, int* __restrict__ runs) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  const int64_t base = ((int64_t)blockIdx.x * RLE_THREADS + threadIdx.x) * LRLE_PER_THREAD;
  int v[LRLE_PER_THREAD];
  unsigned starts, ends;
  lrle_edges(T, n, base, v, starts, ends);
  const int last = starts ? (int)(base + 31 - __clz((int)starts)) : -1;
  int es, em, ts, tm;
  rle_block_scan(__popc(ends), last, sa, sm, es, em, ts, tm);
  int64_t k = (int64_t)ends_before[blockIdx.x] + es;
  int open = max(carry[blockIdx.x], em);      // the start of a run that was open when this thread's values began
#pragma unroll
  for (int e = 0; e < LRLE_PER_THREAD; ++e) {
    if (starts >> e & 1u) open = (int)(base + e);
    if (ends >> e & 1u) {
      runs[3 * k] = v[e];
      runs[3 * k + 1] = open + 1;
      runs[3 * k + 2] = (int)(base + e) - open + 1;
      ++k;
    }
  }
}

static inline int64_t lrle_blocks(int64_t n) { return (n + LRLE_BLOCK - 1) / LRLE_BLOCK; }
static inline size_t lrle_workspace_bytes(int64_t n) { return (size_t)(n * 4 + round16(lrle_blocks(n) * 4 * (int64_t)sizeof(int))); }

extern "C" size_t stp_label_rle_workspace_bytes(int32_t h, int32_t w) {
  if (!cc_size_ok(h, w)) return 0;
  return lrle_workspace_bytes((int64_t)h * w);
}

extern "C" int stp_label_rle(const int32_t* labels, int32_t h, int32_t w, int32_t* runs, int32_t* count, int64_t capacity, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (!labels || !runs || !count || !workspace || !cc_size_ok(h, w)) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  if (capacity < n) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return STP_E_BADARG;
  if (workspace_bytes < lrle_workspace_bytes(n)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t tiles_x = ((int64_t)w + 63) / 64, tiles_y = ((int64_t)h + 63) / 64;      // (tiles_x * tiles_y < 2^31 / 4096 + h + w)
  const int blocks = (int)lrle_blocks(n);
  int* T = (int*)workspace;
  int* block_ends = T + n;
  int *block_last = block_ends + blocks, *ends_before = block_last + blocks, *carry = ends_before + blocks;
  hipLaunchKernelGGL(lrle_transpose_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, st, labels, h, w, (int)tiles_x, T);
  hipLaunchKernelGGL(lrle_count_kernel, dim3(blocks), dim3(RLE_THREADS), 0, st, T, n, block_ends, block_last);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(RLE_THREADS), 0, st, block_ends, block_last, blocks, ends_before, carry, count);
  hipLaunchKernelGGL(lrle_write_kernel, dim3(blocks), dim3(RLE_THREADS), 0, st, T, n, ends_before, carry, runs);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
