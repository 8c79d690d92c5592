// Masks on the device (segmentation_pipeline/segmentation.py: predict_masks, predict_to_csv, find_threshold): what the users of a trained
// binary model do with the finished fp32 probability map of ONE image at its own size (stp_predict_finish mode 0) - threshold it, clean the
// mask with a disk opening / closing, run-length encode it, or count it against a target at many thresholds at once.  uint8, fp32 and
// integers only (nothing here depends on the build's 16-bit storage format); every result is exact integer work, so each entry point
// equals its host statement (tests/_mask_reference.py: numpy, scipy.ndimage, impl/rle.py) bit for bit.  No float atomics; int64 element
// indices; every count that leaves a workgroup is summed in a fixed order or is an integer sum.
//
//   stp_mask_threshold    one thread per 16 pixels of a destination row (one 16-byte store where base and pitch allow it, else per pixel)
//   stp_mask_morph        bit rows in LDS: a wave packs 64 pixels of a row with one ballot, a thread owns 64 output pixels of a row as
//                         one 64-bit word and combines the disk's horizontal spans with funnel shifts of the words of the rows above / below
//   stp_mask_rle          64 x 64 tiles transposed through LDS into a column-major bit stream (global loads stay row-contiguous), run
//                         ends and the last run start counted per workgroup, one fixed-order scan, a compacting write of (start, length)
//   stp_threshold_counts  per pixel j = #thresholds below the value, a workgroup LDS table [T + 1][2] of integers (wave peel of
//                         wave_count.h), workgroup tables summed and suffix-summed by a finalize launch
#include "common.h"
#include "rle_scan.h"
#include "wave_count.h"

static inline bool mask_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static inline int mask_stream_grid(int64_t items) {
  int64_t g = (items + 255) / 256;
  return (int)(g > 16384 ? 16384 : g);
}

// ------------------------------------------------------------------------------------------------ threshold
template <int VEC> struct alignas(VEC) MaskPack {
  uint8_t v[VEC];
};

// MODE 0: px[channel] > thr (false for a NaN);  1: the first index of the largest of the C values (finish_one<2> of predict.hip) == channel
template <int MODE> __device__ __forceinline__ uint8_t mask_one(const float* __restrict__ px, int C, int channel, float thr) {
  if (MODE == 0) return px[channel] > thr;
  float best = px[0];
  int arg = 0;
  for (int c = 1; c < C; ++c) {
    const float v = px[c];
    if (v > best) best = v, arg = c;
  }
  return arg == channel;
}

template <int MODE, int VEC>
__global__ __launch_bounds__(256) void mask_threshold_kernel(const float* __restrict__ map, int h, int w, int C, int channel, float thr,
                                                             uint8_t* __restrict__ out, int64_t pitch) {
  typedef MaskPack<VEC> P;
  const int vpr = (w + VEC - 1) / VEC;
  const int64_t total = (int64_t)h * vpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int y = (int)(i / vpr);
    const int x0 = (int)(i - (int64_t)y * vpr) * VEC;
    const float* srow = map + ((int64_t)y * w + x0) * C;
    uint8_t* dptr = out + (int64_t)y * pitch + x0;
    if (x0 + VEC <= w) {
      P v;
#pragma unroll
      for (int j = 0; j < VEC; ++j) v.v[j] = mask_one<MODE>(srow + (int64_t)j * C, C, channel, thr);
      *reinterpret_cast<P*>(dptr) = v;
    } else {      // the row's tail: fewer than VEC pixels left
      for (int j = 0; x0 + j < w; ++j) dptr[j] = mask_one<MODE>(srow + (int64_t)j * C, C, channel, thr);
    }
  }
}

template <int MODE>
static void launch_threshold(const float* map, int h, int w, int C, int channel, float thr, uint8_t* out, int64_t pitch, hipStream_t st) {
  if (mask_aligned16(out) && pitch % 16 == 0) {
    hipLaunchKernelGGL((mask_threshold_kernel<MODE, 16>), dim3(mask_stream_grid((int64_t)h * ((w + 15) / 16))), dim3(256), 0, st, map, h, w, C,
                       channel, thr, out, pitch);
  } else {
    hipLaunchKernelGGL((mask_threshold_kernel<MODE, 1>), dim3(mask_stream_grid((int64_t)h * w)), dim3(256), 0, st, map, h, w, C, channel, thr, out,
                       pitch);
  }
}

extern "C" int stp_mask_threshold(const float* map, int32_t h, int32_t w, int32_t C, int32_t channel, int32_t mode, float threshold,
                                  uint8_t* out, int32_t out_ld, void* stream) {
  if (!map || !out || (const void*)map == (const void*)out || h <= 0 || w <= 0 || C <= 0 || channel < 0 || channel >= C || mode < 0 || mode > 1 ||
      out_ld < w)
    return STP_E_BADARG;
  if (mode == 1 && C > 32) return STP_E_BADARG;
  if (mode == 0) launch_threshold<0>(map, h, w, C, channel, threshold, out, out_ld, (hipStream_t)stream);
  else launch_threshold<1>(map, h, w, C, channel, threshold, out, out_ld, (hipStream_t)stream);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------------ erosion / dilation by a disk
// A workgroup owns MORPH_ROWS x (64 * MORPH_WORDS) output pixels.  It holds the rows y0 - r .. y0 + MORPH_ROWS - 1 + r of the columns
// x0 - r .. x0 - r + 64 * (MORPH_WORDS + 1) - 1 as bits (bit i of word k of a row = column x0 - r + 64 k + i; 0 outside the image).  Output
// word k of a row (columns x0 + 64 k ..) takes, for the row dy above / below and every dx of the disk's span |dx| <= span[|dy|], the 128
// bits of words k and k + 1 of that row shifted down by r + dx: AND for the erosion, OR for the dilation.
#define MORPH_ROWS 64
#define MORPH_WORDS 4
#define MORPH_RMAX 7
#define MORPH_LROWS (MORPH_ROWS + 2 * MORPH_RMAX)
#define MORPH_BATCH 8

struct MorphDisk {
  int span[MORPH_RMAX + 1];      // span[d]: the largest dx with dx * dx + d * d <= r * r
};

__global__ __launch_bounds__(256) void mask_morph_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int h, int w, int r,
                                                         int dilate, int tiles_x, const MorphDisk disk) {
  __shared__ unsigned long long bits[MORPH_LROWS][MORPH_WORDS + 1];
  __shared__ unsigned long long outw[MORPH_ROWS][MORPH_WORDS];
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int64_t y0 = (int64_t)ty * MORPH_ROWS, x0 = (int64_t)tx * (64 * MORPH_WORDS);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrows = MORPH_ROWS + 2 * r;
  // MORPH_BATCH loads are in flight before the first ballot waits for one (a wave's loads would otherwise wait for each other's latency);
  // the trip count is the same in every lane of a wave: the ballot is called by all 64
  const int lwords = lrows * (MORPH_WORDS + 1);
  for (int idx0 = wave; idx0 < lwords; idx0 += 4 * MORPH_BATCH) {
    uint8_t v[MORPH_BATCH];
#pragma unroll
    for (int u = 0; u < MORPH_BATCH; ++u) {
      const int idx = idx0 + 4 * u;
      const int row = idx / (MORPH_WORDS + 1), word = idx - row * (MORPH_WORDS + 1);
      const int64_t gy = y0 - r + row, gx = x0 - r + word * 64 + lane;
      v[u] = 0;
      if (idx < lwords && gy >= 0 && gy < h && gx >= 0 && gx < w) v[u] = src[gy * w + gx];
    }
#pragma unroll
    for (int u = 0; u < MORPH_BATCH; ++u) {
      const int idx = idx0 + 4 * u;
      const int row = idx / (MORPH_WORDS + 1), word = idx - row * (MORPH_WORDS + 1);
      const unsigned long long b = __ballot(v[u] != 0);
      if (lane == 0 && idx < lwords) bits[row][word] = b;
    }
  }
  __syncthreads();
  {
    const int orow = threadIdx.x / MORPH_WORDS, k = threadIdx.x - orow * MORPH_WORDS;
    unsigned long long acc = dilate ? 0ull : ~0ull;
    for (int dy = -r; dy <= r; ++dy) {
      const unsigned long long lo = bits[orow + r + dy][k], hi = bits[orow + r + dy][k + 1];
      const int span = disk.span[dy < 0 ? -dy : dy];
      for (int s = r - span; s <= r + span; ++s) {
        const unsigned long long v = s == 0 ? lo : (lo >> s) | (hi << (64 - s));
        acc = dilate ? (acc | v) : (acc & v);
      }
    }
    outw[orow][k] = acc;
  }
  __syncthreads();
  const int64_t gx = x0 + threadIdx.x;
  if (gx < w) {
    for (int i = 0; i < MORPH_ROWS && y0 + i < h; ++i) dst[(y0 + i) * w + gx] = (uint8_t)((outw[i][wave] >> lane) & 1ull);
  }
}

extern "C" int stp_mask_morph(const uint8_t* src, uint8_t* dst, int32_t h, int32_t w, int32_t r, int32_t op, void* stream) {
  if (!src || !dst || src == dst || h <= 0 || w <= 0 || r < 1 || r > MORPH_RMAX || op < 0 || op > 1) return STP_E_BADARG;
  const int64_t tiles_x = ((int64_t)w + 64 * MORPH_WORDS - 1) / (64 * MORPH_WORDS), tiles_y = ((int64_t)h + MORPH_ROWS - 1) / MORPH_ROWS;
  if (tiles_x * tiles_y > 0x7fffffff) return STP_E_BADARG;
  MorphDisk disk;
  for (int d = 0; d <= MORPH_RMAX; ++d) {
    int s = 0;
    while (d <= r && (s + 1) * (s + 1) + d * d <= r * r) ++s;
    disk.span[d] = s;
  }
  hipLaunchKernelGGL(mask_morph_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(256), 0, (hipStream_t)stream, src, dst, h, w, r, op, (int)tiles_x, disk);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------------ run-length code
// The code numbers pixels column-major, p = x * h + y.  The bit stream: column x is HW = ceil(h / 64) words, word x * HW + yw holds rows
// 64 yw .. of it (bit b = row 64 yw + b; the bits past the column's end are 0), so the words in index order ARE the flat array in order
// and a column's last word has nb = h - 64 (HW - 1) valid bits.  A run starts at a 1 whose flat predecessor is 0 (or missing) and ends at a
// 1 whose flat successor is 0 (or missing); the k-th end closes the k-th start, and the start of a run is the last start at or before its
// end - inside the end's word, or carried: the largest start position of the words before it.
struct RleGeo {
  int h, HW, nb_last;      // nb_last: valid bits of a column's last word
  int64_t words;           // w * HW
};

__global__ __launch_bounds__(256) void rle_pack_kernel(const uint8_t* __restrict__ img, int h, int w, int HW, int tiles_x,
                                                       unsigned long long* __restrict__ words) {
  __shared__ uint8_t tileT[64][68];      // [x][y]; a wave writes one y of 64 x: 17 dwords apart, every bank once per half wave
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int64_t y0 = (int64_t)ty * 64, x0 = (int64_t)tx * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 4
  for (int rr = wave; rr < 64; rr += 4) {
    const int64_t y = y0 + rr, x = x0 + lane;
    uint8_t v = 0;
    if (y < h && x < w) v = img[y * w + x] != 0;      // a wave reads 64 consecutive bytes of an image row
    tileT[lane][rr] = v;
  }
  __syncthreads();
  // (the trip count is the same in every lane of a wave: the ballot is called by all 64)
  for (int c = wave; c < 64; c += 4) {
    const unsigned long long b = __ballot(tileT[c][lane] != 0);
    if (lane == 0 && x0 + c < w) words[(x0 + c) * HW + ty] = b;
  }
}

// word i of the stream: its run starts s, run ends e and the flat index of its bit 0
__device__ __forceinline__ void rle_word_edges(const unsigned long long* __restrict__ words, int64_t i, const RleGeo g, unsigned long long& s,
                                               unsigned long long& e, int64_t& base) {
  s = e = 0ull;
  base = 0;
  if (i >= g.words) return;
  const int64_t x = i / g.HW;
  const int yw = (int)(i - x * g.HW);
  base = x * g.h + (int64_t)yw * 64;
  const unsigned long long v = words[i];
  const int nb = yw == g.HW - 1 ? g.nb_last : 64;
  unsigned long long prev = 0ull, next = 0ull;
  if (i > 0) prev = (words[i - 1] >> ((yw == 0 ? g.nb_last : 64) - 1)) & 1ull;      // (the word before the first of a column is a last one)
  if (i + 1 < g.words) next = words[i + 1] & 1ull;
  s = v & ~((v << 1) | prev);
  e = v & ~((v >> 1) | (next << (nb - 1)));
}

// per workgroup of 256 words: how many runs end in it, and the position of its last run start (-1: none)
__global__ __launch_bounds__(RLE_THREADS) void rle_count_kernel(const unsigned long long* __restrict__ words, const RleGeo g,
                                                                int* __restrict__ block_ends, int* __restrict__ block_last) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  unsigned long long s, e;
  int64_t base;
  rle_word_edges(words, (int64_t)blockIdx.x * RLE_THREADS + threadIdx.x, g, s, e, base);
  const int last = s ? (int)(base + 63 - __clzll((long long)s)) : -1;
  int es, em, ts, tm;
  rle_block_scan(__popcll(e), last, sa, sm, es, em, ts, tm);
  if (threadIdx.x == 0) {
    block_ends[blockIdx.x] = ts;
    block_last[blockIdx.x] = tm;
  }
}

__global__ __launch_bounds__(RLE_THREADS) void rle_write_kernel(const unsigned long long* __restrict__ words, const RleGeo g,
                                                                const int* __restrict__ ends_before, const int* __restrict__ carry,
                                                                int* __restrict__ runs) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  unsigned long long s, e;
  int64_t base;
  rle_word_edges(words, (int64_t)blockIdx.x * RLE_THREADS + threadIdx.x, g, s, e, base);
  const int last = s ? (int)(base + 63 - __clzll((long long)s)) : -1;
  int es, em, ts, tm;
  rle_block_scan(__popcll(e), last, sa, sm, es, em, ts, tm);
  int64_t k = (int64_t)ends_before[blockIdx.x] + es;
  const int open = max(carry[blockIdx.x], em);      // the start of a run that was open when this word began
  while (e) {
    const int b = __ffsll((long long)e) - 1;
    e &= e - 1;
    const unsigned long long at_or_below = s & (b == 63 ? ~0ull : ((2ull << b) - 1ull));
    const int start = at_or_below ? (int)(base + 63 - __clzll((long long)at_or_below)) : open;
    runs[2 * k] = start + 1;
    runs[2 * k + 1] = (int)(base + b) - start + 1;
    ++k;
  }
}

static inline int64_t rle_words(int64_t h, int64_t w) { return w * ((h + 63) / 64); }
static inline int64_t rle_blocks(int64_t words) { return (words + RLE_THREADS - 1) / RLE_THREADS; }
static inline size_t rle_workspace_bytes(int64_t h, int64_t w) {
  const int64_t words = rle_words(h, w);
  return (size_t)(words * 8 + ((rle_blocks(words) * 4 * (int64_t)sizeof(int) + 15) / 16) * 16);
}

extern "C" size_t stp_mask_rle_workspace_bytes(int32_t h, int32_t w) {
  if (h <= 0 || w <= 0 || (int64_t)h * w >= (1ll << 31)) return 0;
  return rle_workspace_bytes(h, w);
}

extern "C" int stp_mask_rle(const uint8_t* img, int32_t h, int32_t w, int32_t* runs, int32_t* count, int64_t capacity, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (!img || !runs || !count || !workspace || h <= 0 || w <= 0 || (int64_t)h * w >= (1ll << 31)) return STP_E_BADARG;
  if (capacity < ((int64_t)h * w + 1) / 2) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return STP_E_BADARG;
  if (workspace_bytes < rle_workspace_bytes(h, w)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  RleGeo g;
  g.h = h;
  g.HW = (h + 63) / 64;
  g.nb_last = h - 64 * (g.HW - 1);
  g.words = rle_words(h, w);
  const int64_t tiles_x = ((int64_t)w + 63) / 64;
  const int blocks = (int)rle_blocks(g.words);      // (< 2^31 / 64 / 256 + w: fits)
  unsigned long long* words = (unsigned long long*)workspace;
  int* block_ends = (int*)(words + g.words);
  int *block_last = block_ends + blocks, *ends_before = block_last + blocks, *carry = ends_before + blocks;
  hipLaunchKernelGGL(rle_pack_kernel, dim3((unsigned)(tiles_x * g.HW)), dim3(256), 0, st, img, h, w, g.HW, (int)tiles_x, words);
  hipLaunchKernelGGL(rle_count_kernel, dim3(blocks), dim3(RLE_THREADS), 0, st, words, g, block_ends, block_last);
  hipLaunchKernelGGL(rle_scan_kernel, dim3(1), dim3(RLE_THREADS), 0, st, block_ends, block_last, blocks, ends_before, carry, count);
  hipLaunchKernelGGL(rle_write_kernel, dim3(blocks), dim3(RLE_THREADS), 0, st, words, g, ends_before, carry, runs);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

// ------------------------------------------------------------------------------------------------ threshold sweep counters
#define THR_MAX 64
#define THR_THREADS 1024
#define THR_MAX_BLOCKS 256          // one workgroup per CU; stp_threshold_counts_workspace_bytes() covers 256 tables

struct ThrTable {
  float v[THR_MAX];
};

// table[j][g]: pixels with exactly j thresholds below their value (a NaN: 0) and g = (target != 0)
__global__ __launch_bounds__(THR_THREADS) void threshold_counts_kernel(const float* __restrict__ map, const uint8_t* __restrict__ target,
                                                                       int64_t pixels, int C, int channel, int T, const ThrTable thr,
                                                                       int* __restrict__ partial) {
  __shared__ int table[(THR_MAX + 1) * 2];
  __shared__ float sthr[THR_MAX];
  const int entries = (T + 1) * 2;
  for (int e = threadIdx.x; e < entries; e += THR_THREADS) table[e] = 0;
  if (threadIdx.x < T) sthr[threadIdx.x] = thr.v[threadIdx.x];
  __syncthreads();
  // (the trip count is the same in every lane of a wave: wave_count is called by all 64)
  for (int64_t base = (int64_t)blockIdx.x * THR_THREADS; base < pixels; base += (int64_t)gridDim.x * THR_THREADS) {
    const int64_t i = base + threadIdx.x;
    int key = -1;
    if (i < pixels) {
      const float v = map[i * C + channel];
      int j = 0;
      for (int t = 0; t < T; ++t) j += v > sthr[t];
      key = j * 2 + (target[i] != 0);
    }
    wave_count(table, key);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < entries; e += THR_THREADS) partial[(size_t)blockIdx.x * entries + e] = table[e];
}

// sums the workgroup tables, then counts[t] = the suffix sums over j > t.  One workgroup: thread (slice, e) adds tables slice, slice +
// THR_SLICES, ... of entry e with several loads in flight, the slices meet in LDS
#define THR_ENTRIES ((THR_MAX + 1) * 2)
#define THR_SLICES 7          // 7 * 130 threads of 1024
__global__ __launch_bounds__(1024) void threshold_counts_finalize_kernel(const int* __restrict__ partial, int blocks, int T, int64_t pixels,
                                                                         int64_t* __restrict__ counts, int64_t* __restrict__ totals) {
  __shared__ long long part[THR_SLICES][THR_ENTRIES];
  __shared__ long long sum[THR_ENTRIES];
  const int entries = (T + 1) * 2;
  const int slice = threadIdx.x / THR_ENTRIES, e = threadIdx.x - slice * THR_ENTRIES;
  if (slice < THR_SLICES) {
    long long a = 0;
    if (e < entries) {
#pragma unroll 8
      for (int b = slice; b < blocks; b += THR_SLICES) a += partial[(size_t)b * entries + e];
    }
    part[slice][e] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < entries) {
    long long a = 0;
#pragma unroll
    for (int k = 0; k < THR_SLICES; ++k) a += part[k][threadIdx.x];
    sum[threadIdx.x] = a;
  }
  __syncthreads();
  if ((int)threadIdx.x < T) {
    long long above = 0, hit = 0;
    for (int j = threadIdx.x + 1; j <= T; ++j) above += sum[2 * j] + sum[2 * j + 1], hit += sum[2 * j + 1];
    counts[2 * threadIdx.x] = above;
    counts[2 * threadIdx.x + 1] = hit;
  }
  if (threadIdx.x == 0) {
    long long positives = 0;
    for (int j = 0; j <= T; ++j) positives += sum[2 * j + 1];
    totals[0] = positives;
    totals[1] = pixels;
  }
}

static inline size_t thr_workspace_bytes(int T) { return (size_t)THR_MAX_BLOCKS * (T + 1) * 2 * sizeof(int); }

extern "C" size_t stp_threshold_counts_workspace_bytes(int32_t T) {
  if (T < 1 || T > THR_MAX) return 0;
  return thr_workspace_bytes(T);
}

extern "C" int stp_threshold_counts(const float* map, const uint8_t* target, int32_t h, int32_t w, int32_t C, int32_t channel,
                                    const float* thresholds, int32_t T, int64_t* counts, int64_t* totals, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  if (!map || !target || !thresholds || !counts || !totals || !workspace || h <= 0 || w <= 0 || C <= 0 || channel < 0 || channel >= C || T < 1 ||
      T > THR_MAX)
    return STP_E_BADARG;
  if ((int64_t)h * w >= (1ll << 40)) return STP_E_BADARG;      // (a workgroup's int32 table: at most pixels / 256 + 1024 pixels each)
  ThrTable thr;
  for (int t = 0; t < THR_MAX; ++t) thr.v[t] = 0.f;
  for (int t = 0; t < T; ++t) {
    const float v = thresholds[t];      // (a HOST pointer)
    if (!(fabsf(v) <= 3.402823466e38f) || (t > 0 && !(v > thresholds[t - 1]))) return STP_E_BADARG;      // finite and strictly ascending
    thr.v[t] = v;
  }
  if (workspace_bytes < thr_workspace_bytes(T)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int64_t pixels = (int64_t)h * w;
  const int64_t want = (pixels + THR_THREADS - 1) / THR_THREADS;
  const int blocks = (int)(want > THR_MAX_BLOCKS ? THR_MAX_BLOCKS : want);
  int* partial = (int*)workspace;
  hipLaunchKernelGGL(threshold_counts_kernel, dim3(blocks), dim3(THR_THREADS), 0, st, map, target, pixels, C, channel, T, thr, partial);
  hipLaunchKernelGGL(threshold_counts_finalize_kernel, dim3(1), dim3(1024), 0, st, partial, blocks, T, pixels, counts, totals);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
