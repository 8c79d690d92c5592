// Splitting touching objects on the device (segmentation_pipeline/segmentation.py: predict_instances / score_instances / find_split): the
// exact squared Euclidean distance transform of ONE uint8 mask [h, w], its cores {D2 > c2}, and the growth of numbered seeds through
// the mask.  uint8, uint16, int32 only; every result is exact integer work and equals its host statement (tests/_split_reference.py)
// bit for bit.  h, w <= SPLIT_MAX_DIM = 32767 (D2 <= 2 * 32766^2 < 2^31 - 1, the value that means "no background") and h * w < 2^31.
//
// No workgroup reads what another workgroup writes in the same launch, none waits for another, and there is no atomic: what a launch
// needs from other workgroups was written by an earlier launch on the same stream.
//
//   stp_mask_edt       2 launches.  edt_rows_kernel: one wave per row walks it in 64-pixel segments, left to right and back; the
//                      nearest zero at or before / after a lane falls out of the segment's ballot, the nearest zero of the segments
//                      already passed is carried in a register.  G[y][x] = |x - nearest zero of row y| as uint16 (0xffff: the row has
//                      none).  edt_cols_kernel: a workgroup owns 32 columns x 64 rows and holds ITS 32 COLUMNS OF G, all h rows, in LDS
//                      (64 bytes per row; h <= 1024 - taller images read G from global memory, the same code); a pixel starts from
//                      best = G^2 of its own row and looks at the rows dy = 1, 2, ... above and below while dy * dy < best - the exact
//                      minimum without a lower envelope; a background pixel (best = 0) looks at nothing.
//   stp_edt_threshold  out = D2 > c2: 1 launch.
//   stp_label_grow     1 + SPLIT_GROW_ROUNDS launches: labels = seeds on the foreground, then synchronous rounds that ping-pong
//                      between `labels` and the workspace.  Round r reads flag[r - 1], written by round r - 1: 0 - the state is final,
//                      the round does nothing; else every pixel is written (an unlabelled foreground pixel takes the smallest non-zero
//                      label among its 8 neighbours) and a workgroup that changed a pixel stores 1 to flag[r].  The last round's flag
//                      is *changed.  An even number of rounds: the newest state is always in `labels`.
//   stp_label_unclaimed, stp_label_merge   the two steps that number the components no core reached: 1 launch each.
#include "common.h"

#define SPLIT_THREADS 256
#define SPLIT_MAX_DIM 32767
#define SPLIT_NO_BACKGROUND 0x7fffffff
#define SPLIT_GROW_ROUNDS 32          // (even)
#define EDT_NONE 0xffffu              // G of a row without a zero
#define EDT_STRIP 32                  // columns of a workgroup of edt_cols_kernel
#define EDT_ROWS 64                   // rows of a workgroup of edt_cols_kernel
#define EDT_LDS_ROWS 1024             // the tallest strip LDS holds: 1024 rows x 32 columns x 2 bytes = 64 KB

// One wave per row.  Forward: the distance to the nearest zero at or left of x (EDT_NONE: none yet); backward: the minimum with the
// distance to the nearest zero at or right of x.  A lane re-reads only what it wrote itself.
__global__ __launch_bounds__(SPLIT_THREADS) void edt_rows_kernel(const uint8_t* __restrict__ img, int h, int w, uint16_t* __restrict__ G) {
  const int lane = threadIdx.x & 63;
  const int y = blockIdx.x * (SPLIT_THREADS / 64) + (threadIdx.x >> 6);
  if (y >= h) return;      // (the same in every lane of a wave: the ballots are called by all 64)
  const uint8_t* row = img + (int64_t)y * w;
  uint16_t* g = G + (int64_t)y * w;
  const int segs = (w + 63) / 64;
  int last = -1;           // the last zero of the segments already passed
  for (int s = 0; s < segs; ++s) {
    const int x = s * 64 + lane;
    const bool zero = x < w && row[x] == 0;
    const unsigned long long z = __ballot(zero);
    const unsigned long long upto = z & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    const int near = upto ? s * 64 + 63 - __clzll((long long)upto) : last;
    if (x < w) g[x] = (uint16_t)(near >= 0 ? x - near : EDT_NONE);
    if (z) last = s * 64 + 63 - __clzll((long long)z);
  }
  int next = -1;           // the first zero of the segments already passed, coming from the right
  for (int s = segs - 1; s >= 0; --s) {
    const int x = s * 64 + lane;
    const bool zero = x < w && row[x] == 0;
    const unsigned long long z = __ballot(zero);
    const unsigned long long from = z >> lane;
    const int near = from ? x + __ffsll((long long)from) - 1 : next;
    if (x < w && near >= 0) {
      const unsigned d = (unsigned)(near - x);
      if (d < g[x]) g[x] = (uint16_t)d;
    }
    if (z) next = s * 64 + __ffsll((long long)z) - 1;
  }
}

// G^2 + dy^2 of one row of the strip, SPLIT_NO_BACKGROUND where that row has no zero
__device__ __forceinline__ int edt_candidate(unsigned g, int dy2) { return g == EDT_NONE ? SPLIT_NO_BACKGROUND : (int)(g * g) + dy2; }

// 256 threads = 32 columns x 8 rows, each thread 8 pixels of its column.  LDS: the strip's h rows of 32 uint16 (columns past w hold
// EDT_NONE and are never asked for).
template <bool LDS> __global__ __launch_bounds__(SPLIT_THREADS) void edt_cols_kernel(const uint16_t* __restrict__ G, int h, int w, int strips,
                                                                                   int* __restrict__ D2) {
  extern __shared__ uint16_t strip[];      // [h][EDT_STRIP] when LDS
  const int sx = blockIdx.x % strips, sy = blockIdx.x / strips;
  const int x0 = sx * EDT_STRIP, y0 = sy * EDT_ROWS;
  const int tx = threadIdx.x & (EDT_STRIP - 1), ty = threadIdx.x / EDT_STRIP;
  const int x = x0 + tx;
  if (LDS) {
    for (int r = ty; r < h; r += SPLIT_THREADS / EDT_STRIP) strip[r * EDT_STRIP + tx] = x < w ? G[(int64_t)r * w + x] : (uint16_t)EDT_NONE;
    __syncthreads();
  }
  if (x >= w) return;
  for (int y = y0 + ty; y < min(y0 + EDT_ROWS, h); y += SPLIT_THREADS / EDT_STRIP) {
    int best = edt_candidate(LDS ? strip[y * EDT_STRIP + tx] : G[(int64_t)y * w + x], 0);
    for (int dy = 1; dy < h; ++dy) {
      const int dy2 = dy * dy;
      if (dy2 >= best) break;
      const int up = y - dy, down = y + dy;
      if (up < 0 && down >= h) break;
      if (up >= 0) best = min(best, edt_candidate(LDS ? strip[up * EDT_STRIP + tx] : G[(int64_t)up * w + x], dy2));
      if (down < h) best = min(best, edt_candidate(LDS ? strip[down * EDT_STRIP + tx] : G[(int64_t)down * w + x], dy2));
    }
    D2[(int64_t)y * w + x] = best;
  }
}

__global__ __launch_bounds__(SPLIT_THREADS) void edt_threshold_kernel(const int* __restrict__ D2, int64_t n, int c2, uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
  if (i < n) out[i] = D2[i] > c2;
}

// labels = seeds on the foreground, 0 off it (a thread reads and writes its own pixel: seeds == labels is fine); flag[0] = 1 (the
// first round runs), flag[1 .. rounds - 1] = 0 and *changed = 0.
__global__ __launch_bounds__(SPLIT_THREADS) void grow_init_kernel(const uint8_t* __restrict__ mask, const int* seeds, int64_t n, int* labels,
                                                                 int* __restrict__ flags, int rounds, int* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
  if (i < n) labels[i] = mask[i] != 0 ? seeds[i] : 0;
  if (blockIdx.x == 0) {
    if (threadIdx.x < rounds) flags[threadIdx.x] = threadIdx.x == 0;
    if (threadIdx.x == 0) *changed = 0;
  }
}

// One synchronous round src -> dst.  `before` and `after` were / are written by other launches only.
__global__ __launch_bounds__(SPLIT_THREADS) void grow_round_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ src, int h, int w,
                                                                  int* __restrict__ dst, const int* __restrict__ before, int* __restrict__ after) {
  if (*before == 0) return;      // (the same for every thread of the launch)
  const int64_t n = (int64_t)h * w;
  const int64_t i = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
  int took = 0;
  if (i < n) {
    int v = src[i];
    if (v == 0 && mask[i] != 0) {
      const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
      int best = 0x7fffffff;
      for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= h) continue;
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = x + dx;
          if (xx < 0 || xx >= w) continue;
          const int u = src[(int64_t)yy * w + xx];      // (0 off the foreground and on the pixel itself)
          if (u != 0) best = min(best, u);
        }
      }
      if (best != 0x7fffffff) {
        v = best;
        took = 1;
      }
    }
    dst[i] = v;
  }
  if (__syncthreads_or(took) && threadIdx.x == 0) *after = 1;
}

// the foreground pixels no core reached
__global__ __launch_bounds__(SPLIT_THREADS) void unclaimed_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, int64_t n,
                                                                 uint8_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
  if (i < n) out[i] = mask[i] != 0 && labels[i] == 0;
}

// labels = rest + *nc where rest != 0; *total = *nc + *nr (total is neither nc nor nr: both are only read here)
__global__ __launch_bounds__(SPLIT_THREADS) void merge_kernel(const int* __restrict__ rest, int64_t n, const int* __restrict__ nc,
                                                             const int* __restrict__ nr, int* __restrict__ labels, int* __restrict__ total) {
  const int64_t i = (int64_t)blockIdx.x * SPLIT_THREADS + threadIdx.x;
  const int base = *nc;
  if (i < n) {
    const int r = rest[i];
    if (r != 0) labels[i] = r + base;
  }
  if (i == 0) *total = base + *nr;
}

static inline bool split_size_ok(int32_t h, int32_t w) {
  return h > 0 && w > 0 && h <= SPLIT_MAX_DIM && w <= SPLIT_MAX_DIM && (int64_t)h * w < (1ll << 31);
}
static inline unsigned split_blocks(int64_t n) { return (unsigned)((n + SPLIT_THREADS - 1) / SPLIT_THREADS); }
static inline int64_t split_round16(int64_t v) { return (v + 15) / 16 * 16; }
static inline size_t edt_workspace_bytes(int64_t n) { return (size_t)split_round16(n * 2); }
static inline size_t grow_workspace_bytes(int64_t n) { return (size_t)(split_round16(n * 4) + split_round16(SPLIT_GROW_ROUNDS * 4)); }

extern "C" size_t stp_mask_edt_workspace_bytes(int32_t h, int32_t w) {
  if (!split_size_ok(h, w)) return 0;
  return edt_workspace_bytes((int64_t)h * w);
}

extern "C" int stp_mask_edt(const uint8_t* img, int32_t h, int32_t w, int32_t* d2, void* workspace, size_t workspace_bytes, void* stream) {
  if (!img || !d2 || !workspace || !split_size_ok(h, w)) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  if (workspace_bytes < edt_workspace_bytes(n)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  uint16_t* G = (uint16_t*)workspace;
  hipLaunchKernelGGL(edt_rows_kernel, dim3((unsigned)((h + 3) / 4)), dim3(SPLIT_THREADS), 0, st, img, h, w, G);
  const int strips = (w + EDT_STRIP - 1) / EDT_STRIP, chunks = (h + EDT_ROWS - 1) / EDT_ROWS;      // (strips * chunks < 2^21)
  if (h <= EDT_LDS_ROWS)
    hipLaunchKernelGGL(edt_cols_kernel<true>, dim3((unsigned)(strips * chunks)), dim3(SPLIT_THREADS), (size_t)h * EDT_STRIP * sizeof(uint16_t), st,
                       G, h, w, strips, d2);
  else
    hipLaunchKernelGGL(edt_cols_kernel<false>, dim3((unsigned)(strips * chunks)), dim3(SPLIT_THREADS), 0, st, G, h, w, strips, d2);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_edt_threshold(const int32_t* d2, int32_t h, int32_t w, int32_t c2, uint8_t* out, void* stream) {
  if (!d2 || !out || !split_size_ok(h, w) || c2 < 0) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(edt_threshold_kernel, dim3(split_blocks(n)), dim3(SPLIT_THREADS), 0, (hipStream_t)stream, d2, n, c2, out);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" size_t stp_label_grow_workspace_bytes(int32_t h, int32_t w) {
  if (!split_size_ok(h, w)) return 0;
  return grow_workspace_bytes((int64_t)h * w);
}

extern "C" int32_t stp_label_grow_rounds(void) { return SPLIT_GROW_ROUNDS; }

extern "C" int stp_label_grow(const uint8_t* mask, const int32_t* seeds, int32_t h, int32_t w, int32_t* labels, int32_t* changed, void* workspace,
                              size_t workspace_bytes, void* stream) {
  if (!mask || !seeds || !labels || !changed || !workspace || !split_size_ok(h, w)) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  if (workspace_bytes < grow_workspace_bytes(n)) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int* other = (int*)workspace;
  int* flags = (int*)((char*)workspace + split_round16(n * 4));      // flag[r]: the rounds up to r left something for round r + 1
  const unsigned blocks = split_blocks(n);
  hipLaunchKernelGGL(grow_init_kernel, dim3(blocks), dim3(SPLIT_THREADS), 0, st, mask, seeds, n, labels, flags, SPLIT_GROW_ROUNDS, changed);
  for (int r = 1; r <= SPLIT_GROW_ROUNDS; ++r) {
    const int* src = (r & 1) ? labels : other;
    int* dst = (r & 1) ? other : labels;
    int* after = r == SPLIT_GROW_ROUNDS ? changed : flags + r;
    hipLaunchKernelGGL(grow_round_kernel, dim3(blocks), dim3(SPLIT_THREADS), 0, st, mask, src, h, w, dst, (const int*)(flags + r - 1), after);
  }
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_label_unclaimed(const uint8_t* mask, const int32_t* labels, int32_t h, int32_t w, uint8_t* out, void* stream) {
  if (!mask || !labels || !out || !split_size_ok(h, w)) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(unclaimed_kernel, dim3(split_blocks(n)), dim3(SPLIT_THREADS), 0, (hipStream_t)stream, mask, labels, n, out);
  STP_LAUNCH_CHECK();
  return STP_OK;
}

extern "C" int stp_label_merge(const int32_t* rest, const int32_t* nc, const int32_t* nr, int32_t h, int32_t w, int32_t* labels, int32_t* total,
                               void* stream) {
  if (!rest || !nc || !nr || !labels || !total || total == nc || total == nr || rest == labels || !split_size_ok(h, w)) return STP_E_BADARG;
  const int64_t n = (int64_t)h * w;
  hipLaunchKernelGGL(merge_kernel, dim3(split_blocks(n)), dim3(SPLIT_THREADS), 0, (hipStream_t)stream, rest, n, nc, nr, labels, total);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
