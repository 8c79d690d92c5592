// Boundary scores of two masks on the device (segmentation_pipeline/segmentation.py: surface_distances, score_boundaries,
// find_boundary_threshold): the counters behind the Hausdorff distance, its percentile form (HD95), the average symmetric surface distance
// and the boundary F-score / surface Dice at pixel tolerances.  uint8, uint16, int32 and int64 only; every result is exact integer work,
// equals its host statement (tests/_boundary_reference.py) and is the same from run to run: all that workgroups exchange are integer sums
// and maxima.  1 <= h, w <= 32767, the limits of stp_mask_edt (D2 < 2^31 - 1, the value that means "the other surface is empty").
//
// No workgroup waits for another: what a launch needs from other workgroups was written by an earlier launch on the same stream.
//   bd_clear_kernel    zeroes the state block (counters, cursor, select state, the five digit histograms)
//   bd_surface_kernel  both masks in one launch.  A wave owns 64 consecutive pixels of a row: the left / right neighbours are the wave's
//                      ballot shifted by one lane (lanes 0 and 63 read the pixel across the segment's edge), up / down come from the rows
//                      above and below, outside the image is background.  Writes the image stp_mask_edt wants - 0 on the surface, 1
//                      elsewhere - and adds the workgroup's surface counts (one barrier count per mask, one atomicAdd each).
//   stp_mask_edt       twice: D2 to the truth surface and D2 to the pred surface, every pixel.
//   bd_reduce_kernel   a workgroup owns BD_CHUNK consecutive pixels.  A surface pixel of either mask reads the other image's D2 and keeps
//                      max and sum q in registers; within[k] is a ballot popcount that lane k keeps.  The values are appended to ONE list
//                      (ballot + prefix popcount, one cursor atomicAdd per wave and step; the order is unspecified) and counted into the
//                      first digit histogram, private to each wave in LDS.  Per workgroup: one LDS merge, then one integer atomic per
//                      non-zero counter and histogram bin.  Returns at once when a surface is empty: every distance is "none".
//   radix select       of the ranks j and min(j + 1, n - 1) over the 31-bit values, digits of 11 + 10 + 10 bits.  bd_pick_kernel<P> (one
//                      workgroup) scans pass P's histogram in bin order and narrows (prefix, rank) for both ranks - pass 0 first forms j
//                      from the counts on the device -; bd_hist_kernel<P> counts the next digit of the listed values whose higher digits
//                      equal a prefix, into two histograms (one when both prefixes are equal).  Its grid covers the list's bound 2 h w;
//                      workgroups past the cursor return.  bd_pick_kernel<2> writes all of `out`.
#include "common.h"

#define BD_THREADS 256
#define BD_WAVES (BD_THREADS / 64)
#define BD_MAX_T 16
#define BD_MAX_DEN 1000
#define BD_MAX_DIM 32767
#define BD_CHUNK 4096                 // pixels (reduce) / listed values (histogram) per workgroup
#define BD_NONE 0x7fffffff            // stp_mask_edt's value when the image has no zero
#define BD_BINS0 2048                 // bits 30..20
#define BD_BINS 1024                  // bits 19..10, then 9..0

typedef unsigned long long bd_u64;

struct BdThresholds {
  int c2[BD_MAX_T];
};

// everything the launches exchange besides the images and the list; cleared by bd_clear_kernel
struct BdState {
  bd_u64 n[2];                        // surface pixels of pred, truth
  bd_u64 sumq[2];
  bd_u64 within[2][BD_MAX_T];
  bd_u64 cursor;                      // values in the list
  long long sel[3][4];                // after pass P: (prefix of rank lo, prefix of rank hi, rank lo, rank hi inside their prefixes)
  int maxd2[2];
  unsigned hist0[BD_BINS0];
  unsigned hist[2][2][BD_BINS];       // [pass - 1][which prefix][digit]
};

__global__ __launch_bounds__(BD_THREADS) void bd_clear_kernel(unsigned* __restrict__ words, int count) {
  const int i = blockIdx.x * BD_THREADS + threadIdx.x;
  if (i < count) words[i] = 0u;
}

// Is (y, x) a surface pixel of M: foreground with a 4-neighbour that is background or outside the image.  Called by all 64 lanes.
__device__ __forceinline__ bool bd_surface(const uint8_t* __restrict__ M, int h, int w, int y, int x, int lane) {
  const uint8_t* row = M + (int64_t)y * w;
  const bool c = x < w && row[x] != 0;
  const bd_u64 fg = __ballot(c);
  if (!c) return false;
  const bool l = lane > 0 ? ((fg >> (lane - 1)) & 1ull) != 0 : (x > 0 && row[x - 1] != 0);
  const bool r = lane < 63 ? ((fg >> (lane + 1)) & 1ull) != 0 : (x + 1 < w && row[x + 1] != 0);      // (a lane past w holds 0)
  const bool u = y > 0 && row[x - w] != 0;
  const bool d = y + 1 < h && row[x + w] != 0;
  return !(l && r && u && d);
}

__global__ __launch_bounds__(BD_THREADS) void bd_surface_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, int h, int w,
                                                                int segs, uint8_t* __restrict__ imgP, uint8_t* __restrict__ imgT,
                                                                BdState* __restrict__ s) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * BD_WAVES + (threadIdx.x >> 6);
  const bool live = item < (int64_t)h * segs;      // (a wave past the image stays for the ballots and the barriers: x = w, no pixel)
  const int y = live ? (int)(item / segs) : 0;
  const int x = live ? (int)(item - (int64_t)y * segs) * 64 + lane : w;
  const bool sp = bd_surface(pred, h, w, y, x, lane);
  const bool st = bd_surface(truth, h, w, y, x, lane);
  if (x < w) {
    const int64_t i = (int64_t)y * w + x;
    imgP[i] = sp ? 0 : 1;
    imgT[i] = st ? 0 : 1;
  }
  const int np = __syncthreads_count(sp);
  const int nt = __syncthreads_count(st);
  if (threadIdx.x == 0) {
    if (np) atomicAdd(&s->n[0], (bd_u64)np);
    if (nt) atomicAdd(&s->n[1], (bd_u64)nt);
  }
}

// floor(sqrt(v)) for v < 2^48, one bit per step: r * r <= v < (r + 1)^2 exactly
__device__ __forceinline__ bd_u64 bd_isqrt(bd_u64 v) {
  bd_u64 r = 0;
  for (int b = 23; b >= 0; --b) {
    const bd_u64 t = r | (1ull << b);
    if (t * t <= v) r = t;
  }
  return r;
}

__device__ __forceinline__ int bd_wave_max(int v) {
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ bd_u64 bd_wave_sum(bd_u64 v) {
  for (int o = 32; o > 0; o >>= 1) v += (bd_u64)__shfl_xor((long long)v, o);
  return v;
}

// the workgroup's per-wave histograms `priv` [BD_WAVES][bins] -> the global table, one atomicAdd per non-zero bin (after a barrier)
__device__ __forceinline__ void bd_hist_flush(const unsigned* priv, int bins, unsigned* __restrict__ table) {
  for (int b = threadIdx.x; b < bins; b += BD_THREADS) {
    unsigned c = 0;
    for (int wv = 0; wv < BD_WAVES; ++wv) c += priv[wv * bins + b];
    if (c) atomicAdd(table + b, c);
  }
}

__global__ __launch_bounds__(BD_THREADS) void bd_reduce_kernel(const uint8_t* __restrict__ imgP, const uint8_t* __restrict__ imgT,
                                                               const int* __restrict__ d2T, const int* __restrict__ d2P, int64_t n,
                                                               BdThresholds thr, int T, int* __restrict__ list, BdState* s) {
  __shared__ unsigned priv[BD_WAVES * BD_BINS0];
  __shared__ bd_u64 acc[2][1 + BD_MAX_T];      // sum q, within[k]
  __shared__ int top[2];
  if (s->n[0] == 0 || s->n[1] == 0) return;      // (the same for every thread of the launch; written by an earlier launch)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = threadIdx.x; b < BD_WAVES * BD_BINS0; b += BD_THREADS) priv[b] = 0u;
  if (threadIdx.x < 2 * (1 + BD_MAX_T)) acc[threadIdx.x / (1 + BD_MAX_T)][threadIdx.x % (1 + BD_MAX_T)] = 0ull;
  if (threadIdx.x < 2) top[threadIdx.x] = 0;
  __syncthreads();
  const bd_u64 below = (1ull << lane) - 1ull;
  int mx[2] = {0, 0};
  bd_u64 sq[2] = {0ull, 0ull};
  unsigned mine = 0;      // lane k: within[0][k], lane 16 + k: within[1][k], of this wave
  const int64_t base = (int64_t)blockIdx.x * BD_CHUNK;
  for (int it = 0; it < BD_CHUNK / BD_THREADS; ++it) {
    const int64_t i = base + it * BD_THREADS + threadIdx.x;
    bool a[2] = {false, false};
    int v[2] = {0, 0};
    if (i < n) {
      a[0] = imgP[i] == 0;
      a[1] = imgT[i] == 0;
      if (a[0]) v[0] = d2T[i];
      if (a[1]) v[1] = d2P[i];
    }
    const bd_u64 on[2] = {__ballot(a[0]), __ballot(a[1])};
    if (!(on[0] | on[1])) continue;      // (the same in every lane of the wave)
    long long start = 0;
    if (lane == 0) start = (long long)atomicAdd(&s->cursor, (bd_u64)(__popcll(on[0]) + __popcll(on[1])));
    start = __shfl(start, 0);
    for (int d = 0; d < 2; ++d) {
      for (int k = 0; k < T; ++k) {
        const int c = __popcll(__ballot(a[d] && v[d] <= thr.c2[k]));
        if (lane == d * BD_MAX_T + k) mine += (unsigned)c;
      }
      if (a[d]) {
        list[start + (d ? __popcll(on[0]) : 0) + __popcll(on[d] & below)] = v[d];
        mx[d] = max(mx[d], v[d]);
        sq[d] += bd_isqrt((bd_u64)v[d] << 16);
        atomicAdd(&priv[wave * BD_BINS0 + (v[d] >> 20)], 1u);
      }
    }
  }
  for (int d = 0; d < 2; ++d) {
    const int m = bd_wave_max(mx[d]);
    const bd_u64 q = bd_wave_sum(sq[d]);
    if (lane == 0) {
      atomicMax(&top[d], m);
      if (q) atomicAdd(&acc[d][0], q);
    }
  }
  if (lane < 2 * BD_MAX_T && mine) atomicAdd(&acc[lane / BD_MAX_T][1 + lane % BD_MAX_T], (bd_u64)mine);
  __syncthreads();
  if (threadIdx.x < 2 * (1 + BD_MAX_T)) {
    const int d = threadIdx.x / (1 + BD_MAX_T), k = threadIdx.x % (1 + BD_MAX_T);
    const bd_u64 c = acc[d][k];
    if (c) atomicAdd(k == 0 ? &s->sumq[d] : &s->within[d][k - 1], c);
  } else if (threadIdx.x < 2 * (1 + BD_MAX_T) + 2) {
    const int d = threadIdx.x - 2 * (1 + BD_MAX_T);
    if (top[d]) atomicMax(&s->maxd2[d], top[d]);
  }
  bd_hist_flush(priv, BD_BINS0, s->hist0);
}

// PASS 1: the digit of bits 19..10 of the values whose bits 30..20 equal a prefix; PASS 2: bits 9..0 under bits 30..10.
template <int PASS> __global__ __launch_bounds__(BD_THREADS) void bd_hist_kernel(const int* __restrict__ list, BdState* s) {
  __shared__ unsigned priv[BD_WAVES * 2 * BD_BINS];
  const long long total = (long long)s->cursor;
  const long long base = (long long)blockIdx.x * BD_CHUNK;
  if (base >= total) return;      // (the same for every thread of the workgroup)
  constexpr int shift = PASS == 1 ? 10 : 0;
  const long long p0 = s->sel[PASS - 1][0], p1 = s->sel[PASS - 1][1];
  const int wave = threadIdx.x >> 6;
  for (int b = threadIdx.x; b < BD_WAVES * 2 * BD_BINS; b += BD_THREADS) priv[b] = 0u;
  __syncthreads();
  for (int it = 0; it < BD_CHUNK / BD_THREADS; ++it) {
    const long long i = base + it * BD_THREADS + threadIdx.x;
    if (i >= total) break;
    const int key = list[i];
    const long long high = key >> (shift + 10);
    const int digit = (key >> shift) & (BD_BINS - 1);
    if (high == p0)
      atomicAdd(&priv[wave * 2 * BD_BINS + digit], 1u);      // (both ranks under one prefix: counted once, here)
    else if (high == p1)
      atomicAdd(&priv[wave * 2 * BD_BINS + BD_BINS + digit], 1u);
  }
  __syncthreads();
  bd_hist_flush(priv, 2 * BD_BINS, &s->hist[PASS - 1][0][0]);
}

// One workgroup.  Scans pass PASS's histogram(s) in bin order; for each of the two ranks: the bin that holds it, the rank inside the bin.
template <int PASS> __global__ __launch_bounds__(BD_THREADS) void bd_pick_kernel(BdState* s, int T, long long pct_num, long long pct_den,
                                                                                long long* __restrict__ out) {
  constexpr int bins = PASS == 0 ? BD_BINS0 : BD_BINS, bits = PASS == 0 ? 11 : 10, per = bins / BD_THREADS;
  __shared__ bd_u64 before[2][BD_THREADS];      // the values in the bins of the threads in front, per rank
  const long long n = (long long)(s->n[0] + s->n[1]);
  const bool none = s->n[0] == 0 || s->n[1] == 0;
  long long* tail = out + 2 * (3 + T);
  if (!none) {
    long long prefix[2], rank[2];
    if (PASS == 0) {
      const long long j = pct_num * (n - 1) / pct_den;
      prefix[0] = prefix[1] = 0;
      rank[0] = j;
      rank[1] = min(j + 1, n - 1);
    } else {
      for (int r = 0; r < 2; ++r) prefix[r] = s->sel[PASS - 1][r], rank[r] = s->sel[PASS - 1][2 + r];
    }
    const bool same = prefix[0] == prefix[1];
    const unsigned* table[2];
    for (int r = 0; r < 2; ++r) {
      table[r] = PASS == 0 ? s->hist0 : s->hist[PASS - 1][same ? 0 : r];
      bd_u64 c = 0;
      for (int b = 0; b < per; ++b) c += table[r][threadIdx.x * per + b];
      before[r][threadIdx.x] = c;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      bd_u64 run = 0;
      for (int t = 0; t < BD_THREADS; ++t) {
        const bd_u64 c = before[threadIdx.x][t];
        before[threadIdx.x][t] = run;
        run += c;
      }
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
      long long cum = (long long)before[r][threadIdx.x];
      for (int b = 0; b < per; ++b) {
        const long long c = table[r][threadIdx.x * per + b];
        if (rank[r] >= cum && rank[r] < cum + c) {      // (true in exactly one thread and bin)
          const long long key = (prefix[r] << bits) | (threadIdx.x * per + b);
          s->sel[PASS][r] = key;
          s->sel[PASS][2 + r] = rank[r] - cum;
          if (PASS == 2) tail[r] = key;
        }
        cum += c;
      }
    }
  }
  if (PASS == 2) {
    if (threadIdx.x < 2 * (3 + T)) {
      const int d = threadIdx.x / (3 + T), k = threadIdx.x % (3 + T);
      long long v;
      if (k == 0) v = (long long)s->n[d];
      else if (k == 1) v = none ? -1 : s->maxd2[d];
      else if (k == 2) v = (long long)s->sumq[d];
      else v = (long long)s->within[d][k - 3];
      out[threadIdx.x] = v;
    }
    if (threadIdx.x == 0) {
      if (none) tail[0] = tail[1] = -1;
      tail[2] = none ? 0 : pct_num * (n - 1) % pct_den;
    }
  }
}

static inline bool bd_size_ok(int32_t h, int32_t w) { return h > 0 && w > 0 && h <= BD_MAX_DIM && w <= BD_MAX_DIM; }
static inline int64_t bd_round16(int64_t v) { return (v + 15) / 16 * 16; }

// the workspace: the state, the two distance images, the list (every pixel may be on both surfaces), stp_mask_edt's row table, the two
// inverted surface images
struct BdPlan {
  int64_t n;
  BdState* state;
  int *d2T, *d2P, *list;
  void* edt;
  size_t edt_bytes;
  uint8_t *imgP, *imgT;
  size_t bytes;
};

static BdPlan bd_plan(int32_t h, int32_t w, void* workspace) {
  BdPlan p;
  p.n = (int64_t)h * w;
  char* at = (char*)workspace;
  p.state = (BdState*)at, at += bd_round16(sizeof(BdState));
  p.d2T = (int*)at, at += bd_round16(p.n * 4);
  p.d2P = (int*)at, at += bd_round16(p.n * 4);
  p.list = (int*)at, at += bd_round16(p.n * 8);
  p.edt_bytes = stp_mask_edt_workspace_bytes(h, w);
  p.edt = at, at += bd_round16((int64_t)p.edt_bytes);
  p.imgP = (uint8_t*)at, at += bd_round16(p.n);
  p.imgT = (uint8_t*)at, at += bd_round16(p.n);
  p.bytes = (size_t)(at - (char*)workspace);
  return p;
}

extern "C" size_t stp_surface_distances_workspace_bytes(int32_t h, int32_t w) {
  if (!bd_size_ok(h, w)) return 0;
  return bd_plan(h, w, nullptr).bytes;
}

extern "C" int stp_surface_distances(const uint8_t* pred, const uint8_t* truth, int32_t h, int32_t w, const int32_t* c2, int32_t T,
                                     int32_t pct_num, int32_t pct_den, int64_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!pred || !truth || !out || !workspace || !bd_size_ok(h, w)) return STP_E_BADARG;
  if (T < 0 || T > BD_MAX_T || (T > 0 && !c2) || pct_den < 1 || pct_den > BD_MAX_DEN || pct_num < 0 || pct_num > pct_den) return STP_E_BADARG;
  BdThresholds thr;
  for (int k = 0; k < BD_MAX_T; ++k) thr.c2[k] = 0;
  for (int k = 0; k < T; ++k) {
    if (c2[k] < 0 || (k > 0 && c2[k] <= c2[k - 1])) return STP_E_BADARG;
    thr.c2[k] = c2[k];
  }
  if ((reinterpret_cast<uintptr_t>(out) & 7u) != 0) return STP_E_BADARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0) return STP_E_WORKSPACE;
  const BdPlan p = bd_plan(h, w, workspace);
  if (workspace_bytes < p.bytes) return STP_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int words = (int)(sizeof(BdState) / 4);
  hipLaunchKernelGGL(bd_clear_kernel, dim3((unsigned)((words + BD_THREADS - 1) / BD_THREADS)), dim3(BD_THREADS), 0, st, (unsigned*)p.state, words);
  const int segs = (w + 63) / 64;
  const int64_t items = (int64_t)h * segs;
  hipLaunchKernelGGL(bd_surface_kernel, dim3((unsigned)((items + BD_WAVES - 1) / BD_WAVES)), dim3(BD_THREADS), 0, st, pred, truth, h, w, segs,
                     p.imgP, p.imgT, p.state);
  int rc = stp_mask_edt(p.imgT, h, w, p.d2T, p.edt, p.edt_bytes, stream);      // D2 to the truth surface, for the pixels of S(pred)
  if (rc == STP_OK) rc = stp_mask_edt(p.imgP, h, w, p.d2P, p.edt, p.edt_bytes, stream);
  if (rc != STP_OK) return rc;
  hipLaunchKernelGGL(bd_reduce_kernel, dim3((unsigned)((p.n + BD_CHUNK - 1) / BD_CHUNK)), dim3(BD_THREADS), 0, st, p.imgP, p.imgT, p.d2T, p.d2P,
                     p.n, thr, T, p.list, p.state);
  const dim3 list_grid((unsigned)((2 * p.n + BD_CHUNK - 1) / BD_CHUNK));      // the list holds at most 2 h w values; n is known on the device only
  long long* o = (long long*)out;
  hipLaunchKernelGGL(bd_pick_kernel<0>, dim3(1), dim3(BD_THREADS), 0, st, p.state, T, (long long)pct_num, (long long)pct_den, o);
  hipLaunchKernelGGL(bd_hist_kernel<1>, list_grid, dim3(BD_THREADS), 0, st, p.list, p.state);
  hipLaunchKernelGGL(bd_pick_kernel<1>, dim3(1), dim3(BD_THREADS), 0, st, p.state, T, (long long)pct_num, (long long)pct_den, o);
  hipLaunchKernelGGL(bd_hist_kernel<2>, list_grid, dim3(BD_THREADS), 0, st, p.list, p.state);
  hipLaunchKernelGGL(bd_pick_kernel<2>, dim3(1), dim3(BD_THREADS), 0, st, p.state, T, (long long)pct_num, (long long)pct_den, o);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
