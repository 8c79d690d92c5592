// The scans of the run-length launches (csrc/mask.hip: stp_mask_rle; csrc/components.hip: the root ranks of stp_mask_label and the runs
// of stp_label_rle): a fixed-order Hillis-Steele pass over the 256 threads' integers in LDS, and the one-workgroup kernel that scans the
// workgroups' totals in block order - no atomics, the same sums from run to run.
#pragma once
#include "common.h"

#define RLE_THREADS 256

// over the workgroup's 256 threads: the exclusive sum of `a` and the exclusive maximum of `m` (-1 for thread 0), and both totals
__device__ __forceinline__ void rle_block_scan(int a, int m, int (&sa)[RLE_THREADS], int (&sm)[RLE_THREADS], int& excl_sum, int& excl_max,
                                               int& total_sum, int& total_max) {
  const int t = threadIdx.x;
  sa[t] = a;
  sm[t] = m;
  __syncthreads();
  for (int off = 1; off < RLE_THREADS; off <<= 1) {
    const int xa = t >= off ? sa[t - off] : 0, xm = t >= off ? sm[t - off] : -1;
    __syncthreads();
    sa[t] += xa;
    sm[t] = max(sm[t], xm);
    __syncthreads();
  }
  excl_sum = sa[t] - a;
  excl_max = t > 0 ? sm[t - 1] : -1;
  total_sum = sa[RLE_THREADS - 1];
  total_max = sm[RLE_THREADS - 1];
  __syncthreads();      // (the arrays are free again)
}

// one workgroup, the blocks in order: ends_before[b] = runs that end before block b, carry[b] = the last run start before it; *count
// (static: both files that include this header launch their own copy)
static __global__ __launch_bounds__(RLE_THREADS) void rle_scan_kernel(const int* __restrict__ block_ends, const int* __restrict__ block_last,
                                                                      int blocks, int* __restrict__ ends_before, int* __restrict__ carry,
                                                                      int* __restrict__ count) {
  __shared__ int sa[RLE_THREADS], sm[RLE_THREADS];
  int run_sum = 0, run_max = -1;
  for (int b0 = 0; b0 < blocks; b0 += RLE_THREADS) {
    const int b = b0 + threadIdx.x;
    const int a = b < blocks ? block_ends[b] : 0, m = b < blocks ? block_last[b] : -1;
    int es, em, ts, tm;
    rle_block_scan(a, m, sa, sm, es, em, ts, tm);
    if (b < blocks) {
      ends_before[b] = run_sum + es;
      carry[b] = max(run_max, em);
    }
    run_sum += ts;
    run_max = max(run_max, tm);
  }
  if (threadIdx.x == 0) *count = run_sum;
}
