// Integer counting into a workgroup's LDS table with the wave peel (class_confusion.hip, mask.hip): neighbouring pixels mostly share one
// key, so a wave first peels off up to WAVE_COUNT_PEEL distinct keys with one LDS add of a popcount each, and only lanes whose key is
// still unserved add on their own.  Integer adds: the table does not depend on the order.
#pragma once
#include "common.h"

#define WAVE_COUNT_PEEL 4

// every lane of the wave calls this (key < 0: no pixel): table[key] += 1 for each lane with a pixel
__device__ __forceinline__ void wave_count(int* table, int key) {
  const int lane = threadIdx.x & 63;
  unsigned long long rem = __ballot(key >= 0);
#pragma unroll 1
  for (int r = 0; r < WAVE_COUNT_PEEL && rem; ++r) {
    const int leader = __ffsll(rem) - 1;
    const int k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k);      // (k >= 0: lanes without a pixel never match; the leader always does)
    if (lane == leader) atomicAdd(table + k, __popcll(same));
    rem &= ~same;
  }
  if ((rem >> lane) & 1ull) atomicAdd(table + key, 1);
}
