// Host-side launch helpers every .hip file may include: the one CU query, and the one place that launches a kernel whose
// dynamic LDS may exceed the 64 KB a kernel gets by default.
//
// A kernel that asks for more than 64 KB of dynamic LDS needs its hipFuncAttributeMaxDynamicSharedMemorySize raised to that size before
// its first launch.  stp_launch_lds() keeps the largest size granted so far PER KERNEL FUNCTION POINTER - the pointer that is
// launched is the key, so an arm that selects another instantiation cannot inherit a neighbour's grant - and raises the grant only when
// a launch needs more than 64 KB and more than it has.  The grant is per process (one process per device), as the flags it replaces were.
#pragma once
#include "common.h"
#include <mutex>
#include <unordered_map>
#include <utility>

// (hidden: one copy per library, nothing added to its exported symbols)
#define STP_LIB_LOCAL inline __attribute__((visibility("hidden")))

STP_LIB_LOCAL int stp_cu_count() {
  static const int cus = [] {
    int d = 0, n = 0;
    if (hipGetDevice(&d) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n <= 0) n = 256;
    return n;      // MI355X (also the answer on a build host without a GPU: plan sizes must not depend on where they are computed)
  }();
  return cus;
}

constexpr size_t STP_LDS_DEFAULT = 64 * 1024;      // dynamic LDS a kernel may use without the attribute

// Raise kern's dynamic-LDS grant to `want` bytes if it is below it.  One table per library, behind a mutex: ctypes releases the GIL,
// so two host threads may launch at once.
STP_LIB_LOCAL bool stp_lds_grant(const void* kern, size_t want) {
  static std::mutex mu;
  static std::unordered_map<const void*, size_t> granted;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = granted[kern];
  if (want <= have) return true;
  if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)want) != hipSuccess) return false;
  have = want;
  return true;
}

// Launch kern with `lds` bytes of dynamic LDS; returns STP_OK or STP_E_LAUNCH.  `reserve`: the grant to ask for when one is needed
// (a site whose LDS size varies per launch asks once for its ceiling); max(lds, reserve) <= 64 KB touches neither table nor mutex.
template <typename... P, typename... A>
static inline int stp_launch_lds_reserve(void (*kern)(P...), size_t reserve, dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args) {
  const size_t want = lds > reserve ? lds : reserve;
  if (want > STP_LDS_DEFAULT && !stp_lds_grant(reinterpret_cast<const void*>(kern), want)) return STP_E_LAUNCH;
  hipLaunchKernelGGL(kern, grid, block, lds, s, std::forward<A>(args)...);
  STP_LAUNCH_CHECK();
  return STP_OK;
}
template <typename... P, typename... A>
static inline int stp_launch_lds(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, A&&... args) {
  return stp_launch_lds_reserve(kern, 0, grid, block, lds, s, std::forward<A>(args)...);
}
