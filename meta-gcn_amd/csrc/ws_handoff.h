// The LDS counter hand-off of the warp-specialised kernels (fused_wide.hip,
// fused_dws.hip, fused_fwd_ws.hip): monotonic counters in LDS, polled with a
// bounded spin; a spin that runs past its bound sets the workgroup's abort
// word and every wave leaves its loop (internal, device code only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mgcn {
namespace {

__device__ __forceinline__ int lds_load(const int *p) {
  return __builtin_amdgcn_readfirstlane(
      __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

// wait until *p >= target (false: the abort word is set, leave)
__device__ __forceinline__ bool lds_wait_ge(const int *p, int target, int *abort_word,
                                            uint32_t limit) {
  for (uint32_t n = 0;; ++n) {
    if (lds_load(p) >= target) break;
    if (lds_load(abort_word) != 0) return false;
    if (n >= limit) {
      __hip_atomic_store(abort_word, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      return false;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  asm volatile("" ::: "memory");
  return true;
}

// this wave's LDS writes complete, then lane 0 adds v to *p; returns the old value
__device__ __forceinline__ int lds_signal(int *p, int v, int lane) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int old = 0;
  if (lane == 0) old = __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return __builtin_amdgcn_readfirstlane(old);
}

}  // namespace
}  // namespace mgcn
