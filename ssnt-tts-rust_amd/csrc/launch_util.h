// launch_util.h -- host-side launch glue shared by the kernel files: pointer alignment, the
// status of a launch, and the launch of a kernel whose dynamic LDS may exceed 64 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ssnt_internal.h"
#include "ssnt_tts_c.h"

namespace ssnt {

// p is a multiple of m (a power of two); null counts as aligned
inline bool aligned_to(const void* p, uintptr_t m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) == 0; }

// fwd-bwd tensors aligned: log_trans / grad to `pair` bytes, the f32-element ones to `scalar`
inline bool all_aligned(const FwdBwdArgs& a, uintptr_t pair, uintptr_t scalar, uintptr_t ws) {
  return aligned_to(a.log_trans, pair) && aligned_to(a.grad, pair) && aligned_to(a.log_obs, scalar) &&
         aligned_to(a.grad_obs, scalar) && aligned_to(a.log_alpha, scalar) &&
         aligned_to(a.log_beta, scalar) && aligned_to(a.workspace, ws);
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? SSNT_OK : SSNT_ERR_HIP; }

// Launch with `lds` bytes of dynamic LDS. Above 64 KiB the kernel needs its attribute raised (to
// `cap`, the caller's LDS budget); it is per device, so it is set on every such launch (a
// host-side call, no device work) rather than cached in a process-wide flag.
template <typename K, typename... A>
int launch_lds(K kern, dim3 grid, dim3 block, size_t lds, size_t cap, hipStream_t st, const A&... args) {
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)cap);
  hipLaunchKernelGGL(kern, grid, block, lds, st, args...);
  return launch_status();
}

}  // namespace ssnt
