// Raw buffer loads/stores bound to the LLVM intrinsics by name. In this toolchain the clang
// builtins __builtin_amdgcn_raw_buffer_load_b64 / _b128 lower to a single buffer_load_dword
// (upper dwords undefined), so the wide forms are declared here instead.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

extern "C" __device__ float rbuf_ld1(__amdgpu_buffer_rsrc_t, int, int, int) __asm("llvm.amdgcn.raw.ptr.buffer.load.f32");
extern "C" __device__ f32x2 rbuf_ld2(__amdgpu_buffer_rsrc_t, int, int, int) __asm("llvm.amdgcn.raw.ptr.buffer.load.v2f32");
extern "C" __device__ f32x4 rbuf_ld4(__amdgpu_buffer_rsrc_t, int, int, int) __asm("llvm.amdgcn.raw.ptr.buffer.load.v4f32");
extern "C" __device__ void rbuf_st1(float, __amdgpu_buffer_rsrc_t, int, int, int) __asm("llvm.amdgcn.raw.ptr.buffer.store.f32");
extern "C" __device__ void rbuf_st2(f32x2, __amdgpu_buffer_rsrc_t, int, int, int) __asm("llvm.amdgcn.raw.ptr.buffer.store.v2f32");
extern "C" __device__ void rbuf_st4(f32x4, __amdgpu_buffer_rsrc_t, int, int, int) __asm("llvm.amdgcn.raw.ptr.buffer.store.v4f32");

// raw buffer over [base, base+bytes): out-of-range lanes read 0 / drop their stores.
// `base` must be wave-uniform (the descriptor lives in SGPRs).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}

// compile-time loop: f(integral_constant<int, 0>) ... f(integral_constant<int, N-1>), unrolled in
// the source, so per-iteration register arrays are split into scalars before any loop pass
template <typename F, int... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}
