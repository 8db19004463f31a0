// v2_lattice_dev.h -- the v2 duration-class lattice as its kernels share it (v2_fwd_bwd.hip: the
// sum over paths, v2_viterbi.hip: the best path): the per-utterance state, the window of a row,
// the no-lattice rule, the row capacity and the LDS-only barrier. One definition, so both
// kernels walk exactly the same cells (oracle/ssnt_oracle.c "F4").
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ssnt_internal.h"

namespace ssnt {

constexpr int kF4Pad = 64;  // neutral cells either side of a row window (PADDED: dmax <= kF4Pad)

__device__ __forceinline__ int f4_f2i(float x) {  // Rust `f32 as i32` (saturating, NaN -> 0)
  if (x != x) return 0;
  if (x >= 2147483648.0f) return 2147483647;
  if (x <= -2147483648.0f) return (-2147483647 - 1);
  return (int)x;
}

struct F4Utt {
  int I, O, X, dmax;
  bool test;
};

// cells of row r that can hold mass: [lo, hi] (empty when lo > hi); = oracle f4_window
__device__ __forceinline__ void f4_window(const F4Utt& u, int r, int& lo, int& hi) {
  if (r == 0) {
    lo = 0;
    hi = 0;
    return;
  }
  if (u.test) {
    const long long h = (long long)r * u.dmax;
    lo = 0;
    hi = h < u.X - 1 ? (int)h : u.X - 1;
    return;
  }
  const int t = r - 1;
  if ((long long)(u.I - (t + 1)) * 3 > u.O) {  // will_overrun (src/v2.rs:106-111)
    lo = 1;
    hi = 0;
    return;
  }
  const float diagonal = (float)u.O / (float)u.I * (float)(t + 1);  // src/v2.rs:94-104
  const float upper_range = (float)u.O * 0.1f;
  const float lower_range = (float)u.O * 0.05f;
  int lb = f4_f2i(fmaxf(diagonal - lower_range, 0.0f));
  int ub = f4_f2i(fminf(diagonal + upper_range, (float)u.O));
  if (t == u.I - 1) {  // src/v2.rs:135-137
    lb = max(lb, u.O);
    ub = min(ub, u.O);
  }
  lo = max(lb, 0);
  hi = min(ub, u.X - 1);
}

// workgroup barrier ordering LDS only: __syncthreads() would also wait for every global store
// in flight (vmcnt(0)), i.e. one HBM write round trip per sweep step. Not for a kernel phase
// that reads back global memory written in the same launch: that needs __syncthreads().
__device__ __forceinline__ void lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// per-utterance state every v2 lattice kernel derives the same way (Args: V2FwdBwdArgs or
// V2ViterbiArgs); false: no lattice (the caller writes the empty outputs). `report`: this
// workgroup ORs the bad-length / bad-table bits into the status word.
template <typename Args>
__device__ __forceinline__ bool f4_setup(const Args& a, int b, const int* dur, F4Utt& u, bool report) {
  u.I = a.input_length[b];
  u.O = a.output_length[b];
  u.X = a.X;
  u.test = a.test_mode;
  u.dmax = 0;
  bool neg = false;
  for (int i = 0; i < a.D; ++i) {
    u.dmax = max(u.dmax, dur[i]);
    neg |= dur[i] < 0;
  }
  const bool bad_len = u.I < 0 || u.I > a.Imax || u.O < 0;
  if (report && (bad_len || neg) && threadIdx.x == 0 && a.status)
    atomicOr(a.status, neg ? kStatusBadIndex : kStatusBadLength);
  // band mode with O > max_total: the final total can never equal O (src/v2.rs:135-137), so the
  // lattice is empty (= oracle f4_one); its windows could also exceed the band-sized Wcap
  const bool beyond = !u.test && u.O > u.X - 1;
  return !(bad_len || neg || u.I == 0 || beyond);
}

// cells a stored row holds: every window of the shape fits (band: ub - lb + 1 <= 0.15 O + 3)
inline size_t v2_fwd_bwd_wcap(int max_total, bool test_mode) {
  const int X = max_total + 1;
  if (test_mode) return (size_t)X;
  const size_t band = (size_t)(0.15 * (double)max_total) + 8;
  return band < (size_t)X ? band : (size_t)X;
}

}  // namespace ssnt
