// ec_rows.h -- where k_expected_cost_sweep (expected_cost.hip) leaves its rows in the workspace, for
// the launches that read them: k_expected_cost_grad and k_duration_posterior
// (duration_posterior.hip). Included inside namespace ssnt::{anonymous}, behind align_dev.h.
//
//   head   B records of 16 bytes: Z.m, Z.e, risk (0 without the mean), 0
//   rows   from the first 16-byte boundary behind the head: direction (0 alpha, 1 beta), utterance,
//          step row, then the planes m, e (and the mean), each ec_upad(U) floats
#pragma once
#include "align_dev.h"

namespace ssnt {
namespace {

constexpr size_t kEcHeadRec = 16;      // workspace head per utterance: Z.m, Z.e, risk, 0

// stored rows are padded to whole lane slices
inline int ec_upad(int U) {
  const int K = aln_k(U);
  return (U + K - 1) / K * K;
}
// the rows start at the first 16-byte boundary behind the head (the workspace itself: 8-byte aligned)
__host__ __device__ inline float* ec_rows_base(void* ws, int B) {
  const uintptr_t p = reinterpret_cast<uintptr_t>(ws) + (size_t)B * kEcHeadRec;
  return reinterpret_cast<float*>((p + 15) & ~(uintptr_t)15);
}

}  // namespace
}  // namespace ssnt
