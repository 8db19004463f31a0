// align_dev.h -- the chain-and-loaders scaffold of the emit/shift alignment kernels: what
// k_viterbi (viterbi.hip) and k_sample_align (sample_align.hip) have in common. DESIGN.md 5.6.
// Included inside namespace ssnt::{anonymous}, by those two files only.
//
// One workgroup = one utterance, 5 waves:
//
//   wave 0      the chain: row s of the lattice from row s-1, for s = 1..S-1. A lane holds K
//               consecutive positions (p = K*lane + k, K = 1..16, so one wave spans U <= 1024 and
//               no row needs a cross-wave neighbour); the left neighbour of k = 0 is one DPP wave
//               shift, never under a select on the lane index (shr1_ninf, viterbi.hip). A compare
//               per k lands in an SGPR pair, which is a 64-bit decision word (bit `lane` of word
//               k <-> position K*lane + k); two v_writelane put it into lane k, and lanes 0..K-1
//               store the K words of a step.
//   waves 1..4  loaders: the rows of the next chunk (R rows) go global -> registers while the
//               chain sweeps the current chunk, then registers -> LDS, transposed to
//               [row][k][lane] (k-planes padded by 32/K so both the loaders' writes and the
//               chain's reads are bank-conflict free). Two LDS buffers, one workgroup barrier per
//               chunk: the load latency of a chunk hides behind R chain steps. The loads are
//               range-checked buffer loads, all issued back to back: a unit outside the chunk has
//               an offset no range contains and writes to the junk behind the buffer. No
//               predicate, or the compiler waits for each load before it issues the next. The
//               per-unit arrays are indexed through static_for only, or they fall to scratch.
//
// Decision words: K*8 bytes per step, in LDS when they fit beside the buffers, else in the
// caller's workspace, read back for the walk in blocks through the chunk buffers, free by then.
// The walk, same launch: the path is monotone, so a wave walks it by runs: 64 lanes test the bit
// of the current position at 64 consecutive steps, one ballot finds the step that entered it: at
// most (P-1) + S/64 LDS round trips instead of S. start[p] (the first step at p) then gives
// duration[p] = start[p+1] - start[p] and position[s] by a binary search.
//
// Each kernel keeps its arithmetic, its issue / commit bodies, its LDS layout and its word storage.
// It also writes out the chunk loop (issue(c+1), sweep, commit(c+1), barrier) and the two-rows loop
// in it: as helpers over the kernels' lambdas both changed register allocation.
#pragma once
#include <hip/hip_runtime.h>

#include "lattice_dev.h"
#include "launch_util.h"

namespace ssnt {
namespace {

constexpr int kAlnLoaders = 4;                        // loader waves
constexpr int kAlnWaves = 1 + kAlnLoaders;
constexpr int kAlnThreads = 64 * kAlnWaves;
constexpr int kAlnUnits = 16;                         // load units per loader lane and chunk
constexpr int kAlnMaxRpw = 8;                         // rows per loader wave and chunk, at most
constexpr size_t kAlnHeadBytes = 64;
constexpr int kAlnNoUnit = 0x7fffffff;                // byte offset no buffer range contains

// ---------------------------------------------------------------------- host: shape plan, checks
constexpr int aln_k(int U) { return U <= 64 ? 1 : U <= 128 ? 2 : U <= 256 ? 4 : U <= 512 ? 8 : 16; }
constexpr int aln_kstride(int K) { return 64 + (K > 1 ? 32 / K : 0); }  // elements of one k-plane
// Rows per chunk: a loader lane moves kAlnUnits units per chunk, `per_row` of them in each row
inline int aln_chunk_rows(int per_row) {
  int r = kAlnUnits / per_row;
  r = r < 1 ? 1 : r > kAlnMaxRpw ? kAlnMaxRpw : r;
  return kAlnLoaders * r;
}
// layout(R) of the deepest chunk the unit count gives, shortened until everything fits LDS or R
// is down to `floor` rows
template <typename F>
inline auto aln_pick(int R, int floor, F layout) {
  auto L = layout(R);
  while (L.total > kLdsBudget && R > floor) {
    R = R > kAlnLoaders ? R - kAlnLoaders : R / 2;
    L = layout(R);
  }
  return L;
}
// f(integral_constant<int, K>) for the K of the shape
template <typename F>
inline int aln_with_k(int K, F f) {
  switch (K) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}
// The checks both entry points make, in their order (`ptrs`: every required pointer is there).
// SSNT_OK with B == 0 means "nothing to do": the caller returns it as it does any other code.
inline int aln_check_args(int B, int T, int U, unsigned flags, bool ptrs, const void* log_trans,
                          const void* log_obs) {
  if (B < 0 || T < 0 || U < 0 || (flags & ~SSNT_FLAG_TERMINAL_EMIT)) return SSNT_ERR_INVALID_ARG;
  if (B == 0) return SSNT_OK;
  if (!ptrs) return SSNT_ERR_INVALID_ARG;
  if (U > 1024) return SSNT_ERR_UNSUPPORTED;
  if (!aligned_to(log_trans, 8) || !aligned_to(log_obs, 4)) return SSNT_ERR_UNSUPPORTED;
  return SSNT_OK;
}
// the workspace a shape needs whose words do not fit LDS: given, large enough, 8-byte aligned
inline bool aln_workspace_ok(const void* ws, size_t b, size_t need) { return ws && b >= need && aligned_to(ws, 8); }

// ---------------------------------------------------------------------- device: chain and loaders
// v_writelane_b32: lane `lane` of the result holds the wave-uniform `v`, the other lanes keep `old`
// (bound to the LLVM intrinsic by name, as buffer_ops.h does: this toolchain has no clang builtin)
extern "C" __device__ int aln_writelane(int v, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// the ballot word w goes straight into lane k of (mlo, mhi): no select, no copy
__device__ __forceinline__ void aln_put_word(unsigned long long w, int k, int& mlo, int& mhi) {
  mlo = aln_writelane((int)(unsigned)w, k, mlo);
  mhi = aln_writelane((int)(unsigned)(w >> 32), k, mhi);
}
// this lane's 64-bit word
__device__ __forceinline__ unsigned long long aln_my_word(int mlo, int mhi) {
  return ((unsigned long long)(unsigned)mhi << 32) | (unsigned)mlo;
}

// Is there a lattice at all? Lengths outside the tensor also raise kStatusBadLength.
__device__ __forceinline__ bool aln_lengths_ok(int S, int P, int T, int U, int* status, int tid) {
  if (S >= 1 && P >= 1 && S <= T && P <= U && S >= P) return true;
  if ((S > T || P > U || S < 0 || P < 0) && status && tid == 0) atomicOr(status, kStatusBadLength);
  return false;
}

// Loader wave w takes rows w, w+4, ... of a chunk; its lanes stride across a row, `upr` units per
// row and lane, `ppu` positions and `bytes` bytes per unit. Everything but the chunk's base is
// chunk-invariant, so unit u's offsets are formed once: goff = byte offset from the chunk's first
// row (kAlnNoUnit for a unit outside the geometry: its load is out of every range), loff = LDS
// element in the buffer (the junk behind it for such a unit). The run-time inputs come by reference,
// as a lambda's captures do: by value the helper is simplified on its own before it is inlined, and
// the row arithmetic then lands in branches and VALU instead of SALU selects.
template <int K>
__device__ __forceinline__ void aln_unit(const int& w, const int& lane, int u, const int& upr, const int& ppu,
                                         int bytes, const int& R, const int& U, int& goff, int& loff) {
  constexpr int kKs = aln_kstride(K);
  constexpr int kRow = K * kKs;
  const int row = w + kAlnLoaders * (u / upr);
  const int p = (lane + 64 * (u % upr)) * ppu;
  const bool ok = row < R && p < U;
  goff = ok ? (row * U + p) * bytes : kAlnNoUnit;
  loff = ok ? row * kRow + (p % K) * kKs + p / K : R * kRow + lane;
}

// ---------------------------------------------------------------------- device: walk and outputs
// nw words of the workspace -> LDS by NT threads (t = 0..NT-1), 8 loads in flight per lane. The
// caller orders it against the words' writers and the LDS block's readers.
template <int NT>
__device__ __forceinline__ void aln_read_back(const unsigned long long* src, unsigned long long* dst, int nw,
                                              int t) {
  for (int j0 = t; j0 < nw; j0 += 8 * NT) {
    unsigned long long v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
      v[i] = __hip_atomic_load(src + min(j0 + i * NT, nw - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (j0 + i * NT < nw) dst[j0 + i * NT] = v[i];
  }
}

// One wave walks from (s, p) down over the block wb, which holds the words of rows lo_row.. ; it
// stops below row `first` or at p == 0, fills start[] on the way and returns where it stopped.
struct AlnAt {
  int s, p;
};
template <int K>
__device__ __forceinline__ AlnAt aln_walk(const unsigned long long* wb, int lo_row, int first, int lane,
                                          int* start, int s, int p) {
  while (p > 0 && s >= first) {
    const int ss = s - lane;
    int bit = 0;
    if (ss >= first) bit = (int)((wb[(size_t)(ss - lo_row) * K + (p & (K - 1))] >> (p / K)) & 1ull);
    const unsigned long long m = __ballot(bit != 0);
    if (m == 0) {
      s = max(s - 64, first - 1);
    } else {  // the nearest step below s that entered p
      const int st = s - (__ffsll((long long)m) - 1);
      if (lane == 0) start[p] = st;
      s = st - 1;
      p = p - 1;
    }
  }
  return {s, p};
}

// the last p with start[p] <= s (start[0] = 0, increasing)
__device__ __forceinline__ int aln_pos_of(const int* start, int P, int s) {
  int lo_p = 0, hi_p = P - 1;
  while (lo_p < hi_p) {
    const int mid = (lo_p + hi_p + 1) >> 1;
    if (start[mid] <= s) lo_p = mid; else hi_p = mid - 1;
  }
  return lo_p;
}

// duration[0..U) and position[0..T) of one path from its start[], by NT threads (t = 0..NT-1);
// a null output is not written
template <int NT>
__device__ __forceinline__ void aln_write_path(const int* start, int S, int P, int T, int U, int* dur, int* pos,
                                               int t) {
  if (dur)
    for (int p = t; p < U; p += NT) dur[p] = p < P ? start[p + 1] - start[p] : 0;
  if (pos)
    for (int s = t; s < T; s += NT) pos[s] = s < S ? aln_pos_of(start, P, s) : -1;
}

}  // namespace
}  // namespace ssnt
