// viterbi.hip -- exact best path (Viterbi) over the emit/shift lattice for gfx950.
//
// Semantics: DESIGN.md 2.2. A max-plus sweep over the (B,T,U,2) tensor of the forward-backward:
// f32 adds and one strict compare per cell, no reassociation, so every form is bit-identical to
// the plain f32 restatement (tests/viterbi_ref.py). The structure (one chain wave, four loader
// waves, chunks, decision words, the walk by runs) is align_dev.h's. What is this kernel's own:
//
//   the chain   V[s][p] in f32; the compare of each k is that step's backpointer word k.
//   the loaders log_trans moves in 16-byte units (two positions) when it is 16-byte aligned with
//               even U, else in 8-byte units; log_obs as single floats. Nothing is converted.
//   the words   T*K*8 bytes per utterance. In workspace mode they are staged through LDS and
//               flushed 64 rows at a time with vector stores, and read back for the backtrace in
//               blocks as large as the two chunk buffers. With no path output nothing is kept.
//   the walk    wave 0 walks; all waves read a block back and write duration and position.
#include <hip/hip_runtime.h>

#include "align_dev.h"

namespace ssnt {
namespace {

constexpr int kVitStageRows = 64;                     // workspace mode: rows staged per flush
// elements behind each buffer, for unused units' writes: lane (< 64) and, for the second half of
// a 16-byte unit, kKs (<= 80) further
constexpr int kVitJunk = 160;

// shr1 (lattice_dev.h) with -inf for lane 0: the lane without a source keeps `old`. No select on
// the lane index around it -- a DPP read of a lane that EXEC masks off counts as "no source", and
// the compiler is free to turn such a select into exactly that mask.
__device__ __forceinline__ float shr1_ninf(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000u, __builtin_bit_cast(int, x),
                                                               0x138, 0xf, 0xf, false));
}

struct VitShared {
  int feasible, s, p;
};

struct VitLayout {
  int K, R;
  size_t start_off, lt_off, ob_off, bits_off, total;  // bytes
};
// mode: 0 no backpointers, 1 backpointer words in LDS, 2 in the workspace (stage rows)
inline VitLayout vit_layout(int T, int U, int R, bool obs, int mode) {
  VitLayout L{};
  L.K = aln_k(U);
  L.R = R;
  const size_t buf = (size_t)R * L.K * aln_kstride(L.K) + kVitJunk;  // elements of one buffer
  L.start_off = kAlnHeadBytes;
  L.lt_off = (L.start_off + (size_t)(U + 2) * 4 + 15) & ~(size_t)15;
  L.ob_off = L.lt_off + 2 * buf * 8;
  L.bits_off = L.ob_off + (obs ? 2 * buf * 4 : 0);
  L.total = L.bits_off + (mode == 1 ? (size_t)T * L.K * 8
                          : mode == 2 ? (size_t)kVitStageRows * L.K * 8 : 0);
  return L;
}
// A loader lane moves 16-byte units (two positions) when log_trans is 16-byte aligned with even U
// and there is no log_obs, else one position per unit (log_obs moves as single floats, so it sets
// the unit count whenever it is there). A chunk keeps at least one row per loader wave.
inline VitLayout vit_pick(int T, int U, bool wide_units, bool obs, int mode) {
  const int R = aln_chunk_rows(wide_units ? (U + 127) / 128 : (U + 63) / 64);
  return aln_pick(R, kAlnLoaders, [&](int r) { return vit_layout(T, U, r, obs, mode); });
}
// The backpointer words stay in LDS when they fit beside the chunk buffers the log_obs form has
// in workspace mode (from the shape alone: the query knows neither log_obs nor the alignment).
inline bool vit_bits_fit(int T, int U) {
  const int R = vit_pick(T, U, false, true, 2).R;
  return vit_layout(T, U, R, true, 1).total <= kLdsBudget;
}

struct VitParams {
  int R;
  int vec;  // log_trans moves in 16-byte units (16-byte aligned, U even), else 8-byte
  unsigned start_off, lt_off, ob_off, bits_off;
};

// MODE: 0 no path output (no backpointers), 1 backpointer words in LDS, 2 in the workspace
template <int K, bool OBS, int MODE>
__global__ __launch_bounds__(kAlnThreads) void k_viterbi(ViterbiArgs a, VitParams q) {
  constexpr int kKs = aln_kstride(K);
  constexpr int kRow = K * kKs;  // LDS row stride (float2 units for log_trans, floats for log_obs)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int T = a.T, U = a.U, R = q.R;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const size_t TU = (size_t)T * U;
  const float* lt = a.log_trans + (size_t)b * TU * 2;
  const float* lo = OBS ? a.log_obs + (size_t)b * TU : nullptr;
  int* pos_out = (MODE && a.position) ? a.position + (size_t)b * T : nullptr;
  int* dur_out = (MODE && a.duration) ? a.duration + (size_t)b * U : nullptr;
  const float ninf = -__builtin_inff();

  VitShared* sh = reinterpret_cast<VitShared*>(smem);
  int* start = reinterpret_cast<int*>(smem + q.start_off);
  float2* ltb = reinterpret_cast<float2*>(smem + q.lt_off);
  float* obb = reinterpret_cast<float*>(smem + q.ob_off);
  const int bufsz = R * kRow + kVitJunk;  // elements of one buffer
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(smem + q.bits_off);
  unsigned long long* stage = bits;                          // workspace mode
  // workspace mode, backtrace: the chunk buffers are free by then and hold 2 * bufsz / K rows
  unsigned long long* wbuf = reinterpret_cast<unsigned long long*>(ltb);
  const int walk_rows = 2 * bufsz / K;
  unsigned long long* ws = MODE == 2 ? reinterpret_cast<unsigned long long*>(a.workspace) + (size_t)b * T * K
                                     : nullptr;

  auto fill_empty = [&]() {  // the infeasible rule: every position -1, every duration 0
    if (pos_out)
      for (int s = tid; s < T; s += kAlnThreads) pos_out[s] = -1;
    if (dur_out)
      for (int p = tid; p < U; p += kAlnThreads) dur_out[p] = 0;
  };
  if (!aln_lengths_ok(S, P, T, U, a.status, tid)) {
    if (tid == 0) a.log_prob[b] = ninf;
    fill_empty();
    return;
  }

  // ------------------------------------------------------------------ loaders
  const int NC = (S - 1 + R - 1) / R;  // chunks of transition rows 0..S-2
  int goff[kAlnUnits], loff[kAlnUnits], goffo[OBS ? kAlnUnits : 1], loffo[OBS ? kAlnUnits : 1];
  f32x4 lreg[kAlnUnits];
  float oreg[OBS ? kAlnUnits : 1];
  const bool loader = wave >= 1;
  if (loader) {
    const int ppu = q.vec ? 2 : 1;                       // positions per log_trans unit
    const int upr = (U + 64 * ppu - 1) / (64 * ppu);     // units per row and lane
    const int upro = (U + 63) / 64;
    const int w = wave - 1;
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      aln_unit<K>(w, lane, u, upr, ppu, 8, R, U, goff[u], loff[u]);
      if constexpr (OBS) aln_unit<K>(w, lane, u, upro, 1, 4, R, U, goffo[u], loffo[u]);
    });
  }
  // global -> registers: rows [c*R, min(c*R + R, S-1))
  auto issue = [&](int c) __attribute__((always_inline)) {
    const int r0 = c * R;
    const int n = min(R, S - 1 - r0);
    const __amdgpu_buffer_rsrc_t rs = brsrc(lt + (size_t)r0 * U * 2, (unsigned)(n * U) * 8u);
    if (q.vec) {
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        lreg[u] = rbuf_ld4(rs, goff[u], 0, 0);
      });
    } else {
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        const f32x2 v = rbuf_ld2(rs, goff[u], 0, 0);
        lreg[u].x = v.x; lreg[u].y = v.y;
      });
    }
    if constexpr (OBS) {  // log_obs rows [c*R + 1, ...): the row a step adds is its own
      const __amdgpu_buffer_rsrc_t ro = brsrc(lo + (size_t)(r0 + 1) * U, (unsigned)(n * U) * 4u);
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        oreg[u] = rbuf_ld1(ro, goffo[u], 0, 0);
      });
    }
  };
  // registers -> LDS buffer c & 1 (rows past the chunk's end get zeros)
  auto commit = [&](int c) __attribute__((always_inline)) {
    float2* dst = ltb + (size_t)(c & 1) * bufsz;
    if (q.vec) {
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        dst[loff[u]] = make_float2(lreg[u].x, lreg[u].y);
        dst[loff[u] + (K == 1 ? 1 : kKs)] = make_float2(lreg[u].z, lreg[u].w);
      });
    } else {
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        dst[loff[u]] = make_float2(lreg[u].x, lreg[u].y);
      });
    }
    if constexpr (OBS) {
      float* dsto = obb + (size_t)(c & 1) * bufsz;
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        dsto[loffo[u]] = oreg[u];
      });
    }
  };

  // ------------------------------------------------------------------ sweep
  float V[K];
  int mlo = 0, mhi = 0;  // lane k < K: the low / high half of this step's backpointer word k
#pragma unroll
  for (int k = 0; k < K; ++k) V[k] = ninf;
  if (wave == 0 && lane == 0) V[0] = OBS ? lo[0] : 0.0f;
  if (loader && NC > 0) {
    issue(0);
    commit(0);
  }
  __syncthreads();
  for (int c = 0; c < NC; ++c) {
    if (loader && c + 1 < NC) issue(c + 1);
    if (wave == 0) {
      const int r0 = c * R;
      const float2* B = ltb + (size_t)(c & 1) * bufsz + lane;
      const float* OB = obb + (size_t)(c & 1) * bufsz + lane;
      struct Row {
        float2 t[K];
        float o[OBS ? K : 1];
      };
      auto ld = [&](Row& r, int i) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
          r.t[k] = B[i * kRow + k * kKs];
          if constexpr (OBS) r.o[k] = OB[i * kRow + k * kKs];
        }
      };
      // V[s] from V[s-1] and transition row s-1
      auto step = [&](const Row& r, int s) __attribute__((always_inline)) {
        float mv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) mv[k] = V[k] + r.t[k].y;  // V[s-1][p] + h[s-1][p]
        const float left = shr1_ninf(mv[K - 1]);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float stay = V[k] + r.t[k].x;
          const float move = k == 0 ? left : mv[k > 0 ? k - 1 : 0];
          const bool bp = move > stay;  // strict: a tie keeps the emit
          float v = bp ? move : stay;
          if constexpr (OBS) v = v + r.o[k];
          V[k] = v;
          if constexpr (MODE != 0) aln_put_word(__ballot(bp), k, mlo, mhi);
        }
        const unsigned long long myw = aln_my_word(mlo, mhi);
        if constexpr (MODE == 1) {
          if (lane < K) bits[(size_t)s * K + lane] = myw;
        } else if constexpr (MODE == 2) {
          const int sr = s & (kVitStageRows - 1);
          if (lane < K) stage[sr * K + lane] = myw;
          if (sr == kVitStageRows - 1 || s == S - 1) {  // flush rows [s - sr, s]
            unsigned long long* dst = ws + (size_t)(s - sr) * K;
            for (int j = lane; j < (sr + 1) * K; j += 64) dst[j] = stage[j];
          }
        }
      };
      // two rows in registers: the next row's LDS reads go out before this row's arithmetic
      const int n = min(R, S - 1 - r0);
      Row ra, rb;
      ld(ra, 0);
      int i = 0;
      for (; i + 1 < n; i += 2) {
        ld(rb, i + 1);
        step(ra, r0 + i + 1);
        ld(ra, min(i + 2, n - 1));
        step(rb, r0 + i + 2);
      }
      if (i < n) step(ra, r0 + i + 1);
    }
    if (loader && c + 1 < NC) commit(c + 1);
    __syncthreads();
  }

  // ------------------------------------------------------------------ log_prob, feasibility
  if (wave == 0) {
    float v = ninf;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (K * lane + k == P - 1) v = V[k];
    if (K * lane <= P - 1 && P - 1 < K * lane + K) {  // the one lane that holds P-1
      if (a.flags & SSNT_FLAG_TERMINAL_EMIT) v = v + lt[((size_t)(S - 1) * U + (P - 1)) * 2];
      a.log_prob[b] = v;
      sh->feasible = v > ninf;
      sh->s = S - 1;
      sh->p = P - 1;
    }
    if constexpr (MODE == 2) __threadfence();  // the flushed words, before the other waves read them
  }
  if constexpr (MODE == 0) return;
  __syncthreads();
  if (!sh->feasible) {
    fill_empty();
    return;
  }

  // ------------------------------------------------------------------ backtrace by runs
  for (int p = tid; p < P; p += kAlnThreads) start[p] = 0;
  if (tid == 0) start[P] = S;
  for (;;) {
    __syncthreads();
    int s = sh->s, p = sh->p;
    if (p <= 0 || s < 1) break;
    int lo_row = 0;
    const unsigned long long* wb = bits;
    if constexpr (MODE == 2) {  // rows [lo_row, s] of the workspace -> LDS, by all waves
      lo_row = max(1, s - walk_rows + 1);
      aln_read_back<kAlnThreads>(ws + (size_t)lo_row * K, wbuf, (s - lo_row + 1) * K, tid);
      wb = wbuf;
    }
    __syncthreads();
    if (wave == 0) {
      const AlnAt at = aln_walk<K>(wb, lo_row, max(lo_row, 1), lane, start, s, p);
      if (lane == 0) {
        sh->s = at.s;
        sh->p = at.p;
      }
    }
  }

  // ------------------------------------------------------------------ outputs
  aln_write_path<kAlnThreads>(start, S, P, T, U, dur_out, pos_out, tid);
}

template <int K, bool OBS, int MODE>
int launch_viterbi_k(const ViterbiArgs& a, const VitLayout& L, bool vec, hipStream_t st) {
  const VitParams q{L.R, vec, (unsigned)L.start_off, (unsigned)L.lt_off, (unsigned)L.ob_off, (unsigned)L.bits_off};
  return launch_lds(k_viterbi<K, OBS, MODE>, dim3(a.B), dim3(kAlnThreads), L.total, kLdsBudget, st, a, q);
}

template <bool OBS>
int launch_viterbi_obs(const ViterbiArgs& a, const VitLayout& L, bool vec, int mode, hipStream_t st) {
  return aln_with_k(L.K, [&](auto Kc) {
    constexpr int K = decltype(Kc)::value;
    if (mode == 0) return launch_viterbi_k<K, OBS, 0>(a, L, vec, st);
    if (mode == 1) return launch_viterbi_k<K, OBS, 1>(a, L, vec, st);
    return launch_viterbi_k<K, OBS, 2>(a, L, vec, st);
  });
}

}  // namespace

size_t viterbi_workspace_bytes(int B, int T, int U) {
  if (vit_bits_fit(T, U)) return 0;
  return (size_t)B * T * aln_k(U) * 8;
}

int launch_viterbi(const ViterbiArgs& a, hipStream_t st) {
  const int rc = aln_check_args(a.B, a.T, a.U, a.flags, a.log_trans && a.step_len && a.pos_len && a.log_prob,
                                a.log_trans, a.log_obs);
  if (rc != SSNT_OK || a.B == 0) return rc;
  const bool path = a.position || a.duration;
  const bool obs = a.log_obs != nullptr;
  const int U = a.U > 0 ? a.U : 1;  // (T == 0 or U == 0: every utterance is infeasible)
  const bool fit = a.T == 0 || a.U == 0 || vit_bits_fit(a.T, U);
  if (path && !fit && !aln_workspace_ok(a.workspace, a.workspace_bytes, viterbi_workspace_bytes(a.B, a.T, a.U)))
    return SSNT_ERR_WORKSPACE;
  const int mode = !path ? 0 : fit ? 1 : 2;
  const bool vec = aligned_to(a.log_trans, 16) && U % 2 == 0;
  const VitLayout L = vit_pick(a.T, U, vec && !obs, obs, mode);
  if (L.total > kLdsBudget) return SSNT_ERR_UNSUPPORTED;
  return obs ? launch_viterbi_obs<true>(a, L, vec, mode, st) : launch_viterbi_obs<false>(a, L, vec, mode, st);
}

}  // namespace ssnt
