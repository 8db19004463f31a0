// viterbi_band.hip -- exact best path (Viterbi) on a band of the emit/shift lattice for gfx950.
//
// Semantics: DESIGN.md 2.12. The max-plus sweep of viterbi.hip over the band tensors of
// fwd_bwd_band.hip: W columns per step, the first of them band_start[b,s], which stays or moves
// down by one from a step to the next. The band tensor is addressed as a dense lattice with
// U := W, on align_dev.h's scaffold (one chain wave, four loader waves, chunks, decision words, the
// walk by runs). What is this kernel's own:
//
//   the row     is held in the coordinates of its own step. band_start is staged and validated in
//               LDS by a prologue; its word holds the start and, in bit 30, whether the next step
//               starts one column further. The chain reads the word of the next step one step ahead.
//   the step    the band stays: stay from column r, move from column r-1 (one DPP shift, as
//               k_viterbi). It moves: stay from column r+1 (one DPP shift the other way, filled with
//               -inf), move from column r. Both forms are computed and chosen by selects on the
//               wave-uniform bit; no DPP sits under a select on the lane index. Columns r >= W of
//               the new row are set to -inf: the shift out of r = W-1 where the band stays lands
//               there, and what a column beyond the band holds would stay into r = W-1 at the
//               next move. The LDS buffers are zeroed once, so the transition cells of those
//               columns, which no loader writes, are finite.
//   the walk    aln_walk_band: the column of position p differs per step, p - band_start[ss].
//   the plan    vb_plan: one function for the launcher and the workspace query.
#include <hip/hip_runtime.h>

#include "align_dev.h"

namespace ssnt {
namespace {

constexpr int kVbStageRows = 64;   // workspace mode: rows staged per flush
constexpr int kVbJunk = 160;       // as viterbi.hip's kVitJunk
constexpr int kVbStartMask = (1 << 30) - 1;  // the staged word: band_start, and in bit 30 the move

// lane l gets lane l-1's x, lane 0 gets -inf (viterbi.hip shr1_ninf; never under a lane select)
__device__ __forceinline__ float vb_shr1_ninf(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000u, __builtin_bit_cast(int, x),
                                                               0x138, 0xf, 0xf, false));
}
// lane l gets lane l+1's x, lane 63 gets -inf
__device__ __forceinline__ float vb_shl1_ninf(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000u, __builtin_bit_cast(int, x),
                                                               0x130, 0xf, 0xf, false));
}

struct VbShared {
  int feasible, s, p;
};

struct VbLayout {
  int K, CR;  // columns per lane, rows per chunk
  size_t bs_off, start_off, lt_off, ob_off, bits_off, total;  // bytes
};
// mode: 0 no decision words, 1 words in LDS, 2 in the workspace (stage rows).
// LDS: head | band_start words [T+1] | start[] [T+2] (P + 1 <= T + 1 entries) | two log_trans
// chunk buffers | two log_obs chunk buffers | the words
inline VbLayout vb_layout(int T, int W, int CR, bool obs, int mode) {
  VbLayout L{};
  L.K = aln_k(W);
  L.CR = CR;
  const size_t buf = (size_t)CR * L.K * aln_kstride(L.K) + kVbJunk;  // elements of one buffer
  L.bs_off = kAlnHeadBytes;
  L.start_off = L.bs_off + (((size_t)(T + 1) * 4 + 15) & ~(size_t)15);
  L.lt_off = L.start_off + (((size_t)(T + 2) * 4 + 15) & ~(size_t)15);
  L.ob_off = L.lt_off + 2 * buf * 8;
  L.bits_off = L.ob_off + (obs ? 2 * buf * 4 : 0);
  L.total = L.bits_off + (mode == 1 ? (size_t)T * L.K * 8 : mode == 2 ? (size_t)kVbStageRows * L.K * 8 : 0);
  return L;
}
inline VbLayout vb_pick(int T, int W, bool wide_units, bool obs, int mode) {
  const int CR = aln_chunk_rows(wide_units ? (W + 127) / 128 : (W + 63) / 64);
  return aln_pick(CR, kAlnLoaders, [&](int r) { return vb_layout(T, W, r, obs, mode); });
}

// What the shape alone decides, for the launcher and the query: is it taken at all (the log_obs
// form in workspace mode fits LDS), do the words stay in LDS (they fit beside that form's chunk
// buffers), else the workspace.
struct VbPlan {
  bool supported, lds;
  int K;
  size_t workspace_bytes;
};
inline VbPlan vb_plan(int B, int T, int W) {
  VbPlan p{};
  if (B <= 0 || T <= 0 || W < 1 || W > 256) return p;
  p.K = aln_k(W);
  const VbLayout L2 = vb_pick(T, W, false, true, 2);
  p.supported = L2.total <= kLdsBudget;
  p.lds = p.supported && vb_layout(T, W, L2.CR, true, 1).total <= kLdsBudget;
  p.workspace_bytes = (p.supported && !p.lds) ? (size_t)B * T * p.K * 8 : 0;
  return p;
}

struct VbParams {
  int CR;
  int vec;  // log_trans moves in 16-byte units (16-byte aligned, W even), else 8-byte
  unsigned bs_off, start_off, lt_off, ob_off, bits_off, zero_words;
};

// aln_walk over a band: the words of step ss are in the coordinates of that step, so the bit of
// position p is that of column p - band_start[ss]. A lane whose column falls outside [0, W)
// contributes 0 and reads nothing.
template <int K>
__device__ __forceinline__ AlnAt aln_walk_band(const unsigned long long* wb, int lo_row, int first, int lane,
                                               int* start, const int* bsl, int W, int s, int p) {
  while (p > 0 && s >= first) {
    const int ss = s - lane;
    int bit = 0;
    if (ss >= first) {
      const int c = p - (bsl[ss] & kVbStartMask);
      if (c >= 0 && c < W) bit = (int)((wb[(size_t)(ss - lo_row) * K + (c & (K - 1))] >> (c / K)) & 1ull);
    }
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

// MODE: 0 no path output (no decision words), 1 words in LDS, 2 in the workspace
template <int K, bool OBS, int MODE>
__global__ __launch_bounds__(kAlnThreads) void k_viterbi_band(ViterbiBandArgs a, VbParams q) {
  constexpr int kKs = aln_kstride(K);
  constexpr int kRow = K * kKs;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int T = a.T, W = a.W, CR = q.CR;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const size_t TW = (size_t)T * W;
  const float* lt = a.log_trans + (size_t)b * TW * 2;
  const float* lo = OBS ? a.log_obs + (size_t)b * TW : nullptr;
  int* pos_out = (MODE && a.position) ? a.position + (size_t)b * T : nullptr;
  int* dur_out = (MODE && a.duration) ? a.duration + (size_t)b * a.max_pos : nullptr;
  const int DU = a.max_pos;  // sizes duration only
  const float ninf = -__builtin_inff();

  VbShared* sh = reinterpret_cast<VbShared*>(smem);
  int* bsl = reinterpret_cast<int*>(smem + q.bs_off);
  int* start = reinterpret_cast<int*>(smem + q.start_off);
  float2* ltb = reinterpret_cast<float2*>(smem + q.lt_off);
  float* obb = reinterpret_cast<float*>(smem + q.ob_off);
  const int bufsz = CR * kRow + kVbJunk;
  unsigned long long* bits = reinterpret_cast<unsigned long long*>(smem + q.bits_off);
  unsigned long long* stage = bits;
  unsigned long long* wbuf = reinterpret_cast<unsigned long long*>(ltb);
  const int walk_rows = 2 * bufsz / K;
  unsigned long long* ws = MODE == 2 ? reinterpret_cast<unsigned long long*>(a.workspace) + (size_t)b * T * K
                                     : nullptr;

  auto fill_empty = [&]() {  // the infeasible rule: every position -1, every duration 0
    if (pos_out)
      for (int s = tid; s < T; s += kAlnThreads) pos_out[s] = -1;
    if (dur_out)
      for (int p = tid; p < DU; p += kAlnThreads) dur_out[p] = 0;
  };
  // ------------------------------------------------------------------ lengths
  {
    const bool long_p = dur_out && P > DU;  // duration has no room for this utterance
    if (!(S >= 1 && P >= 1 && S <= T && S >= P) || long_p) {
      if ((S > T || S < 0 || P < 0 || long_p) && a.status && tid == 0) atomicOr(a.status, kStatusBadLength);
      if (tid == 0) a.log_prob[b] = ninf;
      fill_empty();
      return;
    }
  }
  // -------------- band prologue: stage and validate (comparisons only, nothing addressed by it) ----
  {
    const int* __restrict__ bs = a.band_start + (size_t)b * T;
    bool bad = false;
    for (int s = tid; s < S; s += kAlnThreads) {
      const int v = bs[s];
      if (s == 0) bad |= v != 0;
      unsigned mv = 0;
      if (s == S - 1) {
        const long long room = (long long)P - 1 - (long long)v;  // column of P-1 in the last window
        bad |= room < 0 || room >= W;
      } else {
        mv = (unsigned)bs[s + 1] - (unsigned)v;
        bad |= mv > 1u;
      }
      bsl[s] = (v & kVbStartMask) | (int)((mv & 1u) << 30);
    }
    // the chunk buffers start as zeros: the cells of the columns >= W, which no loader writes
    int* z = reinterpret_cast<int*>(smem + q.lt_off);
    for (int i = tid; i < (int)q.zero_words; i += kAlnThreads) z[i] = 0;
    if (__syncthreads_or(bad ? 1 : 0)) {
      if (a.status && tid == 0) atomicOr(a.status, kStatusBadBand);
      if (tid == 0) a.log_prob[b] = ninf;
      fill_empty();
      return;
    }
  }

  // ------------------------------------------------------------------ loaders
  const int NC = (S - 1 + CR - 1) / CR;  // chunks of transition rows 0..S-2
  int goff[kAlnUnits], loff[kAlnUnits], goffo[OBS ? kAlnUnits : 1], loffo[OBS ? kAlnUnits : 1];
  f32x4 lreg[kAlnUnits];
  float oreg[OBS ? kAlnUnits : 1];
  const bool loader = wave >= 1;
  if (loader) {
    const int ppu = q.vec ? 2 : 1;                       // positions per log_trans unit
    const int upr = (W + 64 * ppu - 1) / (64 * ppu);     // units per row and lane
    const int upro = (W + 63) / 64;
    const int w = wave - 1;
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      aln_unit<K>(w, lane, u, upr, ppu, 8, CR, W, goff[u], loff[u]);
      if constexpr (OBS) aln_unit<K>(w, lane, u, upro, 1, 4, CR, W, goffo[u], loffo[u]);
    });
  }
  // global -> registers: rows [c*CR, min(c*CR + CR, S-1))
  auto issue = [&](int c) __attribute__((always_inline)) {
    const int r0 = c * CR;
    const int n = min(CR, S - 1 - r0);
    const __amdgpu_buffer_rsrc_t rs = brsrc(lt + (size_t)r0 * W * 2, (unsigned)(n * W) * 8u);
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
    if constexpr (OBS) {  // log_obs rows [c*CR + 1, ...): the row a step adds is its own
      const __amdgpu_buffer_rsrc_t ro = brsrc(lo + (size_t)(r0 + 1) * W, (unsigned)(n * W) * 4u);
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
  bool inb[K];  // this column is one of the band's
  int mlo = 0, mhi = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    V[k] = ninf;
    inb[k] = K * lane + k < W;
  }
  if (wave == 0 && lane == 0) V[0] = OBS ? lo[0] : 0.0f;
  int word_ahead = bsl[0];  // the staged word of the next transition row
  if (loader && NC > 0) {
    issue(0);
    commit(0);
  }
  __syncthreads();
  for (int c = 0; c < NC; ++c) {
    if (loader && c + 1 < NC) issue(c + 1);
    if (wave == 0) {
      const int r0 = c * CR;
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
      // V[s] (in the coordinates of step s) from V[s-1] and transition row s-1
      auto step = [&](const Row& r, int s) __attribute__((always_inline)) {
        const bool mvu = (__builtin_amdgcn_readfirstlane(word_ahead) >> 30) & 1;  // step s starts one further
        word_ahead = bsl[s];
        float st[K], mv[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          st[k] = V[k] + r.t[k].x;  // V[s-1][r] + e[s-1][r]
          mv[k] = V[k] + r.t[k].y;  // V[s-1][r] + h[s-1][r]
        }
        const float left = vb_shr1_ninf(mv[K - 1]);
        const float up = vb_shl1_ninf(st[0]);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float st1 = k == K - 1 ? up : st[k + 1 < K ? k + 1 : 0];
          const float mv0 = k == 0 ? left : mv[k > 0 ? k - 1 : 0];
          const float stay = mvu ? st1 : st[k];
          const float move = mvu ? mv[k] : mv0;
          const bool bp = move > stay;  // strict: a tie keeps the emit
          float v = bp ? move : stay;
          if constexpr (OBS) v = v + r.o[k];
          V[k] = inb[k] ? v : ninf;
          if constexpr (MODE != 0) aln_put_word(__ballot(bp), k, mlo, mhi);
        }
        const unsigned long long myw = aln_my_word(mlo, mhi);
        if constexpr (MODE == 1) {
          if (lane < K) bits[(size_t)s * K + lane] = myw;
        } else if constexpr (MODE == 2) {
          const int sr = s & (kVbStageRows - 1);
          if (lane < K) stage[sr * K + lane] = myw;
          if (sr == kVbStageRows - 1 || s == S - 1) {  // flush rows [s - sr, s]
            unsigned long long* dst = ws + (size_t)(s - sr) * K;
            for (int j = lane; j < (sr + 1) * K; j += 64) dst[j] = stage[j];
          }
        }
      };
      const int n = min(CR, S - 1 - r0);
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
    const int rl = P - 1 - (bsl[S - 1] & kVbStartMask);  // in [0, W): the prologue checked it
    float v = ninf;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (K * lane + k == rl) v = V[k];
    if (K * lane <= rl && rl < K * lane + K) {  // the one lane that holds P-1
      if (a.flags & SSNT_FLAG_TERMINAL_EMIT) v = v + lt[((size_t)(S - 1) * W + rl) * 2];
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
      const AlnAt at = aln_walk_band<K>(wb, lo_row, max(lo_row, 1), lane, start, bsl, W, s, p);
      if (lane == 0) {
        sh->s = at.s;
        sh->p = at.p;
      }
    }
  }

  // ------------------------------------------------------------------ outputs
  aln_write_path<kAlnThreads>(start, S, P, T, DU, dur_out, pos_out, tid);
}

template <int K, bool OBS, int MODE>
int launch_vb_k(const ViterbiBandArgs& a, const VbLayout& L, bool vec, hipStream_t st) {
  const VbParams q{L.CR, vec, (unsigned)L.bs_off, (unsigned)L.start_off, (unsigned)L.lt_off, (unsigned)L.ob_off,
                   (unsigned)L.bits_off, (unsigned)((L.bits_off - L.lt_off) / 4)};
  return launch_lds(k_viterbi_band<K, OBS, MODE>, dim3(a.B), dim3(kAlnThreads), L.total, kLdsBudget, st, a, q);
}

template <int K, bool OBS>
int launch_vb_mode(const ViterbiBandArgs& a, const VbLayout& L, bool vec, int mode, hipStream_t st) {
  if (mode == 0) return launch_vb_k<K, OBS, 0>(a, L, vec, st);
  if (mode == 1) return launch_vb_k<K, OBS, 1>(a, L, vec, st);
  return launch_vb_k<K, OBS, 2>(a, L, vec, st);
}

template <bool OBS>
int launch_vb_obs(const ViterbiBandArgs& a, const VbLayout& L, bool vec, int mode, hipStream_t st) {
  if (L.K == 1) return launch_vb_mode<1, OBS>(a, L, vec, mode, st);
  return L.K == 2 ? launch_vb_mode<2, OBS>(a, L, vec, mode, st) : launch_vb_mode<4, OBS>(a, L, vec, mode, st);
}

}  // namespace

size_t viterbi_band_workspace_bytes(int B, int T, int W) { return vb_plan(B, T, W).workspace_bytes; }

int launch_viterbi_band(const ViterbiBandArgs& a, hipStream_t st) {
  if (a.W < 1 || a.W > 256) return SSNT_ERR_UNSUPPORTED;  // (first: an empty tensor has no address)
  if (a.B < 0 || a.T <= 0 || (a.flags & ~SSNT_FLAG_TERMINAL_EMIT)) return SSNT_ERR_INVALID_ARG;
  if (!a.log_trans || !a.band_start || !a.step_len || !a.pos_len || !a.log_prob) return SSNT_ERR_INVALID_ARG;
  if (a.duration && a.max_pos < 0) return SSNT_ERR_INVALID_ARG;
  if (a.B == 0) return SSNT_OK;
  if (!aligned_to(a.log_trans, 8) || !aligned_to(a.log_obs, 4)) return SSNT_ERR_UNSUPPORTED;
  const VbPlan p = vb_plan(a.B, a.T, a.W);
  if (!p.supported) return SSNT_ERR_UNSUPPORTED;
  const bool path = a.position || a.duration;
  if (path && !p.lds && !aln_workspace_ok(a.workspace, a.workspace_bytes, p.workspace_bytes))
    return SSNT_ERR_WORKSPACE;
  const int mode = !path ? 0 : p.lds ? 1 : 2;
  const bool obs = a.log_obs != nullptr;
  const bool vec = aligned_to(a.log_trans, 16) && a.W % 2 == 0;
  const VbLayout L = vb_pick(a.T, a.W, vec && !obs, obs, mode);
  if (L.total > kLdsBudget) return SSNT_ERR_UNSUPPORTED;
  ViterbiBandArgs x = a;
  if (mode != 2) x.workspace = nullptr;
  return obs ? launch_vb_obs<true>(x, L, vec, mode, st) : launch_vb_obs<false>(x, L, vec, mode, st);
}

}  // namespace ssnt
