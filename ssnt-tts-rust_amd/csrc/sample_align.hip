// sample_align.hip -- alignments drawn from the posterior of the emit/shift lattice for gfx950.
//
// Semantics: DESIGN.md 2.4. Forward filter, backward sample: the forward sweep is the alpha
// recurrence of the forward-backward in split-exponent ("xf") f32; for every cell it leaves, per
// sample k, the bit "uniform[k][s] * t < m'" (m' = the move term entering the cell, t = stay +
// move, both at their common exponent). The structure (one chain wave, four loader waves, chunks,
// decision words, the walk by runs) is align_dev.h's. What is this kernel's own:
//
//   the chain   alpha[s][p] in xf form. Per sample and j one multiply and one compare; the compare
//               is the decision word j of that sample and step.
//   the loaders one position per load unit. The rows are converted in registers (exp() of the
//               inputs as unnormalized xf, the clamp of the uniforms: nothing transcendental on the
//               chain) on their way to LDS. The chunk's uniforms travel the same way.
//   who decides (HELP, smp_help) in the helper form the chain leaves (t, m') of every cell in a
//               third pair of LDS buffers, and loader wave w decides the rows w, w+4, ... of the
//               previous chunk between issuing its loads and committing them (it alone loads and
//               reads those rows' uniforms, so the barrier per chunk is all the ordering needed).
//   the words   NS*T*K*8 bytes per utterance, [sample][step][j]; stored by the deciding wave.
//   the walks   sample k belongs to wave k mod 5. Each wave reads back into its own share of the
//               chunk buffers, walks, fills its own start[], writes duration / position from it and
//               sums the path's log-probability in f32, 64 gathered terms at a time in step order.
#include <hip/hip_runtime.h>

#include "align_dev.h"

namespace ssnt {
namespace {

constexpr int kSmpMaxR = kAlnLoaders * kAlnMaxRpw;    // rows per chunk, at most
constexpr int kSmpMaxSamples = 64;
constexpr int kSmpUUnits = kSmpMaxR * kSmpMaxSamples / (64 * kAlnLoaders);  // uniforms per loader lane and chunk
constexpr int kSmpUStride = kSmpMaxSamples + 1;       // floats per row of the uniform buffer (padded)
// elements behind each buffer, for unused units' writes: lane (< 64); no unit has a second half
constexpr int kSmpJunk = 64;
constexpr float kSmpUMax = 0x1.fffffep-1f;            // 1 - 2^-24

struct SmpShared {
  int feasible;
};

// Who takes the decisions (measured): the loader waves, a chunk behind the chain,
// from (t, m') rows the chain leaves in LDS -- except one sample on a long row (K >= 8), where the
// chain wave takes them itself.
inline bool smp_help(int U, int NS) { return !(NS == 1 && aln_k(U) >= 8); }
struct SmpLayout {
  int K, R;
  bool help;
  size_t start_off, lt_off, ob_off, u_off, tm_off, bits_off, total;  // bytes
};
// lds_bits: the decision words of the utterance in LDS (else: the workspace, no LDS of their own)
inline SmpLayout smp_layout(int T, int U, int R, int NS, bool obs, bool lds_bits) {
  SmpLayout L{};
  L.K = aln_k(U);
  L.R = R;
  L.help = smp_help(U, NS);
  const size_t buf = (size_t)R * L.K * aln_kstride(L.K) + kSmpJunk;  // elements of one buffer
  const size_t ubuf = (size_t)R * kSmpUStride + kSmpJunk;
  L.start_off = kAlnHeadBytes;
  L.lt_off = (L.start_off + (size_t)kAlnWaves * (U + 2) * 4 + 15) & ~(size_t)15;
  L.ob_off = L.lt_off + 2 * buf * 16;
  L.u_off = L.ob_off + (obs ? 2 * buf * 8 : 0);
  L.tm_off = L.u_off + 2 * ubuf * 4;
  L.bits_off = L.tm_off + (L.help ? 2 * (size_t)R * L.K * 64 * 8 : 0);  // two chunks of (t, m') rows
  L.total = L.bits_off + (lds_bits ? (size_t)NS * T * L.K * 8 : 0);
  return L;
}
// one position per load unit; where LDS is short a chunk goes down to a single row
inline SmpLayout smp_pick(int T, int U, int NS, bool obs, bool lds_bits) {
  return aln_pick(aln_chunk_rows((U + 63) / 64), 1,
                  [&](int r) { return smp_layout(T, U, r, NS, obs, lds_bits); });
}
// The decision words stay in LDS when they fit beside the chunk buffers the log_obs form has in
// workspace mode (from the shape alone: the query does not know whether log_obs is given).
inline bool smp_bits_fit(int T, int U, int NS) {
  const int R = smp_pick(T, U, NS, true, false).R;
  return smp_layout(T, U, R, NS, true, true).total <= kLdsBudget;
}

struct SmpParams {
  int R;
  unsigned start_off, lt_off, ob_off, u_off, tm_off, bits_off;
};

// WS: the decision words live in the workspace (else in LDS); HELP: the loader waves decide
template <int K, bool OBS, bool WS, bool HELP>
__global__ __launch_bounds__(kAlnThreads) void k_sample_align(SampleAlignArgs a, SmpParams q) {
  constexpr int kKs = aln_kstride(K);
  constexpr int kRow = K * kKs;  // LDS row stride in cells
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int T = a.T, U = a.U, R = q.R, NS = a.NS;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const size_t TU = (size_t)T * U;
  const float* lt = a.log_trans + (size_t)b * TU * 2;
  const float* lo = OBS ? a.log_obs + (size_t)b * TU : nullptr;
  const float* un = a.uniform + (size_t)b * NS * T;
  float* lp_out = a.log_prob + (size_t)b * NS;
  int* pos_out = a.position ? a.position + (size_t)b * NS * T : nullptr;
  int* dur_out = a.duration ? a.duration + (size_t)b * NS * U : nullptr;
  const float ninf = -__builtin_inff();

  SmpShared* sh = reinterpret_cast<SmpShared*>(smem);
  int* startb = reinterpret_cast<int*>(smem + q.start_off);
  float4* ltb = reinterpret_cast<float4*>(smem + q.lt_off);
  float2* obb = reinterpret_cast<float2*>(smem + q.ob_off);
  float* ubb = reinterpret_cast<float*>(smem + q.u_off);
  float2* tmb = reinterpret_cast<float2*>(smem + q.tm_off);
  const int bufsz = R * kRow + kSmpJunk;       // cells of one buffer
  const int ubufsz = R * kSmpUStride + kSmpJunk;
  unsigned long long* bits = WS ? reinterpret_cast<unsigned long long*>(a.workspace) + (size_t)b * NS * T * K
                                : reinterpret_cast<unsigned long long*>(smem + q.bits_off);

  auto fill_empty = [&]() {  // the infeasible rule, every sample
    for (int k = tid; k < NS; k += kAlnThreads) lp_out[k] = ninf;
    if (pos_out)
      for (int s = tid; s < NS * T; s += kAlnThreads) pos_out[s] = -1;
    if (dur_out)
      for (int p = tid; p < NS * U; p += kAlnThreads) dur_out[p] = 0;
  };
  if (!aln_lengths_ok(S, P, T, U, a.status, tid)) {
    fill_empty();
    return;
  }

  // ------------------------------------------------------------------ loaders
  // The uniforms of a chunk: row i of sample k at ugoff, to uloff = [i][k].
  const int NC = (S - 1 + R - 1) / R;  // chunks of transition rows 0..S-2
  int goff[kAlnUnits], loff[kAlnUnits], ugoff[kSmpUUnits], uloff[kSmpUUnits];
  f32x2 lreg[kAlnUnits];
  float oreg[OBS ? kAlnUnits : 1], ureg[kSmpUUnits];
  const bool loader = wave >= 1;
  if (loader) {
    const int w = wave - 1;
    const int upr = (U + 63) / 64;  // units per row and lane
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      aln_unit<K>(w, lane, u, upr, 1, 8, R, U, goff[u], loff[u]);
    });
    static_for<kSmpUUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      const int f = u * 64 + lane;  // this wave's rows w, w+4, ... only: it alone reads them back
      const int i = w + kAlnLoaders * (f % kAlnMaxRpw), k = f / kAlnMaxRpw;
      const bool ok = i < R && k < NS;
      ugoff[u] = ok ? (k * T + i) * 4 : kAlnNoUnit;
      uloff[u] = ok ? i * kSmpUStride + k : R * kSmpUStride + lane;
    });
  }
  // global -> registers: transition rows [c*R, min(c*R + R, S-1)); log_obs and uniforms of the
  // rows they lead to, [c*R + 1, ...)
  auto issue = [&](int c) __attribute__((always_inline)) {
    const int r0 = c * R;
    const int n = min(R, S - 1 - r0);
    const __amdgpu_buffer_rsrc_t rs = brsrc(lt + (size_t)r0 * U * 2, (unsigned)(n * U) * 8u);
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      lreg[u] = rbuf_ld2(rs, goff[u], 0, 0);
    });
    if constexpr (OBS) {
      const __amdgpu_buffer_rsrc_t ro = brsrc(lo + (size_t)(r0 + 1) * U, (unsigned)(n * U) * 4u);
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        oreg[u] = rbuf_ld1(ro, goff[u] == kAlnNoUnit ? kAlnNoUnit : goff[u] >> 1, 0, 0);
      });
    }
    // the range ends with row r0 + n of the last sample (r0 + n <= S - 1 < T: inside the tensor)
    const __amdgpu_buffer_rsrc_t ru = brsrc(un + r0 + 1, (unsigned)((NS - 1) * T + n) * 4u);
    static_for<kSmpUUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      ureg[u] = rbuf_ld1(ru, ugoff[u], 0, 0);
    });
  };
  // registers -> LDS buffer c & 1, converted: (E.m, E.e, Sh.m, Sh.e) per cell, (O.m, O.e), and the
  // clamped uniforms (NaN -> 0)
  auto commit = [&](int c) __attribute__((always_inline)) {
    float4* dst = ltb + (size_t)(c & 1) * bufsz;
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      float me, ms;
      int ee, es;
      xf_exp_pair(lreg[u].x, lreg[u].y, true, true, me, ee, ms, es);
      dst[loff[u]] = make_float4(me, __builtin_bit_cast(float, ee), ms, __builtin_bit_cast(float, es));
    });
    if constexpr (OBS) {
      float2* dsto = obb + (size_t)(c & 1) * bufsz;
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        const xf o = xf_exp(oreg[u], true);
        dsto[loff[u]] = make_float2(o.m, __builtin_bit_cast(float, o.e));
      });
    }
    float* dstu = ubb + (size_t)(c & 1) * ubufsz;
    static_for<kSmpUUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      float x = ureg[u];
      x = x >= 0.0f ? x : 0.0f;
      dstu[uloff[u]] = fminf(x, kSmpUMax);
    });
  };

  // ------------------------------------------------------------------ sweep
  float Am[K];
  int Ae[K];
  int mlo = 0, mhi = 0;  // lane j < K: the low / high half of the decision word j in flight
#pragma unroll
  for (int j = 0; j < K; ++j) {
    Am[j] = 0.0f;
    Ae[j] = XF_EZERO;
  }
  if (wave == 0 && lane == 0) {
    const xf a0 = alpha0<OBS>(lo);
    Am[0] = a0.m;
    Ae[0] = a0.e;
  }
  // the decisions of step s (row s of every sample's words) from the aligned terms of its cells
  // and the row's uniforms (lane k: sample k)
  auto decide = [&](const float* tt, const float* mp, float urow, int s) __attribute__((always_inline)) {
    unsigned long long* dst = bits + (size_t)s * K;
    for (int k = 0; k < NS; ++k) {
      const float uk = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, urow), k));
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const bool mv = uk * tt[j] < mp[j];
        aln_put_word(__ballot(mv), j, mlo, mhi);
      }
      if (lane < K) dst[(size_t)k * T * K + lane] = aln_my_word(mlo, mhi);
    }
  };
  // helper form: loader wave w decides rows w, w+4, ... of chunk c from the chain's (t, m') rows
  auto help = [&](int c) __attribute__((always_inline)) {
    const int r0 = c * R;
    const int n = min(R, S - 1 - r0);
    const float2* TM = tmb + (size_t)(c & 1) * R * K * 64 + lane;
    const float* UB = ubb + (size_t)(c & 1) * ubufsz + lane;
    for (int i = wave - 1; i < n; i += kAlnLoaders) {
      float tt[K], mp[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const float2 v = TM[(i * K + j) * 64];
        tt[j] = v.x;
        mp[j] = v.y;
      }
      decide(tt, mp, UB[i * kSmpUStride], r0 + i + 1);
    }
  };
  if (loader && NC > 0) {
    issue(0);
    commit(0);
  }
  __syncthreads();
  for (int c = 0; c < NC; ++c) {
    if (loader && c + 1 < NC) issue(c + 1);
    if (HELP && loader && c > 0) help(c - 1);
    if (wave == 0) {
      const int r0 = c * R;
      const float4* Bf = ltb + (size_t)(c & 1) * bufsz + lane;
      const float2* OB = obb + (size_t)(c & 1) * bufsz + lane;
      const float* UB = ubb + (size_t)(c & 1) * ubufsz + lane;
      struct Row {
        float4 t[K];
        float2 o[OBS ? K : 1];
        float u;
      };
      auto ld = [&](Row& r, int i) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < K; ++j) {
          r.t[j] = Bf[i * kRow + j * kKs];
          if constexpr (OBS) r.o[j] = OB[i * kRow + j * kKs];
        }
        r.u = HELP ? 0.0f : UB[i * kSmpUStride];
      };
      // alpha[s] from alpha[s-1] and transition row s-1 (the operations of alpha_step,
      // lattice_dev.h, with the two aligned terms kept for the decisions)
      auto step = [&](const Row& r, int s) __attribute__((always_inline)) {
        float sm[K], hm[K], tt[K], mp[K];
        int se[K], he[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          sm[j] = Am[j] * r.t[j].x;
          se[j] = Ae[j] + __builtin_bit_cast(int, r.t[j].y);
          hm[j] = Am[j] * r.t[j].z;
          he[j] = Ae[j] + __builtin_bit_cast(int, r.t[j].w);
        }
        const float lm = shr1(hm[K - 1]);
        const int le = shr1(he[K - 1]);
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const float xm = (j == 0) ? lm : hm[j > 0 ? j - 1 : 0];
          const int xe = (j == 0) ? le : he[j > 0 ? j - 1 : 0];
          const int em = max(se[j], xe);
          mp[j] = xldexp(xm, xe - em);
          tt[j] = xldexp(sm[j], se[j] - em) + mp[j];
          float sum = tt[j];
          int ee = em;
          if constexpr (OBS) {
            sum = sum * r.o[j].x;
            ee = ee + __builtin_bit_cast(int, r.o[j].y);
          }
          const xf nv = xf_norm(sum, ee);
          Am[j] = nv.m;
          Ae[j] = nv.e;
        }
        if constexpr (HELP) {  // the terms of row i of this chunk, for the helpers
          float2* TM = tmb + (size_t)(c & 1) * R * K * 64 + lane;
#pragma unroll
          for (int j = 0; j < K; ++j) TM[((s - 1 - r0) * K + j) * 64] = make_float2(tt[j], mp[j]);
        } else {
          decide(tt, mp, r.u, s);
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

  // ------------------------------------------------------------------ feasibility
  if (wave == 0) {
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (K * lane + j == P - 1) v = Am[j];
    if (K * lane <= P - 1 && P - 1 < K * lane + K) sh->feasible = v != 0.0f;  // the one lane that holds P-1
  } else if (HELP && NC > 0) {
    help(NC - 1);  // the last chunk's decisions
  }
  if constexpr (WS) __threadfence();  // the stored words, before the other waves read them
  __syncthreads();
  if (!sh->feasible) {
    fill_empty();
    return;
  }

  // ------------------------------------------------------------------ one walk per sample
  int* start = startb + wave * (U + 2);
  // workspace mode: this wave's share of the chunk buffers holds walk_rows rows of one sample
  const int region = (4 * bufsz / kAlnWaves) / K * K;  // 8-byte words (a cell of the buffer is two)
  unsigned long long* wbuf = reinterpret_cast<unsigned long long*>(ltb) + (size_t)wave * region;
  const int walk_rows = region / K;
  auto pos_of = [&](int s) { return aln_pos_of(start, P, s); };
  for (int k = wave; k < NS; k += kAlnWaves) {
    cbar();
    for (int p = lane; p < P; p += 64) start[p] = 0;
    if (lane == 0) start[P] = S;
    const unsigned long long* kb = bits + (size_t)k * T * K;
    AlnAt at{S - 1, P - 1};
    while (at.p > 0 && at.s >= 1) {
      int lo_row = 0;
      const unsigned long long* wb = kb;
      if constexpr (WS) {  // rows [lo_row, s] of the sample -> this wave's LDS
        lo_row = max(1, at.s - walk_rows + 1);
        cbar();
        aln_read_back<64>(kb + (size_t)lo_row * K, wbuf, (at.s - lo_row + 1) * K, lane);
        cbar();
        wb = wbuf;
      }
      at = aln_walk<K>(wb, lo_row, max(lo_row, 1), lane, start, at.s, at.p);
    }
    cbar();
    aln_write_path<64>(start, S, P, T, U, dur_out ? dur_out + (size_t)k * U : nullptr,
                       pos_out ? pos_out + (size_t)k * T : nullptr, lane);
    // log_prob: the sequential f32 sum of DESIGN.md 2.4, 64 steps' terms gathered at a time
    float v = OBS ? lo[0] : 0.0f;
    for (int s0 = 0; s0 < S - 1; s0 += 64) {
      const int ss = s0 + lane;
      float x = 0.0f, y = 0.0f;
      if (ss < S - 1) {
        const int p0 = pos_of(ss), p1 = pos_of(ss + 1);
        x = lt[((size_t)ss * U + p0) * 2 + (p1 - p0)];
        if constexpr (OBS) y = lo[(size_t)(ss + 1) * U + p1];
      }
      const int n = min(64, S - 1 - s0);
      for (int i = 0; i < n; ++i) {
        v = v + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), i));
        if constexpr (OBS)
          v = v + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y), i));
      }
    }
    if (a.flags & SSNT_FLAG_TERMINAL_EMIT) v = v + lt[((size_t)(S - 1) * U + (P - 1)) * 2];
    if (lane == 0) lp_out[k] = v;
  }
}

template <int K, bool OBS, bool WS>
int launch_sample_k(const SampleAlignArgs& a, const SmpLayout& L, hipStream_t st) {
  const SmpParams q{L.R, (unsigned)L.start_off, (unsigned)L.lt_off, (unsigned)L.ob_off,
                    (unsigned)L.u_off, (unsigned)L.tm_off, (unsigned)L.bits_off};
  if (L.help)
    return launch_lds(k_sample_align<K, OBS, WS, true>, dim3(a.B), dim3(kAlnThreads), L.total, kLdsBudget, st, a, q);
  return launch_lds(k_sample_align<K, OBS, WS, false>, dim3(a.B), dim3(kAlnThreads), L.total, kLdsBudget, st, a, q);
}

}  // namespace

size_t sample_align_workspace_bytes(int B, int T, int U, int NS) {
  if (smp_bits_fit(T, U, NS)) return 0;
  return (size_t)B * NS * T * aln_k(U) * 8;
}

int launch_sample_align(const SampleAlignArgs& a, hipStream_t st) {
  // (NS and uniform: each beside the shared checks that return the same code, so no precedence moves)
  if (a.NS < 1 || a.NS > kSmpMaxSamples) return SSNT_ERR_INVALID_ARG;
  const int rc = aln_check_args(a.B, a.T, a.U, a.flags,
                                a.log_trans && a.step_len && a.pos_len && a.uniform && a.log_prob, a.log_trans,
                                a.log_obs);
  if (rc != SSNT_OK || a.B == 0) return rc;
  if (!aligned_to(a.uniform, 4)) return SSNT_ERR_UNSUPPORTED;
  // the byte offsets of the range-checked loads are 32-bit
  if ((size_t)a.NS * a.T * 4 >= (size_t)kAlnNoUnit) return SSNT_ERR_UNSUPPORTED;
  const bool obs = a.log_obs != nullptr;
  const int U = a.U > 0 ? a.U : 1;  // (T == 0 or U == 0: every utterance is infeasible)
  const bool fit = a.T == 0 || a.U == 0 || smp_bits_fit(a.T, U, a.NS);
  if (!fit && !aln_workspace_ok(a.workspace, a.workspace_bytes, sample_align_workspace_bytes(a.B, a.T, a.U, a.NS)))
    return SSNT_ERR_WORKSPACE;
  const SmpLayout L = smp_pick(a.T, U, a.NS, obs, fit);
  if (L.total > kLdsBudget) return SSNT_ERR_UNSUPPORTED;
  return aln_with_k(L.K, [&](auto Kc) {
    constexpr int K = decltype(Kc)::value;
    if (fit) return obs ? launch_sample_k<K, true, false>(a, L, st) : launch_sample_k<K, false, false>(a, L, st);
    return obs ? launch_sample_k<K, true, true>(a, L, st) : launch_sample_k<K, false, true>(a, L, st);
  });
}

}  // namespace ssnt
