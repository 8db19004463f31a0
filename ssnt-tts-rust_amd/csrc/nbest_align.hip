// nbest_align.hip -- the exact N best alignments over the emit/shift lattice for gfx950.
//
// Semantics: DESIGN.md 2.6. The max-plus sweep of viterbi.hip with a sorted list of NB entries per
// cell instead of one value: f32 adds and compares under one total order (value descending, tag
// ascending), nothing reassociated, so every form is bit-identical to the plain f32 restatement
// (tests/nbest_ref.py). The structure (one chain wave, four loader waves, chunks, the backtrace in
// the same launch) is align_dev.h's; the loaders are k_viterbi's. What is this kernel's own:
//
//   the chain   V[k][r], r = 0..NB-1 sorted, in f32. Per cell 2*NB adds, NB compare-selects of
//               stay_i against move_{NB-1-i} (the NB best of both lists, as a bitonic sequence) and
//               log2(NB) clean-up stages; a tag (r for stay_r, NB + r for move_r) travels with each
//               value in a register of its own. k runs downwards so the old V[k-1] is still there.
//   the tags    ceil(log2(2*NB)) bits each, NB per cell, the K cells of a lane packed into one
//               record of K*NB*bits bits: a byte, a half word, or 1..4 dwords per lane and step,
//               stored [step][dword][lane] (consecutive lanes, conflict-free, K-independent count
//               of stores). In LDS when T rows fit beside the chunk buffers, else straight to the
//               caller's workspace with ordinary vector stores (every lane stores its own record,
//               so there is nothing to stage). With no path output nothing is kept.
//   the walk    the rank changes from step to step, so there are no runs to ballot for: lane n of
//               wave 0 walks rank n, one LDS read per step, all ranks at the same step. NB = 1 has
//               no rank to follow and walks by runs like aln_walk, over its own records. In
//               workspace mode all waves read a block of rows back into the chunk buffers first.
//               start[] per rank, then aln_write_path by all waves.
//
// Envelope: num_best 1..8, run as NB = 1, 2, 4, 8; aln_k(max_pos) * NB <= 32 (the list registers of
// the chain), so max_pos <= 256 for N > 4, <= 512 for N > 2, <= 1024 else.
#include <hip/hip_runtime.h>

#include "align_dev.h"

namespace ssnt {
namespace {

// elements behind each buffer, for unused units' writes (as kVitJunk, viterbi.hip)
constexpr int kNbJunk = 160;
constexpr int kNbMaxBest = 8;
constexpr int kNbMaxRegs = 32;  // K * NB at most

// the DPP wave shift with -inf for lane 0 (as shr1_ninf, viterbi.hip): never under a select on the
// lane index
__device__ __forceinline__ float nb_shr1_ninf(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp((int)0xff800000u, __builtin_bit_cast(int, x),
                                                               0x138, 0xf, 0xf, false));
}

// ---------------------------------------------------------------------- the tag records
constexpr int nb_round(int N) { return N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : 8; }
constexpr int nb_tag_bits(int NB) { return NB == 1 ? 1 : NB == 2 ? 2 : NB == 4 ? 3 : 4; }
constexpr int nb_lane_bits(int K, int NB) { return K * NB * nb_tag_bits(NB); }
// bytes of one stored element and elements per lane and step
constexpr int nb_elem_bytes(int K, int NB) { return nb_lane_bits(K, NB) <= 8 ? 1 : nb_lane_bits(K, NB) <= 16 ? 2 : 4; }
constexpr int nb_words(int K, int NB) { return nb_lane_bits(K, NB) <= 32 ? 1 : (nb_lane_bits(K, NB) + 31) / 32; }
constexpr int nb_row_bytes(int K, int NB) { return 64 * nb_elem_bytes(K, NB) * nb_words(K, NB); }

// this lane's record of step `row` -> base (LDS or the workspace)
template <int K, int NB>
__device__ __forceinline__ void nb_store(unsigned char* base, int row, int lane, const unsigned* pk) {
  constexpr int kEb = nb_elem_bytes(K, NB), kW = nb_words(K, NB);
  if constexpr (kEb == 1) {
    base[(size_t)row * 64 + lane] = (unsigned char)pk[0];
  } else if constexpr (kEb == 2) {
    reinterpret_cast<unsigned short*>(base)[(size_t)row * 64 + lane] = (unsigned short)pk[0];
  } else {
    unsigned* dst = reinterpret_cast<unsigned*>(base) + (size_t)row * kW * 64 + lane;
#pragma unroll
    for (int w = 0; w < kW; ++w) dst[w * 64] = pk[w];
  }
}
// the tag of rank r of position p (0 <= p < 64 * K, 0 <= r < NB) at step `row` of the block at base
template <int K, int NB>
__device__ __forceinline__ int nb_read_tag(const unsigned char* base, int row, int p, int r) {
  constexpr int kEb = nb_elem_bytes(K, NB), kW = nb_words(K, NB), kTb = nb_tag_bits(NB);
  const int ln = p / K;
  const int off = ((p % K) * NB + r) * kTb;
  unsigned long long v;
  if constexpr (kEb == 1) {
    v = base[(size_t)row * 64 + ln];
  } else if constexpr (kEb == 2) {
    v = reinterpret_cast<const unsigned short*>(base)[(size_t)row * 64 + ln];
  } else {
    const unsigned* src = reinterpret_cast<const unsigned*>(base) + (size_t)row * kW * 64 + ln;
    const int w = off >> 5;
    v = src[w * 64];
    if constexpr (kW > 1) v |= (unsigned long long)src[min(w + 1, kW - 1) * 64] << 32;  // a tag may straddle
    return (int)(v >> (off & 31)) & ((1 << kTb) - 1);
  }
  return (int)(v >> off) & ((1 << kTb) - 1);
}

struct NbShared {
  int count;  // present ranks among the num_best requested
};

struct NbLayout {
  int K, NB, R;
  size_t start_off, lt_off, ob_off, bp_off, total;  // bytes
};
inline size_t nb_row_bytes_rt(int K, int NB) {
  const int bits = K * NB * nb_tag_bits(NB);
  const int eb = bits <= 8 ? 1 : bits <= 16 ? 2 : 4;
  return (size_t)64 * eb * (bits <= 32 ? 1 : (bits + 31) / 32);
}
// mode: 0 no tags kept, 1 tag records in LDS, 2 in the workspace (no LDS of their own)
inline NbLayout nb_layout(int T, int U, int NB, int R, bool obs, int mode) {
  NbLayout L{};
  L.K = aln_k(U);
  L.NB = NB;
  L.R = R;
  const size_t buf = (size_t)R * L.K * aln_kstride(L.K) + kNbJunk;  // elements of one buffer
  L.start_off = kAlnHeadBytes;
  L.lt_off = (L.start_off + (size_t)NB * (U + 2) * 4 + 15) & ~(size_t)15;
  L.ob_off = L.lt_off + 2 * buf * 8;
  L.bp_off = (L.ob_off + (obs ? 2 * buf * 4 : 0) + 15) & ~(size_t)15;
  L.total = L.bp_off + (mode == 1 ? (size_t)T * nb_row_bytes_rt(L.K, NB) : 0);
  return L;
}
// the unit geometry of k_viterbi's loaders (vit_pick)
inline NbLayout nb_pick(int T, int U, int NB, bool wide_units, bool obs, int mode) {
  const int R = aln_chunk_rows(wide_units ? (U + 127) / 128 : (U + 63) / 64);
  return aln_pick(R, kAlnLoaders, [&](int r) { return nb_layout(T, U, NB, r, obs, mode); });
}
// The records stay in LDS when they fit beside the chunk buffers the log_obs form has in
// workspace mode (from the shape alone: the query knows neither log_obs nor the alignment).
inline bool nb_tags_fit(int T, int U, int NB) {
  const int R = nb_pick(T, U, NB, false, true, 2).R;
  return nb_layout(T, U, NB, R, true, 1).total <= kLdsBudget;
}

struct NbParams {
  int R;
  int vec;  // log_trans moves in 16-byte units (16-byte aligned, U even), else 8-byte
  unsigned start_off, lt_off, ob_off, bp_off;
};

// MODE: 0 no path output (no tags), 1 tag records in LDS, 2 in the workspace
template <int K, int NB, bool OBS, int MODE>
__global__ __launch_bounds__(kAlnThreads) void k_nbest_align(NbestAlignArgs a, NbParams q) {
  constexpr int kKs = aln_kstride(K);
  constexpr int kRow = K * kKs;  // LDS row stride (float2 units for log_trans, floats for log_obs)
  constexpr int kTb = nb_tag_bits(NB);
  constexpr int kW = nb_words(K, NB);
  constexpr int kRowBytes = nb_row_bytes(K, NB);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int T = a.T, U = a.U, R = q.R, N = a.N;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const size_t TU = (size_t)T * U;
  const float* lt = a.log_trans + (size_t)b * TU * 2;
  const float* lo = OBS ? a.log_obs + (size_t)b * TU : nullptr;
  float* lp_out = a.log_prob + (size_t)b * N;
  int* pos_out = (MODE && a.position) ? a.position + (size_t)b * N * T : nullptr;
  int* dur_out = (MODE && a.duration) ? a.duration + (size_t)b * N * U : nullptr;
  const float ninf = -__builtin_inff();

  NbShared* sh = reinterpret_cast<NbShared*>(smem);
  int* startb = reinterpret_cast<int*>(smem + q.start_off);  // [rank][U + 2]
  float2* ltb = reinterpret_cast<float2*>(smem + q.lt_off);
  float* obb = reinterpret_cast<float*>(smem + q.ob_off);
  const int bufsz = R * kRow + kNbJunk;  // elements of one buffer
  unsigned char* bp = MODE == 2 ? reinterpret_cast<unsigned char*>(a.workspace) + (size_t)b * T * kRowBytes
                                : smem + q.bp_off;
  // workspace mode, backtrace: the log_trans chunk buffers are free by then
  unsigned char* wbuf = reinterpret_cast<unsigned char*>(ltb);
  const int walk_rows = 2 * bufsz * 8 / kRowBytes;

  // the absent rule for ranks [r0, N): positions -1, durations 0
  auto fill_absent = [&](int r0) {
    if (pos_out)
      for (int i = r0 * T + tid; i < N * T; i += kAlnThreads) pos_out[i] = -1;
    if (dur_out)
      for (int i = r0 * U + tid; i < N * U; i += kAlnThreads) dur_out[i] = 0;
  };
  if (!aln_lengths_ok(S, P, T, U, a.status, tid)) {
    if (tid < N) lp_out[tid] = ninf;
    fill_absent(0);
    return;
  }

  // ------------------------------------------------------------------ loaders (as k_viterbi)
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
  float V[K][NB];
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int r = 0; r < NB; ++r) V[k][r] = ninf;
  if (wave == 0 && lane == 0) V[0][0] = OBS ? lo[0] : 0.0f;
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
      // the lists of row s from those of row s-1 and transition row s-1
      auto step = [&](const Row& row, int s) __attribute__((always_inline)) {
        unsigned pk[kW];
#pragma unroll
        for (int w = 0; w < kW; ++w) pk[w] = 0u;
        float left[NB];  // the left neighbour's move list, for k = 0
#pragma unroll
        for (int r = 0; r < NB; ++r) left[r] = nb_shr1_ninf(V[K - 1][r] + row.t[K - 1].y);
        static_for<K>([&](auto Kc) __attribute__((always_inline)) {
          constexpr int k = K - 1 - decltype(Kc)::value;  // downwards: V[k-1] is still row s-1
          float cv[NB];
          int ct[NB];
          // the NB best of both sorted lists: stay_i against move_{NB-1-i}. A stay tag is below
          // every move tag, so "move first" is the strict compare (a tie keeps the emit).
          static_for<NB>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int i = decltype(Ic)::value;
            constexpr int j = NB - 1 - i;
            const float stay = V[k][i] + row.t[k].x;
            float move;
            if constexpr (k == 0) move = left[j];
            else move = V[k > 0 ? k - 1 : 0][j] + row.t[k > 0 ? k - 1 : 0].y;
            const bool m = move > stay;
            cv[i] = m ? move : stay;
            ct[i] = m ? NB + j : i;
          });
          // bitonic clean-up under (value descending, tag ascending)
#pragma unroll
          for (int d = NB / 2; d >= 1; d >>= 1) {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
              if ((i & d) == 0) {
                const float va = cv[i], vb = cv[i + d];
                const int ta = ct[i], tb = ct[i + d];
                const bool keep = va > vb || (va == vb && ta < tb);
                cv[i] = keep ? va : vb;
                cv[i + d] = keep ? vb : va;
                ct[i] = keep ? ta : tb;
                ct[i + d] = keep ? tb : ta;
              }
            }
          }
          static_for<NB>([&](auto Ic) __attribute__((always_inline)) {
            constexpr int i = decltype(Ic)::value;
            float v = cv[i];
            if constexpr (OBS) v = v + row.o[k];
            V[k][i] = v;
            if constexpr (MODE != 0) {
              constexpr int off = (k * NB + i) * kTb;
              pk[off / 32] |= (unsigned)ct[i] << (off % 32);
              if constexpr (off % 32 + kTb > 32) pk[off / 32 + 1] |= (unsigned)ct[i] >> (32 - off % 32);
            }
          });
        });
        if constexpr (MODE != 0) nb_store<K, NB>(bp, s, lane, pk);
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

  // ------------------------------------------------------------------ log_prob, present ranks
  if (wave == 0) {
    if (K * lane <= P - 1 && P - 1 < K * lane + K) {  // the one lane that holds P-1
      float fin[NB];
#pragma unroll
      for (int r = 0; r < NB; ++r) fin[r] = ninf;
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (K * lane + k == P - 1) {
#pragma unroll
          for (int r = 0; r < NB; ++r) fin[r] = V[k][r];
        }
      const bool term = (a.flags & SSNT_FLAG_TERMINAL_EMIT) != 0;
      const float te = term ? lt[((size_t)(S - 1) * U + (P - 1)) * 2] : 0.0f;
      int count = 0;  // present ranks come first: the list is sorted
#pragma unroll
      for (int r = 0; r < NB; ++r) {
        if (r < N) {
          float v = fin[r];
          if (term) v = v + te;
          const bool present = count == r && v > ninf;
          lp_out[r] = present ? v : ninf;
          count += present;
        }
      }
      sh->count = count;
    }
    if constexpr (MODE == 2) __threadfence();  // the stored records, before the other waves read them
  }
  if constexpr (MODE == 0) return;
  __syncthreads();
  const int count = sh->count;
  fill_absent(count);
  if (count == 0) return;

  // ------------------------------------------------------------------ backtrace, a lane per rank
  const int sstride = U + 2;
  for (int i = tid; i < count * sstride; i += kAlnThreads) {
    const int p = i % sstride;
    if (p <= P) startb[i] = p == P ? S : 0;
  }
  {
    int p = P - 1;
    [[maybe_unused]] int r = lane;
    [[maybe_unused]] const bool walker = wave == 0 && lane < count;
    int s = S - 1;  // uniform: every rank is at the same step
    while (s >= 1) {
      int lo_row = 1;
      const unsigned char* blk = bp;
      if constexpr (MODE == 2) {  // steps [lo_row, s] of the workspace -> LDS, by all waves
        lo_row = max(1, s - walk_rows + 1);
        __syncthreads();  // the previous block's walk is over
        aln_read_back<kAlnThreads>(reinterpret_cast<const unsigned long long*>(bp + (size_t)lo_row * kRowBytes),
                                   reinterpret_cast<unsigned long long*>(wbuf), (s - lo_row + 1) * (kRowBytes / 8),
                                   tid);
        blk = wbuf;
      }
      __syncthreads();  // start[] and the block are there
      const int base_row = MODE == 2 ? lo_row : 0;  // the step that row 0 of blk holds
      if constexpr (NB == 1) {
        // one path and no rank to follow: wave 0 walks it by runs, as aln_walk does over its words
        // (64 lanes test the tag of position p at 64 consecutive steps, one ballot finds the step
        // that entered p)
        if (wave == 0) {
          int sw = s;
          while (p > 0 && sw >= lo_row) {
            const int ss = sw - lane;
            int bit = 0;
            if (ss >= lo_row) bit = nb_read_tag<K, NB>(blk, ss - base_row, p, 0);
            const unsigned long long m = __ballot(bit != 0);
            if (m == 0) {
              sw = max(sw - 64, lo_row - 1);
            } else {
              const int st = sw - (__ffsll((long long)m) - 1);
              if (lane == 0) startb[p] = st;
              sw = st - 1;
              p -= 1;
            }
          }
        }
      } else if (walker) {
        for (int ss = s; ss >= lo_row && p > 0; --ss) {
          const int tag = nb_read_tag<K, NB>(blk, ss - base_row, p, r);
          if (tag >= NB) {  // entered p at step ss (p > 0 here: the walk never leaves the lattice)
            startb[lane * sstride + p] = ss;
            p -= 1;
          }
          r = tag & (NB - 1);
        }
      }
      s = lo_row - 1;
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ outputs
  for (int r = 0; r < count; ++r)
    aln_write_path<kAlnThreads>(startb + r * sstride, S, P, T, U, dur_out ? dur_out + (size_t)r * U : nullptr,
                                pos_out ? pos_out + (size_t)r * T : nullptr, tid);
}

template <int K, int NB, bool OBS>
int launch_nbest_obs(const NbestAlignArgs& a, const NbLayout& L, bool vec, int mode, hipStream_t st) {
  const NbParams q{L.R, vec, (unsigned)L.start_off, (unsigned)L.lt_off, (unsigned)L.ob_off, (unsigned)L.bp_off};
  const dim3 grid(a.B), block(kAlnThreads);
  if (mode == 0) return launch_lds(k_nbest_align<K, NB, OBS, 0>, grid, block, L.total, kLdsBudget, st, a, q);
  if (mode == 1) return launch_lds(k_nbest_align<K, NB, OBS, 1>, grid, block, L.total, kLdsBudget, st, a, q);
  return launch_lds(k_nbest_align<K, NB, OBS, 2>, grid, block, L.total, kLdsBudget, st, a, q);
}

template <int NB>
int launch_nbest_nb(const NbestAlignArgs& a, const NbLayout& L, bool vec, bool obs, int mode, hipStream_t st) {
  return aln_with_k(L.K, [&](auto Kc) {
    constexpr int K = decltype(Kc)::value;
    if constexpr (K * NB <= kNbMaxRegs) {
      return obs ? launch_nbest_obs<K, NB, true>(a, L, vec, mode, st)
                 : launch_nbest_obs<K, NB, false>(a, L, vec, mode, st);
    } else {
      return (int)SSNT_ERR_UNSUPPORTED;
    }
  });
}

inline bool nb_supported(int U, int N) {
  return N >= 1 && N <= kNbMaxBest && U <= 1024 && aln_k(U > 0 ? U : 1) * nb_round(N) <= kNbMaxRegs;
}

}  // namespace

size_t nbest_align_workspace_bytes(int B, int T, int U, int N) {
  if (!nb_supported(U, N)) return 0;
  const int NB = nb_round(N);
  if (nb_tags_fit(T, U, NB)) return 0;
  return (size_t)B * T * nb_row_bytes_rt(aln_k(U), NB);
}

int launch_nbest_align(const NbestAlignArgs& a, hipStream_t st) {
  if (a.N < 1 || a.N > kNbMaxBest) return SSNT_ERR_INVALID_ARG;
  const int rc = aln_check_args(a.B, a.T, a.U, a.flags, a.log_trans && a.step_len && a.pos_len && a.log_prob,
                                a.log_trans, a.log_obs);
  if (rc != SSNT_OK || a.B == 0) return rc;
  if (!nb_supported(a.U, a.N)) return SSNT_ERR_UNSUPPORTED;
  const int NB = nb_round(a.N);
  const bool path = a.position || a.duration;
  const bool obs = a.log_obs != nullptr;
  const int U = a.U > 0 ? a.U : 1;  // (T == 0 or U == 0: every utterance is infeasible)
  const bool fit = a.T == 0 || a.U == 0 || nb_tags_fit(a.T, U, NB);
  if (path && !fit &&
      !aln_workspace_ok(a.workspace, a.workspace_bytes, nbest_align_workspace_bytes(a.B, a.T, a.U, a.N)))
    return SSNT_ERR_WORKSPACE;
  const int mode = !path ? 0 : fit ? 1 : 2;
  const bool vec = aligned_to(a.log_trans, 16) && U % 2 == 0;
  const NbLayout L = nb_pick(a.T, U, NB, vec && !obs, obs, mode);
  if (L.total > kLdsBudget) return SSNT_ERR_UNSUPPORTED;
  switch (NB) {
    case 1: return launch_nbest_nb<1>(a, L, vec, obs, mode, st);
    case 2: return launch_nbest_nb<2>(a, L, vec, obs, mode, st);
    case 4: return launch_nbest_nb<4>(a, L, vec, obs, mode, st);
    default: return launch_nbest_nb<8>(a, L, vec, obs, mode, st);
  }
}

}  // namespace ssnt
