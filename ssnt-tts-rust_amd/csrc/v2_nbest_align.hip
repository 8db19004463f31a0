// v2_nbest_align.hip -- the exact N best duration paths on the v2 duration-class lattice, gfx950.
//
// Semantics: DESIGN.md 2.7. The max-plus sweep of v2_viterbi.hip with a sorted list of NB entries
// per cell instead of one value: IEEE f32 adds and ordered compares under one total order (value
// descending, then class, then predecessor rank ascending), nothing contracted or reassociated,
// so every form is bit-identical to the plain f32 restatement (tests/v2_nbest_ref.py). num_best
// 1..8 runs at list width NB = 1, 2, 4, 8: a rank does not depend on the width.
//
// Layout. One workgroup (512 threads) per utterance, as k_v2_viterbi; what that kernel's sweep
// needs (chunk staging, the padded and the clamped cell addressing, the read-back) is restated
// here, the windows and the no-lattice rule are v2_lattice_dev.h's:
//   LDS:  final list | duration table | path bytes [rank][step] | class log-probs (f32, chunks of
//         64 or 32 steps, double-buffered, the class rule applied: a masked class and every unused
//         class slot hold -inf) | 2 row buffers (ping-pong, window-relative) of NB planes, plane q
//         holding rank q of every cell with kF4Pad cells of -inf on both sides of its window, so a
//         wave reads 64 consecutive cells of one rank | backpointers (LDS mode)
// A cell: a running list of NB (value, key) registers, -inf at first. The classes in increasing
// order; class i's candidates are the predecessor cell's list plus w[i] (NB reads, NB adds; still
// sorted, the add is monotone), key i * NB + q. Every key of class i is above every key already
// kept, so the first merge stage is NB strict `cand > kept` compare-selects of kept_j against
// cand_{NB-1-j} (the NB best of both, as a bitonic sequence), followed by log2(NB) clean-up stages
// under the full order. At NB = 1 that is k_v2_viterbi's `c > best`. A class whose best candidate
// does not beat the list's last entry changes nothing: the merge is skipped when that holds for
// every lane of the wave (bit-exact).
//   Classes and offsets: at NB = 1 in registers with the class loop unrolled, as k_v2_viterbi. At
//   NB > 1 the loop is rolled over the D real classes, offsets and weights reread from LDS at
//   uniform addresses, software-pipelined: the cells of class i + 1 and the offset and weight of
//   class i + 2 are loading while class i merges (the unrolled form of the merge is a code size
//   no instance needs: the merge, not the loop, is the cost).
//
// Backpointers: one entry i * NB + q per (row, rank, window cell), a byte where DC * NB <= 256,
// else 16 bits, stored [row][rank][cell] (a wave stores 64 consecutive elements): in LDS when one
// utterance's fit beside the buffers, else in the caller's workspace. No path output: none kept.
//
// Final selection: wave 0 takes the N best of (value, total x, rank q) over the last window,
// per-lane sorted lists merged by an xor butterfly under the full order. Walk: lane n of wave 0
// walks rank n, all ranks on the same row, one entry read per step; class, rank and cell are
// masked and clamped, so no input takes a read outside the block. In workspace mode the rows are
// first read back in blocks into the LDS the sweep no longer needs (agent-scope loads that bypass
// the per-CU cache, 8 in flight per lane, after __threadfence() and a full __syncthreads()).
#include <hip/hip_runtime.h>
#include <limits.h>

#include "buffer_ops.h"
#include "launch_util.h"
#include "ssnt_internal.h"
#include "v2_lattice_dev.h"

// the merge's wave-uniform shortcut; 0 only in a measurement build (tools/bench_v2_nbest_align.py)
#ifndef SSNT_V2NB_SKIP
#define SSNT_V2NB_SKIP 1
#endif

namespace ssnt {
namespace {

constexpr int kVnThreads = 512;
constexpr size_t kVnLdsBudget = 160 * 1024 - 256;  // one workgroup per CU may use ~all 160 KiB
constexpr size_t kVnWalkTarget = 80 * 1024;        // workspace mode: LDS up to which the read-back block grows
constexpr int kVnMaxBest = 8;
constexpr unsigned kVnHead = 128;  // VnShared

struct VnShared {
  int count, pad[3];
  float value[kVnMaxBest];
  int x[kVnMaxBest], q[kVnMaxBest];
};
static_assert(sizeof(VnShared) <= kVnHead, "head");

constexpr int vn_round(int N) { return N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : 8; }
constexpr int vn_log2(int NB) { return NB == 1 ? 0 : NB == 2 ? 1 : NB == 4 ? 2 : 3; }
constexpr int vn_entry_bytes(int DC, int NB) { return DC * NB <= 256 ? 1 : 2; }
constexpr bool vn_unrolled(int DC, int NB) { return NB == 1; }
template <int DC>
constexpr int vn_chunk() { return DC <= 32 ? 64 : 32; }  // sweep steps per staged chunk (= F4's)

// LDS carve of one launch; mode: 0 no backpointers, 1 backpointers in LDS, 2 in the workspace.
// The launcher and the size query both come here.
struct VnLayout {
  unsigned dur_off, path_off, cw_off, row_off, bp_off;
  int path_stride;  // bytes of one rank's path
  int walk_rows;    // mode 2: rows per read-back block
  size_t total;
};
inline VnLayout vn_layout(int Imax, int Wc, int DC, int NB, int mode) {
  VnLayout L{};
  const size_t a16 = 15;
  L.dur_off = kVnHead;
  L.path_off = L.dur_off + (unsigned)DC * 4;
  const size_t ps = ((size_t)Imax + a16) & ~a16;
  L.path_stride = (int)ps;
  const size_t cw = L.path_off + (mode ? (size_t)NB * ps : 0);
  const int ch = DC <= 32 ? 64 : 32;
  const size_t rowo = cw + 2u * ch * DC * 4;
  const size_t rowb = (2 * (size_t)NB * ((size_t)Wc + 2 * kF4Pad + 2) * 4 + a16) & ~a16;
  const size_t sweep_end = rowo + rowb;
  L.cw_off = (unsigned)cw;
  L.row_off = (unsigned)rowo;
  L.bp_off = (unsigned)sweep_end;
  L.total = sweep_end;
  const size_t rb = (size_t)Wc * NB * vn_entry_bytes(DC, NB);  // the entries of one lattice row
  if (mode == 1) L.total = sweep_end + (((size_t)Imax * rb + a16) & ~a16);
  if (mode == 2) {
    // the block lies over the class log-probs and the row buffers (free after the selection)
    size_t avail = sweep_end - cw;
    if (kVnWalkTarget > cw && kVnWalkTarget - cw > avail) avail = kVnWalkTarget - cw;
    size_t rows = (avail - 8) / rb;  // (8: the block starts on a dword of the workspace)
    rows = rows < 1 ? 1 : rows > (size_t)Imax ? (size_t)Imax : rows;
    L.walk_rows = (int)rows;
    const size_t blk = (rows * rb + 8 + a16) & ~a16;
    L.total = cw + (blk > sweep_end - cw ? blk : sweep_end - cw);
  }
  return L;
}
// From the shape alone (the size query does not know D): entries as wide as the widest class
// padding makes them, in LDS when they fit beside that padding's buffers (v2v_bits_fit's rule).
inline size_t vn_row_bytes_q(int Wc, int NB) { return (size_t)Wc * NB * vn_entry_bytes(64, NB); }
inline bool vn_bits_fit(int Imax, int Wc, int NB) { return vn_layout(Imax, Wc, 64, NB, 1).total <= kVnLdsBudget; }
inline size_t vn_ws_stride(int Imax, int Wc, int NB) {
  return ((size_t)Imax * vn_row_bytes_q(Wc, NB) + 4 + 15) & ~(size_t)15;
}

struct VnParams {
  unsigned dur_off, path_off, cw_off, row_off, bp_off;
  int path_stride, walk_rows;
  unsigned long long ws_stride;
};

// `a` before `b` under the full order: value descending, key ascending
__device__ __forceinline__ bool vn_before(float va, int ka, float vb, int kb) {
  return va > vb || (va == vb && ka < kb);
}

// the bitonic clean-up of NB entries under the full order
template <int NB>
__device__ __forceinline__ void vn_cleanup(float (&R)[NB], int (&K)[NB]) {
#pragma unroll
  for (int d = NB / 2; d >= 1; d >>= 1) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if ((j & d) == 0) {
        const float va = R[j], vb = R[j + d];
        const int ka = K[j], kb = K[j + d];
        const bool keep = vn_before(va, ka, vb, kb);
        R[j] = keep ? va : vb;
        R[j + d] = keep ? vb : va;
        K[j] = keep ? ka : kb;
        K[j + d] = keep ? kb : ka;
      }
    }
  }
}

// The NB best of the kept list and a sorted candidate list whose keys key0 + q all lie above
// every kept key: a tie keeps the kept entry, so the first stage is the strict compare.
template <int NB>
__device__ __forceinline__ void vn_merge(float (&R)[NB], int (&K)[NB], const float (&c)[NB], int key0) {
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int jj = NB - 1 - j;
    const bool m = c[jj] > R[j];  // strict: a NaN never enters
    R[j] = m ? c[jj] : R[j];
    K[j] = m ? key0 + jj : K[j];
  }
  vn_cleanup<NB>(R, K);
}

// The sweep: rows 1..I from row 0 = {total 0: [0.0f, -inf, ...]}. On return the last row is in row
// buffer I & 1, its window [plo, phi]. false: a window beyond the row capacity (reported).
//  PADDED (dmax <= kF4Pad): kF4Pad cells of -inf on both sides of every plane's window; the cell
//   offset is clamped into the band from which every candidate stays inside them.
//  else: offsets are taken +1, so anything left of the window wraps to a huge unsigned value and
//   one unsigned min clamps an out-of-window candidate onto the -inf cell just right of the
//   window (index span + 1); offset 0 is the -inf cell left of it (index -1).
template <int DC, int NB, bool PADDED, int MODE>
__device__ __forceinline__ bool vn_sweep(const V2NbestArgs& a, const VnParams& q, unsigned char* smem,
                                         const F4Utt& u, int& plo, int& phi) {
  constexpr int CH = vn_chunk<DC>();
  constexpr int NPF = (CH * DC + kVnThreads - 1) / kVnThreads;  // staged values per thread
  constexpr bool UNR = vn_unrolled(DC, NB);
  constexpr int EB = vn_entry_bytes(DC, NB);
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int D = a.D, Imax = a.Imax, Wc = a.Wcap, dmax = u.dmax, I = u.I;
  const float ninf = -__builtin_inff();
  const int* dur = reinterpret_cast<const int*>(smem + q.dur_off);
  float* cw = reinterpret_cast<float*>(smem + q.cw_off);  // [2][CH][DC]
  float* row = reinterpret_cast<float*>(smem + q.row_off);
  const int RS = Wc + 2 * kF4Pad + 2;                                // cells of one plane
  auto rw = [&](int k) { return row + k * NB * RS + kF4Pad; };       // buffer k, plane 0, window cell 0
  unsigned char* bp = MODE == 2 ? reinterpret_cast<unsigned char*>(a.workspace) + (size_t)b * q.ws_stride
                                : smem + q.bp_off;                   // [I][NB][Wc] entries
  const float* lg = a.logits + (size_t)b * Imax * D;
  int dk[UNR ? DC : 1];  // candidate offsets (VGPRs)
  if constexpr (UNR) {
#pragma unroll
    for (int i = 0; i < DC; ++i) dk[i] = dur[i];
  }
  float pre[NPF];
  // class log-probs through one descriptor: masked entries read past its end, so the loads need
  // no exec mask (their value is never used: put_chunk writes -inf for them)
  const __amdgpu_buffer_rsrc_t lg_r = brsrc(lg, (unsigned)((size_t)Imax * D * sizeof(float)));
  auto load_chunk = [&](int c) {  // chunk c = sweep steps [c CH, (c + 1) CH)
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int idx = tid + kVnThreads * j;
      const int k = c * CH + idx / DC, i = idx % DC;
      const bool live = idx < CH * DC && i < D && k < I;
      pre[j] = rbuf_ld1(lg_r, live ? (k * D + i) * (int)sizeof(float) : (int)0x80000000, 0, 0);
    }
  };
  auto put_chunk = [&](int c) {  // ... into the chunk's LDS buffer, the class rule applied
    float* dst = cw + (c & 1) * CH * DC;
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int idx = tid + kVnThreads * j;
      const int i = idx % DC;
      if (idx < CH * DC) dst[idx] = (i < D && (a.allow_skip || i != a.zid)) ? pre[j] : ninf;
    }
  };
  // both row buffers -inf (the cells around every window stay -inf: see the step)
  for (int k = tid; k < 2 * NB * RS; k += kVnThreads) row[k] = ninf;
  load_chunk(0);
  put_chunk(0);
  load_chunk(1);
  put_chunk(1);
  lds_sync();  // (-inf before the first row's cell)
  if (tid == 0) rw(0)[0] = 0.0f;  // V[0][0] = [0.0f, -inf, ...]
  plo = 0;
  phi = 0;
  lds_sync();
  // the windows of 64 consecutive rows, one per lane, formed once per block (as F4)
  int wlo = 0, whi = 0;
  auto win_block = [&](int k0) { f4_window(u, k0 + lane, wlo, whi); };
  auto win_at = [&](int kk, int& l, int& h) {
    l = __builtin_amdgcn_readlane(wlo, kk & 63);
    h = __builtin_amdgcn_readlane(whi, kk & 63);
  };
  win_block(0);
  int lo, hi;  // window of the row the next step produces (formed before the barrier)
  win_at(1, lo, hi);
  auto step = [&](int k) {  // row k from row k - 1 with the class log-probs of input step k - 1
    if (hi - lo + 1 > Wc) {  // host sizing bug: report (uniform branch)
      if (tid == 0 && a.status) atomicOr(a.status, kStatusBadLength);
      return false;
    }
    const int ci = (k - 1) / CH, kk = (k - 1) - ci * CH;
    const float* w = cw + (ci & 1) * CH * DC + kk * DC;
    const float* srcw = rw((k - 1) & 1);
    float* dst = rw(k & 1);
    const bool pe = phi >= plo;  // previous window non-empty
    const int slo = pe ? plo : 0;
    const int span = pe ? phi - plo : -1;
    // PADDED: a cell whose every candidate lies outside the previous window is -inf; the others
    // have xr = x - slo within [0, span + dmax], so every candidate's cell lies within kF4Pad of
    // the window
    const int xlo = PADDED ? 0 : INT_MIN, xhi = PADDED ? span + dmax : INT_MAX;
    const unsigned lim = (unsigned)(span + 2);
    float wh[UNR ? DC : 1];
    if constexpr (UNR) {
#pragma unroll
      for (int i = 0; i < DC; ++i) wh[i] = w[i];
    }
    for (int x = lo + tid; x <= hi; x += kVnThreads) {
      const int xr = x - slo;
      const int xc = min(max(xr, xlo), xhi);
      // opaque: keeps the cell offset out of the uniform address sums (as F4's f4_cell)
      int xb = PADDED ? xc : xc + 1;
      asm volatile("" : "+v"(xb));
      const float* px = srcw + xb;
      float R[NB];
      int K[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        R[n] = ninf;
        K[n] = 0;
      }
      // the predecessor cell's list for a class of duration d (any d in [0, dmax] stays inside)
      auto cells = [&](int d, float (&v)[NB]) __attribute__((always_inline)) {
#pragma unroll
        for (int n = 0; n < NB; ++n) {
          if constexpr (PADDED) {
            v[n] = px[n * RS - d];
          } else {
            const unsigned yr1 = (unsigned)(xb - d);
            v[n] = srcw[n * RS + (int)min(yr1, lim) - 1];
          }
        }
      };
      if constexpr (UNR) {
#pragma unroll
        for (int i = 0; i < DC; ++i) {
          float c[NB];
          cells(dk[i], c);
#pragma unroll
          for (int n = 0; n < NB; ++n) c[n] = c[n] + wh[i];
          vn_merge<NB>(R, K, c, i * NB);
        }
      } else {
        // class i + 1's cells and class i + 2's offset and weight are on their way while class i
        // merges (slots beyond D: duration 0, weight -inf, loaded and never merged)
        float v0[NB];
        cells(dur[0], v0);
        float w0 = w[0], w1 = w[1];
        int d1 = dur[1];
#pragma unroll 1
        for (int i = 0; i < D; ++i) {
          float v1[NB];
          cells(d1, v1);
          const int i2 = min(i + 2, DC - 1);
          const int d2 = dur[i2];
          const float w2 = w[i2];
          float c[NB];
#pragma unroll
          for (int n = 0; n < NB; ++n) c[n] = v0[n] + w0;
          // no lane's best candidate beats its list's last entry: nothing changes (wave-uniform)
          if (!SSNT_V2NB_SKIP || __builtin_amdgcn_ballot_w64(c[0] > R[NB - 1]) != 0)
            vn_merge<NB>(R, K, c, i * NB);
#pragma unroll
          for (int n = 0; n < NB; ++n) v0[n] = v1[n];
          w0 = w1;
          w1 = w2;
          d1 = d2;
        }
      }
      const bool dead = PADDED && (xr != xc || !pe);
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        dst[n * RS + (x - lo)] = dead ? ninf : R[n];
        if constexpr (MODE != 0) {
          const size_t e = ((size_t)(k - 1) * NB + n) * Wc + (x - lo);
          if constexpr (EB == 1) bp[e] = (unsigned char)K[n];
          else reinterpret_cast<unsigned short*>(bp)[e] = (unsigned short)K[n];
        }
      }
    }
    // the cells right of the new window that the next step can reach: -inf in every plane (a row
    // two steps back may have left values there). Wave 7's lanes: idle unless the window exceeds
    // 448 cells.
    const int nz = PADDED ? dmax : 1;
    const int zi = tid - (kVnThreads - 64);
    if (zi >= 0 && zi < nz) {
#pragma unroll
      for (int n = 0; n < NB; ++n) dst[n * RS + max(hi - lo + 1, 0) + zi] = ninf;
    }
    plo = lo;
    phi = hi;
    if (k < I) {  // (before the barrier)
      if (((k + 1) & 63) == 0) win_block(k + 1);
      win_at(k + 1, lo, hi);
    }
    lds_sync();
    return true;
  };
  // chunk c = steps k in [c CH + 1, (c + 1) CH]; the class log-probs of chunk c + 1 are loaded
  // into registers as chunk c starts and put into LDS halfway through it (their buffer's last
  // reader, chunk c - 1, is done by then): one wait for global memory per chunk
  for (int c = 0; c * CH < I; ++c) {
    const bool next = c >= 1 && (c + 1) * CH < I;  // (chunks 0 and 1 are in place)
    if (next) load_chunk(c + 1);
    const int kmid = min(c * CH + CH / 2, I), kend = min((c + 1) * CH, I);
    bool ok = true;
    for (int k = c * CH + 1; ok && k <= kmid; ++k) ok = step(k);
    if (!ok) return false;
    if (next) put_chunk(c + 1);  // (the next step's barrier publishes it before its first reader)
    for (int k = kmid + 1; ok && k <= kend; ++k) ok = step(k);
    if (!ok) return false;
  }
  return true;
}

// DC: class padding; NB: list width; MODE: 0 no path output (no backpointers), 1 backpointers in
// LDS, 2 in the workspace
template <int DC, int NB, int MODE>
__global__ __launch_bounds__(kVnThreads) void k_v2_nbest(V2NbestArgs a, VnParams q) {
  constexpr int LOG = vn_log2(NB);
  constexpr int EB = vn_entry_bytes(DC, NB);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Imax = a.Imax, Wc = a.Wcap, N = a.N;
  const float ninf = -__builtin_inff();
  VnShared* sh = reinterpret_cast<VnShared*>(smem);
  int* dur = reinterpret_cast<int*>(smem + q.dur_off);
  unsigned char* path = smem + q.path_off;  // [rank][path_stride]
  float* lp_out = a.log_prob + (size_t)b * N;
  int* tot_out = a.total ? a.total + (size_t)b * N : nullptr;
  int* cls_out = (MODE && a.duration_class) ? a.duration_class + (size_t)b * N * Imax : nullptr;
  int* dur_out = (MODE && a.duration) ? a.duration + (size_t)b * N * Imax : nullptr;
  for (int i = tid; i < DC; i += kVnThreads) dur[i] = i < a.D ? a.table[i] : 0;
  lds_sync();

  auto fill_empty = [&]() {  // every rank absent: -inf, every class -1, every duration 0, total -1
    if (tid < N) {
      lp_out[tid] = ninf;
      if (tot_out) tot_out[tid] = -1;
    }
    if (cls_out)
      for (int t = tid; t < N * Imax; t += kVnThreads) cls_out[t] = -1;
    if (dur_out)
      for (int t = tid; t < N * Imax; t += kVnThreads) dur_out[t] = 0;
  };
  F4Utt u;
  if (!f4_setup(a, b, dur, u, true)) {
    fill_empty();
    return;
  }
  int plo, phi;
  const bool swept = u.dmax <= kF4Pad ? vn_sweep<DC, NB, true, MODE>(a, q, smem, u, plo, phi)
                                      : vn_sweep<DC, NB, false, MODE>(a, q, smem, u, plo, phi);
  if (!swept) {  // (uniform)
    fill_empty();
    return;
  }
  const int I = u.I;
  const int RS = Wc + 2 * kF4Pad + 2;

  // ---- final selection: the N best of (value, total, rank) over window(I)
  if (wave == 0) {
    const float* rI = reinterpret_cast<const float*>(smem + q.row_off) + (I & 1) * NB * RS + kF4Pad;
    float R[NB];
    int K[NB];  // x * NB + q
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      R[n] = ninf;
      K[n] = 0;
    }
    for (int x = plo + lane; x <= phi; x += 64) {  // a later cell's keys are above every kept one
      float c[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) c[n] = rI[n * RS + (x - plo)];
      vn_merge<NB>(R, K, c, x * NB);
    }
#pragma unroll 1
    for (int off = 32; off >= 1; off >>= 1) {  // both lanes of a pair end with the same list
      float oR[NB];
      int oK[NB];
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        oR[n] = __shfl_xor(R[n], off);
        oK[n] = __shfl_xor(K[n], off);
      }
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const int jj = NB - 1 - j;
        const bool mine = vn_before(R[j], K[j], oR[jj], oK[jj]);
        R[j] = mine ? R[j] : oR[jj];
        K[j] = mine ? K[j] : oK[jj];
      }
      vn_cleanup<NB>(R, K);
    }
    if (lane == 0) {
      int count = 0;  // present ranks come first: the list is sorted
#pragma unroll
      for (int n = 0; n < NB; ++n) {
        const bool present = n < N && count == n && R[n] > ninf;
        count += present;
        sh->value[n] = R[n];
        sh->x[n] = K[n] >> LOG;
        sh->q[n] = K[n] & (NB - 1);
      }
      sh->count = count;
    }
  }
  if constexpr (MODE == 2) __threadfence();  // the backpointer stores, before they are read back
  __syncthreads();  // (full: in workspace mode it also drains the sweep's global stores)
  const int count = sh->count;
  if (count == 0) {
    fill_empty();
    return;
  }
  if (tid < N) {
    const bool present = tid < count;
    lp_out[tid] = present ? sh->value[tid] : ninf;
    if (tot_out) tot_out[tid] = present ? sh->x[tid] : -1;
  }
  if constexpr (MODE == 0) return;

  // ---- backtrace: lane n of wave 0 walks rank n, every rank on the same row
  const bool walker = lane < count;
  int x = sh->x[lane & (NB - 1)];
  int qr = sh->q[lane & (NB - 1)];
  // rows rtop..rbot (descending); the entry of (row r, rank n, cell j) is EB bytes at
  // rows[(((r - 1) * NB + n) * Wc + j) * EB - off]
  auto walk = [&](int rtop, int rbot, const unsigned char* rows, int off) {
    for (int r0 = rtop; r0 >= rbot; r0 -= 64) {
      int wl, wh_;
      f4_window(u, max(r0 - lane, 0), wl, wh_);  // lane l: the window of row r0 - l
      const int n = min(64, r0 - rbot + 1);
      for (int j = 0; j < n; ++j) {
        const int r = r0 - j;
        const int lo = __builtin_amdgcn_readlane(wl, j);
        if (walker) {
          const int cell = min(max(x - lo, 0), Wc - 1);
          const int e = (((r - 1) * NB + qr) * Wc + cell) * EB - off;
          const int v = EB == 1 ? (int)rows[e] : (int)*reinterpret_cast<const unsigned short*>(rows + e);
          const int cls = min(v >> LOG, a.D - 1);
          qr = v & (NB - 1);
          path[lane * q.path_stride + (r - 1)] = (unsigned char)cls;
          x -= dur[cls];
        }
      }
    }
  };
  if constexpr (MODE == 1) {
    if (wave == 0) walk(I, 1, smem + q.bp_off, 0);
  } else {
    const unsigned char* bpg = reinterpret_cast<const unsigned char*>(a.workspace) + (size_t)b * q.ws_stride;
    unsigned* wbuf = reinterpret_cast<unsigned*>(smem + q.cw_off);  // over the sweep's buffers
    const int rb = Wc * NB * EB;                                    // bytes of one row's entries
    for (int rtop = I; rtop >= 1; rtop -= q.walk_rows) {
      const int rbot = max(1, rtop - q.walk_rows + 1);
      const int g0 = (rbot - 1) * rb, g1 = rtop * rb;  // the block's bytes [g0, g1)
      const int a0 = g0 & ~3;
      const int nd = (g1 - a0 + 3) >> 2;
      const unsigned* src = reinterpret_cast<const unsigned*>(bpg + a0);
      for (int j0 = tid; j0 < nd; j0 += 8 * kVnThreads) {  // 8 loads in flight per lane
        unsigned t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          t[i] = __hip_atomic_load(src + min(j0 + i * kVnThreads, nd - 1), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (j0 + i * kVnThreads < nd) wbuf[j0 + i * kVnThreads] = t[i];
      }
      __syncthreads();
      if (wave == 0) walk(rtop, rbot, reinterpret_cast<const unsigned char*>(wbuf), a0);
      __syncthreads();  // (the block's last reader, before the next block overwrites it)
    }
  }
  __syncthreads();

  // ---- outputs: absent ranks and steps t >= I get class -1 and duration 0
  for (int idx = tid; idx < N * Imax; idx += kVnThreads) {
    const int n = idx / Imax, t = idx - n * Imax;
    const int cls = (n < count && t < I) ? (int)path[n * q.path_stride + t] : -1;
    if (cls_out) cls_out[idx] = cls;
    if (dur_out) dur_out[idx] = cls >= 0 ? dur[cls] : 0;
  }
}

template <int DC, int NB, int MODE>
int launch_vn_k(const V2NbestArgs& a, const VnLayout& L, hipStream_t st) {
  VnParams q{};
  q.dur_off = L.dur_off; q.path_off = L.path_off; q.cw_off = L.cw_off; q.row_off = L.row_off;
  q.bp_off = L.bp_off; q.path_stride = L.path_stride; q.walk_rows = L.walk_rows;
  q.ws_stride = vn_ws_stride(a.Imax, a.Wcap, NB);
  return launch_lds(k_v2_nbest<DC, NB, MODE>, dim3(a.B), dim3(kVnThreads), L.total, kVnLdsBudget, st, a, q);
}

template <int DC, int NB>
int launch_vn_mode(const V2NbestArgs& a, int mode, hipStream_t st) {
  const VnLayout L = vn_layout(a.Imax, a.Wcap, DC, NB, mode);
  if (L.total > kVnLdsBudget) return SSNT_ERR_UNSUPPORTED;
  if (mode == 0) return launch_vn_k<DC, NB, 0>(a, L, st);
  if (mode == 1) return launch_vn_k<DC, NB, 1>(a, L, st);
  return launch_vn_k<DC, NB, 2>(a, L, st);
}

template <int DC>
int launch_vn_nb(const V2NbestArgs& a, int NB, int mode, hipStream_t st) {
  switch (NB) {
    case 1: return launch_vn_mode<DC, 1>(a, mode, st);
    case 2: return launch_vn_mode<DC, 2>(a, mode, st);
    case 4: return launch_vn_mode<DC, 4>(a, mode, st);
    default: return launch_vn_mode<DC, 8>(a, mode, st);
  }
}

}  // namespace

size_t v2_nbest_workspace_bytes(int B, int Imax, int max_total, bool test_mode, int N) {
  if (B <= 0 || Imax <= 0 || max_total < 0 || N < 1 || N > kVnMaxBest) return 0;
  const int Wc = (int)v2_fwd_bwd_wcap(max_total, test_mode);
  const int NB = vn_round(N);
  if (vn_bits_fit(Imax, Wc, NB)) return 0;
  return (size_t)B * vn_ws_stride(Imax, Wc, NB);
}

int launch_v2_nbest_align(const V2NbestArgs& in, hipStream_t st) {
  V2NbestArgs a = in;
  const int rc = v2_check_args(a, a.N >= 1 && a.N <= kVnMaxBest);
  if (rc != SSNT_OK || a.B == 0) return rc;
  const int NB = vn_round(a.N);
  // (backpointer entries; one utterance's outputs are no larger)
  if (!v2_offsets_ok(a, (size_t)a.Imax * vn_row_bytes_q(a.Wcap, NB))) return SSNT_ERR_UNSUPPORTED;
  const bool path = a.duration_class || a.duration;
  const bool fit = vn_bits_fit(a.Imax, a.Wcap, NB);
  const int mode = !path ? 0 : fit ? 1 : 2;
  const int DC = v2_class_cap(a.D);
  // rows that do not fit LDS at this list width: unsupported, whatever the workspace
  if (vn_layout(a.Imax, a.Wcap, DC, NB, mode).total > kVnLdsBudget) return SSNT_ERR_UNSUPPORTED;
  if (mode == 2 && !v2_workspace_ok(a, v2_nbest_workspace_bytes(a.B, a.Imax, a.X - 1, a.test_mode, a.N), 4))
    return SSNT_ERR_WORKSPACE;
  if (DC == 8) return launch_vn_nb<8>(a, NB, mode, st);
  if (DC == 16) return launch_vn_nb<16>(a, NB, mode, st);
  if (DC == 32) return launch_vn_nb<32>(a, NB, mode, st);
  return launch_vn_nb<64>(a, NB, mode, st);
}

}  // namespace ssnt
