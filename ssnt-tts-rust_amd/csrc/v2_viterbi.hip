// v2_viterbi.hip -- exact best duration path (Viterbi) on the v2 duration-class lattice, gfx950.
//
// Semantics: DESIGN.md 2.3. The max-plus counterpart of F4's forward sweep (v2_fwd_bwd.hip) over
// the same states (r input steps consumed, total x) and the same windows (v2_lattice_dev.h):
// f32 adds and one strict compare per class, classes in increasing order, nothing reassociated,
// so the outputs are bit-identical to the plain f32 restatement (tests/v2_viterbi_ref.py).
//
// Layout. One workgroup (512 threads) per utterance, the F4 sweep's:
//   LDS:  final selection | duration table | path bytes | class log-probs (f32, chunks of 64 or
//         32 steps, double-buffered, the class rule already applied: a masked class and every
//         unused class slot hold -inf) | 2 row buffers (ping-pong, window-relative), each with
//         kF4Pad cells of -inf on both sides of its window | backpointers (LDS mode)
// A step: each thread owns cells x = lo + tid (+512 ...) of the new row; its DC candidates are
// V[r-1][x - d_i] + w[i], the step's class log-probs read into registers once; a candidate that
// leaves the previous window reads a -inf cell and cannot win (-inf > -inf is false, a NaN
// compares false), which is the recurrence's "skip". With dmax <= kF4Pad a candidate's LDS
// address is one subtraction from its cell's; else F4's clamped-offset form onto the -inf cell
// beside the window. One LDS-only barrier per step; class log-probs are loaded a chunk ahead, so
// no global load sits on the I-step chain.
//
// Backpointers: the winning class, one byte per (row, window cell), I * Wcap bytes per utterance:
// in LDS when they fit beside the buffers, else in the caller's workspace (coalesced byte
// stores). With no path output nothing is kept.
//
// Final selection (max value, lowest total) over the last window and the backtrace run in the
// same launch. LDS mode: wave 0 walks the I rows (uniform across its lanes: the class byte goes
// to an SGPR, its duration is one v_readlane from the table held one entry per lane; the windows
// of 64 rows are formed at once, one per lane). Workspace mode: the rows are read back, highest
// first, into the LDS the sweep no longer needs, a block of rows per round trip, with loads that
// bypass the per-CU cache, after a full __syncthreads() has drained the sweep's stores. All
// threads then write the duration_class / duration rows.
#include <hip/hip_runtime.h>
#include <limits.h>

#include "buffer_ops.h"
#include "launch_util.h"
#include "ssnt_internal.h"
#include "v2_lattice_dev.h"

namespace ssnt {
namespace {

constexpr int kV2vThreads = 512;
constexpr size_t kV2vLdsBudget = 160 * 1024 - 256;  // one workgroup per CU may use ~all 160 KiB
constexpr size_t kV2vWalkTarget = 80 * 1024;        // workspace mode: LDS up to which the read-back block grows
constexpr unsigned kV2vHead = 16;                   // V2vShared

struct V2vShared {
  float best;
  int x, feasible, pad;
};

template <int DC>
constexpr int v2v_chunk() { return DC <= 32 ? 64 : 32; }  // sweep steps per staged chunk (= F4's)

// LDS carve of one launch; mode: 0 no backpointers, 1 backpointers in LDS, 2 in the workspace
struct V2vLayout {
  unsigned dur_off, path_off, cw_off, row_off, bp_off;
  int walk_rows;  // mode 2: rows per read-back block
  size_t total;
};
inline V2vLayout v2v_layout(int Imax, int Wc, int DC, int mode) {
  V2vLayout L{};
  const size_t a16 = 15;
  L.dur_off = kV2vHead;
  L.path_off = L.dur_off + (unsigned)DC * 4;
  L.cw_off = L.path_off + (mode ? (unsigned)(((size_t)Imax + a16) & ~a16) : 0u);
  const int ch = DC <= 32 ? 64 : 32;
  L.row_off = L.cw_off + 2u * ch * DC * 4;
  const size_t rowb = (2 * ((size_t)Wc + 2 * kF4Pad + 2) * 4 + a16) & ~a16;
  const size_t sweep_end = L.row_off + rowb;
  L.bp_off = (unsigned)sweep_end;
  L.total = sweep_end;
  if (mode == 1) L.total = sweep_end + (((size_t)Imax * Wc + a16) & ~a16);
  if (mode == 2) {
    // the block lies over the class log-probs and the row buffers (free after the selection)
    size_t avail = sweep_end - L.cw_off;
    if (kV2vWalkTarget > L.cw_off && kV2vWalkTarget - L.cw_off > avail) avail = kV2vWalkTarget - L.cw_off;
    size_t rows = (avail - 8) / (size_t)Wc;  // (8: the block starts on a dword of the workspace)
    rows = rows < 1 ? 1 : rows > (size_t)Imax ? (size_t)Imax : rows;
    L.walk_rows = (int)rows;
    const size_t blk = (rows * Wc + 8 + a16) & ~a16;
    L.total = L.cw_off + (blk > sweep_end - L.cw_off ? blk : sweep_end - L.cw_off);
  }
  return L;
}
// The backpointers of one utterance stay in LDS when they fit beside the buffers of the widest
// class padding (from the shape alone: the size query does not know D).
inline bool v2v_bits_fit(int Imax, int Wc) { return v2v_layout(Imax, Wc, 64, 1).total <= kV2vLdsBudget; }
inline size_t v2v_ws_stride(int Imax, int Wc) { return ((size_t)Imax * Wc + 4 + 15) & ~(size_t)15; }

struct V2vParams {
  unsigned dur_off, path_off, cw_off, row_off, bp_off;
  int walk_rows;
  unsigned long long ws_stride;
};

// one cell: best = max over classes i (increasing) of src[x - d_i] + w[i], arg = the lowest class
// that attains it (-1: none above -inf). srcw is the source row's window cell 0; xr the cell's
// offset from it. Every cell a candidate can reach outside the window holds -inf.
//  PADDED (dmax <= kF4Pad): kF4Pad cells of -inf on both sides of the window; the caller clamps xr
//   into the band from which every candidate stays inside them.
//  else: offsets are taken +1, so anything left of the window wraps to a huge unsigned value and
//   one unsigned min clamps an out-of-window candidate onto the -inf cell just right of the
//   window (index span + 1); offset 0 is the -inf cell left of it (index -1).
template <int DC, bool PADDED>
__device__ __forceinline__ void v2v_cell(int xr, const int (&dk)[DC], const float (&w)[DC], const float* srcw,
                                         int span, float& best, int& arg) {
  // opaque: keeps the cell offset out of 2 DC uniform address sums (as F4's f4_cell)
  int xb = PADDED ? xr : xr + 1;
  asm volatile("" : "+v"(xb));
  const float* px = srcw + xb;
  const unsigned lim = (unsigned)(span + 2);
  float v[DC];
#pragma unroll
  for (int i = 0; i < DC; ++i) {
    if constexpr (PADDED) {
      v[i] = px[-dk[i]];
    } else {
      const unsigned yr1 = (unsigned)(xb - dk[i]);
      v[i] = srcw[(int)min(yr1, lim) - 1];
    }
  }
  // The compare in class order. Two equally exact forms were measured at configs[4] and not kept:
  // four independent chains merged low to high (299 us against 294 us) and a full pairwise
  // (value, lowest class) tree (809 us: its DC live compare masks spill the SGPR file).
  best = -__builtin_inff();
  arg = -1;
#pragma unroll
  for (int i = 0; i < DC; ++i) {
    const float c = v[i] + w[i];
    if (c > best) {  // strict: a tie keeps the lower class; a NaN never wins
      best = c;
      arg = i;
    }
  }
}

// The sweep: rows 1..I from row 0 = {total 0: 0.0f}. On return the last row is in row buffer
// I & 1, its window [plo, phi]. false: a window beyond the row capacity (reported).
template <int DC, bool PADDED, int MODE>
__device__ __forceinline__ bool v2v_sweep(const V2ViterbiArgs& a, const V2vParams& q, unsigned char* smem,
                                          const F4Utt& u, int& plo, int& phi) {
  constexpr int CH = v2v_chunk<DC>();
  constexpr int NPF = (CH * DC + kV2vThreads - 1) / kV2vThreads;  // staged values per thread
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int D = a.D, Imax = a.Imax, Wc = a.Wcap, dmax = u.dmax, I = u.I;
  const float ninf = -__builtin_inff();
  const int* dur = reinterpret_cast<const int*>(smem + q.dur_off);
  float* cw = reinterpret_cast<float*>(smem + q.cw_off);  // [2][CH][DC]
  float* row = reinterpret_cast<float*>(smem + q.row_off);
  const int RS = Wc + 2 * kF4Pad + 2;
  auto rw = [&](int k) { return row + k * RS + kF4Pad; };  // buffer k's window cell 0
  unsigned char* bpl = smem + q.bp_off;                    // MODE 1: [I][Wc]
  unsigned char* bpg = MODE == 2 ? reinterpret_cast<unsigned char*>(a.workspace) + (size_t)b * q.ws_stride
                                 : nullptr;
  const float* lg = a.logits + (size_t)b * Imax * D;
  int dk[DC];  // candidate offsets (VGPRs)
#pragma unroll
  for (int i = 0; i < DC; ++i) dk[i] = dur[i];
  float pre[NPF];
  // class log-probs through one descriptor: masked entries read past its end, so the loads need
  // no exec mask (their value is never used: put_chunk writes -inf for them)
  const __amdgpu_buffer_rsrc_t lg_r = brsrc(lg, (unsigned)((size_t)Imax * D * sizeof(float)));
  auto load_chunk = [&](int c) {  // chunk c = sweep steps [c CH, (c + 1) CH)
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int idx = tid + kV2vThreads * j;
      const int k = c * CH + idx / DC, i = idx % DC;
      const bool live = idx < CH * DC && i < D && k < I;
      pre[j] = rbuf_ld1(lg_r, live ? (k * D + i) * (int)sizeof(float) : (int)0x80000000, 0, 0);
    }
  };
  auto put_chunk = [&](int c) {  // ... into the chunk's LDS buffer, the class rule applied
    float* dst = cw + (c & 1) * CH * DC;
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
      const int idx = tid + kV2vThreads * j;
      const int i = idx % DC;
      if (idx < CH * DC) dst[idx] = (i < D && (a.allow_skip || i != a.zid)) ? pre[j] : ninf;
    }
  };
  // both row buffers -inf (the cells around every window stay -inf: see the step)
  for (int k = tid; k < 2 * RS; k += kV2vThreads) row[k] = ninf;
  load_chunk(0);
  put_chunk(0);
  load_chunk(1);
  put_chunk(1);
  lds_sync();  // (-inf before the first row's cell)
  if (tid == 0) rw(0)[0] = 0.0f;  // V[0][0]
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
    float wh[DC];
#pragma unroll
    for (int i = 0; i < DC; ++i) wh[i] = w[i];
    for (int x = lo + tid; x <= hi; x += kV2vThreads) {
      const int xr = x - slo;
      const int xc = min(max(xr, xlo), xhi);
      float best;
      int arg;
      v2v_cell<DC, PADDED>(xc, dk, wh, srcw, span, best, arg);
      if (PADDED && (xr != xc || !pe)) {
        best = ninf;
        arg = -1;
      }
      dst[x - lo] = best;
      if constexpr (MODE == 1) bpl[(k - 1) * Wc + (x - lo)] = (unsigned char)arg;
      if constexpr (MODE == 2) bpg[(size_t)(k - 1) * Wc + (x - lo)] = (unsigned char)arg;
    }
    // the cells right of the new window that the next step can reach: -inf (a row two steps back
    // may have left values there). Wave 7's lanes: idle unless the window exceeds 448 cells.
    const int nz = PADDED ? dmax : 1;
    const int zi = tid - (kV2vThreads - 64);
    if (zi >= 0 && zi < nz) dst[max(hi - lo + 1, 0) + zi] = ninf;
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

// MODE: 0 no path output (no backpointers), 1 backpointer bytes in LDS, 2 in the workspace
template <int DC, int MODE>
__global__ __launch_bounds__(kV2vThreads) void k_v2_viterbi(V2ViterbiArgs a, V2vParams q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Imax = a.Imax, Wc = a.Wcap;
  const float ninf = -__builtin_inff();
  V2vShared* sh = reinterpret_cast<V2vShared*>(smem);
  int* dur = reinterpret_cast<int*>(smem + q.dur_off);
  unsigned char* path = smem + q.path_off;
  int* cls_out = (MODE && a.duration_class) ? a.duration_class + (size_t)b * Imax : nullptr;
  int* dur_out = (MODE && a.duration) ? a.duration + (size_t)b * Imax : nullptr;
  for (int i = tid; i < DC; i += kV2vThreads) dur[i] = i < a.D ? a.table[i] : 0;
  lds_sync();

  auto fill_empty = [&]() {  // the infeasible rule: -inf, every class -1, every duration 0, total -1
    if (tid == 0) {
      a.log_prob[b] = ninf;
      if (a.total) a.total[b] = -1;
    }
    if (cls_out)
      for (int t = tid; t < Imax; t += kV2vThreads) cls_out[t] = -1;
    if (dur_out)
      for (int t = tid; t < Imax; t += kV2vThreads) dur_out[t] = 0;
  };
  F4Utt u;
  if (!f4_setup(a, b, dur, u, true)) {
    fill_empty();
    return;
  }
  int plo, phi;
  const bool swept = u.dmax <= kF4Pad ? v2v_sweep<DC, true, MODE>(a, q, smem, u, plo, phi)
                                      : v2v_sweep<DC, false, MODE>(a, q, smem, u, plo, phi);
  if (!swept) {  // (uniform)
    fill_empty();
    return;
  }
  const int I = u.I;

  // ---- final selection: (largest value, lowest total) over window(I)
  if (wave == 0) {
    const float* rI = reinterpret_cast<const float*>(smem + q.row_off) +
                      (I & 1) * (Wc + 2 * kF4Pad + 2) + kF4Pad;
    float bv = ninf;
    int bx = -1;
    for (int x = plo + lane; x <= phi; x += 64) {
      const float v = rI[x - plo];
      if (v > bv) {
        bv = v;
        bx = x;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {  // a lane has bx >= 0 exactly when its bv > -inf
      const float ov = __shfl_xor(bv, off);
      const int ox = __shfl_xor(bx, off);
      if (ov > bv || (ov == bv && ox < bx)) {
        bv = ov;
        bx = ox;
      }
    }
    if (lane == 0) {
      sh->best = bv;
      sh->x = bx;
      sh->feasible = bv > ninf;
    }
  }
  if constexpr (MODE == 2) __threadfence();  // the backpointer stores, before they are read back
  __syncthreads();  // (full: in workspace mode it also drains the sweep's global stores)
  const float best = sh->best;
  const int xbest = sh->x;
  if (!sh->feasible) {
    fill_empty();
    return;
  }
  if (tid == 0) {
    a.log_prob[b] = best;
    if (a.total) a.total[b] = xbest;
  }
  if constexpr (MODE == 0) return;

  // ---- backtrace (wave 0; every lane runs the same walk)
  const int mydur = lane < a.D ? dur[lane] : 0;
  int x = xbest;
  // rows rtop..rbot (descending); the byte of (row r, cell j) is at rows[(r - 1) * Wc + j - off]
  auto walk = [&](int rtop, int rbot, const unsigned char* rows, int off) {
    for (int r0 = rtop; r0 >= rbot; r0 -= 64) {
      int wl, wh_;
      f4_window(u, max(r0 - lane, 0), wl, wh_);  // lane l: the window of row r0 - l
      const int n = min(64, r0 - rbot + 1);
      for (int j = 0; j < n; ++j) {
        const int r = r0 - j;
        const int lo = __builtin_amdgcn_readlane(wl, j);
        const int cell = min(max(x - lo, 0), Wc - 1);
        const int cls = __builtin_amdgcn_readfirstlane((int)rows[(r - 1) * Wc + cell - off]) & 63;
        if (lane == 0) path[r - 1] = (unsigned char)cls;
        x -= __builtin_amdgcn_readlane(mydur, cls);
      }
    }
  };
  if constexpr (MODE == 1) {
    if (wave == 0) walk(I, 1, smem + q.bp_off, 0);
  } else {
    const unsigned char* bpg = reinterpret_cast<const unsigned char*>(a.workspace) + (size_t)b * q.ws_stride;
    unsigned* wbuf = reinterpret_cast<unsigned*>(smem + q.cw_off);  // over the sweep's buffers
    for (int rtop = I; rtop >= 1; rtop -= q.walk_rows) {
      const int rbot = max(1, rtop - q.walk_rows + 1);
      const int g0 = (rbot - 1) * Wc, g1 = rtop * Wc;  // the block's bytes [g0, g1)
      const int a0 = g0 & ~3;
      const int nd = (g1 - a0 + 3) >> 2;
      const unsigned* src = reinterpret_cast<const unsigned*>(bpg + a0);
      for (int j0 = tid; j0 < nd; j0 += 8 * kV2vThreads) {  // 8 loads in flight per lane
        unsigned t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
          t[i] = __hip_atomic_load(src + min(j0 + i * kV2vThreads, nd - 1), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (j0 + i * kV2vThreads < nd) wbuf[j0 + i * kV2vThreads] = t[i];
      }
      __syncthreads();
      if (wave == 0) walk(rtop, rbot, reinterpret_cast<const unsigned char*>(wbuf), a0);
      __syncthreads();  // (the block's last reader, before the next block overwrites it)
    }
  }
  __syncthreads();

  // ---- outputs: steps t >= I get class -1 and duration 0
  for (int t = tid; t < Imax; t += kV2vThreads) {
    const int cls = t < I ? (int)path[t] : -1;
    if (cls_out) cls_out[t] = cls;
    if (dur_out) dur_out[t] = t < I ? dur[cls] : 0;
  }
}

template <int DC, int MODE>
int launch_v2v_k(const V2ViterbiArgs& a, const V2vLayout& L, hipStream_t st) {
  V2vParams q{};
  q.dur_off = L.dur_off; q.path_off = L.path_off; q.cw_off = L.cw_off; q.row_off = L.row_off;
  q.bp_off = L.bp_off; q.walk_rows = L.walk_rows;
  q.ws_stride = v2v_ws_stride(a.Imax, a.Wcap);
  return launch_lds(k_v2_viterbi<DC, MODE>, dim3(a.B), dim3(kV2vThreads), L.total, kV2vLdsBudget, st, a, q);
}

template <int DC>
int launch_v2v_mode(const V2ViterbiArgs& a, int mode, hipStream_t st) {
  const V2vLayout L = v2v_layout(a.Imax, a.Wcap, DC, mode);
  if (L.total > kV2vLdsBudget) return SSNT_ERR_UNSUPPORTED;
  if (mode == 0) return launch_v2v_k<DC, 0>(a, L, st);
  if (mode == 1) return launch_v2v_k<DC, 1>(a, L, st);
  return launch_v2v_k<DC, 2>(a, L, st);
}

}  // namespace

size_t v2_viterbi_workspace_bytes(int B, int Imax, int max_total, bool test_mode) {
  if (B <= 0 || Imax <= 0 || max_total < 0) return 0;
  const int Wc = (int)v2_fwd_bwd_wcap(max_total, test_mode);
  if (v2v_bits_fit(Imax, Wc)) return 0;
  return (size_t)B * v2v_ws_stride(Imax, Wc);
}

int launch_v2_viterbi(const V2ViterbiArgs& in, hipStream_t st) {
  V2ViterbiArgs a = in;
  const int rc = v2_check_args(a);
  if (rc != SSNT_OK || a.B == 0) return rc;
  if (!v2_offsets_ok(a, (size_t)a.Imax * a.Wcap)) return SSNT_ERR_UNSUPPORTED;  // (backpointer bytes)
  const bool path = a.duration_class || a.duration;
  const bool fit = v2v_bits_fit(a.Imax, a.Wcap);
  const int mode = !path ? 0 : fit ? 1 : 2;
  const int DC = v2_class_cap(a.D);
  // a row that does not fit LDS: unsupported, whatever the workspace
  if (v2v_layout(a.Imax, a.Wcap, DC, mode).total > kV2vLdsBudget) return SSNT_ERR_UNSUPPORTED;
  if (mode == 2 && !v2_workspace_ok(a, v2_viterbi_workspace_bytes(a.B, a.Imax, a.X - 1, a.test_mode), 4))
    return SSNT_ERR_WORKSPACE;
  if (DC == 8) return launch_v2v_mode<8>(a, mode, st);
  if (DC == 16) return launch_v2v_mode<16>(a, mode, st);
  if (DC == 32) return launch_v2v_mode<32>(a, mode, st);
  return launch_v2v_mode<64>(a, mode, st);
}

}  // namespace ssnt
