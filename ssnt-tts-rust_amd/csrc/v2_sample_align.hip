// v2_sample_align.hip -- duration paths drawn from the posterior of the v2 duration-class lattice,
// gfx950.
//
// Semantics: DESIGN.md 2.5. Forward filter, backward sample on F4's lattice (v2_lattice_dev.h), in
// two launches on the caller's stream:
//   1  F4's forward sweep (v2_fwd_bwd.hip, launch_v2_fwd_only): alpha rows 0..I of every utterance,
//      window-relative, and Z into the workspace. The arithmetic is stated there, once.
//   2  k_v2_sample_walk (this file): one wave per (utterance, sample), one lane per class slot.
//
// The walk. A workgroup holds up to 8 samples of one utterance. It first forms the final-total
// CDF, common to its samples: the cells of row I aligned to their largest exponent (all threads),
// then their sequential f32 prefix sum (wave 0: one dependent add per cell) in LDS; each wave
// then takes its total with one ballot per 64 cells. Standing on (r, x), lane i holds the term of
// class i: alpha[r-1][x - d_i] (x) exp(logits[r-1][i]); the wave max of the exponents (DPP within
// rows of 16, four v_readlane across them), the class-ordered prefix sum (DC - 1 dependent adds,
// each taking the lower lane's running sum through a one-lane wavefront shift: the definition is
// sequential, a log-step lane scan would associate differently), one ballot for the class, one
// v_readlane for its duration. The class bytes go to LDS; the output rows and the forward-order
// log_prob sum are written afterwards, 64 gathered terms at a time.
//
// What a step waits for is alpha[r-1][x - d_i]: a global gather whose address depends on the
// previous decision. Two forms:
//   gather  lane i loads its own cell; one memory round trip per step. Any dmax.
//   cone<J> (J * dmax <= 63) the cells of rows r-1..r-J a walk can reach from x all lie in
//           [x - J dmax, x]: lane l loads cell x - l of each of the J rows at once (J independent
//           loads, one round trip), and step q takes its term from lane (x0 - x) + d_i of row
//           r-q's span with one ds_bpermute pair.
// Class log-probs and uniforms do not depend on x: they are loaded a group of steps ahead and
// converted (xf_exp, the clamp) while the row loads are in flight. An out-of-window cell is a
// range-checked load past the descriptor's end plus a select of the canonical zero: no branch.
#include <hip/hip_runtime.h>

#include "buffer_ops.h"
#include "launch_util.h"
#include "ssnt_internal.h"
#include "v2_lattice_dev.h"
#include "xf_math.h"

namespace ssnt {
namespace {

constexpr int kV2sMaxSamples = 64;
constexpr int kV2sMaxWaves = 8;                     // samples (waves) of a workgroup, at most
constexpr size_t kV2sLdsBudget = 160 * 1024 - 256;  // one workgroup per CU may use ~all 160 KiB
constexpr unsigned kV2sHead = 16 + 64 * 4;          // V2sShared | duration table (64 slots)
constexpr float kV2sUMax = 0x1.fffffep-1f;          // 1 - 2^-24
constexpr int kV2sNoCell = (int)0x80000000;         // a byte offset past every descriptor: reads 0

struct V2sShared {
  int emax;     // largest exponent over window(I)
  float clast;  // the last prefix sum of the final-total CDF
  int pad[2];
};

struct V2sParams {
  unsigned path_off, cdf_off;  // class bytes [waves][ipad] | CDF cells [Wcap] (a', c)
  int ipad;
  int cone;  // steps per round trip, at most (1, 2, 4)
};

__device__ __forceinline__ float clamp_uniform(float x) {  // NaN -> 0, then [0, 1 - 2^-24]
  x = x >= 0.0f ? x : 0.0f;
  return fminf(x, kV2sUMax);
}

template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
// max over the 64 lanes (whole wave active); exact, so the order does not matter
__device__ __forceinline__ int wave_max(int v) {
  v = max(v, dpp_i<0xB1>(v));   // quad_perm [1,0,3,2]
  v = max(v, dpp_i<0x4E>(v));   // quad_perm [2,3,0,1]
  v = max(v, dpp_i<0x141>(v));  // row_half_mirror
  v = max(v, dpp_i<0x140>(v));  // row_mirror: every row of 16 uniform
  return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ float readlane_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// The sequential prefix sum over the lanes, p_l = (..((v_0 + v_1) + v_2).. + v_l), for lanes
// 0..N-1: N-1 dependent adds whose first operand is the lower lane's running sum (a wavefront
// shift by one lane inside the add; lane 0 shifts in 0). After step k lanes 0..k hold their final
// sums, each formed in exactly the sequential order (f32 add is commutative) -- the bits N
// v_readlane + add pairs would give, without their N lane masks. Not a log-step scan: that would
// associate differently. Whole wave active.
template <int N>
__device__ __forceinline__ float seq_prefix(float v) {
  float p = v;
#pragma unroll
  for (int i = 1; i < N; ++i)
    p = v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, p), 0x138, 0xf, 0xf, false));
  return p;
}
__device__ __forceinline__ int lowest(unsigned long long m) { return __builtin_ctzll(m); }
__device__ __forceinline__ int highest(unsigned long long m) { return 63 - __builtin_clzll(m); }

// The class of one step from lane i's source cell v, class weight w and the
// step's clamped uniform: the lowest class with m' > 0 and u * c_last < c_i, else the highest with
// m' > 0. Lanes >= D hold w = 0, so their terms are exact zeros.
template <int DC>
__device__ __forceinline__ int v2s_choose(xf v, xf w, float uu, int lane) {
  const float m = v.m * w.m;  // f4_cell<FWD>'s operand order
  const int e = v.e + w.e;
  const int em = wave_max(e);
  const float mp = xldexp(m, e - em);
  const float mine = seq_prefix<DC>(mp);  // c_i (lanes >= DC: unused, m' = 0 there)
  const float thr = uu * readlane_f(mine, DC - 1);
  const unsigned long long pos = __ballot(mp > 0.0f);
  const unsigned long long hit = __ballot(mp > 0.0f && thr < mine);
  return hit ? lowest(hit) : pos ? highest(pos) : 0;
}

// The walk of one sample from (I, x) down to row 0; the class of step t goes to path[t].
// J steps form a group: their class log-probs and uniforms are loaded one group ahead; CONE: their
// source rows' spans are loaded together when the group starts (J * dmax <= 63), else each step
// gathers its own cells.
template <int DC, int J, bool CONE>
__device__ __forceinline__ void v2s_walk(const V2SampleArgs& a, const F4Utt& u, const xf* rows, const float* lg,
                                         const float* un, int mydur, int x, unsigned char* path, int lane) {
  const int D = a.D, Wc = a.Wcap, I = u.I;
  const __amdgpu_buffer_rsrc_t ws_r = brsrc(rows, (unsigned)((size_t)(a.Imax + 1) * Wc * sizeof(xf)));
  const __amdgpu_buffer_rsrc_t lg_r = brsrc(lg, (unsigned)((size_t)a.Imax * D * sizeof(float)));
  const __amdgpu_buffer_rsrc_t un_r = brsrc(un, (unsigned)((size_t)(a.Imax + 1) * sizeof(float)));
  const bool cls_lane = lane < D;
  const bool valid = cls_lane && (a.allow_skip || lane != a.zid);
  float wn[J], unext;
  auto prefetch = [&](int r) {  // the steps of the group standing on row r: t = r-1 .. r-J
#pragma unroll
    for (int q = 0; q < J; ++q) {
      const int t = r - 1 - q;
      wn[q] = rbuf_ld1(lg_r, (cls_lane && t >= 0) ? (t * D + lane) * (int)sizeof(float) : kV2sNoCell, 0, 0);
    }
    const int t = r - 1 - lane;  // lane q: the uniform of step r-1-q
    unext = rbuf_ld1(un_r, (lane < J && t >= 0) ? t * (int)sizeof(float) : kV2sNoCell, 0, 0);
  };
  // cell y of row rr, the canonical zero outside [lo, hi] (no branch: a load past the end)
  auto cell = [&](int rr, int y, int lo, int hi, bool want) {
    const bool inw = want && rr >= 0 && y >= lo && y <= hi;
    const f32x2 t = rbuf_ld2(ws_r, inw ? (rr * Wc + (y - lo)) * (int)sizeof(xf) : kV2sNoCell, 0, 0);
    // (the element into a float first: a bit cast applied to the vector element itself reads
    // element 0 in this toolchain)
    const float tm = t.x, te = t.y;
    return inw ? xf{tm, __builtin_bit_cast(int, te)} : xf_zero();
  };
  prefetch(I);
  for (int r0 = I; r0 >= 1; r0 -= 64) {
    // the windows of rows r0-1 .. r0-64, one per lane (a group never straddles two blocks: J | 64)
    int wl, wh;
    f4_window(u, max(r0 - 1 - lane, 0), wl, wh);
    const int rend = max(r0 - 63, 1);
    for (int r = r0; r >= rend; r -= J) {
      const int wi = r0 - r;  // lane holding window(r - 1)
      float wc[J];
#pragma unroll
      for (int q = 0; q < J; ++q) wc[q] = wn[q];
      const float uc = unext;
      xf sp[J];
      if constexpr (CONE) {
#pragma unroll
        for (int q = 0; q < J; ++q)
          sp[q] = cell(r - 1 - q, x - lane, __builtin_amdgcn_readlane(wl, wi + q),
                       __builtin_amdgcn_readlane(wh, wi + q), true);
      }
      prefetch(r - J);
      xf w[J];
#pragma unroll
      for (int q = 0; q < J; ++q) w[q] = cls_lane ? xf_exp(wc[q], valid) : xf_zero();
      const float uq = clamp_uniform(uc);
      const int x0 = x;
#pragma unroll
      for (int q = 0; q < J; ++q) {
        if (q < r) {  // (uniform) the step standing on row r - q, from row r - 1 - q
          xf v;
          if constexpr (CONE) {
            const int src = (x0 - x) + mydur;  // <= J * dmax <= 63
            v.m = __shfl(sp[q].m, src);
            v.e = __shfl(sp[q].e, src);
          } else {
            v = cell(r - 1 - q, x - mydur, __builtin_amdgcn_readlane(wl, wi + q),
                     __builtin_amdgcn_readlane(wh, wi + q), cls_lane);
          }
          const int cls = v2s_choose<DC>(v, w[q], readlane_f(uq, q), lane);
          if (lane == 0) path[r - 1 - q] = (unsigned char)cls;
          x -= __builtin_amdgcn_readlane(mydur, cls);
        }
      }
    }
  }
}

template <int DC>
__global__ __launch_bounds__(kV2sMaxWaves * 64) void k_v2_sample_walk(V2SampleArgs a, V2sParams q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, nt = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = blockIdx.y * (nt >> 6) + wave;  // this wave's sample
  const int Imax = a.Imax, Wc = a.Wcap, NS = a.NS;
  const bool mine = k < NS;
  const float ninf = -__builtin_inff();
  V2sShared* sh = reinterpret_cast<V2sShared*>(smem);
  int* dur = reinterpret_cast<int*>(smem + 16);
  unsigned char* path = smem + q.path_off + (size_t)wave * q.ipad;
  xf* cdf = reinterpret_cast<xf*>(smem + q.cdf_off);
  const size_t row = (size_t)b * NS + (mine ? k : 0);
  float* lp_out = a.log_prob + row;
  int* cls_out = a.duration_class ? a.duration_class + row * Imax : nullptr;
  int* dur_out = a.duration ? a.duration + row * Imax : nullptr;
  for (int i = tid; i < 64; i += nt) dur[i] = i < a.D ? a.table[i] : 0;
  if (tid == 0) sh->emax = XF_EZERO;
  lds_sync();

  auto fill_empty = [&]() {  // the infeasible rule, this wave's sample
    if (!mine) return;
    if (lane == 0) {
      *lp_out = ninf;
      if (a.total) a.total[row] = -1;
    }
    if (cls_out)
      for (int t = lane; t < Imax; t += 64) cls_out[t] = -1;
    if (dur_out)
      for (int t = lane; t < Imax; t += 64) dur_out[t] = 0;
  };
  F4Utt u;
  if (!f4_setup(a, b, dur, u, false)) {  // (the forward launch reported it)
    fill_empty();
    return;
  }
  const int I = u.I;
  const xf* rows = reinterpret_cast<const xf*>(a.workspace) + (size_t)b * (Imax + 1) * Wc;

  // ---- the final-total CDF over window(I), common to the samples of the utterance
  int plo, phi;
  f4_window(u, I, plo, phi);
  const int n = phi - plo + 1;
  if (n < 1 || n > Wc) {  // (uniform) an empty last window; beyond the row capacity: reported by the sweep
    fill_empty();
    return;
  }
  const xf* rI = rows + (size_t)I * Wc;
  int em = XF_EZERO;
#pragma unroll 4
  for (int j = tid; j < n; j += nt) {
    const xf v = rI[j];
    cdf[j] = v;
    em = max(em, v.e);
  }
  em = wave_max(em);
  if (lane == 0) atomicMax(&sh->emax, em);
  lds_sync();
  const int es = sh->emax;
  for (int j = tid; j < n; j += nt) cdf[j].m = xldexp(cdf[j].m, cdf[j].e - es);  // a' (its own cells)
  lds_sync();
  if (wave == 0) {  // c_x: the sequential prefix sum, into the cells' second word
    float c = 0.0f;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      float av = j < n ? cdf[j].m : 0.0f;
      if (lane == 0) av = c + av;  // the running sum enters ahead of the block's first cell
      const float cm = seq_prefix<64>(av);
      if (j < n) cdf[j].e = __builtin_bit_cast(int, cm);
      c = readlane_f(cm, 63);
    }
    if (lane == 0) sh->clast = c;
  }
  lds_sync();
  const float clast = sh->clast;
  if (!(clast > 0.0f)) {  // (uniform) Z == 0
    fill_empty();
    return;
  }
  if (!mine) return;  // (no barrier below)

  // ---- this sample's total
  const float* un = a.uniform + row * (Imax + 1);
  const float* lg = a.logits + (size_t)b * Imax * a.D;
  const float thr = clamp_uniform(un[Imax]) * clast;
  int xsel = -1, xhigh = 0;
  for (int j0 = 0; j0 < n && xsel < 0; j0 += 64) {
    const int j = j0 + lane;
    const float ap = j < n ? cdf[j].m : 0.0f;
    const float cj = j < n ? __builtin_bit_cast(float, cdf[j].e) : 0.0f;
    const unsigned long long pos = __ballot(ap > 0.0f);
    const unsigned long long hit = __ballot(ap > 0.0f && thr < cj);
    if (hit) xsel = j0 + lowest(hit);
    if (pos) xhigh = j0 + highest(pos);
  }
  const int xtot = plo + (xsel >= 0 ? xsel : xhigh);

  // ---- the walk (every branch below is wave-uniform)
  const int mydur = dur[lane];
  const int span = u.dmax;
  if (q.cone >= 4 && 4 * span <= 63) v2s_walk<DC, 4, true>(a, u, rows, lg, un, mydur, xtot, path, lane);
  else if (q.cone >= 2 && 2 * span <= 63) v2s_walk<DC, 2, true>(a, u, rows, lg, un, mydur, xtot, path, lane);
  else v2s_walk<DC, 4, false>(a, u, rows, lg, un, mydur, xtot, path, lane);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // lane 0's class bytes, before the wave reads them
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  // ---- outputs: the rows (steps t >= I: class -1, duration 0) and log_prob, the sequential f32
  // sum of the path's class log-probs in step order, 64 gathered terms at a time
  float v = 0.0f;
  for (int t0 = 0; t0 < Imax; t0 += 64) {
    const int t = t0 + lane;
    const int cls = t < I ? (int)path[t] : -1;
    if (t < Imax) {
      if (cls_out) cls_out[t] = cls;
      if (dur_out) dur_out[t] = t < I ? dur[cls] : 0;
    }
    const float term = t < I ? lg[(size_t)t * a.D + cls] : 0.0f;
    const int nterm = min(64, I - t0);
    for (int i = 0; i < nterm; ++i) v = v + readlane_f(term, i);
  }
  if (lane == 0) {
    *lp_out = v;
    if (a.total) a.total[row] = xtot;
  }
}

#ifdef SSNT_AB
int g_cone = 0, g_launches = 3;  // A/B build: set_v2_sample_form
#endif
inline int v2s_cone() {
#ifdef SSNT_AB
  return g_cone == 0 ? 4 : g_cone;
#else
  return 4;  // (measured)
#endif
}
inline int v2s_launches() {
#ifdef SSNT_AB
  return g_launches;
#else
  return 3;
#endif
}

// waves of a workgroup: the samples, up to kV2sMaxWaves, fewer where their class bytes crowd LDS
struct V2sLayout {
  int waves, ipad;
  unsigned path_off, cdf_off;
  size_t total;
};
inline V2sLayout v2s_layout(int Imax, int Wc, int NS) {
  V2sLayout L{};
  L.ipad = (Imax + 15) & ~15;
  L.path_off = kV2sHead;
  for (int w = NS < kV2sMaxWaves ? NS : kV2sMaxWaves; w >= 1; --w) {
    L.waves = w;
    L.cdf_off = (unsigned)(L.path_off + (size_t)w * L.ipad);
    L.total = L.cdf_off + (size_t)Wc * sizeof(xf);
    if (L.total <= kV2sLdsBudget) break;
  }
  return L;
}

}  // namespace

size_t v2_sample_workspace_bytes(int B, int Imax, int max_total, bool test_mode) {
  return v2_fwd_only_workspace_bytes(B, Imax, max_total, test_mode);
}

#ifdef SSNT_AB
int set_v2_sample_form(int cone, int launches) {
  if ((cone != 0 && cone != 1 && cone != 2 && cone != 4) || launches < 1 || launches > 3) return SSNT_ERR_INVALID_ARG;
  g_cone = cone;
  g_launches = launches;
  return SSNT_OK;
}
#endif

int launch_v2_sample_align(const V2SampleArgs& in, hipStream_t st) {
  V2SampleArgs a = in;
  if (a.NS < 1 || a.NS > kV2sMaxSamples || a.B < 0) return SSNT_ERR_INVALID_ARG;
  if (a.B == 0) return SSNT_OK;
  if (!a.uniform || !a.log_prob) return SSNT_ERR_INVALID_ARG;
  // the forward launch's arguments; its refusals (F4's, in F4's order) before anything is launched
  V2FwdBwdArgs f = v2_fwd_bwd_args_of(a);
  if (a.workspace && !aligned_to(a.workspace, sizeof(xf))) {
    f.workspace = nullptr;  // (refused as a missing one, after F4's other checks)
  }
  int rc = launch_v2_fwd_only(f, false, st);
  if (rc != SSNT_OK) return rc;
  a.Wcap = (int)v2_fwd_bwd_wcap(a.X - 1, a.test_mode);
  // (the uniforms of one sample and the rows of one utterance are addressed with 32-bit offsets:
  // the latter is F4's limit, checked above)
  if ((size_t)(a.Imax + 1) * sizeof(float) > 0x7fffffffu) return SSNT_ERR_UNSUPPORTED;
  const V2sLayout L = v2s_layout(a.Imax, a.Wcap, a.NS);
  if (L.total > kV2sLdsBudget) return SSNT_ERR_UNSUPPORTED;
  if (v2s_launches() & 1) {
    rc = launch_v2_fwd_only(f, true, st);
    if (rc != SSNT_OK) return rc;
  }
  if (!(v2s_launches() & 2)) return SSNT_OK;
  const V2sParams q{L.path_off, L.cdf_off, L.ipad, v2s_cone()};
  const dim3 grid(a.B, (a.NS + L.waves - 1) / L.waves), block(L.waves * 64);
  if (a.D <= 8) return launch_lds(k_v2_sample_walk<8>, grid, block, L.total, kV2sLdsBudget, st, a, q);
  if (a.D <= 16) return launch_lds(k_v2_sample_walk<16>, grid, block, L.total, kV2sLdsBudget, st, a, q);
  if (a.D <= 32) return launch_lds(k_v2_sample_walk<32>, grid, block, L.total, kV2sLdsBudget, st, a, q);
  return launch_lds(k_v2_sample_walk<64>, grid, block, L.total, kV2sLdsBudget, st, a, q);
}

}  // namespace ssnt
