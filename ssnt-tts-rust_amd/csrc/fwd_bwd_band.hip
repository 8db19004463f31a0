// fwd_bwd_band.hip -- forward-backward on a band of the emit/shift lattice:
// R columns per step, the first of them band_start[b,s], which stays or moves down by one from a
// step to the next. Work and memory are O(T*R); the dense lattice is never formed.
//
// Kernel shape: the two-wave form of fwd_bwd.hip (one workgroup = one utterance, wave 0 sweeps
// alpha upward, wave 1 beta downward, cut at M = (S-1)>>1, gradients stream out in phase 2). The
// band tensor is addressed as a dense lattice with U := R, and a lane holds K consecutive band
// columns r = K*lane + j of the current row. Band cell (s,r) is lattice cell (s, band_start[s]+r),
// so a row is held in the coordinates of its own step; on a step where the band moves
// (delta = band_start[s+1] - band_start[s] = 1) the partner of column r in the next row is column
// r - 1, and the row shifts by one lane through a second DPP move chosen by that wave-uniform bit.
// band_start is validated and staged in LDS before the step loop; the per-step reads of it depend
// on the loop counter alone. Arithmetic: lattice_dev.h / xf_math.h, the bits of the dense result on
// the lattice with every cell outside the band removed (oracle/ssnt_oracle.c on that embedding).
#include <hip/hip_runtime.h>

#include "lattice_dev.h"
#include "launch_util.h"

namespace ssnt {
namespace {

// LDS ahead of the rows: beta[M] (64K xf) | block sums and pad (4 xf) | the cut's product slots,
// two aligned blocks of at most 64K (128K xf) | band_start[0..S] (T+1 i32, padded to 16 B)
__host__ __device__ constexpr size_t band_head_bytes(int K, int T) {
  return (size_t)(64 * K + 4 + 128 * K) * sizeof(xf) + (((size_t)(T + 1) * sizeof(int) + 15) & ~(size_t)15);
}

// What a row's transition needs of the band: does the next row start one column further
// (mv), the emit/shift masks' extent in this row's coordinates (Pc: emits r < Pc, shifts
// r < Pc - 1; the shift out of r = R-1 exists only when the band moves) and the live columns of
// the next row (Po).
// The staged word of step s holds band_start[s] and, in bit 30, whether step s+1 starts one
// column further (never for the last step). The emit out of r = 0 on a moving step needs no mask
// of its own: its partner in the next row is the column the DPP shift fills with the canonical
// zero, its alpha term is not part of any column of the next row, and exp() of any input has a
// finite mantissa, so its products are exact zeros. Past the band (r >= R) alpha is zero by
// induction, and what beta holds there (lanes beyond R only) enters no column below R.
constexpr int kBandStartMask = (1 << 30) - 1;
struct BandStep {
  int mv, Pc, Po, Peff;
};
__device__ __forceinline__ BandStep band_step(int word, int P, int R) {
  const int st = word & kBandStartMask;
  BandStep d;
  d.mv = (word >> 30) & 1;
  d.Peff = P - st;
  d.Pc = min(d.Peff, R + d.mv);
  d.Po = min(d.Peff - d.mv, R);
  return d;
}

// alpha[s+1] from alpha[s] (lattice_dev.h alpha_step, with the next row in its own coordinates):
// the band stays: new[r] = stay[r] + shft[r-1]; it moves: new[r] = stay[r+1] + shft[r].
template <int K, bool OBS>
__device__ __forceinline__ void alpha_step_band(XRow<K>& A, const XRow<K>& E, const XRow<K>& Sh,
                                                const XRow<K>& O, bool mv, XRow<K>& stay, XRow<K>& shft) {
#pragma unroll
  for (int j = 0; j < K; ++j) {
    stay.m[j] = A.m[j] * E.m[j];
    stay.e[j] = A.e[j] + E.e[j];
    shft.m[j] = A.m[j] * Sh.m[j];
    shft.e[j] = A.e[j] + Sh.e[j];
  }
  const float lm = shr1(shft.m[K - 1]);
  const int le = shr1(shft.e[K - 1]);
  const float um = shl1(stay.m[0]);
  const int ue = shl1(stay.e[0]);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float sm1 = (j == K - 1) ? um : stay.m[j + 1 < K ? j + 1 : 0];
    const int se1 = (j == K - 1) ? ue : stay.e[j + 1 < K ? j + 1 : 0];
    const float hm0 = (j == 0) ? lm : shft.m[j > 0 ? j - 1 : 0];
    const int he0 = (j == 0) ? le : shft.e[j > 0 ? j - 1 : 0];
    const float am = mv ? sm1 : stay.m[j];
    const int ae = mv ? se1 : stay.e[j];
    const float hm = mv ? shft.m[j] : hm0;
    const int he = mv ? shft.e[j] : he0;
    const int em = max(ae, he);
    float sum = xldexp(am, ae - em) + xldexp(hm, he - em);
    int ee = em;
    if constexpr (OBS) {
      sum = sum * O.m[j];
      ee = ee + O.e[j];
    }
    const xf r = xf_norm(sum, ee);
    A.m[j] = r.m;
    A.e[j] = r.e;
  }
}

// entering() in the coordinates of the row below: the emit of column r enters the next row at
// r - mv, its shift at r + 1 - mv
template <int K, bool OBS>
__device__ __forceinline__ void entering_band(const XRow<K>& Bn, const XRow<K>& O, bool mv, XRow<K>& Q,
                                              XRow<K>& R) {
  XRow<K> Q0, R0;
  entering<K, OBS>(Bn, O, Q0, R0);
  const float dm = shr1(Q0.m[K - 1]);
  const int de = shr1(Q0.e[K - 1]);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float pm = (j == 0) ? dm : Q0.m[j > 0 ? j - 1 : 0];
    const int pe = (j == 0) ? de : Q0.e[j > 0 ? j - 1 : 0];
    Q.m[j] = mv ? pm : Q0.m[j];
    Q.e[j] = mv ? pe : Q0.e[j];
    R.m[j] = mv ? Q0.m[j] : R0.m[j];
    R.e[j] = mv ? Q0.e[j] : R0.e[j];
  }
}

template <int K, bool OBS, bool LDS, bool VEC>
__global__ __launch_bounds__(128) void k_fwd_bwd_band(FwdBwdBandArgs a) {
  constexpr int kRing = ring_depth<K>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int T = a.T, R = a.R;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const bool term = (a.flags & SSNT_FLAG_TERMINAL_EMIT) != 0;
  const size_t TR = (size_t)T * R;
  const float* __restrict__ lt = a.log_trans + (size_t)b * TR * 2;
  const float* __restrict__ lo = OBS ? a.log_obs + (size_t)b * TR : nullptr;
  float* __restrict__ g = a.grad ? a.grad + (size_t)b * TR * 2 : nullptr;
  float* __restrict__ go = (OBS && a.grad_obs) ? a.grad_obs + (size_t)b * TR : nullptr;
  const bool want = g || go;  // no gradient: no rows are kept, the kernel ends at the cut

  xf* cutb = reinterpret_cast<xf*>(smem);  // 64*K beta[M] slots
  xf* zsh = cutb + 64 * K;                 // the two block sums (+ pad)
  xf* zslot = zsh + 4;                     // 2 * R' product slots at the cut
  int* bsl = reinterpret_cast<int*>(zslot + 128 * K);  // band_start[0..S]
  xf* rows = LDS ? reinterpret_cast<xf*>(smem + band_head_bytes(K, T))
                 : reinterpret_cast<xf*>(a.workspace) + (size_t)b * TR;

  auto fill_rows = [&](int from) {  // zero grads for rows [from, T), split by wave
    for (int s = from + wave; s < T; s += 2) {
      float z[K];
#pragma unroll
      for (int j = 0; j < K; ++j) z[j] = 0.0f;
      if (g) store_grad_row<K, VEC>(g + (size_t)s * R * 2, z, z, R, lane);
      if (go) store_f_row<K, VEC>(go + (size_t)s * R, z, R, lane);
    }
  };
  const float inf_loss = (a.flags & SSNT_FLAG_ZERO_INFINITY) ? 0.0f : __builtin_inff();
  const bool feasible = S >= 1 && P >= 1 && S <= T && S >= P;
  if (!feasible) {
    if ((S > T || S < 0 || P < 0) && a.status && threadIdx.x == 0) atomicOr(a.status, kStatusBadLength);
    fill_rows(0);
    if (threadIdx.x == 0) a.loss[b] = inf_loss;
    return;
  }
  // ---------------- band prologue: stage and validate (comparisons only, nothing addressed by it) ----
  {
    const int* __restrict__ bs = a.band_start + (size_t)b * T;
    bool bad = false;
    for (int s = threadIdx.x; s < S; s += 128) {
      const int v = bs[s];
      if (s == 0) bad |= v != 0;
      unsigned mv = 0;
      if (s == S - 1) {
        const long long room = (long long)P - 1 - (long long)v;  // column of P-1 in the last window
        bad |= room < 0 || room >= R;
        bsl[S] = v & kBandStartMask;  // (read ahead by the forward sweep's last step, never used)
      } else {
        mv = (unsigned)bs[s + 1] - (unsigned)v;
        bad |= mv > 1u;
      }
      bsl[s] = (v & kBandStartMask) | (int)((mv & 1u) << 30);
    }
    for (int i = threadIdx.x; i < 128 * K; i += 128) zslot[i] = xf_zero();
    if (__syncthreads_or(bad ? 1 : 0)) {
      if (a.status && threadIdx.x == 0) atomicOr(a.status, kStatusBadBand);
      fill_rows(0);
      if (threadIdx.x == 0) a.loss[b] = inf_loss;
      return;
    }
  }
  const int M = (S - 1) >> 1;
  const bool fwd = (wave == 0);
  auto srow = [&](int r) { return fwd ? r : S - 1 - r; };

  Item<K, OBS> ring[kRing];
#pragma unroll
  for (int i = 0; i < kRing; ++i) {
    const int row = srow(i);
    ring[i] = load_item<K, OBS, VEC>(lt, lo, row, row + 1, T, R, lane);
  }
  XRow<K> X;  // fwd: alpha row; bwd: beta row -- in the coordinates of its own step
  // ---------------- init ----------------
  if (fwd) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      X.m[j] = 0.0f;
      X.e[j] = XF_EZERO;
    }
    if (lane == 0) {
      const xf a0 = alpha0<OBS>(lo);
      X.m[0] = a0.m;
      X.e[0] = a0.e;
    }
    if (want) store_row<K, VEC>(rows, X, R, lane);
  }
  const int r0 = fwd ? 0 : 1;
  const int r1 = fwd ? M : S - M;
  if (!fwd) {
    const Item<K, OBS> it = ring[0];
    ring[0] = load_item<K, OBS, VEC>(lt, lo, srow(kRing), srow(kRing) + 1, T, R, lane);
    const BandStep d = band_step(__builtin_amdgcn_readfirstlane(bsl[S - 1]), P, R);
    XRow<K> E, Sh;
    convert<K, OBS>(it, d.Pc, lane, E, Sh);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool last = (K * lane + j) == d.Peff - 1;
      xf v = term ? xf_norm(E.m[j], E.e[j]) : xf{0.5f, 1};
      X.m[j] = last ? v.m : 0.0f;
      X.e[j] = last ? v.e : XF_EZERO;
    }
    const int s = S - 1;
    if (s > M) {
      if (want) store_row<K, VEC>(rows + (size_t)s * R, X, R, lane);
    } else {
      store_row<K, VEC>(cutb, X, 64 * K, lane);
    }
  }
  // the staged word of the next transition row, read one step ahead (a wave's rows are
  // consecutive through both phases: forward s, s+1, ..; backward s, s-1, ..)
  auto next_row = [&](int s) { return fwd ? s + 1 : max(s - 1, 0); };
  int word_ahead = bsl[max(srow(r0), 0)];
  // ---------------- phase 1 ----------------
  for (int base = (r0 / kRing) * kRing; base < r1; base += kRing) {
#pragma unroll
    for (int i = 0; i < kRing; ++i) {
      const int r = base + i;
      if (r >= r0 && r < r1) {
        const Item<K, OBS> it = ring[i];
        const int nr = srow(r + kRing);
        ring[i] = load_item<K, OBS, VEC>(lt, lo, nr, nr + 1, T, R, lane);
        const int s = srow(r);  // the transition row
        const BandStep d = band_step(__builtin_amdgcn_readfirstlane(word_ahead), P, R);
        word_ahead = bsl[next_row(s)];
        XRow<K> E, Sh, O;
        convert<K, OBS>(it, d.Pc, lane, E, Sh);
        convert_obs<K, OBS>(it, d.Po, lane, O);
        if (fwd) {  // alpha[r+1]
          XRow<K> stay, shft;
          alpha_step_band<K, OBS>(X, E, Sh, O, d.mv != 0, stay, shft);
          if (want) store_row<K, VEC>(rows + (size_t)(r + 1) * R, X, R, lane);
        } else {  // beta[s]
          XRow<K> Q, Rr;
          entering_band<K, OBS>(X, O, d.mv != 0, Q, Rr);
          beta_step<K>(X, E, Sh, Q, Rr);
          if (s > M) {
            if (want) store_row<K, VEC>(rows + (size_t)s * R, X, R, lane);
          } else {
            store_row<K, VEC>(cutb, X, 64 * K, lane);
          }
        }
      }
    }
  }
  __syncthreads();
  // ---------------- cut: Z = sum_p alpha[M][p] * beta[M][p], in the dense tree's order ----------
  // The dense tree pairs absolute positions (2i, 2i+1) first. With R' = R rounded up to a power of
  // two, the band at row M lies inside the aligned blocks [base, base+R') and [base+R', base+2R'):
  // the products go to slot p - base, each wave sums one block, and Z is the sum of the two (every
  // other leaf of the dense tree is an exact zero, which changes no bits of a sum).
  const int Rp = R <= 1 ? 1 : 1 << (32 - __builtin_clz(R - 1));
  if (fwd) {
    const int off = (__builtin_amdgcn_readfirstlane(bsl[M]) & kBandStartMask) & (Rp - 1);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int r = K * lane + j;
      const xf c = cutb[r];
      if (r < R) zslot[off + r] = xf{X.m[j] * c.m, X.e[j] + c.e};
    }
  }
  __syncthreads();
  {
    float wm[K];
    int we[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const int i = K * lane + j;
      const xf v = i < Rp ? zslot[wave * Rp + i] : xf_zero();
      wm[j] = v.m;
      we[j] = v.e;
    }
#pragma unroll
    for (int len = K; len > 1; len >>= 1) {
#pragma unroll
      for (int i = 0; i < len / 2; ++i) {
        const xf r = xf_add(wm[2 * i], we[2 * i], wm[2 * i + 1], we[2 * i + 1]);
        wm[i] = r.m;
        we[i] = r.e;
      }
    }
    xf z = xf{wm[0], we[0]};
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float om = __shfl_xor(z.m, off);
      const int oe = __shfl_xor(z.e, off);
      z = xf_add(z.m, z.e, om, oe);
    }
    if (lane == 0) zsh[wave] = z;
  }
  __syncthreads();
  const xf Z = xf_add(zsh[0].m, zsh[0].e, zsh[1].m, zsh[1].e);
  if (Z.m == 0.0f) {
    fill_rows(0);
    if (threadIdx.x == 0) a.loss[b] = inf_loss;
    return;
  }
  if (fwd && lane == 0) a.loss[b] = 0.0f - xf_log(Z);
  if (!want) return;
  const float izm = 1.0f / Z.m;
  const int ize = -Z.e;
  // ---------------- phase 2 ----------------
  const int q0 = fwd ? M : S - M;
  const int q1 = S;
  // The other sweep's row a transition needs (forward: beta[s+1]; backward: alpha[s]) is read one
  // step ahead, so its latency -- LDS, or the workspace's -- is not on the step. Every such row
  // was stored before the cut's barriers. (Indices stay inside [0, S-1]; the forward sweep's last
  // step uses none.)
  auto other_row = [&](int s) { return fwd ? min(s + 1, S - 1) : max(s, 0); };
  XRow<K> row_ahead = load_row<K, VEC>(rows + (size_t)other_row(srow(q0)) * R, R, lane);
  XRow<K> Bs = load_row<K, VEC>(cutb, 64 * K, lane);  // forward, log_obs: beta[s], first beta[M]
  for (int base = (q0 / kRing) * kRing; base < q1; base += kRing) {
#pragma unroll
    for (int i = 0; i < kRing; ++i) {
      const int r = base + i;
      if (r >= q0 && r < q1) {
        const Item<K, OBS> it = ring[i];
        const int nr = srow(r + kRing);
        ring[i] = load_item<K, OBS, VEC>(lt, lo, nr, nr + 1, T, R, lane);
        const int s = srow(r);  // transition s
        const BandStep d = band_step(__builtin_amdgcn_readfirstlane(word_ahead), P, R);
        word_ahead = bsl[next_row(s)];
        const XRow<K> other = row_ahead;
        row_ahead = load_row<K, VEC>(rows + (size_t)other_row(fwd ? s + 1 : s - 1) * R, R, lane);
        const bool mv = d.mv != 0;
        XRow<K> E, Sh, O;
        convert<K, OBS>(it, d.Pc, lane, E, Sh);
        convert_obs<K, OBS>(it, d.Po, lane, O);
        float ge[K], gs[K], gob[K];
        if (fwd) {  // alpha[s] (X) -> row s+1
          XRow<K> Q, Rr;
          if (s + 1 < S) {
            entering_band<K, OBS>(other, O, mv, Q, Rr);
          } else {
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const bool last = term && (K * lane + j) == d.Peff - 1;
              Q.m[j] = last ? 1.0f : 0.0f;
              Q.e[j] = last ? 0 : XF_EZERO;
              Rr.m[j] = 0.0f;
              Rr.e[j] = XF_EZERO;
            }
          }
          if constexpr (OBS) {
#pragma unroll
            for (int j = 0; j < K; ++j)
              gob[j] = xf_neg_post((X.m[j] * Bs.m[j]) * izm, X.e[j] + Bs.e[j] + ize);
            Bs = other;  // beta[s+1]: the next step's beta[s]
          }
          XRow<K> stay, shft;
          XRow<K> Xn = X;
          alpha_step_band<K, OBS>(Xn, E, Sh, O, mv, stay, shft);
#pragma unroll
          for (int j = 0; j < K; ++j) {
            ge[j] = xf_neg_post((stay.m[j] * Q.m[j]) * izm, stay.e[j] + Q.e[j] + ize);
            gs[j] = xf_neg_post((shft.m[j] * Rr.m[j]) * izm, shft.e[j] + Rr.e[j] + ize);
          }
          if (g) store_grad_row<K, VEC>(g + (size_t)s * R * 2, ge, gs, R, lane);
          if constexpr (OBS) {
            if (go) store_f_row<K, VEC>(go + (size_t)s * R, gob, R, lane);
          }
          if (s + 1 < S) X = Xn;
        } else {  // beta[s+1] (X) -> beta[s]
          XRow<K> Q, Rr;
          entering_band<K, OBS>(X, O, mv, Q, Rr);
          const XRow<K> A = other;
#pragma unroll
          for (int j = 0; j < K; ++j) {
            ge[j] = xf_neg_post(((A.m[j] * E.m[j]) * Q.m[j]) * izm, A.e[j] + E.e[j] + Q.e[j] + ize);
            gs[j] = xf_neg_post(((A.m[j] * Sh.m[j]) * Rr.m[j]) * izm, A.e[j] + Sh.e[j] + Rr.e[j] + ize);
          }
          beta_step<K>(X, E, Sh, Q, Rr);
          if constexpr (OBS) {
#pragma unroll
            for (int j = 0; j < K; ++j)
              gob[j] = xf_neg_post((A.m[j] * X.m[j]) * izm, A.e[j] + X.e[j] + ize);
            if (go) store_f_row<K, VEC>(go + (size_t)s * R, gob, R, lane);
          }
          if (g) store_grad_row<K, VEC>(g + (size_t)s * R * 2, ge, gs, R, lane);
        }
      }
    }
  }
  fill_rows(S);
}

template <int K, bool OBS, bool LDS, bool VEC>
int launch_kernel(const FwdBwdBandArgs& a, size_t lds, hipStream_t st) {
  return launch_lds(k_fwd_bwd_band<K, OBS, LDS, VEC>, dim3(a.B), dim3(128), lds, kLdsBudget, st, a);
}

template <int K, bool OBS>
int launch_k(const FwdBwdBandArgs& a, bool rows_lds, size_t shm, hipStream_t st) {
  const bool vec = (a.R % K == 0) && aligned_to(a.log_trans, 16) && aligned_to(a.grad, 16) &&
                   aligned_to(a.log_obs, 16) && aligned_to(a.grad_obs, 16) && aligned_to(a.workspace, 16);
  if (rows_lds)
    return vec ? launch_kernel<K, OBS, true, true>(a, shm, st) : launch_kernel<K, OBS, true, false>(a, shm, st);
  return vec ? launch_kernel<K, OBS, false, true>(a, shm, st) : launch_kernel<K, OBS, false, false>(a, shm, st);
}
template <bool OBS>
int launch_obs(const FwdBwdBandArgs& a, int K, bool rows_lds, size_t shm, hipStream_t st) {
  if (K == 1) return launch_k<1, OBS>(a, rows_lds, shm, st);
  return K == 2 ? launch_k<2, OBS>(a, rows_lds, shm, st) : launch_k<4, OBS>(a, rows_lds, shm, st);
}

}  // namespace

// the head (band_head_bytes), then the rows [T][R] of both directions when they fit
RowsPlan band_plan(int B, int T, int R) {
  RowsPlan p{};
  if (B <= 0 || T <= 0 || R < 1 || R > 256) return p;
  p.K = lanes_for(R);
  const size_t head = band_head_bytes(p.K, T), rows = (size_t)T * R * sizeof(xf);
  p.supported = head <= kLdsBudget;
  p.lds = p.supported && head + rows <= kLdsBudget;
  p.shm_bytes = p.lds ? head + rows : head;
  p.workspace_bytes = (p.supported && !p.lds) ? (size_t)B * rows : 0;
  return p;
}

size_t fwd_bwd_band_workspace_bytes(int B, int T, int R) { return band_plan(B, T, R).workspace_bytes; }

int launch_fwd_bwd_band(const FwdBwdBandArgs& a, hipStream_t st) {
  if (a.R < 1 || a.R > 256) return SSNT_ERR_UNSUPPORTED;  // (first: an empty tensor has no address)
  if (a.B < 0 || a.T <= 0 || !a.log_trans || !a.band_start || !a.step_len || !a.pos_len || !a.loss)
    return SSNT_ERR_INVALID_ARG;
  if (a.grad_obs && !a.log_obs) return SSNT_ERR_INVALID_ARG;
  if (a.B == 0) return SSNT_OK;
  const RowsPlan p = band_plan(a.B, a.T, a.R);
  if (!p.supported) return SSNT_ERR_UNSUPPORTED;
  const bool want = a.grad || a.grad_obs;
  if (want && !p.lds && (a.workspace == nullptr || a.workspace_bytes < p.workspace_bytes))
    return SSNT_ERR_WORKSPACE;
  // without a gradient no row is kept: the head alone, whatever the plan says of the rows
  const bool rows_lds = want && p.lds;
  const size_t shm = rows_lds ? p.shm_bytes : band_head_bytes(p.K, a.T);
  FwdBwdBandArgs x = a;
  if (!want || p.lds) x.workspace = nullptr;
  return a.log_obs ? launch_obs<true>(x, p.K, rows_lds, shm, st) : launch_obs<false>(x, p.K, rows_lds, shm, st);
}

}  // namespace ssnt
