// fwd_bwd.hip -- emit/shift lattice forward-backward (loss + gradients) for gfx950: the two-wave
// kernel, the fallback of the dispatcher (fwd_bwd_dispatch.hip); shared device code: lattice_dev.h.
//
// Lattice semantics: DESIGN.md "Lattice semantics" (SURVEY.md 8(a) A11). The reference
// (nii-yamagishilab/ssnt-tts-rust) has no forward-backward; the transition rules come from its
// decode step: emit (s,p)->(s+1,p), shift (s,p)->(s+1,p+1), no shift out of the last input
// position, terminal emit at the last position (src/lib.rs:186-226).
//
// Kernel shape (one workgroup = one utterance, two waves):
//   wave 0 sweeps alpha rows upward, wave 1 sweeps beta rows downward, concurrently. Each row
//   is an anti-diagonal of the (position, emit-count) grid; a lane holds K consecutive
//   positions p = K*lane + j, and the only cross-lane dependency per step is one DPP
//   wave-shift (v_mov_dpp wave_shr:1 / wave_shl:1) of the boundary element.
//   Phase 1: alpha[0..M] and beta[S-1..M] (M = (S-1)>>1), rows kept in LDS (or a global
//   workspace when T*U*8 B does not fit), inputs streamed through a D-deep register ring.
//   Cut: Z = tree-sum over p of alpha[M][p]*beta[M][p] (canonical binary tree).
//   Phase 2: each wave keeps sweeping and, now that Z is known, emits the gradient row of every
//   transition it passes (wave 0: transitions M..S-1, wave 1: M-1..0) -- the gradient stores
//   stream out while the recurrence is still running.
// Arithmetic: split-exponent xf (xf_math.h); bit-exact with oracle/ssnt_oracle.c.
#include <hip/hip_runtime.h>

#include "lattice_dev.h"
#include "launch_util.h"

namespace ssnt {
namespace {

template <int K, bool OBS, bool LDS, bool VEC>
__global__ __launch_bounds__(128) void k_fwd_bwd(FwdBwdArgs a) {
  constexpr int kRing = ring_depth<K>();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: SGPR rsrcs
  const int lane = threadIdx.x & 63;
  const int T = a.T, U = a.U;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const bool term = (a.flags & SSNT_FLAG_TERMINAL_EMIT) != 0;
  const size_t TU = (size_t)T * U;
  const float* __restrict__ lt = a.log_trans + (size_t)b * TU * 2;
  const float* __restrict__ lo = OBS ? a.log_obs + (size_t)b * TU : nullptr;
  float* __restrict__ g = a.grad ? a.grad + (size_t)b * TU * 2 : nullptr;
  float* __restrict__ go = (OBS && a.grad_obs) ? a.grad_obs + (size_t)b * TU : nullptr;
  float* __restrict__ la = a.log_alpha ? a.log_alpha + (size_t)b * TU : nullptr;
  float* __restrict__ lb = a.log_beta ? a.log_beta + (size_t)b * TU : nullptr;
  int* __restrict__ lae = (la && a.log_alpha_e) ? a.log_alpha_e + (size_t)b * TU : nullptr;
  int* __restrict__ lbe = (lb && a.log_beta_e) ? a.log_beta_e + (size_t)b * TU : nullptr;
  const float dbg_zero = a.log_alpha_e ? 0.0f : -__builtin_inff();  // raw state: mantissa 0

  xf* cutb = reinterpret_cast<xf*>(smem);  // 64*K beta[M] slots
  xf* zsh = cutb + 64 * K;                 // Z broadcast (+ pad)
  xf* rows = LDS ? (zsh + 2) : reinterpret_cast<xf*>(a.workspace) + (size_t)b * TU;

  const bool feasible = S >= 1 && P >= 1 && S <= T && P <= U && S >= P;
  auto fill_rows = [&](int from) {  // zero grads / -inf debug for rows [from, T), split by wave
    for (int s = from + wave; s < T; s += 2) {
      float z[K], ninf[K];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        z[j] = 0.0f;
        ninf[j] = dbg_zero;
      }
      if (g) store_grad_row<K, VEC>(g + (size_t)s * U * 2, z, z, U, lane);
      if (go) store_f_row<K, VEC>(go + (size_t)s * U, z, U, lane);
      if (la) store_f_row<K, VEC>(la + (size_t)s * U, ninf, U, lane);
      if (lb) store_f_row<K, VEC>(lb + (size_t)s * U, ninf, U, lane);
    }
  };
  const float inf_loss = (a.flags & SSNT_FLAG_ZERO_INFINITY) ? 0.0f : __builtin_inff();
  if (!feasible) {
    if ((S > T || P > U || S < 0 || P < 0) && a.status && threadIdx.x == 0)
      atomicOr(a.status, kStatusBadLength);
    fill_rows(0);
    if (threadIdx.x == 0) a.loss[b] = inf_loss;
    return;
  }
  const int M = (S - 1) >> 1;
  const bool fwd = (wave == 0);
  // stream position r -> input row: fwd r, bwd S-1-r; obs row = row + 1 (fwd: alpha[row+1]
  // needs obs[row+1]; bwd: Q = beta[row+1]*obs[row+1]).
  auto srow = [&](int r) { return fwd ? r : S - 1 - r; };

  Item<K, OBS> ring[kRing];
#pragma unroll
  for (int i = 0; i < kRing; ++i) {
    const int row = srow(i);
    ring[i] = load_item<K, OBS, VEC>(lt, lo, row, row + 1, T, U, lane);
  }
  XRow<K> X;  // fwd: alpha row; bwd: beta row
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
    store_row<K, VEC>(rows, X, U, lane);
    if (la) store_dbg_row<K, VEC>(la, lae, X, U, lane);
  }
  const int r0 = fwd ? 0 : 1;               // bwd consumes stream slot 0 for its init
  const int r1 = fwd ? M : S - M;           // phase-1 end (exclusive)
  // bwd init uses ring slot 0 (row S-1)
  if (!fwd) {
    const Item<K, OBS> it = ring[0];
    ring[0] = load_item<K, OBS, VEC>(lt, lo, srow(kRing), srow(kRing) + 1, T, U, lane);
    XRow<K> E, Sh;
    convert<K, OBS>(it, P, lane, E, Sh);
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const bool last = (K * lane + j) == P - 1;
      xf v = term ? xf_norm(E.m[j], E.e[j]) : xf{0.5f, 1};
      X.m[j] = last ? v.m : 0.0f;
      X.e[j] = last ? v.e : XF_EZERO;
    }
    const int s = S - 1;
    if (s > M) store_row<K, VEC>(rows + (size_t)s * U, X, U, lane);
    else store_row<K, VEC>(cutb, X, 64 * K, lane);
    if (lb) store_dbg_row<K, VEC>(lb + (size_t)s * U, lbe ? lbe + (size_t)s * U : nullptr, X, U, lane);
  }
  // ---------------- phase 1 ----------------
  for (int base = (r0 / kRing) * kRing; base < r1; base += kRing) {
#pragma unroll
    for (int i = 0; i < kRing; ++i) {
      const int r = base + i;
      if (r >= r0 && r < r1) {
        const Item<K, OBS> it = ring[i];
        const int nr = srow(r + kRing);
        ring[i] = load_item<K, OBS, VEC>(lt, lo, nr, nr + 1, T, U, lane);
        XRow<K> E, Sh, O;
        convert<K, OBS>(it, P, lane, E, Sh);
        convert_obs<K, OBS>(it, P, lane, O);
        if (fwd) {  // alpha[r+1]
          XRow<K> stay, shft;
          alpha_step<K, OBS>(X, E, Sh, O, stay, shft);
          store_row<K, VEC>(rows + (size_t)(r + 1) * U, X, U, lane);
          if (la) store_dbg_row<K, VEC>(la + (size_t)(r + 1) * U, lae ? lae + (size_t)(r + 1) * U : nullptr, X, U, lane);
        } else {  // beta[s], s = S-1-r
          const int s = S - 1 - r;
          XRow<K> Q, R;
          entering<K, OBS>(X, O, Q, R);
          beta_step<K>(X, E, Sh, Q, R);
          if (s > M) store_row<K, VEC>(rows + (size_t)s * U, X, U, lane);
          else store_row<K, VEC>(cutb, X, 64 * K, lane);
          if (lb) store_dbg_row<K, VEC>(lb + (size_t)s * U, lbe ? lbe + (size_t)s * U : nullptr, X, U, lane);
        }
      }
    }
  }
  __syncthreads();
  // ---------------- cut: Z = sum_p alpha[M][p] * beta[M][p] ----------------
  if (fwd) {
    float wm[K];
    int we[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const xf c = cutb[K * lane + j];
      wm[j] = X.m[j] * c.m;
      we[j] = X.e[j] + c.e;
    }
    // in-lane binary tree (pairs (2i,2i+1) first), then the xor butterfly; the same lines stand in
    // fwd_bwd_stream.hip and fwd_bwd_wide.hip (a shared function: this kernel 98.7 vs 95.6 us)
#pragma unroll
    for (int len = K; len > 1; len >>= 1) {
#pragma unroll
      for (int i = 0; i < len / 2; ++i) {
        const xf r = xf_add(wm[2 * i], we[2 * i], wm[2 * i + 1], we[2 * i + 1]);
        wm[i] = r.m;
        we[i] = r.e;
      }
    }
    // (K == 1: the normalization is overwritten at once, yet without these lines two K = 1
    // instances compile differently, one with 52 instead of 20 bytes of scratch: they stay)
    xf z = (K == 1) ? xf_norm(wm[0], we[0]) : xf{wm[0], we[0]};
    if (K == 1) z = xf{wm[0], we[0]};
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float om = __shfl_xor(z.m, off);
      const int oe = __shfl_xor(z.e, off);
      z = xf_add(z.m, z.e, om, oe);
    }
    if (lane == 0) zsh[0] = z;
  }
  __syncthreads();
  const xf Z = zsh[0];
  if (Z.m == 0.0f) {
    fill_rows(0);
    if (threadIdx.x == 0) a.loss[b] = inf_loss;
    return;
  }
  if (fwd && lane == 0) {
    a.loss[b] = 0.0f - xf_log(Z);
    if (a.z_state) {
      a.z_state[2 * b] = Z.m;
      a.z_state[2 * b + 1] = __builtin_bit_cast(float, Z.e);
    }
  }
  const float izm = 1.0f / Z.m;
  const int ize = -Z.e;
  // ---------------- phase 2 ----------------
  const int q0 = fwd ? M : S - M;
  const int q1 = S;
  for (int base = (q0 / kRing) * kRing; base < q1; base += kRing) {
#pragma unroll
    for (int i = 0; i < kRing; ++i) {
      const int r = base + i;
      if (r >= q0 && r < q1) {
        const Item<K, OBS> it = ring[i];
        const int nr = srow(r + kRing);
        ring[i] = load_item<K, OBS, VEC>(lt, lo, nr, nr + 1, T, U, lane);
        XRow<K> E, Sh, O;
        convert<K, OBS>(it, P, lane, E, Sh);
        convert_obs<K, OBS>(it, P, lane, O);
        float ge[K], gs[K], gob[K];
        if (fwd) {
          const int s = r;  // transition s: alpha[s] (X) -> row s+1
          XRow<K> Q, R;
          if (s + 1 < S) {
            const XRow<K> Bn = load_row<K, VEC>(rows + (size_t)(s + 1) * U, U, lane);
            entering<K, OBS>(Bn, O, Q, R);
          } else {
#pragma unroll
            for (int j = 0; j < K; ++j) {
              const bool last = term && (K * lane + j) == P - 1;
              Q.m[j] = last ? 1.0f : 0.0f;
              Q.e[j] = last ? 0 : XF_EZERO;
              R.m[j] = 0.0f;
              R.e[j] = XF_EZERO;
            }
          }
          if constexpr (OBS) {
            const XRow<K> Bs = (s == M) ? load_row<K, VEC>(cutb, 64 * K, lane)
                                        : load_row<K, VEC>(rows + (size_t)s * U, U, lane);
#pragma unroll
            for (int j = 0; j < K; ++j)
              gob[j] = xf_neg_post((X.m[j] * Bs.m[j]) * izm, X.e[j] + Bs.e[j] + ize);
          }
          XRow<K> stay, shft;
          XRow<K> Xn = X;
          alpha_step<K, OBS>(Xn, E, Sh, O, stay, shft);  // (stay/shft of alpha[s])
#pragma unroll
          for (int j = 0; j < K; ++j) {
            ge[j] = xf_neg_post((stay.m[j] * Q.m[j]) * izm, stay.e[j] + Q.e[j] + ize);
            gs[j] = xf_neg_post((shft.m[j] * R.m[j]) * izm, shft.e[j] + R.e[j] + ize);
          }
          if (g) store_grad_row<K, VEC>(g + (size_t)s * U * 2, ge, gs, U, lane);
          if constexpr (OBS) {
            if (go) store_f_row<K, VEC>(go + (size_t)s * U, gob, U, lane);
          }
          if (s + 1 < S) {
            X = Xn;
            if (la) store_dbg_row<K, VEC>(la + (size_t)(s + 1) * U, lae ? lae + (size_t)(s + 1) * U : nullptr, X, U, lane);
          }
        } else {
          const int s = S - 1 - r;  // transition s: beta[s+1] (X) -> beta[s]
          XRow<K> Q, R;
          entering<K, OBS>(X, O, Q, R);
          const XRow<K> A = load_row<K, VEC>(rows + (size_t)s * U, U, lane);
#pragma unroll
          for (int j = 0; j < K; ++j) {
            ge[j] = xf_neg_post(((A.m[j] * E.m[j]) * Q.m[j]) * izm, A.e[j] + E.e[j] + Q.e[j] + ize);
            gs[j] = xf_neg_post(((A.m[j] * Sh.m[j]) * R.m[j]) * izm, A.e[j] + Sh.e[j] + R.e[j] + ize);
          }
          beta_step<K>(X, E, Sh, Q, R);
          if constexpr (OBS) {
#pragma unroll
            for (int j = 0; j < K; ++j)
              gob[j] = xf_neg_post((A.m[j] * X.m[j]) * izm, A.e[j] + X.e[j] + ize);
            if (go) store_f_row<K, VEC>(go + (size_t)s * U, gob, U, lane);
          }
          if (g) store_grad_row<K, VEC>(g + (size_t)s * U * 2, ge, gs, U, lane);
          if (lb) store_dbg_row<K, VEC>(lb + (size_t)s * U, lbe ? lbe + (size_t)s * U : nullptr, X, U, lane);
        }
      }
    }
  }
  fill_rows(S);
}

template <int K, bool OBS, bool LDS, bool VEC>
int launch_kernel(const FwdBwdArgs& a, size_t lds, hipStream_t st) {
  note_fwd_bwd_dispatch("k_fwd_bwd<K=%d,OBS=%d,LDS=%d,VEC=%d>", K, (int)OBS, (int)LDS, (int)VEC);
  return launch_lds(k_fwd_bwd<K, OBS, LDS, VEC>, dim3(a.B), dim3(128), lds, kLdsBudget, st, a);
}

template <int K, bool OBS>
int launch_k(const FwdBwdArgs& a, const RowsPlan& p, hipStream_t st) {
  if (!p.lds && (a.workspace == nullptr || a.workspace_bytes < fwd_bwd_workspace_bytes(a.B, a.T, a.U)))
    return SSNT_ERR_WORKSPACE;
  const bool vec = (a.U % K == 0) && all_aligned(a, 16, 16, 16);
  if (p.lds)
    return vec ? launch_kernel<K, OBS, true, true>(a, p.shm_bytes, st) : launch_kernel<K, OBS, true, false>(a, p.shm_bytes, st);
  return vec ? launch_kernel<K, OBS, false, true>(a, p.shm_bytes, st) : launch_kernel<K, OBS, false, false>(a, p.shm_bytes, st);
}
template <bool OBS>
int launch_obs(const FwdBwdArgs& a, const RowsPlan& p, hipStream_t st) {
  if (p.K == 1) return launch_k<1, OBS>(a, p, st);
  if (p.K == 2) return launch_k<2, OBS>(a, p, st);
  return p.K == 4 ? launch_k<4, OBS>(a, p, st) : launch_k<8, OBS>(a, p, st);
}

}  // namespace

// cut buffer (64K xf) + Z broadcast, then the rows [T][U] when they fit
RowsPlan simple_plan(int T, int U) {
  RowsPlan p{};
  p.K = lanes_for(U);
  const size_t head = (size_t)(64 * p.K + 2) * sizeof(xf), rows = (size_t)T * U * sizeof(xf);
  p.supported = p.K != 0;
  p.lds = head + rows <= kLdsBudget;
  p.shm_bytes = p.lds ? head + rows : head;
  return p;
}

int launch_fwd_bwd_simple(const FwdBwdArgs& a, hipStream_t st) {
  const RowsPlan p = simple_plan(a.T, a.U);
  if (!p.supported) return SSNT_ERR_UNSUPPORTED;
  return a.log_obs ? launch_obs<true>(a, p, st) : launch_obs<false>(a, p, st);
}

}  // namespace ssnt
