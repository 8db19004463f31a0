// expected_cost.hip -- the expected cost of a path under the posterior of the emit/shift lattice
// (the expectation semiring) and its gradients, for gfx950.
//
// Semantics: DESIGN.md 2.8; the kernels: DESIGN.md 5.12. risk = E[sum of cost over the path's
// edges]; grad_cost is the edge posterior q, grad_trans = q * (abar[src] + c + bbar[dst] - risk) a
// covariance, grad_obs the same for a cell. Two launches:
//
//   k_expected_cost_sweep   one workgroup = one utterance and one direction, on align_dev.h's
//               chain-and-loaders scaffold (wave 0 the chain, waves 1..4 the loaders). Workgroups
//               [0, B) sweep forward: alpha in xf form plus abar, the mean cost accumulated before
//               the cell, a plain f32 (form (a) of DESIGN.md 2.8: the convex combination of the two
//               entering terms at their common exponent, one division per cell). Workgroups
//               [B, 2B) sweep backward: beta plus bbar, the same operations mirrored. Forward
//               chunks run up from row 0, backward chunks down from row S-2: a load unit is one
//               position, log_trans + cost (16 B; + log_obs), converted in registers (xf_exp) on
//               the way to LDS; one workgroup barrier per chunk. With gradients requested both
//               sweeps store every row (m, e, mean: 12 B per cell and direction) to the workspace;
//               the forward sweep alone forms risk, loss and Z, so the value-only form (the B
//               forward workgroups, no row stores) returns the same bits.
//   k_expected_cost_grad    a grid over (utterance, block of step rows): alpha-side row s, beta-side
//               rows s and s+1, the inputs again, and every element of every requested gradient,
//               zeros outside the lattice included.
#include <hip/hip_runtime.h>

#include "align_dev.h"
#include "ec_rows.h"

namespace ssnt {
namespace {

constexpr int kEcJunk = 64;  // elements behind each buffer, for unused units' writes: lane (< 64)
constexpr int kEcGradThreads = 256;
constexpr int kEcGradCells = 4096;     // cells per workgroup of the gradient launch, about

struct EcLayout {
  int K, R;
  size_t base_off, total;  // bytes
};
// two chunk buffers each of (E, Sh) as xf, the cost pair (with the mean only), and O as xf
inline EcLayout ec_layout(int U, int R, bool obs, bool mean = true) {
  EcLayout L{};
  L.K = aln_k(U);
  L.R = R;
  const size_t buf = (size_t)R * L.K * aln_kstride(L.K) + kEcJunk;  // elements of one buffer
  L.base_off = kAlnHeadBytes;
  L.total = L.base_off + 2 * buf * (16 + (mean ? 8 : 0) + (obs ? 8 : 0));
  return L;
}
inline EcLayout ec_pick(int U, bool obs, bool mean = true) {
  return aln_pick(aln_chunk_rows((U + 63) / 64), 1, [&](int r) { return ec_layout(U, r, obs, mean); });
}
inline size_t ec_rows_bytes(int B, int T, int U) { return (size_t)B * T * ec_upad(U) * 12; }

struct EcParams {
  int R, Up;
  unsigned base_off;
};

// MEAN == false (GRAD only): alpha and beta alone, for the duration posterior: no
// cost load, no mean arithmetic, no mean plane (m, e: 8 B per cell and direction), no risk.
template <int K, bool OBS, bool GRAD, bool MEAN = true>
__global__ __launch_bounds__(kAlnThreads) void k_expected_cost_sweep(ExpectedCostArgs a, EcParams q) {
  constexpr int kPl = MEAN ? 3 : 2;  // planes of a stored row
  constexpr int kKs = aln_kstride(K);
  constexpr int kRow = K * kKs;  // LDS row stride in cells
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // which direction this workgroup sweeps: 0 forward (rows up from 0), 1 backward (rows down from S-2)
  const int dir = GRAD && (int)blockIdx.x >= a.B ? 1 : 0;
  const int b = blockIdx.x - dir * a.B;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63;
  const int T = a.T, U = a.U, R = q.R, Up = q.Up;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const size_t TU = (size_t)T * U;
  const float* lt = a.log_trans + (size_t)b * TU * 2;
  const float* cs = MEAN ? a.cost + (size_t)b * TU * 2 : nullptr;
  const float* lo = OBS ? a.log_obs + (size_t)b * TU : nullptr;
  const bool term = (a.flags & SSNT_FLAG_TERMINAL_EMIT) != 0;
  float* head = GRAD ? reinterpret_cast<float*>(a.workspace) + (size_t)b * 4 : nullptr;

  auto publish = [&](xf Z, float risk) {  // one lane
    const bool none = Z.m == 0.0f;
    if constexpr (MEAN) a.risk[b] = none ? 0.0f : risk;
    if (a.loss) a.loss[b] = none ? __builtin_inff() : 0.0f - xf_log(Z);
    if constexpr (GRAD) {
      head[0] = Z.m;
      head[1] = __builtin_bit_cast(float, Z.e);
      head[2] = none ? 0.0f : risk;
      head[3] = 0.0f;
    }
  };
  if (!aln_lengths_ok(S, P, T, U, a.status, tid)) {
    if (tid == 0 && dir == 0) publish(xf_zero(), 0.0f);
    return;
  }

  const bool loader = wave >= 1;
  const int bufsz = R * kRow + kEcJunk;  // cells of one buffer
  unsigned char* dbase = smem + q.base_off;
  float4* ltb = reinterpret_cast<float4*>(dbase);
  float2* ccb = reinterpret_cast<float2*>(dbase + (size_t)2 * bufsz * 16);
  float2* obb = reinterpret_cast<float2*>(dbase + (size_t)2 * bufsz * (MEAN ? 24 : 16));
  float* rows = GRAD ? ec_rows_base(a.workspace, a.B) + ((size_t)dir * a.B + b) * T * Up * kPl : nullptr;

  // ------------------------------------------------------------------ loaders
  const int NC = (S - 1 + R - 1) / R;  // chunks of transition rows 0..S-2, in either direction
  int goff[kAlnUnits], loff[kAlnUnits];
  f32x2 lreg[kAlnUnits], creg[MEAN ? kAlnUnits : 1];
  float oreg[OBS ? kAlnUnits : 1];
  if (loader) {
    const int w = wave - 1;
    const int upr = (U + 63) / 64;  // units per row and lane
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      aln_unit<K>(w, lane, u, upr, 1, 8, R, U, goff[u], loff[u]);
    });
  }
  // the transition rows of chunk c, lowest first: [first, first + count)
  auto chunk_first = [&](int c) { return dir ? max(S - 1 - (c + 1) * R, 0) : c * R; };
  auto chunk_count = [&](int c) { return min(R, S - 1 - c * R); };
  // global -> registers: log_trans and cost of the chunk's rows, log_obs of the rows they lead to
  auto issue = [&](int c) __attribute__((always_inline)) {
    const int r0 = chunk_first(c);
    const int n = chunk_count(c);
    const __amdgpu_buffer_rsrc_t rs = brsrc(lt + (size_t)r0 * U * 2, (unsigned)(n * U) * 8u);
    const __amdgpu_buffer_rsrc_t rc = brsrc(MEAN ? cs + (size_t)r0 * U * 2 : nullptr, (unsigned)(n * U) * 8u);
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      lreg[u] = rbuf_ld2(rs, goff[u], 0, 0);
    });
    if constexpr (MEAN) {
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        creg[u] = rbuf_ld2(rc, goff[u], 0, 0);
      });
    }
    if constexpr (OBS) {
      const __amdgpu_buffer_rsrc_t ro = brsrc(lo + (size_t)(r0 + 1) * U, (unsigned)(n * U) * 4u);
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        oreg[u] = rbuf_ld1(ro, goff[u] == kAlnNoUnit ? kAlnNoUnit : goff[u] >> 1, 0, 0);
      });
    }
  };
  // registers -> LDS buffer c & 1: (E.m, E.e, Sh.m, Sh.e) per cell, the cost pair as it is, (O.m, O.e)
  auto commit = [&](int c) __attribute__((always_inline)) {
    float4* dst = ltb + (size_t)(c & 1) * bufsz;
    float2* dstc = ccb + (size_t)(c & 1) * bufsz;
    static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
      constexpr int u = decltype(Ic)::value;
      float me, ms;
      int ee, es;
      xf_exp_pair(lreg[u].x, lreg[u].y, true, true, me, ee, ms, es);
      dst[loff[u]] = make_float4(me, __builtin_bit_cast(float, ee), ms, __builtin_bit_cast(float, es));
      if constexpr (MEAN) dstc[loff[u]] = make_float2(creg[u].x, creg[u].y);
    });
    if constexpr (OBS) {
      float2* dsto = obb + (size_t)(c & 1) * bufsz;
      static_for<kAlnUnits>([&](auto Ic) __attribute__((always_inline)) {
        constexpr int u = decltype(Ic)::value;
        const xf o = xf_exp(oreg[u], true);
        dsto[loff[u]] = make_float2(o.m, __builtin_bit_cast(float, o.e));
      });
    }
  };

  // ------------------------------------------------------------------ chains
  // X: alpha (forward) or beta (backward) in xf form; Mn: abar / bbar. A lane holds positions
  // K*lane .. K*lane + K-1.
  float Xm[K], Mn[K];
  int Xe[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    Xm[j] = 0.0f;
    Xe[j] = XF_EZERO;
    Mn[j] = 0.0f;
  }
  const bool chain = wave == 0;
  const bool my_last = K * lane <= P - 1 && P - 1 < K * lane + K;  // the one lane that holds P-1
  // the terminal emit and its cost (read under the flag only)
  xf Et = xf{0.5f, 1};
  float ct = 0.0f;
  if (chain && term) {
    const size_t at = ((size_t)(S - 1) * U + (P - 1)) * 2;
    const xf e = xf_exp(lt[at], true);
    Et = xf_norm(e.m, e.e);
    if constexpr (MEAN) ct = cs[at];
  }
  auto store_row = [&](int s) __attribute__((always_inline)) {
    if constexpr (GRAD) {
      if (K * lane < Up) {
        float* dst = rows + (size_t)s * Up * kPl + K * lane;
        float ev[K];
#pragma unroll
        for (int j = 0; j < K; ++j) ev[j] = __builtin_bit_cast(float, Xe[j]);
        st_vec<K>(dst, Xm);
        st_vec<K>(dst + Up, ev);
        if constexpr (MEAN) st_vec<K>(dst + 2 * Up, Mn);
      }
    }
  };
  // the mean of a cell from its two entering terms t1, t2 (f32 at their common exponent) and the
  // means-plus-cost x1, x2 they carry: (t1*x1 + t2*x2) / (t1 + t2); a zero term contributes an
  // exact 0 whatever its x holds, and no term at all gives 0 (both directions)
  auto mean_of = [](float t1, float x1, float t2, float x2, float tt) __attribute__((always_inline)) {
    const float n1 = t1 != 0.0f ? t1 * x1 : 0.0f;
    const float n2 = t2 != 0.0f ? t2 * x2 : 0.0f;
    const float num = n1 + n2;
    return tt != 0.0f ? num / tt : 0.0f;
  };
  if (chain && dir == 0) {
    if (lane == 0) {
      const xf a0 = alpha0<OBS>(lo);
      Xm[0] = a0.m;
      Xe[0] = a0.e;
    }
    store_row(0);
  } else if (chain) {
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (K * lane + j == P - 1) {
        Xm[j] = Et.m;
        Xe[j] = Et.e;
        Mn[j] = ct;
      }
    store_row(S - 1);
  }

  if (loader && NC > 0) {
    issue(0);
    commit(0);
  }
  __syncthreads();
  for (int c = 0; c < NC; ++c) {
    if (loader && c + 1 < NC) issue(c + 1);
    if (chain) {
      const int r0 = chunk_first(c);
      const int n = chunk_count(c);
      const float4* Bf = ltb + (size_t)(c & 1) * bufsz + lane;
      const float2* CB = ccb + (size_t)(c & 1) * bufsz + lane;
      const float2* OB = obb + (size_t)(c & 1) * bufsz + lane;
      if (dir == 0) {
        // alpha[s], abar[s] from row s-1 (the operations of alpha_step, lattice_dev.h, with the two
        // aligned terms kept for the mean)
        for (int i = 0; i < n; ++i) {
          float sm[K], hm[K], xs[K], xh[K];
          int se[K], he[K];
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const float4 t = Bf[i * kRow + j * kKs];
            sm[j] = Xm[j] * t.x;
            se[j] = Xe[j] + __builtin_bit_cast(int, t.y);
            hm[j] = Xm[j] * t.z;
            he[j] = Xe[j] + __builtin_bit_cast(int, t.w);
            if constexpr (MEAN) {
              const float2 cc = CB[i * kRow + j * kKs];
              xs[j] = Mn[j] + cc.x;
              xh[j] = Mn[j] + cc.y;
            }
          }
          const float lm = shr1(hm[K - 1]);
          const int le = shr1(he[K - 1]);
          float lx = 0.0f;
          if constexpr (MEAN) lx = shr1(xh[K - 1]);
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const float xm = (j == 0) ? lm : hm[j > 0 ? j - 1 : 0];
            const int xe = (j == 0) ? le : he[j > 0 ? j - 1 : 0];
            const int em = max(se[j], xe);
            const float t1 = xldexp(sm[j], se[j] - em);
            const float t2 = xldexp(xm, xe - em);
            const float tt = t1 + t2;
            if constexpr (MEAN) {
              const float xx = (j == 0) ? lx : xh[j > 0 ? j - 1 : 0];
              Mn[j] = mean_of(t1, xs[j], t2, xx, tt);
            }
            float sum = tt;
            int ee = em;
            if constexpr (OBS) {
              const float2 o = OB[i * kRow + j * kKs];
              sum = sum * o.x;
              ee = ee + __builtin_bit_cast(int, o.y);
            }
            const xf nv = xf_norm(sum, ee);
            Xm[j] = nv.m;
            Xe[j] = nv.e;
          }
          store_row(r0 + i + 1);
        }
      } else {
        // beta[s], bbar[s] from row s (and beta[s+1], O[s+1]), s = r0+n-1 down to r0; the state is
        // forced to zero at p >= P and the shift out of P-1 is masked
        for (int i = n - 1; i >= 0; --i) {
          float qm[K], bn[K];
          int qe[K];
#pragma unroll
          for (int j = 0; j < K; ++j) {
            qm[j] = Xm[j];
            qe[j] = Xe[j];
            bn[j] = Mn[j];
            if constexpr (OBS) {
              const float2 o = OB[i * kRow + j * kKs];
              qm[j] = qm[j] * o.x;
              qe[j] = qe[j] + __builtin_bit_cast(int, o.y);
            }
          }
          const float rm = shl1(qm[0]);
          const int re = shl1(qe[0]);
          float rx = 0.0f;
          if constexpr (MEAN) rx = shl1(bn[0]);
#pragma unroll
          for (int j = 0; j < K; ++j) {
            const int p = K * lane + j;
            const float ym = (j == K - 1) ? rm : qm[j + 1 < K ? j + 1 : 0];
            const int ye = (j == K - 1) ? re : qe[j + 1 < K ? j + 1 : 0];
            const float4 t = Bf[i * kRow + j * kKs];
            const float u1m = t.x * qm[j];
            const int u1e = __builtin_bit_cast(int, t.y) + qe[j];
            // (the shift out of P-1 is masked, exponent included: what stands at p+1 = P may be
            // anything and must not set the common exponent)
            const bool sh = p < P - 1;
            const float u2m = sh ? t.z * ym : 0.0f;
            const int u2e = sh ? __builtin_bit_cast(int, t.w) + ye : XF_EZERO;
            const int em = max(u1e, u2e);
            const float t1 = xldexp(u1m, u1e - em);
            const float t2 = xldexp(u2m, u2e - em);
            const float tt = t1 + t2;
            float mn = 0.0f;
            if constexpr (MEAN) {
              const float yx = (j == K - 1) ? rx : bn[j + 1 < K ? j + 1 : 0];
              const float2 cc = CB[i * kRow + j * kKs];
              mn = mean_of(t1, bn[j] + cc.x, t2, yx + cc.y, tt);
            }
            const xf nv = xf_norm(tt, em);
            const bool live = p < P;
            Xm[j] = live ? nv.m : 0.0f;
            Xe[j] = live ? nv.e : XF_EZERO;
            Mn[j] = live ? mn : 0.0f;
          }
          store_row(r0 + i);
        }
      }
    }
    if (loader && c + 1 < NC) commit(c + 1);
    __syncthreads();
  }

  // ------------------------------------------------------------------ risk, loss, Z
  if (chain && dir == 0 && my_last) {
    float am = 0.0f, mn = 0.0f;
    int ae = XF_EZERO;
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (K * lane + j == P - 1) {
        am = Xm[j];
        ae = Xe[j];
        mn = Mn[j];
      }
    const xf Z = term ? xf_norm(am * Et.m, ae + Et.e) : xf{am, ae};
    publish(Z, term ? mn + ct : mn);
  }
}

// One thread per cell of a block of step rows; every element of every requested gradient.
template <bool OBS>
__global__ __launch_bounds__(kEcGradThreads) void k_expected_cost_grad(ExpectedCostArgs a, int RB, int nblk, int Up) {
  const int b = blockIdx.x / nblk;
  const int r0 = (blockIdx.x - b * nblk) * RB;
  const int T = a.T, U = a.U;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const size_t TU = (size_t)T * U;
  const float* lt = a.log_trans + (size_t)b * TU * 2;
  const float* cs = a.cost + (size_t)b * TU * 2;
  const float* lo = OBS ? a.log_obs + (size_t)b * TU : nullptr;
  float2* gt = a.grad_trans ? reinterpret_cast<float2*>(a.grad_trans) + (size_t)b * TU : nullptr;
  float2* gc = a.grad_cost ? reinterpret_cast<float2*>(a.grad_cost) + (size_t)b * TU : nullptr;
  float* go = (OBS && a.grad_obs) ? a.grad_obs + (size_t)b * TU : nullptr;
  const float* head = reinterpret_cast<const float*>(a.workspace) + (size_t)b * 4;
  const bool term = (a.flags & SSNT_FLAG_TERMINAL_EMIT) != 0;
  const bool lens = S >= 1 && P >= 1 && S <= T && P <= U && S >= P;
  const float Zm = head[0];
  const int Ze = __builtin_bit_cast(int, head[1]);
  const float risk = head[2];
  const bool ok = lens && Zm != 0.0f;
  const float izm = 1.0f / Zm;
  const int ize = -Ze;
  const float* rowsA = ec_rows_base(a.workspace, a.B) + (size_t)b * T * Up * 3;
  const float* rowsB = rowsA + (size_t)a.B * T * Up * 3;
  const int ncell = min(RB, T - r0) * U;
  for (int cell = threadIdx.x; cell < ncell; cell += kEcGradThreads) {
    const int s = r0 + cell / U;
    const int p = cell % U;
    const size_t idx = (size_t)s * U + p;
    float2 vt = make_float2(0.0f, 0.0f), vc = make_float2(0.0f, 0.0f);
    float vo = 0.0f;
    if (ok && s < S - 1 && p < P) {
      const float* A = rowsA + (size_t)s * Up * 3 + p;
      const float* Bn = rowsB + (size_t)(s + 1) * Up * 3 + p;
      const float am = A[0], an = A[2 * Up];
      const int ae = __builtin_bit_cast(int, A[Up]);
      const float2 x = reinterpret_cast<const float2*>(lt)[idx];
      const float2 c = reinterpret_cast<const float2*>(cs)[idx];
      const bool sh = p < P - 1;
      float Em, Sm;
      int Ee, Se;
      xf_exp_pair(x.x, x.y, true, sh, Em, Ee, Sm, Se);
      // emit: into (s+1, p)
      float qm = Bn[0];
      int qe = __builtin_bit_cast(int, Bn[Up]);
      if constexpr (OBS) {
        const xf o = xf_exp(lo[idx + U], true);
        qm = qm * o.m;
        qe = qe + o.e;
      }
      const float q0 = xldexp(((am * Em) * qm) * izm, ae + Ee + qe + ize);
      vc.x = q0;
      vt.x = q0 != 0.0f ? q0 * (((an + c.x) + Bn[2 * Up]) - risk) : 0.0f;
      // shift: into (s+1, p+1)
      if (sh) {
        float rm = Bn[1];
        int re = __builtin_bit_cast(int, Bn[Up + 1]);
        if constexpr (OBS) {
          const xf o = xf_exp(lo[idx + U + 1], true);
          rm = rm * o.m;
          re = re + o.e;
        }
        const float q1 = xldexp(((am * Sm) * rm) * izm, ae + Se + re + ize);
        vc.y = q1;
        vt.y = q1 != 0.0f ? q1 * (((an + c.y) + Bn[2 * Up + 1]) - risk) : 0.0f;
      }
      if (go) {
        const float* Bs = rowsB + (size_t)s * Up * 3 + p;
        const float post = xldexp((am * Bs[0]) * izm, ae + __builtin_bit_cast(int, Bs[Up]) + ize);
        vo = post != 0.0f ? post * ((an + Bs[2 * Up]) - risk) : 0.0f;
      }
    } else if (ok && term && s == S - 1 && p == P - 1) {
      vc.x = 1.0f;  // the terminal emit is part of every path
    }
    if (gt) gt[idx] = vt;
    if (gc) gc[idx] = vc;
    if (go) go[idx] = vo;
  }
}

template <int K, bool OBS>
int launch_sweep_k(const ExpectedCostArgs& a, const EcLayout& L, bool grad, hipStream_t st) {
  const EcParams q{L.R, ec_upad(a.U > 0 ? a.U : 1), (unsigned)L.base_off};
  if (grad)  // workgroups [0, B) sweep forward, [B, 2B) backward
    return launch_lds(k_expected_cost_sweep<K, OBS, true>, dim3(2 * a.B), dim3(kAlnThreads), L.total, kLdsBudget,
                      st, a, q);
  return launch_lds(k_expected_cost_sweep<K, OBS, false>, dim3(a.B), dim3(kAlnThreads), L.total, kLdsBudget, st,
                    a, q);
}

template <int K, bool OBS>
int launch_ab_sweep_k(const ExpectedCostArgs& a, const EcLayout& L, hipStream_t st) {
  const EcParams q{L.R, ec_upad(a.U > 0 ? a.U : 1), (unsigned)L.base_off};
  return launch_lds(k_expected_cost_sweep<K, OBS, true, false>, dim3(2 * a.B), dim3(kAlnThreads), L.total,
                    kLdsBudget, st, a, q);
}

}  // namespace

size_t alpha_beta_rows_workspace_bytes(int B, int T, int U) {
  return (size_t)B * kEcHeadRec + 16 + 2 * (size_t)B * T * ec_upad(U) * 8;
}

int alpha_beta_chunk_rows(int U, bool obs) { return ec_pick(U > 0 ? U : 1, obs, false).R; }

// The caller has made launch_expected_cost's checks (B, T, U >= 1, U <= 1024, flags, pointers,
// alignment, the 32-bit offsets) and holds a workspace of alpha_beta_rows_workspace_bytes().
int launch_alpha_beta_sweep(const ExpectedCostArgs& a, hipStream_t st) {
  const bool obs = a.log_obs != nullptr;
  const EcLayout L = ec_pick(a.U > 0 ? a.U : 1, obs, false);  // (U == 0: every utterance is infeasible)
  if (L.total > kLdsBudget || a.B > kAlnNoUnit / 2) return SSNT_ERR_UNSUPPORTED;
  return aln_with_k(L.K, [&](auto Kc) {
    constexpr int K = decltype(Kc)::value;
    return obs ? launch_ab_sweep_k<K, true>(a, L, st) : launch_ab_sweep_k<K, false>(a, L, st);
  });
}

size_t expected_cost_workspace_bytes(int B, int T, int U) {
  return (size_t)B * kEcHeadRec + 16 + 2 * ec_rows_bytes(B, T, U);
}

int expected_cost_chunk_rows(int U, bool obs) { return ec_pick(U > 0 ? U : 1, obs).R; }

#ifdef SSNT_AB
static int g_ec_launches = 3;
int set_expected_cost_launches(int mask) {
  if (mask < 1 || mask > 3) return SSNT_ERR_INVALID_ARG;
  g_ec_launches = mask;
  return SSNT_OK;
}
#endif

int launch_expected_cost(const ExpectedCostArgs& a, hipStream_t st) {
#ifdef SSNT_AB
  const int launches = g_ec_launches;  // timing one launch alone (tools/bench_expected_cost.py)
#else
  constexpr int launches = 3;
#endif
  const int rc = aln_check_args(a.B, a.T, a.U, a.flags,
                                a.log_trans && a.cost && a.step_len && a.pos_len && a.risk, a.log_trans,
                                a.log_obs);
  if (rc != SSNT_OK) return rc;
  if (a.grad_obs && !a.log_obs) return SSNT_ERR_INVALID_ARG;
  if (a.B == 0) return SSNT_OK;
  if (!aligned_to(a.cost, 8) || !aligned_to(a.grad_trans, 8) || !aligned_to(a.grad_cost, 8) ||
      !aligned_to(a.grad_obs, 4) || !aligned_to(a.risk, 4) || !aligned_to(a.loss, 4))
    return SSNT_ERR_UNSUPPORTED;
  // the byte offsets of the range-checked loads are 32-bit
  if ((size_t)a.T * a.U * 8 >= (size_t)kAlnNoUnit) return SSNT_ERR_UNSUPPORTED;
  const bool grad = a.grad_trans || a.grad_cost || a.grad_obs;
  if (grad && !aln_workspace_ok(a.workspace, a.workspace_bytes, expected_cost_workspace_bytes(a.B, a.T, a.U)))
    return SSNT_ERR_WORKSPACE;
  const bool obs = a.log_obs != nullptr;
  const int U = a.U > 0 ? a.U : 1;  // (T == 0 or U == 0: every utterance is infeasible)
  const EcLayout L = ec_pick(U, obs);
  if (L.total > kLdsBudget) return SSNT_ERR_UNSUPPORTED;
  // the gradient launch's grid: (utterance, block of RB step rows)
  int RB = kEcGradCells / U;
  RB = RB < 1 ? 1 : RB > a.T ? a.T : RB;
  const int nblk = RB > 0 ? (a.T + RB - 1) / RB : 0;
  if ((size_t)a.B * nblk >= (size_t)kAlnNoUnit || a.B > kAlnNoUnit / 2) return SSNT_ERR_UNSUPPORTED;
  if (launches & 1) {
    const int r = aln_with_k(L.K, [&](auto Kc) {
      constexpr int K = decltype(Kc)::value;
      return obs ? launch_sweep_k<K, true>(a, L, grad, st) : launch_sweep_k<K, false>(a, L, grad, st);
    });
    if (r != SSNT_OK) return r;
  }
  if (!grad || !(launches & 2) || a.T == 0 || a.U == 0) return SSNT_OK;
  const dim3 grid((unsigned)(a.B * nblk));
  if (obs)
    hipLaunchKernelGGL(k_expected_cost_grad<true>, grid, dim3(kEcGradThreads), 0, st, a, RB, nblk, ec_upad(a.U));
  else
    hipLaunchKernelGGL(k_expected_cost_grad<false>, grid, dim3(kEcGradThreads), 0, st, a, RB, nblk, ec_upad(a.U));
  return launch_status();
}

}  // namespace ssnt
