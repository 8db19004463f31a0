// duration_posterior.hip -- the posterior distribution of every position's duration on the
// emit/shift lattice, for gfx950.
//
// Semantics: DESIGN.md 2.10; the kernels: DESIGN.md 5.14. dur_post[b,p,d] = P(d_p = d) for
// d < D-1 and P(d_p >= D-1) in the last bin. Two launches:
//
//   k_expected_cost_sweep<.., MEAN = false>   (expected_cost.hip) alpha and beta in xf form, every
//               row stored (m, e: 8 B per cell and direction), Z and loss.
//   k_duration_posterior    one workgroup = one utterance and a tile of kDpTile consecutive
//               positions, 4 waves. The lattice is swept in absolute steps s, in chunks of kDpRows
//               rows. For a chunk all threads first turn the rows of alpha, beta, log_trans (and
//               log_obs) into four plain-f32 coefficients per cell (a thread per cell, a row's tile
//               in consecutive lanes) and leave them in LDS:
//                   ent   entry(s,p)                 / 2^ea[s][p]
//                   stay  stay(s,p) * 2^ea[s][p]     / 2^ea[s+1][p]
//                   ext   exit(s,p) * 2^ea[s][p]     / Z
//                   tail  beta[s][p] * 2^ea[s][p]    / Z
//               (ea: alpha's exponent; all zero outside the band p <= s <= S-P+p, and all at most
//               about 2 because alpha[s][p] * exit <= Z and so on). Then each wave carries the
//               state F[d] of its four positions through the chunk's steps, d along lanes (W lanes
//               per position, NR consecutive d per lane): F[d] is the mass at (s,p) that has been
//               in p for exactly d steps, as a mantissa against alpha[s][p]'s exponent. A step is
//                   F[1] = ent;  acc[d] += F[d] * (d == D-1 ? tail : ext);  F[d+1] = F[d] * stay
//               the last a one-lane DPP shift. The bin D-1 so collects entry * G(s, D-1) * beta at
//               the step the stay reaches D-1 steps: the tail sum itself, no cumulative state.
//               Two coefficient buffers, one workgroup barrier per chunk; sums in step order, no
//               atomics. Every element of dur_post is written, zeros outside the lattice included.
#include <hip/hip_runtime.h>

#include "align_dev.h"
#include "ec_rows.h"

namespace ssnt {
namespace {

constexpr int kDpThreads = 256;
constexpr int kDpWaves = kDpThreads / 64;
constexpr int kDpWavePos = 4;                      // positions a wave carries
constexpr int kDpTile = kDpWaves * kDpWavePos;     // positions of a workgroup
constexpr int kDpRows = 32;                        // step rows of a chunk
constexpr int kDpCells = kDpRows * kDpTile;        // cells of a chunk (two per thread)

// lanes per position and bins per lane for D bins (bins 1..D-1 live in W * NR slots)
inline void dp_form(int D, int& W, int& NR) {
  const int n = D - 1;
  W = n <= 16 ? 16 : n <= 32 ? 32 : 64;
  NR = n <= 64 ? 1 : n <= 128 ? 2 : 4;
}

// lane l <- lane l-1, lane 0 <- 0 (bound_ctrl: no old value to set up)
__device__ __forceinline__ float dp_shr1(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x138, 0xf, 0xf, true));
}

template <int W, int NR, bool OBS>
__global__ __launch_bounds__(kDpThreads) void k_duration_posterior(DurationPosteriorArgs a, int ntile, int Up) {
  constexpr int kSegs = 64 / W;              // positions side by side in a wave
  constexpr int NP = kDpWavePos / kSegs;     // positions a lane carries, one after the other
  static_assert(kSegs * NP == kDpWavePos, "a wave carries four positions");
  __shared__ float4 coef[2][kDpCells];

  const int b = blockIdx.x / ntile;
  const int p0 = (blockIdx.x - b * ntile) * kDpTile;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int lw = lane & (W - 1);
  const int T = a.T, U = a.U, D = a.D;
  const int S = a.step_len[b];
  const int P = a.pos_len[b];
  const size_t TU = (size_t)T * U;
  const float2* lt = reinterpret_cast<const float2*>(a.log_trans) + (size_t)b * TU;
  const float* lo = OBS ? a.log_obs + (size_t)b * TU : nullptr;
  const float* head = reinterpret_cast<const float*>(a.workspace) + (size_t)b * 4;
  const bool lens = S >= 1 && P >= 1 && S <= T && P <= U && S >= P;
  // (an utterance without a lattice has no rows and a zero Z in its head: nothing but the head is read)
  const float Zm = head[0];
  const int Ze = __builtin_bit_cast(int, head[1]);
  const bool ok = lens && Zm != 0.0f;
  const float* rowsA = ec_rows_base(a.workspace, a.B) + (size_t)b * T * Up * 2;
  const float* rowsB = rowsA + (size_t)a.B * T * Up * 2;

  // the steps this tile sweeps: from the first step of its first position to the last step of its
  // last live one
  const int pe = min(p0 + kDpTile, P);                   // one past the last live position
  const int nsteps = ok && p0 < P ? (S - P + pe) - p0 : 0;
  const int NC = (nsteps + kDpRows - 1) / kDpRows;

  // ------------------------------------------------------------------ coefficients of a chunk
  auto fill = [&](int c) __attribute__((always_inline)) {
    float4* dst = coef[c & 1];
#pragma unroll
    for (int k = 0; k < kDpCells / kDpThreads; ++k) {
      const int cell = tid + k * kDpThreads;
      const int s = p0 + c * kDpRows + cell / kDpTile;
      const int p = p0 + cell % kDpTile;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (p < P && s >= p && s <= S - P + p) {
        const float* A = rowsA + (size_t)s * Up * 2 + p;
        const float* Bs = rowsB + (size_t)s * Up * 2 + p;
        const float am = A[0];
        const int ae = __builtin_bit_cast(int, A[Up]);
        const size_t idx = (size_t)s * U + p;
        if (am != 0.0f) {
          const int ze = ae - Ze;
          const bool sh = p < P - 1;         // (then s <= S-2)
          const bool st = s < S - P + p;     // the stay into (s+1, p) is in the band
          float2 x = make_float2(0.0f, 0.0f);
          if (sh || st) x = lt[idx];
          float Em, Sm;
          int Ee, Se;
          xf_exp_pair(x.x, x.y, st, sh, Em, Ee, Sm, Se);
          // tail: beta[s][p]
          v.w = xldexp(Bs[0] / Zm, __builtin_bit_cast(int, Bs[Up]) + ze);
          // exit: the shift into (s+1, p+1), or the end of the lattice
          if (sh) {
            const float* Bn = rowsB + (size_t)(s + 1) * Up * 2 + p + 1;
            float qm = Sm * Bn[0];
            int qe = Se + __builtin_bit_cast(int, Bn[Up]);
            if constexpr (OBS) {
              const xf o = xf_exp(lo[idx + U + 1], true);
              qm = qm * o.m;
              qe = qe + o.e;
            }
            v.z = xldexp(qm / Zm, qe + ze);
          } else {
            v.z = s == S - 1 ? v.w : 0.0f;
          }
          // stay: the emit into (s+1, p), against alpha[s+1][p]'s exponent
          if (st) {
            const float* An = A + (size_t)Up * 2;
            float gm = Em;
            int ge = Ee;
            if constexpr (OBS) {
              const xf o = xf_exp(lo[idx + U], true);
              gm = gm * o.m;
              ge = ge + o.e;
            }
            v.x = An[0] != 0.0f ? xldexp(gm, ge + ae - __builtin_bit_cast(int, An[Up])) : 0.0f;
          }
          // entry: alpha[s][s] is the entry itself; else the shift out of (s-1, p-1)
          if (s == p) {
            v.y = am;
          } else if (p >= 1) {
            const float* Ap = rowsA + (size_t)(s - 1) * Up * 2 + p - 1;
            const xf h = xf_exp(lt[idx - U - 1].y, true);
            float nm = Ap[0] * h.m;
            int ne = __builtin_bit_cast(int, Ap[Up]) + h.e;
            if constexpr (OBS) {
              const xf o = xf_exp(lo[idx], true);
              nm = nm * o.m;
              ne = ne + o.e;
            }
            v.y = xldexp(nm, ne - ae);
          }
        }
      }
      dst[cell] = v;
    }
  };

  // ------------------------------------------------------------------ the duration state
  float G[NP][NR], acc[NP][NR];
  int wsel[NR];  // the coefficient a bin closes with: 2 ext, 3 tail (bin D-1)
#pragma unroll
  for (int j = 0; j < NR; ++j) wsel[j] = 1 + lw * NR + j == D - 1 ? 3 : 2;
#pragma unroll
  for (int n = 0; n < NP; ++n)
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      G[n][j] = 0.0f;
      acc[n][j] = 0.0f;
    }
  const int t0 = wave * kDpWavePos + (lane / W) * NP;  // this lane's first position in the tile

  if (NC > 0) fill(0);
  __syncthreads();
  for (int c = 0; c < NC; ++c) {
    if (c + 1 < NC) fill(c + 1);
    const float* src = reinterpret_cast<const float*>(coef[c & 1] + t0);
    const int n_rows = min(kDpRows, nsteps - c * kDpRows);
    for (int i = 0; i < n_rows; ++i) {
#pragma unroll
      for (int n = 0; n < NP; ++n) {
        // (stay, ent) for every lane; ext or tail by the lane's own address: two addresses per
        // read, which LDS broadcasts, instead of a select per bin
        const float* q = src + (i * kDpTile + n) * 4;
        const float2 se = *reinterpret_cast<const float2*>(q);
        float g[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
          const float f = (j == 0 && lw == 0) ? se.y : G[n][j];
          acc[n][j] = acc[n][j] + f * q[wsel[j]];
          g[j] = f * se.x;
        }
        G[n][0] = dp_shr1(g[NR - 1]);
#pragma unroll
        for (int j = 1; j < NR; ++j) G[n][j] = g[j - 1];
      }
    }
    __syncthreads();
  }

  // ------------------------------------------------------------------ every bin of the tile's rows
#pragma unroll
  for (int n = 0; n < NP; ++n) {
    const int p = p0 + t0 + n;
    if (p < U) {
      float* dst = a.dur_post + ((size_t)b * U + p) * D;
      const bool live = ok && p < P;
      if (lw == 0) dst[0] = 0.0f;
#pragma unroll
      for (int j = 0; j < NR; ++j) {
        const int d = 1 + lw * NR + j;
        if (d < D) dst[d] = live ? acc[n][j] : 0.0f;
      }
    }
  }
}

template <int W, int NR>
int launch_dp(const DurationPosteriorArgs& a, hipStream_t st) {
  const int ntile = (a.U + kDpTile - 1) / kDpTile;
  const dim3 grid((unsigned)(a.B * ntile));
  if (a.log_obs)
    hipLaunchKernelGGL((k_duration_posterior<W, NR, true>), grid, dim3(kDpThreads), 0, st, a, ntile, ec_upad(a.U));
  else
    hipLaunchKernelGGL((k_duration_posterior<W, NR, false>), grid, dim3(kDpThreads), 0, st, a, ntile, ec_upad(a.U));
  return launch_status();
}

}  // namespace

size_t duration_posterior_workspace_bytes(int B, int T, int U, int D) {
  (void)D;  // the duration state lives in registers
  return alpha_beta_rows_workspace_bytes(B, T, U);
}

#ifdef SSNT_AB
static int g_dp_launches = 3;
int set_duration_posterior_launches(int mask) {
  if (mask < 1 || mask > 3) return SSNT_ERR_INVALID_ARG;
  g_dp_launches = mask;
  return SSNT_OK;
}
int duration_posterior_block(int U, int D, bool obs) {
  (void)U; (void)D; (void)obs;  // one form for every shape
  return kDpRows | (kDpTile << 16);
}
#endif

int launch_duration_posterior(const DurationPosteriorArgs& a, hipStream_t st) {
#ifdef SSNT_AB
  const int launches = g_dp_launches;  // timing one launch alone (tools/bench_duration_posterior.py)
#else
  constexpr int launches = 3;
#endif
  if (a.D < 2 || a.D > 256) return SSNT_ERR_INVALID_ARG;
  const int rc = aln_check_args(a.B, a.T, a.U, a.flags, a.log_trans && a.step_len && a.pos_len && a.dur_post,
                                a.log_trans, a.log_obs);
  if (rc != SSNT_OK) return rc;
  if (a.B == 0) return SSNT_OK;
  if (!aligned_to(a.dur_post, 4) || !aligned_to(a.loss, 4)) return SSNT_ERR_UNSUPPORTED;
  // the byte offsets of the range-checked loads are 32-bit
  if ((size_t)a.T * a.U * 8 >= (size_t)kAlnNoUnit) return SSNT_ERR_UNSUPPORTED;
  const int ntile = (a.U + kDpTile - 1) / kDpTile;
  if ((size_t)a.B * ntile >= (size_t)kAlnNoUnit || a.B > kAlnNoUnit / 2) return SSNT_ERR_UNSUPPORTED;
  if (!aln_workspace_ok(a.workspace, a.workspace_bytes, duration_posterior_workspace_bytes(a.B, a.T, a.U, a.D)))
    return SSNT_ERR_WORKSPACE;
  if (launches & 1) {
    ExpectedCostArgs e{};
    e.log_trans = a.log_trans; e.log_obs = a.log_obs; e.step_len = a.step_len; e.pos_len = a.pos_len;
    e.B = a.B; e.T = a.T; e.U = a.U; e.flags = a.flags; e.loss = a.loss;
    e.workspace = a.workspace; e.workspace_bytes = a.workspace_bytes; e.status = a.status;
    const int r = launch_alpha_beta_sweep(e, st);
    if (r != SSNT_OK) return r;
  }
  if (!(launches & 2) || a.U == 0) return SSNT_OK;  // (U == 0: dur_post has no element)
  int W, NR;
  dp_form(a.D, W, NR);
  if (NR == 4) return launch_dp<64, 4>(a, st);
  if (NR == 2) return launch_dp<64, 2>(a, st);
  if (W == 64) return launch_dp<64, 1>(a, st);
  if (W == 32) return launch_dp<32, 1>(a, st);
  return launch_dp<16, 1>(a, st);
}

}  // namespace ssnt
