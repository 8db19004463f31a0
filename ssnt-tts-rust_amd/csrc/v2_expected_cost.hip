// v2_expected_cost.hip -- the expected cost of a duration path under the posterior of the v2
// duration-class lattice (the expectation semiring on F4's lattice) and its gradients, for gfx950.
//
// Semantics: DESIGN.md 2.9; the kernels: DESIGN.md 5.13. risk = E[sum_t cost[t, class_t]];
// grad_cost is the class posterior q (= -grad of v2_fwd_bwd, to the bit), grad_logits the
// covariance sum_x q(t,x,i) (abar[t][x] + cost[t,i] + bbar[t+1][x + d_i] - risk). Both launches
// are F4's (v2_lattice_dev.h) with MEAN set:
//
//   k_v2ec_sweep   one 512-thread workgroup per (utterance, direction): F4's sweep, every cell with
//               the mean cost of the paths through it, a plain f32, beside its xf value (form (a) of
//               the D terms at their common exponent, one division per cell). The
//               step's class costs are staged with the class log-probs, a chunk ahead, so no global
//               load sits on the step chain. The forward workgroup forms Z, the loss and risk.
//               Value only (both gradients null): the forward workgroups alone, no row stored, no
//               workspace touched; the same instructions on the chain, so the same bits.
//   k_f4_grad<DC, true>  (v2_lattice_dev.h) one workgroup per (utterance, step): F4's lane
//               partials and transposed butterfly per class, twice -- the posterior sum and the
//               signed covariance sum.
//
// Workspace (gradients only): F4's (alpha rows | beta rows | Z) | abar rows | bbar rows | risk,
// rows as [B][Imax+1][Wcap], the mean rows f32.
#include <hip/hip_runtime.h>

#include "buffer_ops.h"
#include "launch_util.h"
#include "ssnt_internal.h"
#include "v2_lattice_dev.h"
#include "xf_math.h"

namespace ssnt {
namespace {

// MEAN: 1 both directions, rows stored; 2 the forward direction alone, nothing stored
template <int DC, int MEAN>
__global__ __launch_bounds__(kF4Threads) void k_v2ec_sweep(V2FwdBwdArgs a, F4Mean mn) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const bool fwd = blockIdx.y == 0;
  const int tid = threadIdx.x;
  int* dur = reinterpret_cast<int*>(smem);
  for (int i = tid; i < DC; i += kF4Threads) dur[i] = i < a.D ? a.table[i] : 0;
  lds_sync();
  F4Utt u;
  if (!f4_setup(a, b, dur, u, fwd)) {
    if (fwd && tid == 0) {
      mn.risk[b] = 0.0f;
      if (a.loss) a.loss[b] = __builtin_inff();
    }
    return;
  }
  const bool padded = u.dmax <= kF4Pad;  // (uniform)
  if (fwd) {
    if (padded) f4_sweep<DC, true, true, MEAN>(a, smem, u, u.dmax, mn);
    else f4_sweep<DC, true, false, MEAN>(a, smem, u, u.dmax, mn);
  } else if constexpr (MEAN == 1) {
    if (padded) f4_sweep<DC, false, true, MEAN>(a, smem, u, u.dmax, mn);
    else f4_sweep<DC, false, false, MEAN>(a, smem, u, u.dmax, mn);
  }
}

// bytes of F4's part of the workspace (a multiple of 8) and of one direction's mean rows
size_t ec_f4_bytes(int B, int Imax, int max_total, bool test_mode) {
  return (2 * (size_t)B * (Imax + 1) * v2_fwd_bwd_wcap(max_total, test_mode) + B) * sizeof(xf);
}
size_t ec_mean_bytes(int B, int Imax, int max_total, bool test_mode) {
  return (size_t)B * (Imax + 1) * v2_fwd_bwd_wcap(max_total, test_mode) * sizeof(float);
}

#ifdef SSNT_AB
int g_v2ec_launches = 3;
#endif

template <int DC>
int launch_v2ec(const V2FwdBwdArgs& a, const F4Mean& mn, bool grad, size_t lds, size_t glds, hipStream_t st) {
#ifdef SSNT_AB
  const int launches = g_v2ec_launches;  // timing one launch alone (tools/bench_v2_expected_cost.py)
#else
  constexpr int launches = 3;
#endif
  if (!grad) return launch_lds(k_v2ec_sweep<DC, 2>, dim3(a.B, 1), dim3(kF4Threads), lds, lds, st, a, mn);
  if (launches & 1) {
    const int rc = launch_lds(k_v2ec_sweep<DC, 1>, dim3(a.B, 2), dim3(kF4Threads), lds, lds, st, a, mn);
    if (rc != SSNT_OK) return rc;
  }
  if (!(launches & 2)) return SSNT_OK;
  return launch_lds(k_f4_grad<DC, true, F4Mean>, dim3(a.B, a.Imax), dim3(f4_grad_threads<DC>()), glds, glds, st, a,
                    mn);
}

// f(the class-count instantiation DC that D classes run on)
template <typename F>
int ec_with_dc(int D, F&& f) {
  if (D <= 8) return f(std::integral_constant<int, 8>{});
  if (D <= 16) return f(std::integral_constant<int, 16>{});
  if (D <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

}  // namespace

size_t v2_expected_cost_workspace_bytes(int B, int Imax, int max_total, bool test_mode, bool need_grad) {
  if (B <= 0 || Imax <= 0 || max_total < 0 || !need_grad) return 0;
  return ec_f4_bytes(B, Imax, max_total, test_mode) + 2 * ec_mean_bytes(B, Imax, max_total, test_mode) +
         (((size_t)B * sizeof(float) + 7) & ~(size_t)7);
}

#ifdef SSNT_AB
int set_v2_expected_cost_launches(int mask) {
  if (mask < 1 || mask > 3) return SSNT_ERR_INVALID_ARG;
  g_v2ec_launches = mask;
  return SSNT_OK;
}
#endif

int launch_v2_expected_cost(const V2ExpectedCostArgs& in, hipStream_t st) {
  V2FwdBwdArgs a = v2_fwd_bwd_args_of(in);
  a.loss = in.loss; a.grad = in.grad_cost;
  if (!in.cost || !in.risk) return SSNT_ERR_INVALID_ARG;
  size_t lds = 0, glds = 0;
  const int rc = f4_plan(a, false, lds, glds, true);
  if (rc != SSNT_OK || a.B == 0) return rc;
  const bool grad = in.grad_logits || in.grad_cost;
  F4Mean mn{};
  mn.cost = in.cost; mn.risk = in.risk; mn.grad_logits = in.grad_logits;
  if (grad) {
    const size_t need = v2_expected_cost_workspace_bytes(a.B, a.Imax, a.X - 1, a.test_mode, true);
    if (!a.workspace || a.workspace_bytes < need || !aligned_to(a.workspace, 8)) return SSNT_ERR_WORKSPACE;
    unsigned char* base = static_cast<unsigned char*>(a.workspace);
    const size_t f4b = ec_f4_bytes(a.B, a.Imax, a.X - 1, a.test_mode);
    const size_t mb = ec_mean_bytes(a.B, a.Imax, a.X - 1, a.test_mode);
    mn.abar = reinterpret_cast<float*>(base + f4b);
    mn.bbar = reinterpret_cast<float*>(base + f4b + mb);
    mn.ws_risk = reinterpret_cast<float*>(base + f4b + 2 * mb);
  } else {
    glds = 0;
  }
  return ec_with_dc(a.D, [&](auto dc) { return launch_v2ec<decltype(dc)::value>(a, mn, grad, lds, glds, st); });
}

#ifdef SSNT_AB
// the staging depth of the sweep instance a call with D classes launches
int v2_expected_cost_chunk_steps(int D) {
  return ec_with_dc(D, [](auto dc) { return f4_chunk<decltype(dc)::value>(); });
}
#endif

}  // namespace ssnt
