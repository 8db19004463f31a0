// v2_fwd_bwd.hip -- F4: the v2 duration-class (semi-Markov) forward-backward for gfx950.
//
// The training-side counterpart of the v2 decode (not in the reference). The
// lattice, its move rules (src/v2.rs:94-166) and the split-exponent arithmetic are defined in
// oracle/ssnt_oracle.c ("F4") and DESIGN.md "Duration lattice"; this kernel reproduces that
// definition bit for bit.
//
// Layout. alpha does not depend on beta or the other way round, so the two sweeps run at the
// same time: launch 1 has one workgroup (512 threads, 8 waves) per (utterance, direction).
// State rows r = 0..I (input steps consumed) over totals x; only the window of row r
// (f4_window: the v2 band, or [0, r*dmax] in test mode) can hold mass, so rows are stored
// window-relative, Wcap xf wide:
//   LDS:  duration table | class weights (xf, chunks of 64 steps, double-buffered) | 2 row
//         buffers (ping-pong), each with kF4Pad zero cells on both sides of its window
//   HBM:  alpha and beta rows 0..I of every utterance (workspace), Z per utterance.
// A sweep step: each thread owns cells x = lo + tid (+512 ...) and sums its D class terms
// (exponent max, then the ldexp-aligned f32 sum in class order; the class loop is unrolled for
// D <= 64, the step's weights read into registers once); one barrier per step. With the zero
// cells around every window, a term's LDS address is one subtraction from its cell's (the
// clamp to the window happens once per cell, not per term). Class log-probs are loaded a
// chunk ahead and converted into LDS half a chunk later, so no global load and no exp sits on
// the I-step dependency chain. The forward workgroup also forms Z (lane partials x mod 64 +
// butterfly) and the loss.
// Launch 2 (one workgroup per (utterance, step)): the gradients of step t -- class i on wave
// i % 4, every class of a wave accumulated in one pass over the destination totals (lane
// partial x mod 64, the oracle's order), one butterfly per class (DPP quad/mirror moves, a
// swizzle, one bpermute) -- and the debug beta row. Fully parallel (B * I workgroups).
// launch_v2_fwd_only runs the forward workgroups of launch 1 alone (alpha rows and Z, no loss, into
// a workspace without the beta rows): the forward filter of v2_sample_align.hip.
// The device code of both launches (f4_cell, f4_sweep, k_f4_grad, the butterflies) and f4_plan live
// in v2_lattice_dev.h, where v2_expected_cost.hip instantiates them with a mean beside every cell.
#include <hip/hip_runtime.h>

#include "buffer_ops.h"
#include "launch_util.h"
#include "ssnt_internal.h"
#include "v2_lattice_dev.h"
#include "xf_math.h"

namespace ssnt {
namespace {

template <int DC>
__global__ __launch_bounds__(kF4Threads) void k_f4_sweep(V2FwdBwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x;
  const bool fwd = blockIdx.y == 0;
  const int tid = threadIdx.x;
  int* dur = reinterpret_cast<int*>(smem);
  for (int i = tid; i < DC; i += kF4Threads) dur[i] = i < a.D ? a.table[i] : 0;
  lds_sync();
  F4Utt u;
  if (!f4_setup(a, b, dur, u, fwd)) {
    if (fwd) {
      const float inf_loss = (a.flags & SSNT_FLAG_ZERO_INFINITY) ? 0.0f : __builtin_inff();
      if (tid == 0 && a.loss) a.loss[b] = inf_loss;
      if (a.log_alpha)
        for (int r = 0; r <= a.Imax; ++r)
          f4_log_row(a.log_alpha + b * (size_t)(a.Imax + 1) * a.X + (size_t)r * a.X, nullptr, 0, -1, a.X);
    }
    return;
  }
  const bool padded = u.dmax <= kF4Pad;  // (uniform)
  if (fwd) {
    if (padded) f4_sweep<DC, true, true>(a, smem, u, u.dmax);
    else f4_sweep<DC, true, false>(a, smem, u, u.dmax);
  } else {
    if (padded) f4_sweep<DC, false, true>(a, smem, u, u.dmax);
    else f4_sweep<DC, false, false>(a, smem, u, u.dmax);
  }
}

// (the gradient kernel, k_f4_grad, is in v2_lattice_dev.h)

}  // namespace

size_t v2_fwd_bwd_workspace_bytes(int B, int Imax, int max_total, bool test_mode) {
  if (B <= 0 || Imax <= 0 || max_total < 0) return 0;
  return (2 * (size_t)B * (Imax + 1) * v2_fwd_bwd_wcap(max_total, test_mode) + B) * sizeof(xf);
}

size_t v2_fwd_only_workspace_bytes(int B, int Imax, int max_total, bool test_mode) {
  if (B <= 0 || Imax <= 0 || max_total < 0) return 0;
  return ((size_t)B * (Imax + 1) * v2_fwd_bwd_wcap(max_total, test_mode) + B) * sizeof(xf);
}

// the sweep launch: both directions, or (fwd_only) the alpha workgroups alone -- blockIdx.y == 0
template <int DC>
int launch_f4(const V2FwdBwdArgs& a, size_t lds, size_t glds, hipStream_t st) {
  // (each launch raises its own attribute to what it asks for)
  const int rc = launch_lds(k_f4_sweep<DC>, dim3(a.B, a.fwd_only ? 1 : 2), dim3(kF4Threads), lds, lds, st, a);
  if (rc != SSNT_OK || a.fwd_only || (!a.grad && !a.log_beta)) return rc;
  return launch_lds(k_f4_grad<DC>, dim3(a.B, a.Imax + 1), dim3(f4_grad_threads<DC>()), glds, glds, st, a,
                    F4NoMean{});
}

namespace {
int f4_dispatch(const V2FwdBwdArgs& a, size_t lds, size_t glds, hipStream_t st) {
  if (a.D <= 8) return launch_f4<8>(a, lds, glds, st);
  if (a.D <= 16) return launch_f4<16>(a, lds, glds, st);
  if (a.D <= 32) return launch_f4<32>(a, lds, glds, st);
  return launch_f4<64>(a, lds, glds, st);
}
}  // namespace

int launch_v2_fwd_bwd(const V2FwdBwdArgs& in, hipStream_t st) {
  V2FwdBwdArgs a = in;
  a.fwd_only = false;
  size_t lds = 0, glds = 0;
  const int rc = f4_plan(a, true, lds, glds);
  if (rc != SSNT_OK || a.B == 0) return rc;
  if (!a.workspace || a.workspace_bytes < v2_fwd_bwd_workspace_bytes(a.B, a.Imax, a.X - 1, a.test_mode))
    return SSNT_ERR_WORKSPACE;
  return f4_dispatch(a, lds, glds, st);
}

int launch_v2_fwd_only(const V2FwdBwdArgs& in, bool launch, hipStream_t st) {
  V2FwdBwdArgs a = in;
  a.fwd_only = true;
  a.grad = nullptr;
  a.log_alpha = a.log_beta = nullptr;
  size_t lds = 0, glds = 0;
  const int rc = f4_plan(a, false, lds, glds);
  if (rc != SSNT_OK || a.B == 0) return rc;
  if (!a.workspace || a.workspace_bytes < v2_fwd_only_workspace_bytes(a.B, a.Imax, a.X - 1, a.test_mode))
    return SSNT_ERR_WORKSPACE;
  return launch ? f4_dispatch(a, lds, glds, st) : SSNT_OK;
}

}  // namespace ssnt
