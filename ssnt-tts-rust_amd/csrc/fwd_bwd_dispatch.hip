// fwd_bwd_dispatch.hip -- host side of the lattice forward-backward: which of the three kernels
// a call runs (fwd_bwd_stream.hip, fwd_bwd_wide.hip, fwd_bwd.hip), the one workspace size that
// serves them all, the batch loss sum as a pass of its own, and the float64 debug outputs.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "lattice_dev.h"
#include "launch_util.h"

namespace ssnt {
namespace {

// Kernel choice. The product dispatches by shape only (the streaming kernel, else the segmented
// kernel, else the two-wave kernel). The A/B build (-DSSNT_AB, `make lib-ab`; tests and tools
// only) adds a process-wide override: 1 two-wave kernel only, 2 segmented kernel;
// SSNT_FWD_BWD_KERNEL=simple selects 1 there. (The pair and rows kernels of rounds 2-4, both
// bit-exact and measured slower -- DESIGN.md 5.1a / 5.1c -- were retired to git history.)
#ifdef SSNT_AB
std::atomic<int> g_variant{0};
std::once_flag g_variant_env;
int variant() {
  std::call_once(g_variant_env, [] {
    const char* e = getenv("SSNT_FWD_BWD_KERNEL");
    if (e && strcmp(e, "simple") == 0) g_variant.store(1);
  });
  return g_variant.load(std::memory_order_relaxed);
}
#else
constexpr int variant() { return 0; }
#endif

thread_local char t_dispatch[160];

}  // namespace

void note_fwd_bwd_dispatch(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(t_dispatch, sizeof t_dispatch, fmt, ap);
  va_end(ap);
}
const char* last_fwd_bwd_dispatch() { return t_dispatch; }

size_t fwd_bwd_workspace_bytes(int B, int T, int U) {
  // 0 when the plans the launchers themselves run keep every row in LDS: the streaming kernel's
  // with and without log_obs, and the two-wave kernel's. (A/B forced kernels: always a workspace.)
  if (variant() == 0) {
    const RowsPlan s0 = stream_plan(B, T, U, false), s1 = stream_plan(B, T, U, true);
    const RowsPlan tw = simple_plan(T, U);
    if (s0.supported && s0.lds && s1.supported && s1.lds && tw.supported && tw.lds) return 0;
  }
  // the segmented kernel keeps its rows (plus beta at the cut) in the workspace at every T; one size
  // serves every kernel (two-wave: B*T*U xf; streaming, rows padded to lane slices: U + 3 at most)
  const size_t wide = fwd_bwd_wide_workspace_bytes(B, T, U);
  const size_t stream = (size_t)B * T * ((size_t)U + 3) * sizeof(xf);
  return wide > stream ? wide : stream;
}

#ifdef SSNT_AB
int set_fwd_bwd_variant(int v) {
  // 0 default dispatch, 1 two-wave kernel, 2 segmented kernel at every U it takes
  if (v < 0 || v > 2) return SSNT_ERR_INVALID_ARG;
  variant();  // the environment is read once, before any explicit choice
  g_variant.store(v);
  return SSNT_OK;
}
#endif

namespace {
__global__ __launch_bounds__(64) void k_loss_sum(const float* loss, int B, float* out) {
  const float sum = wave_loss_sum(loss, B);
  if (threadIdx.x == 0) *out = sum;
}

int launch_variant(const FwdBwdArgs& a, hipStream_t st, bool& summed) {
  summed = false;
  if (variant() == 0) {
    FwdBwdArgs x = a;
    if (!a.sum_state) x.loss_sum = nullptr;
    int rc = launch_fwd_bwd_stream(x, st);
    summed = x.loss_sum != nullptr;
    if (rc != SSNT_ERR_UNSUPPORTED) return rc;
    summed = false;
    // long rows, and what the streaming kernel declines (4-byte-aligned log_trans / grad): the
    // segmented kernel takes any U <= 1024 at 8-byte alignment (loss sum: the separate pass)
    if (a.workspace && a.workspace_bytes >= fwd_bwd_wide_workspace_bytes(a.B, a.T, a.U)) {
      rc = launch_fwd_bwd_wide(a, st, true);
      if (rc != SSNT_ERR_UNSUPPORTED) return rc;
    }
  } else if (variant() == 2) {
    const int rc = launch_fwd_bwd_wide(a, st, true);
    if (rc != SSNT_ERR_UNSUPPORTED) return rc;
  }
  FwdBwdArgs x = a;
  x.loss_sum = nullptr;  // the two-wave kernel only writes loss[]
  return launch_fwd_bwd_simple(x, st);
}
}  // namespace

// ---- float64 debug outputs (ssnt_fwd_bwd_debug64_device) -------------------------------------
// The kernels run in raw-state mode: mantissa / exponent planes of alpha and beta and Z per
// utterance land in the workspace; this pass forms e*ln2 + ln(m) in float64 (zero mantissa:
// -inf; loss: -ln Z, or the f32 kernel's +inf / 0 where Z was never formed or is 0).
__global__ __launch_bounds__(256) void k_debug64(const float* am, const int* ae, const float* bm,
                                                 const int* be, size_t n, double* la, double* lb,
                                                 const float* zs, const float* loss32, int B,
                                                 double* loss) {
  constexpr double kLn2 = 0x1.62e42fefa39efp-1;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (la) la[i] = am[i] == 0.0f ? -__builtin_inf() : (double)ae[i] * kLn2 + log((double)am[i]);
    if (lb) lb[i] = bm[i] == 0.0f ? -__builtin_inf() : (double)be[i] * kLn2 + log((double)bm[i]);
  }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)B; i += stride) {
    const float zm = zs[2 * i];
    const int ze = __builtin_bit_cast(int, zs[2 * i + 1]);
    loss[i] = zm == 0.0f ? (double)loss32[i] : -((double)ze * kLn2 + log((double)zm));
  }
}

static inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

size_t fwd_bwd_debug64_workspace_bytes(int B, int T, int U) {
  const size_t cells = (size_t)B * T * U;
  return al256(fwd_bwd_workspace_bytes(B, T, U)) + 4 * al256(cells * 4) + al256((size_t)B * 8) +
         al256((size_t)B * 4);
}

int launch_fwd_bwd_debug64(const FwdBwdArgs& a0, double* loss64, double* la64, double* lb64,
                           hipStream_t st) {
  if (a0.B < 0 || a0.T <= 0 || a0.U <= 0 || !loss64 || a0.loss_sum) return SSNT_ERR_INVALID_ARG;
  if (a0.B == 0) return SSNT_OK;
  const size_t need = fwd_bwd_debug64_workspace_bytes(a0.B, a0.T, a0.U);
  if (!a0.workspace || a0.workspace_bytes < need) return SSNT_ERR_WORKSPACE;
  const size_t cells = (size_t)a0.B * a0.T * a0.U;
  const size_t base = fwd_bwd_workspace_bytes(a0.B, a0.T, a0.U);
  unsigned char* w = static_cast<unsigned char*>(a0.workspace);
  size_t off = al256(base);
  auto take = [&](size_t bytes) { unsigned char* p = w + off; off += al256(bytes); return p; };
  float* am = reinterpret_cast<float*>(take(cells * 4));
  int* ae = reinterpret_cast<int*>(take(cells * 4));
  float* bm = reinterpret_cast<float*>(take(cells * 4));
  int* be = reinterpret_cast<int*>(take(cells * 4));
  float* zs = reinterpret_cast<float*>(take((size_t)a0.B * 8));
  float* l32 = reinterpret_cast<float*>(take((size_t)a0.B * 4));
  FwdBwdArgs a = a0;
  a.workspace = base ? a0.workspace : nullptr;  // the product dispatch sees the plain call's workspace
  a.workspace_bytes = base;
  a.loss = l32;
  a.log_alpha = am;
  a.log_beta = bm;
  a.log_alpha_e = ae;
  a.log_beta_e = be;
  a.z_state = zs;
  if (hipMemsetAsync(zs, 0, (size_t)a.B * 8, st) != hipSuccess) return SSNT_ERR_HIP;
  int rc = launch_fwd_bwd(a, st);
  if (rc != SSNT_OK) return rc;
  const size_t n = la64 || lb64 ? cells : 0;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 + 1 : 4096);
  hipLaunchKernelGGL(k_debug64, dim3(blocks), dim3(256), 0, st, am, ae, bm, be, n, la64, lb64, zs,
                     l32, a.B, loss64);
  return launch_status();
}

size_t fwd_bwd_sum_state_bytes(int B) { return kSumGranuleOffset + 8 * (size_t)(B > 0 ? B : 0); }

int launch_fwd_bwd(const FwdBwdArgs& a, hipStream_t st) {
  t_dispatch[0] = 0;  // (an argument error or an empty batch dispatches nothing)
  if (a.B < 0 || a.T <= 0 || a.U <= 0 || !a.log_trans || !a.step_len || !a.pos_len || !a.loss)
    return SSNT_ERR_INVALID_ARG;
  if (a.grad_obs && !a.log_obs) return SSNT_ERR_INVALID_ARG;
  if (a.B == 0) {
    if (a.loss_sum) return hipMemsetAsync(a.loss_sum, 0, sizeof(float), st) == hipSuccess ? SSNT_OK : SSNT_ERR_HIP;
    return SSNT_OK;
  }
  // batch loss sum: inside the streaming kernel when the caller gives a sum state, else one
  // extra single-wave pass over loss[] (same fixed order, same bits)
  bool summed = false;
  const int rc = launch_variant(a, st, summed);
  if (rc != SSNT_OK || !a.loss_sum || summed) return rc;
  const size_t n = strlen(t_dispatch);
  snprintf(t_dispatch + n, sizeof t_dispatch - n, "+k_loss_sum");
  hipLaunchKernelGGL(k_loss_sum, dim3(1), dim3(64), 0, st, a.loss, a.B, a.loss_sum);
  return launch_status();
}

}  // namespace ssnt
