// ssnt_internal.h -- launchers shared between the kernel files (fwd_bwd*.hip, v2_*.hip, viterbi.hip,
// sample_align.hip, decode.hip, fused_decode.hip) and the C-ABI host layer (capi.hip). Not part of the public interface (that is include/ssnt_tts_c.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ssnt_tts_c.h"

namespace ssnt {

// device status word bits (OR-ed by kernels, read by the host layer)
constexpr int kStatusNoCandidate = 1 << 0;       // v2: no duration sequence fits (src/v2.rs:292)
constexpr int kStatusDurationMismatch = 1 << 1;  // upsample: sum(d) != output_length (src/v2_util.rs:58)
constexpr int kStatusBadLength = 1 << 2;         // fwd-bwd: step/pos length outside the tensor
constexpr int kStatusBadIndex = 1 << 3;          // backtrace: branch index outside [0, W)
constexpr int kStatusTimeout = 1 << 4;           // fwd-bwd: an intra-workgroup wait hit its bound
constexpr int kStatusRingTag = 1 << 5;           // diagnostic builds only: a ring slot / row held another row
constexpr int kStatusBadBand = 1 << 6;           // banded fwd-bwd: band_start is not a valid band

int status_bits_to_code(int bits);

// ---- lattice forward-backward (fwd_bwd_dispatch.hip: entry, kernel choice, workspace) ----
struct FwdBwdArgs {
  const float* log_trans;  // (B,T,U,2)
  const float* log_obs;    // (B,T,U) or null
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  int B, T, U, flags;
  float* loss;       // (B)
  float* grad;       // (B,T,U,2) or null
  float* grad_obs;   // (B,T,U) or null (requires log_obs)
  float* log_alpha;  // (B,T,U) or null
  float* log_beta;   // (B,T,U) or null
  void* workspace;   // row storage when the rows do not fit LDS
  size_t workspace_bytes;
  int* status;  // device status word or null
  float* loss_sum;   // fixed-order sum of loss[0..B) or null
  void* sum_state;   // in-launch sum state (lattice_dev.h; zero before the first call) or null
  // raw-state debug mode (ssnt_fwd_bwd_debug64_device): with log_alpha_e / log_beta_e set, the
  // debug rows log_alpha / log_beta receive the normalized split-exponent mantissas (0 outside
  // the lattice) and these planes the exponents, (B,T,U); z_state (B x {m, e bits}) receives Z
  int* log_alpha_e;
  int* log_beta_e;
  float* z_state;
};
size_t fwd_bwd_workspace_bytes(int B, int T, int U);
// float64 debug outputs (ssnt_fwd_bwd_debug64_device): workspace bytes and the launch, which runs
// the product dispatch in raw-state mode and then forms e*ln2 + ln(m) in float64 on the GPU
size_t fwd_bwd_debug64_workspace_bytes(int B, int T, int U);
int launch_fwd_bwd_debug64(const FwdBwdArgs& a, double* loss64, double* log_alpha64,
                           double* log_beta64, hipStream_t stream);
size_t fwd_bwd_sum_state_bytes(int B);  // 64 + 8 B
int launch_fwd_bwd(const FwdBwdArgs& a, hipStream_t stream);
// positions per lane of the one-wave-per-row kernels: 1, 2, 4, 8 up to U = 64, 128, 256, 512; else 0
inline int lanes_for(int U) { return U <= 64 ? 1 : U <= 128 ? 2 : U <= 256 ? 4 : U <= 512 ? 8 : 0; }
// What a rows-in-LDS-or-workspace kernel decides from the shape alone (launcher and query share it)
struct RowsPlan {
  bool supported, lds;  // the kernel takes this shape; its rows fit LDS (else: the workspace)
  int K;                // positions per lane
  size_t shm_bytes, workspace_bytes;  // dynamic LDS of the launch; rows in the workspace (0 when lds)
};
RowsPlan stream_plan(int B, int T, int U, bool obs);  // fwd_bwd_stream.hip (rows padded to whole lane slices)
RowsPlan simple_plan(int T, int U);  // fwd_bwd.hip (workspace_bytes unset: the query's size)
// streaming kernel (fwd_bwd_stream.hip): SSNT_ERR_UNSUPPORTED for shapes it does not take
int launch_fwd_bwd_stream(const FwdBwdArgs& a, hipStream_t stream);
// two-wave fallback (fwd_bwd.hip): U <= 512, any alignment; writes loss[] only (no loss_sum)
int launch_fwd_bwd_simple(const FwdBwdArgs& a, hipStream_t stream);
// segmented kernel (fwd_bwd_wide.hip): long rows (256 < U <= 1024), or any U <= 1024 when
// any_u; SSNT_ERR_UNSUPPORTED for other shapes
int launch_fwd_bwd_wide(const FwdBwdArgs& a, hipStream_t stream, bool any_u);
size_t fwd_bwd_wide_workspace_bytes(int B, int T, int U);
// Process-wide A/B knobs and the kernels only they reach: the A/B build (-DSSNT_AB, `make
// lib-ab`, lib/ab/libssnt_tts_c_ab.so; tests and tools) only. The product dispatches by shape.
#ifdef SSNT_AB
int set_fwd_bwd_variant(int v);
int set_fwd_bwd_wide_lanes(int k);  // positions per lane of the long-row kernel (1 or 2)
int set_fwd_bwd_wide_split(int mode);  // two workgroups per direction (-1 auto, 0 off, 1 on)
int set_fwd_bwd_wide_lag(int sleeps);  // split form: downstream wave 0 idles per block (race test)
#endif
int diag_read(void* host, size_t bytes);  // -DSSNT_DIAG builds only (tools/diag_fwd_bwd.py)
// the fwd-bwd kernel instance this thread dispatched last ("k_fwd_bwd_stream<K=2,...>"; one
// name per launch of a multi-launch kernel, joined by '+'); for bench.py's profile check
void note_fwd_bwd_dispatch(const char* fmt, ...);
const char* last_fwd_bwd_dispatch();

// ---- forward-backward on a band of the emit/shift lattice (fwd_bwd_band.hip) ----
struct FwdBwdBandArgs {
  const float* log_trans;  // (B,T,R,2): band cell (s,r) is lattice cell (s, band_start[b,s] + r)
  const float* log_obs;    // (B,T,R) or null
  const int* band_start;   // (B,T): first column of every step's window
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  int B, T, R, flags;      // R: band width, 1..256
  float* loss;       // (B)
  float* grad;       // (B,T,R,2) or null
  float* grad_obs;   // (B,T,R) or null (requires log_obs)
  void* workspace;   // row storage when the rows do not fit LDS; gradients only
  size_t workspace_bytes;
  int* status;
};
// the head of the kernel's LDS, then the rows of both directions when they fit; else workspace_bytes
RowsPlan band_plan(int B, int T, int R);
size_t fwd_bwd_band_workspace_bytes(int B, int T, int R);
int launch_fwd_bwd_band(const FwdBwdBandArgs& a, hipStream_t stream);

// ---- exact best path on the emit/shift lattice (viterbi.hip) ----
struct ViterbiArgs {
  const float* log_trans;  // (B,T,U,2)
  const float* log_obs;    // (B,T,U) or null
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  int B, T, U, flags;
  float* log_prob;   // (B)
  int* position;     // (B,T) or null
  int* duration;     // (B,U) or null
  void* workspace;   // backpointer bits when they do not fit LDS
  size_t workspace_bytes;
  int* status;
};
size_t viterbi_workspace_bytes(int B, int T, int U);
int launch_viterbi(const ViterbiArgs& a, hipStream_t stream);

// ---- exact best path on a band of the emit/shift lattice (viterbi_band.hip) ----
struct ViterbiBandArgs {
  const float* log_trans;  // (B,T,W,2): band cell (s,r) is lattice cell (s, band_start[b,s] + r)
  const float* log_obs;    // (B,T,W) or null
  const int* band_start;   // (B,T): first column of every step's window
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  int B, T, W, max_pos, flags;  // W: band width, 1..256; max_pos sizes duration only
  float* log_prob;   // (B)
  int* position;     // (B,T) or null: absolute positions
  int* duration;     // (B,max_pos) or null
  void* workspace;   // decision words when they do not fit LDS; paths only
  size_t workspace_bytes;
  int* status;
};
size_t viterbi_band_workspace_bytes(int B, int T, int W);
int launch_viterbi_band(const ViterbiBandArgs& a, hipStream_t stream);

// ---- the exact N best alignments on the emit/shift lattice (nbest_align.hip) ----
struct NbestAlignArgs {
  const float* log_trans;  // (B,T,U,2)
  const float* log_obs;    // (B,T,U) or null
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  int B, T, U, N, flags;   // N: alignments per utterance, 1..8
  float* log_prob;   // (B,N)
  int* position;     // (B,N,T) or null
  int* duration;     // (B,N,U) or null
  void* workspace;   // backpointer tags when they do not fit LDS
  size_t workspace_bytes;
  int* status;
};
size_t nbest_align_workspace_bytes(int B, int T, int U, int N);
int launch_nbest_align(const NbestAlignArgs& a, hipStream_t stream);

// ---- alignments drawn from the posterior of the emit/shift lattice (sample_align.hip) ----
struct SampleAlignArgs {
  const float* log_trans;  // (B,T,U,2)
  const float* log_obs;    // (B,T,U) or null
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  const float* uniform;    // (B,NS,T): the random input, one number per sample and step
  int B, T, U, NS, flags;  // NS: samples per utterance, 1..64
  float* log_prob;   // (B,NS)
  int* position;     // (B,NS,T) or null
  int* duration;     // (B,NS,U) or null
  void* workspace;   // decision bits when they do not fit LDS
  size_t workspace_bytes;
  int* status;
};
size_t sample_align_workspace_bytes(int B, int T, int U, int NS);
int launch_sample_align(const SampleAlignArgs& a, hipStream_t stream);

// ---- expected path cost and its gradients on the emit/shift lattice (expected_cost.hip) ----
struct ExpectedCostArgs {
  const float* log_trans;  // (B,T,U,2)
  const float* log_obs;    // (B,T,U) or null
  const float* cost;       // (B,T,U,2): added to a path's cost when it takes the edge
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  int B, T, U, flags;
  float* risk;        // (B)
  float* loss;        // (B) or null
  float* grad_trans;  // (B,T,U,2) or null
  float* grad_cost;   // (B,T,U,2) or null
  float* grad_obs;    // (B,T,U) or null (requires log_obs)
  void* workspace;    // Z and risk per utterance, then both chains' rows; gradients only
  size_t workspace_bytes;
  int* status;
};
size_t expected_cost_workspace_bytes(int B, int T, int U);
int launch_expected_cost(const ExpectedCostArgs& a, hipStream_t stream);
#ifdef SSNT_AB
// the transition rows of one chunk of the sweep for this shape, and which launches run (bit 0 the
// sweep, bit 1 the gradient launch; 3 default)
int expected_cost_chunk_rows(int U, bool obs);
int set_expected_cost_launches(int mask);
#endif
// the same sweeps without the mean (expected_cost.hip): alpha and beta rows (m, e: 8 B per cell and
// direction), Z and loss into a workspace of alpha_beta_rows_workspace_bytes(); cost, risk and the
// gradient pointers of `a` are not read. The caller has made launch_expected_cost's checks.
size_t alpha_beta_rows_workspace_bytes(int B, int T, int U);
int alpha_beta_chunk_rows(int U, bool obs);
int launch_alpha_beta_sweep(const ExpectedCostArgs& a, hipStream_t stream);

// ---- the posterior duration distribution on the emit/shift lattice (duration_posterior.hip) ----
struct DurationPosteriorArgs {
  const float* log_trans;  // (B,T,U,2)
  const float* log_obs;    // (B,T,U) or null
  const int* step_len;     // (B)
  const int* pos_len;      // (B)
  int B, T, U, D, flags;   // D: bins, 2..256; bin d < D-1 is P(d_p = d), bin D-1 the tail P(d_p >= D-1)
  float* dur_post;    // (B,U,D)
  float* loss;        // (B) or null
  void* workspace;    // Z per utterance, then both chains' rows
  size_t workspace_bytes;
  int* status;
};
size_t duration_posterior_workspace_bytes(int B, int T, int U, int D);
int launch_duration_posterior(const DurationPosteriorArgs& a, hipStream_t stream);
#ifdef SSNT_AB
// the step rows of one staged chunk and the positions of one workgroup's tile for this shape
// (rows in the low 16 bits, positions above), and which launches run (bit 0 the sweeps, bit 1 the
// duration launch; 3 default); the sweeps' chunk depth is alpha_beta_chunk_rows
int duration_posterior_block(int U, int D, bool obs);
int set_duration_posterior_launches(int mask);
#endif

// ---- F4: v2 duration-class forward-backward (v2_fwd_bwd.hip) ----
struct V2FwdBwdArgs {
  const float* logits;       // (B, Imax, D) per-step class log-probs
  const int* table;          // (D) duration_table, >= 0
  const int* input_length;   // (B) I_b <= Imax
  const int* output_length;  // (B) O_b
  int B, Imax, D, X;         // X = max_total + 1 totals per row
  int zid;                   // zero_duration_id
  bool allow_skip, test_mode;
  int flags;                 // SSNT_FLAG_ZERO_INFINITY
  float* loss;               // (B)
  float* grad;               // (B, Imax, D) or null
  float* log_alpha;          // (B, Imax+1, X) or null
  float* log_beta;           // (B, Imax+1, X) or null
  void* workspace;
  size_t workspace_bytes;
  int Wcap;                  // set by the launcher
  int chunk;                 // set by the launcher
  bool fwd_only;             // set by the launcher: alpha rows and Z only (workspace: rows | Z)
  int* status;
};
size_t v2_fwd_bwd_workspace_bytes(int B, int Imax, int max_total, bool test_mode);
int launch_v2_fwd_bwd(const V2FwdBwdArgs& a, hipStream_t stream);
// F4's forward sweep alone, for the sampler: alpha rows 0..I and Z into a workspace of
// v2_fwd_only_workspace_bytes() (loss may be null; grad and the debug rows are ignored).
// launch == false: F4's refusals only, nothing launched.
size_t v2_fwd_only_workspace_bytes(int B, int Imax, int max_total, bool test_mode);
int launch_v2_fwd_only(const V2FwdBwdArgs& a, bool launch, hipStream_t stream);

// ---- expected path cost and its gradients on the v2 lattice (v2_expected_cost.hip) ----
struct V2ExpectedCostArgs {
  const float* logits;       // (B, Imax, D) per-step class log-probs
  const float* cost;         // (B, Imax, D) added to a path's cost when step t takes class i
  const int* table;          // (D) duration_table, >= 0
  const int* input_length;   // (B) I_b <= Imax
  const int* output_length;  // (B) O_b
  int B, Imax, D, X;         // X = max_total + 1 totals per row
  int zid;                   // zero_duration_id
  bool allow_skip, test_mode;
  float* risk;               // (B)
  float* loss;               // (B) or null
  float* grad_logits;        // (B, Imax, D) or null
  float* grad_cost;          // (B, Imax, D) or null
  void* workspace;           // F4's rows and Z, the mean rows, risk; gradients only
  size_t workspace_bytes;
  int* status;
};
size_t v2_expected_cost_workspace_bytes(int B, int Imax, int max_total, bool test_mode, bool need_grad);
int launch_v2_expected_cost(const V2ExpectedCostArgs& a, hipStream_t stream);
#ifdef SSNT_AB
// the sweep steps of one staged chunk for D classes (the instance a call launches), and which
// launches of the full call run (bit 0 the sweeps, bit 1 the gradient launch; 3 default)
int v2_expected_cost_chunk_steps(int D);
int set_v2_expected_cost_launches(int mask);
#endif

// ---- exact best duration path on the v2 lattice (v2_viterbi.hip) ----
struct V2ViterbiArgs {
  const float* logits;       // (B, Imax, D) per-step class log-probs
  const int* table;          // (D) duration_table, >= 0
  const int* input_length;   // (B) I_b <= Imax
  const int* output_length;  // (B) O_b
  int B, Imax, D, X;         // X = max_total + 1 totals per row
  int zid;                   // zero_duration_id
  bool allow_skip, test_mode;
  float* log_prob;           // (B)
  int* duration_class;       // (B, Imax) or null
  int* duration;             // (B, Imax) or null
  int* total;                // (B) or null
  void* workspace;           // backpointer bytes when they do not fit LDS
  size_t workspace_bytes;
  int Wcap;                  // set by the launcher
  int* status;
};
size_t v2_viterbi_workspace_bytes(int B, int Imax, int max_total, bool test_mode);
int launch_v2_viterbi(const V2ViterbiArgs& a, hipStream_t stream);

// ---- the exact N best duration paths on the v2 lattice (v2_nbest_align.hip) ----
struct V2NbestArgs {
  const float* logits;       // (B, Imax, D) per-step class log-probs
  const int* table;          // (D) duration_table, >= 0
  const int* input_length;   // (B) I_b <= Imax
  const int* output_length;  // (B) O_b
  int B, Imax, D, X, N;      // X = max_total + 1 totals per row; N: paths per utterance, 1..8
  int zid;                   // zero_duration_id
  bool allow_skip, test_mode;
  float* log_prob;           // (B, N)
  int* duration_class;       // (B, N, Imax) or null
  int* duration;             // (B, N, Imax) or null
  int* total;                // (B, N) or null
  void* workspace;           // backpointer entries when they do not fit LDS
  size_t workspace_bytes;
  int Wcap;                  // set by the launcher
  int* status;
};
size_t v2_nbest_workspace_bytes(int B, int Imax, int max_total, bool test_mode, int N);
int launch_v2_nbest_align(const V2NbestArgs& a, hipStream_t stream);

// ---- duration paths drawn from the posterior of the v2 lattice (v2_sample_align.hip) ----
struct V2SampleArgs {
  const float* logits;       // (B, Imax, D) per-step class log-probs
  const int* table;          // (D) duration_table, >= 0
  const int* input_length;   // (B) I_b <= Imax
  const int* output_length;  // (B) O_b
  const float* uniform;      // (B, NS, Imax+1): the random input; [.., t] step t's class, [.., Imax] the total
  int B, Imax, D, X, NS;     // X = max_total + 1 totals per row; NS: samples per utterance, 1..64
  int zid;                   // zero_duration_id
  bool allow_skip, test_mode;
  float* log_prob;           // (B, NS)
  int* duration_class;       // (B, NS, Imax) or null
  int* duration;             // (B, NS, Imax) or null
  int* total;                // (B, NS) or null
  void* workspace;           // F4's alpha rows and Z
  size_t workspace_bytes;
  int Wcap;                  // set by the launcher
  int* status;
};
size_t v2_sample_workspace_bytes(int B, int Imax, int max_total, bool test_mode);
int launch_v2_sample_align(const V2SampleArgs& a, hipStream_t stream);
#ifdef SSNT_AB
// steps per memory round trip of the walk (0 auto, 1, 2, 4) and which launches run (bit 0 the
// forward sweep, bit 1 the walk; 3 default)
int set_v2_sample_form(int cone, int launches);
#endif

// ---- beam-search decode (decode.hip) ----
enum class Variant : int { V1 = 0, V2 = 1, Tone = 2 };

struct StepArgs {
  Variant variant;
  int B, W, Wmax, C;  // C: classes per beam (2 for v1, D for v2, tone classes)
  const float* h;     // (B,W,C)
  const float* hist;  // (B,W)
  const bool* fin;    // (B,W)
  const int* t;       // (B,W)
  const int* u;       // (B,W)
  const int* input_length;   // (B) (v1: may be null -> scalar_input_length)
  int scalar_input_length;   // v1 reference symbol: one max_t for the batch (src/lib.rs:99)
  const int* output_length;  // (B) v2
  const int* total;          // (B,W) v2
  const int* table;          // (D) v2
  int special_id;            // v2 zero_duration_id / tone empty_tone_id
  bool allow_skip, test_mode;
  int* prediction;
  float* log_prob;
  int* next_t;
  int* next_u;
  bool* next_fin;
  int* next_total;  // v2
  int* beam_branch;
  int* status;
};
int launch_decode_step(const StepArgs& a, hipStream_t stream);

// Fused multi-step decode (fused_decode.hip): all beams start at t = u = 0, log-prob 0,
// total 0, not finished; step s feeds the exact per-step contract with
//   V1:        h[w] = src[b, s, t_w, :]  (src = (B,T,U,2) lattice; live beams have u_w == s)
//   V2 / Tone: h    = src[b, s]          (src = (B,T,W,C) per-step logits)
// and the step's outputs become the next state (the role of the TF decode loop). After the
// last step the final slots are backtraced in the same launch.
struct FusedDecodeArgs {
  Variant variant;
  int B, T, U, W, C;         // U: lattice positions (V1 only); C: classes (2 for V1)
  const float* src;
  const int* table;          // (C) v2 duration_table
  const int* input_length;   // (B)
  const int* output_length;  // (B) v2
  int special_id;            // v2 zero_duration_id / tone empty_tone_id (v1: 0)
  bool allow_skip, test_mode;
  // per-step outputs (B,T,W)
  int* prediction;
  float* log_prob;
  int* next_t;
  int* next_u;
  bool* next_fin;
  int* next_total;           // v2 (required)
  int* beam_branch;
  // path outputs, each optional
  int* ordered;              // (B,W,T): order_beam_branch with final_branch = [0..W)
  int* path_pred;            // (B,W,T): prediction along each path
  int* duration;             // (B,W,T): v2 duration added at each step of each path
  int* best_beam_branch;     // (B,T): path of slot 0 (util.rs:20-33)
  int* best_t_history;       // (B,T): next_t along that path
  int* status;
};
int launch_fused_decode(const FusedDecodeArgs& a, hipStream_t stream);
int diag_decode_read(void* host, size_t bytes);  // -DSSNT_DIAG builds only

int launch_extract_best(int B, int W, int U, const int* best_final_branch, const int* beam_branch,
                        const int* t_history, int* best_beam_branch, int* best_t_history,
                        int* status, hipStream_t stream);
int launch_order_beam_branch(int B, int W, int T, const int* final_branch,
                             const int* beam_branch, int* ordered, int* status,
                             hipStream_t stream);
int launch_upsample(int B, int W, int T, int max_u, const int* duration,
                    const int* output_length, int* out, int* status, hipStream_t stream);
int launch_levenshtein(int B, int max_length, const int* a, const int* b, const int* a_len,
                       const int* b_len, int* dist, hipStream_t stream);

}  // namespace ssnt
