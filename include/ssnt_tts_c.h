/*
 * ssnt_tts_c.h -- drop-in C ABI of libssnt_tts_c, MI355X (gfx950) implementation.
 *
 * Part 1 re-exports, with identical names, argument order, types and meaning, the seven
 * unmangled symbols of the reference's Rust `staticlib` ssnt_tts_c
 * (nii-yamagishilab/ssnt-tts-rust, ssnt_tts_c/src/lib.rs), which the TensorFlow custom ops in
 * ssnt-tts-tensorflow/src/ (*_op.cc) declare `extern "C"` and link with -lssnt_tts_c
 * (ssnt-tts-tensorflow/setup.py:15,40-42). Arguments are HOST pointers; each call is
 * synchronous; contract violations print to stderr and abort(), as the Rust assert!/panic in
 * an extern fn does. The work runs on the GPU (per-thread stream and scratch; reentrant).
 *
 * Part 2 adds entry points the reference does not have: the lattice forward-backward
 * (SURVEY.md 8(a) A11), batched and fused decode, and device-pointer + hipStream_t variants of
 * every kernel. They return an ssnt_status code instead of aborting.
 *
 * `bool` is the 1-byte C99/C++ bool, identical to Rust's `bool` in extern fns.
 */
#ifndef SSNT_TTS_C_H
#define SSNT_TTS_C_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ===================== Part 1: reference symbols (host pointers) ===================== */

/* One v1 emit/shift beam-search step, batch fixed to 1.
 * Replaces ssnt_tts_c/src/lib.rs:11-83 (-> src/lib.rs:121-230); caller
 * ssnt-tts-tensorflow/src/ssnt_tts_beam_search_decode_op.cc:5-8,116-128.
 * h (W,2) [emit, shift] log-probs; log_prob_history, is_finished, t, u (W); outputs (W). */
void ssnt_tts_beam_search_decode(const float *h, const float *log_prob_history,
                                 const bool *is_finished, const int *t, const int *u, int max_t,
                                 int beam_width, int *prediction, float *log_probs, int *next_t,
                                 int *next_u, bool *next_is_finished, int *beam_branch);

/* Backtrace of the best final beam. Replaces ssnt_tts_c/src/lib.rs:87-116
 * (-> src/util.rs:20-33); caller ssnt_extract_best_beam_branch_op.cc:6-8 (declared `bool`
 * there, return value ignored). beam_branch, t_history (max_u, W); outputs (max_u). */
void ssnt_extract_best_beam_branch(int best_final_branch, const int *beam_branch,
                                   const int *t_history, int beam_width, int max_u,
                                   int *best_beam_branch, int *best_t_history);

/* One v2 duration-class beam-search step. Replaces ssnt_tts_c/src/lib.rs:119-218
 * (-> src/v2.rs:221-339); caller ssnt_tts_v2_beam_search_decode_op.cc:5-26,179-200.
 * h (B,W,D); state (B,W); duration_table (D); input/output_length (B); outputs (B,W). */
void ssnt_tts_v2_beam_search_decode(const float *h, const float *log_prob_history,
                                    const bool *is_finished, const int *total_duration,
                                    const int *duration_table, const int *t, const int *u,
                                    const int *input_length, const int *output_length,
                                    int batch_size, int beam_width, int duration_class_size,
                                    int zero_duration_id, bool allow_skip, bool test_mode,
                                    int *prediction, float *log_probs, int *next_t, int *next_u,
                                    bool *next_is_finished, int *next_total_duration,
                                    int *beam_branch);

/* Backtrace of every final beam. Replaces ssnt_tts_c/src/lib.rs:221-241
 * (-> src/v2_util.rs:6-36); caller ssnt_order_beam_branch_op.cc:6-11.
 * final_branch (B,W); beam_branch (B,max_t,W); ordered_beam_branch (B,W,max_t). */
void ssnt_order_beam_branch(const int *final_branch, const int *beam_branch, int batch_size,
                            int beam_width, int max_t, int *ordered_beam_branch);

/* Durations -> frame-to-input index map. Replaces ssnt_tts_c/src/lib.rs:245-265
 * (-> src/v2_util.rs:39-66); caller upsample_source_indexes_op.cc:6-12. Writes only the first
 * min(output_length[b,w], max_u) entries of each (b,w) row (the op prefills the rest). */
void ssnt_upsample_source_indexes(const int *duration, const int *output_length, int batch_size,
                                  int beam_width, int max_t, int max_u,
                                  int *upsampled_source_indexes);

/* One tone-latent beam-search step. Replaces ssnt_tts_c/src/lib.rs:268-343
 * (-> src/tone_latent.rs:144-234); caller tone_latent_beam_search_decode_op.cc. */
void tone_latent_beam_search_decode(const float *h, const float *log_prob_history,
                                    const bool *is_finished, const int *t, const int *u,
                                    const int *input_length, int batch_size, int beam_width,
                                    int tone_class_size, int empty_tone_id, int *prediction,
                                    float *log_probs, int *next_t, int *next_u,
                                    bool *next_is_finished, int *beam_branch);

/* Batched Levenshtein distance. Replaces ssnt_tts_c/src/lib.rs:347-381
 * (-> src/edit_distance.rs:6-60); caller ssnt_tts_edit_distance.cc. */
void tone_latent_levenshtein_edit_distance(const int *a, const int *b, const int *a_lengths,
                                           const int *b_lengths, int batch_size,
                                           int max_length, int *distance);

/* ===================== Part 2: extensions ===================== */

typedef enum {
  SSNT_OK = 0,
  SSNT_ERR_INVALID_ARG = 1,
  SSNT_ERR_HIP = 2,
  SSNT_ERR_NO_CANDIDATE = 3,      /* v2: src/v2.rs:292 assert */
  SSNT_ERR_DURATION_MISMATCH = 4, /* upsample: src/v2_util.rs:58 assert */
  SSNT_ERR_UNSUPPORTED = 5,       /* size outside what the kernels handle */
  SSNT_ERR_WORKSPACE = 6,         /* workspace missing / too small */
  SSNT_ERR_BAD_LENGTH = 7,        /* a length exceeds the tensor extent */
  SSNT_ERR_BAD_INDEX = 8,         /* backtrace branch index outside [0, W) */
  SSNT_ERR_INTERNAL = 9,          /* fwd-bwd: a bounded intra-kernel wait expired (a bug) */
  SSNT_ERR_BAD_BAND = 10          /* banded fwd-bwd: band_start is not a valid band */
} ssnt_status;

const char *ssnt_status_string(int status);
/* translate the bits a kernel OR-ed into a device status word into an ssnt_status */
int ssnt_status_from_bits(int bits);
/* library / device info: fills a short human-readable string, returns SSNT_OK */
int ssnt_version(char *buf, size_t len);

/* lattice flags */
#define SSNT_FLAG_TERMINAL_EMIT 1 /* Z includes the terminal emit at (S-1,P-1) (src/lib.rs:187-195) */
#define SSNT_FLAG_ZERO_INFINITY 2 /* infeasible utterances report loss 0 instead of +inf */

/* ---- emit/shift lattice forward-backward ----
 * log_trans (B,T,U,2) f32 natural-log [emit, shift] probabilities, row-major;
 * log_obs (B,T,U) optional per-cell log-likelihood (NULL = none);
 * step_len, pos_len (B): lattice extent S_b <= T steps, P_b <= U positions.
 * Outputs: loss (B) = -ln Z; grad_trans (B,T,U,2) = d loss / d log_trans (NULL = skip);
 * grad_obs (B,T,U) = d loss / d log_obs (NULL = skip); log_alpha / log_beta (B,T,U) debug
 * outputs (NULL = skip). Cells outside (S_b,P_b) get grad 0 and log-alpha/beta -inf.
 * Never read into a result, whatever they hold (NaN and +-inf included): log_trans and log_obs at
 * steps >= S_b or positions >= P_b, the shift out of position P_b - 1, every entry of step
 * S_b - 1 but the terminal emit at (S_b - 1, P_b - 1) -- that one too without
 * SSNT_FLAG_TERMINAL_EMIT -- and the previous contents of the outputs and the workspace.
 * Input domain of the cells that are read: a value below -1e6 and a NaN are exact zeros (as -inf),
 * a value above +1e6 is clamped to +1e6, and the results are specified only while every partial
 * log-probability (log alpha, log beta, ln Z) stays above about -2^29 ln 2 = -3.7e8 (DESIGN.md 3
 * "Input domain").
 * Device variant: all pointers are device pointers; `stream` is a hipStream_t (NULL = legacy
 * default); `workspace` must hold ssnt_fwd_bwd_workspace_size() bytes -- always take the size
 * from that query, never compute it: it is 0 (NULL workspace) when every row of the dispatched
 * kernel stays in LDS (U <= 256 and T*U small enough), else the segmented kernel's rows
 * ((T+1)*U xf per utterance) plus its hand-off counter block and hand-off rings, each padded to
 * 256 B; `status` (device int, may be NULL) receives error bits. Asynchronous. The kernel is
 * chosen from the shape and alignment alone (no process-wide state). */
size_t ssnt_fwd_bwd_workspace_size(int batch, int max_steps, int max_pos);
/* Name of the forward-backward kernel instance the calling thread's last ssnt_fwd_bwd* call
 * dispatched (e.g. "k_fwd_bwd_stream<K=2,OBS=0,LDS=1,NC=3,NH=4,NV=0>"; launches of one call
 * joined by '+'), copied into buf (truncated to len); returns its full length. Lets a profile be
 * matched to the kernel a benchmark actually ran. */
int ssnt_fwd_bwd_last_kernel(char *buf, size_t len);
int ssnt_fwd_bwd_device(const float *log_trans, const float *log_obs, const int *step_len,
                        const int *pos_len, int batch, int max_steps, int max_pos, int flags,
                        float *loss, float *grad_trans, float *grad_obs, float *log_alpha,
                        float *log_beta, void *workspace, size_t workspace_bytes, int *status,
                        void *stream);
/* As ssnt_fwd_bwd_device, plus the batch loss sum *loss_sum = sum_b loss[b] (device float) in a
 * fixed summation order (deterministic; independent of the kernel variant). `sum_state` is a
 * device buffer of ssnt_fwd_bwd_sum_state_size(batch) bytes, zeroed once before its first use
 * and then left to the library: with it, workgroup 0 forms the sum inside the same launch from
 * per-utterance 8-byte {tag, loss} granules; NULL costs one extra single-wave launch. One state
 * per stream of concurrent calls. New: the reference has no forward-backward (SURVEY.md 8(a)
 * A11). */
size_t ssnt_fwd_bwd_sum_state_size(int batch);
int ssnt_fwd_bwd_sum_device(const float *log_trans, const float *log_obs, const int *step_len,
                            const int *pos_len, int batch, int max_steps, int max_pos, int flags,
                            float *loss, float *grad_trans, float *grad_obs, float *log_alpha,
                            float *log_beta, void *workspace, size_t workspace_bytes, int *status,
                            float *loss_sum, void *sum_state, void *stream);
/* Float64 outputs of the same computation (the north_star bar is 1e-5 abs on
 * log-alpha / log-beta, which an f32 value cannot hold once |log alpha| > ~84 -- half an f32
 * ulp at configs[4]'s |log alpha| ~ 2231 is 1.2e-4). The dispatched kernel writes its
 * split-exponent state m * 2^e (m in [0.5, 1)) instead of f32 logs, and a second pass forms
 * e*ln2 + ln(m) in float64 on the GPU: loss (B) = -ln Z, log_alpha / log_beta (B,T,U) (NULL =
 * skip; -inf outside the lattice). grad_trans / grad_obs and every rule as
 * ssnt_fwd_bwd_device (the same launch, the same kernel the shape dispatches; gradients
 * bit-identical). `workspace`: ssnt_fwd_bwd_debug64_workspace_size() bytes (the plain
 * workspace plus the state planes, 16 B per cell). The input cells never read into a result
 * are those of ssnt_fwd_bwd_device. Device pointers, asynchronous. New: the
 * reference has no forward-backward. */
size_t ssnt_fwd_bwd_debug64_workspace_size(int batch, int max_steps, int max_pos);
int ssnt_fwd_bwd_debug64_device(const float *log_trans, const float *log_obs, const int *step_len,
                                const int *pos_len, int batch, int max_steps, int max_pos,
                                int flags, double *loss, float *grad_trans, float *grad_obs,
                                double *log_alpha, double *log_beta, void *workspace,
                                size_t workspace_bytes, int *status, void *stream);
/* ---- forward-backward on a band of the emit/shift lattice ----
 * The lattice of ssnt_fwd_bwd_device with every cell outside a band removed: at step s only the
 * band_width = R columns p = band_start[b,s] + r, r in [0, R), exist. log_trans_band (B,T,R,2),
 * log_obs_band (B,T,R) (NULL = none) and the gradients hold band cell (s,r) = lattice cell
 * (s, band_start[b,s] + r); band_start (B,T) i32; step_len S_b <= T and pos_len P_b (no max_pos:
 * the dense lattice is never formed). A band is valid when band_start[b,0] == 0, every
 * band_start[b,s+1] - band_start[b,s] is 0 or 1 (s + 1 < S_b), and the last window holds the last
 * position: band_start[b,S_b-1] <= P_b - 1 < band_start[b,S_b-1] + R. Outputs: loss (B) = -ln of
 * the mass of the paths inside the band; grad_band (B,T,R,2) and grad_obs_band (B,T,R) its
 * gradients (NULL = skip), bit for bit those of ssnt_fwd_bwd_device on the dense lattice that is
 * -inf outside the band and on the two kinds of edges that leave it: the shift out of r = R-1
 * when the band stays, the emit out of r = 0 when it moves. Those edges get gradient +0.
 * Never read into a result: what ssnt_fwd_bwd_device never reads (with p = band_start + r; columns
 * at p >= P_b are dead), the band-leaving edges, and band_start at steps >= S_b. Infeasible
 * utterances, bad lengths (S_b > T or a negative length: SSNT_ERR_BAD_LENGTH in `status`) and the
 * flags as ssnt_fwd_bwd_device. An invalid band makes its utterance infeasible (loss +inf, or 0
 * with SSNT_FLAG_ZERO_INFINITY; gradients 0) and sets SSNT_ERR_BAD_BAND in `status`; it is refused
 * by comparisons alone and the other utterances are unaffected. band_width outside [1, 256] and
 * a max_steps whose band_start does not fit LDS (above about 39000) return SSNT_ERR_UNSUPPORTED.
 * `workspace` holds ssnt_fwd_bwd_band_workspace_size() bytes when a gradient is requested: 0 (NULL
 * workspace) while the rows of both sweeps fit LDS, else 8 bytes per band cell; missing or short:
 * SSNT_ERR_WORKSPACE. Without gradients no workspace is needed and loss has the same bits. A
 * refused call writes nothing. Device pointers, asynchronous on `stream`. New: the reference has
 * no forward-backward. */
size_t ssnt_fwd_bwd_band_workspace_size(int batch, int max_steps, int band_width);
int ssnt_fwd_bwd_band_device(const float *log_trans_band, const float *log_obs_band,
                             const int *band_start, const int *step_len, const int *pos_len,
                             int batch, int max_steps, int band_width, int flags, float *loss,
                             float *grad_band, float *grad_obs_band, void *workspace,
                             size_t workspace_bytes, int *status, void *stream);
/* Host-pointer variant (synchronous; copies through the calling thread's GPU context). */
int ssnt_fwd_bwd(const float *log_trans, const float *log_obs, const int *step_len,
                 const int *pos_len, int batch, int max_steps, int max_pos, int flags,
                 float *loss, float *grad_trans, float *grad_obs, float *log_alpha,
                 float *log_beta);

/* ---- exact best path (Viterbi) on the emit/shift lattice ----
 * The max-plus recurrence over the tensors of ssnt_fwd_bwd_device, IEEE f32 adds and compares in
 * the order DESIGN.md 2.2 states (a tie keeps the emit), so the outputs are bit-identical to a
 * plain f32 restatement. log_prob (B) = log-probability of the most probable monotone alignment
 * (with the terminal emit under SSNT_FLAG_TERMINAL_EMIT, the only flag accepted); position (B,T)
 * = the input position of every step on that path (-1 for steps >= S_b; NULL = skip); duration
 * (B,U) = the number of steps each position holds (0 for positions >= P_b; NULL = skip). An
 * infeasible utterance (S_b < P_b, S_b = 0, P_b = 0, log_prob = -inf, or a length beyond the
 * tensor, which also sets SSNT_ERR_BAD_LENGTH in `status`) gets log_prob -inf, positions -1 and
 * durations 0. -inf inputs are legal; the input cells ssnt_fwd_bwd_device never reads into a result
 * are never read into one here. max_pos > 1024 returns SSNT_ERR_UNSUPPORTED. `workspace`
 * holds ssnt_viterbi_align_workspace_size() bytes: 0 (NULL workspace) while the backpointer bits
 * of one utterance fit LDS; with position and duration both NULL no backpointers are kept and
 * no workspace is needed. Device pointers, asynchronous on `stream` (a hipStream_t). New: the
 * reference only searches this lattice with a pruned beam. */
size_t ssnt_viterbi_align_workspace_size(int batch, int max_steps, int max_pos);
int ssnt_viterbi_align_device(const float *log_trans, const float *log_obs, const int *step_len,
                              const int *pos_len, int batch, int max_steps, int max_pos, int flags,
                              float *log_prob, int *position, int *duration, void *workspace,
                              size_t workspace_bytes, int *status, void *stream);

/* ---- exact best path (Viterbi) on a band of the emit/shift lattice ----
 * ssnt_viterbi_align_device on the lattice of ssnt_fwd_bwd_band_device: log_trans_band (B,T,R,2),
 * log_obs_band (B,T,R) (NULL = none), band_start (B,T) i32, step_len, pos_len and the validity of a
 * band exactly as there, band_width = R. The outputs are bit for bit those of
 * ssnt_viterbi_align_device on the dense lattice that is the band inside it and -inf outside it and
 * on the two kinds of band-leaving edges (a tie keeps the emit): log_prob (B) = log-probability of
 * the best path whose every cell lies in the band (with the terminal emit under
 * SSNT_FLAG_TERMINAL_EMIT, the only flag accepted); position (B,T) = its absolute position
 * band_start + r at every step (-1 for steps >= S_b; NULL = skip); duration (B,max_pos) = the steps
 * each position holds (0 for positions >= P_b; NULL = skip). max_pos only sizes duration: with
 * duration NULL it is ignored, with duration given an utterance with P_b > max_pos is a bad length.
 * An utterance gets log_prob -inf, positions -1 and durations 0 when S_b < P_b, S_b = 0, P_b = 0 or
 * log_prob = -inf; for a bad length (S_b > T, a negative length, P_b > max_pos), which also sets
 * SSNT_ERR_BAD_LENGTH in `status`; and for an invalid band, which also sets SSNT_ERR_BAD_BAND: the
 * band is refused by comparisons alone and the other utterances are unaffected. Never read into a
 * result: what ssnt_fwd_bwd_band_device never reads, the previous contents of the outputs and of
 * the workspace. -inf inputs are legal. band_width outside [1, 256] and a max_steps whose staged
 * band_start and run starts do not fit LDS (above about 16000) return SSNT_ERR_UNSUPPORTED, a flag
 * other than SSNT_FLAG_TERMINAL_EMIT or a missing required pointer SSNT_ERR_INVALID_ARG. `workspace`
 * holds ssnt_viterbi_align_band_workspace_size() bytes when a path is requested: 0 (NULL workspace)
 * while the decision bits of one utterance fit LDS, else 8 bytes per step and 64 columns, 8-byte
 * aligned; missing, short or misaligned: SSNT_ERR_WORKSPACE. With position and duration both NULL
 * no decision bits are kept, no workspace is needed and log_prob has the same bits. A refused call
 * writes nothing. Device pointers, asynchronous on `stream`. New: the reference only searches this
 * lattice with a pruned beam. */
size_t ssnt_viterbi_align_band_workspace_size(int batch, int max_steps, int band_width);
int ssnt_viterbi_align_band_device(const float *log_trans_band, const float *log_obs_band,
                                   const int *band_start, const int *step_len, const int *pos_len,
                                   int batch, int max_steps, int band_width, int max_pos, int flags,
                                   float *log_prob, int *position, int *duration, void *workspace,
                                   size_t workspace_bytes, int *status, void *stream);

/* ---- the exact N best alignments on the emit/shift lattice ----
 * The beam search over this lattice with an unbounded beam, truncated to num_best: every cell of
 * the recurrence of ssnt_viterbi_align_device keeps the num_best best prefixes instead of one,
 * ordered by (value descending; on equal values the emit before the shift, then the better-ranked
 * predecessor). IEEE f32 adds and compares only, in the order DESIGN.md 2.6 states, so the outputs
 * are bit-identical to a plain f32 restatement, a rank's result does not depend on num_best, and
 * num_best = 1 is ssnt_viterbi_align_device. log_prob (B, num_best) = the log-probabilities of the
 * num_best most probable monotone alignments, non-increasing (with the terminal emit under
 * SSNT_FLAG_TERMINAL_EMIT, the only flag accepted); the alignments are pairwise distinct and each
 * one's sequential f32 sum is its log_prob. position (B, num_best, T) and duration
 * (B, num_best, U) as ssnt_viterbi_align_device, per rank (NULL = skip). A rank beyond the number
 * of alignments with positive probability is absent: log_prob -inf, positions -1, durations 0;
 * present ranks come first. An infeasible utterance (S_b < P_b, S_b = 0, P_b = 0, rank 0 absent,
 * or a length beyond the tensor, which also sets SSNT_ERR_BAD_LENGTH in `status`) has every rank
 * absent. -inf inputs are legal; NaN and +inf inputs give unspecified values, but every access
 * stays inside its buffers, positions in [-1, U) and durations in [0, T]. The input cells
 * ssnt_fwd_bwd_device never reads into a result are never read into one here. num_best outside
 * [1, 8] returns SSNT_ERR_INVALID_ARG. Supported: max_pos <= 1024 for num_best <= 2, <= 512 for
 * num_best <= 4, <= 256 for num_best <= 8; beyond that SSNT_ERR_UNSUPPORTED. `workspace` holds
 * ssnt_nbest_align_workspace_size() bytes, 8-byte aligned: 0 (NULL workspace) while the
 * backpointers of one utterance fit LDS; with position and duration both NULL no backpointers
 * are kept and no workspace is needed. A refused call writes nothing. Device pointers,
 * asynchronous on `stream`. New: the reference only searches this lattice with a pruned beam. */
size_t ssnt_nbest_align_workspace_size(int batch, int max_steps, int max_pos, int num_best);
int ssnt_nbest_align_device(const float *log_trans, const float *log_obs, const int *step_len,
                            const int *pos_len, int batch, int max_steps, int max_pos,
                            int num_best, int flags, float *log_prob, int *position,
                            int *duration, void *workspace, size_t workspace_bytes, int *status,
                            void *stream);

/* ---- alignments drawn from the posterior of the emit/shift lattice ----
 * Forward filter, backward sample over the tensors of ssnt_fwd_bwd_device: the forward sweep is
 * the forward-backward's alpha recurrence in split-exponent f32; walking back from (S_b-1, P_b-1),
 * sample k moves from position p to p-1 at step s iff uniform[b,k,s] * t < m', where m' is the
 * move term entering (s,p) and t the sum of its stay and move terms, both f32 at their common
 * exponent (one multiply, one ordered compare). uniform (B, num_samples, T) is the caller's
 * randomness: values are clamped to [0, 1 - 2^-24], NaN counts as 0, so every output is a valid
 * monotone path for any input and the call is a pure function of its arguments (the library holds
 * no generator state). With uniform i.i.d. on [0,1) a path is drawn with its posterior probability
 * p(path | log_trans, log_obs), up to the f32 rounding of alpha. log_prob (B, num_samples) = the
 * log-probability of each drawn path, summed in f32 along the path in the order of DESIGN.md 2.4
 * (with the terminal emit under SSNT_FLAG_TERMINAL_EMIT, the only flag accepted); position
 * (B, num_samples, T) and duration (B, num_samples, U) as ssnt_viterbi_align_device, per sample
 * (NULL = skip). An infeasible utterance (S_b < P_b, S_b = 0, P_b = 0, alpha[S_b-1][P_b-1] = 0, or
 * a length beyond the tensor, which also sets SSNT_ERR_BAD_LENGTH in `status`) gets log_prob
 * -inf, positions -1 and durations 0 for every sample. -inf inputs are legal; the log_trans and
 * log_obs cells ssnt_fwd_bwd_device never reads into a result are never read into one here.
 * max_pos > 1024 returns SSNT_ERR_UNSUPPORTED, num_samples outside [1, 64]
 * SSNT_ERR_INVALID_ARG. `workspace` holds ssnt_sample_align_workspace_size() bytes: 0 (NULL workspace) while the decision bits of
 * one utterance (num_samples * T words per lane slot) fit LDS; the bits are needed for log_prob
 * too, so the workspace does not depend on which outputs are requested. Device pointers,
 * asynchronous on `stream`. New: the reference has no sampler. */
size_t ssnt_sample_align_workspace_size(int batch, int max_steps, int max_pos, int num_samples);
int ssnt_sample_align_device(const float *log_trans, const float *log_obs, const int *step_len,
                             const int *pos_len, const float *uniform, int batch, int max_steps,
                             int max_pos, int num_samples, int flags, float *log_prob,
                             int *position, int *duration, void *workspace,
                             size_t workspace_bytes, int *status, void *stream);

/* ---- expected path cost and its gradients on the emit/shift lattice ----
 * The expectation semiring over the tensors of ssnt_fwd_bwd_device: cost (B,T,U,2) f32 is added
 * to a path's cost when it takes the edge [b,s,p,k] (k = 0 emit, 1 shift; the terminal emit's cost
 * counts iff SSNT_FLAG_TERMINAL_EMIT, the only flag accepted), and risk (B) = the expectation of
 * that sum under p(path | log_trans, log_obs). loss (B) = -ln Z as ssnt_fwd_bwd_device, with
 * Z = alpha[S-1][P-1] * beta[S-1][P-1]. With q the posterior probability of an edge, abar the mean
 * cost accumulated before a cell and bbar the mean cost from it on (both given that the path
 * passes the cell): grad_cost (B,T,U,2) = d risk / d cost = q; grad_trans (B,T,U,2) =
 * d risk / d log_trans = q * (abar[src] + cost + bbar[dst] - risk), exactly 0 for the terminal
 * emit; grad_obs (B,T,U) = d risk / d log_obs = (alpha*beta/Z) * (abar + bbar - risk). alpha and
 * beta are the forward-backward's recurrences in split-exponent f32; a mean is the plain f32
 * convex combination (t1*(m1 + c1) + t2*(m2 + c2)) / (t1 + t2) of the two terms entering the cell
 * at their common exponent, in both directions. loss and each gradient may be NULL (skip);
 * grad_obs requires log_obs. Every element of every requested output is written: 0 outside
 * (S_b, P_b), for the masked shift out of P_b-1 and in row S_b-1, except grad_cost = 1 at the
 * terminal emit under the flag. An infeasible utterance (S_b < P_b, S_b = 0, P_b = 0, Z = 0, or a
 * length beyond the tensor, which also sets SSNT_ERR_BAD_LENGTH in `status`) gets risk 0, loss
 * +inf and gradients 0. -inf in log_trans / log_obs is legal; cost must be finite on the edges
 * inside the lattice (elsewhere values are unspecified, every access stays in bounds); the
 * log_trans, log_obs and cost cells ssnt_fwd_bwd_device never reads into a result are never read
 * into one here. max_pos > 1024 returns SSNT_ERR_UNSUPPORTED, as do log_trans, cost, grad_trans
 * or grad_cost not 8-byte aligned. `workspace` holds ssnt_expected_cost_workspace_size() bytes,
 * 8-byte aligned (both sweeps' rows, 12 B per cell and direction); with all three gradients NULL
 * only the forward sweep runs and the workspace may be NULL; missing or short otherwise:
 * SSNT_ERR_WORKSPACE. risk and loss have the same bits with and without gradients. A refused
 * call writes nothing. Device pointers, asynchronous on `stream`. New: the reference has no
 * expectation over alignments. */
size_t ssnt_expected_cost_workspace_size(int batch, int max_steps, int max_pos);
int ssnt_expected_cost_device(const float *log_trans, const float *log_obs, const float *cost,
                              const int *step_len, const int *pos_len, int batch, int max_steps,
                              int max_pos, int flags, float *risk, float *loss,
                              float *grad_trans, float *grad_cost, float *grad_obs,
                              void *workspace, size_t workspace_bytes, int *status, void *stream);

/* ---- the posterior duration distribution on the emit/shift lattice ----
 * Over the tensors of ssnt_fwd_bwd_device: the duration of position p on a path is the number of
 * steps s with position[s] = p (>= 1 for every p < P_b). dur_post (B, max_pos, num_bins) f32, the
 * bin index being the duration: dur_post[b,p,d] = P(d_p = d | log_trans, log_obs) for
 * d < num_bins-1 (bin 0 an exact 0), and dur_post[b,p,num_bins-1] = P(d_p >= num_bins-1), the tail,
 * formed by its own sum and never as one minus the rest; a row p < P_b sums to 1. loss (B) = -ln Z
 * with the bits of ssnt_expected_cost_device's loss; it may be NULL. 2 <= num_bins <= 256 and no
 * flag but SSNT_FLAG_TERMINAL_EMIT, else SSNT_ERR_INVALID_ARG, as for a NULL dur_post. Every
 * element of dur_post is written: rows p >= P_b are 0, every bin d > S_b-P_b+1 is an exact 0 (no
 * position can hold more steps), a zero term contributes an exact 0 (with one live path every bin
 * off its durations is +0), and an infeasible utterance (S_b < P_b, S_b = 0, P_b = 0, Z = 0, or a
 * length beyond the tensor, which also sets SSNT_ERR_BAD_LENGTH in `status`) gets dur_post 0 and
 * loss +inf. -inf in log_trans / log_obs is legal; the cells ssnt_fwd_bwd_device never reads into a
 * result are never read into one here. Sums run in step order without atomics: the same bits on
 * every call, alone or in any batch. max_pos > 1024 returns SSNT_ERR_UNSUPPORTED, as does a
 * log_trans not 8-byte aligned. `workspace` holds ssnt_duration_posterior_workspace_size() bytes,
 * 8-byte aligned (alpha's and beta's rows, 8 B per cell and direction; a function of the shape
 * alone, 0 for a shape the call refuses); missing or short: SSNT_ERR_WORKSPACE. A refused call
 * writes nothing. Device pointers, asynchronous on `stream`. New: the reference has no posterior
 * over durations. */
size_t ssnt_duration_posterior_workspace_size(int batch, int max_steps, int max_pos, int num_bins);
int ssnt_duration_posterior_device(const float *log_trans, const float *log_obs,
                                   const int *step_len, const int *pos_len, int batch,
                                   int max_steps, int max_pos, int num_bins, int flags,
                                   float *dur_post, float *loss, void *workspace,
                                   size_t workspace_bytes, int *status, void *stream);

/* ---- F4: v2 duration-class (semi-Markov) forward-backward (DESIGN.md
 * "Duration lattice"). New: the reference only decodes this lattice; the move rules are the v2
 * decode's (src/v2.rs:94-166 -- band, overrun, exact final total, zero-duration class; test_mode
 * keeps only the class rule). logits (B,T,D) per-step class log-probs (teacher-forced, one row
 * per input step); duration_table (D) >= 0; input_length I_b <= T, output_length O_b (B).
 * State totals run 0..max_total (totals above it -- test mode only -- are outside the lattice).
 * Outputs: loss (B) = -ln Z, Z = sum over every admissible class sequence of its probability
 * (+inf when none, 0 with SSNT_FLAG_ZERO_INFINITY); grad (B,T,D) = d loss / d logits = minus
 * the class posteriors (NULL = skip); log_alpha / log_beta (B,T+1,max_total+1) debug rows
 * (NULL = skip). Never read into a result, whatever they hold: logits rows at steps >= I_b, and
 * column zero_duration_id when allow_skip is false; grad is 0 there, and rows beyond I_b of the
 * debug outputs are -inf. `workspace` holds ssnt_v2_fwd_bwd_workspace_size() bytes. Device
 * pointers, asynchronous on `stream`; a negative duration sets SSNT_ERR_BAD_INDEX in `status`. */
size_t ssnt_v2_fwd_bwd_workspace_size(int batch, int max_steps, int max_total, bool test_mode);
int ssnt_v2_fwd_bwd_device(const float *logits, const int *duration_table, const int *input_length,
                           const int *output_length, int batch, int max_steps,
                           int duration_class_size, int max_total, int zero_duration_id,
                           bool allow_skip, bool test_mode, int flags, float *loss, float *grad,
                           float *log_alpha, float *log_beta, void *workspace,
                           size_t workspace_bytes, int *status, void *stream);

/* ---- expected path cost and its gradients on the v2 duration-class lattice ----
 * The expectation semiring over F4's lattice: inputs, states, windows, class rule, duration_table,
 * zero_duration_id, allow_skip, test_mode and max_total are those of ssnt_v2_fwd_bwd_device. cost
 * (B,T,D) f32 is added to a path's cost when step t takes class i, and risk (B) = the expectation
 * of that sum under the posterior over admissible class sequences; loss (B) = -ln Z, the bits of
 * ssnt_v2_fwd_bwd_device. With q(t,x,i) = alpha[t][x] w[t][i] beta[t+1][x+d_i] / Z, abar the mean
 * cost accumulated before a state and bbar the mean cost from it on (both given that the path
 * passes the state): grad_cost (B,T,D) = d risk / d cost = sum_x q, the class posterior (the bits
 * of minus ssnt_v2_fwd_bwd_device's grad); grad_logits (B,T,D) = d risk / d logits =
 * sum_x q * (abar[t][x] + cost[t,i] + bbar[t+1][x+d_i] - risk). alpha and beta are F4's, bit for
 * bit; a mean is the plain f32 convex combination of a cell's D terms at their common exponent
 * (pairwise tree, one division per cell), in both directions. loss and each gradient may be NULL
 * (skip). Every element of every requested output is written: gradient rows at steps >= I_b are 0,
 * as is column zero_duration_id when allow_skip is false. An utterance with no admissible path
 * (I_b = 0, band mode with O_b > max_total, Z = 0, a length outside the tensor, which also sets
 * SSNT_ERR_BAD_LENGTH in `status`, or a negative duration, which sets SSNT_ERR_BAD_INDEX) gets
 * risk 0, loss +inf and gradients 0. -inf logits are legal; a move of weight zero contributes an
 * exact 0 whatever its cost holds (-inf, NaN and +inf included), so cost = logits gives the
 * entropy; where the weight is non-zero cost must be finite. logits and cost rows at steps >= I_b,
 * and column zero_duration_id of both when allow_skip is false, are never read into a result, nor
 * are the previous contents of the outputs and the workspace. duration_class_size > 64 returns
 * SSNT_ERR_UNSUPPORTED, as does a row that does not fit LDS beside its means: 24 bytes per row
 * cell and 12 per staged class, so at 16 classes test mode takes max_total up to about 5,600 (F4,
 * 16 and 8 bytes: about 9,000) and band mode max_total up to about 37,000. max_total outside [0, 1<<24] returns
 * SSNT_ERR_INVALID_ARG. With a gradient requested, `workspace` holds
 * ssnt_v2_expected_cost_workspace_size(.., need_grad = true) bytes, 8-byte aligned (F4's rows plus
 * the two mean rows); missing, short or misaligned: SSNT_ERR_WORKSPACE. With both gradients NULL
 * only the forward sweep runs, no row is kept, the size is 0 and the workspace may be NULL. risk
 * and loss have the same bits with and without gradients, and a result does not depend on the
 * batch around the utterance. A refused call writes nothing. Device pointers, asynchronous on
 * `stream`. New: the reference has no expectation over duration paths. */
size_t ssnt_v2_expected_cost_workspace_size(int batch, int max_steps, int max_total,
                                            bool test_mode, bool need_grad);
int ssnt_v2_expected_cost_device(const float *logits, const float *cost, const int *duration_table,
                                 const int *input_length, const int *output_length, int batch,
                                 int max_steps, int duration_class_size, int max_total,
                                 int zero_duration_id, bool allow_skip, bool test_mode,
                                 float *risk, float *loss, float *grad_logits, float *grad_cost,
                                 void *workspace, size_t workspace_bytes, int *status, void *stream);

/* ---- exact best duration path (Viterbi) on the v2 duration-class lattice.
 * The max-plus recurrence over F4's lattice (same inputs, states, windows and class rule as
 * ssnt_v2_fwd_bwd_device): IEEE f32 adds and strict compares, classes in increasing order (a tie
 * keeps the lower class; the final total is the lowest among equal maxima), so the outputs are
 * bit-identical to a plain f32 restatement. log_prob (B) = log-probability of the most probable
 * admissible class sequence; duration_class (B,T) = its class at every step (-1 for steps >=
 * I_b); duration (B,T) = duration_table[class] (0 for steps >= I_b); total (B) = its final total
 * (= O_b in band mode). Each of the three may be NULL. An utterance with no admissible path (I_b
 * = 0, band mode with O_b > max_total, log_prob = -inf, a length outside the tensor, which also
 * sets SSNT_ERR_BAD_LENGTH in `status`, or a negative duration, which sets SSNT_ERR_BAD_INDEX)
 * gets log_prob -inf, classes -1, durations 0 and total -1. -inf logits are legal; +inf is not
 * clamped. Logits rows at steps >= I_b, and column zero_duration_id when allow_skip is false, are
 * never read into a result. Limits as F4: duration_class_size > 64 and a row beyond LDS return
 * SSNT_ERR_UNSUPPORTED, max_total outside [0, 1<<24] SSNT_ERR_INVALID_ARG. `workspace` holds
 * ssnt_v2_viterbi_align_workspace_size() bytes: 0 (NULL workspace) while the backpointer bytes
 * of one utterance fit LDS; with duration_class and duration both NULL no backpointers are kept
 * and no workspace is needed. Device pointers, asynchronous on `stream`. New: the reference only
 * searches this lattice with a pruned beam. */
size_t ssnt_v2_viterbi_align_workspace_size(int batch, int max_steps, int max_total, bool test_mode);
int ssnt_v2_viterbi_align_device(const float *logits, const int *duration_table,
                                 const int *input_length, const int *output_length, int batch,
                                 int max_steps, int duration_class_size, int max_total,
                                 int zero_duration_id, bool allow_skip, bool test_mode,
                                 float *log_prob, int *duration_class, int *duration, int *total,
                                 void *workspace, size_t workspace_bytes, int *status,
                                 void *stream);

/* ---- the exact N best duration paths on the v2 duration-class lattice.
 * ssnt_v2_viterbi_align_device's sweep (same inputs, states, windows and class rule) with a
 * sorted list of N = num_best entries per cell, 1 <= N <= 8: IEEE f32 adds and ordered compares
 * under one total order -- value descending, then class, then predecessor rank ascending inside
 * the lattice; value descending, then final total, then rank ascending in the final selection --
 * so the outputs are bit-identical to a plain f32 restatement. log_prob (B,N) = the N largest
 * sequential f32 sums (from 0.0f, in step order) over all admissible class sequences,
 * non-increasing; duration_class (B,N,T) = the class sequence of each rank (-1 for steps >= I_b);
 * duration (B,N,T) = duration_table[class] (0 for steps >= I_b); total (B,N) = its final total
 * (= O_b in band mode). Each of the three may be NULL. The N class sequences of an utterance are
 * pairwise distinct (two classes of equal duration give distinct sequences with equal duration
 * rows), each re-sums to its log_prob bit for bit, rank n is the same at every num_best > n, and
 * num_best = 1 gives ssnt_v2_viterbi_align_device's outputs. A rank beyond the number of
 * admissible sequences with positive probability is absent: log_prob -inf, classes -1, durations
 * 0, total -1; present ranks come first. An utterance with no admissible path (I_b = 0, band mode
 * with O_b > max_total, a length outside the tensor, which also sets SSNT_ERR_BAD_LENGTH in
 * `status`, or a negative duration, which sets SSNT_ERR_BAD_INDEX) has every rank absent. -inf
 * logits are legal; NaN and +inf give unspecified values for num_best > 1, and no input takes an
 * access outside the buffers. Logits rows at steps >= I_b, and column zero_duration_id when
 * allow_skip is false, are never read into a result. Limits: num_best outside [1, 8] and
 * max_total outside [0, 1<<24] return SSNT_ERR_INVALID_ARG; duration_class_size > 64, rows
 * that do not fit LDS at that num_best (2 * NB * (row cells + 130) * 4 bytes beside 8-16 KiB of
 * class log-probs, NB = num_best rounded up to 1, 2, 4, 8) and backpointers of one utterance
 * beyond 32-bit offsets SSNT_ERR_UNSUPPORTED. `workspace` holds
 * ssnt_v2_nbest_align_workspace_size() bytes, 4-byte aligned: 0 (NULL workspace) while the
 * backpointer entries of one utterance (max_steps * row cells * NB, a byte each, 16 bits at
 * NB = 8) fit LDS; a missing, short or misaligned one returns SSNT_ERR_WORKSPACE; with
 * duration_class and duration both NULL no backpointers are kept and no workspace is needed. A
 * refused call writes nothing. Device pointers, asynchronous on `stream`. New: the reference only
 * searches this lattice with a pruned beam. */
size_t ssnt_v2_nbest_align_workspace_size(int batch, int max_steps, int max_total, bool test_mode,
                                          int num_best);
int ssnt_v2_nbest_align_device(const float *logits, const int *duration_table,
                               const int *input_length, const int *output_length, int batch,
                               int max_steps, int duration_class_size, int max_total,
                               int zero_duration_id, bool allow_skip, bool test_mode, int num_best,
                               float *log_prob, int *duration_class, int *duration, int *total,
                               void *workspace, size_t workspace_bytes, int *status, void *stream);

/* ---- duration paths drawn from the posterior of the v2 duration-class lattice (DESIGN.md 2.5,
 * 5.9). Forward filter, backward sample on F4's lattice (same inputs, states, windows and class
 * rule as ssnt_v2_fwd_bwd_device): the forward rows are F4's alpha, bit for bit; walking back from
 * the final total, each step draws its class among the D <= 64 terms entering the cell, in class
 * order, with one uniform number. `uniform` (B,K,T+1) is the randomness, K = num_samples in
 * [1, 64]: [b,k,t] chooses the class of step t, [b,k,T] the final total (band mode: forced to
 * O_b); each number is clamped to [0, 1 - 2^-24], NaN counts as 0. The library holds no generator
 * state: a call is a pure function of its arguments, and every output is an admissible class
 * sequence whatever `uniform` holds. log_prob (B,K) = the drawn sequence's log-probability, the
 * sequential f32 sum of logits[b,t,class_t] over t = 0..I_b-1 from 0.0f; duration_class (B,K,T)
 * (-1 for steps >= I_b); duration (B,K,T) = duration_table[class] (0 for steps >= I_b); total
 * (B,K) = the drawn final total. Each of the three may be NULL. An utterance with no admissible
 * path (I_b = 0, band mode with O_b > max_total, Z = 0, a length outside the tensor, which also
 * sets SSNT_ERR_BAD_LENGTH in `status`, or a negative duration, which sets SSNT_ERR_BAD_INDEX)
 * gets log_prob -inf, classes -1, durations 0 and total -1 for every sample. -inf logits are
 * legal; NaN and +inf are unspecified in value. Logits rows at steps >= I_b, and column
 * zero_duration_id when allow_skip is false, are never read into a result. Limits as F4:
 * duration_class_size > 64 and a row beyond LDS return SSNT_ERR_UNSUPPORTED; num_samples outside
 * [1, 64] and max_total outside [0, 1<<24] SSNT_ERR_INVALID_ARG. `workspace` holds
 * ssnt_v2_sample_align_workspace_size() bytes, 8-byte aligned (F4's forward rows and Z; the same
 * whichever outputs are requested); a missing, short or misaligned one returns
 * SSNT_ERR_WORKSPACE. A refused call writes nothing. Device pointers, asynchronous on `stream`
 * (two launches). New: the reference has no sampler. */
size_t ssnt_v2_sample_align_workspace_size(int batch, int max_steps, int max_total, bool test_mode,
                                           int num_samples);
int ssnt_v2_sample_align_device(const float *logits, const int *duration_table,
                                const int *input_length, const int *output_length,
                                const float *uniform, int batch, int max_steps,
                                int duration_class_size, int max_total, int zero_duration_id,
                                bool allow_skip, bool test_mode, int num_samples, float *log_prob,
                                int *duration_class, int *duration, int *total, void *workspace,
                                size_t workspace_bytes, int *status, void *stream);

/* ---- batched decode steps, device pointers (the reference FFI fixes v1 to B=1,
 * ssnt_tts_c/src/lib.rs:13; its Rust API takes B, src/lib.rs:121). max_beam_width = beam_width
 * as in every reference call site (ssnt_tts_c/src/lib.rs:82,217,342). ---- */
int ssnt_beam_search_decode_device(const float *h, const float *log_prob_history,
                                   const bool *is_finished, const int *t, const int *u,
                                   const int *input_length, int batch_size, int beam_width,
                                   int *prediction, float *log_probs, int *next_t, int *next_u,
                                   bool *next_is_finished, int *beam_branch, int *status,
                                   void *stream);
int ssnt_v2_beam_search_decode_device(const float *h, const float *log_prob_history,
                                      const bool *is_finished, const int *total_duration,
                                      const int *duration_table, const int *t, const int *u,
                                      const int *input_length, const int *output_length,
                                      int batch_size, int beam_width, int duration_class_size,
                                      int zero_duration_id, bool allow_skip, bool test_mode,
                                      int *prediction, float *log_probs, int *next_t,
                                      int *next_u, bool *next_is_finished,
                                      int *next_total_duration, int *beam_branch, int *status,
                                      void *stream);
int ssnt_tone_latent_beam_search_decode_device(const float *h, const float *log_prob_history,
                                               const bool *is_finished, const int *t,
                                               const int *u, const int *input_length,
                                               int batch_size, int beam_width,
                                               int tone_class_size, int empty_tone_id,
                                               int *prediction, float *log_probs, int *next_t,
                                               int *next_u, bool *next_is_finished,
                                               int *beam_branch, int *status, void *stream);

/* Fused multi-step decodes (the three entries below) pack next_t / next_u into 16 bits each:
 * max_steps > 32767 returns SSNT_ERR_UNSUPPORTED, and so does beam_width > 64 for v1 (v2 / tone
 * take any W*C through the LDS step kernel).
 * Fused T-step v1 decode over a (B,T,U,2) log-prob lattice: step s feeds each beam
 * h = lattice[b, u, t, :]; all beams start at t=u=0, log-prob 0. Per-step outputs (B,T,W);
 * best_beam_branch / best_t_history (B,T) = backtrace of slot 0 after the last step with
 * t_history = next_t (src/util.rs:20-33). */
int ssnt_lattice_beam_search_decode_device(const float *lattice, const int *input_length,
                                           int batch_size, int max_steps, int max_pos,
                                           int beam_width, int *prediction, float *log_probs,
                                           int *next_t, int *next_u, bool *next_is_finished,
                                           int *beam_branch, int *best_beam_branch,
                                           int *best_t_history, int *status, void *stream);

/* Fused multi-step v2 duration-class decode (BASELINE configs[4] "v2 path"). Every beam starts
 * at t = u = 0, log-prob 0, total_duration 0, not finished; step s runs the exact
 * ssnt_tts_v2_beam_search_decode step (src/v2.rs:221-339, max_beam_width = beam_width) on
 * h = logits[b, s] (W,D) and feeds its outputs back as the next state -- what the TF decode loop
 * does around the per-step op, one launch instead of max_steps. logits (B,T,W,D); per-step
 * outputs (B,T,W). Then, in the same launch, every final slot w is backtraced
 * (src/v2_util.rs:6-36 with final_branch = [0..W)): ordered_beam_branch (B,W,T), the class
 * chosen at each step of each path (path_prediction, B,W,T) and the duration it added
 * (duration, B,W,T; sums to the path's final total, the input of
 * ssnt_upsample_source_indexes). The three path outputs may be NULL. An utterance where no
 * candidate survives (the reference panics, src/v2.rs:292) sets SSNT_ERR_NO_CANDIDATE in
 * `status` and its outputs are unspecified. New: the reference steps once per call. */
int ssnt_v2_lattice_beam_search_decode_device(
    const float *logits, const int *duration_table, const int *input_length,
    const int *output_length, int batch_size, int max_steps, int beam_width,
    int duration_class_size, int zero_duration_id, bool allow_skip, bool test_mode,
    int *prediction, float *log_probs, int *next_t, int *next_u, bool *next_is_finished,
    int *next_total_duration, int *beam_branch, int *ordered_beam_branch, int *path_prediction,
    int *duration, int *status, void *stream);

/* Fused multi-step tone-latent decode (BASELINE configs[4] "tone_latent path"): as
 * ssnt_v2_lattice_beam_search_decode_device with the tone step (src/tone_latent.rs:144-234),
 * logits (B,T,W,C); path outputs ordered_beam_branch and path_prediction (the tone sequence of
 * each final slot, the input of the edit-distance evaluation) may be NULL. */
int ssnt_tone_latent_lattice_beam_search_decode_device(
    const float *logits, const int *input_length, int batch_size, int max_steps, int beam_width,
    int tone_class_size, int empty_tone_id, int *prediction, float *log_probs, int *next_t,
    int *next_u, bool *next_is_finished, int *beam_branch, int *ordered_beam_branch,
    int *path_prediction, int *status, void *stream);

/* Batched backtraces / utilities, device pointers. */
int ssnt_extract_best_beam_branch_device(const int *best_final_branch, const int *beam_branch,
                                         const int *t_history, int batch_size, int beam_width,
                                         int max_u, int *best_beam_branch, int *best_t_history,
                                         int *status, void *stream);
int ssnt_order_beam_branch_device(const int *final_branch, const int *beam_branch,
                                  int batch_size, int beam_width, int max_t,
                                  int *ordered_beam_branch, int *status, void *stream);
int ssnt_upsample_source_indexes_device(const int *duration, const int *output_length,
                                        int batch_size, int beam_width, int max_t, int max_u,
                                        int *upsampled_source_indexes, int *status,
                                        void *stream);
int ssnt_levenshtein_edit_distance_device(const int *a, const int *b, const int *a_lengths,
                                          const int *b_lengths, int batch_size, int max_length,
                                          int *distance, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SSNT_TTS_C_H */
