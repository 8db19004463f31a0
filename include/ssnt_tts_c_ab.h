/*
 * ssnt_tts_c_ab.h -- extra symbols of the A/B build of libssnt_tts_c (`make lib-ab`:
 * ssnt-tts-rust_amd/lib/ab/libssnt_tts_c_ab.so, compiled -DSSNT_AB). Tests and tuning tools only.
 *
 * The product library (include/ssnt_tts_c.h) dispatches every call by its shape alone and holds
 * no process-wide mutable state. The A/B build adds the knobs below, each PROCESS-WIDE: one
 * caller flipping one changes the kernel every other thread's next call runs. They exist to
 * force a kernel the default dispatch would not pick for a shape (parity of every kernel on
 * the same inputs) and to time alternatives. Every form they select is bit-identical to the
 * default.
 * The workspace size ssnt_fwd_bwd_workspace_size() returns holds for the knobs' values at the
 * time of the query.
 */
#ifndef SSNT_TTS_C_AB_H
#define SSNT_TTS_C_AB_H

#include <stddef.h>

#include "ssnt_tts_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* forward-backward kernel: 0 default dispatch, 1 two-wave kernel, 2 segmented kernel at every U
 * it takes; env SSNT_FWD_BWD_KERNEL=simple selects 1 at first use */
int ssnt_fwd_bwd_set_variant(int variant);
/* segmented kernel: positions per lane (1 or 2) and the workgroup split (-1 auto, 0, 1) */
int ssnt_fwd_bwd_wide_lanes(int k);
int ssnt_fwd_bwd_wide_split(int mode);
/* segmented kernel, split form: the downstream workgroup's first compute wave sleeps `sleeps`
 * x s_sleep 127 per block (0 default), so the receiver runs a whole ring ahead (race test) */
int ssnt_fwd_bwd_wide_lag(int sleeps);
/* v2 posterior sampler: steps per memory round trip of the walk (0 by dmax, 1 one gather per
 * step, 2, 4; the deeper forms apply while steps * dmax <= 63) and the launches that run (bit 0
 * the forward sweep, bit 1 the walk; 3 default: timing one launch over a workspace an earlier full
 * call left) */
int ssnt_v2_sample_align_form(int cone, int launches);
/* expected path cost: the transition rows of one chunk of the sweep for a shape (host query; 0 for
 * a max_pos it does not take), and the launches that run (bit 0 the sweep, bit 1 the gradient
 * launch; 3 default: timing one launch over a workspace an earlier full call left) */
int ssnt_expected_cost_chunk_rows(int max_pos, int has_obs);
int ssnt_expected_cost_launches(int mask);
/* duration posterior: the step rows of one staged chunk (low 16 bits) and the positions of one
 * workgroup's tile (the bits above) of the duration launch for a shape, the transition rows of one
 * chunk of its sweeps, which stage no cost (host queries; 0 for a shape the call does not take),
 * and the launches that run (bit 0 the sweeps, bit 1 the duration launch; 3 default: timing one
 * launch over a workspace an earlier full call left) */
int ssnt_duration_posterior_block(int max_pos, int num_bins, int has_obs);
int ssnt_duration_posterior_sweep_rows(int max_pos, int has_obs);
int ssnt_duration_posterior_launches(int mask);
/* expected duration-path cost: the sweep steps of one staged chunk for a class count (host query;
 * 0 beyond 64 classes), and the launches of the full call that run (bit 0 the sweeps, bit 1 the
 * gradient launch; 3 default: timing one launch over a workspace an earlier full call left) */
int ssnt_v2_expected_cost_chunk_steps(int duration_class_size);
int ssnt_v2_expected_cost_launches(int mask);
/* per-step reference symbols: host staging 0 copies / 1 zero-copy; completion 0 stream
 * synchronise / 1 hipStreamWriteValue32 word / 2 flag kernel; both return the previous mode */
int ssnt_set_host_staging(int mode);
int ssnt_set_host_sync(int mode);
/* diagnostics: per-phase clock of the per-step symbols, empty-kernel launch + sync floor, and the
 * in-kernel stamps of the diagnostic build (make lib-diag; -1 elsewhere) */
int ssnt_diag_step_clock(int enable, double *out);
int ssnt_diag_null_launch(int reps, double *out);
/* diagnostics of the host-pointer layer: the staging plan of the calling thread's last
 * host-pointer call ("zero-copy", "copy" or "direct"; thread-local, returns the string's length),
 * and the number of live per-thread host contexts in the process (a context is counted from its
 * thread's first host-pointer call until that thread exits) */
int ssnt_diag_host_path(char *buf, size_t len);
int ssnt_diag_host_contexts(void);
int ssnt_diag_read(void *host, size_t bytes);
int ssnt_diag_decode_read(void *host, size_t bytes);

#ifdef __cplusplus
}
#endif

#endif /* SSNT_TTS_C_AB_H */
