/*
 * mixemt_hip_bootstrap.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h (which defines mxm_coded,
 * mxm_em_state and the samples plan these entries build on), not meant to be included on its own.
 * Additions behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entries have a header and a binding table (_lib.BOOTSTRAP_SIGNATURES) of their own, as those of
 * mixemt_hip_samples_runs.h have; their refusals are pinned in tests/test_bootstrap_host.py.
 */
#ifndef MIXEMT_HIP_BOOTSTRAP_H
#define MIXEMT_HIP_BOOTSTRAP_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * A non-parametric bootstrap of the refinement EM (mixemt_hip_samples_finish.h) for the samples of a cohort: B replicates
 * per sample, one value for the whole batch, 2 <= B <= MXM_BOOTSTRAP_MAX (a cap, not a measurement: one column's
 * replicates sort in 4096 x 8 bytes = 32 KB of LDS).  A replicate is the sample's reduced matrix under row weights
 * resampled from the sample's own (a multinomial draw of N_s = sum of w over the sample's rows); the reference has no
 * counterpart.
 * c / row0_host / S / H, the tile plan and the refusals are those of mixemt_hip_samples_finish.h: the first two entries
 * below return -1 WITHOUT touching the device for c->qrec != NULL, c->R_rest != 0, a row0_host that is not ascending, an
 * empty sample, row0_host[S] != c->R, B outside [2, MXM_BOOTSTRAP_MAX], a workspace that is too small or not 16-byte
 * aligned, and (the loop) ld not one of 4, 8, 16 or an ncol_host[s] outside [0, ld]; mxm_bootstrap_summary refuses S
 * outside 1 .. 65535, B, ld and ncol_host in the same way.  Every per-replicate table is [S][B][...], replicate-major
 * inside a sample; the weights are wb[B * row0[s] + b * R_s + i] (row i of replicate b of sample s; c->R x B doubles).
 * A sample's outputs depend on its own rows, its tables and (seed, s_id[s], b) alone: the same bits whichever samples
 * share the batch, wherever the sample stands in it, and whatever B is (replicate b is the same under every B > b).  No
 * float atomics.
 * ws: mxm_bootstrap_workspace_bytes(n_tiles of mxm_samples_plan, S, B, ld) bytes on the device, 16-byte aligned: the
 * workspace of mixemt_hip_samples_finish.h, then the samples' prefix sums, totals and ids, then the counters of the rows
 * of min(B, 64) replicates (ld = 0 for mxm_bootstrap_weights).
 *   mxm_bootstrap_weights   wb <- the multinomial resamples of w.  w [R] (device) holds non-negative integers stored as
 *       doubles.  Checked ON THE DEVICE, because w is a device array and the entry only enqueues -- so these refusals are
 *       a non-zero state[s].error, not a return value: 1 for a weight that is negative, not an integer or not finite,
 *       2 for N_s = 0 or N_s >= 2^31; state[s].error = 0 otherwise (state [S] is required; its other fields are left
 *       alone).  A refused sample's wb is NaN throughout, and its neighbours are intact.
 *       s_id_host [S]: caller-chosen 32-bit sample ids; they go into the counter, so a sample's draws do not depend on its
 *       place in the batch.  Replicate b of sample s takes N_s draws; draw j uses word j mod 4 of Philox4x64-10 with key
 *       (seed, 0) and counter (j / 4 + 1, b, s_id[s], 0): multipliers 0xD2E7470EE14C6C93 / 0xCA5A826395121157, Weyl
 *       constants 0x9E3779B97F4A7C15 / 0xBB67AE8584CAA73B, ten rounds -- the stream of
 *       numpy.random.Philox(counter=[0, b, s_id, 0], key=[seed, 0]).random_raw(N_s) (numpy advances the counter before it
 *       generates, hence the + 1).  With t = (u * N_s) >> 64 (the high half of the 128-bit product) the drawn row is the
 *       number of the sample's rows whose inclusive prefix sum of w is <= t: integers only, a row of weight 0 is never
 *       drawn.  t takes each of its N_s values with probability within 2^-64 of 1 / N_s, a relative bias below
 *       N_s / 2^64 < 2^-33.  wb[...] = (double) the number of draws of the row: integer atomics, so the result does not
 *       depend on the order of the draws -- in LDS for a sample of at most MXM_BOOTSTRAP_LDS_ROWS rows, in 32-bit global
 *       counters in the workspace above it.  MXM_BOOTSTRAP_LDS_ROWS = 8192: the draw kernel keeps a 32-bit prefix sum and
 *       a 32-bit counter per row and nothing else in LDS, and 8192 x 8 bytes are the 64 KB a workgroup gets without the
 *       opt-in to more (two such workgroups still fit a CU's 160 KB).
 *       The prefix sums are built per sample on the device.  STREAM: the entry only enqueues; its host tables (row0_host,
 *       s_id_host) are copied to memory of the call's own first, as mixemt_hip_samples_finish.h describes, so they may be
 *       changed as soon as the call has returned.  Not meant to be captured: a replay would not upload them again.
 *   mxm_em_loop_samples_narrow_boot   mxm_em_loop_samples_narrow_runs (mixemt_hip_samples_runs.h) with the weights of
 *       entry (s, b) = wb + B * row0[s] + b * R_s in place of the sample's w: ONE workgroup per (sample, replicate), the
 *       same loop body, the same linearise pass into E for a sample of more than 9216 cells (E exactly c->R x ld doubles;
 *       NULL accepted when every sample has at most 9216 cells, refused otherwise), the same stop / resume / state
 *       contract with a finished replicate frozen while its siblings go on.  props_cur / ln_cur / ln_new [S][B][ld], state
 *       and state_host [S * B] (entry s * B + b).  Replicate b comes out with the bits -- ln_cur, ln_new, props_cur,
 *       iters, l1, done -- of mxm_em_loop_samples_narrow on that sample alone with w = its wb slice and the same start.
 *       mxm_em_loop_samples_narrow_boot blocks the calling thread (one read-back of the states per launch); state_host
 *       receives the final states.
 *   mxm_bootstrap_summary   one workgroup per (sample, column k < ncol_host[s]): x[s][b][k] = exp(ln_new[s][b][k]) is
 *       written out ([S][B][ld]; the pad columns are not touched), the B values are sorted in LDS with a bitonic network
 *       padded with +inf, and lo / hi [S][ld] are the quantiles at q_lo / q_hi: x_(i) + g * (x_(i+1) - x_(i)) with
 *       h = q * (B - 1), i = floor(h), g = h - i and the upper index clamped to B - 1 (numpy.quantile's "linear"), each
 *       operation rounded on its own.  mean [S][ld] is summed over the SORTED values in one fixed order (thread t: i = t,
 *       t + 256, ...; then the threads pairwise), sd [S][ld] two-pass over the same order with ddof = 1.  A replicate
 *       whose x is not finite, whose state (state [S * B], the loop's) has done = 0 or its error field set makes the
 *       column's four numbers NaN; flag[s] (int32 [S]) = 1 when that happened in any of the sample's columns, else 0.
 *       A replicate that the loop stopped at max_iter (done = 2) IS included, as run_em reports such a run's proportions:
 *       a caller who wants converged replicates only looks at the loop's states.
 *       q_lo / q_hi outside [0, 1] are refused.
 *       STREAM: the entry only enqueues.  ncol_host IS uploaded (into flag, which a last one-thread-per-sample kernel then
 *       overwrites with the flags), from memory of the call's own: class B like its siblings, not meant to be captured.
 */
#define MXM_BOOTSTRAP_MAX 4096
#define MXM_BOOTSTRAP_LDS_ROWS 8192

size_t mxm_bootstrap_workspace_bytes(int64_t n_tiles, int32_t S, int32_t B, int32_t ld);
int mxm_bootstrap_weights(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t B, const double *w, uint64_t seed,
                          const uint32_t *s_id_host, double *wb, mxm_em_state *state, void *ws, size_t ws_bytes, void *stream);
int mxm_em_loop_samples_narrow_boot(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *M,
                                    int32_t ld, const int32_t *ncol_host, const double *wb, double *props_cur, double *ln_cur,
                                    double *ln_new, mxm_em_state *state, double tol, int32_t max_iter, int32_t check_every,
                                    double *E, void *ws, size_t ws_bytes, void *stream, mxm_em_state *state_host);
int mxm_bootstrap_summary(int32_t S, int32_t B, int32_t ld, const int32_t *ncol_host, const double *ln_new,
                          const mxm_em_state *state, double q_lo, double q_hi, double *x, double *lo, double *hi, double *mean,
                          double *sd, int32_t *flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_BOOTSTRAP_H */
