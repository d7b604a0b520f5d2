/*
 * mixemt_hip_samples_runs.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h (which defines mxm_coded,
 * mxm_em_state and the samples plan these entries build on), not meant to be included on its own.
 * Additions behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entries have a header and a binding table (_lib.SAMPLES_RUNS_SIGNATURES) of their own, as those of
 * mixemt_hip_samples_finish.h have; their refusals are pinned in tests/test_samples_runs_host.py.
 */
#ifndef MIXEMT_HIP_SAMPLES_RUNS_H
#define MIXEMT_HIP_SAMPLES_RUNS_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The second half of a cohort run (mixemt_hip_samples_finish.h) for samples whose EM ran SEVERAL times (mixemt's -M,
 * em.py:119-161): B runs per sample, one value for the whole batch, 2 <= B <= MXM_SAMPLES_RUNS_MAX (a cap, not a
 * measurement).  B = 1 is refused: the entries of mixemt_hip_samples_finish.h are the one-run form.
 * c / row0_host / S / H, the tile plan and the refusals are those of mixemt_hip_samples_finish.h: every entry below
 * returns -1 WITHOUT touching the device for c->qrec != NULL, c->R_rest != 0, a row0_host that is not ascending, an
 * empty sample, row0_host[S] != c->R, B outside [2, MXM_SAMPLES_RUNS_MAX], and (where it takes them) ld not one of 4, 8,
 * 16, an ncol_host[s] outside [0, ld], a contributor ordinal outside [0, ncol_host[s]), a workspace that is too small or
 * not 16-byte aligned.  Every per-run table is [S][B][...], run-major inside a sample.
 * A sample's outputs depend on its own rows and tables alone: the same bits whichever samples share the batch and
 * wherever it stands in it.  No float atomics.
 * ws: mxm_samples_runs_workspace_bytes(n_tiles of mxm_samples_plan, S, B, ld) bytes on the device, 16-byte aligned (the
 * tile table and the per-sample tables, uploaded by every call, ordered on `stream`; ld = 0 for mxm_votes_samples_runs).
 * STREAM: mxm_votes_samples_runs and mxm_assign_reads_samples_runs only enqueue; their host tables are copied to memory
 * of the call's own first, as mixemt_hip_samples_finish.h describes, so they may be changed as soon as the call has
 * returned.  The loop entry is the exception: see its own paragraph.  None of the three is meant to be captured.
 *   mxm_votes_samples_runs   assemble.py:115-123 over the folded posterior of em.py:145-161 (one workgroup per tile of
 *       the plan, then one per sample).  For a row r of sample s: lse_b = the row normaliser under run b's props /
 *       ln_props [S][B][H] (rowmax[r] + log sum_h props[s][b][h] P[r][h], redone in log space where that sum is below
 *       2^-960 or not finite, as mxm_em_step_coded does); v_h = the fold over b, in run order starting from run 0, of
 *       logaddexp((ln_props[s][b][h] + M[r][h]) - lse_b); best[r] = the first index of the maximum, a NaN winning
 *       (numpy.argmax) -- the arithmetic of mxm_row_argmax_votes_coded with n_runs = B on the sample's own records, row
 *       for row (the - log B of em.py:161 shifts every column alike and drops out).  votes / counts (nullable) / first /
 *       state (nullable) as mxm_votes_samples.  lse (nullable) [R][B] receives the lse_b: the unrefined assignment's
 *       normalisers.  props, ln_props and rowmax are all required.  A row without a usable record (ndist outside
 *       1 .. 1024) is never dereferenced: best[r] = -1, its lse NaN, its sample's votes NaN and state[s].error = 1.
 *   mxm_em_loop_samples_narrow_runs   em.py:126-143 once per (sample, run) on the sample's reduced matrix M [R][ld]:
 *       ONE workgroup per (sample, run) with the whole loop inside it.  props_cur / ln_cur / ln_new [S][B][ld], state and
 *       state_host [S * B] (entry s * B + b).  Stop / resume / state as mxm_em_loop_samples_narrow; a finished run is
 *       frozen while its siblings go on.  Run b of sample s comes out with the same bits -- ln_cur, ln_new, props_cur,
 *       iters, l1, done -- as that sample through mxm_em_loop_samples_narrow started from the same proportions: the two
 *       kernels share one loop body.  e = exp(M - rowmax) does not depend on the run: for a sample of more than 9216
 *       cells (R_s x ncol) it is formed ONCE per call by a pass of its own into E, which the B workgroups of the sample
 *       then only read; a smaller sample is linearised in each workgroup's LDS and never touches E.
 *       E: exactly c->R x ld doubles ([R][ld], the layout of M); NULL is accepted when every sample has at most 9216
 *       cells, and refused otherwise.  Samples with ncol 0 are left alone.
 *       mxm_em_loop_samples_narrow_runs blocks the calling thread (one read-back of the states per launch); state_host
 *       receives the final states.
 *   mxm_assign_reads_samples_runs   assemble.py:284-334 per row under the folded posterior of its sample's B runs.
 *       ln_theta / props [S][B][ld] (log theta_k of run b and its exponential), log_props [S][ld] (the log of the
 *       FOLDED proportions the caller reports: run_em's geometric mean).  Per row: L_b = the row normaliser of run b
 *       exactly as mxm_assign_reads_samples forms it for one run, its log-space redo of an underflowing sum included -- or
 *       lse[r * B + b] when lse [R][B] is given (the first EM's full-width normalisers, for the unrefined assignment);
 *       X_c = the fold over b, in run order, of logaddexp((ln_theta[s][b][c] + M[r][c]) - L_b), then + (-log B) as ONE
 *       addition (mxm_add_scalar in the per-sample path); v_c = X_c - log_props[s][c].  Best / runner-up /
 *       log_min_fold / exactly equal values to the later column / perm_host / ncol <= 1 as mxm_assign_reads_samples.
 *       post (nullable) [R][ld] receives X (-inf in the pad columns).
 */
#define MXM_SAMPLES_RUNS_MAX 64

size_t mxm_samples_runs_workspace_bytes(int64_t n_tiles, int32_t S, int32_t B, int32_t ld);
int mxm_votes_samples_runs(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *w,
                           const double *ln_props, const double *props, const double *rowmax, int32_t *best, double *votes,
                           int64_t *counts, int64_t *first, double *lse, mxm_em_state *state, void *ws, size_t ws_bytes,
                           void *stream);
int mxm_em_loop_samples_narrow_runs(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *M,
                                    int32_t ld, const int32_t *ncol_host, const double *w, double *props_cur, double *ln_cur,
                                    double *ln_new, mxm_em_state *state, double tol, int32_t max_iter, int32_t check_every,
                                    double *E, void *ws, size_t ws_bytes, void *stream, mxm_em_state *state_host);
int mxm_assign_reads_samples_runs(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *M,
                                  int32_t ld, const int32_t *ncol_host, const int32_t *perm_host, const double *ln_theta,
                                  const double *props, const double *log_props, const double *lse, double log_min_fold,
                                  int32_t *assigned, double *post, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_SAMPLES_RUNS_H */
