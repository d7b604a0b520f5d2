/*
 * mixemt_hip_samples_finish.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h (which defines mxm_coded,
 * mxm_em_state and the samples plan these entries build on), not meant to be included on its own.
 * Additions behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entries have a header and a binding table (_lib.FINISH_SIGNATURES) of their own because the refusals of everything
 * mixemt_hip.h declares are pinned, entry by entry, in one table of the test suite; theirs are pinned beside their tests.
 */
#ifndef MIXEMT_HIP_SAMPLES_FINISH_H
#define MIXEMT_HIP_SAMPLES_FINISH_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The SECOND HALF of a cohort run for the samples of one batched EM -- bin/mixemt:298-323 once per sample: contributor
 * vote, column gather, refinement EM, read assignment.  c / row0_host / S / H as for mxm_em_loop_samples, and the same
 * refusals: every entry below returns -1 WITHOUT touching the device for c->qrec != NULL, c->R_rest != 0, a row0_host that
 * is not ascending, an empty sample, row0_host[S] != c->R, and (where it takes them) ld not one of 4, 8, 16, an
 * ncol_host[s] outside [0, ld], a column index outside [0, H), a contributor ordinal outside [0, ncol_host[s]).
 * A sample's outputs depend on its own rows alone: the same bits whichever samples share the batch and wherever it
 * stands in it.  No float atomics.  Still MXM_VERSION 603: additions only.
 * ws: mxm_samples_finish_workspace_bytes(n_tiles of mxm_samples_plan, S, ld) bytes on the device, 16-byte aligned (the
 * tile table and the per-sample tables, uploaded by every call, ordered on `stream`; ld = 0 for mxm_votes_samples).
 * STREAM: mxm_votes_samples, mxm_gather_columns_samples and mxm_assign_reads_samples only enqueue: the tables are copied
 * from pageable host memory of the call's own (the caller's *_host arrays are copied there first, so they are read before
 * the call returns whether they are pageable or pinned, and may be changed as soon as it has returned); the runtime has
 * taken those bytes when the copy call returns.  At the table sizes measured (a few hundred bytes, on a stream with work
 * pending: profiles/streams/README.md) the copies are only enqueued too; HIP lets a runtime hold a larger pageable upload
 * until the stream has got there, which changes the call's host time, never its results or their order.  The loop entry
 * is the exception: see its own paragraph.  None of the four is meant to be captured: a replay would not upload the
 * tables again.
 *   mxm_votes_samples   assemble.py:115-123 per sample, over the concatenated records (one workgroup per tile of the
 *       plan, then one per sample): best[r] = first index of max_h (ln_props[s][h] + M[r][h]) for the rows of sample s (one
 *       run: the row normaliser drops out, see mxm_row_argmax_votes_coded); votes[s][h] = sum of w[r] (NULL: 1) over the
 *       sample's rows with best[r] == h, in ascending row order; counts[s][h] (nullable) their number (stats.py:39-40);
 *       first[s][h] = the smallest such row counted from the sample's first row, or R_s when there is none.  lse[r]
 *       (nullable; needs props [S][H] = exp(ln_props) and rowmax [R]) = rowmax[r] + log sum_h props[s][h] P[r][h], the row
 *       normaliser of mxm_em_step_coded.  A row without a usable record (ndist outside 1 .. 1024) is never
 *       dereferenced: best[r] = -1, its sample's votes are NaN and state[s].error = 1 (state nullable).
 *   mxm_gather_columns_samples   preprocess.py:247-251 per sample: out[r][i] = M[r][cols_host[s][i]] for i < ncol_host[s]
 *       (from the records' log tables, as mxm_gather_columns_coded), -inf for ncol_host[s] <= i < ld.  out [R][ld];
 *       cols_host [S][ld] HOST int32, ascending haplogroup index per sample as reduce_em_matrix keeps them.
 *   mxm_em_loop_samples_narrow   em.py:126-143 for every reduced sample (bin/mixemt:311-320): ONE workgroup per sample
 *       with the whole loop inside it -- no grid barrier, no co-residency requirement.  M [R][ld] (the gather's output),
 *       props_cur / ln_cur / ln_new [S][ld], state [S]: stop / resume / state as mxm_em_loop (ln_cur = log theta_k,
 *       ln_new = log theta_{k+1}); a launch runs at most check_every iterations per unfinished sample and the host
 *       re-launches until every state is done.  e = exp(M - rowmax) is formed once per launch, in LDS for a sample of up
 *       to 9216 cells (R_s x ncol), else in E [R][ld] (nullable when every sample fits).  Samples with ncol 0 are left alone.
 *       mxm_em_loop_samples_narrow blocks the calling thread (one read-back of the states per launch); state_host[S]
 *       receives the final states.
 *   mxm_assign_reads_samples   assemble.py:284-334 per row under its sample's columns: X_c = (ln_theta[s][c] + M[r][c]) -
 *       (rowmax_r + log sum_c props[s][c] exp(M[r][c] - rowmax_r)) as mxm_em_step documents it -- redone in log space with
 *       a max shift where that sum is below 2^-960 or not finite, as mxm_em_step_coded does -- (or minus lse[r] when lse is
 *       given: the first EM's full-width normaliser, for the unrefined assignment), v_c = X_c - log_props[s][c] (the
 *       returned theta_{k+1}); assigned[r] = perm_host[s][c] of the best c when it beats the runner-up by log_min_fold,
 *       else -1; exactly equal values: the later column wins, as in mxm_assign_reads.  Samples with ncol <= 1 get 0
 *       throughout.  post (nullable) [R][ld] receives X (-inf in the pad columns).
 */
size_t mxm_samples_finish_workspace_bytes(int64_t n_tiles, int32_t S, int32_t ld);
int mxm_votes_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const double *w,
                      const double *ln_props, const double *props, const double *rowmax, int32_t *best, double *votes,
                      int64_t *counts, int64_t *first, double *lse, mxm_em_state *state, void *ws, size_t ws_bytes, void *stream);
int mxm_gather_columns_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const int32_t *cols_host,
                               const int32_t *ncol_host, int32_t ld, double *out, void *ws, size_t ws_bytes, void *stream);
int mxm_em_loop_samples_narrow(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const double *M, int32_t ld,
                               const int32_t *ncol_host, const double *w, double *props_cur, double *ln_cur, double *ln_new,
                               mxm_em_state *state, double tol, int32_t max_iter, int32_t check_every, double *E, void *ws,
                               size_t ws_bytes, void *stream, mxm_em_state *state_host);
int mxm_assign_reads_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const double *M, int32_t ld,
                             const int32_t *ncol_host, const int32_t *perm_host, const double *ln_theta, const double *props,
                             const double *log_props, const double *lse, double log_min_fold, int32_t *assigned, double *post,
                             void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_SAMPLES_FINISH_H */
