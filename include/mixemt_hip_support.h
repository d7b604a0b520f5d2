/*
 * mixemt_hip_support.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h (which defines mxm_coded,
 * mxm_em_state and the samples plan these entries build on), not meant to be included on its own.
 * Additions behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entries have a header and a binding table (_lib.SUPPORT_SIGNATURES) of their own, as those of
 * mixemt_hip_bootstrap.h have; their refusals are pinned in tests/test_support_host.py.
 */
#ifndef MIXEMT_HIP_SUPPORT_H
#define MIXEMT_HIP_SUPPORT_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Nested-model fits of the refinement EM (mixemt_hip_samples_finish.h) for the samples of a cohort: B fits per sample, one
 * value for the whole batch, 1 <= B <= MXM_SUPPORT_MAX_FITS (a cap, not a measurement: all non-empty subsets of 8 columns
 * are 255).  A fit is a SUBSET of the columns of the sample's reduced matrix M [R][ld], given as a 32-bit mask (bit k =
 * column k) in mask_host [S][B] (host, uint32); its maximised log-likelihood answers whether the data support a
 * contributor.  The reference has no counterpart.  Mask 0 marks an unused slot: its outputs and its state are left alone,
 * so samples with different numbers of fits share one B.
 * c / row0_host / S / H, the tile plan and the refusals are those of mixemt_hip_samples_finish.h: the two entries below
 * return -1 WITHOUT touching the device for c->qrec != NULL, c->R_rest != 0, a row0_host that is not ascending, an empty
 * sample, row0_host[S] != c->R, ld not one of 4, 8, 16, an ncol_host[s] outside [0, ld], a workspace that is too small or
 * not 16-byte aligned, B outside [1, MXM_SUPPORT_MAX_FITS] and a mask with a bit at or above ncol_host[s].  Every per-fit
 * table is [S][B][ld], fit-major inside a sample, as in mixemt_hip_samples_runs.h.  A fit's outputs depend on its sample's
 * rows, its mask and its own tables alone: the same bits whichever samples and fits share the batch and wherever the
 * sample stands in it.  No float atomics.
 * ws: mxm_support_workspace_bytes(n_tiles of mxm_samples_plan, S, B, ld) bytes on the device, 16-byte aligned: the
 * workspace of mixemt_hip_samples_finish.h, then the S x B masks.
 *   mxm_em_loop_samples_narrow_masks   mxm_em_loop_samples_narrow_runs (mixemt_hip_samples_runs.h) with mask_host as one
 *       more argument: ONE workgroup per (sample, fit), the whole loop inside it, the same loop body.  A column outside the
 *       fit's mask is treated exactly as a pad column (k >= ncol) is: its e is 0 and it takes no part in the row maximum of
 *       the linearise step (the row shift is the maximum over the MASKED-IN columns), p = 0 and ln = -inf, never updated;
 *       its ln_cur / ln_new come out -inf and its props_cur 0.  Fit (s, b) comes out with the bits -- ln_cur, ln_new,
 *       props_cur, iters, l1, done -- of mxm_em_loop_samples_narrow on that sample alone with its matrix gathered at just
 *       the masked-in columns, in the same ascending order, and the same start, whatever ld either call uses (an absent
 *       column contributes fma(0, 0, z) = z exactly).
 *       E: the shift depends on the mask, so the fits of a sample of more than 9216 cells (judged on R_s x ncol_host[s])
 *       cannot share one linearised copy: E is exactly B x c->R x ld doubles, fit (s, b) owns the slice at
 *       (B * row0[s] + b * R_s) * ld (R_s x ld doubles; the layout wb has in mixemt_hip_bootstrap.h) and writes and
 *       re-reads only that.  NULL accepted when every sample has at most 9216 cells, refused otherwise.
 *       props_cur / ln_cur / ln_new [S][B][ld], state and state_host [S * B] (entry s * B + b); the stop / resume / state
 *       / check_every contract is the runs entry's, a finished fit frozen while its siblings go on.
 *       mxm_em_loop_samples_narrow_masks blocks the calling thread (one read-back of the states per launch); state_host
 *       receives the final states.
 *   mxm_loglik_samples_masks   ll[s][b] = sum over the sample's rows of w_r (m_r + log sum_{k in mask} p_k exp(M_rk - m_r))
 *       with m_r the maximum of M_rk over the masked-in columns and p = exp(ln_props[s][b][k]) (ln_props [S][B][ld]: whatever
 *       the caller passes, e.g. the loop's ln_new).  Where the linear sum is below 2^-960 or not finite the row is redone
 *       in log space with a max shift of ln p_k + M_rk (the rule mixemt_hip.h gives for the row normalisers).  A row with
 *       w_r == 0 is skipped; w = NULL means every w_r is 1; a row with w_r != 0 and no finite masked-in cell makes the fit's
 *       ll -inf.  ONE workgroup per (sample, fit): thread t takes rows t, t + 256, ... in ascending order, the wave sums are
 *       fixed-order ladders and the waves are summed in ascending order.  ll [S][B] (an unused slot's is left alone);
 *       n_eff [S] = sum of w over the sample, in the same fixed order.  Reads M [R][ld] and needs no E.
 *       STREAM: the entry only enqueues; its host tables (row0_host, ncol_host, mask_host) are copied to memory of the
 *       call's own first, as mixemt_hip_samples_finish.h describes, so they may be changed as soon as the call has
 *       returned.  Not meant to be captured: a replay would not upload them again.
 */
#define MXM_SUPPORT_MAX_FITS 256

size_t mxm_support_workspace_bytes(int64_t n_tiles, int32_t S, int32_t B, int32_t ld);
int mxm_em_loop_samples_narrow_masks(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *M,
                                     int32_t ld, const int32_t *ncol_host, const uint32_t *mask_host, const double *w,
                                     double *props_cur, double *ln_cur, double *ln_new, mxm_em_state *state, double tol,
                                     int32_t max_iter, int32_t check_every, double *E, void *ws, size_t ws_bytes, void *stream,
                                     mxm_em_state *state_host);
int mxm_loglik_samples_masks(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *M,
                             int32_t ld, const int32_t *ncol_host, const uint32_t *mask_host, const double *w,
                             const double *ln_props, double *ll, double *n_eff, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_SUPPORT_H */
