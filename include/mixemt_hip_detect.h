/*
 * mixemt_hip_detect.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h (which defines mxm_em_state), not
 * meant to be included on its own.
 * Additions behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entries have a header and a binding table (_lib.DETECT_SIGNATURES) of their own, as those of mixemt_hip_bootstrap.h and
 * mixemt_hip_support.h have; their refusals are pinned in tests/test_detect_host.py.
 */
#ifndef MIXEMT_HIP_DETECT_H
#define MIXEMT_HIP_DETECT_H

#ifdef __cplusplus
extern "C" {
#endif

/*
 * What follows the contributor vote when the DETECTION itself is bootstrapped (assign.detect_many): the batch's entries are
 * (sample, replicate) pairs, so the candidate rule and the variant check read and write device tables only.  The reference
 * has no counterpart.  Neither entry needs a workspace; no float atomics; an entry's outputs depend on its own rows of the
 * tables alone: the same bits alone, first or last in a batch.
 *   mxm_detect_candidates   assemble.py:115-123 and the sort of :85-86 per entry e of E, ONE workgroup each.
 *       votes [E][H] double, first [E][H] int64   as mxm_votes_samples leaves them (device)
 *       rows_host [E] int64   HOST: R_e, the entry's number of rows
 *       props [E][H] double   theta_{k+1}, the proportions the contributor table reports (device)
 *       state [E]             mxm_em_state of the entries' loop (device; nullable)
 *       cand [E][ld] int32, ncand [E] int32, cprop [E][ld] double   device; ld one of 4, 8, 16, 32, 64
 *       Haplogroup h is a candidate when first[e][h] < R_e (it won a row: the reference's vote table holds no other) and
 *       votes[e][h] >= min_reads, compared in doubles (a NaN vote is no candidate).  cand[e][0 .. ncand[e]) are the
 *       candidates in CHECKING order -- descending props[e][h], equal proportions by ascending first (what Python's stable
 *       sort(reverse=True) leaves of the first-seen order; should two firsts be equal too, by ascending h) -- and cprop their
 *       proportions; slots at and past ncand[e] are not written.  ncand[e] is the number of candidates found, also when it
 *       exceeds ld: row cand[e] / cprop[e] is then unspecified and must not be read.  ncand[e] = -1 when any vote of the
 *       entry is NaN (a poisoned sample), state[e].error != 0 or state[e].done == 0, or a candidate's proportion is NaN.
 *       Refused with -1 before any HIP call: E < 0; H < 1; ld not one of 4, 8, 16, 32, 64; votes, first, rows_host, props,
 *       cand, ncand or cprop NULL; a negative rows_host[e].  E == 0: 0, nothing launched.
 *   mxm_check_variants_entries   mxm_check_variants_samples (mixemt_hip_var_check.h: the same tree tables, thresholds and
 *       decisions, the same kernel body) for E entries whose candidate lists are ON THE DEVICE and whose pileups may be shared:
 *       counts [T][L][16]     T pileup tables (device, 16-byte aligned)
 *       table_of_host [E] int32   HOST: entry e is checked against table table_of_host[e]
 *       cand [E][ld], ncand [E]   device int32, as mxm_detect_candidates leaves them
 *       keep [E][ld] uint8, n_uniq / n_found [E][ld] int32 (both nullable), flag [E] int32   device
 *       flag[e] = 0: the entry was checked (ncand[e] == 0: trivially, nothing else written); 1: ncand[e] < 0 or > ld; 2: a
 *       candidate index outside [0, H) (the host refusal of the samples entry cannot be made for device lists).  An entry
 *       flagged 1 or 2 is left alone: nothing of its rows is written.  ONE workgroup per entry.
 *       Refused with -1 before any HIP call: E < 0; T < 1 (with E > 0); ld not one of 4, 8, 16, 32, 64; table_of_host, cand,
 *       ncand or flag NULL; a table_of_host[e] outside [0, T); counts, key_ptr, key or keep NULL (site / site_key with
 *       n_sites > 0); counts not 16-byte aligned; L <= 0 or n_sites < 0; H < 1; max_pos >= L; L > MXM_VAR_CHECK_MAX_L.
 *       E == 0: 0, nothing launched.
 * STREAM: both entries only enqueue.  The host table (rows_host, table_of_host) goes into stream-ordered memory of the
 * call's own through a pageable copy of the call's own, as mixemt_hip_var_check.h describes: it is read before the call
 * returns and may be changed as soon as it has.  Not meant to be captured: a replay would not upload it again.
 */
int mxm_detect_candidates(const double *votes, const int64_t *first, const int64_t *rows_host, const double *props,
                          const mxm_em_state *state, int32_t E, int32_t H, double min_reads, int32_t ld, int32_t *cand,
                          int32_t *ncand, double *cprop, void *stream);
int mxm_check_variants_entries(const uint32_t *counts, int32_t T, int64_t L, const int32_t *key_ptr, const int32_t *key, int32_t H,
                               const int32_t *site, const int32_t *site_key, int32_t n_sites, int64_t max_pos,
                               const int32_t *table_of_host, int32_t E, const int32_t *cand, const int32_t *ncand, int32_t ld,
                               double min_var_reads, double frac_var_reads, double var_fraction, int32_t has_var_count,
                               int32_t var_count, uint8_t *keep, int32_t *n_uniq, int32_t *n_found, int32_t *flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_DETECT_H */
