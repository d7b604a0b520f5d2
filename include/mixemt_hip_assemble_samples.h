/*
 * mixemt_hip_assemble_samples.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h, not meant to be included
 * on its own.
 * Two additions behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entries have a header and a binding table (_lib.ASSEMBLE_SAMPLES_SIGNATURES) of their own because three things about
 * everything the four older headers declare are pinned by tables of the test suite that name those headers: the headers'
 * names are the union of the three older binding tables, every one of their device buffers is guard-banded in one list,
 * and their 51 stream-taking entries are classified in one table of stream cases.  The refusals, the guard-banded calls and
 * the stream cases of these two entries are pinned beside their own tests (tests/test_assemble_samples_host.py,
 * tests/test_gpu_guarded_assemble_samples.py, tests/test_gpu_stream_contract_assemble_samples.py).
 */
#ifndef MIXEMT_HIP_ASSEMBLE_SAMPLES_H
#define MIXEMT_HIP_ASSEMBLE_SAMPLES_H

#ifdef __cplusplus
extern "C" {
#endif

/* participants a sample may have: an owner in a newvar word is an int8 */
#define MXM_ASSEMBLE_SAMPLES_MAX_USE 127

/*
 * mxm_new_variants -- find_new_variants, assemble.py:469-501 -- for S samples in ONE launch over strict consensus rows
 * that stay on the device (a thread per (sample, position); integer atomics only).
 *   cons [n_rows][ld]   DEVICE uint8: the rows mxm_consensus wrote (strict), one per label of the cohort; ld >= ref_len
 *   use_host [use_ptr_host[S]], use_ptr_host [S + 1]   HOST int32: the participants of sample s are the rows
 *                       use_host[use_ptr_host[s] .. use_ptr_host[s + 1]); an EMPTY range: the sample takes no part -- its
 *                       newvar row is set to all -1 and its counter is left alone
 *   newvar [S][ref_len] DEVICE uint32: the word of mxm_new_variants, four int8 owners (A C G T; -1 none); owner k is the
 *                       k-th participant OF THAT SAMPLE
 *   n_new [S]           DEVICE uint32, ADDED to: the owners written for the sample
 * Per sample the rules of mxm_new_variants: a position where any participating consensus of the sample is N, '-' or X is
 * skipped (all -1); a base is owned when exactly one participant of the sample has it.
 * The host tables are validated on the host, uploaded by the call into stream-ordered memory of its own (hipMallocAsync /
 * hipFreeAsync on `stream`: not meant to be captured) through a pageable copy of the call's own, and read before the call
 * returns.  The call only enqueues on `stream`; nothing is waited for.
 * Refused with -1 WITHOUT touching the device: S < 0; ref_len < 0, ld < ref_len or n_rows < 0; use_ptr_host NULL;
 * use_ptr_host[0] < 0 or a use_ptr_host that decreases; more than 127 participants in a sample; use_host NULL with
 * participants; a row outside [0, n_rows); cons, newvar or n_new NULL.
 * S == 0, ref_len == 0, or no sample with participants: 0, nothing launched.
 */
int mxm_new_variants_samples(const uint8_t *cons, int64_t ld, int32_t n_rows, const int32_t *use_host,
                             const int32_t *use_ptr_host, int32_t S, int64_t ref_len, uint32_t *newvar, uint32_t *n_new,
                             void *stream);

/*
 * mxm_extend_assign -- assign_reads_from_new_vars, assemble.py:504-546 -- for S samples whose alignments lie in ONE set of
 * columns, in one walk and one move launch.  Labels are GLOBAL: every (sample, contributor) has a label of its own.
 *   cols                as mxm_extend_assign: a HOST struct of DEVICE arrays, with frag and n_frag
 *   aln_sample [n_aln]  DEVICE int32: the sample of each alignment
 *   label, joined [n_aln]   DEVICE int32, updated in place
 *   unassigned_host [S] HOST int32: the GLOBAL label of the sample's 'unassigned'; -1: the sample is frozen -- none of its
 *                       alignments is walked or moved
 *   use_host, use_ptr_host   HOST int32, as mxm_new_variants_samples; here they map owner k of sample s's newvar row to the
 *                       global label use_host[use_ptr_host[s] + k]
 *   n_labels            the number of global labels: every entry of use_host and every unassigned_host[s] >= 0 lies in
 *                       [0, n_labels)
 *   round, min_mq, min_bq   as mxm_extend_assign
 *   newvar [S][ref_len] DEVICE uint32 (mxm_new_variants_samples); an owner >= the sample's participants is no owner
 *   frag_state [n_frag] DEVICE int32 scratch, reset by the call
 *   moved_owner [n_aln] DEVICE int32, nullable: the GLOBAL label an alignment moved to, or -1 -- the labels of the next
 *                       additive pileup as they are
 *   n_moved [S]         DEVICE uint32, ADDED to: the sample's alignments that moved
 * Walk: a wave per alignment with label == unassigned_host[its sample] and mapq >= min_mq, with the filters and the quality
 * rule of mxm_extend_assign; a base is looked up in its own sample's newvar row (read from global memory: S rows of ref_len
 * words are served by L2).  The state folded into frag_state[f] is the GLOBAL label of the owner, or empty, or conflict: a
 * function of the SET of owners, so a fragment index that alignments of two samples share and that both show an owner for
 * ends in conflict.  Move: an alignment with label == unassigned_host[its sample] (whatever its mapq) whose fragment has ONE
 * owner that is a participant OF ITS OWN SAMPLE takes that label and joined = round; no alignment ever moves to another
 * sample's contributor.  Integer atomics only: the same result for any order.
 * The host tables are validated on the host, uploaded by the call into stream-ordered memory of its own and read before the
 * call returns.  HOST, blocking: like mxm_extend_assign this entry waits for its work on `stream` and reads the error word
 * back before it returns.
 * Returns 0; -1 (a refusal, or at run time the FIRST alignment with a fragment index outside [0, n_frag) or with an
 * aln_sample outside [0, S)); -2 (a HIP error); -4 (the first alignment whose CIGAR runs past its sequence or holds an
 * unknown operation).
 * Refused with -1 WITHOUT touching the device: cols NULL, n_aln < 0 or > 2^31 - 1, a column of cols missing; S < 0,
 * n_labels < 0, ref_len < 0, n_frag < 0 or round < 0; unassigned_host or use_ptr_host NULL with S > 0; use_ptr_host[0] < 0
 * or a use_ptr_host that decreases; more than 127 participants in a sample; use_host NULL with participants; an entry of
 * use_host or a non-negative unassigned_host[s] outside [0, n_labels); with n_aln > 0: label, joined, frag, aln_sample or
 * n_moved NULL, frag_state NULL with n_frag > 0, newvar NULL with S > 0 and ref_len > 0.
 * n_aln == 0: 0, nothing launched.
 */
int mxm_extend_assign_samples(const mxm_aln_columns *cols, const int32_t *aln_sample, int32_t *label, int32_t *joined,
                              const int32_t *unassigned_host, const int32_t *use_host, const int32_t *use_ptr_host,
                              int32_t S, int32_t n_labels, int32_t round, int32_t min_mq, int32_t min_bq,
                              const uint32_t *newvar, int64_t ref_len, int32_t *frag_state, int32_t *moved_owner,
                              uint32_t *n_moved, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_ASSEMBLE_SAMPLES_H */
