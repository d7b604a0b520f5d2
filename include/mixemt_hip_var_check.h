/*
 * mixemt_hip_var_check.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h, not meant to be included on
 * its own.
 * An addition behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entry has a header and a binding table (_lib.VARCHECK_SIGNATURES) of its own because the refusals of everything
 * mixemt_hip.h declares are pinned, entry by entry, in one table of the test suite; its own are pinned beside its tests
 * (tests/test_var_check_host.py).
 */
#ifndef MIXEMT_HIP_VAR_CHECK_H
#define MIXEMT_HIP_VAR_CHECK_H

#ifdef __cplusplus
extern "C" {
#endif

/* positions a pileup table may have for the check kernel: its two bitsets (L / 2 + L / 8 bytes) live in LDS */
#define MXM_VAR_CHECK_MAX_L 131072

/*
 * mixemt's variant check -- assemble._check_contrib_phy_vars, assemble.py:157-208 -- for S samples in ONE launch over
 * pileup tables that stay on the device (one workgroup per sample; a sample's candidates strictly one after another).
 *   counts [S][L][16]   the samples' pileups in the bins of the pileup entries (device, 16-byte aligned)
 *   key_ptr [H + 1], key   per haplogroup the distinct pos * 4 + code of (pos_from_var(v), der_allele(v)) over its
 *                       variants, code = index in "ACGT" (device int32)
 *   site [n_sites], site_key [n_sites]   phylo.get_variant_pos() and site * 4 + code of the reference base there, -1
 *                       where that base is not one of ACGT (device int32); max_pos: the largest position of key / site
 *   cand_host [S][ld], ncand_host [S]   HOST int32: the candidates' haplogroup indexes in checking order (descending
 *                       proportion, ties as Python's stable sort(reverse=True) leaves them); ld one of 4, 8, 16, 32, 64
 *   min_var_reads, frac_var_reads, var_fraction; has_var_count (0: args.var_count is None), var_count
 *   keep [S][ld] uint8, n_uniq / n_found [S][ld] int32 (both nullable): device; entries c >= ncand_host[s] are not written
 * Candidate c of a sample: n_uniq = its keys no kept candidate before it has claimed; such a key is found when
 * (double)seen >= max(min_var_reads, (double)total * frac_var_reads) with seen = counts[pos][code] + counts[pos][code + 7]
 * and total = bins 0-3 + bins 7-10 (assemble.py:178-184); kept when n_uniq == 0, or has_var_count and n_found >=
 * var_count, or (double)n_found / (double)n_uniq >= var_fraction (:185-187).  A kept candidate claims its found keys and
 * site_key of every site none of its keys -- found or not, claimed before or not -- falls on (phylo.get_ancestral,
 * phylotree.py:317-336); a dropped one claims nothing.  Integer counts and bit-ORs only: the same bits for any thread
 * order and wherever the sample stands in the batch; no float atomics.
 * The host tables are uploaded by the call into stream-ordered memory of its own (hipMallocAsync / hipFreeAsync on `stream`:
 * not meant to be captured), through a pageable copy of the call's own: cand_host / ncand_host are read before the call
 * returns, from pageable or pinned memory alike.  The kernel is ordered on `stream` and nothing is waited for at the table
 * sizes measured (S = 3, ld = 8: 108 bytes, on a stream with work pending; profiles/streams/README.md); HIP lets a runtime
 * hold a larger pageable upload until the stream has got there, which changes the call's host time, never its results.
 * Refused with -1 WITHOUT touching the device: S < 0; ld not one of 4, 8, 16, 32, 64; cand_host / ncand_host NULL; an
 * ncand_host[s] outside [0, ld]; a candidate index outside [0, H); counts, key_ptr, key or keep NULL (site / site_key
 * with n_sites > 0); counts not 16-byte aligned; L <= 0 or n_sites < 0; max_pos >= L; L > MXM_VAR_CHECK_MAX_L.
 * S == 0, or every ncand_host[s] == 0: 0, nothing launched.
 */
int mxm_check_variants_samples(const uint32_t *counts, int32_t S, int64_t L, const int32_t *key_ptr, const int32_t *key,
                               int32_t H, const int32_t *site, const int32_t *site_key, int32_t n_sites, int64_t max_pos,
                               const int32_t *cand_host, const int32_t *ncand_host, int32_t ld, double min_var_reads,
                               double frac_var_reads, double var_fraction, int32_t has_var_count, int32_t var_count,
                               uint8_t *keep, int32_t *n_uniq, int32_t *n_found, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_VAR_CHECK_H */
