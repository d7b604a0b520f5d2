// var_check_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only.
// mixemt's variant check (assemble._check_contrib_phy_vars, assemble.py:157-208) for the samples of a cohort in one
// launch, over pileup tables that stay on the device (mxm_check_variants_samples, include/mixemt_hip_var_check.h).
//
// ONE workgroup per sample.  The sample's candidates are taken strictly one after another -- each depends on what the
// kept ones before it claimed -- and the workgroup's threads share the keys and the variant sites of the current one.
// Per sample, in LDS:
//     used      bitset over pos * 4 + code: the reference's used_vars (claimed (position, base) pairs); L / 2 bytes
//     touched   bitset over positions: those a kept candidate's own variants fall on (get_ancestral pops them); L / 8 bytes
// VCHK_MAX_L = 131 072 positions: 64 KiB of `used` + 16 KiB of `touched` + the two tally words, so at the cap ONE
// workgroup fits a CU's 160 KiB (two up to L = 131 059); at Build 17's L = 16 589 a workgroup takes 10.4 KB and LDS does
// not limit residency.  Everything is integer counts and bit-ORs (LDS integer atomics, a barrier between the phases): the same
// bits for any thread order and wherever the sample stands in the batch.  The decisions are fp64 in the reference's
// order of operations (no fast-math flag in the build).
#ifndef MIXEMT_VAR_CHECK_KERNELS_HPP
#define MIXEMT_VAR_CHECK_KERNELS_HPP

#define VCHK_THREADS 256
#define VCHK_MAX_L 131072
#define VCHK_MAX_LD 64

// words of the two bitsets, then the two counters
__host__ __device__ static inline int64_t vchk_used_words(int64_t L) { return (4 * L + 31) / 32; }
__host__ __device__ static inline int64_t vchk_touched_words(int64_t L) { return (L + 31) / 32; }
static inline size_t vchk_lds_bytes(int64_t L) { return (size_t)(vchk_used_words(L) + vchk_touched_words(L) + 2) * sizeof(uint32_t); }

__device__ __forceinline__ bool vchk_bit(const uint32_t *words, int32_t i) {
    // (other threads OR into the same words meanwhile, never into the bit asked for)
    return (__atomic_load_n(&words[i >> 5], __ATOMIC_RELAXED) >> (i & 31)) & 1u;
}

// assemble.py:178-184 for one (position, base): seen = obs_at(pos, base), total = total_obs(pos) (A + C + G + T of both
// strands), found when seen >= max(min_var_reads, total * frac_var_reads)
__device__ __forceinline__ bool vchk_found(const uint32_t *table, int32_t key, double min_var_reads, double frac_var_reads) {
    const uint32_t *row = table + (int64_t)(key >> 2) * 16;
    const int code = key & 3;
    const uint4 f = *reinterpret_cast<const uint4 *>(row);            // forward A C G T
    const uint32_t r0 = row[7], r1 = row[8], r2 = row[9], r3 = row[10];   // reverse a c g t
    const unsigned long long total = (unsigned long long)f.x + f.y + f.z + f.w + r0 + r1 + r2 + r3;
    const unsigned long long seen = (unsigned long long)row[code] + row[code + 7];
    const double scaled = (double)total * frac_var_reads;
    const double threshold = min_var_reads > scaled ? min_var_reads : scaled;   // max(a, b): a unless b is larger
    return (double)seen >= threshold;
}

// The check of ONE sample by its workgroup: table [L][16] its pileup, cand_row [n] its candidates in checking order (n > 0),
// keep_row / uniq_row / found_row (the last two nullable) its rows of the outputs.  Shared by check_variants_samples_kernel and
// check_variants_entries_kernel (detect_kernels.hpp): every thread of the workgroup calls it.
__device__ __forceinline__ void vchk_check_sample(
    uint32_t *vchk_lds, const uint32_t *__restrict__ table, int64_t L, const int32_t *__restrict__ key_ptr,
    const int32_t *__restrict__ key, const int32_t *__restrict__ site, const int32_t *__restrict__ site_key, int n_sites,
    const int32_t *__restrict__ cand_row, int n, double min_var_reads, double frac_var_reads, double var_fraction, int has_var_count,
    int var_count, uint8_t *__restrict__ keep_row, int32_t *__restrict__ uniq_row, int32_t *__restrict__ found_row) {
    const int tid = threadIdx.x;
    const int64_t uw = vchk_used_words(L), tw = vchk_touched_words(L);
    uint32_t *used = vchk_lds, *touched = used + uw, *tally = touched + tw;
    for (int64_t i = tid; i < uw + tw + 2; i += VCHK_THREADS) vchk_lds[i] = 0u;
    __syncthreads();
    const int32_t n_keys_max = (int32_t)(L < (1 << 29) ? 4 * L : 0x7fffffff);

    for (int c = 0; c < n; ++c) {
        const int h = cand_row[c];
        const int32_t k0 = key_ptr[h], k1 = key_ptr[h + 1];
        // ---- the candidate's keys that nobody has claimed, and those of them the sample shows ----
        int uniq = 0, found = 0;
        for (int32_t k = k0 + tid; k < k1; k += VCHK_THREADS) {
            const int32_t kk = key[k];
            const bool inside = kk >= 0 && kk < n_keys_max;
            if (inside && vchk_bit(used, kk)) continue;
            ++uniq;
            if (inside && vchk_found(table, kk, min_var_reads, frac_var_reads)) ++found;
        }
        if (uniq) atomicAdd(&tally[0], (uint32_t)uniq);
        if (found) atomicAdd(&tally[1], (uint32_t)found);
        __syncthreads();
        const int nu = (int)tally[0], nf = (int)tally[1];
        // assemble.py:185-187, the same operations in the same order
        const bool kept = nu == 0 || (has_var_count && nf >= var_count) || ((double)nf / (double)nu >= var_fraction);
        __syncthreads();                                              // (everyone has read the tally)
        if (tid == 0) {
            tally[0] = 0u;
            tally[1] = 0u;
            keep_row[c] = kept ? 1 : 0;
            if (uniq_row != nullptr) uniq_row[c] = nu;
            if (found_row != nullptr) found_row[c] = nf;
        }
        if (kept) {                                                   // (uniform: a dropped candidate claims nothing)
            // ---- its found keys are claimed; every position it has a variant on is touched ----
            for (int32_t k = k0 + tid; k < k1; k += VCHK_THREADS) {
                const int32_t kk = key[k];
                if (kk < 0 || kk >= n_keys_max) continue;
                const int32_t pos = kk >> 2;
                atomicOr(&touched[pos >> 5], 1u << (pos & 31));
                if (!vchk_bit(used, kk) && vchk_found(table, kk, min_var_reads, frac_var_reads))
                    atomicOr(&used[kk >> 5], 1u << (kk & 31));
            }
            __syncthreads();
            // ---- and the reference base of every other variant site (phylo.get_ancestral) ----
            for (int i = tid; i < n_sites; i += VCHK_THREADS) {
                const int32_t sk = site_key[i], pos = site[i];
                if (sk < 0 || sk >= n_keys_max || pos < 0 || pos >= L) continue;
                if (!vchk_bit(touched, pos)) atomicOr(&used[sk >> 5], 1u << (sk & 31));
            }
            __syncthreads();
            for (int32_t k = k0 + tid; k < k1; k += VCHK_THREADS) {
                const int32_t kk = key[k];
                if (kk >= 0 && kk < n_keys_max) touched[kk >> 7] = 0u;     // (word of position kk >> 2)
            }
        }
        __syncthreads();
    }
}

// counts [S][L][16]; key_ptr [H + 1] / key: every haplogroup's pos * 4 + code, distinct; site / site_key [n_sites]: the
// tree's variant sites and site * 4 + code of the reference base there (-1: not one of ACGT); cand [S][ld] / ncand [S]:
// the candidates in checking order.  A key outside [0, 4 L) (the entry's max_pos check rules it out) is counted as
// unseen and touches nothing.
__global__ __launch_bounds__(VCHK_THREADS) void check_variants_samples_kernel(
    const uint32_t *__restrict__ counts, int64_t L, const int32_t *__restrict__ key_ptr, const int32_t *__restrict__ key,
    const int32_t *__restrict__ site, const int32_t *__restrict__ site_key, int n_sites, const int32_t *__restrict__ cand,
    const int32_t *__restrict__ ncand, int ld, double min_var_reads, double frac_var_reads, double var_fraction,
    int has_var_count, int var_count, uint8_t *__restrict__ keep, int32_t *__restrict__ n_uniq, int32_t *__restrict__ n_found) {
    extern __shared__ uint32_t vchk_lds[];
    const int s = blockIdx.x;
    const int n = ncand[s];
    if (n <= 0) return;
    const int64_t at = (int64_t)s * ld;
    vchk_check_sample(vchk_lds, counts + (int64_t)s * L * 16, L, key_ptr, key, site, site_key, n_sites, cand + at, n, min_var_reads,
                      frac_var_reads, var_fraction, has_var_count, var_count, keep + at, n_uniq != nullptr ? n_uniq + at : nullptr,
                      n_found != nullptr ? n_found + at : nullptr);
}

#endif  // MIXEMT_VAR_CHECK_KERNELS_HPP
