// detect_kernels.hpp -- part of libmixemt_hip.so (gfx950, wave64); included by mixemt_hip.hip only, after var_check_kernels.hpp.
// What follows the vote when the DETECTION is bootstrapped (include/mixemt_hip_detect.h; assign.detect_many): entries are
// (sample, replicate) pairs, thousands of them, so the candidate rule and the variant check stay on the device.
//
//   detect_candidates_kernel       assemble.py:115-123 and the sort of :85-86: ONE workgroup per entry.  The H votes are
//       scanned 256 at a time; a wave compacts its candidates with a ballot and a popcount into an LDS list of at most 64
//       (one LDS integer add per wave and step reserves the wave's slots).  The list's order depends on the order the waves
//       arrive in, the OUTPUT does not: every candidate is then ranked by comparison counting under the total order
//       (proportion descending, first ascending, haplogroup ascending), and the rank is its slot.  Past `ld` candidates only the
//       count is kept.  No scratch, no float atomics.
//   check_variants_entries_kernel  vchk_check_sample (var_check_kernels.hpp) per entry, the candidates read from the device
//       and the pileup picked by table_of[e], so the replicates of a sample share its table.
#ifndef MIXEMT_DETECT_KERNELS_HPP
#define MIXEMT_DETECT_KERNELS_HPP

#define DETECT_THREADS 256
#define DETECT_MAX_LD 64

__global__ __launch_bounds__(DETECT_THREADS) void detect_candidates_kernel(
    const double *__restrict__ votes, const int64_t *__restrict__ first, const int64_t *__restrict__ rows,
    const double *__restrict__ props, const mxm_em_state *__restrict__ state, int H, double min_reads, int ld,
    int32_t *__restrict__ cand, int32_t *__restrict__ ncand, double *__restrict__ cprop) {
    __shared__ int32_t list_h[DETECT_MAX_LD];
    __shared__ double list_p[DETECT_MAX_LD];
    __shared__ int64_t list_f[DETECT_MAX_LD];
    __shared__ int32_t found, poisoned;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) {
        found = 0;
        poisoned = 0;
    }
    __syncthreads();
    const int64_t n_rows = rows[e];
    const double *v = votes + (int64_t)e * H, *p = props + (int64_t)e * H;
    const int64_t *f = first + (int64_t)e * H;
    bool bad = false;
    for (int h0 = 0; h0 < H; h0 += DETECT_THREADS) {                 // (uniform trip count: the ballot sees whole waves)
        const int h = h0 + tid;
        bool is_cand = false;
        double ph = 0.0;
        int64_t fh = 0;
        if (h < H) {
            const double vh = v[h];
            bad = bad || vh != vh;
            fh = f[h];
            is_cand = fh < n_rows && vh >= min_reads;                // (a NaN vote compares false)
            if (is_cand) {
                ph = p[h];
                bad = bad || ph != ph;
            }
        }
        const unsigned long long mask = __ballot(is_cand);
        if (mask != 0ull) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&found, __popcll(mask));
            base = __shfl(base, 0);
            const int slot = base + __popcll(mask & ((1ull << lane) - 1ull));
            if (is_cand && slot < DETECT_MAX_LD) {
                list_h[slot] = h;
                list_p[slot] = ph;
                list_f[slot] = fh;
            }
        }
    }
    if (bad) atomicOr(&poisoned, 1);
    __syncthreads();
    const int n = found;
    bool refused = poisoned != 0;
    if (state != nullptr) refused = refused || state[e].error != 0u || state[e].done == 0;
    if (refused || n > ld) {
        if (tid == 0) ncand[e] = refused ? -1 : n;
        return;
    }
    if (tid == 0) ncand[e] = n;
    if (tid < n) {
        const int32_t hi = list_h[tid];
        const double pi = list_p[tid];
        const int64_t fi = list_f[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const double pj = list_p[j];
            const int64_t fj = list_f[j];
            rank += (pj > pi || (pj == pi && (fj < fi || (fj == fi && list_h[j] < hi)))) ? 1 : 0;
        }
        cand[(int64_t)e * ld + rank] = hi;
        cprop[(int64_t)e * ld + rank] = pi;
    }
}

// counts [T][L][16]; table_of [E]: entry e's table (the entry has checked it against T); cand [E][ld] / ncand [E] on the
// device, as detect_candidates_kernel leaves them.  flag[e]: 0 checked, 1 ncand outside [0, ld], 2 a candidate outside [0, H);
// an entry flagged 1 or 2 is left alone.
__global__ __launch_bounds__(VCHK_THREADS) void check_variants_entries_kernel(
    const uint32_t *__restrict__ counts, int64_t L, const int32_t *__restrict__ key_ptr, const int32_t *__restrict__ key, int H,
    const int32_t *__restrict__ site, const int32_t *__restrict__ site_key, int n_sites, const int32_t *__restrict__ table_of,
    const int32_t *__restrict__ cand, const int32_t *__restrict__ ncand, int ld, double min_var_reads, double frac_var_reads,
    double var_fraction, int has_var_count, int var_count, uint8_t *__restrict__ keep, int32_t *__restrict__ n_uniq,
    int32_t *__restrict__ n_found, int32_t *__restrict__ flag) {
    extern __shared__ uint32_t vchk_lds[];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int n = ncand[e];
    const int64_t at = (int64_t)e * ld;
    if (n < 0 || n > ld) {
        if (tid == 0) flag[e] = 1;
        return;
    }
    int outside = 0;
    if (tid < n) {
        const int32_t h = cand[at + tid];
        outside = (h < 0 || h >= H) ? 1 : 0;
    }
    if (__syncthreads_or(outside)) {                                 // (uniform: nobody follows a key_ptr that is not there)
        if (tid == 0) flag[e] = 2;
        return;
    }
    if (tid == 0) flag[e] = 0;
    if (n == 0) return;
    vchk_check_sample(vchk_lds, counts + (int64_t)table_of[e] * L * 16, L, key_ptr, key, site, site_key, n_sites, cand + at, n,
                      min_var_reads, frac_var_reads, var_fraction, has_var_count, var_count, keep + at,
                      n_uniq != nullptr ? n_uniq + at : nullptr, n_found != nullptr ? n_found + at : nullptr);
}

#endif  // MIXEMT_DETECT_KERNELS_HPP
