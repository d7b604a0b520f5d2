// observe_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only.
//
// The pileup of the variant check: observe.ObservedBases._observe_aln (mixemt/observe.py:56-86) over
// every alignment, i.e. one count per (reference position, observed character) of pysam's
// get_aligned_pairs(matches_only=False):
//   M / = / X   one observation per base: the upper-cased query base, or 'N' when the alignment has qualities and this
//               base's is below min_bq; a reverse alignment counts it in the lower-case bin
//   D / N       one gap per reference position: '-' forward, '+' reverse (pysam emits (None, rpos) for N as well)
//   I / S       the query only;  H / P  neither
// Bins of counts[L][16]: 0-6 forward A C G T N other '-', 7-13 reverse a c g t n other '+', 14-15 pad (never written).
// The walk itself, the base rule and the error word are aln_walk.hpp's.
//
// Shape (everything is an integer count: the table is the same bits for any input order and any launch shape):
//   1. bucket   alignments that count (mapq >= min_mq, ref_start >= 0) by ref_start / OBS_BUCKET; per workgroup an LDS
//               histogram, one global atomic per (workgroup, bucket) to reserve slots, the alignment indices scattered
//               into their bucket's range of `perm` (order inside a bucket is arbitrary and does not matter)
//   2. count    a workgroup per OBS_CHUNK alignments of ONE bucket: an LDS histogram of the window
//               [bucket start, + OBS_WIN) (bin-major: lanes on consecutive positions hit consecutive banks), a wave per
//               alignment with its lanes on the bases of an op; a position past the window (a long D / N, a long
//               read) goes to a global atomic; the window is flushed with one atomic per non-zero bin, a wave's
//               atomics covering 4 positions x 16 bins = 256 contiguous bytes
// Errors (aln_walk.hpp's word): the walk's two (-4), a reference position >= L (kind 3, -1: the table is too short), and
// in the labelled form a label >= n_labels (kind 0, -1).
//
// Labelled form (LABELLED = true, mxm_observe_bases_labelled): alignment i with label[i] in [0, n_labels) is counted into
// table counts[label[i]][L][16]; label[i] < 0 is not counted, label[i] >= n_labels is an error (-1).  The bucket key
// widens to label * nb + ref_start / OBS_BUCKET over n_labels * nb buckets (nb = windows of one table), so a count
// workgroup still holds ONE window of ONE table: the key gives the label (the table's base) and the window.  With
// LABELLED = false the key is the window and the kernels are the unlabelled pileup's.
#ifndef MIXEMT_OBSERVE_KERNELS_HPP
#define MIXEMT_OBSERVE_KERNELS_HPP

#define OBS_BUCKET 512             // reference positions per bucket (= window start step)
#define OBS_WIN 768                // window of a count workgroup: its bucket plus 256 positions of overhang
#define OBS_NBIN 14                // bins written (the 2 pad bins of a row are not)
#define OBS_THREADS 512            // count workgroup: 8 waves
#define OBS_CHUNK 1024             // alignments per count workgroup
#define OBS_BKT_THREADS 256        // bucket workgroups
#define OBS_BKT_PER_WG 4096        // alignments per bucket workgroup
#define OBS_LDS_BUCKETS 2048       // buckets an LDS histogram of step 1 holds (L up to 1 M); more: global atomics

__device__ __forceinline__ bool obs_counts(const int64_t *ref_start, const int32_t *mapq, int32_t min_mq, int64_t i) {
    return mapq[i] >= min_mq && ref_start[i] >= 0;
}

// The bucket of alignment i, or -1 when it is not counted (LABELLED: a negative label, or an error of kind 0, which
// mode 0 records).  nb: windows of one table.
template <bool LABELLED, int MODE>
__device__ __forceinline__ int64_t obs_bucket_of(const int64_t *ref_start, const int32_t *mapq, const int32_t *label,
                                                 int32_t n_labels, int32_t min_mq, int64_t L, int64_t nb, int64_t i,
                                                 unsigned long long *err) {
    int64_t lab = 0;
    if (LABELLED) {
        lab = label[i];
        if (lab >= n_labels) {
            if (MODE == 0) aln_error(err, i, 0);
            return -1;
        }
        if (lab < 0) return -1;
    }
    if (!obs_counts(ref_start, mapq, min_mq, i)) return -1;
    const int64_t r = ref_start[i];
    if (r >= L) {
        if (MODE == 0) aln_error(err, i, 3);
        return -1;
    }
    return (LABELLED ? lab * nb : 0) + r / OBS_BUCKET;
}

// step 1a / 1b: mode 0 counts the alignments of each bucket into cnt[b]; mode 1 scatters their indices into perm at
// cursor[b] (cursor = the buckets' exclusive offsets, advanced by the reservations).  nbk: buckets in all
// (n_labels * nb labelled, nb otherwise).
template <bool LABELLED, int MODE>
__global__ __launch_bounds__(OBS_BKT_THREADS) void observe_bucket_kernel(const int64_t *__restrict__ ref_start,
                                                                         const int32_t *__restrict__ mapq,
                                                                         const int32_t *__restrict__ label,
                                                                         int32_t n_labels, int64_t n_aln,
                                                                         int32_t min_mq, int64_t L, int64_t nb,
                                                                         int64_t nbk,
                                                                         unsigned long long *cnt_or_cursor,
                                                                         int32_t *__restrict__ perm,
                                                                         unsigned long long *err) {
    __shared__ unsigned int h[OBS_LDS_BUCKETS];
    __shared__ unsigned long long base[OBS_LDS_BUCKETS];
    const int64_t lo = (int64_t)blockIdx.x * OBS_BKT_PER_WG;
    const int64_t hi = min(n_aln, lo + (int64_t)OBS_BKT_PER_WG);
    const bool in_lds = nbk <= OBS_LDS_BUCKETS;
    if (in_lds) {
        for (int64_t b = threadIdx.x; b < nbk; b += blockDim.x) h[b] = 0;
        __syncthreads();
    }
    // pass over this workgroup's alignments: per-workgroup counts
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const int64_t b = obs_bucket_of<LABELLED, MODE>(ref_start, mapq, label, n_labels, min_mq, L, nb, i, err);
        if (b < 0) continue;
        if (in_lds) {
            atomicAdd(&h[b], 1u);
        } else if (MODE == 0) {
            atomicAdd(&cnt_or_cursor[b], 1ull);
        } else {
            perm[atomicAdd(&cnt_or_cursor[b], 1ull)] = (int32_t)i;
        }
    }
    if (!in_lds) return;
    __syncthreads();
    if (MODE == 0) {
        for (int64_t b = threadIdx.x; b < nbk; b += blockDim.x)
            if (h[b]) atomicAdd(&cnt_or_cursor[b], (unsigned long long)h[b]);
        return;
    }
    // reserve this workgroup's slots in every bucket it has alignments in, then hand them out
    for (int64_t b = threadIdx.x; b < nbk; b += blockDim.x) {
        if (h[b]) base[b] = atomicAdd(&cnt_or_cursor[b], (unsigned long long)h[b]);
        h[b] = 0;
    }
    __syncthreads();
    for (int64_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const int64_t b = obs_bucket_of<LABELLED, 1>(ref_start, mapq, label, n_labels, min_mq, L, nb, i, err);
        if (b < 0) continue;
        perm[base[b] + atomicAdd(&h[b], 1u)] = (int32_t)i;
    }
}

// step 1c, one workgroup: off[b] = exclusive prefix of cnt (also copied to cursor), chunk_off[b] = exclusive prefix of
// ceil(cnt[b] / OBS_CHUNK); off[nb] / chunk_off[nb] the totals.  Each thread scans a contiguous run of buckets.
__global__ __launch_bounds__(1024) void observe_scan_kernel(const unsigned long long *__restrict__ cnt, int64_t nb,
                                                            unsigned long long *__restrict__ off,
                                                            unsigned long long *__restrict__ chunk_off,
                                                            unsigned long long *__restrict__ cursor) {
    __shared__ unsigned long long s_a[1024], s_c[1024];
    const int t = threadIdx.x, nt = blockDim.x;
    const int64_t per = (nb + nt - 1) / nt;
    const int64_t lo = min(nb, (int64_t)t * per), hi = min(nb, lo + per);
    unsigned long long a = 0, c = 0;
    for (int64_t b = lo; b < hi; ++b) {
        a += cnt[b];
        c += (cnt[b] + OBS_CHUNK - 1) / OBS_CHUNK;
    }
    s_a[t] = a;
    s_c[t] = c;
    __syncthreads();
    if (t == 0) {
        unsigned long long ra = 0, rc = 0;
        for (int k = 0; k < nt; ++k) {
            const unsigned long long xa = s_a[k], xc = s_c[k];
            s_a[k] = ra;
            s_c[k] = rc;
            ra += xa;
            rc += xc;
        }
        off[nb] = ra;
        chunk_off[nb] = rc;
    }
    __syncthreads();
    a = s_a[t];
    c = s_c[t];
    for (int64_t b = lo; b < hi; ++b) {
        off[b] = a;
        cursor[b] = a;
        chunk_off[b] = c;
        a += cnt[b];
        c += (cnt[b] + OBS_CHUNK - 1) / OBS_CHUNK;
    }
}

// step 2: grid = an upper bound of the chunk count (workgroups past chunk_off[nbk] leave at once).  nb: windows of one
// table, nbk: buckets in all (see observe_bucket_kernel).
template <bool LABELLED>
__global__ __launch_bounds__(OBS_THREADS) void observe_count_kernel(
    aln_view aln, const uint8_t *__restrict__ is_reverse, int64_t L, int64_t nb, int64_t nbk,
    const unsigned long long *__restrict__ off, const unsigned long long *__restrict__ chunk_off,
    const int32_t *__restrict__ perm, uint32_t *__restrict__ counts_all, unsigned long long *err) {
    __shared__ uint32_t hist[OBS_NBIN * OBS_WIN];
    const unsigned long long g = blockIdx.x;
    if (g >= chunk_off[nbk]) return;
    // the bucket holding chunk g: the last key with chunk_off[key] <= g (buckets without alignments have no chunk)
    int64_t lo_b = 0, hi_b = nbk;                            // chunk_off[lo_b] <= g < chunk_off[hi_b]
    while (hi_b - lo_b > 1) {
        const int64_t mid = (lo_b + hi_b) >> 1;
        if (chunk_off[mid] <= g) lo_b = mid;
        else hi_b = mid;
    }
    const int64_t key = lo_b;
    const unsigned long long a0 = off[key] + (g - chunk_off[key]) * OBS_CHUNK;
    const unsigned long long a1 = min(off[key + 1], a0 + (unsigned long long)OBS_CHUNK);
    const int64_t b = LABELLED ? key % nb : key;             // the window within its table
    uint32_t *__restrict__ counts = LABELLED ? counts_all + (key / nb) * L * 16 : counts_all;
    const int64_t w0 = b * OBS_BUCKET;                       // window [w0, w0 + OBS_WIN)
    for (int k = threadIdx.x; k < OBS_NBIN * OBS_WIN; k += blockDim.x) hist[k] = 0;
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_wave = blockDim.x >> 6;
    for (unsigned long long a = a0 + wave; a < a1; a += n_wave) {
        const int64_t i = perm[a];
        const int rev = (is_reverse != nullptr && is_reverse[i] != 0) ? 7 : 0;
        aln_walk(aln, i, lane, err, [&](bool match, int64_t r, int64_t qp, int64_t len, bool has_q) -> unsigned {
            if (r + len > L) return 3;                       // (positions only grow: the op's last one decides)
            for (int64_t j = lane; j < len; j += 64) {
                const int bin = (match ? aln_base_bin(aln, has_q, qp + j) : 6) + rev;
                const int64_t rp = r + j, w = rp - w0;
                if (w < OBS_WIN) atomicAdd(&hist[bin * OBS_WIN + (int)w], 1u);
                else atomicAdd(&counts[rp * 16 + bin], 1u);
            }
            return 0;
        });
    }
    __syncthreads();
    // flush: thread k takes (position k / 16, bin k % 16) so that a wave's atomics cover 256 contiguous bytes
    const int64_t w_end = min((int64_t)OBS_WIN, L - w0);
    for (int64_t k = threadIdx.x; k < w_end * 16; k += blockDim.x) {
        const int p = (int)(k >> 4), bin = (int)(k & 15);
        if (bin >= OBS_NBIN) continue;
        const uint32_t v = hist[bin * OBS_WIN + p];
        if (v) atomicAdd(&counts[(w0 + p) * 16 + bin], v);
    }
}

#endif  // MIXEMT_OBSERVE_KERNELS_HPP
