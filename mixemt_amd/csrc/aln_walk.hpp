// aln_walk.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only.
//
// The ONE walk of an alignment on the device: a wave per alignment, its lanes on the bases of a CIGAR operation.  The
// pileup (observe_count_kernel), the tie rule of the majority consensus (first_observed_kernel) and the assembly
// extension (extend_walk_kernel) all see an alignment through aln_walk, which is what makes the tables, the consensus
// and the extension agree with each other:
//   M / = / X   consume query and reference: one observation per base (pysam's aligned pairs)
//   D / N       consume the reference only: one gap per position (get_aligned_pairs(matches_only=False) emits
//               (None, rpos) for N as well; with matches_only=True they only advance)
//   I / S       consume the query only;  H / P  neither
// The CIGAR is walked exactly as the host encoder's aln_detail::walker (aln_encode.hpp) walks it -- same operations,
// same two errors, same quality rule -- so the device stages and the EM input agree on query offsets.  (The walker
// is a different job and stays apart: host threads over variant sites, not lanes over bases.)
// A base is its upper-cased character in the bins A C G T N other = 0..5; when the alignment has qualities and the
// base's is below min_bq it is an 'N' (bin 4).
//
// Errors are one packed word per call, (alignment index << 2) | kind, lowered by atomicMin: the first alignment in
// index order wins.  Kind 1 = the CIGAR runs past its sequence, 2 = it holds an unknown operation (both raised here,
// -4 as mxm_aln_encode), 3 and 0 = the caller's own (a position past the table, a fragment that is none, a label
// >= n_labels).
#ifndef MIXEMT_ALN_WALK_HPP
#define MIXEMT_ALN_WALK_HPP

#define ALN_ERR_NONE 0xffffffffffffffffull

// The device columns a walk reads and the two quality floors, by value (a kernel argument).
struct aln_view {
    const int64_t *ref_start;
    const int32_t *mapq;
    const int64_t *cig_ptr;
    const uint32_t *cigar;
    const int64_t *seq_ptr;
    const uint8_t *seq, *qual, *has_qual;
    int64_t n_aln;
    int32_t min_mq, min_bq;
};

static aln_view aln_view_of(const mxm_aln_columns *cols, int32_t min_mq, int32_t min_bq) {
    return aln_view{cols->ref_start, cols->mapq, cols->cig_ptr, cols->cigar, cols->seq_ptr, cols->seq,
                    cols->qual,      cols->has_qual, cols->n_aln, min_mq, min_bq};
}

__device__ __forceinline__ void aln_error(unsigned long long *err, int64_t i, unsigned kind) {
    atomicMin(err, ((unsigned long long)i << 2) | kind);
}

__device__ __forceinline__ int obs_base_bin(uint8_t b) {
    if (b >= 'a' && b <= 'z') b = (uint8_t)(b - 32);       // str.upper() on an ASCII character
    switch (b) {
        case 'A': return 0;
        case 'C': return 1;
        case 'G': return 2;
        case 'T': return 3;
        case 'N': return 4;
        default: return 5;
    }
}

// the bin of the query base at qp (an index into seq / qual) of an alignment with (has_q) or without qualities
__device__ __forceinline__ int aln_base_bin(const aln_view &v, bool has_q, int64_t qp) {
    return (has_q && (int32_t)v.qual[qp] < v.min_bq) ? 4 : obs_base_bin(v.seq[qp]);
}

// Walks alignment i with the calling wave.  For every operation that consumes the reference,
//   visit(match, r, qp, len, has_q)   match: M / = / X (else D / N); r: the reference position of its first base; qp:
//                                     the index of its first query base in seq / qual (match only); len: its length
// is called by all lanes, which share the op's bases as `for (j = lane; j < len; j += 64)`.  visit returns 0, or an
// error kind of its own that ends the walk.  An error is reported by lane 0, once.
template <typename Visit>
__device__ __forceinline__ void aln_walk(const aln_view &v, int64_t i, int lane, unsigned long long *err, Visit visit) {
    const int64_t s0 = v.seq_ptr[i], slen = v.seq_ptr[i + 1] - s0;
    const bool has_q = v.qual != nullptr && (v.has_qual == nullptr || v.has_qual[i] != 0);
    int64_t r = v.ref_start[i], q = 0;
    for (int64_t k = v.cig_ptr[i]; k < v.cig_ptr[i + 1]; ++k) {
        const uint32_t op = v.cigar[k] & 15u;
        const int64_t len = (int64_t)(v.cigar[k] >> 4);
        const bool match = op == 0 || op == 7 || op == 8, gap = op == 2 || op == 3;
        unsigned kind = 0;
        if (op > 8) kind = 2;
        else if (match && q + len > slen) kind = 1;
        else if (match || gap) kind = visit(match, r, s0 + q, len, has_q);
        if (kind) {
            if (lane == 0) aln_error(err, i, kind);
            break;
        }
        if (match || op == 1 || op == 4) q += len;
        if (match || gap) r += len;
    }
}

// A wave per 64 alignments of [0, n_aln): each lane tests one (`use(i)`), then the wave takes those that qualify one
// by one, `body(i, lane)` with all its lanes.
template <typename Use, typename Body>
__device__ __forceinline__ void aln_for_each(int64_t n_aln, Use use, Body body) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t n_wave = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i0 = wave * 64; i0 < n_aln; i0 += n_wave * 64) {
        const int64_t mine = i0 + lane;
        unsigned long long todo = __ballot(mine < n_aln && use(mine));
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            body(i0 + src, lane);
        }
    }
}

#endif  // MIXEMT_ALN_WALK_HPP
