// assemble_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only.
//
// mixemt's assembly stage over labelled pileups (assemble.py:431-585 of the reference): every kernel is integer work,
// and every result is the same bits for any alignment order and any launch shape.
//   consensus_kernel       call_consensus' consensus_base (assemble.py:444-459) for every position of every table
//   new_variants_kernel    find_new_variants (assemble.py:469-501): the bases one participating consensus has alone
//   first_observed_kernel  Counter.most_common(1)'s tie rule of the non-strict consensus: the base observed FIRST in
//   first_resolve_kernel   the contributor's alignment list (order key (joined, index)), only at tied positions
//   extend_walk_kernel     assign_reads_from_new_vars (assemble.py:504-546): the owners an unassigned fragment's bases
//   extend_move_kernel     show, folded into one state per fragment; then the move of the fragments with ONE owner
// The alignment walk (CIGAR, query offsets, quality rule), the wave-per-alignment loop and the error word are
// aln_walk.hpp's.
#ifndef MIXEMT_ASSEMBLE_KERNELS_HPP
#define MIXEMT_ASSEMBLE_KERNELS_HPP

#define ASM_THREADS 256
#define ASM_WALK_THREADS 512           // 8 waves; with newvar in LDS two workgroups share a CU up to 80 KiB each
#define ASM_MAX_USE 127                // participating contributors: an owner is an int8
#define ASM_LDS_MAX_BYTES 163840       // gfx950: 160 KiB of LDS per CU, all of it open to one workgroup
#define ASM_KEY_NONE 0xffffffffffffffffull
#define ASM_FRAG_EMPTY (-1)
#define ASM_FRAG_CONFLICT (-2)

// the character of a consensus by folded bin: A C G T, (N is never called from counts), other, gap
__device__ __forceinline__ uint8_t asm_bin_char(int bin) { return (uint8_t)"ACGTNX-"[bin]; }

// rows of the participating contributors: passed by value (<= 127 of them)
struct asm_rows {
    int32_t row[ASM_MAX_USE + 1];
};

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A thread per (table, position < ref_len).  Strands folded (bin i + bin i + 7); N observations ignored; gaps and `other`
// count towards the coverage and can be called.  tied[.]: 0, or (not strict, coverage met, several bins share the
// largest count) the mask of those bins -- cons[.] then holds the first of them in bin order until
// first_resolve_kernel puts the reference's choice there.
__global__ __launch_bounds__(ASM_THREADS) void consensus_kernel(const uint32_t *__restrict__ counts, int32_t n_labels,
                                                                int64_t L, int64_t ref_len, int64_t min_cov, int strict,
                                                                uint8_t *__restrict__ cons, uint8_t *__restrict__ tied,
                                                                uint32_t *n_tied) {
    const int64_t n = (int64_t)n_labels * ref_len;
    uint32_t mine = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lab = t / ref_len, pos = t - lab * ref_len;
        uint32_t c[7] = {0, 0, 0, 0, 0, 0, 0};
        if (pos < L) {
            const uint4 *row = reinterpret_cast<const uint4 *>(counts + (lab * L + pos) * 16);
            const uint4 a = row[0], b = row[1], d = row[2], e = row[3];          // bins 0-3, 4-7, 8-11, 12-15
            c[0] = a.x + b.w;
            c[1] = a.y + d.x;
            c[2] = a.z + d.y;
            c[3] = a.w + d.z;
            c[5] = b.y + e.x;
            c[6] = b.z + e.y;
        }
        const unsigned long long total = (unsigned long long)c[0] + c[1] + c[2] + c[3] + c[5] + c[6];
        uint8_t out = 'N', mask = 0;
        if (total > 0 && (long long)total >= min_cov) {
            uint32_t best = 0;
#pragma unroll
            for (int k = 0; k < 7; ++k) best = c[k] > best ? c[k] : best;
            int first = -1, n_best = 0;
#pragma unroll
            for (int k = 0; k < 7; ++k)
                if (k != 4 && c[k] == best) {
                    if (first < 0) first = k;
                    mask |= (uint8_t)(1u << k);
                    ++n_best;
                }
            if (strict) {
                out = best == total ? asm_bin_char(first) : (uint8_t)'N';
                mask = 0;
            } else {
                out = asm_bin_char(first);
                if (n_best < 2) mask = 0;
            }
        }
        cons[t] = out;
        if (tied != nullptr) tied[t] = mask;
        mine += mask != 0;
    }
    if (n_tied != nullptr) {
        mine = wave_sum_u32(mine);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_tied, mine);
    }
}

__device__ __forceinline__ int asm_acgt(uint8_t b) {
    const int bin = obs_base_bin(b);
    return bin < 4 ? bin : -1;
}

// A thread per position: newvar[pos] = four int8 owners (A, C, G, T; -1 none), owner k = the k-th participating row.
// Skipped (all -1) when any participating consensus is N, '-' or X there.
__global__ __launch_bounds__(ASM_THREADS) void new_variants_kernel(const uint8_t *__restrict__ cons, int64_t ld,
                                                                   asm_rows rows, int32_t n_use, int64_t ref_len,
                                                                   uint32_t *__restrict__ newvar, uint32_t *n_new) {
    uint32_t mine = 0;
    for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < ref_len;
         pos += (int64_t)gridDim.x * blockDim.x) {
        int cnt[4] = {0, 0, 0, 0}, own[4] = {-1, -1, -1, -1};
        bool skip = n_use <= 0;
        for (int k = 0; k < n_use; ++k) {
            const int b = asm_acgt(cons[(int64_t)rows.row[k] * ld + pos]);
            if (b < 0) {
                skip = true;
                break;
            }
#pragma unroll
            for (int x = 0; x < 4; ++x)                      // (constant indexes: the arrays stay in registers)
                if (x == b) {
                    ++cnt[x];
                    own[x] = k;
                }
        }
        uint32_t word = 0xffffffffu;
        if (!skip) {
            word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int o = cnt[b] == 1 ? own[b] : -1;
                word |= (uint32_t)(uint8_t)(int8_t)o << (8 * b);
                mine += o >= 0;
            }
        }
        newvar[pos] = word;
    }
    mine = wave_sum_u32(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_new, mine);
}

// A wave per alignment of a labelled list (label in [0, n_labels), mapq >= min_mq, placed): every observation the
// pileup counts at a position whose `tied` byte is set offers its order key -- (joined << 32) | index, the place of the
// alignment in its contributor's list -- to first[(label * ref_len + pos) * 8 + folded bin] by atomicMin.  Positions
// that are not tied cost one byte read and no atomic.  Error kind 3: a label >= n_labels.
__global__ __launch_bounds__(ASM_WALK_THREADS) void first_observed_kernel(
    aln_view aln, const int32_t *__restrict__ label, const int32_t *__restrict__ joined, int32_t n_labels,
    int64_t ref_len, const uint8_t *__restrict__ tied, unsigned long long *__restrict__ first, unsigned long long *err) {
    aln_for_each(
        aln.n_aln,
        [&](int64_t i) {
            const int32_t lab = label[i];
            if (lab >= n_labels) aln_error(err, i, 3);
            return lab >= 0 && lab < n_labels && obs_counts(aln.ref_start, aln.mapq, aln.min_mq, i);
        },
        [&](int64_t i, int lane) {
            const int64_t lab = label[i];
            const unsigned long long key = ((unsigned long long)(uint32_t)(joined != nullptr ? joined[i] : 0) << 32) |
                                           (unsigned long long)i;
            aln_walk(aln, i, lane, err, [&](bool match, int64_t r, int64_t qp, int64_t len, bool has_q) -> unsigned {
                const int64_t stop = min(len, ref_len - r);              // positions past ref_len have no consensus
                for (int64_t j = lane; j < stop; j += 64) {
                    const int64_t cell = lab * ref_len + r + j;
                    const uint8_t m = tied[cell];
                    if (!m) continue;
                    const int bin = match ? aln_base_bin(aln, has_q, qp + j) : 6;
                    if ((m >> bin) & 1) atomicMin(&first[cell * 8 + bin], key);
                }
                return 0;
            });
        });
}

// A thread per (table, position): at a tied position the bin of the mask with the smallest key is the consensus.
__global__ __launch_bounds__(ASM_THREADS) void first_resolve_kernel(const uint8_t *__restrict__ tied,
                                                                    const unsigned long long *__restrict__ first,
                                                                    int64_t n, uint8_t *__restrict__ cons) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t m = tied[t];
        if (!m) continue;
        unsigned long long best = ASM_KEY_NONE;
        int pick = -1;
        for (int k = 0; k < 7; ++k)
            if (((m >> k) & 1) && first[t * 8 + k] < best) {
                best = first[t * 8 + k];
                pick = k;
            }
        if (pick >= 0) cons[t] = asm_bin_char(pick);
    }
}

// the state of a fragment as a function of the SET of owners seen: empty, one owner, or conflict
__device__ __forceinline__ int asm_merge(int a, int b) {
    if (a == ASM_FRAG_EMPTY) return b;
    if (b == ASM_FRAG_EMPTY || a == b) return a;
    return ASM_FRAG_CONFLICT;
}

// A wave per unassigned alignment with mapq >= min_mq: lanes on the bases of an M / = / X operation (I / S advance the
// query, D / N the reference: get_aligned_pairs(matches_only=True)); a base counts when the alignment has no qualities
// or its quality is >= min_bq; its upper-cased character is looked up in newvar (staged in LDS when IN_LDS).  The wave
// merges its lanes' owners and folds ONE state into frag_state[fragment]: the final state does not depend on the order.
// Error kind 3: a fragment index outside [0, n_frag) (the alignment is skipped).
template <bool IN_LDS>
__global__ __launch_bounds__(ASM_WALK_THREADS) void extend_walk_kernel(
    aln_view aln, const int64_t *__restrict__ frag, const int32_t *__restrict__ label, int32_t unassigned, int64_t n_frag,
    const uint32_t *__restrict__ newvar, int64_t ref_len, int32_t *__restrict__ frag_state, unsigned long long *err) {
    extern __shared__ uint32_t nv_lds[];
    if (IN_LDS) {
        for (int64_t k = threadIdx.x; k < ref_len; k += blockDim.x) nv_lds[k] = newvar[k];
        __syncthreads();
    }
    aln_for_each(
        aln.n_aln,
        [&](int64_t i) { return label[i] == unassigned && obs_counts(aln.ref_start, aln.mapq, aln.min_mq, i); },
        [&](int64_t i, int lane) {
            const int64_t f = frag[i];
            if (f < 0 || f >= n_frag) {
                if (lane == 0) aln_error(err, i, 3);
                return;
            }
            int state = ASM_FRAG_EMPTY;
            aln_walk(aln, i, lane, err, [&](bool match, int64_t r, int64_t qp, int64_t len, bool has_q) -> unsigned {
                if (!match) return 0;
                const int64_t stop = min(len, ref_len - r);              // newvar ends at ref_len
                for (int64_t j = lane; j < stop; j += 64) {
                    const int b = aln_base_bin(aln, has_q, qp + j);
                    if (b > 3) continue;                                 // a low quality, N or no base at all
                    const uint32_t word = IN_LDS ? nv_lds[r + j] : newvar[r + j];
                    const int owner = (int)(int8_t)(uint8_t)(word >> (8 * b));
                    if (owner >= 0) state = asm_merge(state, owner);
                }
                return 0;
            });
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) state = asm_merge(state, __shfl_xor(state, off, 64));
            if (lane == 0 && state != ASM_FRAG_EMPTY) {
                int32_t *cell = &frag_state[f];
                if (state == ASM_FRAG_CONFLICT) {
                    atomicExch(cell, ASM_FRAG_CONFLICT);
                } else {
                    const int32_t old = atomicCAS(cell, ASM_FRAG_EMPTY, state);
                    if (old != ASM_FRAG_EMPTY && old != state) atomicExch(cell, ASM_FRAG_CONFLICT);
                }
            }
        });
}

// A thread per alignment: an unassigned alignment (whatever its mapq) whose fragment has ONE owner takes the owner's
// label and joined = round; moved_owner[i] = the owner (the index of its table) or -1, the labels of the next round's
// additive pileup.
__global__ __launch_bounds__(ASM_THREADS) void extend_move_kernel(const int64_t *__restrict__ frag, int64_t n_aln,
                                                                  int64_t n_frag, int32_t unassigned, asm_rows rows,
                                                                  int32_t n_use, int32_t round,
                                                                  const int32_t *__restrict__ frag_state,
                                                                  int32_t *__restrict__ label, int32_t *__restrict__ joined,
                                                                  int32_t *__restrict__ moved_owner, uint32_t *n_moved) {
    uint32_t mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_aln; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t owner = -1;
        if (label[i] == unassigned) {
            const int64_t f = frag[i];
            if (f >= 0 && f < n_frag) owner = frag_state[f];
            if (owner >= 0 && owner < n_use) {
                label[i] = rows.row[owner];
                joined[i] = round;
                ++mine;
            } else {
                owner = -1;
            }
        }
        if (moved_owner != nullptr) moved_owner[i] = owner;
    }
    mine = wave_sum_u32(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(n_moved, mine);
}

#endif  // MIXEMT_ASSEMBLE_KERNELS_HPP
