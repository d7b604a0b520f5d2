// assemble_samples_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only, after
// assemble_kernels.hpp (the owner word, asm_merge, the fragment states and wave_sum_u32 are that file's).
//
// The assembly extension for the S samples of a cohort whose alignments lie in ONE set of columns and whose labels are
// GLOBAL (one per (sample, contributor)): integer work only, the same bits for any alignment order and launch shape.
//   new_variants_samples_kernel   new_variants_kernel per sample: a thread per (sample, position), the sample in blockIdx.y
//   extend_walk_samples_kernel    extend_walk_kernel with the sample's own newvar row (read from global memory; S rows of
//                                 ref_len words stay in L2) and the GLOBAL label of the owner folded into the fragment's state
//   extend_move_samples_kernel    extend_move_kernel: a thread per alignment, one counter per sample
// The per-sample tables (participants, their offsets, the 'unassigned' labels) are device arrays the host side uploads.
#ifndef MIXEMT_ASSEMBLE_SAMPLES_KERNELS_HPP
#define MIXEMT_ASSEMBLE_SAMPLES_KERNELS_HPP

// use[use_ptr[s] .. use_ptr[s + 1]): the consensus rows (= global labels) of sample s's participants.  Every wave of a block
// works for ONE sample, so its partial count is that sample's.  A sample without participants: its row becomes all -1 and
// its counter is left alone.
__global__ __launch_bounds__(ASM_THREADS) void new_variants_samples_kernel(const uint8_t *__restrict__ cons, int64_t ld,
                                                                           const int32_t *__restrict__ use,
                                                                           const int32_t *__restrict__ use_ptr, int32_t S,
                                                                           int64_t ref_len, uint32_t *__restrict__ newvar,
                                                                           uint32_t *n_new) {
    for (int32_t s = blockIdx.y; s < S; s += gridDim.y) {
        const int32_t lo = use_ptr[s], n_use = use_ptr[s + 1] - lo;
        uint32_t mine = 0;
        for (int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pos < ref_len;
             pos += (int64_t)gridDim.x * blockDim.x) {
            int cnt[4] = {0, 0, 0, 0}, own[4] = {-1, -1, -1, -1};
            bool skip = n_use <= 0;
            for (int k = 0; k < n_use; ++k) {
                const int b = asm_acgt(cons[(int64_t)use[lo + k] * ld + pos]);
                if (b < 0) {
                    skip = true;
                    break;
                }
#pragma unroll
                for (int x = 0; x < 4; ++x)                  // (constant indexes: the arrays stay in registers)
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
            newvar[(int64_t)s * ref_len + pos] = word;
        }
        mine = wave_sum_u32(mine);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&n_new[s], mine);
    }
}

// A wave per alignment of a sample that is not frozen (unassigned[s] >= 0) with label == unassigned[s] and mapq >= min_mq.
// s and unassigned[s] are per alignment, hence the same in every lane of the walk.  A hit's owner k becomes the global
// label use[use_ptr[s] + k] BEFORE it is merged: the state is a function of the set of global owners.
// Error kind 0: an aln_sample outside [0, S); kind 3: a fragment index outside [0, n_frag) (both: the alignment is skipped).
__global__ __launch_bounds__(ASM_WALK_THREADS) void extend_walk_samples_kernel(
    aln_view aln, const int64_t *__restrict__ frag, const int32_t *__restrict__ label,
    const int32_t *__restrict__ aln_sample, int32_t S, const int32_t *__restrict__ unassigned,
    const int32_t *__restrict__ use, const int32_t *__restrict__ use_ptr, int64_t n_frag,
    const uint32_t *__restrict__ newvar, int64_t ref_len, int32_t *__restrict__ frag_state, unsigned long long *err) {
    aln_for_each(
        aln.n_aln,
        [&](int64_t i) {
            const int32_t s = aln_sample[i];
            if (s < 0 || s >= S) {
                aln_error(err, i, 0);
                return false;
            }
            const int32_t un = unassigned[s];
            return un >= 0 && label[i] == un && obs_counts(aln.ref_start, aln.mapq, aln.min_mq, i);
        },
        [&](int64_t i, int lane) {
            const int64_t f = frag[i];
            if (f < 0 || f >= n_frag) {
                if (lane == 0) aln_error(err, i, 3);
                return;
            }
            const int32_t s = aln_sample[i];
            const int32_t lo = use_ptr[s], n_use = use_ptr[s + 1] - lo;
            const uint32_t *__restrict__ row = newvar + (int64_t)s * ref_len;
            int state = ASM_FRAG_EMPTY;
            aln_walk(aln, i, lane, err, [&](bool match, int64_t r, int64_t qp, int64_t len, bool has_q) -> unsigned {
                if (!match) return 0;
                const int64_t stop = min(len, ref_len - r);              // a newvar row ends at ref_len
                for (int64_t j = lane; j < stop; j += 64) {
                    const int b = aln_base_bin(aln, has_q, qp + j);
                    if (b > 3) continue;                                 // a low quality, N or no base at all
                    const int owner = (int)(int8_t)(uint8_t)(row[r + j] >> (8 * b));     // (consecutive lanes: coalesced)
                    if (owner >= 0 && owner < n_use) state = asm_merge(state, use[lo + owner]);
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

// A thread per alignment: one with label == unassigned[its sample] (whatever its mapq) whose fragment has ONE owner, a
// participant of the alignment's OWN sample, takes the owner's global label and joined = round; moved_owner[i] = that
// label or -1.  The participants are searched only for an alignment that is about to move.
__global__ __launch_bounds__(ASM_THREADS) void extend_move_samples_kernel(
    const int64_t *__restrict__ frag, int64_t n_aln, int64_t n_frag, const int32_t *__restrict__ aln_sample, int32_t S,
    const int32_t *__restrict__ unassigned, const int32_t *__restrict__ use, const int32_t *__restrict__ use_ptr,
    int32_t round, const int32_t *__restrict__ frag_state, int32_t *__restrict__ label, int32_t *__restrict__ joined,
    int32_t *__restrict__ moved_owner, uint32_t *n_moved) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_aln; i += (int64_t)gridDim.x * blockDim.x) {
        int32_t owner = -1;
        const int32_t s = aln_sample[i];
        if (s >= 0 && s < S) {
            const int32_t un = unassigned[s];
            if (un >= 0 && label[i] == un) {
                const int64_t f = frag[i];
                const int32_t state = (f >= 0 && f < n_frag) ? frag_state[f] : ASM_FRAG_EMPTY;
                if (state >= 0) {
                    bool own_sample = false;
                    for (int32_t k = use_ptr[s]; k < use_ptr[s + 1]; ++k) own_sample = own_sample || use[k] == state;
                    if (own_sample) {
                        owner = state;
                        label[i] = state;
                        joined[i] = round;
                        atomicAdd(&n_moved[s], 1u);
                    }
                }
            }
        }
        if (moved_owner != nullptr) moved_owner[i] = owner;
    }
}

#endif  // MIXEMT_ASSEMBLE_SAMPLES_KERNELS_HPP
