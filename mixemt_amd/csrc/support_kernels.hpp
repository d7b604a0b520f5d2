// support_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only, after
// samples_finish_kernels.hpp, whose loop body these kernels run over SUBSETS of a sample's columns.
// Nested-model fits of the refinement EM (include/mixemt_hip_support.h): B fits per sample, each a column mask.
#ifndef MIXEMT_SUPPORT_KERNELS_HPP
#define MIXEMT_SUPPORT_KERNELS_HPP

// ------------------------------------------------------------------------------------------
// Every per-fit table is [S][B][...]; fit (s, b) has the 32-bit column mask masks[s * B + b], all of its bits below
// ncol[s]; mask 0 is an unused slot that no kernel touches.  As in samples_finish_kernels.hpp, what a fit gets out of these
// kernels is a function of its sample's rows, its mask and its own tables alone, and there are no float atomics.
//   em_loop_samples_narrow_masks_kernel  workgroup = (sample, fit): sfin_em_loop_body<.., MASKED> -- the one-run loop with a
//                                        masked-out column treated as a pad column; a sample too large for LDS keeps its
//                                        e = exp(M - rowmax over the MASK) in the fit's own slice of E
//   loglik_samples_masks_kernel          workgroup = (sample, fit): ll = sum_r w_r log sum_{k in mask} p_k exp(M_rk)
// ------------------------------------------------------------------------------------------
#define SUP_MAX_FITS 256
static_assert(SUP_MAX_FITS == MXM_SUPPORT_MAX_FITS, "the header's cap is the kernels'");

// workgroup s * B + b: fit b of sample s.  E slice: (B * row0[s] + b * R_s) * LD, R_s * LD doubles, this workgroup's alone.
template <int LD>
__global__ __launch_bounds__(SFIN_THREADS, 2) void em_loop_samples_narrow_masks_kernel(
    const double *__restrict__ M, double *__restrict__ E, const double *__restrict__ w, const int64_t *__restrict__ row0,
    const int32_t *__restrict__ ncol, const uint32_t *__restrict__ masks, int B, double *__restrict__ ln_cur,
    double *__restrict__ ln_new, double *__restrict__ props_cur, mxm_em_state *__restrict__ state, double tol, int max_iter,
    int chunk, int lds_doubles) {
    const int entry = blockIdx.x, s = entry / B, b = entry - s * B;
    const uint32_t mask = masks[entry];
    if (mask == 0) return;                                 // an unused slot: its tables and its state are not touched
    mxm_em_state *st = state + entry;
    if (st->done != 0) return;                             // written before the launch: a finished fit stays as it is
    const int K = ncol[s];
    if (K < 1 || K > LD || (mask >> K) != 0) return;       // (the host has refused these)
    const int64_t lo = row0[s], n = row0[s + 1] - lo;
    sfin_em_loop_body<LD, false, true>(M + lo * LD, E + ((int64_t)B * lo + (int64_t)b * n) * LD, (w != nullptr) ? w + lo : nullptr, n,
                                       K, ln_cur + (int64_t)entry * LD, ln_new + (int64_t)entry * LD,
                                       props_cur + (int64_t)entry * LD, st, tol, max_iter, chunk, lds_doubles, mask);
}

// the sum of v over the workgroup: the wave sums through wave_sum_lane63, then the waves in ascending order; every thread
// gets it.  All SFIN_THREADS threads must call it.
__device__ __forceinline__ double sup_block_sum(double v, double *s_red) {
    constexpr int NW = SFIN_THREADS / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double a = wave_sum_lane63(v);
    if (lane == 63) s_red[wv] = a;
    __syncthreads();
    double total = s_red[0];
#pragma unroll
    for (int q = 1; q < NW; ++q) total += s_red[q];
    __syncthreads();                                        // s_red is free again
    return total;
}

// ll[s][b] = sum over the sample's rows, thread t taking rows t, t + T, ... in ascending order, of
// w_r (m_r + log sum_{k in mask} p_k exp(M_rk - m_r)) with m_r the row's maximum over the mask and p = exp(ln_props[s][b]);
// a row whose linear sum lse_linear_ok refuses (common.hpp) is redone in log space with a max shift of ln p_k + M_rk, as
// assign_samples_kernel redoes it.  A row of weight 0 is skipped (weight_over_norm skips it); a row of weight != 0
// without a finite masked-in cell gives -inf.  Fit 0's workgroup also writes n_eff[s] = sum of w, in the same order --
// whether or not slot 0 is used.
template <int LD>
__global__ __launch_bounds__(SFIN_THREADS) void loglik_samples_masks_kernel(
    const double *__restrict__ M, const double *__restrict__ w, const int64_t *__restrict__ row0, const int32_t *__restrict__ ncol,
    const uint32_t *__restrict__ masks, int B, const double *__restrict__ ln_props, double *__restrict__ ll,
    double *__restrict__ n_eff) {
    __shared__ double s_red[SFIN_THREADS / 64];
    const int t = threadIdx.x, entry = blockIdx.x, s = entry / B, b = entry - s * B;
    const int64_t lo = row0[s], n = row0[s + 1] - lo;
    if (b == 0) {                                           // uniform
        double part = 0.0;
        for (int64_t r = t; r < n; r += SFIN_THREADS) part += (w != nullptr) ? w[lo + r] : 1.0;
        const double total = sup_block_sum(part, s_red);
        if (t == 0) n_eff[s] = total;
    }
    const uint32_t mask = masks[entry];
    const int K = ncol[s];
    if (mask == 0 || K < 1 || K > LD || (mask >> K) != 0) return;   // uniform: an unused slot (the host has refused the rest)
    double p[LD], lnp[LD];
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        lnp[k] = sfin_col_on<true>(k, K, mask) ? ln_props[(int64_t)entry * LD + k] : -INFINITY;
        p[k] = sfin_col_on<true>(k, K, mask) ? exp(lnp[k]) : 0.0;
    }
    double acc = 0.0;
    for (int64_t r = t; r < n; r += SFIN_THREADS) {
        const double wr = (w != nullptr) ? w[lo + r] : 1.0;
        if (wr == 0.0) continue;
        const double *row = M + (lo + r) * LD;
        double x[LD];
        double m = -INFINITY;
#pragma unroll
        for (int k = 0; k < LD; ++k) {
            x[k] = sfin_col_on<true>(k, K, mask) ? row[k] : -INFINITY;
            m = fmax(m, x[k]);
        }
        const double shift = isfinite(m) ? m : 0.0;
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < LD; ++k) z = fma(p[k], exp(x[k] - shift), z);
        double lse = shift + log(z);
        if (!lse_linear_ok(z)) {                            // the columns underflow (common.hpp): in log space
            double mm = -INFINITY;
#pragma unroll
            for (int k = 0; k < LD; ++k)
                if (sfin_col_on<true>(k, K, mask)) mm = fmax(mm, lnp[k] + x[k]);
            const double sh = (mm > -INFINITY && mm < INFINITY) ? mm : 0.0;
            double sacc = 0.0;
#pragma unroll
            for (int k = 0; k < LD; ++k)
                if (sfin_col_on<true>(k, K, mask)) sacc += exp((lnp[k] + x[k]) - sh);
            lse = log(sacc) + mm;
        }
        acc += wr * lse;
    }
    const double total = sup_block_sum(acc, s_red);
    if (t == 0) ll[entry] = total;
}

#endif  // MIXEMT_SUPPORT_KERNELS_HPP
