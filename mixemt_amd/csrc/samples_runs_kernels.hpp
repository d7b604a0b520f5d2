// samples_runs_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only, after
// samples_finish_kernels.hpp, whose one-run kernels these are the several-run forms of.
// The second half of a cohort run for samples whose EM ran B times (mixemt's -M): run_em returns the posteriors of its
// runs folded with logaddexp in run order (em.py:145-161), and the vote and the read assignment work on that fold.
#ifndef MIXEMT_SAMPLES_RUNS_KERNELS_HPP
#define MIXEMT_SAMPLES_RUNS_KERNELS_HPP

// ------------------------------------------------------------------------------------------
// Every per-run table is [S][B][...], run-major inside a sample; B <= SRUN_MAX.  As in samples_finish_kernels.hpp, what a
// sample gets out of these kernels is a function of its own rows and tables alone, and there are no float atomics.
//   votes_best_samples_runs_kernel   workgroup = tile: best[r] (and lse[r][b]) of the tile's rows under ITS sample's runs;
//                                    votes_sum_samples_kernel then sums the votes as for one run (it only reads best)
//   linearise_samples_runs_kernel    workgroup = tile: e = exp(M - rowmax) of the samples too large for LDS, once per call
//   em_loop_samples_narrow_runs_kernel  workgroup = (sample, run): sfin_em_loop_body, the one-run kernel's own loop
//   assign_samples_runs_kernel       workgroup = tile, thread = row: the assignment under the folded reduced posterior
// ------------------------------------------------------------------------------------------
#define SRUN_MAX 64
static_assert(SRUN_MAX == MXM_SAMPLES_RUNS_MAX, "the header's cap is the kernels' LDS table");

// best[r] = first index of max_h of the fold over the runs of (ln_props[s][b][h] + M[r][h]) - lse_b[r]: the arithmetic of
// posterior_argmax_kernel<true> (records_kernels.hpp) with the run tables of the row's sample.  The row's value tables
// stay in LDS across the B normaliser passes (coded_row_lse) and the fold; so do the B normalisers.
__global__ __launch_bounds__(SFIN_THREADS) void votes_best_samples_runs_kernel(
    const uint8_t *__restrict__ rec, const int64_t *__restrict__ rec_off, const int32_t *__restrict__ ndist, int ldc, int H, int B,
    const mxm_sample_tile *__restrict__ tiles, const double *__restrict__ ln_props, const double *__restrict__ props,
    const double *__restrict__ rowmax, int32_t *__restrict__ best, double *__restrict__ lse) {
    __shared__ double s_m[ENC_MAX_WIDE], s_p[ENC_MAX_WIDE];
    __shared__ double s_lse[SRUN_MAX];
    __shared__ double s_val[SFIN_THREADS];
    __shared__ int s_idx[SFIN_THREADS], s_nan[SFIN_THREADS];
    __shared__ double s_red[4];
    const int t = threadIdx.x;
    const int sample = tiles[blockIdx.x].sample, count = tiles[blockIdx.x].count;
    const int64_t first = tiles[blockIdx.x].first;
    const double *lp = ln_props + (int64_t)sample * B * H;
    const double *pp = props + (int64_t)sample * B * H;
    for (int i = 0; i < count; ++i) {                       // uniform
        const int64_t r = first + i;
        const int nd = ndist[r];
        if (nd <= 0 || nd > ENC_MAX_WIDE) {                  // no usable record: not dereferenced
            if (t == 0) best[r] = -1;
            if (lse != nullptr && t < B) lse[r * B + t] = __builtin_nan("");
            continue;
        }
        const bool wide = nd > ENC_MAX_CODES;
        const uint8_t *codes = rec + rec_off[r];
        const double *ptab = reinterpret_cast<const double *>(codes + rec_code_bytes(nd, ldc));
        __syncthreads();                                    // the tables and normalisers of the row before have been read
        for (int j = t; j < nd; j += SFIN_THREADS) {
            s_p[j] = ptab[j];
            s_m[j] = ptab[nd + j];
        }
        __syncthreads();
        for (int b = 0; b < B; ++b) {                       // uniform; the helper holds barriers
            const double v = coded_row_lse(codes, wide, s_p, s_m, pp + (int64_t)b * H, lp + (int64_t)b * H, rowmax[r], H, s_red);
            if (t == 0) s_lse[b] = v;
        }
        __syncthreads();
        if (lse != nullptr && t < B) lse[r * B + t] = s_lse[t];
        int cn = 0, ci = 0x7fffffff;
        double cv = -INFINITY;
        for (int h = t; h < H; h += SFIN_THREADS) {          // ascending: a thread keeps its first maximum
            const double m = s_m[rec_code_at(codes, h, wide)];
            double v = lp[h] + m;
            v -= s_lse[0];
            for (int b = 1; b < B; ++b) v = logaddexp_f64(v, (lp[(int64_t)b * H + h] + m) - s_lse[b]);   // h consecutive across lanes
            const int vn = (v != v) ? 1 : 0;
            if (sfin_better(vn, v, h, cn, cv, ci)) { cn = vn; cv = v; ci = h; }
        }
        s_val[t] = cv; s_idx[t] = ci; s_nan[t] = cn;
        __syncthreads();
        for (int half = SFIN_THREADS / 2; half > 0; half >>= 1) {
            if (t < half && sfin_better(s_nan[t + half], s_val[t + half], s_idx[t + half], s_nan[t], s_val[t], s_idx[t])) {
                s_nan[t] = s_nan[t + half]; s_val[t] = s_val[t + half]; s_idx[t] = s_idx[t + half];
            }
            __syncthreads();
        }
        if (t == 0) best[r] = (s_idx[0] >= H) ? 0 : s_idx[0];
    }
}

// E[r][:] = exp(M[r][:] - rowmax_r) for the rows of the samples that do not fit the loop's LDS (more than lds_cells
// cells): the loop's own sfin_linear_row, once per call, so that the B workgroups of a sample only read E.
template <int LD>
__global__ __launch_bounds__(64) void linearise_samples_runs_kernel(
    const double *__restrict__ M, const mxm_sample_tile *__restrict__ tiles, const int64_t *__restrict__ row0,
    const int32_t *__restrict__ ncol, int lds_cells, double *__restrict__ E) {
    const int sample = tiles[blockIdx.x].sample, count = tiles[blockIdx.x].count;
    const int K = ncol[sample];
    if (K < 1 || K > LD || (row0[sample + 1] - row0[sample]) * K <= (int64_t)lds_cells) return;
    for (int i = threadIdx.x; i < count; i += 64) {
        const int64_t r = tiles[blockIdx.x].first + i;
        double e[LD];
        sfin_linear_row<LD>(M + r * LD, K, e);
#pragma unroll
        for (int k = 0; k < LD; ++k) E[r * LD + k] = e[k];
    }
}

// workgroup s * B + b: run b of sample s -- the one-run kernel's loop on the sample's rows and the entry's own tables
template <int LD>
__global__ __launch_bounds__(SFIN_THREADS, 2) void em_loop_samples_narrow_runs_kernel(
    const double *__restrict__ M, double *__restrict__ E, const double *__restrict__ w, const int64_t *__restrict__ row0,
    const int32_t *__restrict__ ncol, int B, double *__restrict__ ln_cur, double *__restrict__ ln_new,
    double *__restrict__ props_cur, mxm_em_state *__restrict__ state, double tol, int max_iter, int chunk, int lds_doubles) {
    const int entry = blockIdx.x, s = entry / B;
    mxm_em_state *st = state + entry;
    if (st->done != 0) return;                             // written before the launch: a finished run stays as it is
    const int K = ncol[s];
    if (K < 1 || K > LD) return;
    const int64_t lo = row0[s], n = row0[s + 1] - lo;
    sfin_em_loop_body<LD, true>(M + lo * LD, E + lo * LD, (w != nullptr) ? w + lo : nullptr, n, K, ln_cur + (int64_t)entry * LD,
                                ln_new + (int64_t)entry * LD, props_cur + (int64_t)entry * LD, st, tol, max_iter, chunk,
                                lds_doubles);
}

// ------------------------------------------------------------------------------------------
// assign_samples_kernel under B runs: X_c = fold over b, in run order, of logaddexp((ln_theta[s][b][c] + M[r][c]) - L_b)
// with L_b the run's row normaliser as assign_samples_kernel forms it (or the caller's lse[r][b]), then + neg_log_runs
// (-log B, formed by the host as the per-sample path forms it) as one addition; v_c = X_c - log_props[s][c].
// ------------------------------------------------------------------------------------------
template <int LD>
__global__ __launch_bounds__(64) void assign_samples_runs_kernel(
    const double *__restrict__ M, const mxm_sample_tile *__restrict__ tiles, const int32_t *__restrict__ ncol,
    const int32_t *__restrict__ perm, int B, const double *__restrict__ ln_theta, const double *__restrict__ props,
    const double *__restrict__ log_props, const double *__restrict__ lse_in, double neg_log_runs, double log_min_fold,
    int32_t *__restrict__ assigned, double *__restrict__ post) {
    const int sample = tiles[blockIdx.x].sample, count = tiles[blockIdx.x].count;
    const int t = threadIdx.x;
    if (t >= count) return;
    const int64_t r = tiles[blockIdx.x].first + t;
    const int K = ncol[sample];
    if (K <= 1) {
        assigned[r] = 0;
        if (post == nullptr || K < 1) return;
    }
    const int64_t so = (int64_t)sample * LD;
    double x[LD], X[LD];
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        x[k] = (k < K) ? M[r * LD + k] : -INFINITY;
        m = fmax(m, x[k]);
    }
    const double shift = isfinite(m) ? m : 0.0;
    for (int b = 0; b < B; ++b) {
        const double *lt = ln_theta + ((int64_t)sample * B + b) * LD;
        double lse;
        if (lse_in != nullptr) {
            lse = lse_in[r * B + b];
        } else {
            const double *pr = props + ((int64_t)sample * B + b) * LD;
            double z = 0.0;
#pragma unroll
            for (int k = 0; k < LD; ++k) z = fma((k < K) ? pr[k] : 0.0, exp(x[k] - shift), z);
            lse = shift + log(z);
            if (!lse_linear_ok(z)) {                        // the columns underflow (common.hpp): in log space, as mxm_em_step does
                double mm = -INFINITY;
#pragma unroll
                for (int k = 0; k < LD; ++k)
                    if (k < K) mm = fmax(mm, lt[k] + x[k]);
                const double sh = (mm > -INFINITY && mm < INFINITY) ? mm : 0.0;
                double sacc = 0.0;
#pragma unroll
                for (int k = 0; k < LD; ++k)
                    if (k < K) sacc += exp((lt[k] + x[k]) - sh);
                lse = log(sacc) + mm;
            }
        }
#pragma unroll
        for (int k = 0; k < LD; ++k) {
            if (k < K) {
                const double v = (lt[k] + x[k]) - lse;
                X[k] = (b == 0) ? v : logaddexp_f64(X[k], v);
            }
        }
    }
    double v1 = -INFINITY, v2 = -INFINITY;                  // best, runner-up
    int c1 = -1, c2 = -1;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        if (k < K) {
            const double Xk = X[k] + neg_log_runs;
            if (post != nullptr) post[r * LD + k] = Xk;
            const double v = Xk - log_props[so + k];
            if (c1 < 0 || v > v1 || v == v1) {              // (columns ascend: an equal value in a later column wins)
                v2 = v1; c2 = c1;
                v1 = v; c1 = k;
            } else if (c2 < 0 || v > v2 || v == v2) {
                v2 = v; c2 = k;
            }
        } else if (post != nullptr) {
            post[r * LD + k] = -INFINITY;
        }
    }
    if (K >= 2) assigned[r] = ((v1 - v2) >= log_min_fold) ? perm[so + c1] : -1;
}

#endif  // MIXEMT_SAMPLES_RUNS_KERNELS_HPP
