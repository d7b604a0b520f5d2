// samples_finish_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only.
// The second half of a cohort run, for the samples of one batched EM (samples_kernels.hpp): the contributor vote, the
// column gather, the refinement EM and the read assignment of MANY samples per launch (bin/mixemt:298-323 once per
// sample in the reference).
#ifndef MIXEMT_SAMPLES_FINISH_KERNELS_HPP
#define MIXEMT_SAMPLES_FINISH_KERNELS_HPP

// ------------------------------------------------------------------------------------------
// The rows of all samples sit back to back in one records matrix, cut into mxm_samples_plan's tiles (a tile never spans
// two samples).  After the column gather a sample is R_s x K_s with K_s <= 16: small enough for ONE workgroup to own a
// sample and run its whole refinement loop -- no grid barrier, no co-residency requirement, nothing read that another
// workgroup writes.  Everything a sample gets out of these kernels is a function of its own rows alone: the same bits
// whichever samples share the batch and wherever the sample stands in it.  No float atomics anywhere.
//   votes_best_samples_kernel     workgroup = tile: best[r] (and lse[r]) of the tile's rows under ITS sample's ln_props
//   votes_sum_samples_kernel      workgroup = sample: votes / counts / first-seen rows, rows in ascending order
//   gather_samples_kernel         workgroup = tile: out[r][i] = M[r][cols[s][i]], -inf in the pad columns
//   em_loop_samples_narrow_kernel workgroup = sample: em.py:126-143 on the sample's reduced matrix
//   assign_samples_kernel         workgroup = tile, thread = row: assemble.py:284-334 under the sample's columns
// A row without a usable record (ndist outside 1 .. 1024) is never dereferenced: best = -1, its sample's votes NaN and
// its state's error raised; gathered as NaN.
// ------------------------------------------------------------------------------------------
#define SFIN_THREADS 256
#define SFIN_KMAX 16

// numpy.argmax over candidates (nan flag, value, index): the first NaN wins, else the largest value, ties to the lower index
__device__ __forceinline__ bool sfin_better(int an, double av, int ai, int bn, double bv, int bi) {
    if (an != bn) return an > bn;
    if (an) return ai < bi;
    return av > bv || (av == bv && ai < bi);
}

template <bool WANT_LSE>
__global__ __launch_bounds__(SFIN_THREADS) void votes_best_samples_kernel(
    const uint8_t *__restrict__ rec, const int64_t *__restrict__ rec_off, const int32_t *__restrict__ ndist, int ldc, int H,
    const mxm_sample_tile *__restrict__ tiles, const double *__restrict__ ln_props, const double *__restrict__ props,
    const double *__restrict__ rowmax, int32_t *__restrict__ best, double *__restrict__ lse) {
    __shared__ double s_m[ENC_MAX_WIDE], s_p[WANT_LSE ? ENC_MAX_WIDE : 1];
    __shared__ double s_val[SFIN_THREADS];
    __shared__ int s_idx[SFIN_THREADS], s_nan[SFIN_THREADS];
    __shared__ double s_red[4];
    const int t = threadIdx.x;
    const int sample = tiles[blockIdx.x].sample, count = tiles[blockIdx.x].count;
    const int64_t first = tiles[blockIdx.x].first;
    const double *lp = ln_props + (int64_t)sample * H;
    const double *pp = WANT_LSE ? props + (int64_t)sample * H : nullptr;
    for (int i = 0; i < count; ++i) {                       // uniform
        const int64_t r = first + i;
        const int nd = ndist[r];
        if (nd <= 0 || nd > ENC_MAX_WIDE) {                  // no usable record: not dereferenced
            if (t == 0) {
                best[r] = -1;
                if (WANT_LSE) lse[r] = __builtin_nan("");
            }
            continue;
        }
        const bool wide = nd > ENC_MAX_CODES;
        const uint8_t *codes = rec + rec_off[r];
        const double *ptab = reinterpret_cast<const double *>(codes + rec_code_bytes(nd, ldc));
        __syncthreads();                                    // the tables of the row before have been read
        for (int j = t; j < nd; j += SFIN_THREADS) {
            s_m[j] = ptab[nd + j];
            if (WANT_LSE) s_p[j] = ptab[j];
        }
        __syncthreads();
        int cn = 0, ci = 0x7fffffff;
        double cv = -INFINITY;
        for (int h = t; h < H; h += SFIN_THREADS) {          // ascending: a thread keeps its first maximum
            int code = rec_code_at(codes, h, wide);
            if (code >= nd) code = 0;
            const double v = lp[h] + s_m[code];
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
        if constexpr (WANT_LSE) {
            const double v = coded_row_lse(codes, wide, s_p, s_m, pp, lp, rowmax[r], H, s_red);
            if (t == 0) lse[r] = v;
        }
    }
}

// votes[s][h] = sum of w[r] over the sample's rows with best[r] == h, counts[s][h] their number, first[s][h] the
// smallest such row counted from the sample's first (R_s: none).  Thread t owns the haplogroups h = t (mod 256): it walks
// the sample's rows in ascending order and adds the ones that are its own, so every sum has ONE fixed order.
// Dynamic LDS: H doubles + 2 H ints.
__global__ __launch_bounds__(SFIN_THREADS) void votes_sum_samples_kernel(
    const int32_t *__restrict__ best, const double *__restrict__ w, const int64_t *__restrict__ row0, int H,
    double *__restrict__ votes, int64_t *__restrict__ counts, int64_t *__restrict__ first_seen, mxm_em_state *__restrict__ state) {
    extern __shared__ double sfin_lds[];
    double *s_votes = sfin_lds;
    int *s_count = reinterpret_cast<int *>(sfin_lds + H);
    int *s_first = s_count + H;
    __shared__ int s_best[SFIN_THREADS];
    __shared__ double s_w[SFIN_THREADS];
    __shared__ int s_bad;
    const int t = threadIdx.x, s = blockIdx.x;
    const int64_t lo = row0[s], n = row0[s + 1] - lo;
    const int none = (int)(n < 0x7fffffff ? n : 0x7fffffff);
    for (int h = t; h < H; h += SFIN_THREADS) { s_votes[h] = 0.0; s_count[h] = 0; s_first[h] = none; }
    if (t == 0) s_bad = 0;
    for (int64_t q = 0; q < n; q += SFIN_THREADS) {
        __syncthreads();                                    // the block before has been read (and the clears are done)
        const int here = (int)((n - q) < SFIN_THREADS ? (n - q) : SFIN_THREADS);
        if (t < here) {
            const int b = best[lo + q + t];
            s_best[t] = b;
            s_w[t] = (w != nullptr) ? w[lo + q + t] : 1.0;
            if (b < 0 || b >= H) s_bad = 1;
        }
        __syncthreads();
        for (int i = 0; i < here; ++i) {
            const int b = s_best[i];
            if (b >= 0 && b < H && (b & (SFIN_THREADS - 1)) == t) {
                s_votes[b] += s_w[i];
                s_count[b] += 1;
                if (s_first[b] == none) s_first[b] = (int)(q + i);
            }
        }
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    for (int h = t; h < H; h += SFIN_THREADS) {
        votes[(int64_t)s * H + h] = bad ? __builtin_nan("") : s_votes[h];
        if (counts != nullptr) counts[(int64_t)s * H + h] = s_count[h];
        first_seen[(int64_t)s * H + h] = (s_first[h] == none) ? n : (int64_t)s_first[h];
    }
    if (bad && t == 0 && state != nullptr) state[s].error = 1;
}

// out[r][i] = M[r][cols[s][i]] from the records' log tables (preprocess.py:247-251), -inf in the pad columns
__global__ __launch_bounds__(SFIN_THREADS) void gather_samples_kernel(
    const uint8_t *__restrict__ rec, const int64_t *__restrict__ rec_off, const int32_t *__restrict__ ndist, int ldc,
    const mxm_sample_tile *__restrict__ tiles, const int32_t *__restrict__ cols, const int32_t *__restrict__ ncol, int ld,
    double *__restrict__ out) {
    const int sample = tiles[blockIdx.x].sample, count = tiles[blockIdx.x].count;
    const int64_t first = tiles[blockIdx.x].first;
    const int nc = ncol[sample];
    const int32_t *cs = cols + (int64_t)sample * ld;
    for (int e = threadIdx.x; e < count * ld; e += SFIN_THREADS) {
        const int64_t r = first + e / ld;
        const int i = e % ld;
        double v = -INFINITY;
        if (i < nc) {
            const int nd = ndist[r];
            if (nd <= 0 || nd > ENC_MAX_WIDE) {
                v = __builtin_nan("");
            } else {
                const uint8_t *codes = rec + rec_off[r];
                const double *mtab = reinterpret_cast<const double *>(codes + rec_code_bytes(nd, ldc)) + nd;
                int code = rec_code_at(codes, cs[i], nd > ENC_MAX_CODES);
                if (code >= nd) code = 0;
                v = mtab[code];
            }
        }
        out[r * ld + i] = v;
    }
}

// column k of a K-column row takes part: every k < K, or (MASKED: the fits of support_kernels.hpp) the bits of mask, all of
// them below K.  A column that does not is a pad column to everything below.
template <bool MASKED>
__device__ __forceinline__ bool sfin_col_on(int k, int K, uint32_t mask) {
    return MASKED ? ((mask >> k) & 1u) != 0 : k < K;
}

// e[k] = exp(x[k] - rowmax) of one reduced row x [LD] with K columns: 0 in the pad columns, no shift for a row without a
// finite maximum (the maximum is over the columns that take part)
template <int LD, bool MASKED = false>
__device__ __forceinline__ void sfin_linear_row(const double *__restrict__ row, int K, double (&e)[LD], uint32_t mask = 0) {
    double x[LD];
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        x[k] = sfin_col_on<MASKED>(k, K, mask) ? row[k] : -INFINITY;
        m = fmax(m, x[k]);
    }
    const double shift = isfinite(m) ? m : 0.0;
#pragma unroll
    for (int k = 0; k < LD; ++k) e[k] = exp(x[k] - shift);  // exp(-inf) = 0
}

// ------------------------------------------------------------------------------------------
// The refinement EM of one sample per workgroup (em.py:126-143 on R_s x K_s, K_s <= LD): em_fused_narrow_kernel's
// arithmetic and its stop / resume contract, without its grid -- the sample's rows are dealt over the workgroup's
// threads (thread t: rows t, t + T, ...), the wave sums go through wave_sum_lane63 and then the waves in ascending
// order, and EVERY thread forms the update from the same LDS values (mxm_m_finalize's own form), so all take the same
// stop decision.  e = exp(M - rowmax) is formed once per launch: into LDS (column by column, K_s x R_s doubles: consecutive
// lanes read consecutive words) when the sample fits
// lds_doubles, else into the global copy E [R][LD], which the iterations then re-read.  A launch runs at most `chunk`
// iterations; the host re-launches until every state is done.
// ------------------------------------------------------------------------------------------
// The loop of ONE workgroup on n rows x K columns: Ms / Es / ws point at the sample's first row, ln_cur / ln_new /
// props_cur [LD] and st at the entry's own tables.  E_READY: a pass before the launch has formed the sample's e in Es
// (samples_runs_kernels.hpp: several workgroups share one sample there), so this workgroup only reads it.
// MASKED (support_kernels.hpp): the fit's columns are the bits of mask instead of all k < K; whether the sample fits LDS
// is still judged on n x K, and column k keeps its place k * n there.
template <int LD, bool E_READY, bool MASKED = false>
__device__ __forceinline__ void sfin_em_loop_body(const double *__restrict__ Ms, double *__restrict__ Es, const double *__restrict__ ws,
                                                  int64_t n, int K, double *__restrict__ ln_cur, double *__restrict__ ln_new,
                                                  double *__restrict__ props_cur, mxm_em_state *__restrict__ st, double tol,
                                                  int max_iter, int chunk, int lds_doubles, uint32_t mask = 0) {
    constexpr int THREADS = SFIN_THREADS, NW = THREADS / 64;
    extern __shared__ double sfin_e[];
    __shared__ double s_red[LD][NW];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const bool in_lds = n * K <= (int64_t)lds_doubles;     // uniform

    // ---- linearise once: e = exp(M - rowmax), pad columns 0 ----
    for (int64_t r = t; r < n && (in_lds || !E_READY); r += THREADS) {
        double e[LD];
        sfin_linear_row<LD, MASKED>(Ms + r * LD, K, e, mask);
#pragma unroll
        for (int k = 0; k < LD; ++k) {
            if (in_lds) {
                if (sfin_col_on<MASKED>(k, K, mask)) sfin_e[k * n + r] = e[k];
            } else {
                Es[r * LD + k] = e[k];
            }
        }
    }
    // (a thread reads back only what it wrote itself: no barrier needed for e)

    int iters = st->iters, done = 0;
    double l1 = 0.0;
    double lc[LD], p[LD], ln_next[LD];
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        lc[k] = sfin_col_on<MASKED>(k, K, mask) ? ln_cur[k] : -INFINITY;
        p[k] = sfin_col_on<MASKED>(k, K, mask) ? (iters > 0 ? props_cur[k] : exp(lc[k])) : 0.0;
        ln_next[k] = lc[k];
    }
    for (int it = 0; it < chunk && done == 0; ++it) {
        double acc[LD];
#pragma unroll
        for (int k = 0; k < LD; ++k) acc[k] = 0.0;
        for (int64_t r = t; r < n; r += THREADS) {
            double e[LD];
#pragma unroll
            for (int k = 0; k < LD; ++k) e[k] = in_lds ? (sfin_col_on<MASKED>(k, K, mask) ? sfin_e[k * n + r] : 0.0) : Es[r * LD + k];
            double z = 0.0;
#pragma unroll
            for (int k = 0; k < LD; ++k) z = fma(p[k], e[k], z);
            const double c = weight_over_norm(ws != nullptr ? ws[r] : 1.0, z);
#pragma unroll
            for (int k = 0; k < LD; ++k) acc[k] = fma(c, e[k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < LD; ++k) {
            const double a = wave_sum_lane63(acc[k]);
            if (lane == 63) s_red[k][wv] = a;
        }
        __syncthreads();
        double T[LD], tot = 0.0;
#pragma unroll
        for (int k = 0; k < LD; ++k) {
            double a = 0.0;
            if (sfin_col_on<MASKED>(k, K, mask)) {
                a = s_red[k][0];
#pragma unroll
                for (int q = 1; q < NW; ++q) a += s_red[k][q];
            }
            T[k] = a;
            tot = fma(p[k], a, tot);                       // p = 0 past the sample's columns
        }
        __syncthreads();                                    // s_red is free for the next iteration
        const double ltot = log(tot);
        l1 = 0.0;
        double pn[LD];
#pragma unroll
        for (int k = 0; k < LD; ++k) {
            if (sfin_col_on<MASKED>(k, K, mask)) {
                ln_next[k] = lc[k] + log(T[k]) - ltot;      // em.py:87-89
                pn[k] = exp(ln_next[k]);
                l1 += fabs(pn[k] - p[k]);                   // em.py:53-54
            } else {
                pn[k] = 0.0;
            }
        }
        ++iters;
        const bool conv = l1 < tol;
        done = conv ? 1 : (iters >= max_iter ? 2 : 0);
        if (done == 0) {                                    // em.py:140: props <- new_props
#pragma unroll
            for (int k = 0; k < LD; ++k) {
                lc[k] = ln_next[k];
                p[k] = pn[k];
            }
        }
    }
    // ---- results: ln_cur = log theta_k, props_cur = exp of it, ln_new = log theta_{k+1} ----
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        if (t == k && k < K) {
            ln_cur[k] = lc[k];
            props_cur[k] = p[k];
            if (done > 0 || !sfin_col_on<MASKED>(k, K, mask)) ln_new[k] = ln_next[k];   // (a masked-out column: -inf, 0, -inf)
        }
    }
    if (t == 0) {
        st->iters = iters;
        st->l1 = l1;
        st->done = done;
    }
}

template <int LD>
__global__ __launch_bounds__(SFIN_THREADS, 2) void em_loop_samples_narrow_kernel(
    const double *__restrict__ M, double *__restrict__ E, const double *__restrict__ w, const int64_t *__restrict__ row0,
    const int32_t *__restrict__ ncol, double *__restrict__ ln_cur, double *__restrict__ ln_new, double *__restrict__ props_cur,
    mxm_em_state *__restrict__ state, double tol, int max_iter, int chunk, int lds_doubles) {
    const int s = blockIdx.x;
    mxm_em_state *st = state + s;
    if (st->done != 0) return;                             // written before the launch
    const int K = ncol[s];
    if (K < 1 || K > LD) return;
    const int64_t lo = row0[s], n = row0[s + 1] - lo;
    sfin_em_loop_body<LD, false>(M + lo * LD, E + lo * LD, (w != nullptr) ? w + lo : nullptr, n, K, ln_cur + (int64_t)s * LD,
                                 ln_new + (int64_t)s * LD, props_cur + (int64_t)s * LD, st, tol, max_iter, chunk, lds_doubles);
}

// ------------------------------------------------------------------------------------------
// Read -> contributor assignment of many samples (assemble.py:284-334 per row): X_c = (ln_theta[s][c] + M[r][c]) - lse_r
// with lse_r = rowmax_r + log sum_c props[s][c] exp(M[r][c] - rowmax_r) over the sample's columns (or the caller's lse[r]:
// the first EM's full-width normaliser), v_c = X_c - log_props[s][c]; the best goes to perm[s][c] when it beats the
// runner-up by log_min_fold, else -1.  Exactly equal values: the larger column wins, as in assign_reads_kernel.
// ------------------------------------------------------------------------------------------
template <int LD>
__global__ __launch_bounds__(64) void assign_samples_kernel(
    const double *__restrict__ M, const mxm_sample_tile *__restrict__ tiles, const int32_t *__restrict__ ncol,
    const int32_t *__restrict__ perm, const double *__restrict__ ln_theta, const double *__restrict__ props,
    const double *__restrict__ log_props, const double *__restrict__ lse_in, double log_min_fold,
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
    double x[LD];
    double m = -INFINITY;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        x[k] = (k < K) ? M[r * LD + k] : -INFINITY;
        m = fmax(m, x[k]);
    }
    double lse;
    if (lse_in != nullptr) {
        lse = lse_in[r];
    } else {
        const double shift = isfinite(m) ? m : 0.0;
        double z = 0.0;
#pragma unroll
        for (int k = 0; k < LD; ++k) z = fma((k < K) ? props[so + k] : 0.0, exp(x[k] - shift), z);
        lse = shift + log(z);
        if (!lse_linear_ok(z)) {                            // the columns underflow (common.hpp): in log space, as mxm_em_step does
            double mm = -INFINITY;
#pragma unroll
            for (int k = 0; k < LD; ++k)
                if (k < K) mm = fmax(mm, ln_theta[so + k] + x[k]);
            const double sh = (mm > -INFINITY && mm < INFINITY) ? mm : 0.0;
            double sacc = 0.0;
#pragma unroll
            for (int k = 0; k < LD; ++k)
                if (k < K) sacc += exp((ln_theta[so + k] + x[k]) - sh);
            lse = log(sacc) + mm;
        }
    }
    double v1 = -INFINITY, v2 = -INFINITY;                  // best, runner-up
    int c1 = -1, c2 = -1;
#pragma unroll
    for (int k = 0; k < LD; ++k) {
        if (k < K) {
            const double X = (ln_theta[so + k] + x[k]) - lse;
            if (post != nullptr) post[r * LD + k] = X;
            const double v = X - log_props[so + k];
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

#endif  // MIXEMT_SAMPLES_FINISH_KERNELS_HPP
