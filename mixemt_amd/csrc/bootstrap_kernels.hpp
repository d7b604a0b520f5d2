// bootstrap_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only, after
// samples_runs_kernels.hpp, whose (sample, run) loop these kernels reuse with resampled row weights.
// A non-parametric bootstrap of the refinement EM (include/mixemt_hip_bootstrap.h): B replicates per sample.
#ifndef MIXEMT_BOOTSTRAP_KERNELS_HPP
#define MIXEMT_BOOTSTRAP_KERNELS_HPP

// ------------------------------------------------------------------------------------------
// Every per-replicate table is [S][B][...]; the weights are wb[B * row0[s] + b * R_s + i].  What a sample gets out of
// these kernels is a function of its own rows, its tables and (seed, s_id[s], b) alone; the only atomics are on integers.
//   boot_prefix_kernel        workgroup = sample: checks w, cum[r] = the inclusive prefix sum of w inside the sample
//   boot_draw_kernel<GLOBAL>  workgroup = (sample, replicate): N_s Philox draws, counted in LDS (a sample of at most
//                             BOOT_LDS_ROWS rows) or in the workspace's 32-bit counters (GLOBAL)
//   em_loop_samples_narrow_boot_kernel  workgroup = (sample, replicate): sfin_em_loop_body on the replicate's weights
//   boot_summary_kernel       workgroup = (column, sample): exp, bitonic sort in LDS, quantiles, mean, sd
//   boot_flag_kernel          thread = sample: flag[s] from the NaN of its columns' lo
// ------------------------------------------------------------------------------------------
#define BOOT_MAX 4096
#define BOOT_LDS_ROWS 8192
#define BOOT_THREADS 256
#define BOOT_CHUNK 64                // replicates whose rows' global counters the workspace holds at a time
static_assert(BOOT_MAX == MXM_BOOTSTRAP_MAX && BOOT_LDS_ROWS == MXM_BOOTSTRAP_LDS_ROWS, "the header's limits are the kernels'");
static_assert(BOOT_LDS_ROWS * 8 <= 64 * 1024, "a prefix sum and a counter per row within the LDS a workgroup gets without the opt-in");

// ntot[s]: N_s, or -1 (a weight that is no non-negative integer), -2 (N_s = 0 or N_s >= 2^31)
__global__ __launch_bounds__(BOOT_THREADS) void boot_prefix_kernel(const double *__restrict__ w, const int64_t *__restrict__ row0,
                                                                  uint32_t *__restrict__ cum, int64_t *__restrict__ ntot,
                                                                  mxm_em_state *__restrict__ state) {
    __shared__ unsigned long long s_scan[BOOT_THREADS];
    __shared__ int s_bad;
    const int t = threadIdx.x, s = blockIdx.x;
    const int64_t lo = row0[s], n = row0[s + 1] - lo;
    if (t == 0) s_bad = 0;
    __syncthreads();
    unsigned long long carry = 0;                           // uniform
    for (int64_t q = 0; q < n; q += BOOT_THREADS) {         // uniform
        const int64_t i = q + t;
        unsigned long long v = 0;
        if (i < n) {
            const double x = w[lo + i];
            if (!(x >= 0.0) || x != floor(x) || !(x < INFINITY)) s_bad = 1;      // (NaN fails x >= 0)
            else v = (x < 2147483648.0) ? (unsigned long long)x : 2147483648ull;
        }
        s_scan[t] = v;
        __syncthreads();
        for (int d = 1; d < BOOT_THREADS; d <<= 1) {        // Hillis-Steele: integers, so the order does not matter
            const unsigned long long add = (t >= d) ? s_scan[t - d] : 0;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        const unsigned long long here = carry + s_scan[t];  // < 2^31 x rows: far from 2^64
        if (i < n) cum[lo + i] = (here < 0xffffffffull) ? (uint32_t)here : 0xffffffffu;
        carry += s_scan[BOOT_THREADS - 1];
        __syncthreads();                                    // s_scan is free for the next chunk
    }
    if (t == 0) {
        const int code = s_bad ? 1 : ((carry == 0 || carry >= 2147483648ull) ? 2 : 0);
        ntot[s] = (code == 0) ? (int64_t)carry : -(int64_t)code;
        state[s].error = (uint32_t)code;
    }
}

// Philox4x64-10 (Salmon et al., Random123): out <- the four words of counter (c0, c1, c2, 0) under key (k0, 0)
__device__ __forceinline__ void boot_philox(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t k0, uint64_t (&out)[4]) {
    uint64_t x0 = c0, x1 = c1, x2 = c2, x3 = 0, ka = k0, kb = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = 0xD2E7470EE14C6C93ull, m1 = 0xCA5A826395121157ull;
        const uint64_t hi0 = __umul64hi(m0, x0), lo0 = m0 * x0;
        const uint64_t hi1 = __umul64hi(m1, x2), lo1 = m1 * x2;
        x0 = hi1 ^ x1 ^ ka;
        x1 = lo1;
        x2 = hi0 ^ x3 ^ kb;
        x3 = lo0;
        ka += 0x9E3779B97F4A7C15ull;
        kb += 0xBB67AE8584CAA73Bull;
    }
    out[0] = x0; out[1] = x1; out[2] = x2; out[3] = x3;
}

// the number of entries of cum[0 .. n) that are <= t (cum ascends; t < cum[n - 1], so the answer is a row)
template <typename T>
__device__ __forceinline__ int boot_rows_le(const T *cum, int n, uint32_t t) {
    int lo = 0, hi = n;                                      // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n) ? lo : n - 1;                            // (never taken for t < cum[n - 1]; an index past the sample never leaves here)
}

// workgroup (b, s): replicate b0 + b of sample s.  GLOBAL false: the samples of at most BOOT_LDS_ROWS rows, prefix sums and
// counters in LDS (2 x n words of dynamic LDS); GLOBAL true: the others, counters = cnt[b][row0[s] .. row0[s + 1]) of the
// workspace (ld_cnt words per replicate), which only this workgroup touches in this launch.
template <bool GLOBAL>
__global__ __launch_bounds__(BOOT_THREADS) void boot_draw_kernel(const int64_t *__restrict__ row0, const uint32_t *__restrict__ cum,
                                                                const int64_t *__restrict__ ntot, const uint32_t *__restrict__ sid,
                                                                uint64_t seed, int B, int b0, uint32_t *__restrict__ cnt,
                                                                int64_t ld_cnt, double *__restrict__ wb) {
    extern __shared__ uint32_t boot_lds[];
    const int t = threadIdx.x, s = blockIdx.y, b = b0 + (int)blockIdx.x;
    const int64_t lo = row0[s], n64 = row0[s + 1] - lo;
    if ((n64 > BOOT_LDS_ROWS) != GLOBAL) return;             // the other instance's sample
    const int n = (int)n64;
    double *out = wb + (int64_t)B * lo + (int64_t)b * n;
    const int64_t N = ntot[s];
    if (N <= 0) {                                            // refused (state[s].error says why)
        for (int i = t; i < n; i += BOOT_THREADS) out[i] = __builtin_nan("");
        return;
    }
    const uint32_t *gcum = cum + lo;
    uint32_t *s_cum = boot_lds, *s_cnt = boot_lds + n;       // (GLOBAL: not used)
    uint32_t *g_cnt = cnt + (int64_t)blockIdx.x * ld_cnt + lo;
    for (int i = t; i < n; i += BOOT_THREADS) {
        if (GLOBAL) {
            __hip_atomic_store(g_cnt + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            s_cum[i] = gcum[i];
            s_cnt[i] = 0;
        }
    }
    __syncthreads();
    const uint64_t blocks = ((uint64_t)N + 3) >> 2;
    for (uint64_t q = t; q < blocks; q += BOOT_THREADS) {
        uint64_t u[4];
        boot_philox(q + 1, (uint64_t)b, (uint64_t)sid[s], seed, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (q * 4 + j < (uint64_t)N) {
                const uint32_t at = (uint32_t)__umul64hi(u[j], (uint64_t)N);     // < N < 2^31
                if (GLOBAL) atomicAdd(g_cnt + boot_rows_le(gcum, n, at), 1u);
                else atomicAdd(s_cnt + boot_rows_le(s_cum, n, at), 1u);
            }
        }
    }
    __syncthreads();
    for (int i = t; i < n; i += BOOT_THREADS) {
        // (the global counters are read where the atomics counted them: a line of another workgroup's neighbouring slice
        // that this CU has cached may be older)
        const uint32_t k = GLOBAL ? __hip_atomic_load(g_cnt + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : s_cnt[i];
        out[i] = (double)k;
    }
}

// workgroup s * B + b: replicate b of sample s -- the one-run kernel's loop on the sample's rows under the replicate's weights
template <int LD>
__global__ __launch_bounds__(SFIN_THREADS, 2) void em_loop_samples_narrow_boot_kernel(
    const double *__restrict__ M, double *__restrict__ E, const double *__restrict__ wb, const int64_t *__restrict__ row0,
    const int32_t *__restrict__ ncol, int B, double *__restrict__ ln_cur, double *__restrict__ ln_new,
    double *__restrict__ props_cur, mxm_em_state *__restrict__ state, double tol, int max_iter, int chunk, int lds_doubles) {
    const int entry = blockIdx.x, s = entry / B, b = entry - s * B;
    mxm_em_state *st = state + entry;
    if (st->done != 0) return;                             // written before the launch: a finished replicate stays as it is
    const int K = ncol[s];
    if (K < 1 || K > LD) return;
    const int64_t lo = row0[s], n = row0[s + 1] - lo;
    sfin_em_loop_body<LD, true>(M + lo * LD, E + lo * LD, wb + (int64_t)B * lo + (int64_t)b * n, n, K, ln_cur + (int64_t)entry * LD,
                                ln_new + (int64_t)entry * LD, props_cur + (int64_t)entry * LD, st, tol, max_iter, chunk,
                                lds_doubles);
}

// x_(i) + g (x_(i+1) - x_(i)) at h = q (B - 1), every operation rounded on its own (no contraction: the tests restate it)
__device__ __forceinline__ double boot_quantile(const double *sorted, int B, double q) {
#pragma clang fp contract(off)                              // (the _rn intrinsics are plain operators here: they would fuse)
    const double h = q * (double)(B - 1);
    const double fl = floor(h);
    const int i = (int)fl;
    const int i1 = (i + 1 < B) ? i + 1 : B - 1;
    const double g = h - fl;
    const double step = g * (sorted[i1] - sorted[i]);
    return sorted[i] + step;
}

// the sum of v over the workgroup in one fixed order (the threads pairwise, the upper half onto the lower); all threads get it
__device__ __forceinline__ double boot_block_sum(double v, double *s_red) {
    const int t = threadIdx.x;
    s_red[t] = v;
    __syncthreads();
    for (int half = BOOT_THREADS / 2; half > 0; half >>= 1) {
        if (t < half) s_red[t] += s_red[t + half];
        __syncthreads();
    }
    const double total = s_red[0];
    __syncthreads();                                        // s_red is free again
    return total;
}

__global__ __launch_bounds__(BOOT_THREADS) void boot_summary_kernel(int B, int ld, const int32_t *__restrict__ ncol,
                                                                   const double *__restrict__ ln_new,
                                                                   const mxm_em_state *__restrict__ state, double q_lo, double q_hi,
                                                                   double *__restrict__ x, double *__restrict__ lo,
                                                                   double *__restrict__ hi, double *__restrict__ mean,
                                                                   double *__restrict__ sd) {
    __shared__ double s_x[BOOT_MAX];
    __shared__ double s_red[BOOT_THREADS];
    __shared__ int s_bad;
    const int t = threadIdx.x, k = blockIdx.x, s = blockIdx.y;
    if (k >= ncol[s]) return;                               // uniform
    int P = 2;
    while (P < B) P <<= 1;                                  // B <= BOOT_MAX, a power of two
    if (t == 0) s_bad = 0;
    __syncthreads();
    for (int i = t; i < P; i += BOOT_THREADS) {
        double v = INFINITY;
        if (i < B) {
            const int64_t e = (int64_t)s * B + i;
            v = exp(ln_new[e * ld + k]);
            x[e * ld + k] = v;
            if (!isfinite(v) || state[e].done == 0 || state[e].error != 0) s_bad = 1;
        }
        s_x[i] = v;
    }
    __syncthreads();
    for (int len = 2; len <= P; len <<= 1) {                // the bitonic network, ascending
        for (int j = len >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += BOOT_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const double a = s_x[i], c = s_x[p];
                    const bool up = (i & len) == 0;
                    if (up ? (a > c) : (a < c)) { s_x[i] = c; s_x[p] = a; }
                }
            }
            __syncthreads();
        }
    }
    double part = 0.0;
    for (int i = t; i < B; i += BOOT_THREADS) part += s_x[i];
    const double m = boot_block_sum(part, s_red) / (double)B;
    part = 0.0;
    for (int i = t; i < B; i += BOOT_THREADS) part = fma(s_x[i] - m, s_x[i] - m, part);
    const double var = boot_block_sum(part, s_red) / (double)(B - 1);
    if (t == 0) {
        const int64_t o = (int64_t)s * ld + k;
        const double nan = __builtin_nan("");
        const bool bad = s_bad != 0;
        lo[o] = bad ? nan : boot_quantile(s_x, B, q_lo);
        hi[o] = bad ? nan : boot_quantile(s_x, B, q_hi);
        mean[o] = bad ? nan : m;
        sd[o] = bad ? nan : sqrt(var);
    }
}

// flag[s] holds ncol[s] on entry (the entry's upload); on exit 1 when a column of the sample came out NaN, else 0
__global__ __launch_bounds__(BOOT_THREADS) void boot_flag_kernel(int S, int ld, const double *__restrict__ lo, int32_t *__restrict__ flag) {
    const int s = blockIdx.x * BOOT_THREADS + threadIdx.x;
    if (s >= S) return;
    const int K = flag[s];
    int bad = 0;
    for (int k = 0; k < K; ++k) {
        const double v = lo[(int64_t)s * ld + k];
        bad |= (v != v) ? 1 : 0;
    }
    flag[s] = bad;
}

#endif  // MIXEMT_BOOTSTRAP_KERNELS_HPP
