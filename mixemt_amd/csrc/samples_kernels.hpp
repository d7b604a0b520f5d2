// samples_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only.
// The EM iteration of MANY samples in one launch: every sample has its own rows, weights, proportions and loop state
// (em.py:94-165 once per sample; a cohort is a Python loop over samples in the reference).
#ifndef MIXEMT_SAMPLES_KERNELS_HPP
#define MIXEMT_SAMPLES_KERNELS_HPP

// ------------------------------------------------------------------------------------------
// A de-duplicated sample is a small matrix (600 .. 10^5 rows x 5408): alone it leaves most of the chip idle -- the
// per-iteration kernels deal 600 rows over 512 workgroups and pay three launches for 12 us of work, and the one-launch
// loop wants the device to itself, so two samples cannot overlap.  Here the rows of all samples sit back to back in ONE
// records matrix (sample s owns the rows [row0[s], row0[s + 1])) and the host cuts every sample into TILES of at most
// MXM_SAMPLES_TILE_ROWS consecutive rows of that sample -- a function of the sample's own row count and nothing else.
//   em_iter_samples_kernel    workgroup t = tile t: the tile's rows under ITS sample's proportions -> partial[t][H]
//   samples_colreduce_kernel  colsum[s][h] = sum of partial[t][h] over the tiles of s, in ascending tile order
//   finalize_kernel           unchanged, B = S (a sample is a restart that owns its rows)
// A sample's sums depend on its own rows, weights and proportions alone: the same bits whichever other samples share
// the batch and wherever the sample stands in it.  Plain launches on one stream; no persistent grid, no grid barrier (a
// sample's tiles may outnumber what is co-resident), no float atomics.  Tiles of a finished sample return at once, so a
// sample freezes on the iteration it stops on while the others run on.
//
// The byte-coded rows go through coded_row_pass itself (coded_kernels.hpp), as a "grid" of ONE workgroup over the
// tile's rows: the record arrays are handed in from the tile's first row on, so the pass sees rows 0 .. count - 1.
// Its own loop over WIDE rows (16-bit codes) deals mxm_coded.wide_rows over the whole grid and cannot be used: a wide
// row belongs to its sample's tile.  The tile finds its wide rows from ndist (one ballot of the first wave -- hence at
// most 64 rows per tile -- in row order) and takes them one after another in a loop of its own; mxm_coded.wide_rows is
// not read at all.  What the tile checks instead: every row has a record of 1 .. 1024 values (a row without one would
// need the dense rest, which this path does not have) -- a fault poisons the SAMPLE's sums with NaN and raises its
// state's error; the faulty row is never dereferenced.
// ------------------------------------------------------------------------------------------
#define SAMPLES_THREADS 256
static_assert(MXM_SAMPLES_TILE_ROWS >= 1 && MXM_SAMPLES_TILE_ROWS <= 64, "a tile's wide rows are listed by one wave's ballot");

template <int NCH, int NBUF>
__global__ __launch_bounds__(SAMPLES_THREADS, 2) void em_iter_samples_kernel(
    const uint8_t *__restrict__ rec, const int64_t *__restrict__ rec_off, const int32_t *__restrict__ ndist, int ldc,
    const double *__restrict__ w, const double *__restrict__ props, int H, const mxm_sample_tile *__restrict__ tiles,
    double *__restrict__ partial, int64_t ldpart, int *__restrict__ chk, const mxm_em_state *__restrict__ state) {
    constexpr int THREADS = SAMPLES_THREADS, NW = THREADS / 64;
    const int sample = tiles[blockIdx.x].sample, count = tiles[blockIdx.x].count;
    const int64_t first = tiles[blockIdx.x].first;
    if (state[sample].done != 0) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    props += (int64_t)sample * H;
    rec_off += first;
    ndist += first;
    if (w != nullptr) w += first;

    double p[NCH][4], acc[NCH][4];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * (t + k * THREADS) + e;
            p[k][e] = (c < H) ? props[c] : 0.0;
            acc[k][e] = 0.0;
        }
    }

    // the tile's wide rows in row order, and whether every row has a record
    __shared__ int s_wl[64];
    __shared__ int s_nw, s_bad;
    if (t < 64) {
        const int nd = (t < count) ? ndist[t] : 1;
        const bool bad = nd <= 0 || nd > ENC_MAX_WIDE;
        const bool wide = !bad && nd > ENC_MAX_CODES;
        const unsigned long long mw = __ballot(wide), mb = __ballot(bad);
        if (wide) s_wl[__popcll(mw & ((1ull << t) - 1ull))] = t;
        if (t == 0) {
            s_nw = __popcll(mw);
            s_bad = (mb != 0ull) ? 1 : 0;
        }
    }
    __syncthreads();
    const bool bad = s_bad != 0;                          // uniform
    const int nw = s_nw;

    if (!bad) {
        bool meta_ready = false;
        // rows 0 .. count - 1 of the shifted arrays, workgroup 0 of a grid of 1; wide rows get weight 0 and an empty table
        // there (n_wide = 0: its own wide loop does nothing).  Default cache policy: the batch's records are read again
        // by the next iteration.
        coded_row_pass<THREADS, NCH, NBUF, false, false, false, false>(rec, rec_off, ndist, ldc, w, nullptr, 0, (int64_t)count, p,
                                                                      acc, meta_ready, nullptr, nullptr, 0, nullptr, 0, 1);
        if (nw > 0) {                                     // uniform
            __shared__ double s_wtbl[ENC_MAX_WIDE];
            __shared__ double s_wred[NW];
            const int nword = ldc >> 2;
            for (int i = 0; i < nw; ++i) {
                const int r = s_wl[i];
                const int nd = ndist[r];                  // 257 .. 1024 (checked above)
                const uint8_t *base = rec + rec_off[r];
                const double wr = (w != nullptr) ? w[r] : 1.0;
                const unsigned int *codes = reinterpret_cast<const unsigned int *>(base);     // two 16-bit codes per word
                const double *tbl = reinterpret_cast<const double *>(base + 2 * (int64_t)ldc);
                unsigned int cw[NCH][2];
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    const int word = t + k * THREADS;     // four columns; past the row: code 0 (their p is 0)
                    cw[k][0] = (word < nword) ? codes[2 * word] : 0u;
                    cw[k][1] = (word < nword) ? codes[2 * word + 1] : 0u;
                }
                __syncthreads();                          // the table and the wave sums of the row before have been read
                for (int j = t; j < nd; j += THREADS) s_wtbl[j] = tbl[j];
                __syncthreads();
                double v[NCH][4];
                auto entry = [&](unsigned int code) -> double { return s_wtbl[code < (unsigned int)ENC_MAX_WIDE ? code : 0u]; };
                double s4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int k = 0; k < NCH; ++k) {
                    v[k][0] = entry(cw[k][0] & 0xffffu);
                    v[k][1] = entry(cw[k][0] >> 16);
                    v[k][2] = entry(cw[k][1] & 0xffffu);
                    v[k][3] = entry(cw[k][1] >> 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) s4[e] = fma(v[k][e], p[k][e], s4[e]);
                }
                double s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
                s = wave_sum_lane63(s);
                if (lane == 63) s_wred[wv] = s;
                __syncthreads();
                static_assert(NW == 4, "four wave sums");
                const double cf = readlane_f64(weight_over_norm(wr, (s_wred[0] + s_wred[1]) + (s_wred[2] + s_wred[3])), 0);
#pragma unroll
                for (int k = 0; k < NCH; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[k][e] = fma(cf, v[k][e], acc[k][e]);
            }
        }
    }

    if (t == 0) chk[blockIdx.x] = bad ? 1 : 0;
    double *dst = partial + (int64_t)blockIdx.x * ldpart;
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int c = 4 * (t + k * THREADS);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < H) dst[c + e] = bad ? __builtin_nan("") : acc[k][e];
    }
}

// colsum[s][h] = partial[tile0[s]][h] + partial[tile0[s] + 1][h] + ... in that order: ONE chain per column, so a sample's
// sums are a function of its own tiles alone (eight loads in flight per step; the additions stay in tile order).
// Finished samples are left untouched.  A faulty tile (chk): the sample's sums are NaN and its state's error is raised.
#define SAMPLES_COLRED_THREADS 256
__global__ __launch_bounds__(SAMPLES_COLRED_THREADS) void samples_colreduce_kernel(
    const double *__restrict__ partial, int64_t ldpart, const int32_t *__restrict__ tile0, const int *__restrict__ chk, int H,
    double *__restrict__ colsum, mxm_em_state *state) {
    const int s = blockIdx.y;
    if (state[s].done != 0) return;
    const int t0 = tile0[s], n = tile0[s + 1] - t0;
    __shared__ int s_fault;
    if (threadIdx.x == 0) s_fault = 0;
    __syncthreads();
    int fault = 0;
    for (int i = threadIdx.x; i < n; i += SAMPLES_COLRED_THREADS) fault |= chk[t0 + i];
    if (fault) s_fault = 1;
    __syncthreads();
    const bool poisoned = s_fault != 0;
    if (poisoned && blockIdx.x == 0 && threadIdx.x == 0) state[s].error = 1;
    const int h = blockIdx.x * SAMPLES_COLRED_THREADS + threadIdx.x;
    if (h >= H) return;
    const double *src = partial + (int64_t)t0 * ldpart + h;
    double sum = 0.0;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        double a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = src[(int64_t)(i + j) * ldpart];
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += a[j];
    }
    for (; i < n; ++i) sum += src[(int64_t)i * ldpart];
    colsum[(int64_t)s * H + h] = poisoned ? __builtin_nan("") : sum;
}

#endif  // MIXEMT_SAMPLES_KERNELS_HPP
