// stats_text_kernels.hpp -- part of libmixemt_hip.so (gfx950); included by mixemt_hip.hip only.
//
// mixemt's `-t` tables as text, formatted on the device (include/mixemt_hip_stats_samples.h): a text block is n_pos lines
// over one [>= n_pos][16] uint32 pileup table (the bins of observe.BINS), in one of two line formats
//   kind 0  obs.tab   <prefix>pos\tA\tC\tG\tT\ttotal\n                                            (io.write_base_obs)
//   kind 1  pos.tab   pos+1\tA\tC\tG\tT\t{polymorphic|fixed}\t{variant|sample_fixed}\t<tail>\n      (stats.write_variants)
// A..T are bin[b] + bin[7 + b] (up to 2 * (2^32 - 1): 64-bit), total the 64-bit sum of bins 0..13 (up to 11 digits); bins
// 14 and 15 enter no sum, rows at or past n_pos are never read, a NULL table is a table of zeros.
//   stats_text_sizes_kernel   bytes per tile
//   stats_text_scan_kernel    ONE workgroup: the sizes -> their exclusive scan in place, the total behind them
//   stats_text_write_kernel   the tile's bytes at out + tile_off[t]
//
// A tile is STATS_TILE = 256 consecutive lines of one block and a workgroup of 256 threads takes it, a thread per line:
// one line is one 64-byte row, so a wave reads 4 KiB of rows and the workgroup's LDS stage for the fixed parts of its lines
// stays at 256 * (64 + 67) = 33 536 bytes, which leaves four workgroups per CU their LDS; a 16 569-line block is 65 tiles,
// so the 768 blocks of 256 samples give 5 * 10^4 workgroups, far more than the device holds at once, while the scan kernel's
// one workgroup still passes over the tile sizes in well under the time of the write.  Smaller tiles only lengthen the scan.
//
// Write kernel, per tile: every thread loads its row and recomputes its line's length; two exclusive scans over the
// workgroup (wave scan by __shfl_up, the waves' totals through LDS) give the offset of each line's fixed part in the LDS
// stage and of the line in the output; every thread formats its fixed part into LDS (digits by integer division, no
// floating point, no printf); then the workgroup streams the stage to the output with its lanes on consecutive BYTES (byte
// stores: out + tile_off[t] has no alignment), finding each byte's line by bisection over the LDS offsets -- the final
// '\n' of a kind-1 line moves behind the line's tail; last, every wave copies the tails of its own 64 lines from global
// memory to global memory, its lanes on consecutive bytes.  A tile that does not lie inside [0, out_bytes) is skipped
// whole and bit 0 of the error word is set (the only atomic).  Plain stores to disjoint ranges: the same bytes for any
// launch order.  The only floating-point operation is kind 1's `(double)count >= thr`, which IS the reference's comparison.
#ifndef MIXEMT_STATS_TEXT_KERNELS_HPP
#define MIXEMT_STATS_TEXT_KERNELS_HPP

#ifndef STATS_HD
#define STATS_HD __host__ __device__
#endif

constexpr int STATS_TILE = 256;               // lines of a tile = threads of its workgroup (MXM_STATS_TILE_LINES)
constexpr int STATS_MAX_PREFIX = 64;          // MXM_STATS_MAX_PREFIX
// the longest fixed part without its prefix: kind 0 -- pos (10 digits: n_pos < 2^31) + 4 x (10 digits) + total (11 digits)
// + 6 separators = 67; kind 1 -- 10 + 4 x 10 + 5 tabs + "polymorphic\t" (12) + "sample_fixed\t" (13) + '\n' = 81 <= 64 + 67
constexpr int STATS_FIXED_MAX = 67;
constexpr int STATS_STAGE_BYTES = STATS_TILE * (STATS_MAX_PREFIX + STATS_FIXED_MAX);
constexpr int STATS_SCAN_THREADS = 1024;

// What the kernels read of an mxm_stats_text: the host tables are device arrays the host side uploads.
struct stats_text_view {
    int32_t kind, n_blocks;
    int64_t n_pos;
    int32_t tiles_per_block;
    const uint32_t *const *table;             // [n_blocks] device pointers, nullable
    const uint8_t *prefix;                    // kind 0
    const int64_t *prefix_ptr;                // kind 0: [n_blocks + 1]
    const uint8_t *poly;                      // kind 1: [n_blocks][n_pos]
    const double *thr;                        // kind 1: [n_blocks]
    const uint8_t *tail;                      // kind 1
    const int64_t *tail_ptr;                  // kind 1: [n_blocks * n_pos + 1]
};

// decimal digits of v (v < 10^11 here; right for any v)
STATS_HD static inline int stats_digits(uint64_t v) {
    if (v < 4294967296ull) {
        const uint32_t x = (uint32_t)v;
        return x < 10u ? 1 : x < 100u ? 2 : x < 1000u ? 3 : x < 10000u ? 4 : x < 100000u ? 5 : x < 1000000u ? 6
             : x < 10000000u ? 7 : x < 100000000u ? 8 : x < 1000000000u ? 9 : 10;
    }
    int n = 10;
    uint64_t t = 10000000000ull;
    while (n < 20 && v >= t) {                // (10^20 does not fit: 20 digits is the most a uint64 has)
        ++n;
        if (n < 20) t *= 10;
    }
    return n;
}

// the nd = stats_digits(v) digits of v at p[0 .. nd), most significant first
STATS_HD static inline void stats_put(uint8_t *p, uint64_t v, int nd) {
    int i = nd;
    while (v >= 4294967296ull) {              // nine digits at a time come off in 32-bit arithmetic
        uint32_t low = (uint32_t)(v % 1000000000ull);
        v /= 1000000000ull;
        for (int k = 0; k < 9; ++k) {
            const uint32_t q = low / 10u;
            p[--i] = (uint8_t)('0' + (low - q * 10u));
            low = q;
        }
    }
    uint32_t x = (uint32_t)v;
    while (i > 0) {
        const uint32_t q = x / 10u;
        p[--i] = (uint8_t)('0' + (x - q * 10u));
        x = q;
    }
}

STATS_HD static inline int stats_put_str(uint8_t *p, const char *s, int n) {
    for (int k = 0; k < n; ++k) p[k] = (uint8_t)s[k];
    return n;
}

// One line: its five numbers (A C G T and, kind 0, the total), the number in its first field, its flags and its lengths.
struct stats_line {
    uint64_t v[5];
    uint64_t first;                           // pos (kind 0) or pos + 1 (kind 1)
    int fixed;                                // bytes of the fixed part (kind 1: the final '\n' included)
    int prefix_len;
    int64_t tail_lo, tail_len;
    bool poly, variant;
};

// A..T and the total of a row of 16 words (w[14], w[15] enter nothing)
STATS_HD static inline void stats_sums(const uint32_t *w, uint64_t v[5]) {
    uint64_t total = 0;
    for (int b = 0; b < 14; ++b) total += w[b];
    for (int b = 0; b < 4; ++b) v[b] = (uint64_t)w[b] + (uint64_t)w[7 + b];
    v[4] = total;
}

STATS_HD static inline int stats_fixed_len(int kind, const stats_line &ln) {
    int n = stats_digits(ln.first) + 1;
    for (int b = 0; b < 4; ++b) n += stats_digits(ln.v[b]) + 1;
    if (kind == 0) return ln.prefix_len + n + stats_digits(ln.v[4]) + 1;
    return n + (ln.poly ? 12 : 6) + (ln.variant ? 8 : 13) + 1;
}

// the fixed part of a line at p (the prefix, kind 0, is copied by the caller: p starts behind it); returns its length
STATS_HD static inline int stats_format(int kind, const stats_line &ln, uint8_t *p) {
    int at = 0;
    int nd = stats_digits(ln.first);
    stats_put(p, ln.first, nd);
    at = nd;
    p[at++] = '\t';
    for (int b = 0; b < 4; ++b) {
        nd = stats_digits(ln.v[b]);
        stats_put(p + at, ln.v[b], nd);
        at += nd;
        p[at++] = '\t';
    }
    if (kind == 0) {
        nd = stats_digits(ln.v[4]);
        stats_put(p + at, ln.v[4], nd);
        at += nd;
        p[at++] = '\n';
        return at;
    }
    at += ln.poly ? stats_put_str(p + at, "polymorphic\t", 12) : stats_put_str(p + at, "fixed\t", 6);
    at += ln.variant ? stats_put_str(p + at, "variant\t", 8) : stats_put_str(p + at, "sample_fixed\t", 13);
    p[at++] = '\n';
    return at;
}

#ifdef __HIPCC__
// The line `pos` of block `blk`, loaded and measured (no text yet).
__device__ static inline void stats_load_line(const stats_text_view &t, int32_t blk, int64_t pos, stats_line &ln) {
    uint32_t w[16];
    const uint32_t *table = t.table[blk];
    if (table != nullptr) {
        const uint4 *row = reinterpret_cast<const uint4 *>(table + pos * 16);      // (tables are 16-byte aligned)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 x = row[q];
            w[4 * q] = x.x, w[4 * q + 1] = x.y, w[4 * q + 2] = x.z, w[4 * q + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = 0;
    }
    stats_sums(w, ln.v);
    ln.poly = ln.variant = false;
    ln.tail_lo = ln.tail_len = 0;
    ln.prefix_len = 0;
    if (t.kind == 0) {
        ln.first = (uint64_t)pos;
        ln.prefix_len = (int)(t.prefix_ptr[blk + 1] - t.prefix_ptr[blk]);
    } else {
        ln.first = (uint64_t)pos + 1;
        const int64_t at = (int64_t)blk * t.n_pos + pos;
        ln.poly = t.poly[at] != 0;
        const double thr = t.thr[blk];
        int reach = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) reach += (double)ln.v[b] >= thr ? 1 : 0;
        ln.variant = reach > 1;
        ln.tail_lo = t.tail_ptr[at];
        ln.tail_len = t.tail_ptr[at + 1] - ln.tail_lo;
        if (ln.tail_len < 0) ln.tail_len = 0;                // (a CSR that decreases: no tail, never a negative length)
    }
    ln.fixed = stats_fixed_len(t.kind, ln);
}

// Exclusive scan of v over the 256 threads of the workgroup; *total: the sum.  part: LDS, one int64 per wave + 1.
__device__ static inline int64_t stats_block_scan(int64_t v, int64_t *part, int64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    __syncthreads();                                         // (part may still be read from the scan before)
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int64_t base = 0, all = 0;
#pragma unroll
    for (int w = 0; w < STATS_TILE / 64; ++w) {
        const int64_t p = part[w];
        if (w < wave) base += p;
        all += p;
    }
    *total = all;
    return base + inc - v;
}

__global__ __launch_bounds__(STATS_TILE) void stats_text_sizes_kernel(stats_text_view t, int64_t n_tiles,
                                                                      int64_t *__restrict__ tile_off) {
    __shared__ int64_t part[STATS_TILE / 64];
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int32_t blk = (int32_t)(tile / t.tiles_per_block);
        const int64_t pos = (tile - (int64_t)blk * t.tiles_per_block) * STATS_TILE + threadIdx.x;
        int64_t mine = 0;
        if (pos < t.n_pos) {
            stats_line ln;
            stats_load_line(t, blk, pos, ln);
            mine = ln.fixed + ln.tail_len;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t all = 0;
            for (int w = 0; w < STATS_TILE / 64; ++w) all += part[w];
            tile_off[tile] = all;
        }
    }
}

// ONE workgroup: off[0 .. n) sizes -> their exclusive scan, off[n] = the total.  A thread owns a contiguous chunk.
__global__ __launch_bounds__(STATS_SCAN_THREADS) void stats_text_scan_kernel(int64_t *off, int64_t n) {
    __shared__ int64_t part[STATS_SCAN_THREADS / 64];
    const int64_t chunk = (n + STATS_SCAN_THREADS - 1) / STATS_SCAN_THREADS;
    const int64_t lo = chunk * threadIdx.x < n ? chunk * threadIdx.x : n;
    const int64_t hi = lo + chunk < n ? lo + chunk : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += off[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int64_t base = 0, all = 0;
    for (int w = 0; w < STATS_SCAN_THREADS / 64; ++w) {
        const int64_t p = part[w];
        if (w < wave) base += p;
        all += p;
    }
    int64_t run = base + inc - sum;
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t size = off[i];
        off[i] = run;
        run += size;
    }
    if (threadIdx.x == 0) off[n] = all;
}

__global__ __launch_bounds__(STATS_TILE) void stats_text_write_kernel(stats_text_view t, int64_t n_tiles,
                                                                      const int64_t *__restrict__ tile_off,
                                                                      uint8_t *__restrict__ out, int64_t out_bytes,
                                                                      uint32_t *err) {
    __shared__ uint8_t stage[STATS_STAGE_BYTES];
    __shared__ int32_t fix_at[STATS_TILE + 1];               // the lines' fixed parts in the stage (exclusive scan)
    __shared__ int64_t line_at[STATS_TILE + 1];              // the lines in the tile's output (exclusive scan)
    __shared__ int64_t part[STATS_TILE / 64];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int32_t blk = (int32_t)(tile / t.tiles_per_block);
        const int64_t pos0 = (tile - (int64_t)blk * t.tiles_per_block) * STATS_TILE;
        const int64_t pos = pos0 + tid;
        const bool have = pos < t.n_pos;
        stats_line ln;
        ln.fixed = ln.prefix_len = 0;
        ln.tail_lo = ln.tail_len = 0;
        if (have) stats_load_line(t, blk, pos, ln);
        int64_t fixed_all, bytes_all;
        const int64_t my_fix = stats_block_scan(ln.fixed, part, &fixed_all);
        const int64_t my_line = stats_block_scan(ln.fixed + ln.tail_len, part, &bytes_all);
        const int64_t base = tile_off[tile];
        // (uniform over the workgroup: every thread holds the same base and totals)
        if (base < 0 || base > out_bytes || bytes_all > out_bytes - base) {
            if (tid == 0) atomicOr(err, 1u);
            continue;
        }
        fix_at[tid] = (int32_t)my_fix;
        line_at[tid] = my_line;
        if (tid == 0) {
            fix_at[STATS_TILE] = (int32_t)fixed_all;
            line_at[STATS_TILE] = bytes_all;
        }
        if (have) {
            uint8_t *p = stage + my_fix;
            if (t.kind == 0) {
                const uint8_t *src = t.prefix + t.prefix_ptr[blk];
                for (int k = 0; k < ln.prefix_len; ++k) p[k] = src[k];
                p += ln.prefix_len;
            }
            stats_format(t.kind, ln, p);
        }
        __syncthreads();
        // the stage -> the output, lanes on consecutive bytes
        uint8_t *dst = out + base;
        for (int32_t j = tid; j < (int32_t)fixed_all; j += STATS_TILE) {
            int lo = 0, hi = STATS_TILE;                     // the last line i with fix_at[i] <= j (empty lines: fix_at equal)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (fix_at[mid] <= j) lo = mid; else hi = mid;
            }
            const int32_t in_line = j - fix_at[lo];
            const int32_t fixed = fix_at[lo + 1] - fix_at[lo];
            int64_t at = line_at[lo] + in_line;
            if (in_line == fixed - 1) at = line_at[lo + 1] - 1;          // the '\n': behind the tail
            dst[at] = stage[j];
        }
        // the tails of this wave's 64 lines, global -> global
        if (t.kind == 1) {
            unsigned long long todo = __ballot(ln.tail_len > 0);
            const int64_t my_dst = my_line + ln.fixed - 1;   // the tail starts where the '\n' would stand without it
            while (todo) {
                const int src_lane = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int64_t lo = __shfl(ln.tail_lo, src_lane, 64), len = __shfl(ln.tail_len, src_lane, 64);
                const int64_t to = __shfl(my_dst, src_lane, 64);
                for (int64_t k = lane; k < len; k += 64) dst[to + k] = t.tail[lo + k];
            }
        }
        __syncthreads();                                     // (the stage and the offsets are reused by the next tile)
    }
}
#endif  // __HIPCC__

#endif  // MIXEMT_STATS_TEXT_KERNELS_HPP
