/*
 * mixemt_hip_stats_samples.h -- part of the C ABI of libmixemt_hip.so; included by mixemt_hip.h, not meant to be included on
 * its own.
 * Three additions behind MXM_VERSION 603: the version stays, for the reason mixemt_hip.h gives for the samples entries.  The
 * entries have a header and a binding table (_lib.STATS_SAMPLES_SIGNATURES) of their own for the reason
 * mixemt_hip_assemble_samples.h gives: the older headers' names, guard-banded buffers and stream cases are pinned by tables
 * of the test suite that name those headers.  The refusals, the guard-banded calls and the stream cases of these entries are
 * pinned beside their own tests (tests/test_stats_samples_host.py, tests/test_gpu_guarded_stats_samples.py,
 * tests/test_gpu_stream_contract_stats_samples.py).
 *
 * mixemt's `-t` tables as text, formatted on the device.  A text BLOCK is n_pos lines over one pileup table
 * [>= n_pos][16] uint32 in the bins of observe.BINS (row stride 16 words), in one of two line formats:
 *   kind 0, obs.tab (io.write_base_obs)      <prefix>pos\tA\tC\tG\tT\ttotal\n
 *       pos is 0-based; A..T are bin[0..3] + bin[7..10]; total is the 64-bit sum of bins 0..13 (up to 11 digits);
 *       <prefix> is the block's byte string, written verbatim, possibly empty
 *   kind 1, pos.tab (stats.write_variants)   pos+1\tA\tC\tG\tT\t{polymorphic|fixed}\t{variant|sample_fixed}\t<tail>\n
 *       polymorphic: the block's flag of the position is not 0; variant: more than one of A, C, G, T satisfies
 *       (double)count >= thr[block]; <tail>: the line's bytes of the block's CSR, possibly empty, of any length
 * Bins 14 and 15 enter no sum; rows at or past n_pos are never read; a NULL table is a table of zeros.  The blocks follow
 * one another in the text, so consecutive blocks of one file are one slice of it.
 * A TILE is MXM_STATS_TILE_LINES consecutive lines of one block (the last tile of a block may be shorter): block b owns the
 * tiles b * ceil(n_pos / MXM_STATS_TILE_LINES) and on.
 */
#ifndef MIXEMT_HIP_STATS_SAMPLES_H
#define MIXEMT_HIP_STATS_SAMPLES_H

#ifdef __cplusplus
extern "C" {
#endif

/* lines of a tile: a workgroup of as many threads takes it, a thread per line (csrc/stats_text_kernels.hpp says why 256) */
#define MXM_STATS_TILE_LINES 256
/* bytes a block's prefix may have: the workgroup stages the fixed parts of its lines in LDS */
#define MXM_STATS_MAX_PREFIX 64

/* A HOST struct; which of its arrays live on the host and which on the device is stated per field. */
typedef struct mxm_stats_text {
    int32_t kind;                         /* 0: obs.tab lines, 1: pos.tab lines */
    int32_t n_blocks;
    int64_t n_pos;                        /* lines per block, at most 2^31 - 2 */
    const uint32_t *const *table_host;    /* HOST [n_blocks]: DEVICE pointers, 16-byte aligned, to [>= n_pos][16] uint32; NULL:
                                             a table of zeros */
    const uint8_t *prefix_host;           /* HOST, kind 0: the prefixes' bytes */
    const int64_t *prefix_ptr_host;       /* HOST, kind 0: [n_blocks + 1]; block b's prefix is prefix_host[ptr[b] .. ptr[b + 1]) */
    const uint8_t *poly;                  /* DEVICE, kind 1: [n_blocks][n_pos] uint8 flags */
    const double *thr;                    /* DEVICE, kind 1: [n_blocks] */
    const uint8_t *tail;                  /* DEVICE, kind 1: the tails' bytes; may be NULL when every tail is empty */
    const int64_t *tail_ptr;              /* DEVICE, kind 1: [n_blocks * n_pos + 1]; line (b, pos) has the bytes
                                             tail[ptr[b * n_pos + pos] .. ptr[b * n_pos + pos + 1]) */
} mxm_stats_text;

/*
 * mxm_stats_text_tiles -- the number of tiles of n_blocks blocks of n_pos lines: n_blocks * ceil(n_pos /
 * MXM_STATS_TILE_LINES); -1 when a size is negative or the tiles are more than the entries below take.  A HOST getter.
 */
int64_t mxm_stats_text_tiles(int32_t n_blocks, int64_t n_pos);

/*
 * mxm_stats_text_sizes -- where every tile's bytes begin.
 *   t                   the text (HOST struct)
 *   tile_off [n_tiles + 1]   DEVICE int64, written: the exclusive scan of the tiles' byte counts; tile_off[n_tiles] is the
 *                       text's size.  (The counts are written first, then ONE workgroup scans them in place.)
 * The host tables (table_host, prefix_host, prefix_ptr_host) are validated on the host, uploaded by the call into
 * stream-ordered memory of its own (hipMallocAsync / hipFreeAsync on `stream`: not meant to be captured) through a pageable
 * copy of the call's own, and read before the call returns.  The call only enqueues on `stream`; nothing is waited for.
 * Refused with -1 WITHOUT touching the device: t NULL; n_blocks < 0 or n_pos < 0; a kind other than 0 and 1; n_pos above
 * 2^31 - 2 or more than 2^31 - 1 tiles (the tile index is an int32); tile_off NULL; with n_blocks > 0 and n_pos > 0:
 * table_host NULL, a table that is not 16-byte aligned; kind 0: prefix_ptr_host NULL, prefix_ptr_host[0] < 0, a
 * prefix_ptr_host that decreases, a prefix of more than MXM_STATS_MAX_PREFIX bytes, prefix_host NULL with prefix bytes;
 * kind 1: poly, thr or tail_ptr NULL.
 * n_blocks == 0 or n_pos == 0: 0, nothing launched; tile_off[0] = 0 is still written (a memset on `stream`).
 */
int mxm_stats_text_sizes(const mxm_stats_text *t, int64_t *tile_off, void *stream);

/*
 * mxm_stats_text_write -- the text's bytes.
 *   t, tile_off         as above: tile_off as mxm_stats_text_sizes wrote it for the same t
 *   out [out_bytes]     DEVICE uint8: tile k's lines are written at out + tile_off[k], byte by byte (no alignment of out or
 *                       of a tile is assumed); with out_bytes = tile_off[n_tiles] every byte of out is written
 *   err                 DEVICE uint32, OR-ed into: bit 0 -- a tile whose bytes (recomputed by the kernel, placed at
 *                       tile_off[k]) do not lie inside [0, out_bytes) was skipped WHOLE.  Nothing is ever stored at or past
 *                       out + out_bytes, or before out.
 * Plain stores to disjoint ranges (the only atomic is the one into err): the same bytes for any launch order.
 * The host tables are validated, uploaded and read as by mxm_stats_text_sizes.  The call only enqueues on `stream`; nothing is
 * waited for; not meant to be captured.
 * Refused with -1 WITHOUT touching the device: every refusal of mxm_stats_text_sizes; out_bytes < 0; out NULL with
 * out_bytes > 0; err NULL.
 * n_blocks == 0 or n_pos == 0: 0, nothing launched.
 */
int mxm_stats_text_write(const mxm_stats_text *t, const int64_t *tile_off, uint8_t *out, int64_t out_bytes, uint32_t *err,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MIXEMT_HIP_STATS_SAMPLES_H */
