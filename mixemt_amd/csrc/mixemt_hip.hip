// mixemt_hip.hip -- gfx950 (MI355X, CDNA4) kernels + C ABI for mixemt's EM hot path.
//
// Replaces, behind include/mixemt_hip.h:
//   preprocess.build_em_matrix   /root/reference/mixemt/preprocess.py:177-198
//   em.em_step / em.run_em loop  /root/reference/mixemt/em.py:57-91, :126-143
//   (+ consumers of the result: assemble.py:103-123, :284-334)
//
// Everything here is HBM-bound byte/fp64 streaming + reductions: 64-wide
// wavefronts, 16-byte coalesced loads, rows held in VGPRs between the row
// reduction and the column accumulation, deterministic two-stage column sums
// (no float atomics).  No MFMA: there is no contraction to feed it.
//
// One translation unit; the kernels live in headers beside this file
// (DESIGN.md section 4 has the roofline of each):
//   error.hpp           HOST code: g_err, fail (printf-checked), HIP_TRY -- also included by tests/native/bam_reader_harness.cpp
//   common.hpp          device query, reductions
//   build_kernels.hpp   build_em_matrix_kernel (byte table, L2/MALL: any alphabet, any width)
//   build_lut_kernels.hpp  build_lut_kernel (hit/miss by LDS lookup)
//   build_sparse_kernels.hpp  build_sparse_kernel (the row from the haplogroups' markers: one in-order sum per distinct cell value)
//   em_kernels.hpp      linearize, em_iter_wide_kernel (THE hot kernel: R*H*8 B read per EM iteration,
//                       1-4 restarts per pass), em_iter_wide_f32_kernel (opt-in storage variant),
//                       colreduce_kernel, finalize_kernel
//   estep_kernels.hpp   estep_log_kernel (any H), estep_wide_kernel (register-resident posterior pass)
//   records_kernels.hpp posterior_argmax_kernel (row argmax of the folded posterior from records), votes_from_best_kernel
//   aux_kernels.hpp     log_normalize, l1_exp_diff, add_scalar, row_argmax_votes, assign_reads, gather, fold, diag_stream_read
//   fused_kernels.hpp   em_fused_loop_kernel (the whole EM loop of a cache-resident matrix in one persistent launch)
//   fused_cols_kernels.hpp  em_fused_cols_kernel (the same for up to 1536 rows, columns split over the workgroups, matrix in registers)
//   coded_kernels.hpp   encode_rows_kernel, em_iter_coded_kernel (row-dictionary storage: one byte per cell + the row's distinct values)
//   fused_coded_kernels.hpp  em_fused_coded_kernel (the whole EM loop over records in one persistent launch)
//   fused_narrow_kernels.hpp  em_fused_narrow_kernel (the same for the refinement EM's few columns: the matrix in registers)
//   samples_finish_kernels.hpp  votes, column gather, refinement EM loop and read assignment of many samples per launch
//   samples_runs_kernels.hpp    their forms for samples of several EM runs (the fold of the runs' posteriors)
//   bootstrap_kernels.hpp       bootstrap replicates of the refinement loop: resampled weights, the loop, the summary
//   support_kernels.hpp         nested-model fits of the refinement loop over column masks, and their log-likelihoods
//   samples_kernels.hpp em_iter_samples_kernel, samples_colreduce_kernel (the EM iteration of many samples in one launch: a tile of
//                       one sample's rows per workgroup)
//   aln_encode.hpp      HOST code: mxm_aln_encode, the batched alignment front end (process_reads + reduce_reads + row order)
//   observe_kernels.hpp observe_bucket_kernel, observe_count_kernel (the pileup of the variant check: observe.py:56-86)
//   var_check_kernels.hpp  check_variants_samples_kernel (the variant check of a cohort's samples: assemble.py:157-208)
//   detect_kernels.hpp     the candidate rule and the variant check per (sample, replicate) entry, lists on the device
//   assemble_kernels.hpp  consensus_kernel, new_variants_kernel, first_observed_kernel, extend_walk_kernel, extend_move_kernel
//                       (consensus sequences and assembly extension over labelled pileups: assemble.py:431-585)
//   assemble_samples_kernels.hpp  new_variants_samples_kernel, extend_walk_samples_kernel, extend_move_samples_kernel (a round
//                       of the extension for the samples of a cohort over global labels)
//   stats_text_kernels.hpp  stats_text_sizes_kernel, stats_text_scan_kernel, stats_text_write_kernel (mixemt's -t tables as
//                       text: a tile of 256 lines per workgroup, digits by integer arithmetic)
// This file: the host side of the C ABI (shape checks, grid sizing, dispatch, the loop drivers).  Every refusal goes
// through fail / HIP_TRY / RC_TRY, a runtime chunk count reaches its kernel instance through dispatch_width<MAX>, the
// checks several entry points share are dynamic_lds_ok, rest_check, coded_check, samples_check, records_lists_check.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "mixemt_hip.h"
#include "mixemt_hip_tuning.h"

#include "common.hpp"
#include "aln_encode.hpp"
#include "bam_reader.hpp"
#include "coded_kernels.hpp"
#include "quad_kernels.hpp"
#include "quad_batched_kernels.hpp"
#include "build_kernels.hpp"
#include "build_lut_kernels.hpp"
#include "build_sparse_kernels.hpp"
#include "em_kernels.hpp"
#include "estep_kernels.hpp"
#include "aux_kernels.hpp"
#include "records_kernels.hpp"
#include "fused_kernels.hpp"
#include "fused_cols_kernels.hpp"
#include "fused_coded_kernels.hpp"
#include "fused_narrow_kernels.hpp"
#include "samples_kernels.hpp"
#include "samples_finish_kernels.hpp"
#include "samples_runs_kernels.hpp"
#include "bootstrap_kernels.hpp"
#include "support_kernels.hpp"
#include "exchange.hpp"
#include "aln_walk.hpp"
#include "observe_kernels.hpp"
#include "var_check_kernels.hpp"
#include "detect_kernels.hpp"
#include "assemble_kernels.hpp"
#include "assemble_samples_kernels.hpp"
#include "stats_text_kernels.hpp"


// ------------------------------------------------------------------------------------------
// Tuning / measurement state (include/mixemt_hip_tuning.h).  ONE struct, guarded by a mutex: the setters
// lock it, and every entry point of the ABI takes a private snapshot into thread-local storage when
// it starts (MXM_ENTER), so a call sees one consistent set of knobs from beginning to end whatever
// other host threads (one per GPU) set in the meantime.  Results never depend on any of it beyond the
// rounding of a different summation order.
// ------------------------------------------------------------------------------------------
struct mxm_em_state;
typedef void (*mxm_progress_fn)(const mxm_em_state *state_host, int32_t B, void *user);
struct mxm_tuning {
    int sparse_maxd = -1;           // distinct non-zero masks a row of the marker build may have (-1: the kernel's limit)
    int min_rows_per_wg = 8;        // measured: 1000 x 5408 31 us/step (vs 39 at 2); no effect from 10^4 rows up
    int compact_restarts = 2;       // mxm_em_loop: 1 packs the running restarts, 2 also keeps ONE full tile of them iterating
    int max_bt = 4;                 // restarts per matrix pass (1..MXM_MAX_BT)
    int loop_graph = -1;            // -1 auto (graph when R*H*B is small), 0 never, 1 always
    int loop_fused = -1;            // -1 auto (by size), 0 never, 1 whenever the shape allows
    int fused_chunk = 0;            // iterations per launch of the one-launch loop (0 = run to the end)
    int fused_cols = 1;             // matrices of up to 1536 rows take the transposed form (columns split)
    int fused_coded_wg = 0;         // workgroups of the one-launch loop over records (0 = by size)
    int quad_left_wg = 0;           // workgroups of the leftover pass beside the quad pass (0 = by the rows' measured cost)
    int sparse_long_entries = 5120; // ... whose rows with more marker entries than this go to the fallback list (0: no limit)
    int quad_encoder = 1;           // the quad dictionary's encoder: 1 = a wave per row (quad_encode_wave_kernel), 0 = a workgroup per row
    int sparse_long = 1;            // the marker build's second launch for rows of 65 .. 128 observations (0: they go to the fallback list)
    int coded_bt = 3;               // restarts per pass over records beside a quad dictionary (1 = one per pass, 3 = the batched kernel)
    int fused_force_abort = 0;      // test hook: the one-launch loop starts with its abort flag raised (as if starved)
    double fused_cells = 1.0e8;     // ~18 000 rows at H = 5408: measured break-even is ~30 000 rows (profiles/r02/small_runs.txt)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;     // timing hook around the dominant kernel
    mxm_progress_fn progress = nullptr;
    void *progress_user = nullptr;
    int progress_every = 10;
};
static std::mutex g_tune_mu;
static mxm_tuning g_tune;
static thread_local mxm_tuning T;   // the calling thread's snapshot for the entry point it is in
#define MXM_ENTER() do { std::lock_guard<std::mutex> lk_(g_tune_mu); T = g_tune; } while (0)
template <typename F>
static int tune_set(F f) {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    f(g_tune);
    return 0;
}
extern "C" int mxm_reset_tuning(void) {
    return tune_set([](mxm_tuning &t) { t = mxm_tuning(); });
}

// ------------------------------------------------------------------------------------------
// host side of the C ABI
// ------------------------------------------------------------------------------------------
static inline int clamp_grid(int64_t want, int cap) {
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

static inline int64_t part_ld(int H) { return ((int64_t)H + 1) & ~(int64_t)1; }

// More than 64 KiB of dynamic LDS must be opted into per kernel (and device).  Re-issued on every
// call: the attribute is idempotent and costs a table write, and nothing is cached that two host
// threads (one per GPU) could race on.  A refusal is reported with the kernel's name and the size.
static hipError_t raise_dynamic_lds(const void *kernel, size_t bytes, const char *name) {
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess)
        snprintf(g_err, sizeof(g_err), "%s: cannot opt into %zu bytes of dynamic LDS: %s", name, bytes,
                 hipGetErrorString(e));
    return e;
}
// The dynamic LDS of a launch: refused above 150 KiB where the caller has no other kernel for the width ("<who>: H=<H>
// <too_wide>", -1), opted into above 60 KiB (-2 when the runtime refuses), else 0.
static int dynamic_lds_ok(const void *kernel, size_t bytes, const char *name, const char *who = nullptr, int H = 0,
                          const char *too_wide = nullptr) {
    if (too_wide != nullptr && bytes > 150 * 1024) return fail(-1, "%s: H=%d %s", who, H, too_wide);
    if (bytes > 60 * 1024 && raise_dynamic_lds(kernel, bytes, name) != hipSuccess) return -2;
    return 0;
}

// A step that returns a status of the ABI: the first one that is not 0 ends the calling function.
#define RC_TRY(expr)                                                                         \
    do {                                                                                     \
        const int rc_ = (expr);                                                              \
        if (rc_ != 0) return rc_;                                                            \
    } while (0)

// From a runtime width to a template instance: calls f(std::integral_constant<int, n>{}) where 1 <= n <= MAX and
// returns whether it did (the caller keeps its own "outside the kernel's range" message).  Exactly the instances
// 1 .. MAX of what f launches are compiled; f narrows them further with `if constexpr` on its argument's value.
template <int MAX, typename F>
static bool dispatch_width(int n, F &&f) {
    if constexpr (MAX < 1) {
        return false;
    } else {
        if (n != MAX) return dispatch_width<MAX - 1>(n, f);
        f(std::integral_constant<int, MAX>{});
        return true;
    }
}

extern "C" int mxm_version(void) { return MXM_VERSION; }
extern "C" const char *mxm_last_error(void) { return g_err; }

extern "C" int mxm_linear_supported(int32_t H) {
    return (H >= MXM_LINEAR_MIN_H && H <= 8192) ? 1 : 0;
}

// Scratch layouts of the one-launch loops (fused_kernels.hpp, fused_cols_kernels.hpp), all inside `ws`:
//   [sync block][exchange buffers of the form in use][... free ...][snapshot of the loop vectors at the tail]
static size_t fused_sync_bytes() { return (sizeof(fused_sync) + 255) & ~(size_t)255; }
// The loop vectors of the restarts in flight are saved at the TAIL of the workspace before every launch of a
// one-launch loop (3 x [B][H] doubles + B states), so that a launch that gives up (status -3) can be undone.
static size_t fused_snapshot_bytes(int H, int B) {
    return ((size_t)3 * B * H * sizeof(double) + (size_t)B * sizeof(mxm_em_state) + 255) & ~(size_t)255;
}
// rows split: T / ln T (2 rows) + one partial row per workgroup
static size_t fused_rows_bytes(int H, int nwg) { return (size_t)(nwg + 2) * part_ld(H) * sizeof(double); }
// columns split (R <= FCOLS_MAX_RPT * FCOLS_THREADS): z partials [nwg][ldz] + c [ldz] + L1 partials [2][nwg]
static size_t fused_cols_bytes(int64_t R, int nwg) {
    const size_t ldz = (size_t)((R + 1) & ~(int64_t)1);
    return ((size_t)(nwg + 1) * ldz + 2 * (size_t)nwg) * sizeof(double);
}

extern "C" size_t mxm_workspace_bytes(int64_t R, int32_t H, int32_t B) {
    // restart tiles are processed one after another over the same scratch: one partial row per workgroup and tile member
    const size_t tiles = (size_t)MXM_MAX_WG * MXM_MAX_BT * (size_t)part_ld(H) * sizeof(double);
    // the one-launch loops' blocks (the transposed form's z partials are R-sized, not H-sized, and
    // outgrow the tile scratch of a narrow matrix -- H = 66, R = 1500: 3.2 MB against 2.2 MB)
    size_t fused = fused_rows_bytes(H, MXM_MAX_WG);
    if (R > 0 && R <= (int64_t)FCOLS_MAX_RPT * FCOLS_THREADS) fused = std::max(fused, fused_cols_bytes(R, MXM_MAX_WG));
    fused += fused_sync_bytes() + fused_snapshot_bytes(H, B > 0 ? B : 1) + 512;
    return std::max(tiles, fused);
}

extern "C" int64_t mxm_encode_signatures(const char *text, const int64_t *off, int64_t R,
                                         const int32_t *site_of_pos, int64_t ref_len, int64_t *row_ptr,
                                         uint16_t *site, uint8_t *obs, int64_t cap) {
    int64_t n = 0;
    row_ptr[0] = 0;
    for (int64_t r = 0; r < R; ++r) {
        const char *p = text + off[r];
        const char *end = text + off[r + 1] - 1;           // the separator byte is not part of it
        if (p >= end) return -(r + 1);                     // '' -> int('') in the reference
        while (p < end) {
            int64_t pos = 0;
            int digits = 0;
            while (p < end && *p >= '0' && *p <= '9' && digits < 10) {
                pos = pos * 10 + (*p - '0');
                ++p;
                ++digits;
            }
            if (digits == 0 || digits >= 10 || p >= end || *p != ':') return -(r + 1);
            ++p;
            const char *b = p;
            while (p < end && *p != ',') {
                if (*p == ':') return -(r + 1);
                ++p;
            }
            if (pos >= ref_len || site_of_pos[pos] < 0 || n >= cap) return -(r + 1);
            site[n] = (uint16_t)site_of_pos[pos];
            obs[n] = (p - b == 1) ? (uint8_t)*b : (uint8_t)0;
            ++n;
            if (p < end) {
                ++p;                                       // ','
                if (p >= end) return -(r + 1);             // trailing ',': an empty item
            }
        }
        row_ptr[r + 1] = n;
    }
    return n;
}

extern "C" int mxm_build_em_matrix(const uint8_t *E, int64_t lde, const double *lhit,
                                   const double *lmiss, const int64_t *row_ptr, const uint16_t *site,
                                   const uint8_t *obs, int64_t R, int32_t H, int32_t S, double *M,
                                   int64_t ldm, void *stream) {
    if (R < 0 || H <= 0 || S <= 0) return fail(-1, "mxm_build_em_matrix: bad shape R=%lld H=%d", (long long)R, H);
    if (lde < (((int64_t)H + 7) & ~(int64_t)7) || (lde & 7) != 0 || (reinterpret_cast<uintptr_t>(E) & 7) != 0)
        return fail(-1, "mxm_build_em_matrix: E must be 8-byte aligned with lde a multiple of 8 and >= H rounded up to 8 (lde=%lld)", (long long)lde);
    if (ldm < H) return fail(-1, "mxm_build_em_matrix: ldm < H");
    if (S > 65536) return fail(-1, "mxm_build_em_matrix: more than 65536 variant sites");
    if (R == 0) return 0;
    const int grid = clamp_grid(R, num_cu() * 8);
    const int vec_ok = ((ldm & 1) == 0) && ((reinterpret_cast<uintptr_t>(M) & 15) == 0);
    hipLaunchKernelGGL(build_em_matrix_kernel, dim3(grid), dim3(BUILD_THREADS), 0, (hipStream_t)stream, E,
                       lde, lhit, lmiss, row_ptr, site, obs, R, (int)H, M, ldm, vec_ok);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Both LUT builds after their own first check.  `compact`: row order[i] of the input goes to row i of M (the rows
// entry; else every row to its own place, and a width refusal names the build that takes any width).
static int build_lut_impl(const char *who, const uint8_t *Ecode, int64_t lde, const double *lhit,
                          const double *lmiss, const uint8_t *obsmap, const int64_t *row_ptr, const uint16_t *site,
                          const uint8_t *obs, const int64_t *order, int64_t R, int32_t H, int32_t S, double *M, int64_t ldm,
                          int compact, hipStream_t s) {
    if (H > 8192) return fail(-1, "%s: more than 8192 haplogroups (H=%d)%s", who, H, compact ? "" : ": use mxm_build_em_matrix");
    if (lde < (((int64_t)H + 7) & ~(int64_t)7) || (lde & 7) != 0 || (reinterpret_cast<uintptr_t>(Ecode) & 7) != 0)
        return fail(-1, "%s: Ecode must be 8-byte aligned with lde a multiple of 8 and >= H rounded up to 8 (lde=%lld)", who, (long long)lde);
    if (ldm < H) return fail(-1, "%s: ldm < H", who);
    if (S > 65536 || (int64_t)S * lde >= ((int64_t)1 << 31))
        return fail(-1, "%s: table of %d x %lld bytes exceeds one buffer descriptor", who, S, (long long)lde);
    if (R == 0) return 0;
    const int grid = clamp_grid(R, num_cu() * 8);
    const int nt = (H + LUT_THREADS * LUT_CPL - 1) / (LUT_THREADS * LUT_CPL);
    const int vec_ok = ((ldm & 1) == 0) && ((reinterpret_cast<uintptr_t>(M) & 15) == 0);
    const bool ok = dispatch_width<8>(nt, [&](auto n) {
        constexpr int NT = decltype(n)::value;
        hipLaunchKernelGGL((build_lut_kernel<NT, LUT_CPL>), dim3(grid), dim3(LUT_THREADS), 0, s, Ecode, lde, (int64_t)S * lde, lhit,
                           lmiss, obsmap, row_ptr, site, obs, order, R, (int)H, M, ldm, vec_ok, compact);
    });
    if (!ok) return fail(-1, "%s: H=%d outside the kernel's range", who, H);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_build_em_matrix_lut(const uint8_t *Ecode, int64_t lde, const double *lhit, const double *lmiss,
                                       const uint8_t *obsmap, const int64_t *row_ptr, const uint16_t *site,
                                       const uint8_t *obs, const int64_t *order, int64_t R, int32_t H, int32_t S,
                                       double *M, int64_t ldm, void *stream) {
    if (R < 0 || H <= 0 || S <= 0) return fail(-1, "mxm_build_em_matrix_lut: bad shape R=%lld H=%d", (long long)R, H);
    return build_lut_impl("mxm_build_em_matrix_lut", Ecode, lde, lhit, lmiss, obsmap, row_ptr, site, obs,
                          order, R, H, S, M, ldm, 0, (hipStream_t)stream);
}

// the listed rows into a COMPACT matrix: row rows[i] of the input -> row i of M_out (build_em_records_device's slabs)
extern "C" int mxm_build_em_matrix_lut_rows(const uint8_t *Ecode, int64_t lde, const double *lhit, const double *lmiss,
                                            const uint8_t *obsmap, const int64_t *row_ptr, const uint16_t *site,
                                            const uint8_t *obs, const int64_t *rows, int64_t n_rows, int32_t H, int32_t S,
                                            double *M_out, int64_t ldm, void *stream) {
    if (n_rows < 0 || H <= 0 || S <= 0 || rows == nullptr) return fail(-1, "mxm_build_em_matrix_lut_rows: bad arguments");
    return build_lut_impl("mxm_build_em_matrix_lut_rows", Ecode, lde, lhit, lmiss, obsmap, row_ptr, site, obs, rows, n_rows, H, S,
                          M_out, ldm, 1, (hipStream_t)stream);
}

// The records of a slab of rows that were coded from their dense form (mxm_encode_rows over a compact side matrix) take
// their place in the matrix's record arrays: row rows[i] gets sub_off[i] + base, sub_nd[i], sub_rm[i] where sub_nd[i] > 0.
__global__ __launch_bounds__(256) void scatter_records_kernel(const int64_t *__restrict__ rows, int64_t n, const int64_t *__restrict__ sub_off,
                                                             const int32_t *__restrict__ sub_nd, const double *__restrict__ sub_rm,
                                                             int64_t base, int64_t *__restrict__ rec_off, int32_t *__restrict__ ndist,
                                                             double *__restrict__ rowmax) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n || sub_nd[i] <= 0) return;
    const int64_t r = rows[i];
    rec_off[r] = sub_off[i] + base;
    ndist[r] = sub_nd[i];
    rowmax[r] = sub_rm[i];
}
extern "C" int mxm_scatter_records(const int64_t *rows, int64_t n, const int64_t *sub_off, const int32_t *sub_nd, const double *sub_rm,
                                   int64_t base, int64_t *rec_off, int32_t *ndist, double *rowmax, void *stream) {
    if (n < 0 || (n > 0 && (rows == nullptr || sub_off == nullptr || sub_nd == nullptr || sub_rm == nullptr || rec_off == nullptr ||
                            ndist == nullptr || rowmax == nullptr)))
        return fail(-1, "mxm_scatter_records: bad arguments");
    if (n == 0) return 0;
    hipLaunchKernelGGL(scatter_records_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, n, sub_off,
                       sub_nd, sub_rm, base, rec_off, ndist, rowmax);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Loads the library's code object onto the calling thread's device (HIP does that lazily, on the first launch: ~18 ms that
// would otherwise land in whatever stage launches first) and returns once it is there.
__global__ void preload_kernel() {}
extern "C" int mxm_preload(void) {
    hipLaunchKernelGGL(preload_kernel, dim3(1), dim3(64), 0, (hipStream_t)nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

extern "C" int mxm_set_sparse_max_distinct(int32_t n) {
    return tune_set([n](mxm_tuning &t) { t.sparse_maxd = n < 0 ? -1 : n; });
}

static inline int coded_ld(int H) { return (H + 7) & ~7; }

// marker build: dense rows (M != nullptr) and / or row-dictionary records (out != nullptr)
static int build_sparse_impl(const char *who, const uint8_t *maj, const double *lhit, const double *lmiss,
                             const int32_t *mk_ptr, const uint16_t *mk_hap, const uint8_t *mk_base,
                             const int64_t *row_ptr, const uint16_t *site, const uint8_t *obs, const int64_t *order,
                             int64_t R, int32_t H, int32_t S, double *M, int64_t ldm, const spb_records *out,
                             int64_t *fallback, int64_t *n_fallback, hipStream_t s) {
    if (R < 0 || H <= 0 || S <= 0) return fail(-1, "%s: bad shape R=%lld H=%d", who, (long long)R, H);
    if (H > 8192) return fail(-1, "%s: more than 8192 haplogroups (H=%d): use mxm_build_em_matrix", who, H);
    if (M != nullptr && ldm < H) return fail(-1, "%s: ldm < H", who);
    if (maj == nullptr || mk_ptr == nullptr || fallback == nullptr || n_fallback == nullptr)
        return fail(-1, "%s: marker tables and the fallback list are required", who);
    HIP_TRY(hipMemsetAsync(n_fallback, 0, sizeof(int64_t), s));
    if (out != nullptr) HIP_TRY(hipMemsetAsync(out->stats, 0, 2 * sizeof(int64_t), s));
    if (R == 0) return 0;
    const int hpad = (H + 1) & ~1;
    const int nch = (hpad / 2 + SPB_THREADS - 1) / SPB_THREADS;
    const int vec_ok = (M != nullptr) && ((ldm & 1) == 0) && ((reinterpret_cast<uintptr_t>(M) & 15) == 0);
#ifndef SPB_PASSES
#define SPB_PASSES 3
#endif
    // column ranges per row: the mask array is 1 / passes of a row, which (with the table) decides how many rows a CU holds.
    // 10^6 x 5408, kernel alone, since the marker entries are looked up once per row: 2 ranges 12.0-12.3 ms (4-5 rows per CU),
    // 3 ranges 10.5 ms (6 rows; 12.4 when compiled for 5), 4 ranges 11.2-12.4 ms (profiles/r03/build_kernel_experiments.txt)
    const int passes = SPB_PASSES;
    const int maxd = (T.sparse_maxd < 0 || T.sparse_maxd > SPB_MAXD) ? SPB_MAXD : T.sparse_maxd;
    const int maxd_long = (T.sparse_maxd < 0 || T.sparse_maxd > SPB_MAXD_LONG) ? SPB_MAXD_LONG : T.sparse_maxd;
    const int kpp = (nch + passes - 1) / passes;
    const size_t lds = (size_t)kpp * 2 * SPB_THREADS * 8 + SPB_SLOTS * 8 + 6 * 1024;      // mask array + table + the kernel's other LDS
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 8) per_cu = 8;
    if (per_cu < 1) per_cu = 1;
    const int grid = clamp_grid(R, num_cu() * per_cu * 2);
    const int long_too = T.sparse_long;                  // (0: rows beyond 64 observations go to the fallback list, as before round 6)
    const int grid_long = clamp_grid((R + SPB_LONG_CHUNK - 1) / SPB_LONG_CHUNK, num_cu() * 4 * 2);
    spb_records none = {};
    const spb_records rec = out != nullptr ? *out : none;
    // W = 1: rows of up to 64 observations; W = 2: the rows of 65 .. 128 (below)
    auto launch = [&](auto kernel, int nwg, int max_distinct, int long_rows_too, int long_entries) {
        hipLaunchKernelGGL(kernel, dim3(nwg), dim3(SPB_THREADS), 0, s, maj, lhit, lmiss, mk_ptr, mk_hap, mk_base, row_ptr, site, obs,
                           order, R, (int)H, M, ldm, vec_ok, fallback, reinterpret_cast<unsigned long long *>(n_fallback), max_distinct,
                           rec, long_rows_too, long_entries);
    };
    // (only the instances of the column-range count this build runs with are compiled: the other three quarters of them
    // were a third of the library's build time)
    constexpr int P = SPB_PASSES < 4 ? SPB_PASSES : 4;
    bool one_pass_too_wide = false;
    const bool ok = dispatch_width<16>(nch, [&](auto n) {
        constexpr int N = decltype(n)::value;
        if constexpr (P == 1 && N > 7) one_pass_too_wide = true;
        else if (out != nullptr) launch(build_sparse_kernel<N, P, true, 1>, grid, maxd, long_too, 0);
        else launch(build_sparse_kernel<N, P, false, 1>, grid, maxd, long_too, 0);
    });
    if (one_pass_too_wide) return fail(-1, "%s: one pass covers H <= 3584", who);
    if (!ok) return fail(-1, "%s: H=%d outside the kernel's range", who, H);
    HIP_TRY(hipGetLastError());
    if (long_too != 0) {
        // the rows of 65 .. 128 observations (merged mates, long reads): 128-bit masks, one column range per 512 haplogroups
        // and a table of 1024 slots (build_sparse_kernels.hpp, W = 2); its grid looks at the rows 64 at a time
#ifndef SPB_LONG_KPP
#define SPB_LONG_KPP 2                // 512-haplogroup chunks per column range of the long rows' instance (1: 34.9, 2: 34.5, 4: 36.5 ms
                                      // per 10^6 paired-end fragments before the walk over a long row's further entries was fixed)
#endif
        (void)dispatch_width<16>(nch, [&](auto n) {
            constexpr int N = decltype(n)::value, PL = (N + SPB_LONG_KPP - 1) / SPB_LONG_KPP;
            if (out != nullptr) launch(build_sparse_kernel<N, PL, true, 2>, grid_long, maxd_long, 0, T.sparse_long_entries);
            else launch(build_sparse_kernel<N, PL, false, 2>, grid_long, maxd_long, 0, T.sparse_long_entries);
        });
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_build_em_matrix_sparse(const uint8_t *maj, const double *lhit, const double *lmiss,
                                          const int32_t *mk_ptr, const uint16_t *mk_hap, const uint8_t *mk_base,
                                          const int64_t *row_ptr, const uint16_t *site, const uint8_t *obs,
                                          const int64_t *order, int64_t R, int32_t H, int32_t S, double *M, int64_t ldm,
                                          int64_t *fallback, int64_t *n_fallback, void *stream) {
    MXM_ENTER();
    if (M == nullptr) return fail(-1, "mxm_build_em_matrix_sparse: M required");
    return build_sparse_impl("mxm_build_em_matrix_sparse", maj, lhit, lmiss, mk_ptr, mk_hap, mk_base, row_ptr, site, obs,
                             order, R, H, S, M, ldm, nullptr, fallback, n_fallback, (hipStream_t)stream);
}

extern "C" size_t mxm_record_bytes(int64_t R, int32_t H) {
    if (R < 0 || H <= 0) return 0;
    // the larger of a full byte-coded record and a full wide one
    return (size_t)(R > 0 ? R : 1) * (2 * (size_t)coded_ld(H) + 16 * ENC_MAX_WIDE);
}

extern "C" int mxm_build_em_records(const uint8_t *maj, const double *lhit, const double *lmiss,
                                    const int32_t *mk_ptr, const uint16_t *mk_hap, const uint8_t *mk_base,
                                    const int64_t *row_ptr, const uint16_t *site, const uint8_t *obs,
                                    const int64_t *order, int64_t R, int32_t H, int32_t S, double *M, int64_t ldm,
                                    uint8_t *rec, size_t rec_bytes, int64_t *rec_off, int32_t *ndist, double *rowmax,
                                    int64_t *stats, int64_t *fallback, int64_t *n_fallback, void *stream) {
    MXM_ENTER();
    if (!mxm_linear_supported(H))
        return fail(-1, "mxm_build_em_records: records need H in [65, 8192] (H=%d)", H);
    if (rec == nullptr || (reinterpret_cast<uintptr_t>(rec) & 15) || rec_bytes < (size_t)coded_ld(H) + 16 * ENC_MAX_CODES ||
        rec_off == nullptr || ndist == nullptr || rowmax == nullptr || stats == nullptr)
        return fail(-1, "mxm_build_em_records: record buffer (16-byte aligned, >= one record) and output arrays required");
    spb_records out;
    out.rec = rec;
    out.rec_cap = (long long)rec_bytes;
    out.rec_off = rec_off;
    out.ndist = ndist;
    out.rowmax = rowmax;
    out.stats = reinterpret_cast<unsigned long long *>(stats);
    out.ldc = coded_ld(H);
    return build_sparse_impl("mxm_build_em_records", maj, lhit, lmiss, mk_ptr, mk_hap, mk_base, row_ptr, site, obs, order,
                             R, H, S, M, ldm, &out, fallback, n_fallback, (hipStream_t)stream);
}

template <typename ST>
static int linearize_wide(const double *M, int64_t ldm, int64_t R, int H, ST *P, int64_t ldp, double *rowmax,
                          hipStream_t s) {
    const int nch = (H / 2 + 255) / 256;
    int cap = num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG;
    const int nwg = clamp_grid((R + 1) / 2, cap);           // rows are dealt round-robin (row_deal)
    const bool ok = dispatch_width<16>(nch, [&](auto n) {
        hipLaunchKernelGGL((linearize_wide_kernel<decltype(n)::value, ST>), dim3(nwg), dim3(256), 0, s, M, ldm, R, H, P, ldp, rowmax);
    });
    return ok ? 0 : 1;
}

static inline bool wide_rows_ok(const void *M, int64_t ldm, int H) {
    return ((H & 1) == 0) && ((ldm & 1) == 0) && ((reinterpret_cast<uintptr_t>(M) & 15) == 0) && H >= 64 && H <= 8192;
}

extern "C" int mxm_linearize(const double *M, int64_t ldm, int64_t R, int32_t H, double *P, int64_t ldp,
                             double *rowmax, void *stream) {
    if (R < 0 || H <= 0) return fail(-1, "mxm_linearize: bad shape");
    if (ldm < H || ldp < H || (ldp & 1)) return fail(-1, "mxm_linearize: ldp must be even and >= H (ldp=%lld)", (long long)ldp);
    if (R == 0) return 0;
    if (wide_rows_ok(M, ldm, H) && (reinterpret_cast<uintptr_t>(P) & 15) == 0 &&
        linearize_wide<double>(M, ldm, R, (int)H, P, ldp, rowmax, (hipStream_t)stream) == 0) {
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const int grid = clamp_grid(R, num_cu() * 8);
    hipLaunchKernelGGL(linearize_kernel, dim3(grid), dim3(ROW_THREADS), 0, (hipStream_t)stream, M, ldm, R,
                       (int)H, P, ldp, rowmax);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- optional timing hook (bench.py): events recorded right around the dominant kernel --------
extern "C" int mxm_set_timing_events(void *ev_start, void *ev_stop) {
    return tune_set([=](mxm_tuning &t) { t.ev_start = (hipEvent_t)ev_start; t.ev_stop = (hipEvent_t)ev_stop; });
}

extern "C" int mxm_set_min_rows_per_wg(int32_t n) {
    if (n < 1) return fail(-1, "mxm_set_min_rows_per_wg: n < 1");
    return tune_set([n](mxm_tuning &t) { t.min_rows_per_wg = n; });
}

extern "C" int mxm_set_compact_restarts(int32_t mode) {
    return tune_set([mode](mxm_tuning &t) { t.compact_restarts = mode < 0 ? 0 : (mode > 2 ? 2 : mode); });
}

extern "C" int mxm_set_batch_tile(int32_t bt) {
    if (bt < 1 || bt > 4) return fail(-1, "mxm_set_batch_tile: tile must be 1..4");
    return tune_set([bt](mxm_tuning &t) { t.max_bt = bt; });
}

extern "C" int mxm_set_fused_coded_grid(int32_t nwg) {
    return tune_set([nwg](mxm_tuning &t) { t.fused_coded_wg = nwg > 0 ? nwg : 0; });
}

extern "C" int mxm_set_sparse_long_rows(int32_t on) {
    return tune_set([on](mxm_tuning &t) { t.sparse_long = on ? 1 : 0; });
}
extern "C" int mxm_set_sparse_long_entries(int32_t n) {
    return tune_set([n](mxm_tuning &t) { t.sparse_long_entries = n > 0 ? n : 0; });
}
extern "C" int mxm_set_coded_batch_tile(int32_t bt) {
    if (bt != 1 && bt != 3) return fail(-1, "mxm_set_coded_batch_tile: 1 or 3, got %d", bt);
    return tune_set([bt](mxm_tuning &t) { t.coded_bt = bt; });
}
extern "C" int mxm_set_quad_encoder(int32_t kind) {
    if (kind != 0 && kind != 1) return fail(-1, "mxm_set_quad_encoder: 0 or 1, got %d", kind);
    return tune_set([kind](mxm_tuning &t) { t.quad_encoder = kind; });
}
extern "C" int mxm_set_quad_left_grid(int32_t nwg) {
    return tune_set([nwg](mxm_tuning &t) { t.quad_left_wg = nwg > 0 ? nwg : 0; });
}

extern "C" int mxm_diag_fused_force_abort(int32_t on) {
    return tune_set([on](mxm_tuning &t) { t.fused_force_abort = on ? 1 : 0; });
}

// ---- wide-kernel dispatch over NCH ------------------------------------------------------------
// Tuned shapes of the streaming kernel per batch size: workgroup threads, register ring depth
// (rows in flight = NBUF - 1 per workgroup), workgroups per CU of the persistent grid.
#ifndef MXM_V1_THREADS
#define MXM_V1_THREADS 256
#endif
#ifndef MXM_V1_NBUF
#define MXM_V1_NBUF 2
#endif
#ifndef MXM_V1_WG_PER_CU
#define MXM_V1_WG_PER_CU 2
#endif
#ifndef MXM_V2_THREADS
#define MXM_V2_THREADS 512
#endif
#ifndef MXM_V2_NBUF
#define MXM_V2_NBUF 2                 // with dealt rows: 6.42 ms vs 6.85 ms (ring 3) per pass at 1M x 5408 (profiles/r01/row_mapping.txt)
#endif
#ifndef MXM_V3_THREADS
#define MXM_V3_THREADS 512
#endif
#ifndef MXM_V3_NBUF
#define MXM_V3_NBUF 2
#endif
#ifndef MXM_V4_THREADS
#define MXM_V4_THREADS 512
#endif
#ifndef MXM_V4_NBUF
#define MXM_V4_NBUF 2
#endif
// restarts of a batch whose proportions stay in VGPRs (the rest sit in LDS: 160 KiB hold three
// vectors of H = 5408, so four restarts per pass need one of them in registers)
#ifndef MXM_V2_PREG
#define MXM_V2_PREG 1
#endif
#ifndef MXM_V3_PREG
#define MXM_V3_PREG 2
#endif
#ifndef MXM_V4_PREG
#define MXM_V4_PREG 2
#endif
// the single-restart shape of the dense matrix (512 threads, one workgroup per CU, ring 3: in-process A/B 6.43 vs 6.50 ms
// median, profiles/r01/tune_sweep.txt); the 256-thread shape above runs the dense leftover rows of a row-dictionary plan
#ifndef MXM_V1B_THREADS
#define MXM_V1B_THREADS 512
#endif
#ifndef MXM_V1B_NBUF
#define MXM_V1B_NBUF 3
#endif
#define MXM_MAX_COL2 4096             // column pairs per row the register tiling covers (H <= 8192)
#define MXM_LDS_BUDGET (156 * 1024)   // of the CU's 160 KiB, leaving room for the exchange buffers

static inline int variant_threads(int nb) {
    return nb == 1 ? MXM_V1_THREADS : (nb == 2 ? MXM_V2_THREADS : (nb == 3 ? MXM_V3_THREADS : MXM_V4_THREADS));
}
static inline int variant_preg(int nb) {
    return nb == 1 ? 1 : (nb == 2 ? MXM_V2_PREG : (nb == 3 ? MXM_V3_PREG : MXM_V4_PREG));
}

static size_t batch_lds_bytes(int H, int nb) {
    const int threads = variant_threads(nb);
    const int nch = ((H + 1) / 2 + threads - 1) / threads;
    return (size_t)(nb - variant_preg(nb)) * nch * threads * 16;
}

// A tile of nb restarts needs its LDS-resident proportions to fit and a spill-free kernel
// instance (scratch in the row loop costs 2-5x): column chunks per thread up to which the default
// shapes compile without scratch (-Rpass-analysis=kernel-resource-usage), per tile size.
static bool batch_fits(int H, int nb) {
    if (nb <= 1) return true;
    static const int max_nch[MXM_MAX_BT + 1] = {0, 16, 8, 7, 6};
    const int threads = variant_threads(nb);
    const int nch = ((H + 1) / 2 + threads - 1) / threads;
    return nch <= max_nch[nb] && batch_lds_bytes(H, nb) <= MXM_LDS_BUDGET;
}

template <int THREADS, int NCH, int BT, int NBUF, int PREG>
static int launch_wide(const double *P, int64_t ldp, const double *w, const double *props, int64_t R,
                       int H, int grid, double *partial, int64_t ldpart,
                       const mxm_em_state *state, mxm_slots slots, hipStream_t stream) {
    if constexpr (NCH * THREADS > MXM_MAX_COL2) {
        return fail(-1, "mxm_em_iter: H=%d outside the linear kernel's range", H);
    } else {
        const size_t lds = (size_t)(BT - PREG) * NCH * THREADS * sizeof(d2);
        RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&em_iter_wide_kernel<THREADS, NCH, BT, NBUF, PREG>), lds, "em_iter_wide_kernel"));
        hipLaunchKernelGGL((em_iter_wide_kernel<THREADS, NCH, BT, NBUF, PREG>), dim3(grid), dim3(THREADS), lds,
                           stream, P, ldp, w, props, R, H, partial, ldpart, state, slots);
        return 0;
    }
}

template <int THREADS, int BT, int NBUF, int PREG>
static int dispatch_wide(int nch, const double *P, int64_t ldp, const double *w, const double *props,
                         int64_t R, int H, int grid, double *partial,
                         int64_t ldpart, const mxm_em_state *state, mxm_slots slots, hipStream_t stream) {
    int rc = 0;
    const bool ok = dispatch_width<16>(nch, [&](auto n) {
        rc = launch_wide<THREADS, decltype(n)::value, BT, NBUF, PREG>(P, ldp, w, props, R, H, grid, partial, ldpart, state, slots, stream);
    });
    return ok ? rc : fail(-1, "mxm_em_iter: H=%d outside the linear kernel's range", H);
}

static inline mxm_slots slots_from(int first) {
    mxm_slots sl;
    for (int i = 0; i < MXM_MAX_BT; ++i) sl.s[i] = first + i;
    return sl;
}

// One tile of nb (<= MXM_MAX_BT) restarts over the linear matrix: streaming kernel + column reduce.
// props / state / colsum are the BASES of the loop vectors; the tile's members are slots.s[0 .. nb).
// stream_linear_tile: the streaming kernel alone, partial rows [0, *nwg_out) of `partial`.
static int stream_linear_tile(const double *P, int64_t ldp, const double *w, const double *props, int64_t R,
                              int H, int nb, mxm_slots &slots, const mxm_em_state *state,
                              double *partial, hipStream_t stream, bool timed, int *nwg_out, int max_wg = MXM_MAX_WG,
                              int v1_shape = -1) {
    const int64_t ldpart = part_ld(H);
    const int ncol2 = (H + 1) / 2;
    if (v1_shape < 0) v1_shape = 1;
    const bool alt = (nb == 1) && (v1_shape == 1);          // the second single-restart shape
    const int threads = alt ? MXM_V1B_THREADS : variant_threads(nb);
    const int wg_per_cu = alt ? 1 : ((nb == 1) ? MXM_V1_WG_PER_CU : 1);
    const int nch = (ncol2 + threads - 1) / threads;
    int cap = num_cu() * wg_per_cu;
    if (cap > max_wg) cap = max_wg;
    // rows are dealt round-robin over the workgroups (row_deal, common.hpp).  Small matrices:
    // fewer workgroups with more rows each (every workgroup pays 2 x H x 8 bytes of proportion
    // loads and partial stores, which colreduce then reads back)
    const int nwg = clamp_grid((R + T.min_rows_per_wg - 1) / T.min_rows_per_wg, cap);
    for (int i = nb; i < MXM_MAX_BT; ++i) slots.s[i] = slots.s[0];          // unused entries stay in range
    if (timed && T.ev_start != nullptr) HIP_TRY(hipEventRecord(T.ev_start, stream));
    int rc;
    if (alt)
        rc = dispatch_wide<MXM_V1B_THREADS, 1, MXM_V1B_NBUF, 1>(nch, P, ldp, w, props, R, H, nwg, partial, ldpart, state, slots, stream);
    else if (nb == 1)
        rc = dispatch_wide<MXM_V1_THREADS, 1, MXM_V1_NBUF, 1>(nch, P, ldp, w, props, R, H, nwg, partial, ldpart, state, slots, stream);
    else if (nb == 2)
        rc = dispatch_wide<MXM_V2_THREADS, 2, MXM_V2_NBUF, MXM_V2_PREG>(nch, P, ldp, w, props, R, H, nwg, partial, ldpart, state, slots, stream);
    else if (nb == 3)
        rc = dispatch_wide<MXM_V3_THREADS, 3, MXM_V3_NBUF, MXM_V3_PREG>(nch, P, ldp, w, props, R, H, nwg, partial, ldpart, state, slots, stream);
    else
        rc = dispatch_wide<MXM_V4_THREADS, 4, MXM_V4_NBUF, MXM_V4_PREG>(nch, P, ldp, w, props, R, H, nwg, partial, ldpart, state, slots, stream);
    if (rc != 0) return rc;
    HIP_TRY(hipGetLastError());
    if (timed && T.ev_stop != nullptr) HIP_TRY(hipEventRecord(T.ev_stop, stream));
    *nwg_out = nwg;
    return 0;
}

// The template instance stream_linear_tile launches for a tile of nb restarts at width H, as a profiler prints it
// ("em_iter_wide_kernel<512, 6, 1, 3, 1>"): bench.py matches its committed counter files by this name.
extern "C" int mxm_describe_stream_kernel(int32_t H, int32_t nb, char *buf, size_t len) {
    if (buf == nullptr || len == 0 || H <= 0 || nb < 1 || nb > MXM_MAX_BT) return fail(-1, "mxm_describe_stream_kernel: bad arguments");
    const int ncol2 = (H + 1) / 2;
    const bool alt = nb == 1;
    const int threads = alt ? MXM_V1B_THREADS : variant_threads(nb);
    const int nbuf = alt ? MXM_V1B_NBUF : (nb == 2 ? MXM_V2_NBUF : (nb == 3 ? MXM_V3_NBUF : MXM_V4_NBUF));
    snprintf(buf, len, "em_iter_wide_kernel<%d, %d, %d, %d, %d>", threads, (ncol2 + threads - 1) / threads, nb, nbuf,
             variant_preg(nb));
    return 0;
}

// What the loop driver hands down when the finalize may ride on the column reduce's launch (no collective in between).
struct fin_args {
    double *ln_cur, *ln_new, *props_cur;
    mxm_em_state *state;
    double tol;
    int max_iter;
};

// column reduce of a tile's partial rows [0, nwg); with `fin` the finalize follows in the same launch
static int reduce_tile(const double *partial, int nwg, int nb, int H, double *colsum, const mxm_em_state *state,
                       const mxm_slots &slots, const fin_args *fin, hipStream_t stream,
                       wide_check wc = wide_check{nullptr, 0, 0}) {
    if (fin != nullptr && H <= 64 * FIN_MAX_BLOCKS)
        hipLaunchKernelGGL(colreduce_finalize_kernel, dim3((H + 63) / 64, nb), dim3(COLRED_THREADS), 0, stream, partial,
                           part_ld(H), nwg, nb, H, colsum, fin->ln_cur, fin->ln_new, fin->props_cur, fin->tol, fin->max_iter,
                           fin->state, slots, wc);
    else
        hipLaunchKernelGGL(colreduce_kernel, dim3((H + 63) / 64, nb), dim3(COLRED_THREADS), 0, stream, partial, part_ld(H), nwg,
                           nb, H, (const double *)nullptr, colsum, const_cast<mxm_em_state *>(state), slots, wc);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ... of ONE vector's partial rows (a restart on its own, a vote): no tile, no list check
static int reduce_one(const double *partial, int nwg, int H, double *colsum, const mxm_em_state *state, hipStream_t stream) {
    hipLaunchKernelGGL(colreduce_kernel, dim3((H + 63) / 64, 1), dim3(COLRED_THREADS), 0, stream, partial, part_ld(H), nwg, 1, H,
                       (const double *)nullptr, colsum, const_cast<mxm_em_state *>(state), slots_from(0), wide_check{nullptr, 0, 0});
    HIP_TRY(hipGetLastError());
    return 0;
}

static int em_iter_linear_tile(const double *P, int64_t ldp, const double *w, const double *props, int64_t R,
                               int H, int nb, mxm_slots slots, const mxm_em_state *state, double *colsum,
                               double *partial, hipStream_t stream, bool timed, const fin_args *fin = nullptr) {
    int nwg = 0;
    RC_TRY(stream_linear_tile(P, ldp, w, props, R, H, nb, slots, state, partial, stream, timed, &nwg));
    return reduce_tile(partial, nwg, nb, H, colsum, state, slots, fin, stream);
}

#ifndef MXM_F32_THREADS
#define MXM_F32_THREADS 256
#endif
#ifndef MXM_F32_NBUF
#define MXM_F32_NBUF 2
#endif
#ifndef MXM_F32_WG_PER_CU
#define MXM_F32_WG_PER_CU 2
#endif

template <int NCH>
static int launch_wide_f32(const float *P, int64_t ldp, const double *w, const double *props, int64_t R, int H,
                           int grid, double *partial, int64_t ldpart,
                           const mxm_em_state *state, hipStream_t stream) {
    if constexpr (NCH * MXM_F32_THREADS > 2048) {
        return fail(-1, "mxm_em_iter_f32: H=%d outside the kernel's range", H);
    } else {
        hipLaunchKernelGGL((em_iter_wide_f32_kernel<MXM_F32_THREADS, NCH, MXM_F32_NBUF>), dim3(grid),
                           dim3(MXM_F32_THREADS), 0, stream, P, ldp, w, props, R, H, partial, ldpart,
                           state);
        return 0;
    }
}

static int em_iter_f32_one(const float *P, int64_t ldp, const double *w, const double *props, int64_t R, int H,
                           const mxm_em_state *state, double *colsum, double *partial, hipStream_t stream,
                           bool timed) {
    const int64_t ldpart = part_ld(H);
    const int nch = ((H + 3) / 4 + MXM_F32_THREADS - 1) / MXM_F32_THREADS;
    const int nbuf = MXM_F32_NBUF;
    int cap = num_cu() * MXM_F32_WG_PER_CU;
    if (cap > MXM_MAX_WG) cap = MXM_MAX_WG;
    const int nwg = clamp_grid((R + nbuf - 1) / nbuf, cap);
    if (timed && T.ev_start != nullptr) HIP_TRY(hipEventRecord(T.ev_start, stream));
    int lrc = 0;
    const bool ok = dispatch_width<8>(nch, [&](auto n) {
        lrc = launch_wide_f32<decltype(n)::value>(P, ldp, w, props, R, H, nwg, partial, ldpart, state, stream);
    });
    if (!ok) return fail(-1, "mxm_em_iter_f32: H=%d outside the kernel's range", H);
    if (lrc != 0) return lrc;
    HIP_TRY(hipGetLastError());
    if (timed && T.ev_stop != nullptr) HIP_TRY(hipEventRecord(T.ev_stop, stream));
    return reduce_one(partial, nwg, H, colsum, state, stream);
}

// Narrow matrices (the refinement EM's contributor columns): one thread per row up to 32 columns,
// a lane pair per row up to 64.
#define MXM_NARROW_MAX_H 64
template <bool ITER>
static int launch_narrow(const double *M, int64_t ldm, const double *w, const double *ln_props, int64_t R, int H,
                         double *out, int64_t ldo, int mode, double *partial, int64_t ldpart,
                         const mxm_em_state *state, hipStream_t stream, int *nwg_out) {
    const int cap = num_cu() * 4 < MXM_MAX_WG ? num_cu() * 4 : MXM_MAX_WG;
    const int rows_per_wg = (H <= 32) ? 256 : 128;
    const int nwg = clamp_grid((R + rows_per_wg - 1) / rows_per_wg, cap);
    *nwg_out = nwg;
#define NARROW_LAUNCH(hmax, lpr)                                                                             \
    hipLaunchKernelGGL((estep_narrow_kernel<hmax, ITER, lpr>), dim3(nwg), dim3(256), 0, stream, M, ldm, w, ln_props, R, H, \
                       out, ldo, mode, partial, ldpart, state)
    if (H <= 4) NARROW_LAUNCH(4, 1);
    else if (H <= 8) NARROW_LAUNCH(8, 1);
    else if (H <= 16) NARROW_LAUNCH(16, 1);
    else if (H <= 32) NARROW_LAUNCH(32, 1);
    else NARROW_LAUNCH(32, 2);
#undef NARROW_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

static int em_iter_log_one(const double *M, int64_t ldm, const double *w, const double *ln_props, int64_t R, int H,
                           const mxm_em_state *state, double *colsum, double *partial, hipStream_t stream) {
    if (M == nullptr) return fail(-1, "mxm_em_iter: M is NULL and the linear path does not apply");
    if (ln_props == nullptr) return fail(-1, "mxm_em_iter: ln_props is NULL and the log-space path needs it");
    const size_t lds = 2 * (size_t)H * sizeof(double);
    const int64_t ldpart = part_ld(H);
    int nwg;
    if (lds > 150 * 1024) {
        // wider than the log-space kernel's LDS vectors (9600 columns): the any-width form (vectors in global memory)
        nwg = clamp_grid(R, num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG);
        hipLaunchKernelGGL((estep_global_kernel<true>), dim3(nwg), dim3(ROW_THREADS), 0, stream, M, ldm, w, ln_props, R, H,
                           (double *)nullptr, (int64_t)0, 0, partial, ldpart, state, (const int64_t *)nullptr);
        HIP_TRY(hipGetLastError());
    } else if (H <= MXM_NARROW_MAX_H) {
        const int rc = launch_narrow<true>(M, ldm, w, ln_props, R, H, (double *)nullptr, (int64_t)0, 0, partial, ldpart,
                                           state, stream, &nwg);
        if (rc != 0) return rc;
    } else {
        nwg = clamp_grid(R, num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG);
        RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&estep_log_kernel<true>), lds, "estep_log_kernel"));
        hipLaunchKernelGGL((estep_log_kernel<true>), dim3(nwg), dim3(ROW_THREADS), lds, stream, M, ldm, w, ln_props,
                           R, H, (double *)nullptr, (int64_t)0, 0, partial, ldpart, state);
        HIP_TRY(hipGetLastError());
    }
    return reduce_one(partial, nwg, H, colsum, state, stream);
}

extern "C" int mxm_em_iter(const double *M, int64_t ldm, const double *P, int64_t ldp, const double *w,
                           const double *props, const double *ln_props, int64_t R, int32_t H, int32_t B,
                           const mxm_em_state *state, double *colsum, void *ws, size_t ws_bytes, void *stream) {
    MXM_ENTER();
    if (R <= 0 || H <= 0 || B <= 0) return fail(-1, "mxm_em_iter: bad shape R=%lld H=%d", (long long)R, H);
    if (ws == nullptr || ws_bytes < mxm_workspace_bytes(R, H, B)) return fail(-1, "mxm_em_iter: workspace too small");
    if (P != nullptr && ((ldp & 1) || ldp < H)) return fail(-1, "mxm_em_iter: ldp must be even and >= H");
    if (M != nullptr && ldm < H) return fail(-1, "mxm_em_iter: ldm < H");
    const bool linear = (P != nullptr) && mxm_linear_supported(H);
    // restarts are taken in tiles of up to T.max_bt that share one pass over the matrix; the
    // scratch is reused tile after tile (same stream, so the passes are ordered)
    // a batch keeps (most of) its proportion vectors in LDS: the largest tile that fits
    int max_bt = linear ? T.max_bt : 1;
    while (max_bt > 1 && !batch_fits((int)H, max_bt)) --max_bt;
    for (int b = 0; b < B;) {
        // the fewest passes that cover what is left, restarts spread evenly over them (a pass
        // costs nearly the same for 1..4 restarts, a little more the fuller it is):
        // 10 -> 4 + 3 + 3, 5 -> 3 + 2, 8 -> 4 + 4
        const int left = B - b;
        const int passes = (left + max_bt - 1) / max_bt;
        const int nb = (left + passes - 1) / passes;
        const mxm_em_state *st = state ? state + b : nullptr;
        int rc;
        if (linear)
            rc = em_iter_linear_tile(P, ldp, w, props, R, (int)H, nb, slots_from(b), state, colsum, (double *)ws,
                                     (hipStream_t)stream, b == 0);
        else
            rc = em_iter_log_one(M, ldm, w, ln_props ? ln_props + (int64_t)b * H : nullptr, R, (int)H, st,
                                 colsum + (int64_t)b * H, (double *)ws, (hipStream_t)stream);
        if (rc != 0) return rc;
        b += nb;
    }
    return 0;
}

extern "C" int mxm_linearize_f32(const double *M, int64_t ldm, int64_t R, int32_t H, float *P, int64_t ldp,
                                 double *rowmax, void *stream) {
    if (R < 0 || H <= 0) return fail(-1, "mxm_linearize_f32: bad shape");
    if (ldm < H || ldp < H || (ldp & 3)) return fail(-1, "mxm_linearize_f32: ldp must be a multiple of 4 and >= H (ldp=%lld)", (long long)ldp);
    if (R == 0) return 0;
    if (wide_rows_ok(M, ldm, H) && (reinterpret_cast<uintptr_t>(P) & 7) == 0 && (ldp & 1) == 0 &&
        linearize_wide<float>(M, ldm, R, (int)H, P, ldp, rowmax, (hipStream_t)stream) == 0) {
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const int grid = clamp_grid(R, num_cu() * 8);
    hipLaunchKernelGGL(linearize_f32_kernel, dim3(grid), dim3(ROW_THREADS), 0, (hipStream_t)stream, M, ldm, R, (int)H,
                       P, ldp, rowmax);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_em_iter_f32(const float *P, int64_t ldp, const double *w, const double *props, int64_t R,
                               int32_t H, int32_t B, const mxm_em_state *state, double *colsum, void *ws,
                               size_t ws_bytes, void *stream) {
    MXM_ENTER();
    if (R <= 0 || H <= 0 || B <= 0) return fail(-1, "mxm_em_iter_f32: bad shape R=%lld H=%d", (long long)R, H);
    if (!mxm_linear_supported(H)) return fail(-1, "mxm_em_iter_f32: H=%d outside the linear kernel's range", H);
    if (P == nullptr || (ldp & 3) || ldp < H) return fail(-1, "mxm_em_iter_f32: ldp must be a multiple of 4 and >= H");
    if (ws == nullptr || ws_bytes < mxm_workspace_bytes(R, H, B)) return fail(-1, "mxm_em_iter_f32: workspace too small");
    for (int b = 0; b < B; ++b) {
        const int rc = em_iter_f32_one(P, ldp, w, props + (int64_t)b * H, R, (int)H, state ? state + b : nullptr,
                                       colsum + (int64_t)b * H, (double *)ws, (hipStream_t)stream, b == 0);
        if (rc != 0) return rc;
    }
    return 0;
}

// ---- row-dictionary storage (coded_kernels.hpp) ------------------------------------------------
extern "C" size_t mxm_coded_bytes(int64_t R, int32_t H) { return mxm_record_bytes(R, H); }

extern "C" int mxm_encode_rows(const double *M, int64_t ldm, int64_t R, int32_t H, uint8_t *rec, size_t rec_bytes,
                               int64_t *rec_off, int32_t *ndist, double *rowmax, int64_t *stats, void *stream) {
    if (R <= 0 || H <= 0 || ldm < H) return fail(-1, "mxm_encode_rows: bad shape R=%lld H=%d", (long long)R, H);
    // (round 5: any H in the linear kernels' range and any row stride -- a row's loads go through a descriptor of exactly
    // H doubles and need the doubles' own 8-byte alignment only; an odd H or an odd stride used to send the matrix back to
    // the 7 x larger dense form)
    if (!mxm_linear_supported(H) || (reinterpret_cast<uintptr_t>(M) & 7) != 0)
        return fail(-1, "mxm_encode_rows: needs H in [65, 8192] (H=%d ldm=%lld)", H, (long long)ldm);
    if (rec == nullptr || (reinterpret_cast<uintptr_t>(rec) & 15) || rec_bytes < (size_t)coded_ld(H) + 16 * ENC_MAX_CODES)
        return fail(-1, "mxm_encode_rows: record buffer missing, unaligned or smaller than one record");
    if (rec_off == nullptr || ndist == nullptr || rowmax == nullptr || stats == nullptr)
        return fail(-1, "mxm_encode_rows: output arrays required");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), s));
    const int ldc = coded_ld(H);
    const int nch = (ldc / 4 + ENC_THREADS - 1) / ENC_THREADS;
    const int grid = clamp_grid(R, num_cu() * 4);
    // first pass: every row, byte codes; second pass: the rows it left without a record, 16-bit codes
    const int grid_w = clamp_grid((R + 31) / 32, num_cu() * 3);
    const bool ok = dispatch_width<8>(nch, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        unsigned long long *st = reinterpret_cast<unsigned long long *>(stats);
        hipLaunchKernelGGL((encode_rows_kernel<NCH>), dim3(grid), dim3(ENC_THREADS), 0, s, M, ldm, R, (int)H, ldc, rec,
                           (int64_t)rec_bytes, rec_off, ndist, rowmax, st);
        hipLaunchKernelGGL((encode_wide_rows_kernel<NCH>), dim3(grid_w), dim3(ENC_THREADS), 0, s, M, ldm, R, (int)H, ldc, rec,
                           (int64_t)rec_bytes, rec_off, ndist, rowmax, st);
    });
    if (!ok) return fail(-1, "mxm_encode_rows: H=%d outside the kernel's range", H);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int coded_check(const mxm_coded *c, int32_t H, const char *who) {
    if (c == nullptr || c->R <= 0 || H <= 0 || !mxm_linear_supported(H))
        return fail(-1, "%s: bad coded matrix (rows %lld, H %d)", who, (long long)(c ? c->R : 0), H);
    if (c->rec == nullptr || c->rec_off == nullptr || c->ndist == nullptr) return fail(-1, "%s: coded matrix arrays missing", who);
    if (c->R_rest < 0 || (c->R_rest > 0 && (c->P_rest == nullptr || c->ldp_rest < H || (c->ldp_rest & 1) ||
                                            (reinterpret_cast<uintptr_t>(c->P_rest) & 15))))
        return fail(-1, "%s: the dense rest needs 16-byte aligned rows with an even ld >= H", who);
    if (c->n_wide < 0 || (c->n_wide > 0 && c->wide_rows == nullptr)) return fail(-1, "%s: n_wide > 0 needs wide_rows", who);
    if (c->qrec != nullptr) {                            // a quad dictionary beside the records
        if (c->qoff == nullptr || c->nquad == nullptr || c->n_quad_rows < 0 || c->n_byte_rows < 0 ||
            (c->n_quad_rows > 0 && c->quad_rows == nullptr) || (c->n_byte_rows > 0 && c->byte_rows == nullptr) ||
            (reinterpret_cast<uintptr_t>(c->qrec) & 31))
            return fail(-1, "%s: quad dictionary arrays missing (or qrec not 32-byte aligned)", who);
        if (c->n_quad_rows + c->n_byte_rows + c->n_wide + c->R_rest != c->R)
            return fail(-1, "%s: quad_rows + byte_rows + wide_rows + the dense rest must be all %lld rows", who, (long long)c->R);
    }
    return 0;
}

static int rest_check(const char *who, int32_t H, const double *M_rest, int64_t ldm_rest, const int64_t *rest_rows, int64_t n_rest) {
    if (n_rest < 0 || (n_rest > 0 && (M_rest == nullptr || rest_rows == nullptr || ldm_rest < H)))
        return fail(-1, "%s: the rows without a record need M_rest, rest_rows and ldm_rest >= H", who);
    return 0;
}

extern "C" size_t mxm_quad_bytes(int64_t R, int32_t H) {
    (void)H;
    // the encoders hand `qrec` out in pieces of QUAD_CHUNK bytes: a piece holds at least six records of the largest size
    // (2048 + 256 x 32 bytes) and at most 5120 pieces are open -- reserved, partly unused -- when the call ends
    // (R x the largest record alone, the figure until round 6, left the pieces' tails out)
    constexpr size_t largest = QUAD_CODE_BYTES + QUAD_MAX * 32, per_piece = (size_t)QUAD_CHUNK / largest;
    return R > 0 ? (((size_t)R + per_piece - 1) / per_piece + 5120) * (size_t)QUAD_CHUNK : 0;
}

extern "C" int mxm_expand_tables(const uint8_t *maj, const int32_t *mk_ptr, const uint16_t *mk_hap, const uint8_t *mk_base,
                                 const uint8_t *map256, int32_t S, int32_t H, int64_t lde, uint8_t *out, void *stream) {
    if (maj == nullptr || mk_ptr == nullptr || mk_hap == nullptr || mk_base == nullptr || out == nullptr || S <= 0 || H <= 0 || lde < H)
        return fail(-1, "mxm_expand_tables: bad arguments");
    hipLaunchKernelGGL(expand_tables_kernel, dim3(clamp_grid(S, num_cu() * 8)), dim3(256), 0, (hipStream_t)stream, maj, mk_ptr, mk_hap,
                       mk_base, map256, (int)S, (int)H, lde, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" size_t mxm_quad_lists_scratch_bytes(int64_t R) {
    return R > 0 ? (size_t)((R + QLIST_CHUNK - 1) / QLIST_CHUNK) * 2 * sizeof(long long) : 0;
}

extern "C" int mxm_quad_lists(const int32_t *ndist, const int32_t *nquad, int64_t R, int64_t *quad_rows, int64_t *byte_rows,
                              int64_t *counts, void *scratch, size_t scratch_bytes, void *stream) {
    MXM_ENTER();
    if (ndist == nullptr || nquad == nullptr || R <= 0 || quad_rows == nullptr || byte_rows == nullptr || counts == nullptr)
        return fail(-1, "mxm_quad_lists: bad arguments");
    if (scratch == nullptr || scratch_bytes < mxm_quad_lists_scratch_bytes(R)) return fail(-1, "mxm_quad_lists: scratch too small");
    const int64_t nchunk = (R + QLIST_CHUNK - 1) / QLIST_CHUNK;
    if (nchunk > 0x7fffffff) return fail(-1, "mxm_quad_lists: too many rows");
    hipStream_t s = (hipStream_t)stream;
    long long *cc = static_cast<long long *>(scratch);
    hipLaunchKernelGGL(quad_list_count_kernel, dim3((unsigned)nchunk), dim3(QLIST_THREADS), 0, s, ndist, nquad, R, cc);
    hipLaunchKernelGGL(quad_list_scan_kernel, dim3(1), dim3(QLIST_THREADS), 0, s, cc, nchunk, reinterpret_cast<long long *>(counts));
    hipLaunchKernelGGL(quad_list_fill_kernel, dim3((unsigned)nchunk), dim3(QLIST_THREADS), 0, s, ndist, nquad, R, cc, quad_rows, byte_rows);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_build_quads(const mxm_coded *c, int32_t H, uint8_t *qrec, size_t qrec_bytes, int64_t *qoff, int32_t *nquad,
                               uint64_t *stats, void *stream) {
    MXM_ENTER();
    if (c == nullptr || c->R <= 0 || c->rec == nullptr || c->rec_off == nullptr || c->ndist == nullptr || !mxm_linear_supported(H))
        return fail(-1, "mxm_build_quads: bad coded matrix (rows %lld, H %d)", (long long)(c ? c->R : 0), H);
    if (qoff == nullptr || nquad == nullptr || stats == nullptr || (qrec == nullptr && qrec_bytes > 0) ||
        (reinterpret_cast<uintptr_t>(qrec) & 31))
        return fail(-1, "mxm_build_quads: qoff, nquad, stats and a 32-byte aligned qrec required");
    const int ldc = coded_ld(H);
    if (ldc / 4 > 8 * QUAD_THREADS) return fail(-1, "mxm_build_quads: H=%d beyond eight quads per thread", H);
    HIP_TRY(hipMemsetAsync(stats, 0, 2 * sizeof(uint64_t), (hipStream_t)stream));
    // (either way at most 5120 pieces of QUAD_CHUNK bytes are open at the end: what the caller's first guess leaves room for)
    if (T.quad_encoder == 1 && ldc / 4 <= 64 * QW_K)
        hipLaunchKernelGGL(quad_encode_wave_kernel, dim3(clamp_grid((c->R + QW_WAVES - 1) / QW_WAVES, std::min(num_cu() * QW_MIN_WAVES, 5120 / QW_WAVES))), dim3(QUAD_THREADS),
                           0, (hipStream_t)stream, c->rec, c->rec_off, c->ndist, ldc, (int)H, c->R, qrec,
                           (unsigned long long)qrec_bytes, qoff, nquad, reinterpret_cast<unsigned long long *>(stats));
    else
        hipLaunchKernelGGL(quad_encode_kernel, dim3(clamp_grid(c->R, num_cu() * 8)), dim3(QUAD_THREADS), 0, (hipStream_t)stream,
                           c->rec, c->rec_off, c->ndist, ldc, (int)H, c->R, qrec, (unsigned long long)qrec_bytes, qoff, nquad,
                           reinterpret_cast<unsigned long long *>(stats));
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_decode_rows(const mxm_coded *c, int32_t H, double *P, int64_t ldp, void *stream) {
    RC_TRY(coded_check(c, H, "mxm_decode_rows"));
    if (P == nullptr || ldp < H) return fail(-1, "mxm_decode_rows: ldp < H");
    hipLaunchKernelGGL(decode_rows_kernel, dim3(clamp_grid(c->R, num_cu() * 8)), dim3(256), 0, (hipStream_t)stream, c->rec,
                       c->rec_off, c->ndist, coded_ld(H), c->R, (int)H, P, ldp);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_row_argmax_votes_coded(const mxm_coded *c, int32_t H, int32_t n_runs, const double *ln_props,
                                          const double *props, const double *rowmax, const double *M_rest, int64_t ldm_rest,
                                          const int64_t *rest_rows, int64_t n_rest, const double *w, int32_t *best,
                                          double *votes, void *ws, size_t ws_bytes, void *stream) {
    RC_TRY(coded_check(c, H, "mxm_row_argmax_votes_coded"));
    if (ln_props == nullptr || best == nullptr || n_runs < 1 || n_runs > RECK_MAX_RUNS)
        return fail(-1, "mxm_row_argmax_votes_coded: ln_props, best and 1..%d runs required", RECK_MAX_RUNS);
    if (n_runs > 1 && (props == nullptr || rowmax == nullptr))
        return fail(-1, "mxm_row_argmax_votes_coded: several runs need props and rowmax (each run's row normaliser)");
    RC_TRY(rest_check("mxm_row_argmax_votes_coded", H, M_rest, ldm_rest, rest_rows, n_rest));
    if (votes != nullptr && (ws == nullptr || ws_bytes < mxm_workspace_bytes(c->R, H, 1)))
        return fail(-1, "mxm_row_argmax_votes_coded: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t lse_lds = (size_t)n_runs * sizeof(double);
    const int ldc_a = coded_ld(H);
    const int nch_a = (ldc_a / 4 + 255) / 256;
    // one run: the normaliser drops out -- the register-resident form (records_argmax_kernel)
    const bool fast = n_runs == 1 && dispatch_width<8>(nch_a, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        // one wave of workgroups: as many as are resident at once (a second, partial wave of equally long workgroups
        // would double the kernel's time)
        int per_cu = 2;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, records_argmax_narrow_kernel<NCH>, 256, 0) != hipSuccess || per_cu < 1) {
            (void)hipGetLastError();
            per_cu = 2;
        }
        hipLaunchKernelGGL((records_argmax_narrow_kernel<NCH>), dim3(clamp_grid(c->R, num_cu() * per_cu)), dim3(256), 0, s, c->rec,
                           c->rec_off, c->ndist, ldc_a, c->R, (int)H, ln_props, best);
        // the wide rows, found from ndist itself (no list: the vote must not depend on one)
        hipLaunchKernelGGL((records_argmax_kernel<NCH, true>), dim3(clamp_grid((c->R + 255) / 256, num_cu() * 2)), dim3(256), 0, s,
                           c->rec, c->rec_off, c->ndist, ldc_a, c->R, (int)H, ln_props, best, (const int64_t *)nullptr);
    });
    if (!fast)
        hipLaunchKernelGGL(posterior_argmax_kernel<true>, dim3(clamp_grid(c->R, num_cu() * 8)), dim3(256), lse_lds, s, c->rec, c->rec_off,
                           c->ndist, coded_ld(H), (const double *)nullptr, (int64_t)0, (const int64_t *)nullptr, c->R, (int)H,
                           (int)n_runs, ln_props, props, rowmax, best);
    HIP_TRY(hipGetLastError());
    if (n_rest > 0) {
        hipLaunchKernelGGL(posterior_argmax_kernel<false>, dim3(clamp_grid(n_rest, num_cu() * 8)), dim3(256), lse_lds, s,
                           (const uint8_t *)nullptr, (const int64_t *)nullptr, (const int32_t *)nullptr, 0, M_rest, ldm_rest,
                           rest_rows, n_rest, (int)H, (int)n_runs, ln_props, props, rowmax, best);
        HIP_TRY(hipGetLastError());
    }
    if (votes != nullptr) {
        const int64_t ldpart = part_ld(H);
        const int nwg = clamp_grid((c->R + 255) / 256, num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG);
        const size_t vlds = (size_t)H * sizeof(double);
        RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&votes_from_best_kernel), vlds, "votes_from_best_kernel",
                              "mxm_row_argmax_votes_coded", H, "too wide for the vote kernel"));
        hipLaunchKernelGGL(votes_from_best_kernel, dim3(nwg), dim3(256), vlds, s, best, w, c->R, (int)H, (double *)ws, ldpart);
        HIP_TRY(hipGetLastError());
        return reduce_one((const double *)ws, nwg, (int)H, votes, nullptr, s);
    }
    return 0;
}

extern "C" int mxm_em_step_coded(const mxm_coded *c, int32_t H, const double *ln_props, const double *props,
                                 const double *rowmax, const double *M_rest, int64_t ldm_rest, const int64_t *rest_rows,
                                 int64_t n_rest, double *out, int64_t ldo, int32_t mode, void *stream) {
    RC_TRY(coded_check(c, H, "mxm_em_step_coded"));
    if (ln_props == nullptr || props == nullptr || rowmax == nullptr || out == nullptr || ldo < H)
        return fail(-1, "mxm_em_step_coded: bad arguments");
    RC_TRY(rest_check("mxm_em_step_coded", H, M_rest, ldm_rest, rest_rows, n_rest));
    hipLaunchKernelGGL(coded_posterior_kernel, dim3(clamp_grid(c->R, num_cu() * 8)), dim3(256), 0, (hipStream_t)stream, c->rec,
                       c->rec_off, c->ndist, coded_ld(H), c->R, (int)H, ln_props, props, rowmax, out, ldo, (int)mode);
    HIP_TRY(hipGetLastError());
    if (n_rest > 0) {
        // the rows without a record: the reference's E-step in log space on their dense copies, each written to its
        // own row of `out`
        const size_t lds = 2 * (size_t)H * sizeof(double);
        RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&estep_log_kernel<false>), lds, "estep_log_kernel", "mxm_em_step_coded", H,
                              "too large"));
        hipLaunchKernelGGL((estep_log_kernel<false>), dim3(clamp_grid(n_rest, num_cu() * 2)), dim3(ROW_THREADS), lds,
                           (hipStream_t)stream, M_rest, ldm_rest, (const double *)nullptr, ln_props, n_rest, (int)H, out, ldo,
                           (int)mode, (double *)nullptr, (int64_t)0, (const mxm_em_state *)nullptr, rest_rows);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int mxm_gather_columns_coded(const mxm_coded *c, int32_t H, const int32_t *cols, int32_t nC, const double *M_rest,
                                        int64_t ldm_rest, const int64_t *rest_rows, int64_t n_rest, double *out,
                                        int64_t ldo, void *stream) {
    RC_TRY(coded_check(c, H, "mxm_gather_columns_coded"));
    if (cols == nullptr || out == nullptr || nC <= 0 || ldo < nC) return fail(-1, "mxm_gather_columns_coded: bad arguments");
    RC_TRY(rest_check("mxm_gather_columns_coded", H, M_rest, ldm_rest, rest_rows, n_rest));
    const int64_t blocks = (c->R * nC + 255) / 256;
    hipLaunchKernelGGL(coded_gather_columns_kernel, dim3(clamp_grid(blocks, num_cu() * 16)), dim3(256), 0, (hipStream_t)stream,
                       c->rec, c->rec_off, c->ndist, coded_ld(H), c->R, cols, (int)nC, out, ldo);
    HIP_TRY(hipGetLastError());
    if (n_rest > 0) {
        hipLaunchKernelGGL(gather_columns_kernel, dim3(clamp_grid((n_rest * nC + 255) / 256, num_cu() * 16)), dim3(256), 0,
                           (hipStream_t)stream, M_rest, ldm_rest, n_rest, cols, (int)nC, out, ldo, rest_rows);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// Shape of em_iter_coded_kernel {threads, rows in flight, workgroups per CU}: 256 x 4 x 2 measured best of five
// (profiles/r02/coded_shapes.txt)
struct coded_shape { int threads, nbuf, wg_per_cu; };
static const coded_shape g_coded_shapes[] = {{256, 4, 2}};
static const int g_coded_shape = 0;
template <int THREADS, int NBUF, int MINWG>
static int launch_coded(int nch, int nwg, hipStream_t stream, const mxm_coded *c, int ldc, const double *w, const double *props,
                        int H, double *partial, int64_t ldpart, const mxm_em_state *state, int run,
                        const int64_t *row_list = nullptr, int64_t n_list = 0, int part_row0 = 0) {
    bool launched = false;
    (void)dispatch_width<8>(nch, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        if constexpr (NCH * THREADS <= 2048) {
            hipLaunchKernelGGL((em_iter_coded_kernel<THREADS, NCH, NBUF, MINWG>), dim3(nwg), dim3(THREADS), 0, stream, c->rec, c->rec_off,
                               c->ndist, ldc, w, c->wide_rows, c->n_wide, props, c->R, H, partial, ldpart, state, run, row_list, n_list,
                               c->nquad, part_row0);
            launched = true;
        }
    });
    return launched ? 0 : fail(-1, "mxm_em_iter_coded: H=%d outside the kernel's range", H);
}
#define QUAD_MAX_NCH 6              // H <= 6144: the instances of the quad pass that compile without scratch
// The leftover pass's share of a grid of `slots` workgroups it shares with the quad pass, by the measured cost of a row in
// each pass (us per row and workgroup: quad 0.67; byte 1.0 and wide 1.5 where only a few workgroups run that pass -- a
// sweep of the share at 10^6 rows, profiles/r05/quads_product_1m.txt: 22 workgroups 1.56 ms, 32 1.33, 48 1.36, 64 1.40,
// 128 1.62), so that both finish together; 0 when there is nothing left over.
static int quad_left_share(const mxm_coded *c, int slots) {
    if (c->n_byte_rows <= 0 && c->n_wide <= 0) return 0;
    const double left_cost = 1.0 * (double)c->n_byte_rows + 1.5 * (double)c->n_wide;
    const double quad_cost = 0.67 * (double)c->n_quad_rows;
    int n = (int)((double)slots * left_cost / (left_cost + quad_cost) + 0.5);
    if (T.quad_left_wg > 0) n = T.quad_left_wg;
    if (n < 4) n = 4;
    if (n > slots / 2) n = slots / 2;
    const int64_t left = c->n_byte_rows > c->n_wide ? c->n_byte_rows : c->n_wide;
    n = clamp_grid(left, n);
    return n < 1 ? 1 : n;
}
static int launch_quad(int nch, int nwg, hipStream_t stream, const mxm_coded *c, const double *w, const double *props, int H,
                       double *partial, int64_t ldpart, const mxm_em_state *state, int run) {
    const bool ok = dispatch_width<QUAD_MAX_NCH>(nch, [&](auto n) {               // (7, 8: 35 registers spilled)
        hipLaunchKernelGGL((em_iter_quad_kernel<decltype(n)::value, 4>), dim3(nwg), dim3(QUAD_THREADS), 0, stream, c->qrec, c->qoff,
                           c->nquad, c->quad_rows, c->n_quad_rows, c->R, w, props, H, partial, ldpart, 0, state, run);
    });
    return ok ? 0 : fail(-1, "mxm_em_iter_coded: H=%d outside the quad kernel's range", H);
}
static int launch_quad_coded(int nch, int nwg, int nwg_left, hipStream_t stream, const mxm_coded *c, int ldc, const double *w,
                             const double *props, int H, double *partial, int64_t ldpart, const mxm_em_state *state, int run) {
    // an EMPTY list is still a list: a null pointer would mean "every row" to the pass
    const int64_t *byte_rows = c->byte_rows != nullptr ? c->byte_rows : c->quad_rows;
    const bool ok = dispatch_width<QUAD_MAX_NCH>(nch, [&](auto n) {
        hipLaunchKernelGGL((em_iter_quad_coded_kernel<decltype(n)::value, 4>), dim3(nwg), dim3(QUAD_THREADS), 0, stream, c->rec,
                           c->rec_off, c->ndist, ldc, c->wide_rows, c->n_wide, byte_rows, c->n_byte_rows, c->qrec, c->qoff, c->nquad,
                           c->quad_rows, c->n_quad_rows, c->R, w, props, H, partial, ldpart, nwg_left, state, run);
    });
    return ok ? 0 : fail(-1, "mxm_em_iter_coded: H=%d outside the quad kernel's range", H);
}

// One restart's pass over a coded matrix: dictionary rows through em_iter_coded_kernel, the dense rest
// through em_iter_wide_kernel into the partial rows behind, one column reduce over both.
static int em_iter_coded_one(const mxm_coded *c, const double *w, const double *props, int H, int run,
                             const mxm_em_state *state, double *colsum, double *partial, hipStream_t stream, bool timed,
                             const fin_args *fin = nullptr) {
    const int64_t ldpart = part_ld(H);
    const int ldc = coded_ld(H);
    const coded_shape sh = g_coded_shapes[g_coded_shape];
    const int nch = (ldc / 4 + sh.threads - 1) / sh.threads;
    int cap = num_cu() * sh.wg_per_cu;
    if (cap > MXM_MAX_WG - num_cu()) cap = MXM_MAX_WG - num_cu();             // the dense rest's rows come behind
    if (cap < 1) cap = 1;
    const bool quads = c->qrec != nullptr && c->n_quad_rows > 0 && nch <= QUAD_MAX_NCH;   // (wider: the records alone)
    // beside a quad dictionary: the quad rows' pass (partial rows 0 .. nwg_q) and the pass over the byte-coded rows without
    // quads and the wide rows (rows nwg_q .. nwg) share ONE grid (em_iter_quad_coded_kernel)
    int nwg_q = 0, nwg = 0;
    if (quads) {
        const int slots = cap < 2 * num_cu() ? cap : 2 * num_cu();
        const int nwg_b = quad_left_share(c, slots);
        nwg_q = clamp_grid((c->n_quad_rows + sh.nbuf - 1) / sh.nbuf, slots - nwg_b < 1 ? 1 : slots - nwg_b);
        nwg = nwg_q + nwg_b;
    } else {
        nwg = clamp_grid((c->R + sh.nbuf - 1) / sh.nbuf, cap);
    }
    if (timed && T.ev_start != nullptr) HIP_TRY(hipEventRecord(T.ev_start, stream));
    // {wide rows met, list fault} per workgroup: the kernel leaves them behind the partial rows this path can use
    // (coded_row_pass, CHECK; em_iter_coded_kernel forms the same address)
    int *chk = reinterpret_cast<int *>(partial + (int64_t)MXM_MAX_WG * ldpart);
    int lrc;
    if (quads) {
        // one grid: the leftover pass on its first nwg - nwg_q workgroups beside the quad pass on the others
        // (em_iter_quad_coded_kernel); no leftover rows at all: the quad kernel alone
        if (nwg > nwg_q) lrc = launch_quad_coded(nch, nwg, nwg - nwg_q, stream, c, ldc, w, props, H, partial, ldpart, state, run);
        else lrc = launch_quad(nch, nwg_q, stream, c, w, props, H, partial, ldpart, state, run);
        if (lrc != 0) return lrc;
    } else {
        lrc = launch_coded<256, 4, 2>(nch, nwg, stream, c, ldc, w, props, H, partial, ldpart, state, run);
        if (lrc != 0) return lrc;
    }
    HIP_TRY(hipGetLastError());
    if (timed && T.ev_stop != nullptr) HIP_TRY(hipEventRecord(T.ev_stop, stream));
    int nwg_rest = 0;
    mxm_slots sl;
    for (int i = 0; i < MXM_MAX_BT; ++i) sl.s[i] = run;
    if (c->R_rest > 0) {
        const int rc = stream_linear_tile(c->P_rest, c->ldp_rest, c->w_rest, props, c->R_rest, H, 1, sl, state,
                                          partial + (int64_t)nwg * ldpart, stream, false, &nwg_rest, MXM_MAX_WG - nwg,
                                          0 /* the 256-thread instance: the few dense rows show up under a kernel
                                               name of their own in a trace, apart from the dense matrix's passes */);
        if (rc != 0) return rc;
    }
    // (with a row list the byte pass meets no wide row in its main loop: the lists are checked entry by entry instead)
    return reduce_tile(partial, nwg + nwg_rest, 1, H, colsum, state, sl, fin, stream, wide_check{chk, nwg, quads ? 0ll : (long long)c->n_wide});
}

// ---- QB_BT restarts through one pass over the records beside a quad dictionary (quad_batched_kernels.hpp) ----------
#define QB_BT 3
// Can a tile of QB_BT restarts share one pass over this coded matrix?  It takes a quad dictionary (the kernel's first
// and largest class of rows), a width the quad pass covers, and dense leftover rows (random matrices), if any, that
// the dense kernel takes three restarts at a time too.
static bool coded_batch_ok(const mxm_coded *c, int H) {
    if (T.coded_bt < QB_BT || c == nullptr || c->qrec == nullptr || c->n_quad_rows <= 0) return false;
    if (c->R_rest > 0 && !batch_fits(H, QB_BT)) return false;                // (the dense leftover rows' tile of three)
    const int nch256 = (coded_ld(H) / 4 + QUAD_THREADS - 1) / QUAD_THREADS;
    return nch256 <= QUAD_MAX_NCH && mxm_linear_supported(H);
}
static int em_iter_coded_batched(const mxm_coded *c, const double *w, const double *props, int H, const mxm_slots &tile,
                                 const mxm_em_state *state, double *colsum, double *partial, hipStream_t stream, bool timed,
                                 const fin_args *fin = nullptr) {
    const int64_t ldpart = part_ld(H);
    const int ldc = coded_ld(H);
    const int nch = ((ldc / 4 + QUAD_THREADS - 1) / QUAD_THREADS + 1) / 2;      // code bytes per thread of 512
    int cap = num_cu();
    if (cap > MXM_MAX_WG / QB_BT - num_cu() / QB_BT) cap = MXM_MAX_WG / QB_BT - num_cu() / QB_BT;   // (the dense rest's rows come behind)
    if (cap < 1) cap = 1;
    const int nwg = clamp_grid((c->n_quad_rows + 2) / 3, cap);
    mxm_slots sl = tile;
    for (int i = QB_BT; i < MXM_MAX_BT; ++i) sl.s[i] = sl.s[0];
    if (timed && T.ev_start != nullptr) HIP_TRY(hipEventRecord(T.ev_start, stream));
    const int64_t *byte_rows = c->byte_rows != nullptr ? c->byte_rows : c->quad_rows;      // (an empty list is still a list)
    const int64_t *wide_rows = c->wide_rows != nullptr ? c->wide_rows : c->quad_rows;
    // two launches on the same grid: the quad rows start the partial sums, the leftover rows (byte-coded without quads,
    // wide) are added to them (quad_batched_kernels.hpp: as one kernel the three row loops spill into the quad rows' loop)
    const bool left = c->n_byte_rows > 0 || c->n_wide > 0;
    const bool ok = dispatch_width<3>(nch, [&](auto n) {
        constexpr int NCH = decltype(n)::value;
        auto pass = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(nwg), dim3(QB_THREADS), 0, stream, c->rec, c->rec_off, c->ndist, ldc, wide_rows, c->n_wide,
                               byte_rows, c->n_byte_rows, c->qrec, c->qoff, c->nquad, c->quad_rows, c->n_quad_rows, c->R, w, props, H,
                               partial, ldpart, state, sl);
        };
        pass(em_iter_quad_batched_kernel<QB_BT, NCH, 1>);
        if (left) pass(em_iter_quad_batched_kernel<QB_BT, NCH, 6>);
    });
    if (!ok) return fail(-1, "mxm_em_iter_coded: H=%d outside the batched quad kernel's range", H);
    HIP_TRY(hipGetLastError());
    if (timed && T.ev_stop != nullptr) HIP_TRY(hipEventRecord(T.ev_stop, stream));
    int nwg_rest = 0;
    if (c->R_rest > 0) {
        const int rc = stream_linear_tile(c->P_rest, c->ldp_rest, c->w_rest, props, c->R_rest, H, QB_BT, sl, state,
                                          partial + (int64_t)nwg * QB_BT * ldpart, stream, false, &nwg_rest,
                                          (MXM_MAX_WG - nwg * QB_BT) / QB_BT);
        if (rc != 0) return rc;
    }
    int *chk = reinterpret_cast<int *>(partial + (int64_t)MXM_MAX_WG * ldpart);
    return reduce_tile(partial, nwg + nwg_rest, QB_BT, H, colsum, state, sl, fin, stream, wide_check{chk, nwg, 0ll});
}

extern "C" int mxm_em_iter_coded(const mxm_coded *c, const double *w, const double *props, int32_t H, int32_t B,
                                 mxm_em_state *state, double *colsum, void *ws, size_t ws_bytes, void *stream) {
    MXM_ENTER();
    RC_TRY(coded_check(c, H, "mxm_em_iter_coded"));
    if (B <= 0 || props == nullptr || colsum == nullptr) return fail(-1, "mxm_em_iter_coded: bad arguments");
    if (ws == nullptr || ws_bytes < mxm_workspace_bytes(c->R, H, B)) return fail(-1, "mxm_em_iter_coded: workspace too small");
    // beside a quad dictionary full tiles of QB_BT restarts share a pass (the remainder: one per pass)
    int b = 0;
    if (coded_batch_ok(c, (int)H)) {
        for (; b + QB_BT <= B; b += QB_BT) {
            RC_TRY(em_iter_coded_batched(c, w, props, (int)H, slots_from(b), state, colsum, (double *)ws, (hipStream_t)stream, b == 0));
        }
    }
    for (; b < B; ++b) {
        RC_TRY(em_iter_coded_one(c, w, props, (int)H, b, state, colsum, (double *)ws, (hipStream_t)stream, b == 0));
    }
    return 0;
}

extern "C" int mxm_restart_tile_coded(const mxm_coded *c, int32_t H) {
    MXM_ENTER();
    return coded_batch_ok(c, (int)H) ? QB_BT : 1;
}

extern "C" int mxm_restart_tile(int32_t H) {
    MXM_ENTER();
    if (!mxm_linear_supported(H)) return 1;
    int bt = T.max_bt;
    while (bt > 1 && !batch_fits((int)H, bt)) --bt;
    return bt;
}

extern "C" int mxm_m_finalize(const double *colsum, double *ln_cur, double *ln_new, double *props_cur, int32_t H,
                              int32_t B, double tol, int32_t max_iter, mxm_em_state *state, void *stream) {
    if (H <= 0 || B <= 0 || state == nullptr) return fail(-1, "mxm_m_finalize: bad arguments");
    if (H > 64 * FIN_MAX_BLOCKS) {                        // any width: one workgroup per restart
        hipLaunchKernelGGL(finalize_any_kernel, dim3(1, B), dim3(FIN_THREADS), 0, (hipStream_t)stream, colsum, ln_cur, ln_new,
                           props_cur, (int)H, tol, (int)max_iter, state, 0, 0, slots_from(0));
        HIP_TRY(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(finalize_kernel, dim3((H + FIN_THREADS - 1) / FIN_THREADS, B), dim3(FIN_THREADS), 0, (hipStream_t)stream,
                       colsum, ln_cur, ln_new, props_cur, (int)H, tol, (int)max_iter, state, 0, 0, slots_from(0));
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the run_em inner loop (em.py:126-143) as a native driver -----------------------------------
// Iterations are enqueued in chunks; for small matrices the chunk is captured once into a
// hipGraph and replayed (the loop is launch-bound there: 3 kernels of a few microseconds each),
// for large ones plain launches already run ahead of the GPU.  Either way the kernels of a
// finished restart are no-ops, so the state freezes on the iteration the reference stops on.
extern "C" int mxm_set_loop_graph(int32_t mode) {
    return tune_set([mode](mxm_tuning &t) { t.loop_graph = mode < 0 ? -1 : (mode > 0 ? 1 : 0); });
}

// ---- progress hook: called on the host thread inside mxm_em_loop after every state read-back ------
extern "C" int mxm_set_progress_callback(mxm_progress_fn fn, void *user, int32_t every) {
    return tune_set([=](mxm_tuning &t) { t.progress = fn; t.progress_user = user; t.progress_every = every > 0 ? every : 10; });
}

// ---- one-launch loop for cache-resident matrices (fused_kernels.hpp) ---------------------------
extern "C" int mxm_set_loop_fused(int32_t mode, int32_t chunk) {
    return tune_set([=](mxm_tuning &t) {
        t.loop_fused = mode < 0 ? -1 : (mode > 0 ? 1 : 0);
        t.fused_cols = (mode == 2) ? 0 : 1;            // mode 2: one launch, rows split (A/B against the transposed form)
        t.fused_chunk = chunk > 0 ? chunk : 0;
    });
}

// The transposed one-launch loop (fused_cols_kernels.hpp): up to 1536 rows, a 256-CU grid.
static bool fused_cols_eligible(int64_t R, int H, int nwg) {
    if (!T.fused_cols || nwg != 256) return false;          // the Z reduce is laid out for 256 partials per row
    if (R > (int64_t)FCOLS_MAX_RPT * FCOLS_THREADS || (R + nwg - 1) / nwg > 2 * FCOLS_NQ) return false;
    const int cp = (H + nwg - 1) / nwg;
    if (cp > FCOLS_MAX_CP) return false;
    // 24 columns x 3 rows per thread do not fit the register file without scratch (22 x 3 -- Build 17's width
    // on 256 CUs -- do): the widest matrices up to 1024 rows
    return cp <= 22 || R <= 2 * (int64_t)FCOLS_THREADS;
}
// ... and its exchange buffers must fit between the sync block and the snapshot (a caller may hand in less than
// mxm_workspace_bytes asks for today: the rows-split form or the per-iteration kernels then run instead)
static bool fused_cols_fits(int64_t R, int H, int B, int nwg, size_t ws_bytes) {
    return ws_bytes >= fused_sync_bytes() + fused_cols_bytes(R, nwg) + fused_snapshot_bytes(H, B) + 256;
}

// `running`: restarts that still have iterations to do.  Automatic mode takes the one-launch loop for ONE
// restart only: it runs restarts one after another (17 / 26 / 80 us per restart-iteration at 600 / 2400 /
// 10 000 rows), while the per-iteration kernels share each pass between up to four of them (11 / 15 / 27 us
// from three restarts on; profiles/r02/small_runs_restarts.txt).
static bool fused_eligible(const double *P, int64_t ldp, int64_t R, int H, int B, size_t ws_bytes, bool p_is_f32, int running) {
    if (T.loop_fused == 0 || p_is_f32 || P == nullptr || !mxm_linear_supported(H)) return false;
    if ((ldp & 1) || (reinterpret_cast<uintptr_t>(P) & 15)) return false;
    int nwg = num_cu() < MXM_MAX_WG ? num_cu() : MXM_MAX_WG;
    const int ncol2 = (H + 1) / 2;
    if ((ncol2 + nwg - 1) / nwg > 16 * FUSED_MAX_M) return false;           // slice wider than the column reduce covers
    if ((ncol2 + FUSED_THREADS - 1) / FUSED_THREADS > FUSED_MAX_NCH) return false;   // spill-free instances only
    if ((int64_t)nwg * part_ld(H) * 8 >= ((int64_t)1 << 31)) return false;  // one buffer descriptor over the partials
    if (ws_bytes < fused_sync_bytes() + fused_rows_bytes(H, nwg) + fused_snapshot_bytes(H, B) + 256) return false;
    if (T.loop_fused == 1) return true;
    // the transposed form runs a restart-iteration in 12 us at 600 rows whatever the number of restarts; the
    // batched kernels need 18 / 13 / 11 us with 2 / 3 / 4 restarts per pass: up to three restarts stay here
    if (running <= 3 && fused_cols_eligible(R, H, nwg) && fused_cols_fits(R, H, B, nwg, ws_bytes)) return true;
    return running <= 1 && (double)R * (double)H <= T.fused_cells;
}

// The one-launch loop over records (fused_coded_kernels.hpp): any number of rows, restarts one after another (the
// per-iteration coded kernels take one restart per pass too, so nothing is lost), no dense leftover rows.
static int fused_coded_grid(int64_t R) {
    int nwg = num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG;         // two workgroups of 256 per CU
    if (T.fused_coded_wg > 0) {
        if (T.fused_coded_wg < nwg) nwg = T.fused_coded_wg;
    } else {
        // an iteration costs ~0.7 us per row of a workgroup plus ~0.026 us per workgroup (barriers, one partial row
        // each way through the fabric): the minimum of 0.7 R / n + 0.026 n is at n = 5.2 sqrt(R) (measured sweep:
        // profiles/r04/small_runs_coded_grids.txt -- 600 rows: 128 workgroups 18.8 us, 512 30.1; 10^4 rows: level
        // from 384 up), in whole eights (the XCDs)
        const int best = ((int)(5.2 * sqrt((double)R)) + 7) & ~7;
        if (best < nwg) nwg = best;
    }
    if ((int64_t)nwg > R) nwg = (int)R;
    return nwg < 1 ? 1 : nwg;
}
#define QUAD_PER_ITER_MIN_ROWS 300000
#define QUAD_BATCH_MIN_ROWS 15000     // ... with three or more restarts running: tiles of three share a pass, which beats the one-launch
                                      // loop (restarts one after another) from the smallest record plans on: 45 against 55 us per
                                      // restart-iteration at 2*10^4 rows, 172 against 244 at 1.5*10^5 (profiles/r06/multi_restart_routes.txt)
// the floor a binding's "auto" rule must use too: a dictionary of fewer quad rows is never looked at by mxm_em_loop_coded
extern "C" int64_t mxm_quad_loop_min_rows(int32_t B) { return B >= 3 ? QUAD_BATCH_MIN_ROWS : QUAD_PER_ITER_MIN_ROWS; }
static bool fused_coded_eligible(const mxm_coded *c, int H, int B, size_t ws_bytes, int running = 1) {
    if (T.loop_fused == 0 || c == nullptr || c->R_rest > 0 || !mxm_linear_supported(H) || (H & 1)) return false;
    // beside a quad dictionary the per-iteration kernels are the faster loop from a few 10^5 rows (1.35 against 1.45 ms per
    // iteration at 10^6: the quad pass saves 0.13 ms of the row pass, the one-launch loop ~0.04 ms of launches and tail;
    // a one-launch loop with the quad pass inside ran 1.41): the one-launch loop, which reads the records only, keeps
    // the small matrices (mxm_set_loop_fused(1, ...) still forces it)
    if (c->qrec != nullptr && c->n_quad_rows >= QUAD_PER_ITER_MIN_ROWS && T.loop_fused != 1 &&
        (coded_ld(H) / 4 + QUAD_THREADS - 1) / QUAD_THREADS <= QUAD_MAX_NCH)
        return false;
    // ... and with a full tile of restarts still running, from far fewer rows (round 6)
    if (running >= 3 && T.loop_fused != 1 && c->n_quad_rows >= QUAD_BATCH_MIN_ROWS && coded_batch_ok(c, H)) return false;
    const int nwg = fused_coded_grid(c->R);
    const int ncol2 = H / 2;
    if ((ncol2 + nwg - 1) / nwg > 16 * FCODED_MAX_M) return false;           // slice wider than the column reduce covers
    if ((coded_ld(H) / 4 + FCODED_THREADS - 1) / FCODED_THREADS > 8) return false;
    if ((int64_t)nwg * part_ld(H) * 8 >= ((int64_t)1 << 31)) return false;   // one buffer descriptor over the partials
    return ws_bytes >= fused_sync_bytes() + fused_rows_bytes(H, nwg) + fused_snapshot_bytes(H, B) + 256;
}

// Diagnostic (-DFUSED_STAMPS builds): the per-phase clock sums of the last one-launch loop, from the
// sync block at the start of `ws`; all zeros in the shipped library.
extern "C" int mxm_diag_fused_stamps(const void *ws, unsigned long long *out_host) {
    if (ws == nullptr || out_host == nullptr) return fail(-1, "mxm_diag_fused_stamps: bad arguments");
    const fused_sync *sync = reinterpret_cast<const fused_sync *>(ws);
    HIP_TRY(hipMemcpy(out_host, sync->stamps, sizeof(sync->stamps), hipMemcpyDeviceToHost));
    return 0;
}

// A persistent grid with grid barriers must be co-resident: ask the runtime how many workgroups of the instance fit a
// CU before launching (returns false -> the caller takes the per-iteration kernels instead).
template <typename K>
static bool grid_fits(K kernel, int threads, int nwg) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return (long long)per_cu * num_cu() >= nwg;
}

template <int CP, int RPT>
static bool launch_fused_cols(int nwg, hipStream_t s, const double *P, int64_t ldp, const double *w, int64_t R, int H,
                              int B, double *ln_cur, double *ln_new, double *props_cur, mxm_em_state *state, double tol,
                              int max_iter, int chunk, double *zpart, int64_t ldz, double *cbuf, double *l1part,
                              fused_sync *sync) {
    if (!grid_fits(em_fused_cols_kernel<CP, RPT>, FCOLS_THREADS, nwg)) return false;
    hipLaunchKernelGGL((em_fused_cols_kernel<CP, RPT>), dim3(nwg), dim3(FCOLS_THREADS), 0, s, P, ldp, w, R, H, B, ln_cur,
                       ln_new, props_cur, state, tol, max_iter, chunk, zpart, ldz, cbuf, l1part, sync);
    return true;
}

template <int NCH>
static bool launch_fused(int nwg, hipStream_t s, const double *P, int64_t ldp, const double *w, int64_t R, int H, int B,
                         double *ln_cur, double *ln_new, double *props_cur, mxm_em_state *state, double tol,
                         int max_iter, int chunk, double *partial, int64_t ldpart, double *tbuf, fused_sync *sync) {
    if (!grid_fits(em_fused_loop_kernel<NCH, FUSED_NBUF>, FUSED_THREADS, nwg)) return false;
    hipLaunchKernelGGL((em_fused_loop_kernel<NCH, FUSED_NBUF>), dim3(nwg), dim3(FUSED_THREADS), 0, s, P, ldp, w, R, H, B, ln_cur,
                       ln_new, props_cur, state, tol, max_iter, chunk, partial, ldpart, tbuf, sync);
    return true;
}

template <int NCH>
static bool launch_fused_coded(int nwg, bool resident, hipStream_t s, const mxm_coded *c, int ldc, const double *w, int H, int B,
                               double *ln_cur, double *ln_new, double *props_cur, mxm_em_state *state, double tol,
                               int max_iter, int chunk, double *partial, int64_t ldpart, double *tbuf, fused_sync *sync) {
    if constexpr (NCH * FCODED_THREADS > 2048) {
        return false;
    } else {
        fcoded_args a;
        a.partial = partial; a.tbuf = tbuf; a.ln_cur = ln_cur; a.ln_new = ln_new; a.props_cur = props_cur;
        a.state = state; a.sync = sync; a.ldpart = ldpart; a.tol = tol; a.max_iter = max_iter; a.H = H;
        if (resident) {
            if (!grid_fits(em_fused_coded_kernel<NCH, 4, true>, FCODED_THREADS, nwg)) return false;
            hipLaunchKernelGGL((em_fused_coded_kernel<NCH, 4, true>), dim3(nwg), dim3(FCODED_THREADS), 0, s, c->rec, c->rec_off,
                               c->ndist, ldc, w, c->wide_rows, c->n_wide, c->R, B, chunk, a);
        } else {
            if (!grid_fits(em_fused_coded_kernel<NCH, 4, false>, FCODED_THREADS, nwg)) return false;
            hipLaunchKernelGGL((em_fused_coded_kernel<NCH, 4, false>), dim3(nwg), dim3(FCODED_THREADS), 0, s, c->rec, c->rec_off,
                               c->ndist, ldc, w, c->wide_rows, c->n_wide, c->R, B, chunk, a);
        }
        return true;
    }
}

// The one-launch loop of a narrow matrix (fused_narrow_kernels.hpp): grid and rows per thread, or 0 if it does not apply
// (more than 32 columns, more rows than the grid's registers hold).
static int fused_narrow_grid(int64_t R, int H, int *rpt_out) {
    if (H < 1 || H > 16 || R < 1) return 0;
    const int hmax = H <= 4 ? 4 : (H <= 8 ? 8 : 16);
    int cap = num_cu() < FNARROW_MAX_WG ? num_cu() : FNARROW_MAX_WG;          // one workgroup of 512 per CU
    const int nwg = clamp_grid((R + FNARROW_THREADS - 1) / FNARROW_THREADS, cap);
    const int64_t per = (R + (int64_t)nwg * FNARROW_THREADS - 1) / ((int64_t)nwg * FNARROW_THREADS);
    int rpt = 1;
    while (rpt < per) rpt *= 2;
    if (rpt * hmax > FNARROW_MAX_CELLS || (hmax == 16 && rpt > 1)) return 0;      // the instances that compile without scratch
    *rpt_out = rpt;
    return nwg;
}
static size_t fused_narrow_bytes(int H, int nwg) { return (size_t)2 * H * ((nwg + 7) & ~7) * sizeof(double); }

template <int HMAX, int RPT>
static bool launch_fused_narrow_one(int nwg, hipStream_t s, const double *M, int64_t ldm, const double *w, int64_t R, int H, int B,
                                    double *ln_cur, double *ln_new, double *props_cur, mxm_em_state *state, double tol,
                                    int max_iter, int chunk, double *partial, fused_sync *sync) {
    if constexpr (HMAX * RPT > FNARROW_MAX_CELLS || (HMAX == 16 && RPT > 1)) {
        return false;
    } else {
        if (!grid_fits(em_fused_narrow_kernel<HMAX, RPT>, FNARROW_THREADS, nwg)) return false;
        hipLaunchKernelGGL((em_fused_narrow_kernel<HMAX, RPT>), dim3(nwg), dim3(FNARROW_THREADS), 0, s, M, ldm, w, R, H, B, ln_cur,
                           ln_new, props_cur, state, tol, max_iter, chunk, partial, (nwg + 7) & ~7, sync);
        return true;
    }
}
static bool launch_fused_narrow(int nwg, int rpt, hipStream_t s, const double *M, int64_t ldm, const double *w, int64_t R, int H,
                                int B, double *ln_cur, double *ln_new, double *props_cur, mxm_em_state *state, double tol,
                                int max_iter, int chunk, double *partial, fused_sync *sync) {
    bool fits = false;
    auto columns = [&](auto hmax) {                      // rows per thread: 1, 2, 4 or 8
        (void)dispatch_width<8>(rpt, [&](auto k) {
            constexpr int HMAX = decltype(hmax)::value, RPT = decltype(k)::value;
            if constexpr ((RPT & (RPT - 1)) == 0)
                fits = launch_fused_narrow_one<HMAX, RPT>(nwg, s, M, ldm, w, R, H, B, ln_cur, ln_new, props_cur, state, tol, max_iter,
                                                          chunk, partial, sync);
        });
    };
    if (H <= 4) columns(std::integral_constant<int, 4>{});
    else if (H <= 8) columns(std::integral_constant<int, 8>{});
    else columns(std::integral_constant<int, 16>{});
    return fits;
}

// The form of the one-launch loop and the matrix it reads: records (`coded`), a narrow log-space matrix (M, ldm) or the
// linear matrix (P, ldp; rows or columns split over the workgroups, decided per launch).
enum class fused_route { none, records, narrow, dense };
struct fused_matrix {
    fused_route route;
    const mxm_coded *coded;
    const double *M;
    int64_t ldm;
    const double *P;
    int64_t ldp;
};

// the states of n restarts (samples), once the stream has got there
static int read_state(mxm_em_state *state_host, const mxm_em_state *state, int n, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(state_host, state, sizeof(mxm_em_state) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// The loop of every restart in [0, B) that is not done yet, in launches of at most `chunk` iterations
// per restart (one launch unless the caller wants to look at the state in between).
// Returns 0 when every restart has stopped; MXM_FUSED_GAVE_UP when a launch could not run to its end -- the grid does
// not fit the device, or its bounded grid barrier timed out because not all workgroups became resident (another
// process or stream holding CUs): the loop vectors and states are then back at their values from before that launch
// (snapshot at the tail of the workspace), so the caller can continue with the per-iteration kernels.
#define MXM_FUSED_GAVE_UP 1
static int em_loop_fused(const fused_matrix &m, const double *w, int64_t R, int32_t H, int32_t B, double *props_cur,
                         double *ln_cur, double *ln_new, mxm_em_state *state, double tol, int32_t max_iter, int32_t chunk,
                         void *ws, size_t ws_bytes, hipStream_t s, mxm_em_state *state_host) {
    const mxm_coded *coded = m.coded;
    const double *P = m.P;
    const int64_t ldp = m.ldp;
    // The persistent grid needs every workgroup resident, one per CU.  Two such grids in flight on one
    // device (two host threads, two streams) can each hold a part of the CUs and wait for the rest for
    // ever -- the bounded spins would end both after seconds.  Inside one process the launches are
    // therefore serialised here; across processes sharing a GPU nothing can (see the header).
    static std::mutex one_loop_at_a_time;
    std::lock_guard<std::mutex> guard(one_loop_at_a_time);
    int narrow_rpt = 1;
    const int nwg = m.route == fused_route::narrow    ? fused_narrow_grid(R, (int)H, &narrow_rpt)
                    : m.route == fused_route::records ? fused_coded_grid(coded->R)
                                                      : (num_cu() < MXM_MAX_WG ? num_cu() : MXM_MAX_WG);
    const int64_t ldpart = part_ld(H);
    char *base = static_cast<char *>(ws);
    fused_sync *sync = reinterpret_cast<fused_sync *>(base);
    double *tbuf = reinterpret_cast<double *>(base + fused_sync_bytes());
    double *partial = tbuf + 2 * ldpart;
    const int nch = ((H + 1) / 2 + FUSED_THREADS - 1) / FUSED_THREADS;
    const size_t vec = (size_t)B * H * sizeof(double);
    char *snap = base + ((ws_bytes - fused_snapshot_bytes(H, B)) & ~(size_t)255);
    auto snapshot = [&](bool save) -> hipError_t {
        double *vecs[3] = {props_cur, ln_cur, ln_new};
        for (int i = 0; i < 3; ++i) {
            const hipError_t e = save ? hipMemcpyAsync(snap + i * vec, vecs[i], vec, hipMemcpyDeviceToDevice, s)
                                      : hipMemcpyAsync(vecs[i], snap + i * vec, vec, hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return e;
        }
        return save ? hipMemcpyAsync(snap + 3 * vec, state, sizeof(mxm_em_state) * B, hipMemcpyDeviceToDevice, s)
                    : hipMemcpyAsync(state, snap + 3 * vec, sizeof(mxm_em_state) * B, hipMemcpyDeviceToDevice, s);
    };
    if (chunk < 1) chunk = 1;
    bool launched_once = false;
    for (;;) {
        RC_TRY(read_state(state_host, state, B, s));
        bool all_done = true, gave_up = false;
        for (int b = 0; b < B; ++b) {
            gave_up = gave_up || state_host[b].done < 0;
            all_done = all_done && state_host[b].done != 0;
        }
        if (gave_up) {
            // the grid barrier timed out: undo the launch (its vectors are mid-iteration) and hand back
            HIP_TRY(snapshot(false));
            RC_TRY(read_state(state_host, state, B, s));
            fail(-3, "mxm_em_loop: the one-launch loop's grid barrier timed out: not all %d workgroups became resident "
                     "(is another process or stream using the GPU?)", nwg);
            return MXM_FUSED_GAVE_UP;
        }
        if (launched_once && T.progress != nullptr) T.progress(state_host, B, T.progress_user);
        if (all_done) return 0;
        HIP_TRY(snapshot(true));
        HIP_TRY(hipMemsetAsync(sync, 0, fused_sync_bytes(), s));       // every polled word, before EVERY launch
        if (T.fused_force_abort)                                       // test hook: as if a workgroup had given up
            HIP_TRY(hipMemsetAsync(&sync->abort_[0], 1, sizeof(unsigned), s));
        bool fits = true;
        if (m.route == fused_route::narrow) {
            // narrow matrix: [sync][partial sums 2 x H x grid]; the rows live in registers for the whole launch
            fits = launch_fused_narrow(nwg, narrow_rpt, s, m.M, m.ldm, w, R, (int)H, (int)B, ln_cur, ln_new, props_cur,
                                       state, tol, (int)max_iter, (int)chunk, reinterpret_cast<double *>(base + fused_sync_bytes()), sync);
        } else if (m.route == fused_route::records) {
            // records: [sync][T (1 row)][partial rows]; the metadata of a workgroup's rows stays in LDS for the whole
            // launch when they fit its blocks (256 rows and 256 wide rows per workgroup)
            const int ldc = coded_ld(H);
            const int cnch = (ldc / 4 + FCODED_THREADS - 1) / FCODED_THREADS;
            const bool resident = (coded->R + nwg - 1) / nwg <= FCODED_THREADS && (coded->n_wide + nwg - 1) / nwg <= FCODED_THREADS;
            const bool ok = dispatch_width<8>(cnch, [&](auto n) {
                fits = launch_fused_coded<decltype(n)::value>(nwg, resident, s, coded, ldc, w, (int)H, (int)B, ln_cur, ln_new, props_cur,
                                                              state, tol, (int)max_iter, (int)chunk, partial, ldpart, tbuf, sync);
            });
            if (!ok) return fail(-1, "mxm_em_loop_coded: H=%d outside the one-launch loop's range", H);
        } else if (fused_cols_eligible(R, (int)H, nwg) && fused_cols_fits(R, (int)H, (int)B, nwg, ws_bytes)) {
            // smallest matrices: columns split over the workgroups, the matrix in registers (workspace:
            // [sync][z partials nwg x ldz][c ldz][l1 partials 2 x nwg]; checked against ws_bytes above)
            const int64_t ldz = (R + 1) & ~(int64_t)1;
            double *zpart = reinterpret_cast<double *>(base + fused_sync_bytes());
            double *cbuf = zpart + (int64_t)nwg * ldz;
            double *l1part = cbuf + ldz;
            const int cp = ((int)H + nwg - 1) / nwg;
            const int rpt = (int)((R + FCOLS_THREADS - 1) / FCOLS_THREADS);
            // instances: 12, 22 or 24 columns per workgroup x 1 .. 3 rows per thread (24 columns: at most 2)
            auto columns = [&](auto cpmax) {
                constexpr int CP = decltype(cpmax)::value, MAX_RPT = CP == 24 ? 2 : 3;
                (void)dispatch_width<MAX_RPT>(rpt < 1 ? 1 : (rpt > MAX_RPT ? MAX_RPT : rpt), [&](auto k) {
                    fits = launch_fused_cols<CP, decltype(k)::value>(nwg, s, P, ldp, w, R, (int)H, (int)B, ln_cur, ln_new, props_cur, state,
                                                                    tol, (int)max_iter, (int)chunk, zpart, ldz, cbuf, l1part, sync);
                });
            };
            if (cp <= 12) columns(std::integral_constant<int, 12>{});
            else if (cp <= 22) columns(std::integral_constant<int, 22>{});
            else columns(std::integral_constant<int, 24>{});
        } else {
            const bool ok = dispatch_width<FUSED_MAX_NCH>(nch, [&](auto n) {       // (the spill-free instances)
                fits = launch_fused<decltype(n)::value>(nwg, s, P, ldp, w, R, (int)H, (int)B, ln_cur, ln_new, props_cur, state, tol,
                                                        (int)max_iter, (int)chunk, partial, ldpart, tbuf, sync);
            });
            if (!ok) return fail(-1, "mxm_em_loop: H=%d outside the one-launch loop's range", H);
        }
        if (!fits) {
            fail(-3, "mxm_em_loop: the one-launch loop's %d workgroups cannot be co-resident on this device", nwg);
            return MXM_FUSED_GAVE_UP;                                  // nothing was launched, nothing to undo
        }
        HIP_TRY(hipGetLastError());
        launched_once = true;
    }
}

// One iteration of the restarts named by `tile` (nb <= the restart tile): E+M pass, column reduce,
// finalize.  Linear fp64 matrices share the pass; the other paths (fp32 storage, log-space kernels)
// run one restart per pass through pointers offset to that restart.
static int enqueue_tile_iteration(const double *M, int64_t ldm, const double *P, int64_t ldp, const double *w,
                                  int64_t R, int32_t H, const mxm_slots &tile, int nb, double *props_cur,
                                  double *ln_cur, double *ln_new, double *colsum, mxm_em_state *state, double tol,
                                  int32_t max_iter, void *ws, size_t ws_bytes, hipStream_t s, bool p_is_f32,
                                  bool timed, const mxm_coded *coded) {
    const bool linear = !p_is_f32 && P != nullptr && mxm_linear_supported(H);
    // records and the linear fp64 matrix: the finalize rides on the column reduce's launch (one ticket per restart)
    fin_args fin = {ln_cur, ln_new, props_cur, state, tol, (int)max_iter};
    if (coded != nullptr) {
        if (nb == QB_BT && coded_batch_ok(coded, (int)H))
            return em_iter_coded_batched(coded, w, props_cur, (int)H, tile, state, colsum, (double *)ws, s, timed, &fin);
        for (int i = 0; i < nb; ++i) {
            RC_TRY(em_iter_coded_one(coded, w, props_cur, (int)H, tile.s[i], state, colsum, (double *)ws, s, timed && i == 0, &fin));
        }
        return 0;
    } else if (linear) {
        return em_iter_linear_tile(P, ldp, w, props_cur, R, (int)H, nb, tile, state, colsum, (double *)ws, s, timed, &fin);
    } else {
        for (int i = 0; i < nb; ++i) {
            const int64_t off = (int64_t)tile.s[i] * H;
            const int rc = p_is_f32 ? mxm_em_iter_f32(reinterpret_cast<const float *>(P), ldp, w, props_cur + off, R, H, 1,
                                                      state + tile.s[i], colsum + off, ws, ws_bytes, s)
                                    : mxm_em_iter(M, ldm, P, ldp, w, props_cur + off, ln_cur + off, R, H, 1,
                                                  state + tile.s[i], colsum + off, ws, ws_bytes, s);
            if (rc != 0) return rc;
        }
    }
    if (H > 64 * FIN_MAX_BLOCKS)
        hipLaunchKernelGGL(finalize_any_kernel, dim3(1, nb), dim3(FIN_THREADS), 0, s, colsum, ln_cur, ln_new, props_cur, (int)H, tol,
                           (int)max_iter, state, 0, 1, tile);
    else
        hipLaunchKernelGGL(finalize_kernel, dim3((H + FIN_THREADS - 1) / FIN_THREADS, nb), dim3(FIN_THREADS), 0, s, colsum, ln_cur,
                           ln_new, props_cur, (int)H, tol, (int)max_iter, state, 0, 1, tile);
    HIP_TRY(hipGetLastError());
    return 0;
}

// mxm_coded's contract, checked once by the loops over records (they block anyway; the one-launch loop has no room for
// the in-kernel check the per-iteration kernel carries): wide_rows lists exactly the rows with 16-bit codes -- the loops
// skip those in their main pass and take them from the list -- and, with_quads, quad_rows / byte_rows the rows with /
// without quads.  The quad lists are looked at only when the wide list is sound.  `scratch`: two device words.
static int records_lists_check(const mxm_coded *c, const char *who, void *scratch, hipStream_t s, bool with_quads) {
    unsigned long long *chk = static_cast<unsigned long long *>(scratch), host[2] = {0, 0};
    const dim3 grid(clamp_grid((c->R + 255) / 256, num_cu() * 4));
    auto faults_of = [&](auto launch) -> int {          // host[] = what the kernel `launch` enqueues left in chk[]
        HIP_TRY(hipMemsetAsync(chk, 0, sizeof(host), s));
        launch();
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, chk, sizeof(host), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return 0;
    };
    RC_TRY(faults_of([&] {
        hipLaunchKernelGGL(coded_validate_kernel, grid, dim3(256), 0, s, c->ndist, c->R, c->wide_rows, c->n_wide, chk);
    }));
    if (host[1] != 0 || (long long)host[0] != (long long)c->n_wide)
        return fail(-1, "%s: wide_rows must list exactly the rows with more than 256 values, ascending (%lld such rows, n_wide = %lld)",
                    who, (long long)host[0], (long long)c->n_wide);
    if (!with_quads) return 0;
    RC_TRY(faults_of([&] {
        hipLaunchKernelGGL(quad_validate_kernel, grid, dim3(256), 0, s, c->ndist, c->nquad, c->R, c->quad_rows, c->n_quad_rows,
                           c->byte_rows, c->n_byte_rows, chk);
    }));
    if (host[1] != 0) return fail(-1, "%s: quad_rows / byte_rows must list the rows with / without quads, ascending", who);
    return 0;
}

// What the per-iteration loop owns: its private stream, the event that orders it against the caller's, and the captured
// chunk.  Released in this order: graph exec, graph, the stream (once it has drained), the event.
struct loop_resources {
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    loop_resources() = default;
    loop_resources(const loop_resources &) = delete;
    loop_resources &operator=(const loop_resources &) = delete;
    void drop_graph() {
        if (exec != nullptr) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
        if (graph != nullptr) { (void)hipGraphDestroy(graph); graph = nullptr; }
    }
    ~loop_resources() {
        drop_graph();
        if (s != nullptr) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        if (ev != nullptr) (void)hipEventDestroy(ev);
    }
};

static int em_loop_impl(const double *M, int64_t ldm, const double *P, int64_t ldp, const double *w,
                        int64_t R, int32_t H, int32_t B, double *props_cur, double *ln_cur, double *ln_new,
                        double *colsum, mxm_em_state *state, double tol, int32_t max_iter,
                        int32_t check_every, void *ws, size_t ws_bytes, void *stream,
                        mxm_em_state *state_host, bool p_is_f32, const mxm_coded *coded = nullptr) {
    if (state_host == nullptr || state == nullptr) return fail(-1, "mxm_em_loop: state pointers required");
    if (R <= 0 || H <= 0 || B <= 0) return fail(-1, "mxm_em_loop: bad shape R=%lld H=%d", (long long)R, H);
    if (ws == nullptr || ws_bytes < mxm_workspace_bytes(R, H, B)) return fail(-1, "mxm_em_loop: workspace too small");
    if (check_every < 1) check_every = 1;
    if (T.progress != nullptr && check_every > T.progress_every) check_every = T.progress_every;
    hipStream_t caller = (hipStream_t)stream;
    (void)num_cu();                                    // device query outside any capture
    RC_TRY(read_state(state_host, state, B, caller));
    int running = 0;
    for (int b = 0; b < B; ++b) running += (state_host[b].done == 0) ? 1 : 0;
    // The whole loop in persistent launches on the caller's stream (the host only waits; nothing is decided between
    // iterations), where one of its forms applies:
    //   records  restarts one after another over the records
    //   narrow   the refinement EM on the contributors' columns: restarts one after another, the rows in registers
    //   dense    a cache-resident linear matrix
    fused_matrix fm = {fused_route::none, coded, M, ldm, P, ldp};
    if (coded != nullptr && running > 0 && max_iter > 0 && fused_coded_eligible(coded, (int)H, (int)B, ws_bytes, running)) {
        fm.route = fused_route::records;
    } else if (int nrpt = 0; !p_is_f32 && coded == nullptr && M != nullptr && T.loop_fused != 0 && running > 0 && max_iter > 0 &&
                            !(P != nullptr && mxm_linear_supported(H)) && fused_narrow_grid(R, (int)H, &nrpt) > 0 &&
                            ws_bytes >= fused_sync_bytes() + fused_narrow_bytes((int)H, FNARROW_MAX_WG) + fused_snapshot_bytes(H, B) + 256) {
        fm.route = fused_route::narrow;
    } else if (fused_eligible(P, ldp, R, (int)H, (int)B, ws_bytes, p_is_f32, running)) {
        fm.route = fused_route::dense;
    }
    if (fm.route != fused_route::none) {
        int chunk = T.fused_chunk > 0 ? T.fused_chunk : max_iter;
        if (T.progress != nullptr && chunk > T.progress_every) chunk = T.progress_every;     // someone is watching
        if (fm.route == fused_route::records) {
            // a launch is kept to about half a second (a 10^7-row matrix takes 15 ms per iteration)
            const double est_us = (double)R * ((double)coded_ld(H) + 400.0) / 4.0e6 + 20.0;
            const int cap = (int)std::max(8.0, 5.0e5 / est_us);
            if (chunk > cap) chunk = cap;
        }
        const int frc = em_loop_fused(fm, w, R, H, B, props_cur, ln_cur, ln_new, state, tol, max_iter, chunk, ws, ws_bytes, caller,
                                      state_host);
        // Gave up (grid not co-resident / starved): only mxm_set_loop_fused(1, ...) -- "whenever the shape allows" --
        // makes that an error; by default the same call goes on through the per-iteration kernels from the restored
        // state (another summation order: rounding-level differences, same stopping rule).
        if (frc != MXM_FUSED_GAVE_UP) return frc;
        if (T.loop_fused == 1) return -3;
    }
    const bool want_graph = T.loop_graph == 1 ||
                            (T.loop_graph == -1 && (double)R * (double)H * (double)B < 6.4e7);
    int window = T.max_bt;                             // the largest restart tile that fits (mxm_em_iter)
    if (p_is_f32 || P == nullptr || !mxm_linear_supported(H)) window = 1;
    while (window > 1 && !batch_fits((int)H, window)) --window;
    if (coded != nullptr && coded_batch_ok(coded, (int)H)) window = QB_BT;     // records beside a quad dictionary: tiles of three

    // the loop runs on a private stream (the caller's may be the legacy default stream, which
    // cannot be captured); it is ordered after / before the caller's stream with events
    loop_resources own;
    HIP_TRY(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&own.ev, hipEventDisableTiming));
    const hipStream_t s = own.s;
    const hipEvent_t ev = own.ev;
    std::vector<int> graph_key;
    // Restarts stop on different iterations, and a pass over the matrix costs nearly the same for one
    // restart as for a full tile.  Schedules (mxm_set_compact_restarts):
    //   0  every restart in every iteration, static tiles over all B (a tile idles once all its members stopped)
    //   1  tiles over the restarts still running, spread evenly (10 -> 4 + 3 + 3)
    //   2  ONE full tile per iteration, dealt round-robin over the running restarts chunk by chunk: every
    //      pass carries a full tile until fewer than a tile's worth are left, and all restarts advance at
    //      the same rate, so they also finish together (no half-empty tail generation).
    // A tile names its restarts by index (mxm_slots, by value): nothing is moved in memory.  Each restart
    // counts its own iterations (finalize_kernel), so when it is scheduled changes nothing in its result.
    std::vector<int> order;                            // unfinished restarts, round-robin order
    HIP_TRY(hipEventRecord(ev, caller));
    HIP_TRY(hipStreamWaitEvent(s, ev, 0));
    RC_TRY(read_state(state_host, state, B, s));
    for (int b = 0; b < B; ++b)
        if (state_host[b].done == 0) order.push_back(b);
    if (max_iter <= 0) order.clear();
    while (!order.empty()) {
        // the tiles of this chunk: flat list of restart indices + tile sizes
        std::vector<int> members, sizes;
        // (with one restart per pass every schedule costs the same: no rotation, the tile list then only
        // changes when a restart stops and a captured graph stays valid in between)
        const bool rotating = T.compact_restarts == 2 && window > 1 && (int)order.size() > window;
        if (rotating) {
            members.assign(order.begin(), order.begin() + window);
            sizes.push_back(window);
            std::rotate(order.begin(), order.begin() + window, order.end());       // they go to the back of the queue
        } else {
            std::vector<int> all;
            if (T.compact_restarts == 0) { for (int b = 0; b < B; ++b) all.push_back(b); }
            else all = order;
            for (size_t at = 0; at < all.size();) {
                // the fewest passes that cover what is left, restarts spread evenly over them
                const int left = (int)(all.size() - at);
                const int passes = (left + window - 1) / window;
                // (records: only a FULL tile shares a pass -- 4 left are 3 + 1, not 2 + 2)
                const int nb = coded != nullptr ? (left < window ? left : window) : (left + passes - 1) / passes;
                members.insert(members.end(), all.begin() + at, all.begin() + at + nb);
                sizes.push_back(nb);
                at += nb;
            }
        }
        // finalize stops each restart at its own max_iter and kernels of a stopped restart are no-ops -- but a pass that
        // several restarts share costs the same with a stopped member in it: a chunk ends where its first member reaches
        // max_iter (what converges on the way cannot be known beforehand)
        int64_t n = check_every;
        for (int b : members) {
            const int64_t left = (int64_t)max_iter - (int64_t)state_host[b].iters;
            if (left > 0 && left < n) n = left;
        }
        auto enqueue_chunk = [&]() -> int {
            for (int64_t it = 0; it < n; ++it) {
                size_t at = 0;
                for (size_t ti = 0; ti < sizes.size(); ++ti) {
                    mxm_slots tile;
                    for (int i = 0; i < MXM_MAX_BT; ++i) tile.s[i] = members[at + (i < sizes[ti] ? i : 0)];
                    const int erc = enqueue_tile_iteration(M, ldm, P, ldp, w, R, H, tile, sizes[ti], props_cur, ln_cur,
                                                           ln_new, colsum, state, tol, max_iter, ws, ws_bytes, s,
                                                           p_is_f32, ti == 0, coded);
                    if (erc != 0) return erc;
                    at += sizes[ti];
                }
            }
            return 0;
        };
        bool launched = false;
        if (want_graph && !rotating) {                 // a rotating tile list would be re-captured every chunk
            std::vector<int> key(members);
            key.insert(key.end(), sizes.begin(), sizes.end());
            key.push_back((int)n);
            if (own.exec == nullptr || key != graph_key) {
                own.drop_graph();
                if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                    const int crc = enqueue_chunk();
                    const hipError_t ee = hipStreamEndCapture(s, &own.graph);
                    if (crc == 0 && ee == hipSuccess && hipGraphInstantiate(&own.exec, own.graph, nullptr, nullptr, 0) == hipSuccess) {
                        graph_key = key;
                    } else {
                        own.exec = nullptr;            // capture unavailable: plain launches below
                        (void)hipGetLastError();
                    }
                }
            }
            if (own.exec != nullptr) {
                HIP_TRY(hipGraphLaunch(own.exec, s));
                launched = true;
            }
        }
        if (!launched) RC_TRY(enqueue_chunk());
        RC_TRY(read_state(state_host, state, B, s));
        for (int b = 0; b < B; ++b)
            if (state_host[b].error != 0)
                return fail(-1, "mxm_em_loop: the records' wide_rows list does not match the rows with more than 256 values");
        if (T.progress != nullptr) T.progress(state_host, B, T.progress_user);
        std::vector<int> still;
        for (int b : order)
            if (state_host[b].done == 0) still.push_back(b);
        order.swap(still);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev, s));
    HIP_TRY(hipStreamWaitEvent(caller, ev, 0));
    return 0;                                          // (`own` goes: exec, graph, the stream once it has drained, the event)
}

extern "C" int mxm_em_loop(const double *M, int64_t ldm, const double *P, int64_t ldp, const double *w,
                           int64_t R, int32_t H, int32_t B, double *props_cur, double *ln_cur, double *ln_new,
                           double *colsum, mxm_em_state *state, double tol, int32_t max_iter,
                           int32_t check_every, void *ws, size_t ws_bytes, void *stream,
                           mxm_em_state *state_host) {
    MXM_ENTER();
    return em_loop_impl(M, ldm, P, ldp, w, R, H, B, props_cur, ln_cur, ln_new, colsum, state, tol, max_iter,
                        check_every, ws, ws_bytes, stream, state_host, false);
}

extern "C" int mxm_em_loop_coded(const mxm_coded *c, const double *w, int32_t H, int32_t B, double *props_cur,
                                 double *ln_cur, double *ln_new, double *colsum, mxm_em_state *state, double tol,
                                 int32_t max_iter, int32_t check_every, void *ws, size_t ws_bytes, void *stream,
                                 mxm_em_state *state_host) {
    MXM_ENTER();
    RC_TRY(coded_check(c, H, "mxm_em_loop_coded"));
    if (ws == nullptr || ws_bytes < mxm_workspace_bytes(c->R, H, B)) return fail(-1, "mxm_em_loop_coded: workspace too small");
    RC_TRY(records_lists_check(c, "mxm_em_loop_coded", ws, (hipStream_t)stream, c->qrec != nullptr));
    return em_loop_impl(nullptr, 0, nullptr, 0, w, c->R, H, B, props_cur, ln_cur, ln_new, colsum, state, tol, max_iter,
                        check_every, ws, ws_bytes, stream, state_host, false, c);
}

// ---- the EM loops of many samples in one batched pass (samples_kernels.hpp) ------------------------------------------
extern "C" int mxm_samples_tile_rows(void) { return MXM_SAMPLES_TILE_ROWS; }

extern "C" int64_t mxm_samples_plan(const int64_t *row0_host, int32_t S, mxm_sample_tile *tiles_host, int64_t cap,
                                    int32_t *tile0_host) {
    if (row0_host == nullptr || S < 1) return fail(-1, "mxm_samples_plan: bad arguments (S=%d)", S);
    if (row0_host[0] != 0) return fail(-1, "mxm_samples_plan: row0[0] must be 0 (it is %lld)", (long long)row0_host[0]);
    constexpr int64_t K = MXM_SAMPLES_TILE_ROWS;
    int64_t n = 0;
    for (int32_t s = 0; s < S; ++s) {
        const int64_t rows = row0_host[s + 1] - row0_host[s];
        if (rows <= 0)
            return fail(-1, "mxm_samples_plan: row0 must ascend and no sample may be empty (sample %d has %lld rows)", s, (long long)rows);
        if (tile0_host != nullptr) tile0_host[s] = (int32_t)n;
        const int64_t nt = (rows + K - 1) / K;
        if (n + nt > 0x7fffffffll) return fail(-1, "mxm_samples_plan: more than 2^31 - 1 tiles");
        if (tiles_host != nullptr) {
            if (n + nt > cap) return fail(-1, "mxm_samples_plan: room for %lld tiles, sample %d needs more", (long long)cap, s);
            for (int64_t i = 0; i < nt; ++i) {
                const int64_t left = rows - i * K;
                tiles_host[n + i] = mxm_sample_tile{s, (int32_t)(left < K ? left : K), row0_host[s] + i * K};
            }
        }
        n += nt;
    }
    if (tile0_host != nullptr) tile0_host[S] = (int32_t)n;
    return n;
}

// scratch layout: [tile table][first tile of every sample, S + 1][fault word per tile][partial rows, one per tile]
struct samples_ws {
    mxm_sample_tile *tiles;
    int32_t *tile0;
    int *chk;
    double *partial;
    size_t bytes;
};
static samples_ws samples_layout(void *ws, int64_t n_tiles, int S, int H) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    samples_ws L;
    char *base = static_cast<char *>(ws);
    size_t at = 0;
    L.tiles = reinterpret_cast<mxm_sample_tile *>(base + at);
    at += up((size_t)n_tiles * sizeof(mxm_sample_tile));
    L.tile0 = reinterpret_cast<int32_t *>(base + at);
    at += up((size_t)(S + 1) * sizeof(int32_t));
    L.chk = reinterpret_cast<int *>(base + at);
    at += up((size_t)n_tiles * sizeof(int));
    L.partial = reinterpret_cast<double *>(base + at);
    at += (size_t)n_tiles * (size_t)part_ld(H) * sizeof(double);
    L.bytes = at;
    return L;
}
extern "C" size_t mxm_samples_workspace_bytes(int64_t n_tiles, int32_t S, int32_t H) {
    if (n_tiles <= 0 || S <= 0 || H <= 0) return 0;
    return samples_layout(nullptr, n_tiles, (int)S, (int)H).bytes;
}

// Everything the two entry points refuse before they touch the device; *n_tiles_out = the plan's size.
// has_width false: an entry that reads no record and so takes no H (mxm_bootstrap_weights).
static int samples_check(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const char *who, int64_t *n_tiles_out,
                         bool has_width = true) {
    if (c == nullptr || row0_host == nullptr || S < 1 || S > 65535)
        return fail(-1, "%s: bad arguments (S = %d; 1 .. 65535 samples)", who, S);
    if (c->R <= 0 || c->rec == nullptr || c->rec_off == nullptr || c->ndist == nullptr)
        return fail(-1, "%s: coded matrix arrays missing (rows %lld)", who, (long long)c->R);
    if (has_width && ((H & 1) != 0 || H < 66 || H > 8192)) return fail(-1, "%s: H = %d: an even width in [66, 8192] is required", who, H);
    if (c->qrec != nullptr) return fail(-1, "%s: a quad dictionary is attached; the batched pass reads the records only", who);
    if (c->R_rest != 0) return fail(-1, "%s: %lld rows without a record (the dense rest): such a sample runs on its own", who, (long long)c->R_rest);
    if (c->n_wide < 0 || (c->n_wide > 0 && c->wide_rows == nullptr)) return fail(-1, "%s: n_wide > 0 needs wide_rows", who);
    const int64_t n_tiles = mxm_samples_plan(row0_host, S, nullptr, 0, nullptr);
    if (n_tiles < 0) return -1;                           // (the plan's message stands)
    if (row0_host[S] != c->R) return fail(-1, "%s: row0[S] = %lld, the matrix has %lld rows", who, (long long)row0_host[S], (long long)c->R);
    *n_tiles_out = n_tiles;
    return 0;
}

// the plan into the workspace, ordered on `stream` (from pageable memory: the runtime has taken the bytes when the call returns)
static int samples_upload_plan(const int64_t *row0_host, int S, int64_t n_tiles, const samples_ws &L, hipStream_t stream) {
    static thread_local std::vector<mxm_sample_tile> tiles;
    static thread_local std::vector<int32_t> tile0;
    tiles.resize((size_t)n_tiles);
    tile0.resize((size_t)S + 1);
    if (mxm_samples_plan(row0_host, S, tiles.data(), n_tiles, tile0.data()) != n_tiles) return -1;
    HIP_TRY(hipMemcpyAsync(L.tiles, tiles.data(), (size_t)n_tiles * sizeof(mxm_sample_tile), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(L.tile0, tile0.data(), ((size_t)S + 1) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    return 0;
}

// one pass for every unfinished sample: the tiles, then each sample's column reduce
static int samples_enqueue_pass(const mxm_coded *c, const double *w, const double *props, int H, int S, int64_t n_tiles,
                                const samples_ws &L, mxm_em_state *state, double *colsum, hipStream_t stream) {
    const int ldc = coded_ld(H);
    const int nch = (ldc / 4 + SAMPLES_THREADS - 1) / SAMPLES_THREADS;
    const int64_t ldpart = part_ld(H);
    const bool ok = dispatch_width<8>(nch, [&](auto n) {
        hipLaunchKernelGGL((em_iter_samples_kernel<decltype(n)::value, 4>), dim3((unsigned)n_tiles), dim3(SAMPLES_THREADS), 0, stream, c->rec,
                           c->rec_off, c->ndist, ldc, w, props, H, (const mxm_sample_tile *)L.tiles, L.partial, ldpart, L.chk,
                           (const mxm_em_state *)state);
    });
    if (!ok) return fail(-1, "mxm_em_iter_samples: H=%d outside the kernel's range", H);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(samples_colreduce_kernel, dim3((H + SAMPLES_COLRED_THREADS - 1) / SAMPLES_COLRED_THREADS, S),
                       dim3(SAMPLES_COLRED_THREADS), 0, stream, (const double *)L.partial, ldpart, (const int32_t *)L.tile0,
                       (const int *)L.chk, H, colsum, state);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_em_iter_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, const double *w, const double *props,
                                   int32_t H, mxm_em_state *state, double *colsum, void *ws, size_t ws_bytes, void *stream) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_em_iter_samples", &n_tiles));
    if (props == nullptr || colsum == nullptr || state == nullptr) return fail(-1, "mxm_em_iter_samples: bad arguments");
    if (ws == nullptr || ws_bytes < mxm_samples_workspace_bytes(n_tiles, S, H) || (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(-1, "mxm_em_iter_samples: workspace too small (or not 16-byte aligned)");
    const samples_ws L = samples_layout(ws, n_tiles, (int)S, (int)H);
    RC_TRY(samples_upload_plan(row0_host, (int)S, n_tiles, L, (hipStream_t)stream));
    return samples_enqueue_pass(c, w, props, (int)H, (int)S, n_tiles, L, state, colsum, (hipStream_t)stream);
}

extern "C" int mxm_em_loop_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, const double *w, int32_t H,
                                   double *props_cur, double *ln_cur, double *ln_new, double *colsum, mxm_em_state *state,
                                   double tol, int32_t max_iter, int32_t check_every, void *ws, size_t ws_bytes, void *stream,
                                   mxm_em_state *state_host) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_em_loop_samples", &n_tiles));
    if (props_cur == nullptr || ln_cur == nullptr || ln_new == nullptr || colsum == nullptr || state == nullptr || state_host == nullptr)
        return fail(-1, "mxm_em_loop_samples: bad arguments");
    if (ws == nullptr || ws_bytes < mxm_samples_workspace_bytes(n_tiles, S, H) || (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(-1, "mxm_em_loop_samples: workspace too small (or not 16-byte aligned)");
    if (check_every < 1) check_every = 1;
    if (T.progress != nullptr && check_every > T.progress_every) check_every = T.progress_every;
    hipStream_t s = (hipStream_t)stream;
    const samples_ws L = samples_layout(ws, n_tiles, (int)S, (int)H);
    RC_TRY(records_lists_check(c, "mxm_em_loop_samples", L.partial, s, false));
    RC_TRY(samples_upload_plan(row0_host, (int)S, n_tiles, L, s));
    RC_TRY(read_state(state_host, state, S, s));
    auto running = [&]() {
        int n = 0;
        for (int b = 0; b < S; ++b) n += (state_host[b].done == 0) ? 1 : 0;
        return n;
    };
    while (max_iter > 0 && running() > 0) {
        // a chunk ends where its first unfinished sample reaches max_iter at the latest (kernels of a finished sample are
        // no-ops, so running past a sample's stop changes nothing -- it only costs launches)
        int64_t n = check_every, most_left = 0;
        for (int b = 0; b < S; ++b)
            if (state_host[b].done == 0) most_left = std::max<int64_t>(most_left, (int64_t)max_iter - state_host[b].iters);
        if (most_left > 0 && most_left < n) n = most_left;
        for (int64_t it = 0; it < n; ++it) {
            RC_TRY(samples_enqueue_pass(c, w, props_cur, (int)H, (int)S, n_tiles, L, state, colsum, s));
            RC_TRY(mxm_m_finalize(colsum, ln_cur, ln_new, props_cur, H, S, tol, max_iter, state, s));
        }
        RC_TRY(read_state(state_host, state, S, s));
        for (int b = 0; b < S; ++b)
            if (state_host[b].error != 0)
                return fail(-1, "mxm_em_loop_samples: sample %d has a row without a record (ndist outside 1 .. 1024)", b);
        if (T.progress != nullptr) T.progress(state_host, S, T.progress_user);
    }
    return 0;
}

// ---- the second half of a cohort run: votes, column gather, refinement EM, read assignment (samples_finish_kernels.hpp) ----
// scratch layout: [tile table][row0, S + 1][cols, S x ld][ncol, S][perm, S x ld]
struct finish_ws {
    mxm_sample_tile *tiles;
    int64_t *row0;
    int32_t *cols, *ncol, *perm;
    size_t bytes;
};
static finish_ws finish_layout(void *ws, int64_t n_tiles, int S, int ld) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    finish_ws L;
    char *base = static_cast<char *>(ws);
    size_t at = 0;
    L.tiles = reinterpret_cast<mxm_sample_tile *>(base + at);
    at += up((size_t)n_tiles * sizeof(mxm_sample_tile));
    L.row0 = reinterpret_cast<int64_t *>(base + at);
    at += up((size_t)(S + 1) * sizeof(int64_t));
    L.cols = reinterpret_cast<int32_t *>(base + at);
    at += up((size_t)S * ld * sizeof(int32_t));
    L.ncol = reinterpret_cast<int32_t *>(base + at);
    at += up((size_t)S * sizeof(int32_t));
    L.perm = reinterpret_cast<int32_t *>(base + at);
    at += up((size_t)S * ld * sizeof(int32_t));
    L.bytes = at;
    return L;
}
extern "C" size_t mxm_samples_finish_workspace_bytes(int64_t n_tiles, int32_t S, int32_t ld) {
    if (n_tiles <= 0 || S <= 0 || ld < 0) return 0;
    return finish_layout(nullptr, n_tiles, (int)S, (int)ld).bytes;
}

// What the four entry points refuse beyond samples_check: the reduced matrix's stride and every sample's column count
// (cols_host / perm_host nullable: the entry does not take them).
static int finish_cols_check(const char *who, int32_t S, int32_t H, int32_t ld, const int32_t *ncol_host, const int32_t *cols_host,
                             const int32_t *perm_host) {
    if (ld != 4 && ld != 8 && ld != 16) return fail(-1, "%s: ld = %d: the reduced matrix's row stride must be 4, 8 or 16", who, ld);
    if (ncol_host == nullptr) return fail(-1, "%s: bad arguments (ncol_host missing)", who);
    for (int32_t s = 0; s < S; ++s) {
        const int32_t k = ncol_host[s];
        if (k < 0 || k > ld) return fail(-1, "%s: sample %d has ncol = %d outside [0, %d]", who, s, k, ld);
        for (int32_t i = 0; i < k; ++i) {
            if (cols_host != nullptr && (cols_host[(int64_t)s * ld + i] < 0 || cols_host[(int64_t)s * ld + i] >= H))
                return fail(-1, "%s: sample %d, column %d: haplogroup index %d outside [0, %d)", who, s, i,
                            cols_host[(int64_t)s * ld + i], H);
            if (perm_host != nullptr && (perm_host[(int64_t)s * ld + i] < 0 || perm_host[(int64_t)s * ld + i] >= k))
                return fail(-1, "%s: sample %d, column %d: contributor ordinal %d outside [0, %d)", who, s, i,
                            perm_host[(int64_t)s * ld + i], k);
        }
    }
    return 0;
}

static int finish_ws_check(const char *who, const void *ws, size_t ws_bytes, int64_t n_tiles, int32_t S, int32_t ld) {
    if (ws == nullptr || ws_bytes < mxm_samples_finish_workspace_bytes(n_tiles, S, ld) || (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(-1, "%s: workspace too small (or not 16-byte aligned)", who);
    return 0;
}

// the plan and the per-sample tables into the workspace, ordered on `stream`.  The caller's tables go through vectors of
// the call's own, as the tiles do: from pageable memory the runtime has taken the bytes when hipMemcpyAsync returns
// (without waiting for the stream: tests/test_gpu_stream_contract.py), from a caller's PINNED array it would read them
// whenever the stream gets there, after the caller may have changed them.
static int finish_upload(const int64_t *row0_host, int S, int64_t n_tiles, int ld, const int32_t *ncol_host, const int32_t *cols_host,
                         const int32_t *perm_host, const finish_ws &L, hipStream_t stream) {
    static thread_local std::vector<mxm_sample_tile> tiles;
    static thread_local std::vector<int64_t> row0;
    static thread_local std::vector<int32_t> ncol, cols, perm;
    tiles.resize((size_t)n_tiles);
    if (mxm_samples_plan(row0_host, S, tiles.data(), n_tiles, nullptr) != n_tiles) return -1;
    HIP_TRY(hipMemcpyAsync(L.tiles, tiles.data(), (size_t)n_tiles * sizeof(mxm_sample_tile), hipMemcpyHostToDevice, stream));
    row0.assign(row0_host, row0_host + (size_t)S + 1);
    HIP_TRY(hipMemcpyAsync(L.row0, row0.data(), row0.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream));
    if (ncol_host != nullptr) {
        ncol.assign(ncol_host, ncol_host + (size_t)S);
        HIP_TRY(hipMemcpyAsync(L.ncol, ncol.data(), ncol.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    }
    if (cols_host != nullptr) {
        cols.assign(cols_host, cols_host + (size_t)S * ld);
        HIP_TRY(hipMemcpyAsync(L.cols, cols.data(), cols.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    }
    if (perm_host != nullptr) {
        perm.assign(perm_host, perm_host + (size_t)S * ld);
        HIP_TRY(hipMemcpyAsync(L.perm, perm.data(), perm.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    }
    return 0;
}

extern "C" int mxm_votes_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const double *w,
                                 const double *ln_props, const double *props, const double *rowmax, int32_t *best, double *votes,
                                 int64_t *counts, int64_t *first, double *lse, mxm_em_state *state, void *ws, size_t ws_bytes,
                                 void *stream) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_votes_samples", &n_tiles));
    if (ln_props == nullptr || best == nullptr || votes == nullptr || first == nullptr)
        return fail(-1, "mxm_votes_samples: bad arguments (ln_props, best, votes and first are required)");
    if (lse != nullptr && (props == nullptr || rowmax == nullptr))
        return fail(-1, "mxm_votes_samples: lse needs props and rowmax (the row normaliser's own variables)");
    RC_TRY(finish_ws_check("mxm_votes_samples", ws, ws_bytes, n_tiles, S, 0));
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, 0);
    const size_t vlds = (size_t)H * (sizeof(double) + 2 * sizeof(int));
    RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&votes_sum_samples_kernel), vlds, "votes_sum_samples_kernel",
                          "mxm_votes_samples", H, "too wide for the vote kernel"));
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, 0, nullptr, nullptr, nullptr, L, s));
    const int ldc = coded_ld(H);
    if (lse != nullptr)
        hipLaunchKernelGGL((votes_best_samples_kernel<true>), dim3((unsigned)n_tiles), dim3(SFIN_THREADS), 0, s, c->rec, c->rec_off,
                           c->ndist, ldc, (int)H, (const mxm_sample_tile *)L.tiles, ln_props, props, rowmax, best, lse);
    else
        hipLaunchKernelGGL((votes_best_samples_kernel<false>), dim3((unsigned)n_tiles), dim3(SFIN_THREADS), 0, s, c->rec, c->rec_off,
                           c->ndist, ldc, (int)H, (const mxm_sample_tile *)L.tiles, ln_props, props, rowmax, best, lse);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(votes_sum_samples_kernel, dim3((unsigned)S), dim3(SFIN_THREADS), vlds, s, (const int32_t *)best, w,
                       (const int64_t *)L.row0, (int)H, votes, counts, first, state);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_gather_columns_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H,
                                          const int32_t *cols_host, const int32_t *ncol_host, int32_t ld, double *out, void *ws,
                                          size_t ws_bytes, void *stream) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_gather_columns_samples", &n_tiles));
    if (cols_host == nullptr || out == nullptr) return fail(-1, "mxm_gather_columns_samples: bad arguments");
    RC_TRY(finish_cols_check("mxm_gather_columns_samples", S, H, ld, ncol_host, cols_host, nullptr));
    RC_TRY(finish_ws_check("mxm_gather_columns_samples", ws, ws_bytes, n_tiles, S, ld));
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, (int)ld);
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, (int)ld, ncol_host, cols_host, nullptr, L, s));
    hipLaunchKernelGGL(gather_samples_kernel, dim3((unsigned)n_tiles), dim3(SFIN_THREADS), 0, s, c->rec, c->rec_off, c->ndist,
                       coded_ld(H), (const mxm_sample_tile *)L.tiles, (const int32_t *)L.cols, (const int32_t *)L.ncol, (int)ld, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

// LDS of em_loop_samples_narrow_kernel for the linearised sample: 72 KiB at most, so that two workgroups (each with its
// 0.5 KiB of wave sums) still fit a CU's 160 KiB; a batch of smaller samples asks for what its largest one needs.
#define SFIN_LDS_DOUBLES (72 * 1024 / 8)

extern "C" int mxm_em_loop_samples_narrow(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const double *M,
                                          int32_t ld, const int32_t *ncol_host, const double *w, double *props_cur, double *ln_cur,
                                          double *ln_new, mxm_em_state *state, double tol, int32_t max_iter, int32_t check_every,
                                          double *E, void *ws, size_t ws_bytes, void *stream, mxm_em_state *state_host) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_em_loop_samples_narrow", &n_tiles));
    if (M == nullptr || props_cur == nullptr || ln_cur == nullptr || ln_new == nullptr || state == nullptr || state_host == nullptr)
        return fail(-1, "mxm_em_loop_samples_narrow: bad arguments");
    RC_TRY(finish_cols_check("mxm_em_loop_samples_narrow", S, H, ld, ncol_host, nullptr, nullptr));
    RC_TRY(finish_ws_check("mxm_em_loop_samples_narrow", ws, ws_bytes, n_tiles, S, ld));
    // the linearised samples: in LDS where they fit, else in the global copy E
    int64_t lds_doubles = 0;
    bool spills = false;
    for (int32_t b = 0; b < S; ++b) {
        const int64_t cells = (row0_host[b + 1] - row0_host[b]) * (int64_t)ncol_host[b];
        if (cells <= SFIN_LDS_DOUBLES) lds_doubles = std::max(lds_doubles, cells);
        else spills = true;
    }
    if (spills && E == nullptr)
        return fail(-1, "mxm_em_loop_samples_narrow: a sample of more than %d cells needs the global copy E", SFIN_LDS_DOUBLES);
    if (check_every < 1) check_every = 1;
    if (T.progress != nullptr && check_every > T.progress_every) check_every = T.progress_every;
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, (int)ld);
    const size_t lds = (size_t)lds_doubles * sizeof(double);
    // the opt-in to more than 64 KiB of dynamic LDS once, before the loop
    int lds_rc = -1;
    (void)dispatch_width<SFIN_KMAX>((int)ld, [&](auto n) {
        constexpr int LD = decltype(n)::value;
        if constexpr (LD == 4 || LD == 8 || LD == 16)
            lds_rc = dynamic_lds_ok(reinterpret_cast<const void *>(&em_loop_samples_narrow_kernel<LD>), lds, "em_loop_samples_narrow_kernel");
    });
    RC_TRY(lds_rc);
    auto launch = [&](int chunk) -> int {
        bool launched = false;
        (void)dispatch_width<SFIN_KMAX>((int)ld, [&](auto n) {
            constexpr int LD = decltype(n)::value;
            if constexpr (LD == 4 || LD == 8 || LD == 16) {
                hipLaunchKernelGGL((em_loop_samples_narrow_kernel<LD>), dim3((unsigned)S), dim3(SFIN_THREADS), lds, s, M, E, w,
                                   (const int64_t *)L.row0, (const int32_t *)L.ncol, ln_cur, ln_new, props_cur, state, tol,
                                   (int)max_iter, chunk, (int)lds_doubles);
                launched = true;
            }
        });
        if (!launched) return fail(-1, "mxm_em_loop_samples_narrow: ld = %d has no kernel instance", ld);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, (int)ld, ncol_host, nullptr, nullptr, L, s));
    RC_TRY(read_state(state_host, state, S, s));
    auto running = [&]() {
        int n = 0;
        for (int b = 0; b < S; ++b) n += (state_host[b].done == 0 && ncol_host[b] > 0) ? 1 : 0;
        return n;
    };
    while (max_iter > 0 && running() > 0) {
        RC_TRY(launch((int)check_every));
        RC_TRY(read_state(state_host, state, S, s));
        if (T.progress != nullptr) T.progress(state_host, S, T.progress_user);
    }
    return 0;
}

extern "C" int mxm_assign_reads_samples(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, const double *M,
                                        int32_t ld, const int32_t *ncol_host, const int32_t *perm_host, const double *ln_theta,
                                        const double *props, const double *log_props, const double *lse, double log_min_fold,
                                        int32_t *assigned, double *post, void *ws, size_t ws_bytes, void *stream) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_assign_reads_samples", &n_tiles));
    if (M == nullptr || perm_host == nullptr || ln_theta == nullptr || props == nullptr || log_props == nullptr || assigned == nullptr)
        return fail(-1, "mxm_assign_reads_samples: bad arguments");
    RC_TRY(finish_cols_check("mxm_assign_reads_samples", S, H, ld, ncol_host, nullptr, perm_host));
    RC_TRY(finish_ws_check("mxm_assign_reads_samples", ws, ws_bytes, n_tiles, S, ld));
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, (int)ld);
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, (int)ld, ncol_host, nullptr, perm_host, L, s));
    bool launched = false;
    (void)dispatch_width<SFIN_KMAX>((int)ld, [&](auto n) {
        constexpr int LD = decltype(n)::value;
        if constexpr (LD == 4 || LD == 8 || LD == 16) {
            hipLaunchKernelGGL((assign_samples_kernel<LD>), dim3((unsigned)n_tiles), dim3(64), 0, s, M, (const mxm_sample_tile *)L.tiles,
                               (const int32_t *)L.ncol, (const int32_t *)L.perm, ln_theta, props, log_props, lse, log_min_fold,
                               assigned, post);
            launched = true;
        }
    });
    if (!launched) return fail(-1, "mxm_assign_reads_samples: ld = %d has no kernel instance", ld);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the same for samples of B EM runs each (samples_runs_kernels.hpp; include/mixemt_hip_samples_runs.h) ----
// The workspace is the one-run layout: the tile table and the per-sample tables have no run dimension (the per-run
// tables are the caller's device arrays); B only has to be one the entries take.
static bool runs_ok(int32_t B) { return B >= 2 && B <= MXM_SAMPLES_RUNS_MAX; }
static int runs_check(const char *who, int32_t B) {
    if (!runs_ok(B)) return fail(-1, "%s: B = %d runs per sample: 2 .. %d are taken (one run: the entries of mixemt_hip_samples_finish.h)",
                                 who, B, MXM_SAMPLES_RUNS_MAX);
    return 0;
}
extern "C" size_t mxm_samples_runs_workspace_bytes(int64_t n_tiles, int32_t S, int32_t B, int32_t ld) {
    if (!runs_ok(B)) return 0;
    return mxm_samples_finish_workspace_bytes(n_tiles, S, ld);
}
static int runs_ws_check(const char *who, const void *ws, size_t ws_bytes, int64_t n_tiles, int32_t S, int32_t B, int32_t ld) {
    if (ws == nullptr || ws_bytes < mxm_samples_runs_workspace_bytes(n_tiles, S, B, ld) || (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(-1, "%s: workspace too small (or not 16-byte aligned)", who);
    return 0;
}

extern "C" int mxm_votes_samples_runs(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *w,
                                      const double *ln_props, const double *props, const double *rowmax, int32_t *best,
                                      double *votes, int64_t *counts, int64_t *first, double *lse, mxm_em_state *state, void *ws,
                                      size_t ws_bytes, void *stream) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_votes_samples_runs", &n_tiles));
    RC_TRY(runs_check("mxm_votes_samples_runs", B));
    if (ln_props == nullptr || props == nullptr || rowmax == nullptr || best == nullptr || votes == nullptr || first == nullptr)
        return fail(-1, "mxm_votes_samples_runs: bad arguments (ln_props, props, rowmax, best, votes and first are required)");
    RC_TRY(runs_ws_check("mxm_votes_samples_runs", ws, ws_bytes, n_tiles, S, B, 0));
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, 0);
    const size_t vlds = (size_t)H * (sizeof(double) + 2 * sizeof(int));
    RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&votes_sum_samples_kernel), vlds, "votes_sum_samples_kernel",
                          "mxm_votes_samples_runs", H, "too wide for the vote kernel"));
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, 0, nullptr, nullptr, nullptr, L, s));
    hipLaunchKernelGGL(votes_best_samples_runs_kernel, dim3((unsigned)n_tiles), dim3(SFIN_THREADS), 0, s, c->rec, c->rec_off, c->ndist,
                       coded_ld(H), (int)H, (int)B, (const mxm_sample_tile *)L.tiles, ln_props, props, rowmax, best, lse);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(votes_sum_samples_kernel, dim3((unsigned)S), dim3(SFIN_THREADS), vlds, s, (const int32_t *)best, w,
                       (const int64_t *)L.row0, (int)H, votes, counts, first, state);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The loop of B entries per sample, one workgroup per (sample, entry): the runs of mixemt_hip_samples_runs.h (boot false:
// every entry under the sample's own weights w [R]) or the replicates of mixemt_hip_bootstrap.h (boot true: entry (s, b)
// under w [B * row0[s] + b * R_s ...], which is then required).  The two differ in the kernel's weight pointer alone.
// NARROW_MASKS: the fits of mixemt_hip_support.h -- entry (s, b) over the columns of mask_host[s * B + b] (0: an unused slot,
// which never counts as running), its e in its own slice of E [B x R x ld] instead of one linearise pass for all.
enum narrow_kind { NARROW_RUNS, NARROW_BOOT, NARROW_MASKS };
static int boot_check(const char *who, int32_t B);
static int boot_ws_check(const char *who, const void *ws, size_t ws_bytes, int64_t n_tiles, int32_t S, int32_t B, int32_t ld);
static int support_check(const char *who, int32_t S, int32_t B, const int32_t *ncol_host, const uint32_t *mask_host);
static int support_ws_check(const char *who, const void *ws, size_t ws_bytes, int64_t n_tiles, int32_t S, int32_t B, int32_t ld);
static int support_upload_masks(void *ws, int64_t n_tiles, int S, int B, int ld, const uint32_t *mask_host, hipStream_t stream,
                                const uint32_t **masks_dev);
static int narrow_entries_loop(const char *who, narrow_kind kind, const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B,
                               const double *M, int32_t ld, const int32_t *ncol_host, const double *w, double *props_cur,
                               double *ln_cur, double *ln_new, mxm_em_state *state, double tol, int32_t max_iter,
                               int32_t check_every, double *E, void *ws, size_t ws_bytes, void *stream, mxm_em_state *state_host,
                               const uint32_t *mask_host = nullptr) {
    const bool boot = kind == NARROW_BOOT, masks = kind == NARROW_MASKS;
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, who, &n_tiles));
    if (!masks) RC_TRY(boot ? boot_check(who, B) : runs_check(who, B));
    if ((boot && w == nullptr) || M == nullptr || props_cur == nullptr || ln_cur == nullptr || ln_new == nullptr || state == nullptr || state_host == nullptr)
        return fail(-1, "%s: bad arguments", who);
    RC_TRY(finish_cols_check(who, S, H, ld, ncol_host, nullptr, nullptr));
    if (masks) {
        RC_TRY(support_check(who, S, B, ncol_host, mask_host));
        RC_TRY(support_ws_check(who, ws, ws_bytes, n_tiles, S, B, ld));
    } else {
        RC_TRY(boot ? boot_ws_check(who, ws, ws_bytes, n_tiles, S, B, ld) : runs_ws_check(who, ws, ws_bytes, n_tiles, S, B, ld));
    }
    // the linearised samples: in each workgroup's LDS where they fit, else in the global copy E, formed once below
    int64_t lds_doubles = 0;
    bool spills = false;
    for (int32_t b = 0; b < S; ++b) {
        const int64_t cells = (row0_host[b + 1] - row0_host[b]) * (int64_t)ncol_host[b];
        if (cells <= SFIN_LDS_DOUBLES) lds_doubles = std::max(lds_doubles, cells);
        else spills = true;
    }
    if (spills && E == nullptr)
        return fail(-1, "%s: a sample of more than %d cells needs the global copy E", who, SFIN_LDS_DOUBLES);
    if (check_every < 1) check_every = 1;
    if (T.progress != nullptr && check_every > T.progress_every) check_every = T.progress_every;
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, (int)ld);
    const size_t lds = (size_t)lds_doubles * sizeof(double);
    const int n_entries = (int)S * (int)B;
    const uint32_t *masks_dev = nullptr;                    // (NARROW_MASKS: in the workspace, uploaded below)
    int lds_rc = -1;
    (void)dispatch_width<SFIN_KMAX>((int)ld, [&](auto n) {
        constexpr int LD = decltype(n)::value;
        if constexpr (LD == 4 || LD == 8 || LD == 16)
            lds_rc = masks ? dynamic_lds_ok(reinterpret_cast<const void *>(&em_loop_samples_narrow_masks_kernel<LD>), lds,
                                            "em_loop_samples_narrow_masks_kernel")
                     : boot ? dynamic_lds_ok(reinterpret_cast<const void *>(&em_loop_samples_narrow_boot_kernel<LD>), lds,
                                           "em_loop_samples_narrow_boot_kernel")
                          : dynamic_lds_ok(reinterpret_cast<const void *>(&em_loop_samples_narrow_runs_kernel<LD>), lds,
                                           "em_loop_samples_narrow_runs_kernel");
    });
    RC_TRY(lds_rc);
    auto launch = [&](int chunk, bool linearise) -> int {
        bool launched = false;
        (void)dispatch_width<SFIN_KMAX>((int)ld, [&](auto n) {
            constexpr int LD = decltype(n)::value;
            if constexpr (LD == 4 || LD == 8 || LD == 16) {
                if (linearise)
                    hipLaunchKernelGGL((linearise_samples_runs_kernel<LD>), dim3((unsigned)n_tiles), dim3(64), 0, s, M,
                                       (const mxm_sample_tile *)L.tiles, (const int64_t *)L.row0, (const int32_t *)L.ncol,
                                       (int)SFIN_LDS_DOUBLES, E);
                else if (masks)
                    hipLaunchKernelGGL((em_loop_samples_narrow_masks_kernel<LD>), dim3((unsigned)n_entries), dim3(SFIN_THREADS), lds, s,
                                       M, E, w, (const int64_t *)L.row0, (const int32_t *)L.ncol, masks_dev, (int)B, ln_cur, ln_new,
                                       props_cur, state, tol, (int)max_iter, chunk, (int)lds_doubles);
                else if (boot)
                    hipLaunchKernelGGL((em_loop_samples_narrow_boot_kernel<LD>), dim3((unsigned)n_entries), dim3(SFIN_THREADS), lds, s,
                                       M, E, w, (const int64_t *)L.row0, (const int32_t *)L.ncol, (int)B, ln_cur, ln_new, props_cur,
                                       state, tol, (int)max_iter, chunk, (int)lds_doubles);
                else
                    hipLaunchKernelGGL((em_loop_samples_narrow_runs_kernel<LD>), dim3((unsigned)n_entries), dim3(SFIN_THREADS), lds, s,
                                       M, E, w, (const int64_t *)L.row0, (const int32_t *)L.ncol, (int)B, ln_cur, ln_new, props_cur,
                                       state, tol, (int)max_iter, chunk, (int)lds_doubles);
                launched = true;
            }
        });
        if (!launched) return fail(-1, "%s: ld = %d has no kernel instance", who, ld);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, (int)ld, ncol_host, nullptr, nullptr, L, s));
    if (masks) RC_TRY(support_upload_masks(ws, n_tiles, (int)S, (int)B, (int)ld, mask_host, s, &masks_dev));
    RC_TRY(read_state(state_host, state, n_entries, s));
    auto running = [&]() {
        int n = 0;
        for (int e = 0; e < n_entries; ++e)
            n += (state_host[e].done == 0 && ncol_host[e / B] > 0 && (!masks || mask_host[e] != 0)) ? 1 : 0;
        return n;
    };
    if (spills && !masks && max_iter > 0 && running() > 0) RC_TRY(launch(0, true));
    while (max_iter > 0 && running() > 0) {
        RC_TRY(launch((int)check_every, false));
        RC_TRY(read_state(state_host, state, n_entries, s));
        if (T.progress != nullptr) T.progress(state_host, n_entries, T.progress_user);
    }
    return 0;
}

extern "C" int mxm_em_loop_samples_narrow_runs(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B,
                                               const double *M, int32_t ld, const int32_t *ncol_host, const double *w,
                                               double *props_cur, double *ln_cur, double *ln_new, mxm_em_state *state, double tol,
                                               int32_t max_iter, int32_t check_every, double *E, void *ws, size_t ws_bytes,
                                               void *stream, mxm_em_state *state_host) {
    MXM_ENTER();
    return narrow_entries_loop("mxm_em_loop_samples_narrow_runs", NARROW_RUNS, c, row0_host, S, H, B, M, ld, ncol_host, w, props_cur, ln_cur,
                               ln_new, state, tol, max_iter, check_every, E, ws, ws_bytes, stream, state_host);
}

extern "C" int mxm_assign_reads_samples_runs(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B,
                                             const double *M, int32_t ld, const int32_t *ncol_host, const int32_t *perm_host,
                                             const double *ln_theta, const double *props, const double *log_props,
                                             const double *lse, double log_min_fold, int32_t *assigned, double *post, void *ws,
                                             size_t ws_bytes, void *stream) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, "mxm_assign_reads_samples_runs", &n_tiles));
    RC_TRY(runs_check("mxm_assign_reads_samples_runs", B));
    if (M == nullptr || perm_host == nullptr || ln_theta == nullptr || props == nullptr || log_props == nullptr || assigned == nullptr)
        return fail(-1, "mxm_assign_reads_samples_runs: bad arguments");
    RC_TRY(finish_cols_check("mxm_assign_reads_samples_runs", S, H, ld, ncol_host, nullptr, perm_host));
    RC_TRY(runs_ws_check("mxm_assign_reads_samples_runs", ws, ws_bytes, n_tiles, S, B, ld));
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, (int)ld);
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, (int)ld, ncol_host, nullptr, perm_host, L, s));
    const double neg_log_runs = -log((double)B);            // the host's logarithm, as em.collect_result hands it to mxm_add_scalar
    bool launched = false;
    (void)dispatch_width<SFIN_KMAX>((int)ld, [&](auto n) {
        constexpr int LD = decltype(n)::value;
        if constexpr (LD == 4 || LD == 8 || LD == 16) {
            hipLaunchKernelGGL((assign_samples_runs_kernel<LD>), dim3((unsigned)n_tiles), dim3(64), 0, s, M,
                               (const mxm_sample_tile *)L.tiles, (const int32_t *)L.ncol, (const int32_t *)L.perm, (int)B, ln_theta,
                               props, log_props, lse, neg_log_runs, log_min_fold, assigned, post);
            launched = true;
        }
    });
    if (!launched) return fail(-1, "mxm_assign_reads_samples_runs: ld = %d has no kernel instance", ld);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- bootstrap replicates of the refinement loop (bootstrap_kernels.hpp; include/mixemt_hip_bootstrap.h) ----
// scratch layout: [the one-run layout][cum, rows x u32][ntot, S x i64][sid, S x u32][cnt, min(B, 64) x rows x u32] with
// rows = n_tiles x MXM_SAMPLES_TILE_ROWS, the most rows a plan of n_tiles tiles can hold
struct boot_ws {
    uint32_t *cum, *sid, *cnt;
    int64_t *ntot;
    int64_t rows;
    size_t bytes;
};
static boot_ws boot_layout(void *ws, int64_t n_tiles, int S, int B, int ld) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    boot_ws L;
    char *base = static_cast<char *>(ws);
    size_t at = finish_layout(nullptr, n_tiles, S, ld).bytes;
    L.rows = n_tiles * MXM_SAMPLES_TILE_ROWS;
    L.cum = reinterpret_cast<uint32_t *>(base + at);
    at += up((size_t)L.rows * sizeof(uint32_t));
    L.ntot = reinterpret_cast<int64_t *>(base + at);
    at += up((size_t)S * sizeof(int64_t));
    L.sid = reinterpret_cast<uint32_t *>(base + at);
    at += up((size_t)S * sizeof(uint32_t));
    L.cnt = reinterpret_cast<uint32_t *>(base + at);
    at += up((size_t)std::min(B, BOOT_CHUNK) * (size_t)L.rows * sizeof(uint32_t));
    L.bytes = at;
    return L;
}
static bool boot_ok(int32_t B) { return B >= 2 && B <= MXM_BOOTSTRAP_MAX; }
static int boot_check(const char *who, int32_t B) {
    if (!boot_ok(B)) return fail(-1, "%s: B = %d replicates per sample: 2 .. %d are taken", who, B, MXM_BOOTSTRAP_MAX);
    return 0;
}
extern "C" size_t mxm_bootstrap_workspace_bytes(int64_t n_tiles, int32_t S, int32_t B, int32_t ld) {
    if (!boot_ok(B) || n_tiles <= 0 || S <= 0 || ld < 0) return 0;
    return boot_layout(nullptr, n_tiles, (int)S, (int)B, (int)ld).bytes;
}
static int boot_ws_check(const char *who, const void *ws, size_t ws_bytes, int64_t n_tiles, int32_t S, int32_t B, int32_t ld) {
    if (ws == nullptr || ws_bytes < mxm_bootstrap_workspace_bytes(n_tiles, S, B, ld) || (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(-1, "%s: workspace too small (or not 16-byte aligned)", who);
    return 0;
}

extern "C" int mxm_bootstrap_weights(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t B, const double *w, uint64_t seed,
                                     const uint32_t *s_id_host, double *wb, mxm_em_state *state, void *ws, size_t ws_bytes,
                                     void *stream) {
    MXM_ENTER();
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, 0, "mxm_bootstrap_weights", &n_tiles, false));
    RC_TRY(boot_check("mxm_bootstrap_weights", B));
    if (w == nullptr || s_id_host == nullptr || wb == nullptr || state == nullptr)
        return fail(-1, "mxm_bootstrap_weights: bad arguments (w, s_id_host, wb and state are required)");
    RC_TRY(boot_ws_check("mxm_bootstrap_weights", ws, ws_bytes, n_tiles, S, B, 0));
    hipStream_t s = (hipStream_t)stream;
    const finish_ws F = finish_layout(ws, n_tiles, (int)S, 0);
    const boot_ws L = boot_layout(ws, n_tiles, (int)S, (int)B, 0);
    // which route the samples take: LDS up to the header's row limit (the batch asks for what its largest such sample needs)
    int64_t lds_rows = 0;
    bool large = false;
    for (int32_t i = 0; i < S; ++i) {
        const int64_t n = row0_host[i + 1] - row0_host[i];
        if (n <= BOOT_LDS_ROWS) lds_rows = std::max(lds_rows, n);
        else large = true;
    }
    const size_t lds = (size_t)lds_rows * 2 * sizeof(uint32_t);
    RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&boot_draw_kernel<false>), lds, "boot_draw_kernel"));
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, 0, nullptr, nullptr, nullptr, F, s));
    static thread_local std::vector<uint32_t> sid;
    sid.assign(s_id_host, s_id_host + (size_t)S);
    HIP_TRY(hipMemcpyAsync(L.sid, sid.data(), sid.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(boot_prefix_kernel, dim3((unsigned)S), dim3(BOOT_THREADS), 0, s, w, (const int64_t *)F.row0, L.cum, L.ntot, state);
    HIP_TRY(hipGetLastError());
    if (lds_rows > 0) {
        hipLaunchKernelGGL((boot_draw_kernel<false>), dim3((unsigned)B, (unsigned)S), dim3(BOOT_THREADS), lds, s, (const int64_t *)F.row0,
                           (const uint32_t *)L.cum, (const int64_t *)L.ntot, (const uint32_t *)L.sid, seed, (int)B, 0, L.cnt, L.rows, wb);
        HIP_TRY(hipGetLastError());
    }
    for (int b0 = 0; large && b0 < B; b0 += BOOT_CHUNK) {    // the counters of BOOT_CHUNK replicates at a time
        hipLaunchKernelGGL((boot_draw_kernel<true>), dim3((unsigned)std::min(BOOT_CHUNK, (int)B - b0), (unsigned)S), dim3(BOOT_THREADS), 0, s,
                           (const int64_t *)F.row0, (const uint32_t *)L.cum, (const int64_t *)L.ntot, (const uint32_t *)L.sid, seed,
                           (int)B, b0, L.cnt, L.rows, wb);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int mxm_em_loop_samples_narrow_boot(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B,
                                               const double *M, int32_t ld, const int32_t *ncol_host, const double *wb,
                                               double *props_cur, double *ln_cur, double *ln_new, mxm_em_state *state, double tol,
                                               int32_t max_iter, int32_t check_every, double *E, void *ws, size_t ws_bytes,
                                               void *stream, mxm_em_state *state_host) {
    MXM_ENTER();
    return narrow_entries_loop("mxm_em_loop_samples_narrow_boot", NARROW_BOOT, c, row0_host, S, H, B, M, ld, ncol_host, wb, props_cur, ln_cur,
                               ln_new, state, tol, max_iter, check_every, E, ws, ws_bytes, stream, state_host);
}

extern "C" int mxm_bootstrap_summary(int32_t S, int32_t B, int32_t ld, const int32_t *ncol_host, const double *ln_new,
                                     const mxm_em_state *state, double q_lo, double q_hi, double *x, double *lo, double *hi,
                                     double *mean, double *sd, int32_t *flag, void *stream) {
    MXM_ENTER();
    if (S < 1 || S > 65535) return fail(-1, "mxm_bootstrap_summary: bad arguments (S = %d; 1 .. 65535 samples)", S);
    RC_TRY(boot_check("mxm_bootstrap_summary", B));
    RC_TRY(finish_cols_check("mxm_bootstrap_summary", S, 0, ld, ncol_host, nullptr, nullptr));
    if (!(q_lo >= 0.0 && q_lo <= 1.0 && q_hi >= 0.0 && q_hi <= 1.0))
        return fail(-1, "mxm_bootstrap_summary: the quantiles %g and %g must lie in [0, 1]", q_lo, q_hi);
    if (ln_new == nullptr || state == nullptr || x == nullptr || lo == nullptr || hi == nullptr || mean == nullptr || sd == nullptr ||
        flag == nullptr)
        return fail(-1, "mxm_bootstrap_summary: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    static thread_local std::vector<int32_t> ncol;          // (the call's own copy, as finish_upload keeps one)
    ncol.assign(ncol_host, ncol_host + (size_t)S);
    HIP_TRY(hipMemcpyAsync(flag, ncol.data(), ncol.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(boot_summary_kernel, dim3((unsigned)ld, (unsigned)S), dim3(BOOT_THREADS), 0, s, (int)B, (int)ld,
                       (const int32_t *)flag, ln_new, state, q_lo, q_hi, x, lo, hi, mean, sd);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(boot_flag_kernel, dim3((unsigned)((S + BOOT_THREADS - 1) / BOOT_THREADS)), dim3(BOOT_THREADS), 0, s, (int)S, (int)ld,
                       (const double *)lo, flag);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- nested-model fits of the refinement loop over column masks (support_kernels.hpp; include/mixemt_hip_support.h) ----
// scratch layout: [the one-run layout][masks, S x B x u32]
static bool support_ok(int32_t B) { return B >= 1 && B <= MXM_SUPPORT_MAX_FITS; }
extern "C" size_t mxm_support_workspace_bytes(int64_t n_tiles, int32_t S, int32_t B, int32_t ld) {
    if (!support_ok(B) || n_tiles <= 0 || S <= 0 || ld < 0) return 0;
    return finish_layout(nullptr, n_tiles, (int)S, (int)ld).bytes + (((size_t)S * (size_t)B * sizeof(uint32_t) + 255) & ~(size_t)255);
}
// B and the masks: every bit of a mask below the sample's column count (mask 0: an unused slot)
static int support_check(const char *who, int32_t S, int32_t B, const int32_t *ncol_host, const uint32_t *mask_host) {
    if (!support_ok(B)) return fail(-1, "%s: B = %d fits per sample: 1 .. %d are taken", who, B, MXM_SUPPORT_MAX_FITS);
    if (mask_host == nullptr) return fail(-1, "%s: bad arguments (mask_host missing)", who);
    for (int32_t s = 0; s < S; ++s)
        for (int32_t b = 0; b < B; ++b) {
            const uint32_t mask = mask_host[(int64_t)s * B + b];
            if (((uint64_t)mask >> ncol_host[s]) != 0)
                return fail(-1, "%s: sample %d, fit %d: mask 0x%x has a bit at or above ncol = %d", who, s, b, mask, ncol_host[s]);
        }
    return 0;
}
static int support_ws_check(const char *who, const void *ws, size_t ws_bytes, int64_t n_tiles, int32_t S, int32_t B, int32_t ld) {
    if (ws == nullptr || ws_bytes < mxm_support_workspace_bytes(n_tiles, S, B, ld) || (reinterpret_cast<uintptr_t>(ws) & 15))
        return fail(-1, "%s: workspace too small (or not 16-byte aligned)", who);
    return 0;
}
// the masks into the workspace behind the one-run layout, from a vector of the call's own (finish_upload says why)
static int support_upload_masks(void *ws, int64_t n_tiles, int S, int B, int ld, const uint32_t *mask_host, hipStream_t stream,
                                const uint32_t **masks_dev) {
    static thread_local std::vector<uint32_t> masks;
    uint32_t *dev = reinterpret_cast<uint32_t *>(static_cast<char *>(ws) + finish_layout(nullptr, n_tiles, S, ld).bytes);
    masks.assign(mask_host, mask_host + (size_t)S * B);
    HIP_TRY(hipMemcpyAsync(dev, masks.data(), masks.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    *masks_dev = dev;
    return 0;
}

extern "C" int mxm_em_loop_samples_narrow_masks(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B,
                                                const double *M, int32_t ld, const int32_t *ncol_host, const uint32_t *mask_host,
                                                const double *w, double *props_cur, double *ln_cur, double *ln_new,
                                                mxm_em_state *state, double tol, int32_t max_iter, int32_t check_every, double *E,
                                                void *ws, size_t ws_bytes, void *stream, mxm_em_state *state_host) {
    MXM_ENTER();
    return narrow_entries_loop("mxm_em_loop_samples_narrow_masks", NARROW_MASKS, c, row0_host, S, H, B, M, ld, ncol_host, w, props_cur,
                               ln_cur, ln_new, state, tol, max_iter, check_every, E, ws, ws_bytes, stream, state_host, mask_host);
}

extern "C" int mxm_loglik_samples_masks(const mxm_coded *c, const int64_t *row0_host, int32_t S, int32_t H, int32_t B, const double *M,
                                        int32_t ld, const int32_t *ncol_host, const uint32_t *mask_host, const double *w,
                                        const double *ln_props, double *ll, double *n_eff, void *ws, size_t ws_bytes, void *stream) {
    MXM_ENTER();
    const char *who = "mxm_loglik_samples_masks";
    int64_t n_tiles = 0;
    RC_TRY(samples_check(c, row0_host, S, H, who, &n_tiles));
    if (M == nullptr || ln_props == nullptr || ll == nullptr || n_eff == nullptr) return fail(-1, "%s: bad arguments", who);
    RC_TRY(finish_cols_check(who, S, H, ld, ncol_host, nullptr, nullptr));
    RC_TRY(support_check(who, S, B, ncol_host, mask_host));
    RC_TRY(support_ws_check(who, ws, ws_bytes, n_tiles, S, B, ld));
    hipStream_t s = (hipStream_t)stream;
    const finish_ws L = finish_layout(ws, n_tiles, (int)S, (int)ld);
    RC_TRY(finish_upload(row0_host, (int)S, n_tiles, (int)ld, ncol_host, nullptr, nullptr, L, s));
    const uint32_t *masks_dev = nullptr;
    RC_TRY(support_upload_masks(ws, n_tiles, (int)S, (int)B, (int)ld, mask_host, s, &masks_dev));
    bool launched = false;
    (void)dispatch_width<SFIN_KMAX>((int)ld, [&](auto n) {
        constexpr int LD = decltype(n)::value;
        if constexpr (LD == 4 || LD == 8 || LD == 16) {
            hipLaunchKernelGGL((loglik_samples_masks_kernel<LD>), dim3((unsigned)((int)S * (int)B)), dim3(SFIN_THREADS), 0, s, M, w,
                               (const int64_t *)L.row0, (const int32_t *)L.ncol, masks_dev, (int)B, ln_props, ll, n_eff);
            launched = true;
        }
    });
    if (!launched) return fail(-1, "%s: ld = %d has no kernel instance", who, ld);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_em_loop_f32(const float *P, int64_t ldp, const double *w, int64_t R, int32_t H, int32_t B,
                               double *props_cur, double *ln_cur, double *ln_new, double *colsum,
                               mxm_em_state *state, double tol, int32_t max_iter, int32_t check_every, void *ws,
                               size_t ws_bytes, void *stream, mxm_em_state *state_host) {
    MXM_ENTER();
    return em_loop_impl(nullptr, 0, reinterpret_cast<const double *>(P), ldp, w, R, H, B, props_cur, ln_cur, ln_new,
                        colsum, state, tol, max_iter, check_every, ws, ws_bytes, stream, state_host, true);
}

template <int NCH>
static void launch_estep_wide(const double *M, int64_t ldm, const double *w, const double *lnp, int64_t R, int H,
                              int grid, double *out, int64_t ldo, int mode, double *partial,
                              int64_t ldpart, hipStream_t s) {
    if (partial != nullptr)
        hipLaunchKernelGGL((estep_wide_kernel<NCH, true>), dim3(grid), dim3(256), 0, s, M, ldm, w, lnp, R, H,
                           out, ldo, mode, partial, ldpart);
    else
        hipLaunchKernelGGL((estep_wide_kernel<NCH, false>), dim3(grid), dim3(256), 0, s, M, ldm, w, lnp, R, H,
                           out, ldo, mode, partial, ldpart);
}

extern "C" int mxm_em_step(const double *M, int64_t ldm, const double *w, const double *ln_props, int64_t R,
                           int32_t H, double *out, int64_t ldo, int32_t mode, double *colsum, void *ws,
                           size_t ws_bytes, void *stream) {
    if (R <= 0 || H <= 0 || ldm < H) return fail(-1, "mxm_em_step: bad shape");
    if (out != nullptr && ldo < H) return fail(-1, "mxm_em_step: ldo < H");
    if (colsum != nullptr && (ws == nullptr || ws_bytes < mxm_workspace_bytes(R, H, 1)))
        return fail(-1, "mxm_em_step: workspace too small");
    const int64_t ldpart = part_ld(H);
    hipStream_t s = (hipStream_t)stream;
    double *partial = colsum ? (double *)ws : (double *)nullptr;
    int nwg;
    const bool aligned = ((H & 1) == 0) && ((ldm & 1) == 0) && ((reinterpret_cast<uintptr_t>(M) & 15) == 0) &&
                         (out == nullptr || (((ldo & 1) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0)));
    const int nch = (H / 2 + 255) / 256;
    // register budget of estep_wide_kernel (spill-free instances only): 13 column chunks per
    // thread without the M-step sums, 10 with them
    const int wide_cap = num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG;
    if (aligned && mxm_linear_supported(H) && nch <= (colsum != nullptr ? 10 : 13)) {
        // wide rows: one read + one write per cell, rows held in registers
        nwg = clamp_grid((R + 1) / 2, wide_cap);            // rows are dealt round-robin (row_deal)
        const bool ok = dispatch_width<16>(nch, [&](auto n) {
            launch_estep_wide<decltype(n)::value>(M, ldm, w, ln_props, R, (int)H, nwg, out, ldo, (int)mode, partial, ldpart, s);
        });
        if (!ok) return fail(-1, "mxm_em_step: H=%d outside the wide kernel's range", H);
    } else if (H <= MXM_NARROW_MAX_H) {
        const int rc = launch_narrow<false>(M, ldm, w, ln_props, R, (int)H, out, ldo, (int)mode, partial, ldpart,
                                            (const mxm_em_state *)nullptr, s, &nwg);
        if (rc != 0) return rc;
    } else {
        const size_t lds = 2 * (size_t)H * sizeof(double);
        nwg = clamp_grid(R, num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG);
        if (lds > 150 * 1024) {                            // any width: the vectors in global memory
            hipLaunchKernelGGL((estep_global_kernel<false>), dim3(nwg), dim3(ROW_THREADS), 0, s, M, ldm, w, ln_props, R, (int)H, out,
                               ldo, (int)mode, partial, ldpart, (const mxm_em_state *)nullptr, (const int64_t *)nullptr);
        } else {
            RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&estep_log_kernel<false>), lds, "estep_log_kernel"));
            hipLaunchKernelGGL((estep_log_kernel<false>), dim3(nwg), dim3(ROW_THREADS), lds, s, M, ldm, w, ln_props, R,
                               (int)H, out, ldo, (int)mode, partial, ldpart, (const mxm_em_state *)nullptr, (const int64_t *)nullptr);
        }
    }
    HIP_TRY(hipGetLastError());
    return colsum != nullptr ? reduce_one((const double *)ws, nwg, (int)H, colsum, nullptr, s) : 0;
}

extern "C" int mxm_log_normalize(const double *colsum, int32_t H, double *ln_new, void *stream) {
    if (H <= 0) return fail(-1, "mxm_log_normalize: H <= 0");
    hipLaunchKernelGGL(log_normalize_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, colsum, (int)H, ln_new);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_l1_exp_diff(const double *a, const double *b, int32_t H, double *l1_out, void *stream) {
    if (H <= 0) return fail(-1, "mxm_l1_exp_diff: H <= 0");
    hipLaunchKernelGGL(l1_exp_diff_kernel, dim3(1), dim3(FIN_THREADS), 0, (hipStream_t)stream, a, b, (int)H, l1_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_add_scalar(double *x, int64_t ld, int64_t R, int32_t H, double delta, void *stream) {
    if (R <= 0 || H <= 0 || ld < H) return fail(-1, "mxm_add_scalar: bad shape");
    hipLaunchKernelGGL(add_scalar_kernel, dim3(clamp_grid(R, num_cu() * 8)), dim3(256), 0, (hipStream_t)stream, x, ld, R, (int)H, delta);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_assign_reads(const double *X, int64_t ldx, const double *log_props, const int32_t *cols,
                                int32_t nC, int64_t R, int32_t H, double log_min_fold, int32_t *assigned,
                                void *stream) {
    if (R <= 0 || H <= 0 || nC <= 0 || ldx < H) return fail(-1, "mxm_assign_reads: bad shape");
    hipLaunchKernelGGL(assign_reads_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, (hipStream_t)stream, X,
                       ldx, log_props, cols, (int)nC, R, log_min_fold, assigned);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_diag_stream_read(const void *src, size_t bytes, int32_t wg_per_cu, int32_t blocked, void *sink,
                                    void *stream) {
    if (src == nullptr || sink == nullptr || bytes < 16 || wg_per_cu < 1) return fail(-1, "mxm_diag_stream_read: bad arguments");
    if (blocked == 3) {
        // em_iter_coded_kernel's pattern: records of 5408 code bytes + 27 doubles (5624 bytes), two workgroups per CU
        const int code_bytes = 5408, tbl = 27, rec_bytes = code_bytes + tbl * 8;
        const int64_t recs = (int64_t)bytes / rec_bytes;
        if (recs < 1) return fail(-1, "mxm_diag_stream_read: buffer smaller than one record");
        hipLaunchKernelGGL(diag_stream_records_kernel<6>, dim3(clamp_grid(recs, num_cu() * wg_per_cu)), dim3(256), 0,
                           (hipStream_t)stream, (const uint8_t *)src, recs, rec_bytes, code_bytes, tbl, (unsigned int *)sink);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (blocked == 2) {
        // the EM kernel's pattern: rows of 5408 doubles (2704 x 16 B) dealt over one workgroup per CU
        const int row16 = 2704;
        const int64_t rows = (int64_t)(bytes / 16) / row16;
        if (rows < 1) return fail(-1, "mxm_diag_stream_read: buffer smaller than one row");
        hipLaunchKernelGGL(diag_stream_dealt_kernel<6>, dim3(clamp_grid(rows, num_cu() * wg_per_cu)), dim3(512), 0,
                           (hipStream_t)stream, (const double *)src, rows, row16, (unsigned int *)sink);
    } else if (blocked)
        hipLaunchKernelGGL(diag_stream_read_kernel<true>, dim3(num_cu() * wg_per_cu), dim3(256), 0, (hipStream_t)stream,
                           (const uint4 *)src, (int64_t)(bytes / 16), (unsigned int *)sink);
    else
        hipLaunchKernelGGL(diag_stream_read_kernel<false>, dim3(num_cu() * wg_per_cu), dim3(256), 0, (hipStream_t)stream,
                           (const uint4 *)src, (int64_t)(bytes / 16), (unsigned int *)sink);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_diag_stream_coded(const mxm_coded *c, int32_t H, int32_t wg_per_cu, void *sink, void *stream) {
    RC_TRY(coded_check(c, H, "mxm_diag_stream_coded"));
    if (sink == nullptr || wg_per_cu < 1) return fail(-1, "mxm_diag_stream_coded: bad arguments");
    const int ldc = coded_ld(H);
    if ((ldc / 4 + 255) / 256 != 6) return fail(-1, "mxm_diag_stream_coded: built for H in (5120, 6144]");
    hipLaunchKernelGGL(diag_stream_coded_kernel<6>, dim3(clamp_grid(c->R, num_cu() * wg_per_cu)), dim3(256), 0, (hipStream_t)stream,
                       c->rec, c->rec_off, c->ndist, ldc, c->R, (unsigned int *)sink);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_diag_stream_quads(const mxm_coded *c, int32_t H, int32_t wg_per_cu, void *sink, void *stream) {
    RC_TRY(coded_check(c, H, "mxm_diag_stream_quads"));
    if (sink == nullptr || wg_per_cu < 1 || c->qrec == nullptr || c->n_quad_rows <= 0)
        return fail(-1, "mxm_diag_stream_quads: a coded matrix with a quad dictionary required");
    hipLaunchKernelGGL(diag_stream_quads_kernel, dim3(clamp_grid(c->n_quad_rows, num_cu() * wg_per_cu)), dim3(QUAD_THREADS), 0,
                       (hipStream_t)stream, c->qrec, c->qoff, c->nquad, c->quad_rows, c->n_quad_rows, c->R, (unsigned int *)sink);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_row_argmax_votes(const double *X, int64_t ldx, const double *w, int64_t R, int32_t H,
                                    int32_t *best, double *votes, void *ws, size_t ws_bytes, void *stream) {
    if (R <= 0 || H <= 0 || ldx < H) return fail(-1, "mxm_row_argmax_votes: bad shape");
    if (votes != nullptr && (ws == nullptr || ws_bytes < mxm_workspace_bytes(R, H, 1)))
        return fail(-1, "mxm_row_argmax_votes: workspace too small");
    // votes: every workgroup fills its own row of the scratch (one thread adds in row order), the
    // rows are summed in fixed order -- no float atomics, so fractional weights reproduce bit for bit
    double *part = votes != nullptr ? (double *)ws : (double *)nullptr;
    const int64_t ldpart = part_ld(H);
    int nwg;
    if (wide_rows_ok(X, ldx, H)) {
        const int nch = (H / 2 + 255) / 256;
        const int cap = num_cu() * 2 < MXM_MAX_WG ? num_cu() * 2 : MXM_MAX_WG;
        nwg = clamp_grid((R + 1) / 2, cap);
        const size_t lds = votes != nullptr ? (size_t)H * sizeof(double) : 0;
        int lrc = 0;
        const bool ok = dispatch_width<16>(nch, [&](auto n) {
            constexpr int NCH = decltype(n)::value;
            // (with the static exchange buffers this passes the 64 KiB default)
            lrc = dynamic_lds_ok(reinterpret_cast<const void *>(&row_argmax_wide_kernel<NCH>), lds, "row_argmax_wide_kernel");
            if (lrc == 0)
                hipLaunchKernelGGL((row_argmax_wide_kernel<NCH>), dim3(nwg), dim3(256), lds, (hipStream_t)stream, X, ldx, w, R, (int)H,
                                   best, part, ldpart);
        });
        if (!ok) return fail(-1, "mxm_row_argmax_votes: H=%d outside the wide kernel's range", H);
        if (lrc != 0) return lrc;
    } else {
        nwg = clamp_grid(R, num_cu() * 4 < MXM_MAX_WG ? num_cu() * 4 : MXM_MAX_WG);
        hipLaunchKernelGGL(row_argmax_votes_kernel, dim3(nwg), dim3(ROW_THREADS), 0, (hipStream_t)stream, X, ldx, w, R,
                           (int)H, best, part, ldpart);
    }
    HIP_TRY(hipGetLastError());
    return votes != nullptr ? reduce_one(part, nwg, (int)H, votes, nullptr, (hipStream_t)stream) : 0;
}

extern "C" int mxm_first_seen(const int32_t *best, int64_t R, int32_t H, int64_t *first, void *stream) {
    if (best == nullptr || first == nullptr || R < 0 || H <= 0) return fail(-1, "mxm_first_seen: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(fill_u64_kernel, dim3(clamp_grid((H + 255) / 256, 64)), dim3(256), 0, s,
                       reinterpret_cast<unsigned long long *>(first), (int64_t)H, (unsigned long long)R);
    if (R > 0) {
        // ranges of at least 1024 rows and below 2^32 (32-bit offsets in LDS)
        int grid = clamp_grid((R + 1023) / 1024, num_cu() * 4);
        while ((R + grid - 1) / grid >= ((int64_t)1 << 32)) grid *= 2;
        for (int h0 = 0; h0 < H; h0 += FSEEN_MAX_H)          // (one launch up to 8192 haplogroups)
            hipLaunchKernelGGL(first_seen_kernel, dim3(grid), dim3(256), 0, s, best, R, h0,
                               (int)(H - h0 < FSEEN_MAX_H ? H - h0 : FSEEN_MAX_H), reinterpret_cast<unsigned long long *>(first));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_gather_columns(const double *M, int64_t ldm, int64_t R, int32_t H, const int32_t *cols, int32_t nC,
                                  double *out, int64_t ldo, void *stream) {
    if (R < 0 || H <= 0 || nC <= 0 || ldm < H || ldo < nC) return fail(-1, "mxm_gather_columns: bad shape");
    if (R == 0) return 0;
    const int64_t want = (R * (int64_t)nC + 255) / 256;
    hipLaunchKernelGGL(gather_columns_kernel, dim3(clamp_grid(want, num_cu() * 16)), dim3(256), 0, (hipStream_t)stream,
                       M, ldm, R, cols, (int)nC, out, ldo, (const int64_t *)nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_fold_logaddexp(double *acc, int64_t lda, const double *const *in_host, const int64_t *ld_in_host,
                                  int32_t n_in, int64_t R, int32_t H, double delta, void *stream) {
    if (R < 0 || H <= 0 || lda < H || n_in < 0 || n_in > FOLD_MAX_IN)
        return fail(-1, "mxm_fold_logaddexp: bad shape (at most %d inputs per call)", FOLD_MAX_IN);
    if (R == 0) return 0;
    fold_inputs in;
    bool vec = ((H & 1) == 0) && ((lda & 1) == 0) && ((reinterpret_cast<uintptr_t>(acc) & 15) == 0);
    for (int k = 0; k < FOLD_MAX_IN; ++k) {
        in.ptr[k] = k < n_in ? in_host[k] : nullptr;
        in.ld[k] = k < n_in ? ld_in_host[k] : 0;
        if (k < n_in) {
            if (in.ptr[k] == nullptr || in.ld[k] < H) return fail(-1, "mxm_fold_logaddexp: bad input %d", k);
            vec = vec && ((in.ld[k] & 1) == 0) && ((reinterpret_cast<uintptr_t>(in.ptr[k]) & 15) == 0);
        }
    }
    const int grid = clamp_grid(R, num_cu() * 8);
    if (vec)
        hipLaunchKernelGGL(fold_logaddexp_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, acc, lda, in,
                           (int)n_in, R, (int)H, delta);
    else
        hipLaunchKernelGGL(fold_logaddexp_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, acc, lda, in,
                           (int)n_in, R, (int)H, delta);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------
// Host side of the three entries that walk alignments on the device (aln_walk.hpp): the pileup, the tie rule, the
// extension.  Each is blocking: its scratch is stream-ordered memory of the call's own, and the error word is read
// back before returning.
// ------------------------------------------------------------------------------------------
static int aln_columns_ok(const char *name, const mxm_aln_columns *cols) {
    if (cols == nullptr || cols->n_aln < 0) return fail(-1, "%s: bad arguments", name);
    if (cols->n_aln > 0x7fffffffLL) return fail(-1, "%s: more than 2^31 - 1 alignments (%lld)", name, (long long)cols->n_aln);
    if (cols->n_aln > 0 && (cols->ref_start == nullptr || cols->mapq == nullptr || cols->cig_ptr == nullptr ||
                            cols->cigar == nullptr || cols->seq_ptr == nullptr || cols->seq == nullptr))
        return fail(-1, "%s: ref_start, mapq, cig_ptr, cigar, seq_ptr and seq are required", name);
    return 0;
}

// One pass with an error word: `enqueue(scratch, err)` puts the call's work on the stream (scratch: `bytes` of its own,
// 8-byte aligned; err: the word, ALN_ERR_NONE) and returns the first HIP error it met; the word is copied to *err_host,
// the memory released and the stream synchronised.  The first HIP error wins; after one nothing is waited for.
template <typename F>
static hipError_t aln_pass(hipStream_t s, size_t bytes, unsigned long long *err_host, F enqueue) {
    unsigned long long *err = nullptr;
    *err_host = ALN_ERR_NONE;
    hipError_t e = hipMallocAsync(reinterpret_cast<void **>(&err), 8 + bytes, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(err, 0xff, 8, s);
    if (e == hipSuccess) e = enqueue(static_cast<void *>(err + 1), err);
    if (e == hipSuccess) e = hipMemcpyAsync(err_host, err, 8, hipMemcpyDeviceToHost, s);
    const hipError_t ef = hipFreeAsync(err, s);
    if (e == hipSuccess) e = ef;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    return e;
}

// The error word as a return code and message; kind3 / kind0: the caller's text after "alignment N " for its own kinds.
static int aln_walk_error(const char *name, unsigned long long err_host, const char *kind3, const char *kind0 = nullptr) {
    if (err_host == ALN_ERR_NONE) return 0;
    const long long i = (long long)(err_host >> 2);
    const int kind = (int)(err_host & 3);
    if (kind == 1) return fail(-4, "%s: the CIGAR of alignment %lld runs past its sequence", name, (long long)i);
    if (kind == 2) return fail(-4, "%s: the CIGAR of alignment %lld holds an unknown operation", name, (long long)i);
    snprintf(g_err, sizeof(g_err), "%s: alignment %lld %s", name, i, kind == 0 && kind0 != nullptr ? kind0 : kind3);
    return -1;
}

// The pileup (observe_kernels.hpp).  LABELLED: n_labels tables counts[n_labels][L][16], alignment i into table label[i]
// (negative: not counted); otherwise one table and `label` / n_labels are not read.
template <bool LABELLED>
static int observe_bases_impl(const char *name, const mxm_aln_columns *cols, const uint8_t *is_reverse,
                              const int32_t *label, int32_t n_labels, int32_t min_mq, int32_t min_bq, int64_t L,
                              uint32_t *counts, void *stream) {
    if (cols == nullptr || cols->n_aln < 0 || L < 0 || (L > 0 && n_labels > 0 && counts == nullptr))
        return fail(-1, "%s: bad arguments", name);
    if (LABELLED && n_labels < 0) return fail(-1, "%s: n_labels < 0 (%d)", name, n_labels);
    RC_TRY(aln_columns_ok(name, cols));
    const int64_t n = cols->n_aln;
    if (n == 0) return 0;
    if (LABELLED && label == nullptr) return fail(-1, "%s: label is required", name);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nb = (L + OBS_BUCKET - 1) / OBS_BUCKET;   // windows of one table
    const int64_t nbk = LABELLED ? nb * (int64_t)n_labels : nb;
    // scratch: cnt[nbk], cursor[nbk], off[nbk + 1], chunk_off[nbk + 1], then perm[n] (int32)
    unsigned long long err_host;
    const size_t bytes = (size_t)(4 * nbk + 2) * 8 + (size_t)n * 4;
    HIP_TRY(aln_pass(s, bytes, &err_host, [&](void *scratch, unsigned long long *err) {
        unsigned long long *cnt = static_cast<unsigned long long *>(scratch), *cursor = cnt + nbk, *off = cursor + nbk,
                           *chunk_off = off + nbk + 1;
        int32_t *perm = reinterpret_cast<int32_t *>(chunk_off + nbk + 1);
        const hipError_t e = hipMemsetAsync(cnt, 0, (size_t)nbk * 8, s);
        if (e != hipSuccess) return e;
        const unsigned grid_b = (unsigned)((n + OBS_BKT_PER_WG - 1) / OBS_BKT_PER_WG);
        hipLaunchKernelGGL((observe_bucket_kernel<LABELLED, 0>), dim3(grid_b), dim3(OBS_BKT_THREADS), 0, s,
                           cols->ref_start, cols->mapq, label, n_labels, n, min_mq, L, nb, nbk, cnt, perm, err);
        hipLaunchKernelGGL(observe_scan_kernel, dim3(1), dim3(1024), 0, s, cnt, nbk, off, chunk_off, cursor);
        hipLaunchKernelGGL((observe_bucket_kernel<LABELLED, 1>), dim3(grid_b), dim3(OBS_BKT_THREADS), 0, s,
                           cols->ref_start, cols->mapq, label, n_labels, n, min_mq, L, nb, nbk, cursor, perm, err);
        // at most one partial chunk per bucket beyond the full ones
        const int64_t grid_c = (n + OBS_CHUNK - 1) / OBS_CHUNK + nbk;
        if (grid_c > 0x7fffffffLL) return hipErrorInvalidValue;
        hipLaunchKernelGGL(observe_count_kernel<LABELLED>, dim3((unsigned)grid_c), dim3(OBS_THREADS), 0, s,
                           aln_view_of(cols, min_mq, min_bq), is_reverse, L, nb, nbk, off, chunk_off, perm, counts, err);
        return hipGetLastError();
    }));
    char kind0[64], kind3[64];
    snprintf(kind0, sizeof(kind0), "has a label >= n_labels (%lld)", (long long)n_labels);
    snprintf(kind3, sizeof(kind3), "reaches past the table (L = %lld)", (long long)L);
    return aln_walk_error(name, err_host, kind3, kind0);
}

extern "C" int mxm_observe_bases(const mxm_aln_columns *cols, const uint8_t *is_reverse, int32_t min_mq, int32_t min_bq,
                                 int64_t L, uint32_t *counts, void *stream) {
    return observe_bases_impl<false>("mxm_observe_bases", cols, is_reverse, nullptr, 1, min_mq, min_bq, L, counts,
                                     stream);
}

extern "C" int mxm_observe_bases_labelled(const mxm_aln_columns *cols, const uint8_t *is_reverse, const int32_t *label,
                                          int32_t n_labels, int32_t min_mq, int32_t min_bq, int64_t L, uint32_t *counts,
                                          void *stream) {
    return observe_bases_impl<true>("mxm_observe_bases_labelled", cols, is_reverse, label, n_labels, min_mq, min_bq, L,
                                    counts, stream);
}

// ------------------------------------------------------------------------------------------
// The variant check of a cohort's samples over their pileups (var_check_kernels.hpp).  Every refusal comes before the
// first HIP call.  The host tables go into stream-ordered memory of the call's own (from pageable memory: the runtime has
// taken the bytes when hipMemcpyAsync returns), released behind the kernel; nothing is waited for -- checked on a stream
// with work pending (tests/test_gpu_stream_contract.py: the call returns at once, the tables are overwritten at return).
// ------------------------------------------------------------------------------------------
static_assert(VCHK_MAX_L == MXM_VAR_CHECK_MAX_L, "the header states the kernel's cap");
extern "C" int mxm_check_variants_samples(const uint32_t *counts, int32_t S, int64_t L, const int32_t *key_ptr, const int32_t *key,
                                          int32_t H, const int32_t *site, const int32_t *site_key, int32_t n_sites,
                                          int64_t max_pos, const int32_t *cand_host, const int32_t *ncand_host, int32_t ld,
                                          double min_var_reads, double frac_var_reads, double var_fraction,
                                          int32_t has_var_count, int32_t var_count, uint8_t *keep, int32_t *n_uniq,
                                          int32_t *n_found, void *stream) {
    const char *who = "mxm_check_variants_samples";
    if (S < 0) return fail(-1, "%s: S < 0 (%d)", who, S);
    if (ld != 4 && ld != 8 && ld != 16 && ld != 32 && ld != VCHK_MAX_LD)
        return fail(-1, "%s: ld = %d: the candidate tables' row stride must be 4, 8, 16, 32 or 64", who, ld);
    if (S == 0) return 0;
    if (cand_host == nullptr || ncand_host == nullptr) return fail(-1, "%s: bad arguments (cand_host and ncand_host are required)", who);
    int64_t n_cand = 0;
    for (int32_t s = 0; s < S; ++s) {
        const int32_t k = ncand_host[s];
        if (k < 0 || k > ld) return fail(-1, "%s: sample %d has ncand = %d outside [0, %d]", who, s, k, ld);
        for (int32_t i = 0; i < k; ++i) {
            const int32_t h = cand_host[(int64_t)s * ld + i];
            if (h < 0 || h >= H) return fail(-1, "%s: sample %d, candidate %d: haplogroup index %d outside [0, %d)", who, s, i, h, H);
        }
        n_cand += k;
    }
    if (counts == nullptr || key_ptr == nullptr || key == nullptr || keep == nullptr || (n_sites > 0 && (site == nullptr || site_key == nullptr)))
        return fail(-1, "%s: bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)", who);
    if ((reinterpret_cast<uintptr_t>(counts) & 15) != 0) return fail(-1, "%s: counts must be 16-byte aligned", who);
    if (L <= 0 || n_sites < 0) return fail(-1, "%s: bad shape (L = %lld, n_sites = %d)", who, (long long)L, n_sites);
    if (max_pos >= L)
        return fail(-1, "%s: max_pos = %lld: the tree's variants reach past the pileup (L = %lld)", who, (long long)max_pos, (long long)L);
    if (L > VCHK_MAX_L)
        return fail(-1, "%s: L = %lld: a sample's bitsets do not fit the kernel's LDS (L <= %d)", who, (long long)L, VCHK_MAX_L);
    if (n_cand == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = vchk_lds_bytes(L);
    RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&check_variants_samples_kernel), lds, "check_variants_samples_kernel"));
    int32_t *tables = nullptr;
    const size_t n_tab = (size_t)S * ld;
    // both tables through one vector of the call's own (pageable): a caller's pinned array would be read when the stream
    // gets there, after the caller may have changed it
    static thread_local std::vector<int32_t> staged;
    staged.assign(cand_host, cand_host + n_tab);
    staged.insert(staged.end(), ncand_host, ncand_host + (size_t)S);
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&tables), staged.size() * sizeof(int32_t), st));
    hipError_t e = hipMemcpyAsync(tables, staged.data(), staged.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(check_variants_samples_kernel, dim3((unsigned)S), dim3(VCHK_THREADS), lds, st, counts, L, key_ptr, key,
                           site, site_key, (int)n_sites, (const int32_t *)tables, (const int32_t *)(tables + n_tab), (int)ld,
                           min_var_reads, frac_var_reads, var_fraction, (int)(has_var_count != 0), (int)var_count, keep, n_uniq,
                           n_found);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(tables, st);
    HIP_TRY(e);
    HIP_TRY(ef);
    return 0;
}

// ------------------------------------------------------------------------------------------
// The detection bootstrap's tail (detect_kernels.hpp; include/mixemt_hip_detect.h): the candidate rule and the variant check
// for entries whose tables are on the device.  Every refusal comes before the first HIP call; the one host table of each
// entry is uploaded as mxm_check_variants_samples uploads its own.
// ------------------------------------------------------------------------------------------
static_assert(DETECT_MAX_LD == VCHK_MAX_LD, "the candidate rule fills the check's widest row");
static bool detect_ld_ok(int32_t ld) { return ld == 4 || ld == 8 || ld == 16 || ld == 32 || ld == DETECT_MAX_LD; }

extern "C" int mxm_detect_candidates(const double *votes, const int64_t *first, const int64_t *rows_host, const double *props,
                                     const mxm_em_state *state, int32_t E, int32_t H, double min_reads, int32_t ld, int32_t *cand,
                                     int32_t *ncand, double *cprop, void *stream) {
    const char *who = "mxm_detect_candidates";
    if (E < 0) return fail(-1, "%s: E < 0 (%d)", who, E);
    if (H < 1) return fail(-1, "%s: H = %d: at least one haplogroup is needed", who, H);
    if (!detect_ld_ok(ld)) return fail(-1, "%s: ld = %d: the candidate tables' row stride must be 4, 8, 16, 32 or 64", who, ld);
    if (E == 0) return 0;
    if (votes == nullptr || first == nullptr || rows_host == nullptr || props == nullptr || cand == nullptr || ncand == nullptr ||
        cprop == nullptr)
        return fail(-1, "%s: bad arguments (votes, first, rows_host, props, cand, ncand and cprop are required)", who);
    for (int32_t e = 0; e < E; ++e)
        if (rows_host[e] < 0) return fail(-1, "%s: entry %d has %lld rows", who, e, (long long)rows_host[e]);
    hipStream_t st = (hipStream_t)stream;
    static thread_local std::vector<int64_t> staged;      // (pageable and the call's own: read before the call returns)
    staged.assign(rows_host, rows_host + (size_t)E);
    int64_t *rows = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&rows), staged.size() * sizeof(int64_t), st));
    hipError_t e = hipMemcpyAsync(rows, staged.data(), staged.size() * sizeof(int64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(detect_candidates_kernel, dim3((unsigned)E), dim3(DETECT_THREADS), 0, st, votes, first, (const int64_t *)rows,
                           props, state, (int)H, min_reads, (int)ld, cand, ncand, cprop);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(rows, st);
    HIP_TRY(e);
    HIP_TRY(ef);
    return 0;
}

extern "C" int mxm_check_variants_entries(const uint32_t *counts, int32_t T, int64_t L, const int32_t *key_ptr, const int32_t *key,
                                          int32_t H, const int32_t *site, const int32_t *site_key, int32_t n_sites, int64_t max_pos,
                                          const int32_t *table_of_host, int32_t E, const int32_t *cand, const int32_t *ncand,
                                          int32_t ld, double min_var_reads, double frac_var_reads, double var_fraction,
                                          int32_t has_var_count, int32_t var_count, uint8_t *keep, int32_t *n_uniq, int32_t *n_found,
                                          int32_t *flag, void *stream) {
    const char *who = "mxm_check_variants_entries";
    if (E < 0) return fail(-1, "%s: E < 0 (%d)", who, E);
    if (!detect_ld_ok(ld)) return fail(-1, "%s: ld = %d: the candidate tables' row stride must be 4, 8, 16, 32 or 64", who, ld);
    if (E == 0) return 0;
    if (T < 1) return fail(-1, "%s: T = %d: at least one pileup table is needed", who, T);
    if (table_of_host == nullptr || cand == nullptr || ncand == nullptr || flag == nullptr)
        return fail(-1, "%s: bad arguments (table_of_host, cand, ncand and flag are required)", who);
    for (int32_t e = 0; e < E; ++e)
        if (table_of_host[e] < 0 || table_of_host[e] >= T)
            return fail(-1, "%s: entry %d: table %d outside [0, %d)", who, e, table_of_host[e], T);
    if (counts == nullptr || key_ptr == nullptr || key == nullptr || keep == nullptr || (n_sites > 0 && (site == nullptr || site_key == nullptr)))
        return fail(-1, "%s: bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)", who);
    if ((reinterpret_cast<uintptr_t>(counts) & 15) != 0) return fail(-1, "%s: counts must be 16-byte aligned", who);
    if (L <= 0 || n_sites < 0 || H < 1) return fail(-1, "%s: bad shape (L = %lld, n_sites = %d, H = %d)", who, (long long)L, n_sites, H);
    if (max_pos >= L)
        return fail(-1, "%s: max_pos = %lld: the tree's variants reach past the pileup (L = %lld)", who, (long long)max_pos, (long long)L);
    if (L > VCHK_MAX_L)
        return fail(-1, "%s: L = %lld: a sample's bitsets do not fit the kernel's LDS (L <= %d)", who, (long long)L, VCHK_MAX_L);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = vchk_lds_bytes(L);
    RC_TRY(dynamic_lds_ok(reinterpret_cast<const void *>(&check_variants_entries_kernel), lds, "check_variants_entries_kernel"));
    static thread_local std::vector<int32_t> staged;
    staged.assign(table_of_host, table_of_host + (size_t)E);
    int32_t *table_of = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&table_of), staged.size() * sizeof(int32_t), st));
    hipError_t e = hipMemcpyAsync(table_of, staged.data(), staged.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(check_variants_entries_kernel, dim3((unsigned)E), dim3(VCHK_THREADS), lds, st, counts, L, key_ptr, key, (int)H,
                           site, site_key, (int)n_sites, (const int32_t *)table_of, cand, ncand, (int)ld, min_var_reads, frac_var_reads,
                           var_fraction, (int)(has_var_count != 0), (int)var_count, keep, n_uniq, n_found, flag);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(table_of, st);
    HIP_TRY(e);
    HIP_TRY(ef);
    return 0;
}

// ------------------------------------------------------------------------------------------
// The assembly stage (assemble_kernels.hpp): consensus, new variants, the tie rule, extension.
// ------------------------------------------------------------------------------------------
extern "C" int mxm_consensus(const uint32_t *counts, int32_t n_labels, int64_t L, int64_t ref_len, int64_t min_cov,
                             int32_t strict, uint8_t *cons, uint8_t *tied, uint32_t *n_tied, void *stream) {
    if (n_labels < 0 || L < 0 || ref_len < 0) return fail(-1, "mxm_consensus: bad shape");
    const int64_t n = (int64_t)n_labels * ref_len;
    if (n == 0) return 0;
    if (cons == nullptr || (counts == nullptr && L > 0)) return fail(-1, "mxm_consensus: counts and cons are required");
    if ((reinterpret_cast<uintptr_t>(counts) & 15) != 0) return fail(-1, "mxm_consensus: counts must be 16-byte aligned");
    hipLaunchKernelGGL(consensus_kernel, dim3(clamp_grid((n + ASM_THREADS - 1) / ASM_THREADS, num_cu() * 8)),
                       dim3(ASM_THREADS), 0, (hipStream_t)stream, counts, n_labels, L, ref_len, min_cov, (int)(strict != 0),
                       cons, tied, n_tied);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int asm_rows_from(const char *name, const int32_t *rows_host, int32_t n_use, int64_t n_rows, asm_rows *out) {
    if (n_use < 0 || (n_use > 0 && rows_host == nullptr)) return fail(-1, "%s: bad participating rows", name);
    if (n_use > ASM_MAX_USE)
        return fail(-1, "%s: %d participating contributors, at most %d (an owner is an int8)", name, n_use, ASM_MAX_USE);
    memset(out, 0, sizeof(*out));
    for (int k = 0; k < n_use; ++k) {
        if (rows_host[k] < 0 || rows_host[k] >= n_rows) return fail(-1, "%s: participating row %d is no row", name, rows_host[k]);
        out->row[k] = rows_host[k];
    }
    return 0;
}

extern "C" int mxm_new_variants(const uint8_t *cons, int64_t ld, int32_t n_rows, const int32_t *rows_host, int32_t n_use,
                                int64_t ref_len, uint32_t *newvar, uint32_t *n_new, void *stream) {
    if (ref_len < 0 || ld < ref_len || n_rows < 0) return fail(-1, "mxm_new_variants: bad shape");
    asm_rows rows;
    RC_TRY(asm_rows_from("mxm_new_variants", rows_host, n_use, n_rows, &rows));
    if (ref_len == 0) return 0;
    if (newvar == nullptr || n_new == nullptr || (cons == nullptr && n_use > 0))
        return fail(-1, "mxm_new_variants: cons, newvar and n_new are required");
    hipLaunchKernelGGL(new_variants_kernel, dim3(clamp_grid((ref_len + ASM_THREADS - 1) / ASM_THREADS, num_cu() * 8)),
                       dim3(ASM_THREADS), 0, (hipStream_t)stream, cons, ld, rows, n_use, ref_len, newvar, n_new);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mxm_first_observed(const mxm_aln_columns *cols, const int32_t *label, const int32_t *joined,
                                  int32_t n_labels, int32_t min_mq, int32_t min_bq, int64_t ref_len, const uint8_t *tied,
                                  uint8_t *cons, void *stream) {
    const char *name = "mxm_first_observed";
    RC_TRY(aln_columns_ok(name, cols));
    if (n_labels < 0 || ref_len < 0) return fail(-1, "%s: bad shape", name);
    const int64_t n = cols->n_aln, cells = (int64_t)n_labels * ref_len;
    if (n == 0 || cells == 0) return 0;
    if (label == nullptr || tied == nullptr || cons == nullptr) return fail(-1, "%s: label, tied and cons are required", name);
    hipStream_t s = (hipStream_t)stream;
    // scratch: first[cells][8] order keys (the size of the counts tables the consensus was called from)
    unsigned long long err_host;
    const size_t bytes = (size_t)cells * 8 * 8;
    HIP_TRY(aln_pass(s, bytes, &err_host, [&](void *scratch, unsigned long long *err) {
        unsigned long long *first = static_cast<unsigned long long *>(scratch);
        const hipError_t e = hipMemsetAsync(first, 0xff, bytes, s);                   // ASM_KEY_NONE
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(first_observed_kernel, dim3(clamp_grid(((n + 63) / 64 + 7) / 8, num_cu() * 4)),
                           dim3(ASM_WALK_THREADS), 0, s, aln_view_of(cols, min_mq, min_bq), label, joined, n_labels, ref_len,
                           tied, first, err);
        hipLaunchKernelGGL(first_resolve_kernel, dim3(clamp_grid((cells + ASM_THREADS - 1) / ASM_THREADS, num_cu() * 8)),
                           dim3(ASM_THREADS), 0, s, tied, first, cells, cons);
        return hipGetLastError();
    }));
    return aln_walk_error(name, err_host, "has a label >= n_labels");
}

extern "C" int mxm_extend_assign(const mxm_aln_columns *cols, int32_t *label, int32_t *joined, int32_t unassigned,
                                 int32_t n_rows, const int32_t *rows_host, int32_t n_use, int32_t round, int32_t min_mq,
                                 int32_t min_bq, const uint32_t *newvar, int64_t ref_len, int32_t *frag_state,
                                 int32_t *moved_owner, uint32_t *n_moved, void *stream) {
    const char *name = "mxm_extend_assign";
    RC_TRY(aln_columns_ok(name, cols));
    asm_rows rows;
    RC_TRY(asm_rows_from(name, rows_host, n_use, n_rows, &rows));
    if (ref_len < 0 || cols->n_frag < 0 || round < 0) return fail(-1, "%s: bad shape", name);
    const int64_t n = cols->n_aln, n_frag = cols->n_frag;
    if (n == 0) return 0;
    if (label == nullptr || joined == nullptr || cols->frag == nullptr || n_moved == nullptr ||
        (n_frag > 0 && frag_state == nullptr) || (ref_len > 0 && newvar == nullptr))
        return fail(-1, "%s: label, joined, frag, frag_state, newvar and n_moved are required", name);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long err_host;
    bool lds_refused = false;
    const hipError_t e = aln_pass(s, 0, &err_host, [&](void *, unsigned long long *err) {
        hipError_t st = hipSuccess;
        if (n_frag > 0) st = hipMemsetAsync(frag_state, 0xff, (size_t)n_frag * 4, s);  // ASM_FRAG_EMPTY
        if (st != hipSuccess) return st;
        // newvar in LDS when it fits: at most two workgroups per CU (each stages the whole table once and then walks many
        // alignments); else read from global memory
        const size_t lds = (size_t)ref_len * 4;
        const bool in_lds = lds <= ASM_LDS_MAX_BYTES;
        auto kernel = in_lds ? &extend_walk_kernel<true> : &extend_walk_kernel<false>;
        if (in_lds && lds > 65536) st = raise_dynamic_lds(reinterpret_cast<const void *>(kernel), lds, name);
        if (st != hipSuccess) {
            lds_refused = true;
            return st;
        }
        const int per_cu = !in_lds ? 4 : lds * 2 <= ASM_LDS_MAX_BYTES ? 2 : 1;
        hipLaunchKernelGGL(kernel, dim3(clamp_grid(((n + 63) / 64 + 7) / 8, num_cu() * per_cu)), dim3(ASM_WALK_THREADS),
                           in_lds ? lds : 0, s, aln_view_of(cols, min_mq, min_bq), cols->frag, label, unassigned, n_frag,
                           newvar, ref_len, frag_state, err);
        hipLaunchKernelGGL(extend_move_kernel, dim3(clamp_grid((n + ASM_THREADS - 1) / ASM_THREADS, num_cu() * 8)),
                           dim3(ASM_THREADS), 0, s, cols->frag, n, n_frag, unassigned, rows, n_use, round, frag_state, label,
                           joined, moved_owner, n_moved);
        return hipGetLastError();
    });
    if (lds_refused) return -2;                              // (raise_dynamic_lds wrote the message)
    HIP_TRY(e);
    return aln_walk_error(name, err_host, "has a fragment index outside [0, n_frag)");
}

// ------------------------------------------------------------------------------------------
// The extension for the samples of a cohort (assemble_samples_kernels.hpp; include/mixemt_hip_assemble_samples.h).  Every
// refusal comes before the first HIP call.  The host tables go into stream-ordered memory of the call's own through a
// pageable vector of the call's own, as mxm_check_variants_samples uploads its tables.
// ------------------------------------------------------------------------------------------
static_assert(ASM_MAX_USE == MXM_ASSEMBLE_SAMPLES_MAX_USE, "the header states the kernels' cap");

// The participants' tables of S > 0 samples: use_ptr_host monotone from a start >= 0, at most ASM_MAX_USE entries per
// sample, every entry in [0, limit).  *total = use_ptr_host[S], the entries of use_host that are uploaded.
static int asm_samples_tables_ok(const char *name, const int32_t *use_host, const int32_t *use_ptr_host, int32_t S,
                                 int64_t limit, int64_t *total) {
    if (use_ptr_host == nullptr) return fail(-1, "%s: bad arguments (use_ptr_host is required)", name);
    if (use_ptr_host[0] < 0) return fail(-1, "%s: use_ptr_host[0] = %d is negative", name, use_ptr_host[0]);
    for (int32_t s = 0; s < S; ++s) {
        const int32_t lo = use_ptr_host[s], hi = use_ptr_host[s + 1];
        if (hi < lo) return fail(-1, "%s: use_ptr_host decreases at sample %d (%d after %d)", name, s, hi, lo);
        if (hi - lo > ASM_MAX_USE)
            return fail(-1, "%s: sample %d has %d participants, at most %d (an owner is an int8)", name, s, hi - lo, ASM_MAX_USE);
    }
    *total = use_ptr_host[S];
    if (*total > 0 && use_host == nullptr) return fail(-1, "%s: bad arguments (use_host is required)", name);
    for (int32_t s = 0; s < S; ++s)
        for (int32_t k = use_ptr_host[s]; k < use_ptr_host[s + 1]; ++k)
            if (use_host[k] < 0 || use_host[k] >= limit)
                return fail(-1, "%s: sample %d: participant %d outside [0, %lld)", name, s, use_host[k], (long long)limit);
    return 0;
}

extern "C" int mxm_new_variants_samples(const uint8_t *cons, int64_t ld, int32_t n_rows, const int32_t *use_host,
                                        const int32_t *use_ptr_host, int32_t S, int64_t ref_len, uint32_t *newvar,
                                        uint32_t *n_new, void *stream) {
    const char *name = "mxm_new_variants_samples";
    if (S < 0) return fail(-1, "%s: S < 0 (%d)", name, S);
    if (ref_len < 0 || ld < ref_len || n_rows < 0)
        return fail(-1, "%s: bad shape (ref_len = %lld, ld = %lld, n_rows = %d)", name, (long long)ref_len, (long long)ld, n_rows);
    if (S == 0) return 0;
    int64_t total = 0;
    RC_TRY(asm_samples_tables_ok(name, use_host, use_ptr_host, S, n_rows, &total));
    if (ref_len == 0 || use_ptr_host[S] == use_ptr_host[0]) return 0;
    if (cons == nullptr || newvar == nullptr || n_new == nullptr)
        return fail(-1, "%s: bad arguments (cons, newvar and n_new are required)", name);
    hipStream_t st = (hipStream_t)stream;
    // use_ptr[S + 1], then use[total]
    static thread_local std::vector<int32_t> staged;
    staged.assign(use_ptr_host, use_ptr_host + (size_t)S + 1);
    staged.insert(staged.end(), use_host, use_host + (size_t)total);
    int32_t *tables = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&tables), staged.size() * sizeof(int32_t), st));
    hipError_t e = hipMemcpyAsync(tables, staged.data(), staged.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const int gx = clamp_grid((ref_len + ASM_THREADS - 1) / ASM_THREADS, num_cu() * 8);
        hipLaunchKernelGGL(new_variants_samples_kernel, dim3((unsigned)gx, (unsigned)(S < 65535 ? S : 65535)), dim3(ASM_THREADS),
                           0, st, cons, ld, (const int32_t *)(tables + S + 1), (const int32_t *)tables, S, ref_len, newvar, n_new);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(tables, st);
    HIP_TRY(e);
    HIP_TRY(ef);
    return 0;
}

extern "C" int mxm_extend_assign_samples(const mxm_aln_columns *cols, const int32_t *aln_sample, int32_t *label,
                                         int32_t *joined, const int32_t *unassigned_host, const int32_t *use_host,
                                         const int32_t *use_ptr_host, int32_t S, int32_t n_labels, int32_t round,
                                         int32_t min_mq, int32_t min_bq, const uint32_t *newvar, int64_t ref_len,
                                         int32_t *frag_state, int32_t *moved_owner, uint32_t *n_moved, void *stream) {
    const char *name = "mxm_extend_assign_samples";
    RC_TRY(aln_columns_ok(name, cols));
    if (S < 0) return fail(-1, "%s: S < 0 (%d)", name, S);
    if (n_labels < 0 || ref_len < 0 || cols->n_frag < 0 || round < 0)
        return fail(-1, "%s: bad shape (n_labels = %d, ref_len = %lld, n_frag = %lld, round = %d)", name, n_labels,
                    (long long)ref_len, (long long)cols->n_frag, round);
    int64_t total = 0;
    const int32_t zero = 0;
    if (S > 0) {
        if (unassigned_host == nullptr) return fail(-1, "%s: bad arguments (unassigned_host is required)", name);
        RC_TRY(asm_samples_tables_ok(name, use_host, use_ptr_host, S, n_labels, &total));
        for (int32_t s = 0; s < S; ++s)
            if (unassigned_host[s] >= n_labels)
                return fail(-1, "%s: sample %d: unassigned label %d outside [0, %d)", name, s, unassigned_host[s], n_labels);
    } else {
        use_ptr_host = &zero;                                // (no sample: one offset, no entries)
    }
    const int64_t n = cols->n_aln, n_frag = cols->n_frag;
    if (n == 0) return 0;
    if (label == nullptr || joined == nullptr || cols->frag == nullptr || aln_sample == nullptr || n_moved == nullptr ||
        (n_frag > 0 && frag_state == nullptr) || (S > 0 && ref_len > 0 && newvar == nullptr))
        return fail(-1, "%s: bad arguments (label, joined, frag, aln_sample, frag_state, newvar and n_moved are required)", name);
    hipStream_t s = (hipStream_t)stream;
    // the tables as one upload: unassigned[S], use_ptr[S + 1], use[total]
    static thread_local std::vector<int32_t> staged;
    staged.assign(unassigned_host, unassigned_host + (size_t)S);
    staged.insert(staged.end(), use_ptr_host, use_ptr_host + (size_t)S + 1);
    staged.insert(staged.end(), use_host, use_host + (size_t)total);
    unsigned long long err_host;
    const size_t bytes = staged.size() * sizeof(int32_t);
    HIP_TRY(aln_pass(s, bytes, &err_host, [&](void *scratch, unsigned long long *err) {
        int32_t *un_d = static_cast<int32_t *>(scratch), *ptr_d = un_d + S, *use_d = ptr_d + S + 1;
        hipError_t st = hipMemcpyAsync(un_d, staged.data(), bytes, hipMemcpyHostToDevice, s);
        if (st == hipSuccess && n_frag > 0) st = hipMemsetAsync(frag_state, 0xff, (size_t)n_frag * 4, s);   // ASM_FRAG_EMPTY
        if (st != hipSuccess) return st;
        hipLaunchKernelGGL(extend_walk_samples_kernel, dim3(clamp_grid(((n + 63) / 64 + 7) / 8, num_cu() * 4)),
                           dim3(ASM_WALK_THREADS), 0, s, aln_view_of(cols, min_mq, min_bq), cols->frag, (const int32_t *)label,
                           aln_sample, S, (const int32_t *)un_d, (const int32_t *)use_d, (const int32_t *)ptr_d, n_frag, newvar,
                           ref_len, frag_state, err);
        hipLaunchKernelGGL(extend_move_samples_kernel, dim3(clamp_grid((n + ASM_THREADS - 1) / ASM_THREADS, num_cu() * 8)),
                           dim3(ASM_THREADS), 0, s, cols->frag, n, n_frag, aln_sample, S, (const int32_t *)un_d,
                           (const int32_t *)use_d, (const int32_t *)ptr_d, round, (const int32_t *)frag_state, label, joined,
                           moved_owner, n_moved);
        return hipGetLastError();
    }));
    char kind0[64];
    snprintf(kind0, sizeof(kind0), "has a sample outside [0, %d)", S);
    return aln_walk_error(name, err_host, "has a fragment index outside [0, n_frag)", kind0);
}

// ------------------------------------------------------------------------------------------
// mixemt's -t tables as text (stats_text_kernels.hpp; include/mixemt_hip_stats_samples.h).  Every refusal comes before the
// first HIP call.  The host tables go into stream-ordered memory of the call's own through a pageable vector of the call's
// own, as mxm_new_variants_samples uploads its tables.
// ------------------------------------------------------------------------------------------
static_assert(STATS_TILE == MXM_STATS_TILE_LINES && STATS_MAX_PREFIX == MXM_STATS_MAX_PREFIX, "the header states the kernels' sizes");

static int64_t stats_tiles_per_block(int64_t n_pos) { return (n_pos + STATS_TILE - 1) / STATS_TILE; }

extern "C" int64_t mxm_stats_text_tiles(int32_t n_blocks, int64_t n_pos) {
    if (n_blocks < 0 || n_pos < 0 || n_pos > (int64_t)INT32_MAX - 1) return -1;
    const int64_t tiles = (int64_t)n_blocks * stats_tiles_per_block(n_pos);
    return tiles > (int64_t)INT32_MAX ? -1 : tiles;
}

// The checks both entries share; *n_tiles: the tiles of the text (0: nothing to do).
static int stats_text_ok(const char *name, const mxm_stats_text *t, int64_t *n_tiles) {
    if (t == nullptr) return fail(-1, "%s: bad arguments (the mxm_stats_text is required)", name);
    if (t->n_blocks < 0 || t->n_pos < 0)
        return fail(-1, "%s: bad shape (n_blocks = %d, n_pos = %lld)", name, t->n_blocks, (long long)t->n_pos);
    if (t->kind != 0 && t->kind != 1) return fail(-1, "%s: unknown kind %d (0: obs.tab lines, 1: pos.tab lines)", name, t->kind);
    *n_tiles = mxm_stats_text_tiles(t->n_blocks, t->n_pos);
    if (*n_tiles < 0)
        return fail(-1, "%s: %d blocks of %lld lines are more than the tile index holds (n_pos <= 2^31 - 2, at most 2^31 - 1 "
                        "tiles of %d lines)", name, t->n_blocks, (long long)t->n_pos, STATS_TILE);
    if (*n_tiles == 0) return 0;
    if (t->table_host == nullptr) return fail(-1, "%s: bad arguments (table_host is required)", name);
    for (int32_t b = 0; b < t->n_blocks; ++b)
        if (((uintptr_t)t->table_host[b] & 15) != 0) return fail(-1, "%s: the table of block %d is not 16-byte aligned", name, b);
    if (t->kind == 0) {
        const int64_t *ptr = t->prefix_ptr_host;
        if (ptr == nullptr) return fail(-1, "%s: bad arguments (prefix_ptr_host is required)", name);
        if (ptr[0] < 0) return fail(-1, "%s: prefix_ptr_host[0] = %lld is negative", name, (long long)ptr[0]);
        for (int32_t b = 0; b < t->n_blocks; ++b) {
            if (ptr[b + 1] < ptr[b])
                return fail(-1, "%s: prefix_ptr_host decreases at block %d (%lld after %lld)", name, b, (long long)ptr[b + 1],
                            (long long)ptr[b]);
            if (ptr[b + 1] - ptr[b] > STATS_MAX_PREFIX)
                return fail(-1, "%s: block %d has a prefix of %lld bytes, at most %d (the lines are staged in LDS)", name, b,
                            (long long)(ptr[b + 1] - ptr[b]), STATS_MAX_PREFIX);
        }
        if (ptr[t->n_blocks] > ptr[0] && t->prefix_host == nullptr)
            return fail(-1, "%s: bad arguments (prefix_host is required)", name);
    } else if (t->poly == nullptr || t->thr == nullptr || t->tail_ptr == nullptr) {
        return fail(-1, "%s: bad arguments (poly, thr and tail_ptr are required)", name);
    }
    return 0;
}

// The host tables as ONE upload: table[n_blocks] pointers, then (kind 0) prefix_ptr[n_blocks + 1] re-based to 0 and the
// prefixes' bytes.  `f` enqueues the kernels over the view; the tables are freed behind them in stream order.
template <typename F>
static int stats_text_launch(const mxm_stats_text *t, hipStream_t st, F &&f) {
    static thread_local std::vector<uint64_t> staged;
    const size_t nb = (size_t)t->n_blocks;
    staged.assign(nb, 0);
    for (size_t b = 0; b < nb; ++b) staged[b] = (uint64_t)(uintptr_t)t->table_host[b];
    size_t prefix_bytes = 0;
    if (t->kind == 0) {
        const int64_t lo = t->prefix_ptr_host[0];
        prefix_bytes = (size_t)(t->prefix_ptr_host[nb] - lo);
        for (size_t b = 0; b <= nb; ++b) staged.push_back((uint64_t)(t->prefix_ptr_host[b] - lo));
        staged.resize(staged.size() + (prefix_bytes + 7) / 8, 0);
        if (prefix_bytes) memcpy(staged.data() + 2 * nb + 1, t->prefix_host + lo, prefix_bytes);
    }
    uint64_t *tables = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void **>(&tables), staged.size() * sizeof(uint64_t), st));
    hipError_t e = hipMemcpyAsync(tables, staged.data(), staged.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        stats_text_view v;
        v.kind = t->kind, v.n_blocks = t->n_blocks, v.n_pos = t->n_pos;
        v.tiles_per_block = (int32_t)stats_tiles_per_block(t->n_pos);
        v.table = reinterpret_cast<const uint32_t *const *>(tables);
        v.prefix_ptr = t->kind == 0 ? reinterpret_cast<const int64_t *>(tables + nb) : nullptr;
        v.prefix = t->kind == 0 ? reinterpret_cast<const uint8_t *>(tables + 2 * nb + 1) : nullptr;
        v.poly = t->poly, v.thr = t->thr, v.tail = t->tail, v.tail_ptr = t->tail_ptr;
        f(v);
        e = hipGetLastError();
    }
    const hipError_t ef = hipFreeAsync(tables, st);
    HIP_TRY(e);
    HIP_TRY(ef);
    return 0;
}

extern "C" int mxm_stats_text_sizes(const mxm_stats_text *t, int64_t *tile_off, void *stream) {
    const char *name = "mxm_stats_text_sizes";
    int64_t n_tiles = 0;
    RC_TRY(stats_text_ok(name, t, &n_tiles));
    if (tile_off == nullptr) return fail(-1, "%s: bad arguments (tile_off is required)", name);
    hipStream_t st = (hipStream_t)stream;
    if (n_tiles == 0) {
        HIP_TRY(hipMemsetAsync(tile_off, 0, sizeof(int64_t), st));
        return 0;
    }
    return stats_text_launch(t, st, [&](const stats_text_view &v) {
        hipLaunchKernelGGL(stats_text_sizes_kernel, dim3(clamp_grid(n_tiles, num_cu() * 32)), dim3(STATS_TILE), 0, st, v, n_tiles,
                           tile_off);
        hipLaunchKernelGGL(stats_text_scan_kernel, dim3(1), dim3(STATS_SCAN_THREADS), 0, st, tile_off, n_tiles);
    });
}

extern "C" int mxm_stats_text_write(const mxm_stats_text *t, const int64_t *tile_off, uint8_t *out, int64_t out_bytes,
                                    uint32_t *err, void *stream) {
    const char *name = "mxm_stats_text_write";
    int64_t n_tiles = 0;
    RC_TRY(stats_text_ok(name, t, &n_tiles));
    if (out_bytes < 0) return fail(-1, "%s: out_bytes < 0 (%lld)", name, (long long)out_bytes);
    if (out == nullptr && out_bytes > 0) return fail(-1, "%s: bad arguments (out is NULL with out_bytes = %lld)", name, (long long)out_bytes);
    if (tile_off == nullptr || err == nullptr) return fail(-1, "%s: bad arguments (tile_off and err are required)", name);
    if (n_tiles == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    return stats_text_launch(t, st, [&](const stats_text_view &v) {
        hipLaunchKernelGGL(stats_text_write_kernel, dim3(clamp_grid(n_tiles, num_cu() * 32)), dim3(STATS_TILE), 0, st, v, n_tiles,
                           tile_off, out, out_bytes, err);
    });
}
