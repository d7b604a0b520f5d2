"""
Every kernel instance the host side compiles through dispatch_width<MAX> (mixemt_amd/csrc/mixemt_hip.hip), as a table:
per dispatch site the host's formula from the matrix width H (or coded_ld(H)) to the instance number RESTATED here, the
entry's own constraints on H, and per instance the first and the last width that reach it.  Plain Python: reads no
library, only the csrc sources -- every constant comes from them by regex (as tests/test_var_check_host.py reads
MXM_VAR_CHECK_MAX_L), so a retune moves the edges with it and cannot leave the sweep on stale widths.

    SITES                 {name: Site}: entry, kernel, where the dispatch stands (host function, n-th dispatch in it),
                          the condition beyond the width under which the entry takes this kernel
    classes(site)         [Class(instance, first, last)] in ascending width
    edge_cases(name)      [(instance, width)] -- first and last width of every class, for pytest.mark.parametrize
    rows_for(instance)    3, 37 or 64 rows, picked by the instance number (a one-wave sample, an odd count, a full
                          64 rows) -- every case of tests/test_gpu_instances.py is ONE call on at most 64 rows
    dispatch_sites()      [(host function, n-th dispatch in it, MAX as written)] found in mixemt_hip.hip
    stream_kernel_name(H, nb)   what mxm_describe_stream_kernel must say

tests/test_instances.py checks the table on the CPU (partition of the supported range, instance counts against the
MAX the source names, every dispatch site covered); tests/test_gpu_instances.py runs every instance at both edges.

Sites whose instance is NOT picked by the width are listed with `by_width = False` and swept elsewhere:
  * the rows-per-thread instances of the one-launch loops depend on the row count and the CU count:
    em_fused_cols_kernel<CP, RPT> RPT = ceil(R / FCOLS_THREADS) (1 .. 3), em_fused_narrow_kernel<HMAX, RPT>
    RPT = 1, 2, 4, 8 = ceil(R / (grid * FNARROW_THREADS)) rounded up to a power of two.  tests/test_gpu_fused.py reaches
    RPT = 1, 2 and 3 of the columns-split loop (64, 1024 and 1025 x 5408: <22, 1 / 2 / 3>; 1536 x 3072: <12, 3>;
    257 x 6144 and 513 x 6100: <24, 1 / 2>); tests/test_gpu_narrow_loop.py reaches, on 256 CUs, <4, 1>, <8, 1>, <16, 1>
    (its small shapes), <4, 4> (300 000 x 4), <4, 8> (10^6 x 3) and <8, 4> (400 000 x 7) -- RPT = 2 of the narrow loop
    (131 073 .. 262 144 rows) is reached by NO test.  The sweep here runs RPT = 1 only (at most 64 rows) and adds no
    large-R case;
  * the cohort's narrow kernels (dispatch_width<SFIN_KMAX> on ld = 4, 8 or 16 padded contributor columns):
    the loops' and the assignment's own modules take ld = 4, 8 and 16 as a parameter (tests/test_gpu_samples_runs.py,
    test_gpu_bootstrap.py, test_gpu_support.py, test_gpu_accuracy_consumers.py::test_assign_reads_of_samples).
Three sites depend on the DEVICE as well (256 CUs on the MI355X): the columns-split loop needs a grid of exactly 256
workgroups and picks CP from ceil(H / 256); the records loop's grid is min(2 CUs, 5.2 sqrt(R) rounded up to 8, R)
workgroups and a column slice of at most 16 * FCODED_MAX_M pairs per workgroup bounds the width from above at a given R
(64 rows: 48 workgroups, H <= 6144; 37 rows: 32, H <= 4096; 3 rows: 3, H <= 384) -- its instances 7 and 8 need more than
64 rows and are left to tests/test_gpu_coded.py (513 x 8192).  `cus` below is the MI355X's.
"""
import collections
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mixemt_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
HOST = "mixemt_hip.hip"
CUS = 256                                            # the MI355X (the device-dependent sites only)

_texts = {}


def source(name=HOST):
    if name not in _texts:
        with open(os.path.join(CSRC, name)) as src:
            _texts[name] = src.read()
    return _texts[name]


def _all_sources():
    out = []
    for folder in (CSRC, INCLUDE):
        for name in sorted(os.listdir(folder)):
            if name.endswith((".hpp", ".hip", ".h")):
                with open(os.path.join(folder, name)) as src:
                    out.append(src.read())
    return out


def _eval_int(expr, depth=0):
    """An integer #define: a literal, a product / sum of literals and other defines, or (A == n ? x : y)."""
    expr = expr.strip()
    while expr.startswith("(") and expr.endswith(")") and expr.count("(") == 1:
        expr = expr[1:-1].strip()
    tern = re.match(r"^(\w+)\s*==\s*(\d+)\s*\?\s*(\d+)\s*:\s*(\d+)$", expr)
    if tern:
        return int(tern.group(3)) if const(tern.group(1)) == int(tern.group(2)) else int(tern.group(4))
    assert re.match(r"^[\w\s*+()-]+$", expr) and depth < 4, expr
    names = {n: const(n) for n in set(re.findall(r"[A-Za-z_]\w*", expr))}
    return int(eval(expr, {"__builtins__": {}}, names))     # (digits, defines, + - * and brackets only: checked above)


_consts = {}


def const(name):
    """#define NAME <integer expression> from the csrc sources (the first definition: the #ifndef defaults)."""
    if name not in _consts:
        for text in _all_sources():
            hit = re.search(r"^\s*#define\s+%s\s+([^\n/]+?)\s*(?://.*)?$" % re.escape(name), text, re.M)
            if hit:
                _consts[name] = _eval_int(hit.group(1))
                break
        else:
            raise KeyError("no #define %s in csrc" % name)
    return _consts[name]


def _search(pattern, what):
    hit = re.search(pattern, source(), re.S)
    assert hit, "mixemt_hip.hip no longer holds %s" % what
    return hit


def max_nch_list():
    """batch_fits' spill-free chunk counts per tile size: {0, 16, 8, 7, 6}."""
    hit = _search(r"static const int max_nch\[MXM_MAX_BT \+ 1\]\s*=\s*\{([^}]*)\}", "batch_fits' max_nch list")
    vals = [int(v) for v in hit.group(1).split(",")]
    assert len(vals) == const("MXM_MAX_BT") + 1
    return vals


def coded_shape_threads():
    hit = _search(r"g_coded_shapes\[\]\s*=\s*\{\{(\d+),\s*(\d+),\s*(\d+)\}\}", "the records pass's shape")
    assert _search(r"launch_coded<(\d+),\s*\d+,\s*\d+>\(nch", "launch_coded's instance").group(1) == hit.group(1)
    return int(hit.group(1))


def linear_range():
    """mxm_linear_supported: MXM_LINEAR_MIN_H <= H <= 8192."""
    hit = _search(r"mxm_linear_supported\(int32_t H\)\s*\{\s*return \(H >= MXM_LINEAR_MIN_H && H <= (\d+)\)", "mxm_linear_supported")
    return const("MXM_LINEAR_MIN_H"), int(hit.group(1))


def wide_rows_range():
    """wide_rows_ok: an even H in [64, 8192] (beside the alignment of the pointer and an even ld)."""
    hit = _search(r"wide_rows_ok\(.*?H >= (\d+) && H <= (\d+);", "wide_rows_ok")
    return int(hit.group(1)), int(hit.group(2))


def estep_wide_caps():
    """mxm_em_step's spill-free chunk counts: (with colsum, without)."""
    hit = _search(r"nch <= \(colsum != nullptr \? (\d+) : (\d+)\)", "mxm_em_step's register budget")
    return int(hit.group(1)), int(hit.group(2))


def build_max_h():
    hit = _search(r"build_lut_impl\(.*?if \(H > (\d+)\)", "build_lut_impl's width check")
    hit2 = _search(r"build_sparse_impl\(.*?if \(H > (\d+)\)", "build_sparse_impl's width check")
    assert hit.group(1) == hit2.group(1)
    return int(hit.group(1))


# ---------------------------------------------------------------- the host's arithmetic, restated
def ceil_div(a, b):
    return (a + b - 1) // b


def coded_ld(n_haps):
    return (n_haps + 7) & ~7


def variant_threads(nb):
    """stream_linear_tile: one restart takes the second single-restart shape (MXM_V1B_*), a tile MXM_V<nb>_*."""
    return const("MXM_V1B_THREADS") if nb == 1 else const("MXM_V%d_THREADS" % nb)


def variant_nbuf(nb):
    return const("MXM_V1B_NBUF") if nb == 1 else const("MXM_V%d_NBUF" % nb)


def variant_preg(nb):
    return 1 if nb == 1 else const("MXM_V%d_PREG" % nb)


def stream_nch(n_haps, nb):
    return ceil_div(ceil_div(n_haps, 2), variant_threads(nb))


def batch_fits(n_haps, nb):
    """A tile of nb restarts: a spill-free instance and its LDS-resident proportions inside MXM_LDS_BUDGET."""
    if nb <= 1:
        return True
    nch = stream_nch(n_haps, nb)
    lds = (nb - variant_preg(nb)) * nch * variant_threads(nb) * 16
    return nch <= max_nch_list()[nb] and lds <= const("MXM_LDS_BUDGET")


def stream_kernel_name(n_haps, nb):
    return "em_iter_wide_kernel<%d, %d, %d, %d, %d>" % (variant_threads(nb), stream_nch(n_haps, nb), nb, variant_nbuf(nb),
                                                      variant_preg(nb))


def fused_coded_grid(n_rows, cus=CUS):
    """fused_coded_grid at the default knobs."""
    nwg = min(cus * 2, const("MXM_MAX_WG"))
    best = (int(5.2 * float(n_rows) ** 0.5) + 7) & ~7
    nwg = min(nwg, best, n_rows)
    return max(nwg, 1)


def rows_for(instance):
    return (3, 37, 64)[instance % 3]


# ---------------------------------------------------------------- the table
Class = collections.namedtuple("Class", "instance first last")


class Site(object):
    """One dispatch_width site.  supported(H): the entry takes THIS kernel at width H (its own constraints and the
    host's narrowing); instance(H): the template instance.  where = (host function, n-th dispatch_width call in it).
    count_from: how the number of instances follows from the source -- "MAX" (the dispatch's own maximum) or a short
    statement of the named constant / narrowing that makes it fewer, with its value in `count`."""

    def __init__(self, entry, kernel, where, supported, instance, count, count_from="MAX", condition="", by_width=True,
                 lo=1, hi=8192, first=1):
        self.entry, self.kernel, self.where = entry, kernel, where
        self.supported, self.instance = supported, instance
        self.count, self.count_from, self.condition, self.by_width = count, count_from, condition, by_width
        self.lo, self.hi, self.first = lo, hi, first            # (first: the lowest instance any supported width reaches)


def _linear(n_haps):
    lo, hi = linear_range()
    return lo <= n_haps <= hi


def _linear_even(n_haps):
    return _linear(n_haps) and n_haps % 2 == 0


def _wide_rows(n_haps):
    lo, hi = wide_rows_range()
    return lo <= n_haps <= hi and n_haps % 2 == 0


def _nch_coded(threads):
    return lambda n_haps: ceil_div(coded_ld(n_haps) // 4, threads)


def _quad_ok(n_haps):
    return _linear(n_haps) and _nch_coded(const("QUAD_THREADS"))(n_haps) <= const("QUAD_MAX_NCH")


def _half_chunks(n_haps):
    return (n_haps // 2 + 255) // 256                 # linearize_wide, mxm_em_step, mxm_row_argmax_votes: literal 256


def _stream_site(nb):
    threads = variant_threads(nb)
    cap = min(16, const("MXM_MAX_COL2") // threads, max_nch_list()[nb] if nb > 1 else 16)
    return Site("mxm_em_iter, a tile of %d restart%s" % (nb, "" if nb == 1 else "s"),
                "em_iter_wide_kernel<%d, NCH, %d, %d, %d>" % (threads, nb, variant_nbuf(nb), variant_preg(nb)),
                ("dispatch_wide", 0), lambda h, nb=nb: _linear(h) and batch_fits(h, nb), lambda h, nb=nb: stream_nch(h, nb),
                cap, "min(MAX, MXM_MAX_COL2 / threads, max_nch[%d], the LDS budget)" % nb,
                "P given (ldp even), B = %d and batch_fits(H, %d)" % (nb, nb))


def _sites():
    s = collections.OrderedDict()
    lut_cols = const("LUT_THREADS") * const("LUT_CPL")
    s["build_lut"] = Site("mxm_build_em_matrix_lut", "build_lut_kernel<NT, LUT_CPL>", ("build_lut_impl", 0),
                          lambda h: 1 <= h <= build_max_h(), lambda h: ceil_div(h, lut_cols), 8,
                          condition="tables that qualify for the lookup table (at most 14 distinct bases)")
    spb = const("SPB_THREADS")
    s["build_sparse"] = Site("mxm_build_em_matrix_sparse", "build_sparse_kernel<N, P, false, 1>",
                             ("build_sparse_impl", 0), lambda h: 1 <= h <= build_max_h(),
                             lambda h: ceil_div(((h + 1) & ~1) // 2, spb), 16,
                             condition="rows of up to 64 observations")
    s["build_sparse_long"] = Site("mxm_build_em_matrix_sparse",
                                  "build_sparse_kernel<N, ceil(N / SPB_LONG_KPP), false, 2>", ("build_sparse_impl", 1),
                                  lambda h: 1 <= h <= build_max_h(), lambda h: ceil_div(((h + 1) & ~1) // 2, spb), 16,
                                  condition="rows of 65 .. 128 observations, mxm_set_sparse_long_rows left on")
    for long_rows in (False, True):
        s["build_records_long" if long_rows else "build_records"] = Site(
            "mxm_build_em_records", "build_sparse_kernel<N, %s, true, %d>" % (("ceil(N / SPB_LONG_KPP)", 2) if long_rows else ("P", 1)),
            ("build_sparse_impl", 1 if long_rows else 0), _linear, lambda h: ceil_div(((h + 1) & ~1) // 2, spb), 16,
            condition="the records entry (out != NULL): " + ("rows of 65 .. 128 observations" if long_rows else "rows of up to 64 observations"))
    s["linearize"] = Site("mxm_linearize", "linearize_wide_kernel<NCH, double>", ("linearize_wide", 0), _wide_rows, _half_chunks, 16,
                          condition="H even, ldm even, M and P 16-byte aligned (else the any-shape linearize_kernel)")
    s["linearize_f32"] = Site("mxm_linearize_f32", "linearize_wide_kernel<NCH, float>", ("linearize_wide", 0), _wide_rows, _half_chunks, 16,
                              condition="H even, ldm even, M 16-byte and P 8-byte aligned, ldp a multiple of 4 (else linearize_f32_kernel)")
    for nb in range(1, const("MXM_MAX_BT") + 1):
        s["em_iter_b%d" % nb] = _stream_site(nb)
    v1 = const("MXM_V1_THREADS")
    wide_max = const("ENC_MAX_WIDE")
    s["em_iter_rest"] = Site("mxm_em_iter_coded, the dense rest of a records plan",
                             "em_iter_wide_kernel<%d, NCH, 1, %d, 1>" % (v1, const("MXM_V1_NBUF")), ("dispatch_wide", 0),
                             lambda h: _linear(h) and h > wide_max, lambda h: ceil_div(ceil_div(h, 2), v1),
                             min(16, const("MXM_MAX_COL2") // v1) - ceil_div(ceil_div(wide_max, 2), v1),
                             "min(MAX, MXM_MAX_COL2 / MXM_V1_THREADS) less the instances of H <= ENC_MAX_WIDE: a row of at most 1024 "
                             "columns always gets a record, so no records plan has a dense rest there",
                             "R_rest > 0: a row of more than ENC_MAX_WIDE = 1024 distinct values", first=ceil_div(ceil_div(wide_max + 1, 2), v1))
    f32 = const("MXM_F32_THREADS")
    s["em_iter_f32"] = Site("mxm_em_iter_f32", "em_iter_wide_f32_kernel<%d, NCH, %d>" % (f32, const("MXM_F32_NBUF")),
                            ("em_iter_f32_one", 0), _linear, lambda h: ceil_div(ceil_div(h, 4), f32), min(8, 2048 // f32),
                            "min(MAX, 2048 / MXM_F32_THREADS)", "ldp a multiple of 4")
    enc = const("ENC_THREADS")
    s["encode_rows"] = Site("mxm_encode_rows (read back through mxm_decode_rows)", "encode_rows_kernel<NCH>, encode_wide_rows_kernel<NCH>",
                            ("mxm_encode_rows", 0), _linear, _nch_coded(enc), 8, condition="M 8-byte aligned")
    s["argmax_coded"] = Site("mxm_row_argmax_votes_coded", "records_argmax_narrow_kernel<NCH>, records_argmax_kernel<NCH, true>",
                             ("mxm_row_argmax_votes_coded", 0), _linear, _nch_coded(256), 8,
                             condition="n_runs == 1 (several runs: posterior_argmax_kernel, any width)")
    ct = coded_shape_threads()
    s["em_iter_coded"] = Site("mxm_em_iter_coded, no quad dictionary", "em_iter_coded_kernel<%d, NCH, 4, 2>" % ct, ("launch_coded", 0),
                              _linear, _nch_coded(ct), min(8, 2048 // ct), "min(MAX, 2048 / threads)", "c->qrec == NULL")
    qt = const("QUAD_THREADS")
    s["quad"] = Site("mxm_em_iter_coded, every row a quad row", "em_iter_quad_kernel<NCH, 4>", ("launch_quad", 0), _quad_ok,
                     _nch_coded(qt), const("QUAD_MAX_NCH"), "QUAD_MAX_NCH",
                     "a quad dictionary attached, n_quad_rows > 0, no byte-coded or wide row left over, B != 3 per tile")
    s["quad_coded"] = Site("mxm_em_iter_coded, quad rows beside leftover rows", "em_iter_quad_coded_kernel<NCH, 4>",
                           ("launch_quad_coded", 0), lambda h: _quad_ok(h) and h > const("ENC_MAX_CODES"), _nch_coded(qt),
                           const("QUAD_MAX_NCH"), "QUAD_MAX_NCH",
                           "a quad dictionary attached, n_quad_rows > 0 and byte-coded rows without quads or wide rows beside them: from 257 "
                           "columns (a narrower row is byte-coded with at most 64 quads -- always a quad row)")
    s["quad_batched"] = Site("mxm_em_iter_coded, three restarts per pass", "em_iter_quad_batched_kernel<QB_BT, NCH, 1 and 6>",
                             ("em_iter_coded_batched", 0), _quad_ok, lambda h: (_nch_coded(qt)(h) + 1) // 2, 3,
                             condition="a quad dictionary attached, n_quad_rows > 0, B = QB_BT = 3 (mxm_set_coded_batch_tile left at 3)")
    st = const("SAMPLES_THREADS")
    s["samples"] = Site("mxm_em_iter_samples", "em_iter_samples_kernel<NCH, 4>", ("samples_enqueue_pass", 0),
                        lambda h: _linear(h) and h % 2 == 0 and h >= 66, _nch_coded(st), 8,
                        condition="records without a quad dictionary and without a dense rest")
    with_t, without = estep_wide_caps()
    s["em_step"] = Site("mxm_em_step, the posterior alone", "estep_wide_kernel<NCH, false>", ("mxm_em_step", 0),
                        lambda h: _linear_even(h) and _half_chunks(h) <= without, _half_chunks, without,
                        "the register budget named in mxm_em_step (13 chunks without the M-step sums)",
                        "H even, ldm and ldo even, M and out 16-byte aligned, colsum == NULL (wider: estep_log_kernel)")
    s["em_step_colsum"] = Site("mxm_em_step with colsum", "estep_wide_kernel<NCH, true>", ("mxm_em_step", 0),
                               lambda h: _linear_even(h) and _half_chunks(h) <= with_t, _half_chunks, with_t,
                               "the register budget named in mxm_em_step (10 chunks with the M-step sums)",
                               "as above, colsum given")
    s["argmax"] = Site("mxm_row_argmax_votes", "row_argmax_wide_kernel<NCH>", ("mxm_row_argmax_votes", 0), _wide_rows, _half_chunks, 16,
                       condition="H even, ldx even, X 16-byte aligned (else row_argmax_votes_kernel)")
    # ---- the one-launch loops: mxm_set_loop_fused(1) / (2), so that a launch that cannot run is error -3
    ft = const("FUSED_THREADS")
    fmax = const("FUSED_MAX_NCH")
    s["fused_rows"] = Site("mxm_em_loop under mxm_set_loop_fused(2): rows split", "em_fused_loop_kernel<NCH, FUSED_NBUF>",
                           ("em_loop_fused", 2),
                           lambda h: _linear(h) and ceil_div(ceil_div(h, 2), ft) <= fmax
                           and ceil_div(ceil_div(h, 2), min(CUS, const("MXM_MAX_WG"))) <= 16 * const("FUSED_MAX_M"),
                           lambda h: ceil_div(ceil_div(h, 2), ft), fmax, "FUSED_MAX_NCH",
                           "P 16-byte aligned, ldp even, one restart; mode 2 keeps the columns-split form out")
    fct = const("FCODED_THREADS")
    s["fused_coded"] = Site("mxm_em_loop_coded under mxm_set_loop_fused(1)", "em_fused_coded_kernel<CNCH, 4, resident>",
                            ("em_loop_fused", 0),
                            lambda h: _linear_even(h) and _nch_coded(fct)(h) <= 8
                            and ceil_div(h // 2, fused_coded_grid(64)) <= 16 * const("FCODED_MAX_M"),
                            _nch_coded(fct), 6, "MAX = 8 and 2048 / FCODED_THREADS; at 64 rows the grid of 48 workgroups holds H <= 6144",
                            "records without a dense rest, H even; the widest width depends on the row count (module docstring)")
    cp_max = const("FCOLS_MAX_CP")
    s["fused_cols"] = Site("mxm_em_loop under mxm_set_loop_fused(1): columns split", "em_fused_cols_kernel<12 / 22 / 24, RPT>",
                           ("em_loop_fused", 1), lambda h: _linear(h) and ceil_div(h, CUS) <= cp_max,
                           lambda h: 1 if ceil_div(h, CUS) <= 12 else (2 if ceil_div(h, CUS) <= 22 else 3), 3,
                           "the three column counts 12, 22, 24 of the launcher (instances 1, 2, 3 here); RPT by the row count",
                           "a grid of exactly 256 workgroups (256 CUs), R <= FCOLS_MAX_RPT * FCOLS_THREADS", by_width=True)
    s["fused_narrow"] = Site("mxm_em_loop, narrow one-launch loop", "em_fused_narrow_kernel<4 / 8 / 16, RPT>",
                             ("launch_fused_narrow", 0), lambda h: 1 <= h <= 16, lambda h: 1 if h <= 4 else (2 if h <= 8 else 3), 3,
                             "the three column counts 4, 8, 16 of the launcher (instances 1, 2, 3 here); the dispatch itself is on RPT",
                             "no P (H <= 64): the log matrix in registers; RPT = 1 up to 512 rows per CU", lo=1, hi=16)
    for k, (func, nth) in enumerate([("mxm_em_loop_samples_narrow", 0), ("mxm_em_loop_samples_narrow", 1), ("mxm_assign_reads_samples", 0),
                                     ("narrow_entries_loop", 0), ("narrow_entries_loop", 1), ("mxm_assign_reads_samples_runs", 0),
                                     ("mxm_loglik_samples_masks", 0)]):
        s["narrow_ld_%d" % k] = Site(func, "the cohort's narrow kernels <LD = 4 / 8 / 16>", (func, nth), lambda h: h in (4, 8, 16),
                                     lambda h: h, 3, "LD == 4 || LD == 8 || LD == 16 of SFIN_KMAX", "by ld, not by the width",
                                     by_width=False, lo=4, hi=16)
    return s


SITES = _sites()


def classes(site):
    """[Class] of a site in ascending width: maximal runs of supported widths with the same instance."""
    site = SITES[site] if isinstance(site, str) else site
    out = []
    for n_haps in range(site.lo, site.hi + 1):
        if not site.supported(n_haps):
            continue
        inst = site.instance(n_haps)
        if out and out[-1].instance == inst:
            out[-1] = out[-1]._replace(last=n_haps)
        else:
            out.append(Class(inst, n_haps, n_haps))
    return out


def edge_cases(name):
    """[(instance, width)]: first and last width of every class (once where they coincide)."""
    out = []
    for c in classes(name):
        out.append((c.instance, c.first))
        if c.last != c.first:
            out.append((c.instance, c.last))
    return out


def edge_widths(names=None):
    """Every edge width of the width-dispatched sites, ascending."""
    widths = set()
    for name, site in SITES.items():
        if site.by_width and (names is None or name in names):
            widths.update(w for _, w in edge_cases(name))
    return sorted(widths)


COLSUM_SITES = ("em_iter_b1", "em_iter_b2", "em_iter_b3", "em_iter_b4", "em_iter_rest", "em_iter_f32", "em_iter_coded", "quad",
                "quad_coded", "quad_batched", "samples")


def colsum_shapes():
    """Every (width, rows) at which the sweep checks a `colsum` under the T rule, ascending."""
    return sorted(set((w, rows_for(i)) for name in COLSUM_SITES for i, w in edge_cases(name)))


def dispatch_sites():
    """[(host function, n-th dispatch_width call in it, MAX as written)] of mixemt_hip.hip, comments left out."""
    out, func, nth = [], None, 0
    for line in source().split("\n"):
        code = line.split("//")[0]
        head = re.match(r"^(?:static|extern \"C\")\s[^;=]*?\b(\w+)\s*\(", code)
        if head and not code.startswith("static const"):
            func, nth = head.group(1), 0
        for hit in re.finditer(r"dispatch_width<(\w+)>\(", code):
            if func == "dispatch_width":              # (the dispatcher's own recursion)
                continue
            out.append((func, nth, hit.group(1)))
            nth += 1
    return out
