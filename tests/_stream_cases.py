"""
The cases of tests/test_gpu_stream_contract.py: one call of one C ABI entry through one host route each (tests/_busy_stream.py
runs them).  TABLE lists (entry, route, class, builder) without touching the device; a builder makes its Case on demand.

What matters here is the host route through an entry, not the kernel's arithmetic, so every case is the smallest shape
that takes its route: R in {257, 700}, H = 66 for the any-width kernels and 5408 where a wide or streaming instance is the
route, 1500 alignments over a reference of 3000, S = 3 samples of 33, 64 and 600 rows.  Inputs come from what the suite
already has (tests/_accuracy_inputs.py, the guarded modules' generators, test_gpu_assemble.random_columns).

Classes (tests/test_stream_contract_complete.py holds every stream-taking entry to exactly one):
  A  only enqueues, capturable: gate pending at return, host time under half the delay, and the graph run passes
  B  only enqueues, but uploads a host table on every call or takes stream-ordered memory of its own: the same without
     the capture
  C  waits, and its header says so

Comparison: bit for bit.  The three producers that place their records with a bump allocator (mxm_encode_rows,
mxm_build_em_records, mxm_build_quads) and the fallback list (appended "in any order") are compared bit for bit AFTER
decoding -- every row's values through its offset and its codes, the list sorted -- because the header leaves the placement
in the buffer and the order of a record's table entries free; the snapshots
are compared with the final buffers as they are.  No case needs a tolerance: the design has no float atomics.
"""
import ctypes
import functools

import numpy

from _busy_stream import Case, nan_like, sentinel

TABLE = []
F8, I4, I8, U1 = numpy.float64, numpy.int32, numpy.int64, numpy.uint8
# the entries that read HOST input arrays: their busy run is made twice, with the arrays in pageable and in pinned memory
HOST_ARRAY_ENTRIES = ("mxm_fold_logaddexp", "mxm_new_variants", "mxm_extend_assign", "mxm_em_iter_samples", "mxm_em_loop_samples",
                      "mxm_votes_samples", "mxm_gather_columns_samples", "mxm_em_loop_samples_narrow", "mxm_assign_reads_samples",
                      "mxm_check_variants_samples")


def case(entry, route, klass):
    def register(builder):
        def build(lib):
            made = builder(lib)
            made.entry, made.route, made.klass = entry, route, klass
            return made
        TABLE.append((entry, route, klass, build))
        return builder
    return register


def make(call, bufs, decoy, outs, **kw):
    return Case(None, None, "A", call, bufs, decoy, outs, **kw)


def ids():
    return ["%s[%s]" % (e, r) for e, r, _, _ in TABLE]


def entries_of(klass=None):
    return sorted({e for e, _, k, _ in TABLE if klass is None or k == klass})


# ---- shared inputs (host, made once, never written) ---------------------------------------------------------------------
def states(n, done=()):
    raw = numpy.zeros(n * 6, dtype=I4)
    for b in done:
        raw[6 * b] = 1
    return raw


def stopped(n):
    """The decoy of a state array: every restart done, so a kernel that reads it leaves its outputs alone."""
    return states(n, range(n))


@functools.lru_cache(maxsize=None)
def dense(n_rows, n_haps):
    """(M, P with an even stride and zero pads, rowmax, w) of tests/_accuracy_inputs.few_values."""
    import _accuracy_inputs
    mat = numpy.array(_accuracy_inputs.few_values(n_rows, n_haps))
    wts = _accuracy_inputs.weights(n_rows)
    wts[wts == 0] = 1.0
    rowmax = mat.max(axis=1)
    ldp = n_haps + 2 + (n_haps & 1)
    lin = numpy.zeros((n_rows, ldp))
    lin[:, :n_haps] = numpy.exp(mat - rowmax[:, None])
    return mat, lin, rowmax, wts


def props_of(n_haps, n_runs, seed=0):
    return numpy.random.default_rng(900 + seed + n_haps).dirichlet([1.0] * n_haps, size=n_runs)


def padded(mat, ld, fill=numpy.nan):
    out = numpy.full((mat.shape[0], ld), fill, dtype=mat.dtype)
    out[:, :mat.shape[1]] = mat
    return out


def ws_bytes(lib, n_rows, n_haps, n_runs):
    return int(lib.mxm_workspace_bytes(n_rows, n_haps, n_runs))


# ---- dense EM entries -------------------------------------------------------------------------------------------------
def _linearize(lib, f32):
    n_rows, n_haps = 257, 66
    mat, lin, _, _ = dense(n_rows, n_haps)
    ldm, ldp = n_haps + 3, (n_haps + 3) // 4 * 4 + 4 if f32 else lin.shape[1]
    src = padded(mat, ldm)
    entry = lib.mxm_linearize_f32 if f32 else lib.mxm_linearize

    def call(p, h, stream):
        return entry(p["M"], ldm, n_rows, n_haps, p["P"], ldp, p["rowmax"], stream)
    return make(call, {"M": src, "P": sentinel((n_rows, ldp), numpy.float32 if f32 else F8), "rowmax": sentinel(n_rows, F8)},
                {"M": nan_like(src)}, ["P", "rowmax"])


@case("mxm_linearize", "R=257 H=66", "A")
def _(lib):
    return _linearize(lib, False)


@case("mxm_linearize_f32", "R=257 H=66", "A")
def _(lib):
    return _linearize(lib, True)


def _em_iter(lib, n_rows, n_haps, n_runs, tile=None, linear=True, f32=False):
    mat, lin, _, wts = dense(n_rows, n_haps)
    props = props_of(n_haps, n_runs)
    ldm = n_haps + 3
    nbytes = ws_bytes(lib, n_rows, n_haps, n_runs)
    if f32:
        ldp = (n_haps + 3) // 4 * 4 + 4
        store = numpy.zeros((n_rows, ldp), dtype=numpy.float32)
        store[:, :n_haps] = lin[:, :n_haps]
    else:
        ldp, store = lin.shape[1], lin
    bufs = {"w": wts, "props": props, "state": states(n_runs), "colsum": sentinel((n_runs, n_haps), F8)}
    decoy = {"w": nan_like(wts), "props": nan_like(props), "state": stopped(n_runs)}
    if linear:
        bufs["P"], decoy["P"] = store, nan_like(store)
    else:
        bufs["M"], decoy["M"] = padded(mat, ldm), nan_like(padded(mat, ldm))
        bufs["ln_props"], decoy["ln_props"] = numpy.log(props), nan_like(props)

    def call(p, h, stream):
        if f32:
            return lib.mxm_em_iter_f32(p["P"], ldp, p["w"], p["props"], n_rows, n_haps, n_runs, p["state"], p["colsum"], p["ws"],
                                       nbytes, stream)
        return lib.mxm_em_iter(p.get("M"), ldm if not linear else 0, p.get("P"), ldp if linear else 0, p["w"], p["props"],
                               p.get("ln_props"), n_rows, n_haps, n_runs, p["state"], p["colsum"], p["ws"], nbytes, stream)
    setup = None if tile is None else (lambda handle: handle.mxm_set_batch_tile(tile))
    return make(call, bufs, decoy, ["colsum"], scratch={"ws": nbytes}, setup=setup)


@case("mxm_em_iter", "B=1 H=66", "A")
def _(lib):
    return _em_iter(lib, 700, 66, 1)


@case("mxm_em_iter", "B=5 H=66: two passes", "A")
def _(lib):
    return _em_iter(lib, 700, 66, 5)


@case("mxm_em_iter", "B=5 mxm_set_batch_tile(1)", "A")
def _(lib):
    return _em_iter(lib, 257, 66, 5, tile=1)


@case("mxm_em_iter", "B=4 H=5408: the streaming instance", "A")
def _(lib):
    return _em_iter(lib, 257, 5408, 4)


@case("mxm_em_iter", "log space H=17 B=2", "A")
def _(lib):
    return _em_iter(lib, 257, 17, 2, linear=False)


@case("mxm_em_iter_f32", "B=1", "A")
def _(lib):
    return _em_iter(lib, 257, 66, 1, f32=True)


@case("mxm_em_iter_f32", "B=5", "A")
def _(lib):
    return _em_iter(lib, 700, 66, 5, f32=True)


def _m_finalize(lib, n_haps, n_runs):
    rng = numpy.random.default_rng(n_haps + n_runs)
    props = props_of(n_haps, n_runs, 1)
    sums = rng.random((n_runs, n_haps)) * 40.0 + 1e-3
    bufs = {"colsum": sums, "ln_cur": numpy.log(props), "ln_new": sentinel(props.shape, F8), "props_cur": props,
            "state": states(n_runs, (1,) if n_runs > 1 else ())}
    decoy = {"colsum": nan_like(sums), "ln_cur": nan_like(props), "props_cur": nan_like(props), "state": stopped(n_runs)}

    def call(p, h, stream):
        return lib.mxm_m_finalize(p["colsum"], p["ln_cur"], p["ln_new"], p["props_cur"], n_haps, n_runs, 1e-9, 5, p["state"], stream)
    return make(call, bufs, decoy, ["ln_cur", "ln_new", "props_cur", "state"])


@case("mxm_m_finalize", "H=66 B=1: one workgroup", "A")
def _(lib):
    return _m_finalize(lib, 66, 1)


@case("mxm_m_finalize", "H=5408 B=5: several workgroups", "A")
def _(lib):
    return _m_finalize(lib, 5408, 5)


def _em_step(lib, n_rows, n_haps, even):
    mat = dense(n_rows, n_haps)[0]
    wts = dense(n_rows, n_haps)[3]
    ld = n_haps + 2 + (n_haps & 1) if even else n_haps + 3
    lnp = numpy.log(props_of(n_haps, 1, 2)[0])
    src = padded(mat, ld)
    nbytes = ws_bytes(lib, n_rows, n_haps, 1)

    def call(p, h, stream):
        return lib.mxm_em_step(p["M"], ld, p["w"], p["ln_props"], n_rows, n_haps, p["out"], ld, 0, p["colsum"], p["ws"], nbytes, stream)
    return make(call, {"M": src, "w": wts, "ln_props": lnp, "out": sentinel((n_rows, ld), F8), "colsum": sentinel(n_haps, F8)},
                {"M": nan_like(src), "w": nan_like(wts), "ln_props": nan_like(lnp)}, ["out", "colsum"], scratch={"ws": nbytes})


@case("mxm_em_step", "wide H=66", "A")
def _(lib):
    return _em_step(lib, 257, 66, True)


@case("mxm_em_step", "narrow H=17", "A")
def _(lib):
    return _em_step(lib, 257, 17, False)


@case("mxm_em_step", "log space H=66, odd stride", "A")
def _(lib):
    return _em_step(lib, 257, 66, False)


@case("mxm_em_step", "global H=9700", "A")
def _(lib):
    return _em_step(lib, 33, 9700, False)


@case("mxm_log_normalize", "H=66", "A")
def _(lib):
    sums = numpy.random.default_rng(1).random(66) * 50.0 + 1e-6
    return make(lambda p, h, stream: lib.mxm_log_normalize(p["colsum"], 66, p["ln_new"], stream),
                {"colsum": sums, "ln_new": sentinel(66, F8)}, {"colsum": nan_like(sums)}, ["ln_new"])


@case("mxm_l1_exp_diff", "H=66", "A")
def _(lib):
    a, b = numpy.log(props_of(66, 2, 3))
    return make(lambda p, h, stream: lib.mxm_l1_exp_diff(p["a"], p["b"], 66, p["l1"], stream),
                {"a": a, "b": b, "l1": sentinel(1, F8)}, {"a": nan_like(a), "b": nan_like(b)}, ["l1"])


@case("mxm_add_scalar", "R=257 H=66", "A")
def _(lib):
    src = padded(dense(257, 66)[0], 69)
    return make(lambda p, h, stream: lib.mxm_add_scalar(p["x"], 69, 257, 66, -1.25, stream), {"x": src}, {"x": nan_like(src)}, ["x"])


def _argmax_votes(lib, even):
    n_rows, n_haps = 257, 66
    mat, _, _, wts = dense(n_rows, n_haps)
    ld = n_haps + 2 if even else n_haps + 3
    src = padded(mat, ld)
    nbytes = ws_bytes(lib, n_rows, n_haps, 1)

    def call(p, h, stream):
        return lib.mxm_row_argmax_votes(p["X"], ld, p["w"], n_rows, n_haps, p["best"], p["votes"], p["ws"], nbytes, stream)
    return make(call, {"X": src, "w": wts + 0.25, "best": sentinel(n_rows, I4), "votes": sentinel(n_haps, F8)},
                {"X": nan_like(src), "w": nan_like(wts)}, ["best", "votes"], scratch={"ws": nbytes})


@case("mxm_row_argmax_votes", "wide rows", "A")
def _(lib):
    return _argmax_votes(lib, True)


@case("mxm_row_argmax_votes", "generic, odd stride", "A")
def _(lib):
    return _argmax_votes(lib, False)


@case("mxm_first_seen", "R=700 H=66", "A")
def _(lib):
    rng = numpy.random.default_rng(4)
    best = rng.integers(0, 40, size=700).astype(I4)
    other = rng.integers(20, 66, size=700).astype(I4)                      # in-range labels of another problem
    return make(lambda p, h, stream: lib.mxm_first_seen(p["best"], 700, 66, p["first"], stream),
                {"best": best, "first": sentinel(66, I8)}, {"best": other}, ["first"])


@case("mxm_assign_reads", "R=257 H=66 nC=3", "A")
def _(lib):
    n_rows, n_haps = 257, 66
    src = padded(numpy.round(dense(n_rows, n_haps)[0], 1), n_haps + 3)
    cols = numpy.array([3, 40, 65], dtype=I4)
    log_props = numpy.full(n_haps, numpy.nan)
    log_props[cols] = numpy.log([0.5, 0.3, 0.2])

    def call(p, h, stream):
        return lib.mxm_assign_reads(p["X"], n_haps + 3, p["log_props"], p["cols"], 3, n_rows, n_haps, numpy.log(2.0), p["assigned"], stream)
    return make(call, {"X": src, "log_props": log_props, "cols": cols, "assigned": sentinel(n_rows, I4)},
                {"X": nan_like(src), "log_props": nan_like(log_props)}, ["assigned"])


@case("mxm_gather_columns", "R=257 H=66 nC=5", "A")
def _(lib):
    n_rows, n_haps = 257, 66
    src = padded(dense(n_rows, n_haps)[0], n_haps + 3)
    cols = numpy.array([65, 0, 7, 7, 31], dtype=I4)

    def call(p, h, stream):
        return lib.mxm_gather_columns(p["M"], n_haps + 3, n_rows, n_haps, p["cols"], 5, p["out"], 8, stream)
    return make(call, {"M": src, "cols": cols, "out": sentinel((n_rows, 8), F8)}, {"M": nan_like(src)}, ["out"])


def _fold(lib, even):
    n_rows, n_haps = 257, 66
    ld = n_haps + 2 if even else n_haps + 3
    rng = numpy.random.default_rng(5 + even)
    acc, in0, in1 = (padded(rng.normal(-30.0, 10.0, size=(n_rows, n_haps)), ld) for _ in range(3))
    lds = numpy.array([ld, ld], dtype=I8)

    def pointers(p):
        # the decoy names the same two blocks the other way round: valid pointers of another problem
        return numpy.array([p["in0"], p["in1"]], dtype=numpy.uint64), numpy.array([p["in1"], p["in0"]], dtype=numpy.uint64)

    def call(p, h, stream):
        return lib.mxm_fold_logaddexp(p["acc"], ld, h["in_host"].ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)),
                                      h["ld_in_host"].ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2, n_rows, n_haps, -0.5, stream)
    return make(call, {"acc": acc, "in0": in0, "in1": in1}, {"acc": nan_like(acc), "in0": nan_like(in0), "in1": nan_like(in1)}, ["acc"],
                host={"in_host": pointers, "ld_in_host": (lds, lds)})


@case("mxm_fold_logaddexp", "vector form", "A")
def _(lib):
    return _fold(lib, True)


@case("mxm_fold_logaddexp", "scalar form, odd stride", "A")
def _(lib):
    return _fold(lib, False)


# ---- the builds ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def build_inputs(n_haps, n_rows):
    """The guarded build module's synthetic tables and reads: rows of 1 .. 20 observations, one of 70 (the long rows' launch)
    and one of 130 (the fallback list)."""
    import test_gpu_guarded_build as gb
    tab = gb._tables(n_haps, 10 + n_haps)
    return tab, gb._reads(tab, n_rows, 100 * n_haps + n_rows), gb.N_SITES


def _other_bases(obs, seed):
    letters = numpy.frombuffer(b"ACGT", dtype=U1)
    return letters[numpy.random.default_rng(seed).integers(0, 4, size=len(obs))]


def _table_bufs(tab, names):
    src = {"exp": tab["exp"], "ecode": tab["ecode"], "maj": tab["maj"], "mk_ptr": tab["mk_ptr"], "mk_hap": tab["mk_hap"],
           "mk_base": tab["mk_base"], "lhit": tab["lhit"], "lmiss": tab["lmiss"], "obsmap": tab["obsmap"]}
    return {k: src[k] for k in names}


def _cell_build(lib, which):
    n_haps, n_rows = 66, 257
    tab, (row_ptr, site, obs), n_sites = build_inputs(n_haps, n_rows)
    lde, ldm = tab["lde"], n_haps + 3
    rows = numpy.arange(n_rows - 1, -1, -3, dtype=I8)
    n_out = len(rows) if which == "lut_rows" else n_rows
    bufs = _table_bufs(tab, ["exp", "lhit", "lmiss"] if which == "plain" else ["ecode", "lhit", "lmiss", "obsmap"])
    bufs.update({"row_ptr": row_ptr, "site": site, "obs": obs, "M": sentinel((n_out, ldm), F8)})
    if which == "lut_rows":
        bufs["rows"] = rows
    if which == "lut":
        bufs["order"] = numpy.random.default_rng(1).permutation(n_rows).astype(I8)
    decoy = {"lhit": nan_like(tab["lhit"]), "lmiss": nan_like(tab["lmiss"]), "obs": _other_bases(obs, 3)}

    def call(p, h, stream):
        if which == "plain":
            return lib.mxm_build_em_matrix(p["exp"], lde, p["lhit"], p["lmiss"], p["row_ptr"], p["site"], p["obs"], n_rows, n_haps,
                                           n_sites, p["M"], ldm, stream)
        if which == "lut":
            return lib.mxm_build_em_matrix_lut(p["ecode"], lde, p["lhit"], p["lmiss"], p["obsmap"], p["row_ptr"], p["site"], p["obs"],
                                               p["order"], n_rows, n_haps, n_sites, p["M"], ldm, stream)
        return lib.mxm_build_em_matrix_lut_rows(p["ecode"], lde, p["lhit"], p["lmiss"], p["obsmap"], p["row_ptr"], p["site"], p["obs"],
                                                p["rows"], len(rows), n_haps, n_sites, p["M"], ldm, stream)
    return make(call, bufs, decoy, ["M"])


@case("mxm_build_em_matrix", "R=257 H=66", "A")
def _(lib):
    return _cell_build(lib, "plain")


@case("mxm_build_em_matrix_lut", "ordered rows", "A")
def _(lib):
    return _cell_build(lib, "lut")


@case("mxm_build_em_matrix_lut_rows", "every third row", "A")
def _(lib):
    return _cell_build(lib, "lut_rows")


@case("mxm_expand_tables", "the 4-bit code table", "A")
def _(lib):
    tab, _, n_sites = build_inputs(66, 257)
    lde = tab["lde"]
    bufs = _table_bufs(tab, ["maj", "mk_ptr", "mk_hap", "mk_base"])
    bufs.update({"map256": tab["code_of"], "out": sentinel((n_sites, lde), U1)})
    decoy = {"maj": _other_bases(tab["maj"], 5), "mk_base": _other_bases(tab["mk_base"], 6)}

    def call(p, h, stream):
        return lib.mxm_expand_tables(p["maj"], p["mk_ptr"], p["mk_hap"], p["mk_base"], p["map256"], n_sites, 66, lde, p["out"], stream)
    return make(call, bufs, decoy, ["out"])


def _sorted_list(entries, count):
    n = int(count.view(I8)[0])
    rows = numpy.sort(entries.view(I8)[:max(0, min(n, len(entries.view(I8))))])
    return numpy.concatenate([rows, entries.view(I8)[max(n, 0):]]).view(U1)


def _decoded_records(out, n_haps, limit):
    """rec / rec_off as the rows they decode to, in row order: P table[codes] ++ log table[codes] of every row with a record.
    Where a record lies in `rec` is the bump allocator's choice, and the order of the entries in its tables (hence the
    codes) is the order in which the kernel's threads met the values: neither is the header's promise, the decoded row is."""
    rec, off, ndist = out["rec"], out["rec_off"].view(I8), out["ndist"].view(I4)
    ldc = (n_haps + 7) // 8 * 8
    parts = []
    for r in numpy.flatnonzero(ndist > 0):
        nd = int(ndist[r])
        code_bytes = ldc * (2 if nd > 256 else 1)
        size = code_bytes + 16 * nd
        assert 0 <= off[r] and off[r] + size <= limit and off[r] % 8 == 0, (r, off[r], size, limit)
        codes = rec[off[r]:off[r] + code_bytes].view(numpy.uint16 if nd > 256 else U1)[:n_haps].astype(I8)
        assert int(codes.max()) < nd, r
        tables = rec[off[r] + code_bytes:off[r] + size].view(numpy.int64)          # bit patterns: NaN payloads compare too
        parts += [tables[:nd][codes], tables[nd:][codes]]
    return numpy.concatenate(parts).view(U1) if parts else numpy.zeros(0, dtype=U1)


def _marker_build(lib, records, n_haps, n_rows):
    tab, (row_ptr, site, obs), n_sites = build_inputs(n_haps, n_rows)
    ldm = n_haps + 3
    bufs = _table_bufs(tab, ["maj", "lhit", "lmiss", "mk_ptr", "mk_hap", "mk_base"])
    bufs.update({"row_ptr": row_ptr, "site": site, "obs": obs, "M": sentinel((n_rows, ldm), F8), "fallback": sentinel(n_rows, I8),
                 "n_fallback": numpy.array([3], dtype=I8)})       # (an offset into fallback[]: in range before the call zeroes it)
    outs = ["M", "fallback", "n_fallback"]
    rec_bytes = int(lib.mxm_record_bytes(n_rows, n_haps))
    if records:
        bufs.update({"rec": sentinel(rec_bytes, U1), "rec_off": sentinel(n_rows, I8), "ndist": sentinel(n_rows, I4),
                     "rowmax": sentinel(n_rows, F8), "stats": numpy.array([4096, 1], dtype=I8)})     # ([0]: an offset into rec)
        outs += ["rec", "rec_off", "ndist", "rowmax", "stats"]
    decoy = {"lhit": nan_like(tab["lhit"]), "lmiss": nan_like(tab["lmiss"])}

    def call(p, h, stream):
        if records:
            return lib.mxm_build_em_records(p["maj"], p["lhit"], p["lmiss"], p["mk_ptr"], p["mk_hap"], p["mk_base"], p["row_ptr"],
                                            p["site"], p["obs"], None, n_rows, n_haps, n_sites, p["M"], ldm, p["rec"], rec_bytes,
                                            p["rec_off"], p["ndist"], p["rowmax"], p["stats"], p["fallback"], p["n_fallback"], stream)
        return lib.mxm_build_em_matrix_sparse(p["maj"], p["lhit"], p["lmiss"], p["mk_ptr"], p["mk_hap"], p["mk_base"], p["row_ptr"],
                                              p["site"], p["obs"], None, n_rows, n_haps, n_sites, p["M"], ldm, p["fallback"],
                                              p["n_fallback"], stream)

    def canon(out):
        out = dict(out)
        out["fallback"] = _sorted_list(out["fallback"], out["n_fallback"])
        if records:
            out["rec"] = _decoded_records(out, n_haps, rec_bytes)
            del out["rec_off"]
        return out
    made = make(call, bufs, decoy, outs)
    made.canon = canon
    return made


@case("mxm_build_em_matrix_sparse", "fallback rows and 65-128-site rows", "A")
def _(lib):
    return _marker_build(lib, False, 66, 257)


@case("mxm_build_em_records", "fallback rows and 65-128-site rows", "A")
def _(lib):
    return _marker_build(lib, True, 66, 257)


@case("mxm_build_em_records", "H=5408: wide records", "A")
def _(lib):
    return _marker_build(lib, True, 5408, 257)


# ---- records ------------------------------------------------------------------------------------------------------------
class Records:
    """A matrix in row-dictionary storage, made once on the device by mxm_encode_rows (and mxm_build_quads) on an idle
    stream and kept on the host: the arrays of an mxm_coded, and the decoy of `rec` / `qrec` (the same codes, NaN tables)."""

    def __init__(self, lib, mat, wts, quads=False):
        import torch
        from mixemt_amd import _lib
        self.mat, self.wts = mat, wts
        n_rows, n_haps = mat.shape
        self.R, self.H = n_rows, n_haps
        stream = torch.cuda.current_stream().cuda_stream
        rec_bytes = int(lib.mxm_coded_bytes(n_rows, n_haps))
        dev = {"M": torch.from_numpy(mat).cuda(), "rec": torch.zeros(rec_bytes, dtype=torch.uint8, device="cuda"),
               "rec_off": torch.zeros(n_rows, dtype=torch.int64, device="cuda"), "ndist": torch.zeros(n_rows, dtype=torch.int32, device="cuda"),
               "rowmax": torch.zeros(n_rows, dtype=torch.float64, device="cuda"), "stats": torch.zeros(2, dtype=torch.int64, device="cuda")}
        rc = lib.mxm_encode_rows(dev["M"].data_ptr(), n_haps, n_rows, n_haps, dev["rec"].data_ptr(), rec_bytes, dev["rec_off"].data_ptr(),
                                 dev["ndist"].data_ptr(), dev["rowmax"].data_ptr(), dev["stats"].data_ptr(), stream)
        assert rc == 0, lib.mxm_last_error()
        torch.cuda.synchronize()
        used = int(dev["stats"][0])
        self.rec = dev["rec"][:used + 64].cpu().numpy()
        self.rec_off, self.ndist, self.rowmax = (dev[k].cpu().numpy() for k in ("rec_off", "ndist", "rowmax"))
        self.rest = numpy.flatnonzero(self.ndist == 0).astype(I8)
        self.wide = numpy.flatnonzero(self.ndist > 256).astype(I8)
        ldc = (n_haps + 7) // 8 * 8
        self.rec_decoy = self.rec.copy()
        for r in numpy.flatnonzero(self.ndist > 0):
            nd, off = int(self.ndist[r]), int(self.rec_off[r])
            tables = off + ldc * (2 if nd > 256 else 1)
            self.rec_decoy[tables:tables + 16 * nd].view(F8)[:] = numpy.nan
        self.ldp = n_haps + 2
        top = mat[self.rest].max(axis=1) if len(self.rest) else numpy.zeros(0)
        self.p_rest = numpy.zeros((len(self.rest), self.ldp))
        self.p_rest[:, :n_haps] = numpy.exp(mat[self.rest] - top[:, None])
        self.qrec = None
        if quads:
            assert len(self.rest) == 0
            q_bytes = int(lib.mxm_quad_bytes(n_rows, n_haps))
            st = _lib.Coded(dev["rec"].data_ptr(), dev["rec_off"].data_ptr(), dev["ndist"].data_ptr(), n_rows, None, 0, None, 0, None, 0)
            qd = {"qrec": torch.zeros(q_bytes, dtype=torch.uint8, device="cuda"), "qoff": torch.zeros(n_rows, dtype=torch.int64, device="cuda"),
                  "nquad": torch.zeros(n_rows, dtype=torch.int32, device="cuda"), "stats": torch.zeros(2, dtype=torch.int64, device="cuda")}
            rc = lib.mxm_build_quads(ctypes.byref(st), n_haps, qd["qrec"].data_ptr(), q_bytes, qd["qoff"].data_ptr(), qd["nquad"].data_ptr(),
                                     qd["stats"].data_ptr(), stream)
            assert rc == 0, lib.mxm_last_error()
            torch.cuda.synchronize()
            self.qoff, self.nquad = qd["qoff"].cpu().numpy(), qd["nquad"].cpu().numpy()
            has = numpy.flatnonzero(self.nquad > 0)
            assert len(has) > 0
            end = int((self.qoff[has] + 2048 + 32 * self.nquad[has]).max())
            self.qrec = qd["qrec"][:end + 64].cpu().numpy()
            self.qrec_decoy = self.qrec.copy()
            for r in has:
                at = int(self.qoff[r]) + 2048
                self.qrec_decoy[at:at + 32 * int(self.nquad[r])].view(F8)[:] = numpy.nan
            self.quad_rows = has.astype(I8)
            self.byte_rows = numpy.flatnonzero((self.ndist > 0) & (self.ndist <= 256) & (self.nquad == 0)).astype(I8)

    def bufs(self):
        out = {"rec": self.rec, "rec_off": self.rec_off, "ndist": self.ndist}
        decoy = {"rec": self.rec_decoy}
        if len(self.rest):
            out["P_rest"], decoy["P_rest"] = self.p_rest, nan_like(self.p_rest)
            out["w_rest"], decoy["w_rest"] = self.wts[self.rest], nan_like(self.wts[self.rest])
        if len(self.wide):
            out["wide_rows"] = self.wide
        if self.qrec is not None:
            out.update({"qrec": self.qrec, "qoff": self.qoff, "nquad": self.nquad})
            decoy["qrec"] = self.qrec_decoy
            if len(self.quad_rows):
                out["quad_rows"] = self.quad_rows
            if len(self.byte_rows):
                out["byte_rows"] = self.byte_rows
        return out, decoy

    def struct(self, p):
        from mixemt_amd import _lib
        st = _lib.Coded(p["rec"], p["rec_off"], p["ndist"], self.R, p.get("P_rest"), self.ldp if len(self.rest) else 0, p.get("w_rest"),
                        len(self.rest), p.get("wide_rows"), len(self.wide))
        if self.qrec is not None:
            st.qrec, st.qoff, st.nquad = p["qrec"], p["qoff"], p["nquad"]
            st.quad_rows, st.n_quad_rows = p.get("quad_rows"), len(self.quad_rows)
            st.byte_rows, st.n_byte_rows = p.get("byte_rows"), len(self.byte_rows)
        return st


_records = {}


def records(lib, kind):
    """"mixed 5408": byte, wide and dense-rest rows (the guarded records module's matrix); "quads 5408": rows of few quads
    with byte-coded leftovers and a wide row, beside a quad dictionary; "plain 66": byte-coded rows alone; "samples 66": the
    cohort module's rows for S = 3 samples of 33, 64 and 600 rows."""
    if kind not in _records:
        import test_gpu_guarded_records as gr
        import _accuracy_inputs
        if kind == "mixed 5408":
            mat = gr._matrix(numpy.random.default_rng(5408), 257, 5408)
        elif kind == "quads 5408":
            mat = gr._run_matrix(numpy.random.default_rng(9000 + 5408), 257, 5408)
        elif kind == "plain 66":
            mat = numpy.array(_accuracy_inputs.few_values(257, 66))
        else:
            assert kind == "samples 66", kind
            import test_gpu_guarded_cohort as gc
            mat = gc._matrix(numpy.random.default_rng(366), 697, 66)
        wts = _accuracy_inputs.weights(len(mat))
        wts[wts == 0] = 1.0
        _records[kind] = Records(lib, mat, wts, quads=kind.startswith("quads"))
    return _records[kind]


def _encode_rows(lib, n_haps, wide):
    import test_gpu_guarded_records as gr
    mat = gr._matrix(numpy.random.default_rng(n_haps), 257, n_haps) if wide else numpy.array(dense(257, n_haps)[0])
    n_rows = len(mat)
    rec_bytes = int(lib.mxm_coded_bytes(n_rows, n_haps))

    def call(p, h, stream):
        return lib.mxm_encode_rows(p["M"], n_haps, n_rows, n_haps, p["rec"], rec_bytes, p["rec_off"], p["ndist"], p["rowmax"], p["stats"], stream)

    def canon(out):
        out = dict(out)
        out["rec"] = _decoded_records(out, n_haps, rec_bytes)
        del out["rec_off"]
        return out
    made = make(call, {"M": mat, "rec": sentinel(rec_bytes, U1), "rec_off": sentinel(n_rows, I8), "ndist": sentinel(n_rows, I4),
                       "rowmax": sentinel(n_rows, F8), "stats": numpy.array([4096, 1], dtype=I8)}, {"M": nan_like(mat)},
                ["rec", "rec_off", "ndist", "rowmax", "stats"])
    made.canon = canon
    return made


@case("mxm_encode_rows", "byte rows H=66", "A")
def _(lib):
    return _encode_rows(lib, 66, False)


@case("mxm_encode_rows", "16-bit rows H=5408", "A")
def _(lib):
    return _encode_rows(lib, 5408, True)


def _build_quads(lib, encoder):
    rec = records(lib, "quads 5408")
    n_rows, n_haps = rec.R, rec.H
    # 512 pieces of 64 KB: each of at most 257 waves or workgroups has one open, and 257 records fill a few dozen; canon()
    # asserts that the call asked for no more (a short buffer would make nquad depend on the waves' timing)
    q_bytes = 512 * 65536
    bufs, decoy = rec.bufs()
    for name in ("qrec", "qoff", "nquad", "quad_rows", "byte_rows"):
        bufs.pop(name, None)
        decoy.pop(name, None)
    bufs.update({"qrec_out": sentinel(q_bytes, U1), "qoff": sentinel(n_rows, I8), "nquad": sentinel(n_rows, I4),
                 "stats": numpy.array([65536, 1], dtype=numpy.uint64)})
    plain = Records.__new__(Records)
    plain.__dict__.update(rec.__dict__)
    plain.qrec = None

    def call(p, h, stream):
        st = plain.struct(p)
        return lib.mxm_build_quads(ctypes.byref(st), n_haps, p["qrec_out"], q_bytes, p["qoff"], p["nquad"], p["stats"], stream)

    def canon(out):
        out = dict(out)
        qoff, nquad = out.pop("qoff").view(I8), out["nquad"].view(I4)
        out["qrec_out"] = numpy.concatenate([out["qrec_out"][qoff[r]:qoff[r] + 2048 + 32 * int(nquad[r])] for r in numpy.flatnonzero(nquad > 0)]
                                            or [numpy.zeros(0, dtype=U1)])
        assert int(out["stats"].view(numpy.uint64)[0]) <= q_bytes, "the quad records need a larger buffer than the case gives"
        out["stats"] = out["stats"].view(numpy.uint64)[1:].view(U1)      # [0], bytes RESERVED, depends on the waves' timing
        return out
    made = make(call, bufs, decoy, ["qrec_out", "qoff", "nquad", "stats"], setup=lambda handle: handle.mxm_set_quad_encoder(encoder))
    made.canon = canon
    return made


@case("mxm_build_quads", "a wave per row", "A")
def _(lib):
    return _build_quads(lib, 1)


@case("mxm_build_quads", "a workgroup per row", "A")
def _(lib):
    return _build_quads(lib, 0)


@case("mxm_quad_lists", "R=257", "A")
def _(lib):
    rec = records(lib, "quads 5408")
    n_rows = rec.R
    nbytes = int(lib.mxm_quad_lists_scratch_bytes(n_rows))
    other = numpy.where(rec.nquad > 0, 0, 7).astype(I4)       # valid counts of another dictionary

    def call(p, h, stream):
        return lib.mxm_quad_lists(p["ndist"], p["nquad"], n_rows, p["quad_rows"], p["byte_rows"], p["counts"], p["scratch"], nbytes, stream)
    return make(call, {"ndist": rec.ndist, "nquad": rec.nquad, "quad_rows": sentinel(n_rows, I8), "byte_rows": sentinel(n_rows, I8),
                       "counts": sentinel(2, I8)}, {"nquad": other}, ["quad_rows", "byte_rows", "counts"], scratch={"scratch": nbytes})


@case("mxm_decode_rows", "byte and wide records", "A")
def _(lib):
    rec = records(lib, "mixed 5408")
    bufs, decoy = rec.bufs()
    ldp = rec.H + 3
    bufs["P"] = sentinel((rec.R, ldp), F8)

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_decode_rows(ctypes.byref(st), rec.H, p["P"], ldp, stream)
    return make(call, bufs, decoy, ["P"])


@case("mxm_scatter_records", "n=129", "A")
def _(lib):
    n_rows = 257
    rng = numpy.random.default_rng(257)
    rows = numpy.arange(0, n_rows, 2, dtype=I8)[::-1].copy()
    ins = {"rows": rows, "sub_off": rng.integers(0, 1 << 40, size=len(rows)).astype(I8),
           "sub_nd": (rng.integers(0, 3, size=len(rows)) * 7).astype(I4), "sub_rm": rng.normal(size=len(rows))}
    decoy = {"sub_off": ins["sub_off"] + 8, "sub_nd": numpy.full(len(rows), 3, dtype=I4), "sub_rm": nan_like(ins["sub_rm"])}
    bufs = dict(ins)
    bufs.update({"rec_off": sentinel(n_rows, I8), "ndist": sentinel(n_rows, I4), "rowmax": sentinel(n_rows, F8)})

    def call(p, h, stream):
        return lib.mxm_scatter_records(p["rows"], len(rows), p["sub_off"], p["sub_nd"], p["sub_rm"], 4096, p["rec_off"], p["ndist"],
                                       p["rowmax"], stream)
    return make(call, bufs, decoy, ["rec_off", "ndist", "rowmax"])


def _em_iter_coded(lib, kind, n_runs):
    rec = records(lib, kind)
    bufs, decoy = rec.bufs()
    props = props_of(rec.H, n_runs, 4)
    nbytes = ws_bytes(lib, rec.R, rec.H, n_runs)
    bufs.update({"w": rec.wts, "props": props, "state": states(n_runs), "colsum": sentinel((n_runs, rec.H), F8)})
    decoy.update({"w": nan_like(rec.wts), "props": nan_like(props)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_em_iter_coded(ctypes.byref(st), p["w"], p["props"], rec.H, n_runs, p["state"], p["colsum"], p["ws"], nbytes, stream)
    return make(call, bufs, decoy, ["colsum", "state"], scratch={"ws": nbytes})


@case("mxm_em_iter_coded", "records, wide rows and a dense rest", "A")
def _(lib):
    return _em_iter_coded(lib, "mixed 5408", 2)


@case("mxm_em_iter_coded", "beside a quad dictionary, B=1", "A")
def _(lib):
    return _em_iter_coded(lib, "quads 5408", 1)


@case("mxm_em_iter_coded", "beside a quad dictionary, B=4: a full tile of three", "A")
def _(lib):
    return _em_iter_coded(lib, "quads 5408", 4)


def _rest_bufs(rec, bufs, decoy):
    ld = rec.H + 3
    if len(rec.rest):
        bufs["M_rest"] = padded(rec.mat[rec.rest], ld)
        decoy["M_rest"] = nan_like(bufs["M_rest"])
        bufs["rest_rows"] = rec.rest
    return ld if len(rec.rest) else 0


def _votes_coded(lib, n_runs):
    rec = records(lib, "mixed 5408")
    bufs, decoy = rec.bufs()
    ld_rest = _rest_bufs(rec, bufs, decoy)
    props = props_of(rec.H, n_runs, 5)
    nbytes = ws_bytes(lib, rec.R, rec.H, 1)
    bufs.update({"ln_props": numpy.log(props), "props": props, "rowmax": rec.rowmax, "w": rec.wts + 0.25,
                 "best": sentinel(rec.R, I4), "votes": sentinel(rec.H, F8)})
    decoy.update({"ln_props": nan_like(props), "props": nan_like(props), "rowmax": nan_like(rec.rowmax), "w": nan_like(rec.wts)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_row_argmax_votes_coded(ctypes.byref(st), rec.H, n_runs, p["ln_props"], p["props"], p["rowmax"], p.get("M_rest"),
                                              ld_rest, p.get("rest_rows"), len(rec.rest), p["w"], p["best"], p["votes"], p["ws"], nbytes, stream)
    return make(call, bufs, decoy, ["best", "votes"], scratch={"ws": nbytes})


@case("mxm_row_argmax_votes_coded", "one run: the narrow and the wide kernel, the dense rest", "A")
def _(lib):
    return _votes_coded(lib, 1)


@case("mxm_row_argmax_votes_coded", "two runs: the posterior route", "A")
def _(lib):
    return _votes_coded(lib, 2)


@case("mxm_em_step_coded", "records and a dense rest", "A")
def _(lib):
    rec = records(lib, "mixed 5408")
    bufs, decoy = rec.bufs()
    ld_rest = _rest_bufs(rec, bufs, decoy)
    props = props_of(rec.H, 1, 6)[0]
    ldo = rec.H + 3
    bufs.update({"ln_props": numpy.log(props), "props": props, "rowmax": rec.rowmax, "out": sentinel((rec.R, ldo), F8)})
    decoy.update({"ln_props": nan_like(props), "props": nan_like(props), "rowmax": nan_like(rec.rowmax)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_em_step_coded(ctypes.byref(st), rec.H, p["ln_props"], p["props"], p["rowmax"], p.get("M_rest"), ld_rest,
                                     p.get("rest_rows"), len(rec.rest), p["out"], ldo, 0, stream)
    return make(call, bufs, decoy, ["out"])


@case("mxm_gather_columns_coded", "records and a dense rest", "A")
def _(lib):
    rec = records(lib, "mixed 5408")
    bufs, decoy = rec.bufs()
    ld_rest = _rest_bufs(rec, bufs, decoy)
    cols = numpy.array([rec.H - 1, 0, 17, 17, 4000], dtype=I4)
    bufs.update({"cols": cols, "out": sentinel((rec.R, 8), F8)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_gather_columns_coded(ctypes.byref(st), rec.H, p["cols"], 5, p.get("M_rest"), ld_rest, p.get("rest_rows"),
                                            len(rec.rest), p["out"], 8, stream)
    return make(call, bufs, decoy, ["out"])


# ---- the loops (class C: "Blocks the calling thread") --------------------------------------------------------------------
def _loop_vectors(n_haps, n_runs, seed):
    props = props_of(n_haps, n_runs, seed)
    ln0 = numpy.log(props)
    bufs = {"props_cur": props, "ln_cur": ln0, "ln_new": ln0.copy(), "colsum": sentinel((n_runs, n_haps), F8), "state": states(n_runs)}
    decoy = {"props_cur": nan_like(props), "ln_cur": nan_like(props), "ln_new": nan_like(props), "state": stopped(n_runs)}
    return bufs, decoy, ["props_cur", "ln_cur", "ln_new", "colsum", "state"]


def _state_host(n):
    from mixemt_amd import _lib
    return {"state_host": numpy.zeros(n * ctypes.sizeof(_lib.EmState), dtype=U1)}


def _state_ptr(h):
    from mixemt_amd import _lib
    return h["state_host"].ctypes.data_as(ctypes.POINTER(_lib.EmState))


def _em_loop(lib, n_rows, n_haps, n_runs, setup, f32=False, log_space=False):
    mat, lin, _, wts = dense(n_rows, n_haps)
    bufs, decoy, outs = _loop_vectors(n_haps, n_runs, 7)
    ldm = n_haps + 3
    nbytes = ws_bytes(lib, n_rows, n_haps, n_runs)
    if f32:
        ldp = (n_haps + 3) // 4 * 4 + 4
        store = numpy.zeros((n_rows, ldp), dtype=numpy.float32)
        store[:, :n_haps] = lin[:, :n_haps]
    else:
        ldp, store = lin.shape[1], lin
    bufs["w"], decoy["w"] = wts, nan_like(wts)
    if not log_space:
        bufs["P"], decoy["P"] = store, nan_like(store)
    if not f32:
        bufs["M"], decoy["M"] = padded(mat, ldm), nan_like(padded(mat, ldm))

    def call(p, h, stream):
        if f32:
            return lib.mxm_em_loop_f32(p["P"], ldp, p["w"], n_rows, n_haps, n_runs, p["props_cur"], p["ln_cur"], p["ln_new"], p["colsum"],
                                       p["state"], 0.0, 5, 2, p["ws"], nbytes, stream, _state_ptr(h))
        return lib.mxm_em_loop(p["M"], ldm, p.get("P"), 0 if log_space else ldp, p["w"], n_rows, n_haps, n_runs, p["props_cur"],
                               p["ln_cur"], p["ln_new"], p["colsum"], p["state"], 0.0, 5, 2, p["ws"], nbytes, stream, _state_ptr(h))
    return make(call, bufs, decoy, outs, scratch={"ws": nbytes}, host_outs=_state_host(n_runs), setup=setup)


def _fused(mode):
    return lambda handle: handle.mxm_set_loop_fused(mode, 0)


def _per_iteration(graph):
    def setup(handle):
        handle.mxm_set_loop_fused(0, 0)
        handle.mxm_set_loop_graph(graph)
    return setup


def _give_up(handle):
    handle.mxm_diag_fused_force_abort(1)


@case("mxm_em_loop", "one launch, columns split (R=700 H=66 B=1)", "C")
def _(lib):
    return _em_loop(lib, 700, 66, 1, None)


@case("mxm_em_loop", "one launch, rows split", "C")
def _(lib):
    return _em_loop(lib, 700, 66, 1, _fused(2))


@case("mxm_em_loop", "per iteration, mxm_set_loop_graph(0), B=5", "C")
def _(lib):
    return _em_loop(lib, 257, 66, 5, _per_iteration(0))


@case("mxm_em_loop", "per iteration, mxm_set_loop_graph(1), B=5", "C")
def _(lib):
    return _em_loop(lib, 257, 66, 5, _per_iteration(1))


@case("mxm_em_loop", "one launch gives up and is undone", "C")
def _(lib):
    return _em_loop(lib, 700, 66, 1, _give_up)


@case("mxm_em_loop", "narrow one launch (H=8, log space)", "C")
def _(lib):
    return _em_loop(lib, 700, 8, 1, None, log_space=True)


@case("mxm_em_loop_f32", "mxm_set_loop_graph(0)", "C")
def _(lib):
    return _em_loop(lib, 257, 66, 2, _per_iteration(0), f32=True)


@case("mxm_em_loop_f32", "mxm_set_loop_graph(1)", "C")
def _(lib):
    return _em_loop(lib, 257, 66, 2, _per_iteration(1), f32=True)


def _em_loop_coded(lib, kind, n_runs, setup):
    rec = records(lib, kind)
    bufs, decoy = rec.bufs()
    vec, vec_decoy, outs = _loop_vectors(rec.H, n_runs, 8)
    bufs.update(vec)
    decoy.update(vec_decoy)
    bufs["w"], decoy["w"] = rec.wts, nan_like(rec.wts)
    nbytes = ws_bytes(lib, rec.R, rec.H, n_runs)

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_em_loop_coded(ctypes.byref(st), p["w"], rec.H, n_runs, p["props_cur"], p["ln_cur"], p["ln_new"], p["colsum"],
                                     p["state"], 0.0, 5, 2, p["ws"], nbytes, stream, _state_ptr(h))
    return make(call, bufs, decoy, outs, scratch={"ws": nbytes}, host_outs=_state_host(n_runs), setup=setup)


@case("mxm_em_loop_coded", "one launch over records", "C")
def _(lib):
    return _em_loop_coded(lib, "plain 66", 1, None)


@case("mxm_em_loop_coded", "one launch gives up and is undone", "C")
def _(lib):
    return _em_loop_coded(lib, "plain 66", 1, _give_up)


@case("mxm_em_loop_coded", "per iteration with a dense rest, mxm_set_loop_graph(0)", "C")
def _(lib):
    return _em_loop_coded(lib, "mixed 5408", 2, _per_iteration(0))


@case("mxm_em_loop_coded", "per iteration beside quads, tiles of three, mxm_set_loop_graph(1)", "C")
def _(lib):
    return _em_loop_coded(lib, "quads 5408", 4, _per_iteration(1))


# ---- the cohort: samples, finish entries, variant check --------------------------------------------------------------------
ROW0 = numpy.array([0, 33, 97, 697], dtype=I8)                # S = 3 samples of 33, 64 and 600 rows
ROW0_OTHER = numpy.array([0, 600, 664, 697], dtype=I8)        # the same rows cut another way: the host decoy


def _n_tiles(lib):
    return int(lib.mxm_samples_plan(ROW0.ctypes.data, 3, None, 0, None))


def _samples(lib, loop):
    rec = records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    assert len(rec.rest) == 0
    nbytes = int(lib.mxm_samples_workspace_bytes(max(_n_tiles(lib), int(lib.mxm_samples_plan(ROW0_OTHER.ctypes.data, 3, None, 0, None))),
                                                 3, rec.H))
    bufs["w"], decoy["w"] = rec.wts, nan_like(rec.wts)
    if loop:
        vec, vec_decoy, outs = _loop_vectors(rec.H, 3, 9)
        bufs.update(vec)
        decoy.update(vec_decoy)
    else:
        props = props_of(rec.H, 3, 9)
        bufs.update({"props": props, "state": states(3), "colsum": sentinel((3, rec.H), F8)})
        decoy.update({"props": nan_like(props)})
        outs = ["colsum", "state"]

    def call(p, h, stream):
        st = rec.struct(p)
        if loop:
            return lib.mxm_em_loop_samples(ctypes.byref(st), h["row0_host"].ctypes.data, 3, p["w"], rec.H, p["props_cur"], p["ln_cur"],
                                           p["ln_new"], p["colsum"], p["state"], 0.0, 5, 2, p["ws"], nbytes, stream, _state_ptr(h))
        return lib.mxm_em_iter_samples(ctypes.byref(st), h["row0_host"].ctypes.data, 3, p["w"], p["props"], rec.H, p["state"], p["colsum"],
                                       p["ws"], nbytes, stream)
    return make(call, bufs, decoy, outs, scratch={"ws": nbytes}, host={"row0_host": (ROW0, ROW0_OTHER)},
                host_outs=_state_host(3) if loop else None)


@case("mxm_em_iter_samples", "S=3", "B")
def _(lib):
    return _samples(lib, False)


@case("mxm_em_loop_samples", "S=3", "C")
def _(lib):
    return _samples(lib, True)


def _finish_ws(lib, ld):
    n = max(_n_tiles(lib), int(lib.mxm_samples_plan(ROW0_OTHER.ctypes.data, 3, None, 0, None)))
    return int(lib.mxm_samples_finish_workspace_bytes(n, 3, ld))


@case("mxm_votes_samples", "S=3 with counts and lse", "B")
def _(lib):
    rec = records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    props = props_of(rec.H, 3, 10)
    nbytes = _finish_ws(lib, 0)
    bufs.update({"w": rec.wts + 0.25, "ln_props": numpy.log(props), "props": props, "rowmax": rec.rowmax, "best": sentinel(rec.R, I4),
                 "votes": sentinel((3, rec.H), F8), "counts": sentinel((3, rec.H), I8), "first": sentinel((3, rec.H), I8),
                 "lse": sentinel(rec.R, F8), "state": states(3)})
    decoy.update({"w": nan_like(rec.wts), "ln_props": nan_like(props), "props": nan_like(props), "rowmax": nan_like(rec.rowmax)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_votes_samples(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, p["w"], p["ln_props"], p["props"], p["rowmax"],
                                     p["best"], p["votes"], p["counts"], p["first"], p["lse"], p["state"], p["ws"], nbytes, stream)
    return make(call, bufs, decoy, ["best", "votes", "counts", "first", "lse", "state"], scratch={"ws": nbytes},
                host={"row0_host": (ROW0, ROW0_OTHER)})


@case("mxm_votes_samples", "two calls back to back under two plans", "B")
def _(lib):
    """The second call makes and uploads its tile table while the first one's is still waiting for the stream: a table the
    library kept in one place for both calls would reach the device as the second plan's."""
    rec = records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    props = props_of(rec.H, 3, 21)
    nbytes = _finish_ws(lib, 0)
    bufs.update({"w": rec.wts + 0.25, "ln_props": numpy.log(props)})
    decoy.update({"w": nan_like(rec.wts), "ln_props": nan_like(props)})
    outs = []
    for k in "ab":
        bufs.update({"best_" + k: sentinel(rec.R, I4), "votes_" + k: sentinel((3, rec.H), F8), "first_" + k: sentinel((3, rec.H), I8)})
        outs += ["best_" + k, "votes_" + k, "first_" + k]

    def call(p, h, stream):
        st = rec.struct(p)
        for k in "ab":
            rc = lib.mxm_votes_samples(ctypes.byref(st), h["row0_%s_host" % k].ctypes.data, 3, rec.H, p["w"], p["ln_props"], None, None,
                                       p["best_" + k], p["votes_" + k], None, p["first_" + k], None, None, p["ws_" + k], nbytes, stream)
            if rc != 0:
                return rc
        return 0
    return make(call, bufs, decoy, outs, scratch={"ws_a": nbytes, "ws_b": nbytes},
                host={"row0_a_host": (ROW0, ROW0_OTHER), "row0_b_host": (ROW0_OTHER, ROW0)})


LD = 8
NCOL = numpy.array([1, 3, 7], dtype=I4)
NCOL_OTHER = numpy.array([7, 1, 3], dtype=I4)


def _columns(n_haps):
    rng = numpy.random.default_rng(n_haps + LD)
    cols, other = numpy.zeros((3, LD), dtype=I4), numpy.zeros((3, LD), dtype=I4)
    for s in range(3):
        cols[s, :NCOL[s]] = numpy.sort(rng.choice(n_haps, size=NCOL[s], replace=False))
        other[s, :NCOL_OTHER[s]] = numpy.sort(rng.choice(n_haps, size=NCOL_OTHER[s], replace=False))
    return cols, other


def _reduced(rec):
    cols, _ = _columns(rec.H)
    sub = numpy.full((rec.R, LD), -numpy.inf)
    for s in range(3):
        lo, hi = int(ROW0[s]), int(ROW0[s + 1])
        sub[lo:hi, :NCOL[s]] = rec.mat[lo:hi][:, cols[s, :NCOL[s]]]
    return sub


@case("mxm_gather_columns_samples", "S=3 ld=8", "B")
def _(lib):
    rec = records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    cols, other = _columns(rec.H)
    nbytes = _finish_ws(lib, LD)
    bufs["out"] = sentinel((rec.R, LD), F8)

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_gather_columns_samples(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, h["cols_host"].ctypes.data,
                                              h["ncol_host"].ctypes.data, LD, p["out"], p["ws"], nbytes, stream)
    return make(call, bufs, decoy, ["out"], scratch={"ws": nbytes},
                host={"row0_host": (ROW0, ROW0_OTHER), "cols_host": (cols, other), "ncol_host": (NCOL, NCOL_OTHER)})


def _theta(rec, seed):
    rng = numpy.random.default_rng(seed)
    theta = numpy.zeros((3, LD))
    for s in range(3):
        theta[s, :NCOL[s]] = numpy.log(rng.dirichlet([1.0] * NCOL[s]))
    return theta


@case("mxm_em_loop_samples_narrow", "S=3 ld=8", "C")
def _(lib):
    rec = records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    sub, theta = _reduced(rec), _theta(rec, 11)
    nbytes = _finish_ws(lib, LD)
    bufs.update({"M": sub, "w": rec.wts, "props_cur": numpy.exp(theta), "ln_cur": theta, "ln_new": theta.copy(), "state": states(3),
                 "E": sentinel((rec.R, LD), F8)})
    decoy.update({"M": nan_like(sub), "w": nan_like(rec.wts), "props_cur": nan_like(theta), "ln_cur": nan_like(theta),
                  "ln_new": nan_like(theta), "state": stopped(3)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_em_loop_samples_narrow(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, p["M"], LD, h["ncol_host"].ctypes.data,
                                              p["w"], p["props_cur"], p["ln_cur"], p["ln_new"], p["state"], 0.0, 5, 2, p["E"], p["ws"],
                                              nbytes, stream, _state_ptr(h))
    return make(call, bufs, decoy, ["props_cur", "ln_cur", "ln_new", "state", "E"], scratch={"ws": nbytes},
                host={"row0_host": (ROW0, ROW0_OTHER), "ncol_host": (NCOL, numpy.array([1, 1, 1], dtype=I4))}, host_outs=_state_host(3))


@case("mxm_assign_reads_samples", "S=3 ld=8 with the posterior", "B")
def _(lib):
    rec = records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    sub, theta_k, theta_n = _reduced(rec), _theta(rec, 12), _theta(rec, 13)
    nbytes = _finish_ws(lib, LD)
    rng = numpy.random.default_rng(14)
    perm, other = numpy.zeros((3, LD), dtype=I4), numpy.zeros((3, LD), dtype=I4)
    for s in range(3):
        perm[s, :NCOL[s]] = rng.permutation(NCOL[s])
        other[s, :NCOL[s]] = perm[s, :NCOL[s]][::-1]
    bufs.update({"M": sub, "ln_theta": theta_k, "props": numpy.exp(theta_k), "log_props": theta_n, "assigned": sentinel(rec.R, I4),
                 "post": sentinel((rec.R, LD), F8)})
    decoy.update({"M": nan_like(sub), "ln_theta": nan_like(theta_k), "props": nan_like(theta_k), "log_props": nan_like(theta_n)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_assign_reads_samples(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, p["M"], LD, h["ncol_host"].ctypes.data,
                                            h["perm_host"].ctypes.data, p["ln_theta"], p["props"], p["log_props"], None, numpy.log(2.0),
                                            p["assigned"], p["post"], p["ws"], nbytes, stream)
    return make(call, bufs, decoy, ["assigned", "post"], scratch={"ws": nbytes},
                host={"row0_host": (ROW0, ROW0_OTHER), "ncol_host": (NCOL, NCOL), "perm_host": (perm, other)})


@case("mxm_check_variants_samples", "S=3 ld=8", "B")
def _(lib):
    rng = numpy.random.default_rng(48)
    n_samples, table_len, n_haps, n_sites, ld = 3, 333, 24, 60, 8
    site = numpy.append(numpy.sort(rng.choice(table_len - 1, size=n_sites - 1, replace=False)), table_len - 1).astype(I4)
    ref_code = rng.integers(-1, 4, size=n_sites)
    site_key = numpy.where(ref_code >= 0, site * 4 + ref_code, -1).astype(I4)
    key_ptr, key = [0], []
    for h in range(n_haps):
        at = numpy.sort(rng.choice(n_sites, size=int(rng.integers(0, 9)), replace=False))
        key.extend(int(site[i]) * 4 + int(rng.integers(0, 4)) for i in at)
        key_ptr.append(len(key))
    counts = rng.integers(0, 6, size=(n_samples, table_len, 16)).astype(numpy.uint32)
    other_counts = rng.integers(0, 6, size=counts.shape).astype(numpy.uint32)
    ncand = numpy.array([1, 3, 7], dtype=I4)
    cand, other = numpy.zeros((n_samples, ld), dtype=I4), numpy.zeros((n_samples, ld), dtype=I4)
    for s in range(n_samples):
        cand[s, :ncand[s]] = rng.choice(n_haps, size=ncand[s], replace=False)
        other[s] = rng.choice(n_haps, size=ld, replace=False)             # candidate lists drawn from other valid haplogroups
    bufs = {"counts": counts, "key_ptr": numpy.array(key_ptr, dtype=I4), "key": numpy.array(key, dtype=I4), "site": site,
            "site_key": site_key, "keep": sentinel((n_samples, ld), U1), "n_uniq": sentinel((n_samples, ld), I4),
            "n_found": sentinel((n_samples, ld), I4)}

    def call(p, h, stream):
        return lib.mxm_check_variants_samples(p["counts"], n_samples, table_len, p["key_ptr"], p["key"], n_haps, p["site"], p["site_key"],
                                              n_sites, table_len - 1, h["cand_host"].ctypes.data, h["ncand_host"].ctypes.data, ld, 2.0,
                                              0.3, 0.5, 0, 2, p["keep"], p["n_uniq"], p["n_found"], stream)
    return make(call, bufs, {"counts": other_counts}, ["keep", "n_uniq", "n_found"],
                host={"cand_host": (cand, other), "ncand_host": (ncand, numpy.array([7, 1, 3], dtype=I4))})


# ---- the alignment walk and the assembly stage ------------------------------------------------------------------------------
N_LABELS = 4


@functools.lru_cache(maxsize=None)
def alignments():
    """test_gpu_assemble.random_columns: 1500 alignments of 750 fragments over a reference of 3000, labels, the table
    length that holds every alignment whatever its mapping quality, and the decoys of the payload columns."""
    import test_gpu_assemble as ga
    rng = numpy.random.default_rng(3000)
    _, srcs = ga.random_sources(rng, 3000)
    cols = ga.random_columns(rng, 1500, srcs, 750)
    label = ga.random_labels(rng, cols)
    ref_len = numpy.zeros(len(cols.ref_start), dtype=I8)
    for i in range(len(ref_len)):
        ops = cols.cigar[cols.cig_ptr[i]:cols.cig_ptr[i + 1]]
        ref_len[i] = sum(int(op >> 4) for op in ops if int(op & 15) in (0, 2, 3, 7, 8))
    table_len = int((numpy.maximum(cols.ref_start, 0) + ref_len).max()) + 1
    letters = numpy.frombuffer(b"ACGT", dtype=U1)
    decoy = {"seq": letters[rng.integers(0, 4, size=len(cols.seq))], "qual": rng.choice([5, 40], size=len(cols.qual)).astype(U1),
             "mapq": rng.choice([60, 0], size=len(cols.mapq)).astype(I4), "is_reverse": (1 - cols.is_reverse).astype(U1),
             "label": ((label + 1) % N_LABELS).astype(I4)}
    return cols, label, table_len, decoy


def _aln_bufs(cols, with_frag=False):
    bufs = {"ref_start": cols.ref_start, "mapq": cols.mapq, "cig_ptr": cols.cig_ptr, "cigar": cols.cigar, "seq_ptr": cols.seq_ptr,
            "seq": cols.seq, "qual": cols.qual, "has_qual": cols.has_qual, "is_reverse": cols.is_reverse}
    if with_frag:
        bufs["frag"] = cols.frag
    return bufs


def _aln_struct(p, cols, n_frag=0):
    from mixemt_amd import _lib
    return _lib.AlnColumns(len(cols.ref_start), n_frag, p["ref_start"], p["mapq"], p.get("frag"), p["cig_ptr"], p["cigar"], p["seq_ptr"],
                           p["seq"], p["qual"], p["has_qual"])


def _observe(lib, labelled):
    cols, label, table_len, dec = alignments()
    bufs = _aln_bufs(cols)
    n_tables = N_LABELS if labelled else 1
    bufs["counts"] = numpy.zeros((n_tables, table_len, 16), dtype=numpy.uint32)
    decoy = {k: dec[k] for k in ("seq", "qual", "mapq", "is_reverse")}
    if labelled:
        bufs["label"], decoy["label"] = label, dec["label"]

    def call(p, h, stream):
        st = _aln_struct(p, cols)
        if labelled:
            return lib.mxm_observe_bases_labelled(ctypes.byref(st), p["is_reverse"], p["label"], N_LABELS, 30, 30, table_len, p["counts"], stream)
        return lib.mxm_observe_bases(ctypes.byref(st), p["is_reverse"], 30, 30, table_len, p["counts"], stream)
    return make(call, bufs, decoy, ["counts"])


@case("mxm_observe_bases", "1500 alignments", "C")
def _(lib):
    return _observe(lib, False)


@case("mxm_observe_bases_labelled", "1500 alignments, 4 labels", "C")
def _(lib):
    return _observe(lib, True)


@functools.lru_cache(maxsize=None)
def pileups():
    """counts[N_LABELS][L][16] of the labelled alignments (tests/_pileup_ref.py), thinned so that ties occur, and the
    non-strict consensus with its tie masks (the guarded alignments module's restatement)."""
    import _pileup_ref
    import test_gpu_guarded_alignments as gal
    cols, label, table_len, _ = alignments()
    per = numpy.stack([_pileup_ref.pileup(gal._subset(cols, numpy.flatnonzero(label == k)), table_len, 30, 30) for k in range(N_LABELS)])
    tables = numpy.zeros((N_LABELS, table_len, 16), dtype=numpy.uint32)
    tables[..., :14] = per[..., :14]
    cons, tied = gal._consensus_ref(per, table_len, 1, 0)
    return tables, cons, tied


@case("mxm_consensus", "non-strict with tie masks", "A")
def _(lib):
    tables, _, _ = pileups()
    n_labels, table_len = tables.shape[:2]
    other = numpy.random.default_rng(15).integers(0, 4, size=tables.shape).astype(numpy.uint32)
    bufs = {"counts": tables, "cons": sentinel((n_labels, table_len), U1), "tied": sentinel((n_labels, table_len), U1),
            "n_tied": numpy.array([5], dtype=numpy.uint32)}

    def call(p, h, stream):
        return lib.mxm_consensus(p["counts"], n_labels, table_len, table_len, 1, 0, p["cons"], p["tied"], p["n_tied"], stream)
    return make(call, bufs, {"counts": other, "n_tied": numpy.array([77], dtype=numpy.uint32)}, ["cons", "tied", "n_tied"])


@case("mxm_new_variants", "rows 2 and 0", "A")
def _(lib):
    _, cons, _ = pileups()
    n_labels, ref_len = cons.shape
    # strict consensus rows: a called base nearly everywhere, so that owners exist
    rng = numpy.random.default_rng(16)
    letters = numpy.frombuffer(b"ACGT", dtype=U1)
    rows_cons = letters[rng.integers(0, 4, size=cons.shape)]
    other = letters[rng.integers(0, 4, size=cons.shape)]
    rows, rows_other = numpy.array([2, 0], dtype=I4), numpy.array([1, 3], dtype=I4)
    bufs = {"cons": rows_cons, "newvar": sentinel(ref_len, numpy.uint32), "n_new": numpy.array([11], dtype=numpy.uint32)}

    def call(p, h, stream):
        return lib.mxm_new_variants(p["cons"], ref_len, n_labels, h["rows"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 2, ref_len,
                                    p["newvar"], p["n_new"], stream)
    return make(call, bufs, {"cons": other, "n_new": numpy.array([99], dtype=numpy.uint32)}, ["newvar", "n_new"],
                host={"rows": (rows, rows_other)})


@case("mxm_first_observed", "1500 alignments", "C")
def _(lib):
    cols, label, table_len, dec = alignments()
    _, cons, tied = pileups()
    bufs = _aln_bufs(cols)
    joined = numpy.random.default_rng(17).integers(0, 3, size=len(label)).astype(I4)
    bufs.update({"label": label, "joined": joined, "tied": tied, "cons": cons})
    decoy = {k: dec[k] for k in ("seq", "qual", "mapq", "label")}
    decoy["joined"] = (2 - joined).astype(I4)
    decoy["cons"] = numpy.full_like(cons, ord("N"))

    def call(p, h, stream):
        st = _aln_struct(p, cols)
        return lib.mxm_first_observed(ctypes.byref(st), p["label"], p["joined"], N_LABELS, 30, 30, table_len, p["tied"], p["cons"], stream)
    return make(call, bufs, decoy, ["cons"])


@case("mxm_extend_assign", "1500 alignments of 750 fragments", "C")
def _(lib):
    cols, label, table_len, dec = alignments()
    n_aln, n_frag = len(label), 750
    rng = numpy.random.default_rng(18)
    owners = numpy.full((table_len, 4), -1, dtype=numpy.int8)
    marked = rng.random(owners.shape) < 0.02
    owners[marked] = rng.integers(0, 2, size=int(marked.sum()))
    joined = rng.integers(0, 3, size=n_aln).astype(I4)
    rows, rows_other = numpy.array([2, 0], dtype=I4), numpy.array([1, 2], dtype=I4)
    bufs = _aln_bufs(cols, with_frag=True)
    bufs.update({"label": label, "joined": joined, "newvar": owners, "frag_state": sentinel(n_frag, I4), "moved_owner": sentinel(n_aln, I4),
                 "n_moved": numpy.array([9], dtype=numpy.uint32)})
    decoy = {k: dec[k] for k in ("seq", "qual", "mapq", "label")}
    decoy["joined"] = (2 - joined).astype(I4)
    decoy["n_moved"] = numpy.array([1000], dtype=numpy.uint32)

    def call(p, h, stream):
        st = _aln_struct(p, cols, n_frag)
        return lib.mxm_extend_assign(ctypes.byref(st), p["label"], p["joined"], 3, N_LABELS, h["rows"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                     2, 7, 30, 30, p["newvar"], table_len, p["frag_state"], p["moved_owner"], p["n_moved"], stream)
    return make(call, bufs, decoy, ["label", "joined", "frag_state", "moved_owner", "n_moved"], host={"rows": (rows, rows_other)})


# ---- the one-shot exchange, world of one ---------------------------------------------------------------------------------
_exchange = []


def exchange(lib):
    """One exchange of a world of one (tests/test_gpu_exchange.py's form), shared by the three cases and released by
    close_exchange()."""
    if not _exchange:
        from mixemt_amd import dist
        _exchange.append(dist.OneShotExchange(3 * 66))
    return _exchange[0]


def close_exchange():
    while _exchange:
        _exchange.pop().close()


def _exchange_case(lib, which):
    sums = numpy.random.default_rng(19).random((3, 66)) * 40.0
    bufs = {"colsum": sums, "state": states(3)}
    if which != "reduce":
        bufs["out"] = sentinel(sums.shape, F8)

    def call(p, h, stream):
        x = exchange(lib)
        if which == "reduce":
            return lib.mxm_exchange_reduce(x.handle, p["colsum"], sums.size, p["state"], 3, stream)
        rc = lib.mxm_exchange_push(x.handle, p["colsum"], sums.size, stream)
        return rc if rc != 0 else lib.mxm_exchange_pull(x.handle, p["out"], sums.size, p["state"], 3, stream)
    return make(call, bufs, {"colsum": nan_like(sums)}, ["colsum", "state"] if which == "reduce" else ["out", "state"])


@case("mxm_exchange_push", "world of one: push, then pull", "A")
def _(lib):
    return _exchange_case(lib, "push")


@case("mxm_exchange_pull", "world of one: push, then pull", "A")
def _(lib):
    return _exchange_case(lib, "pull")


@case("mxm_exchange_reduce", "world of one, in place", "A")
def _(lib):
    return _exchange_case(lib, "reduce")


# ---- mxm_preload ---------------------------------------------------------------------------------------------------------
@case("mxm_preload", "the code object is loaded", "C")
def _(lib):
    # no stream and no buffer of its own: the case orders one small kernel of the library behind it, on the side stream
    a, b = numpy.log(props_of(66, 2, 20))

    def call(p, h, stream):
        rc = lib.mxm_preload()
        return rc if rc != 0 else lib.mxm_l1_exp_diff(p["a"], p["b"], 66, p["l1"], stream)
    return make(call, {"a": a, "b": b, "l1": sentinel(1, F8)}, {"a": nan_like(a), "b": nan_like(b)}, ["l1"])
