"""
The build entries of include/mixemt_hip.h called through ctypes with every device pointer guard-banded at its exact
documented size (tests/_guarded.py): mxm_expand_tables, mxm_build_em_matrix, mxm_build_em_matrix_lut, _lut_rows, _sparse and
mxm_build_em_records.  Reference: oracle.c_oracle.build_em_matrix (the reference's arithmetic in its order), bit for bit, as
the existing build tests compare.  Tables are synthetic so that every width can be reached: a few markers per site,
a band of sites with many (rows of hundreds of distinct values: wide records, and the fallback list by that rule), rows of
1 .. 20 observations plus one of 70 (the long rows' launch) and one of 130 (beyond every marker kernel: the fallback list).
"""
import numpy
import pytest

from _guarded_abi import ENC_MAX_CODES, load_lib, records, stream as _stream, sync as _sync
from _guarded import guarded, guarded_2d, guarded_from
from oracle import c_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 257, 700)
WIDTHS = (66, 1026, 5408, 8192)
N_SITES = 160


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _tables(n_haps, seed):
    """Expected bases E[S][lde] (pad bytes 0), their marker form, the lookup-table form and the per-site log terms."""
    rng = numpy.random.default_rng(seed)
    letters = numpy.frombuffer(b"ACGT", dtype=numpy.uint8)
    lde = (n_haps + 7) // 8 * 8 + 8
    maj = letters[rng.integers(0, 4, size=N_SITES)]
    exp = numpy.zeros((N_SITES, lde), dtype=numpy.uint8)
    exp[:, :n_haps] = maj[:, None]
    pool = rng.choice(n_haps, size=min(n_haps, 400), replace=False)
    mk_ptr, mk_hap, mk_base = [0], [], []
    for s in range(N_SITES):
        if 40 <= s < 64:                                                   # the band of many markers
            haps = rng.choice(pool, size=min(64, n_haps // 4), replace=False)
        else:
            haps = rng.choice(n_haps, size=min(n_haps // 4, int(rng.integers(0, 13))), replace=False)
        haps = numpy.sort(haps)
        if s == 7:
            haps = numpy.union1d(haps, [n_haps - 1])                       # the last haplogroup carries a marker
        for h in haps:
            base = letters[(int(numpy.flatnonzero(letters == maj[s])[0]) + int(rng.integers(1, 4))) % 4]
            exp[s, h] = base
            mk_hap.append(h)
            mk_base.append(base)
        mk_ptr.append(len(mk_hap))
    mu = rng.uniform(0.001, 0.01, size=N_SITES)
    code_of = numpy.zeros(256, dtype=numpy.uint8)
    code_of[letters] = numpy.arange(1, 5, dtype=numpy.uint8) << 3
    obsmap = numpy.full(256, 15 << 3, dtype=numpy.uint8)
    obsmap[letters] = code_of[letters]
    return {"H": n_haps, "lde": lde, "exp": exp, "maj": maj, "mk_ptr": numpy.array(mk_ptr, dtype=numpy.int32),
            "mk_hap": numpy.array(mk_hap, dtype=numpy.uint16), "mk_base": numpy.array(mk_base, dtype=numpy.uint8),
            "lhit": numpy.log(1.0 - mu), "lmiss": numpy.log(mu / 3.0), "code_of": code_of, "obsmap": obsmap,
            "ecode": code_of[exp]}


def _reads(tab, n_rows, seed):
    """CSR observations: consecutive sites from a random start; the base is the majority's, a marker's, or noise."""
    rng = numpy.random.default_rng(seed)
    counts = rng.integers(1, 21, size=n_rows)
    if n_rows > 5:
        counts[3], counts[5] = 70, 130
    row_ptr = numpy.zeros(n_rows + 1, dtype=numpy.int64)
    numpy.cumsum(counts, out=row_ptr[1:])
    site = numpy.empty(int(row_ptr[-1]), dtype=numpy.uint16)
    obs = numpy.empty(int(row_ptr[-1]), dtype=numpy.uint8)
    for r in range(n_rows):
        start = int(rng.integers(0, N_SITES - counts[r] + 1))
        if r % 4 == 1 and counts[r] <= 20:
            start = int(rng.integers(40, 64 - 20 + 1))                     # inside the band of many markers
        sl = slice(int(row_ptr[r]), int(row_ptr[r + 1]))
        site[sl] = numpy.arange(start, start + counts[r])
        pick = rng.random(counts[r])
        col = rng.integers(0, tab["H"], size=counts[r])
        obs[sl] = numpy.where(pick < 0.6, tab["maj"][site[sl]], tab["exp"][site[sl], col])
        obs[sl][pick > 0.97] = ord("N")
    return row_ptr, site, obs


def _device_tables(tab):
    return {"exp": guarded_2d(N_SITES, tab["H"], tab["lde"], numpy.uint8, 8, DEV, pad=0).put(tab["exp"][:, :tab["H"]]),
            "ecode": guarded_2d(N_SITES, tab["H"], tab["lde"], numpy.uint8, 8, DEV, pad=0).put(tab["ecode"][:, :tab["H"]]),
            "maj": guarded_from(tab["maj"], numpy.uint8, 1, DEV), "mk_ptr": guarded_from(tab["mk_ptr"], numpy.int32, 4, DEV),
            "mk_hap": guarded_from(tab["mk_hap"], numpy.uint16, 2, DEV), "mk_base": guarded_from(tab["mk_base"], numpy.uint8, 1, DEV),
            "lhit": guarded_from(tab["lhit"], numpy.float64, 8, DEV), "lmiss": guarded_from(tab["lmiss"], numpy.float64, 8, DEV),
            "obsmap": guarded_from(tab["obsmap"], numpy.uint8, 1, DEV)}


def _device_reads(row_ptr, site, obs):
    return {"row_ptr": guarded_from(row_ptr, numpy.int64, 8, DEV), "site": guarded_from(site, numpy.uint16, 2, DEV),
            "obs": guarded_from(obs, numpy.uint8, 1, DEV)}


def _check_inputs(bufs, what):
    for name, buf in bufs.items():
        if hasattr(buf, "check_pads"):
            buf.check("%s %s" % (name, what), pads="unchanged")
        else:
            buf.check("%s %s" % (name, what))


def _ldm(n_haps, align):
    return n_haps + 3 if align == 8 else n_haps + 2 + (n_haps & 1)


@pytest.fixture(scope="module", params=WIDTHS)
def case(request):
    """Per width: the tables, the reads of every row count, the oracle's matrices -- made once, never written."""
    n_haps = request.param
    tab = _tables(n_haps, 10 + n_haps)
    reads = {n: _reads(tab, n, 100 * n_haps + n) for n in ROWS}
    want = {n: c_oracle.build_em_matrix(tab["exp"], tab["lhit"], tab["lmiss"], *reads[n], n_haps) for n in ROWS}
    return tab, reads, want


# ---- mxm_expand_tables ----------------------------------------------------------------------------------------------------
def test_expand_tables(lib, case):
    """mixemt_hip.h: "out[s][h] = map256[maj[s]] for every haplogroup h < H, then out[s][mk_hap[j]] = map256[mk_base[j]] for
    the markers j of site s; columns H .. lde are 0.  map256 NULL = identity"."""
    tab, _, _ = case
    dev = _device_tables(tab)
    for name, table in ((None, tab["exp"]), ("code_of", tab["ecode"])):
        map_buf = None if name is None else guarded_from(tab[name], numpy.uint8, 1, DEV)
        out = guarded_2d(N_SITES, tab["H"], tab["lde"], numpy.uint8, 8, DEV)
        assert lib.mxm_expand_tables(dev["maj"].ptr, dev["mk_ptr"].ptr, dev["mk_hap"].ptr, dev["mk_base"].ptr,
                                     None if map_buf is None else map_buf.ptr, N_SITES, tab["H"], tab["lde"], out.ptr,
                                     _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_inputs(dev, "H=%d" % tab["H"])
        if map_buf is not None:
            map_buf.check("map256")
        out.check("out H=%d map=%s" % (tab["H"], name), pads="zero")
        assert numpy.array_equal(out.get(), table[:, :tab["H"]])


# ---- the cell-by-cell builds ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [8, 16])
def test_build_em_matrix_and_its_lookup_table_forms(lib, case, align):
    """mixemt_hip.h: "M[r][h] = sum over the row's observations k, IN ORDER, of (E[site_k][h] == obs_k ? lhit : lmiss)";
    the lookup-table path "same arithmetic, same order, same bits", with and without `order`; mxm_build_em_matrix_lut_rows
    "row rows[i] of the CSR -> row i of M_out[n_rows][ldm]".  The pad columns [H, ldm) of M are left alone."""
    tab, reads, want = case
    n_haps, lde, ldm = tab["H"], tab["lde"], _ldm(tab["H"], align)
    dev = _device_tables(tab)
    for n_rows in ROWS:
        csr = _device_reads(*reads[n_rows])
        what = "R=%d H=%d align=%d" % (n_rows, n_haps, align)
        rng = numpy.random.default_rng(n_rows)
        order = guarded_from(rng.permutation(n_rows), numpy.int64, 8, DEV)
        runs = [("mxm_build_em_matrix", lambda m: lib.mxm_build_em_matrix(
                    dev["exp"].ptr, lde, dev["lhit"].ptr, dev["lmiss"].ptr, csr["row_ptr"].ptr, csr["site"].ptr, csr["obs"].ptr,
                    n_rows, n_haps, N_SITES, m.ptr, ldm, _stream()))]
        for name, order_ptr in (("lut", None), ("lut, ordered", order.ptr)):
            runs.append((name, lambda m, order_ptr=order_ptr: lib.mxm_build_em_matrix_lut(
                dev["ecode"].ptr, lde, dev["lhit"].ptr, dev["lmiss"].ptr, dev["obsmap"].ptr, csr["row_ptr"].ptr, csr["site"].ptr,
                csr["obs"].ptr, order_ptr, n_rows, n_haps, N_SITES, m.ptr, ldm, _stream())))
        for name, call in runs:
            mat = guarded_2d(n_rows, n_haps, ldm, numpy.float64, align, DEV)
            assert call(mat) == 0, lib.mxm_last_error()
            _sync()
            _check_inputs(dev, what)
            _check_inputs(csr, what)
            order.check("order " + what)
            mat.check("M %s (%s)" % (what, name), pads="unchanged")
            assert numpy.array_equal(mat.get(), want[n_rows]), (what, name)
        # a list of rows into a compact matrix: every third row, the last one first
        rows = numpy.arange(n_rows - 1, -1, -3, dtype=numpy.int64)
        r_buf = guarded_from(rows, numpy.int64, 8, DEV)
        sub = guarded_2d(len(rows), n_haps, ldm, numpy.float64, align, DEV)
        assert lib.mxm_build_em_matrix_lut_rows(dev["ecode"].ptr, lde, dev["lhit"].ptr, dev["lmiss"].ptr, dev["obsmap"].ptr,
                                                csr["row_ptr"].ptr, csr["site"].ptr, csr["obs"].ptr, r_buf.ptr, len(rows), n_haps,
                                                N_SITES, sub.ptr, ldm, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_inputs(dev, what)
        _check_inputs(csr, what)
        r_buf.check("rows " + what)
        sub.check("M_out " + what, pads="unchanged")
        assert numpy.array_equal(sub.get(), want[n_rows][rows]), what


# ---- the marker builds ----------------------------------------------------------------------------------------------------
def _fallback(fb, n_fb, n_rows, what):
    """The list as the kernel appended it: *n_fallback distinct rows; the entries past it are left alone."""
    count = int(n_fb.get(numpy.int64)[0])
    entries = fb.get(numpy.int64)
    assert 0 <= count <= n_rows, what
    rows = entries[:count]
    assert len(set(rows.tolist())) == count and ((rows >= 0) & (rows < n_rows)).all(), what
    assert (entries[count:] == -1).all(), "fallback[] past *n_fallback was written (%s)" % what
    return numpy.sort(rows)


def _finish_with_lut(lib, dev, csr, tab, rows, n_rows, mat, ldm):
    """What the header tells the caller to do with the list: mxm_build_em_matrix_lut(order = fallback, R = *n_fallback)."""
    if len(rows) == 0:
        return
    order = guarded_from(rows, numpy.int64, 8, DEV)
    assert lib.mxm_build_em_matrix_lut(dev["ecode"].ptr, tab["lde"], dev["lhit"].ptr, dev["lmiss"].ptr, dev["obsmap"].ptr,
                                       csr["row_ptr"].ptr, csr["site"].ptr, csr["obs"].ptr, order.ptr, len(rows), tab["H"],
                                       N_SITES, mat.ptr, ldm, _stream()) == 0, lib.mxm_last_error()
    _sync()
    order.check("order = fallback")


def _is_sentinel(rows):
    return bool((numpy.ascontiguousarray(rows).view(numpy.uint8) == 0xFF).all())


@pytest.mark.parametrize("align", [8, 16])
def test_build_em_matrix_sparse_leaves_the_fallback_rows_alone(lib, case, align):
    """mixemt_hip.h: rows beyond the marker kernels "are NOT written: their indices are appended to fallback[] (device
    int64[R], *n_fallback = how many, device) and the caller builds them with mxm_build_em_matrix_lut"."""
    tab, reads, want = case
    n_haps, ldm = tab["H"], _ldm(tab["H"], align)
    dev = _device_tables(tab)
    seen = 0
    for n_rows in ROWS:
        csr = _device_reads(*reads[n_rows])
        what = "R=%d H=%d align=%d" % (n_rows, n_haps, align)
        mat = guarded_2d(n_rows, n_haps, ldm, numpy.float64, align, DEV)
        fb, n_fb = guarded(8 * n_rows, 8, DEV), guarded(8, 8, DEV)
        assert lib.mxm_build_em_matrix_sparse(dev["maj"].ptr, dev["lhit"].ptr, dev["lmiss"].ptr, dev["mk_ptr"].ptr, dev["mk_hap"].ptr,
                                              dev["mk_base"].ptr, csr["row_ptr"].ptr, csr["site"].ptr, csr["obs"].ptr, None, n_rows,
                                              n_haps, N_SITES, mat.ptr, ldm, fb.ptr, n_fb.ptr, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_inputs(dev, what)
        _check_inputs(csr, what)
        fb.check("fallback " + what)
        n_fb.check("n_fallback " + what)
        mat.check("M " + what, pads="unchanged")
        rows = _fallback(fb, n_fb, n_rows, what)
        seen += len(rows)
        got = mat.get()
        built = numpy.setdiff1d(numpy.arange(n_rows), rows)
        assert numpy.array_equal(got[built], want[n_rows][built]), what
        assert _is_sentinel(got[rows]), "a row on the fallback list was written (%s)" % what
        if n_rows > 5:
            assert 5 in rows, what                                     # 130 observations: beyond every marker kernel
        _finish_with_lut(lib, dev, csr, tab, rows, n_rows, mat, ldm)
        mat.check("M " + what, pads="unchanged")
        assert numpy.array_equal(mat.get(), want[n_rows]), what
    assert seen > 0


def _decode_records(rec, rec_off, ndist, rowmax, n_haps, limit, want, what):
    """Every record inside [0, limit), no two overlapping (_guarded_abi.records), and each one's contents:
    M[r][h] = mtable[codes[h]] the oracle's bits, P table = exp(log table - rowmax)."""
    recs, spans = records(rec, rec_off, ndist, n_haps, limit, what)
    for r, codes, ptab, mtab in recs:
        assert numpy.array_equal(mtab[codes], want[r]), (what, r)
        # the shift is the table's largest entry: the row's maximum unless code 0 (the marker-free value, listed whether
        # or not a haplogroup holds it) is the largest and unused
        assert rowmax[r] == mtab.max() and rowmax[r] >= want[r].max(), (what, r)
        assert rowmax[r] == want[r].max() or (mtab[0] == rowmax[r] and not (codes == 0).any()), (what, r)
        assert numpy.allclose(ptab, numpy.exp(mtab - rowmax[r]), rtol=1e-15, atol=0), (what, r)
    return spans


@pytest.mark.parametrize("dense", [True, False])
def test_build_em_records_inside_exactly_record_bytes_and_a_third_of_what_it_needs(lib, case, dense):
    """mixemt_hip.h: "rec_bytes >= mxm_record_bytes(R, H) never overflows"; "rows that get no record have ndist[r] = 0: the
    rows on the fallback list, which the caller builds densely; with M given their dense row is NOT written either";
    "stats[0] = bytes used, stats[1] = rows without a record".  Then once more with a third of stats[0]: rows that no longer
    fit get no record (ndist = 0, their dense row written when M is given), nothing is written past rec_bytes, and stats[0]
    is still the size that suffices."""
    tab, reads, want = case
    n_haps, ldm = tab["H"], tab["H"] + 3
    ldc = (n_haps + 7) // 8 * 8
    dev = _device_tables(tab)
    wide = 0
    for n_rows in ROWS:
        csr = _device_reads(*reads[n_rows])
        full = lib.mxm_record_bytes(n_rows, n_haps)
        used_full = None
        for rec_bytes in (full, None):
            if rec_bytes is None:
                rec_bytes = max(ldc + 16 * ENC_MAX_CODES, used_full // 3)
                if rec_bytes >= used_full:
                    continue                                           # (a single short row: nothing to overflow)
            what = "R=%d H=%d rec_bytes=%d dense=%s" % (n_rows, n_haps, rec_bytes, dense)
            mat = guarded_2d(n_rows, n_haps, ldm, numpy.float64, 8, DEV) if dense else None
            out = {"rec": guarded(rec_bytes, 16, DEV), "rec_off": guarded(8 * n_rows, 8, DEV), "ndist": guarded(4 * n_rows, 4, DEV),
                   "rowmax": guarded(8 * n_rows, 8, DEV), "stats": guarded(16, 8, DEV), "fallback": guarded(8 * n_rows, 8, DEV),
                   "n_fallback": guarded(8, 8, DEV)}
            assert lib.mxm_build_em_records(dev["maj"].ptr, dev["lhit"].ptr, dev["lmiss"].ptr, dev["mk_ptr"].ptr, dev["mk_hap"].ptr,
                                            dev["mk_base"].ptr, csr["row_ptr"].ptr, csr["site"].ptr, csr["obs"].ptr, None, n_rows,
                                            n_haps, N_SITES, mat.ptr if dense else None, ldm if dense else 0, out["rec"].ptr,
                                            rec_bytes, out["rec_off"].ptr, out["ndist"].ptr, out["rowmax"].ptr, out["stats"].ptr,
                                            out["fallback"].ptr, out["n_fallback"].ptr, _stream()) == 0, lib.mxm_last_error()
            _sync()
            _check_inputs(dev, what)
            _check_inputs(csr, what)
            _check_inputs(out, what)
            if dense:
                mat.check("M " + what, pads="unchanged")
            used, n_rest = (int(v) for v in out["stats"].get(numpy.int64))
            ndist = out["ndist"].get(numpy.int32)
            rows = _fallback(out["fallback"], out["n_fallback"], n_rows, what)
            assert n_rest == int((ndist == 0).sum()) and (ndist[rows] == 0).all() and (ndist >= 0).all(), what
            spans = _decode_records(out["rec"].get(numpy.uint8), out["rec_off"].get(numpy.int64), ndist,
                                    out["rowmax"].get(numpy.float64), n_haps, min(rec_bytes, used), want[n_rows], what)
            wide += int((ndist > ENC_MAX_CODES).sum())
            if used_full is None:
                used_full, ndist_full = used, ndist
                assert used <= rec_bytes and used == sum(b - a for a, b in spans), what
                assert numpy.array_equal(numpy.flatnonzero(ndist == 0), rows), what      # only the list's rows lack a record
            else:
                assert used == used_full > rec_bytes, what             # the size that would have sufficed
                lost = (ndist == 0) & (ndist_full > 0)
                assert lost.any() and numpy.array_equal(ndist[~lost], ndist_full[~lost]), what
            if dense:
                got = mat.get()
                built = numpy.setdiff1d(numpy.arange(n_rows), rows)
                assert numpy.array_equal(got[built], want[n_rows][built]), what
                assert _is_sentinel(got[rows]), "the dense row of a row on the fallback list was written (%s)" % what
                _finish_with_lut(lib, dev, csr, tab, rows, n_rows, mat, ldm)
                mat.check("M " + what, pads="unchanged")
                assert numpy.array_equal(mat.get(), want[n_rows]), what
    assert n_haps < 1000 or wide > 0                                   # the band of many markers makes 16-bit records
