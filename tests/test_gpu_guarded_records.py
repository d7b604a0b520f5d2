"""
The row-dictionary entries of include/mixemt_hip.h called through ctypes with every device pointer -- the device arrays
inside mxm_coded included -- guard-banded at its exact documented size (tests/_guarded.py): mxm_encode_rows,
mxm_decode_rows, mxm_scatter_records, mxm_em_iter_coded, mxm_em_step_coded, mxm_gather_columns_coded,
mxm_row_argmax_votes_coded, and -- further down, over rows with few distinct quads -- mxm_build_quads, mxm_quad_lists,
mxm_em_iter_coded beside a quad dictionary and mxm_em_loop_coded.  The matrices mix rows of a few values (byte codes), of about 300 and of up to 1024 (16-bit
codes: "wide") and of more than 1024 (no record: the dense rest), as tests/test_gpu_coded.py does.  References: numpy for
the records' contents, oracle.em_oracle for the passes.
"""
import ctypes

import numpy
import pytest

from _guarded_abi import (ENC_MAX_CODES, check_all as _check_coded, coded as _coded, encode_rows as _encode, load_lib, records,
                          stream as _stream, sync as _sync)
from _guarded import guarded, guarded_2d, guarded_from
from oracle import em_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 257, 700)
WIDTHS = (66, 1026, 5408, 8192)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _matrix(rng, n_rows, n_haps):
    kinds = rng.integers(0, 4, size=n_rows)                        # 0: few values, 1: ~300, 2: up to 1024, 3: too many
    kinds[:4] = [1, 0, 2, 3][:min(4, n_rows)]
    n_val = numpy.where(kinds == 0, 9, numpy.where(kinds == 1, min(300, n_haps), numpy.where(kinds == 2, min(1024, n_haps), n_haps)))
    mat = numpy.empty((n_rows, n_haps))
    for r in range(n_rows):
        vals = rng.normal(-20.0, 6.0, size=n_val[r])
        idx = rng.integers(0, n_val[r], size=n_haps)
        idx[rng.permutation(n_haps)[:n_val[r]]] = numpy.arange(n_val[r])          # every value occurs
        mat[r] = vals[idx]
    if n_rows > 10:
        mat[9, :n_haps // 3] = -numpy.inf                          # -inf is a value like any other
    return mat


@pytest.fixture(scope="module", params=WIDTHS)
def case(request):
    """Per width: the matrices of every row count, their distinct-value counts and weights: made once, never written."""
    n_haps = request.param
    rng = numpy.random.default_rng(n_haps)
    out = {}
    for n_rows in ROWS:
        mat = _matrix(rng, n_rows, n_haps)
        out[n_rows] = (mat, numpy.array([len(numpy.unique(row)) for row in mat]), rng.integers(1, 4, size=n_rows).astype(numpy.float64))
    return n_haps, out


def _check_records(out, mat, limit, what):
    """Every record inside [0, limit), no two overlapping (_guarded_abi.records); codes ++ P table ++ log table decode to
    the row bit for bit, rowmax is the row's maximum (0 if not finite) and P what mxm_linearize writes."""
    n_haps = mat.shape[1]
    ndist, rowmax = out["ndist"].get(numpy.int32), out["rowmax"].get(numpy.float64)
    recs, spans = records(out["rec"].get(numpy.uint8), out["rec_off"].get(numpy.int64), ndist, n_haps, limit, what)
    for r, codes, ptab, mtab in recs:
        assert numpy.array_equal(mtab[codes], mat[r]), (what, r)
        top = mat[r].max()
        assert rowmax[r] == (top if numpy.isfinite(top) else 0.0), (what, r)
        with numpy.errstate(under="ignore"):
            assert numpy.allclose(ptab[codes], numpy.exp(mat[r] - rowmax[r]), rtol=1e-15, atol=0), (what, r)
    return ndist, spans


def test_encode_rows_inside_exactly_coded_bytes_and_a_third_of_what_it_needs(lib, case):
    """mixemt_hip.h: "mxm_coded_bytes(R, H): record buffer size that can never overflow.  A smaller buffer is allowed: rows
    that no longer fit get no record, and stats[0] > rec_bytes afterwards says so (and is the size that would have
    sufficed)"; "stats[0] = bytes asked for, stats[1] = rows left dense"; rows of more than 1024 values get ndist = 0.
    M comes at the doubles' own alignment with an odd stride."""
    n_haps, mats = case
    ldc = (n_haps + 7) // 8 * 8
    for n_rows in ROWS:
        mat, uniq, _ = mats[n_rows]
        what = "R=%d H=%d" % (n_rows, n_haps)
        full = lib.mxm_coded_bytes(n_rows, n_haps)
        out, (used, n_rest) = _encode(lib, mat, n_haps + 3, full, what)
        ndist, spans = _check_records(out, mat, used, what)
        assert numpy.array_equal(ndist, numpy.where(uniq <= 1024, uniq, 0)), what
        assert used <= full and used == sum(b - a for a, b in spans) and n_rest == int((ndist == 0).sum()), what
        third = max(ldc + 16 * ENC_MAX_CODES, used // 3)
        if third >= used:
            continue
        small, (used_s, n_rest_s) = _encode(lib, mat, n_haps + 3, third, what + " rec_bytes=%d" % third)
        ndist_s, _ = _check_records(small, mat, third, what + " rec_bytes=%d" % third)
        assert used_s > third and used_s >= used, what                 # "the size that would have sufficed"
        lost = (ndist_s == 0) & (ndist > 0)
        assert lost.any() and numpy.array_equal(ndist_s[~lost], ndist[~lost]) and n_rest_s == int((ndist_s == 0).sum()), what


def test_decode_and_scatter_records(lib, case):
    """mixemt_hip.h: "mxm_decode_rows: P[r][:] = row r decoded, coded rows only" -- the rows without a record and the pad
    columns of P are left alone; mxm_scatter_records: "where sub_nd[i] > 0, rec_off[rows[i]] = sub_off[i] + base,
    ndist[rows[i]] = sub_nd[i], rowmax[rows[i]] = sub_rm[i]" -- every other entry is left alone."""
    n_haps, mats = case
    for n_rows in ROWS:
        mat, _, wts = mats[n_rows]
        what = "R=%d H=%d" % (n_rows, n_haps)
        st, bufs, ndist, rest = _coded(lib, mat, wts, what)
        ldp = n_haps + 3
        lin = guarded_2d(n_rows, n_haps, ldp, numpy.float64, 8, DEV)
        assert lib.mxm_decode_rows(ctypes.byref(st), n_haps, lin.ptr, ldp, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_coded(bufs, what)
        lin.check("P " + what, pads="unchanged")
        got = lin.get()
        coded = numpy.flatnonzero(ndist > 0)
        top = mat[coded].max(axis=1)
        with numpy.errstate(under="ignore"):
            want = numpy.exp(mat[coded] - numpy.where(numpy.isfinite(top), top, 0.0)[:, None])
        assert numpy.allclose(got[coded], want, rtol=1e-15, atol=0), what
        assert (got[rest].view(numpy.uint8) == 0xFF).all(), "a row without a record was written (%s)" % what
        # scatter: every other row of a compact side list, half of them without a record
        rng = numpy.random.default_rng(n_rows)
        rows = numpy.arange(0, n_rows, 2, dtype=numpy.int64)[::-1].copy()
        sub_nd = rng.integers(0, 3, size=len(rows)).astype(numpy.int32) * 7
        sub_off = rng.integers(0, 1 << 40, size=len(rows)).astype(numpy.int64)
        sub_rm = rng.normal(size=len(rows))
        ins = {"rows": guarded_from(rows, numpy.int64, 8, DEV), "sub_off": guarded_from(sub_off, numpy.int64, 8, DEV),
               "sub_nd": guarded_from(sub_nd, numpy.int32, 4, DEV), "sub_rm": guarded_from(sub_rm, numpy.float64, 8, DEV)}
        outs = {"rec_off": guarded(8 * n_rows, 8, DEV), "ndist": guarded(4 * n_rows, 4, DEV), "rowmax": guarded(8 * n_rows, 8, DEV)}
        assert lib.mxm_scatter_records(ins["rows"].ptr, len(rows), ins["sub_off"].ptr, ins["sub_nd"].ptr, ins["sub_rm"].ptr, 4096,
                                       outs["rec_off"].ptr, outs["ndist"].ptr, outs["rowmax"].ptr, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_coded(ins, what)
        _check_coded(outs, what)
        want_off, want_nd = numpy.full(n_rows, -1, dtype=numpy.int64), numpy.full(n_rows, -1, dtype=numpy.int32)
        want_rm = numpy.frombuffer(b"\xff" * (8 * n_rows), dtype=numpy.float64).copy()
        hit = sub_nd > 0
        want_off[rows[hit]], want_nd[rows[hit]], want_rm[rows[hit]] = sub_off[hit] + 4096, sub_nd[hit], sub_rm[hit]
        assert numpy.array_equal(outs["rec_off"].get(numpy.int64), want_off) and numpy.array_equal(outs["ndist"].get(numpy.int32), want_nd)
        assert numpy.array_equal(outs["rowmax"].get(numpy.uint8), want_rm.view(numpy.uint8)), what


@pytest.mark.parametrize("n_runs", [1, 4, 5, 9])
def test_em_iter_coded_over_records_wide_rows_and_a_dense_rest(lib, case, n_runs):
    """mixemt_hip.h: "mxm_em_iter_coded = mxm_em_iter over a coded matrix (w[R] indexes all rows, coded or not)"; restarts
    with state[b].done != 0 keep their colsum row; only .error of the state is ever written; ws is exactly
    mxm_workspace_bytes(R, H, B)."""
    n_haps, mats = case
    rng = numpy.random.default_rng(n_haps + n_runs)
    for n_rows in ROWS:
        mat, _, wts = mats[n_rows]
        what = "R=%d H=%d B=%d" % (n_rows, n_haps, n_runs)
        st, bufs, ndist, rest = _coded(lib, mat, wts, what)
        props = rng.dirichlet([1.0] * n_haps, size=n_runs)
        done = (1,) if n_runs > 1 else ()
        raw = numpy.zeros(n_runs * 6, dtype=numpy.int32)
        raw[[6 * b for b in done]] = 1
        run = {"w": guarded_from(wts, numpy.float64, 8, DEV), "props": guarded_from(props, numpy.float64, 8, DEV),
               "state": guarded_from(raw, numpy.int32, 8, DEV), "colsum": guarded(8 * n_runs * n_haps, 8, DEV)}
        ws_bytes = lib.mxm_workspace_bytes(n_rows, n_haps, n_runs)
        run["ws"] = guarded(ws_bytes, 8, DEV, row_bytes=8 * (n_haps + 8))
        assert lib.mxm_em_iter_coded(ctypes.byref(st), run["w"].ptr, run["props"].ptr, n_haps, n_runs, run["state"].ptr,
                                     run["colsum"].ptr, run["ws"].ptr, ws_bytes, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_coded(bufs, what)
        _check_coded(run, what)
        assert numpy.array_equal(run["state"].get(numpy.int32), raw), what
        got = run["colsum"].get(numpy.float64, (n_runs, n_haps))
        for b in range(n_runs):
            if b in done:
                assert (got[b].view(numpy.uint8) == 0xFF).all(), "colsum row of finished restart %d was written (%s)" % (b, what)
                continue
            with numpy.errstate(divide="ignore", invalid="ignore", under="ignore"):
                _, new = em_oracle.em_step(mat, wts, numpy.log(props[b]), numpy.empty_like(mat))
            assert numpy.abs(got[b] * props[b] - numpy.exp(new) * wts.sum()).max() <= 1e-12 * wts.sum(), (what, b)


def test_record_consumers_with_a_dense_rest(lib, case):
    """mxm_em_step_coded ("out[r][h] = (ln_props[h] + M[r][h]) - (rowmax[r] + log(sum_h props[h] * P[r][h]))", rows without
    a record from M_rest / rest_rows), mxm_gather_columns_coded and mxm_row_argmax_votes_coded ("best[r] = first index of
    max_h ..."; votes summed without float atomics; ws exactly mxm_workspace_bytes(R, H, 1)).  The pad columns of out are
    left alone, those of M_rest never read."""
    n_haps, mats = case
    rng = numpy.random.default_rng(n_haps + 77)
    for n_rows in ROWS:
        mat, _, wts = mats[n_rows]
        what = "R=%d H=%d" % (n_rows, n_haps)
        st, bufs, ndist, rest = _coded(lib, mat, wts, what)
        ld_rest = n_haps + 3
        if len(rest):
            bufs["M_rest"] = guarded_2d(len(rest), n_haps, ld_rest, numpy.float64, 8, DEV).put(mat[rest])
            bufs["rest_rows"] = guarded_from(rest, numpy.int64, 8, DEV)
        m_rest = bufs["M_rest"].ptr if len(rest) else None
        rest_rows = bufs["rest_rows"].ptr if len(rest) else None
        props = rng.dirichlet([1.0] * n_haps)
        lnp = numpy.log(props)
        bufs["ln_props"], bufs["props"] = guarded_from(lnp, numpy.float64, 8, DEV), guarded_from(props, numpy.float64, 8, DEV)
        bufs["w"] = guarded_from(wts + 0.25, numpy.float64, 8, DEV)
        with numpy.errstate(divide="ignore", invalid="ignore", under="ignore"):
            want_mix, _ = em_oracle.em_step(mat, wts, lnp, numpy.empty_like(mat))
        # the posterior
        ldo = n_haps + 3
        out = guarded_2d(n_rows, n_haps, ldo, numpy.float64, 8, DEV)
        assert lib.mxm_em_step_coded(ctypes.byref(st), n_haps, bufs["ln_props"].ptr, bufs["props"].ptr, bufs["rowmax"].ptr, m_rest,
                                     ld_rest if len(rest) else 0, rest_rows, len(rest), out.ptr, ldo, 0, _stream()) == 0, \
            lib.mxm_last_error()
        _sync()
        _check_coded(bufs, what)
        out.check("out " + what, pads="unchanged")
        got = out.get()
        fin = numpy.isfinite(want_mix)
        assert numpy.array_equal(numpy.isfinite(got), fin), what
        assert numpy.abs(got[fin] - want_mix[fin]).max() < 1e-10, what
        # the column gather
        cols = rng.integers(0, n_haps, size=5).astype(numpy.int32)
        cols[0] = n_haps - 1
        c_buf = guarded_from(cols, numpy.int32, 4, DEV)
        sub = guarded_2d(n_rows, 5, 8, numpy.float64, 8, DEV)
        assert lib.mxm_gather_columns_coded(ctypes.byref(st), n_haps, c_buf.ptr, 5, m_rest, ld_rest if len(rest) else 0, rest_rows,
                                            len(rest), sub.ptr, 8, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_coded(bufs, what)
        c_buf.check("cols " + what)
        sub.check("gathered " + what, pads="unchanged")
        assert numpy.array_equal(sub.get(), mat[:, cols]), what
        # the vote
        best = guarded(4 * n_rows, 4, DEV)
        votes = guarded(8 * n_haps, 8, DEV)
        ws_bytes = lib.mxm_workspace_bytes(n_rows, n_haps, 1)
        ws = guarded(ws_bytes, 8, DEV, row_bytes=8 * (n_haps + 8))
        assert lib.mxm_row_argmax_votes_coded(ctypes.byref(st), n_haps, 1, bufs["ln_props"].ptr, None, None, m_rest,
                                              ld_rest if len(rest) else 0, rest_rows, len(rest), bufs["w"].ptr, best.ptr, votes.ptr,
                                              ws.ptr, ws_bytes, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_coded(bufs, what)
        for name, buf in (("best", best), ("votes", votes), ("ws", ws)):
            buf.check("%s %s" % (name, what))
        want_best = (lnp[None, :] + mat).argmax(axis=1)
        assert numpy.array_equal(best.get(numpy.int32), want_best), what
        assert numpy.array_equal(votes.get(numpy.float64), numpy.bincount(want_best, weights=wts + 0.25, minlength=n_haps)), what


# ---- the quad dictionary beside the records -------------------------------------------------------------------------------
QUAD_CHUNK = 64 * 1024                      # the encoders hand qrec out in pieces of this size (csrc/quad_kernels.hpp)


def _run_matrix(rng, n_rows, n_haps):
    """Rows as build_em_matrix makes them -- one value nearly everywhere, a few columns deviating: few distinct QUADS --
    with every fifth row of nine values at random (byte-coded, but too many quads) and row 2 of 300 values (wide)."""
    mat = numpy.empty((n_rows, n_haps))
    for r in range(n_rows):
        if r % 5 == 4:
            mat[r] = rng.normal(-20.0, 6.0, size=9)[rng.integers(0, 9, size=n_haps)]
            continue
        base = rng.normal(-20.0, 6.0)
        mat[r] = base
        dev = rng.choice(n_haps, size=int(rng.integers(0, min(40, n_haps // 2))), replace=False)
        mat[r, dev] = base - 8.0 * rng.integers(1, 6, size=len(dev))
    if n_rows > 2 and n_haps >= 300:
        mat[2] = rng.normal(-20.0, 6.0, size=300)[numpy.concatenate([numpy.arange(300), rng.integers(0, 300, size=n_haps - 300)])]
    return mat


@pytest.fixture(scope="module")
def quad_case(case):
    n_haps, _ = case
    rng = numpy.random.default_rng(9000 + n_haps)
    return n_haps, {n: (_run_matrix(rng, n, n_haps), rng.integers(1, 4, size=n).astype(numpy.float64)) for n in ROWS}


def _build_quads(lib, st, n_rows, n_haps, qrec_bytes, what):
    out = {"qrec": guarded(qrec_bytes, 32, DEV), "qoff": guarded(8 * n_rows, 8, DEV), "nquad": guarded(4 * n_rows, 4, DEV),
           "qstats": guarded(16, 8, DEV)}
    assert lib.mxm_build_quads(ctypes.byref(st), n_haps, out["qrec"].ptr, qrec_bytes, out["qoff"].ptr, out["nquad"].ptr,
                               out["qstats"].ptr, _stream()) == 0, lib.mxm_last_error()
    _sync()
    _check_coded(out, what)
    return out, [int(v) for v in out["qstats"].get(numpy.uint64)], out["nquad"].get(numpy.int32)


def _with_quads(lib, mat, wts, what):
    """Records + a quad dictionary in exactly mxm_quad_bytes + the two row lists from mxm_quad_lists, all guarded."""
    n_rows, n_haps = mat.shape
    st, bufs, ndist, rest = _coded(lib, mat, wts, what)
    assert len(rest) == 0
    quads, (used, n_left), nquad = _build_quads(lib, st, n_rows, n_haps, lib.mxm_quad_bytes(n_rows, n_haps), what)
    assert used <= quads["qrec"].nbytes and ((nquad >= 0) & (nquad <= 256)).all() and (nquad[ndist > ENC_MAX_CODES] == 0).all(), what
    assert n_left == int(((ndist > 0) & (ndist <= ENC_MAX_CODES) & (nquad == 0)).sum()), what
    s_bytes = lib.mxm_quad_lists_scratch_bytes(n_rows)
    lists = {"quad_rows": guarded(8 * n_rows, 8, DEV), "byte_rows": guarded(8 * n_rows, 8, DEV), "counts": guarded(16, 8, DEV),
             "scratch": guarded(s_bytes, 8, DEV)}
    assert lib.mxm_quad_lists(bufs["ndist"].ptr, quads["nquad"].ptr, n_rows, lists["quad_rows"].ptr, lists["byte_rows"].ptr,
                              lists["counts"].ptr, lists["scratch"].ptr, s_bytes, _stream()) == 0, lib.mxm_last_error()
    _sync()
    _check_coded(bufs, what)
    _check_coded(quads, what)
    _check_coded(lists, what)
    want_q = numpy.flatnonzero(nquad > 0)
    want_b = numpy.flatnonzero((ndist > 0) & (ndist <= ENC_MAX_CODES) & (nquad == 0))
    assert [int(v) for v in lists["counts"].get(numpy.int64)] == [len(want_q), len(want_b)], what
    for name, want in (("quad_rows", want_q), ("byte_rows", want_b)):
        got = lists[name].get(numpy.int64)
        assert numpy.array_equal(got[:len(want)], want), (what, name)
        assert (got[len(want):] == -1).all(), "%s past its count was written (%s)" % (name, what)
    bufs.update(quads)
    # the struct takes lists of exactly their counts
    for name, want in (("quad_rows", want_q), ("byte_rows", want_b)):
        if len(want):
            bufs[name] = guarded_from(want, numpy.int64, 8, DEV)
    st.qrec, st.qoff, st.nquad = quads["qrec"].ptr, quads["qoff"].ptr, quads["nquad"].ptr
    st.quad_rows, st.n_quad_rows = (bufs["quad_rows"].ptr if len(want_q) else None), len(want_q)
    st.byte_rows, st.n_byte_rows = (bufs["byte_rows"].ptr if len(want_b) else None), len(want_b)
    return st, bufs, ndist, nquad, used


def test_build_quads_inside_exactly_quad_bytes_and_two_pieces(lib, quad_case):
    """mixemt_hip.h: "mxm_quad_bytes: a buffer size that can never overflow"; "stats[0] = bytes reserved (a record that no
    longer fits is not written and its row keeps nquad = 0 ...)"; mxm_quad_lists: "quad_rows[R] / byte_rows[R] (room for
    every row), counts[2] ...; scratch of mxm_quad_lists_scratch_bytes(R) bytes" -- the lists past their counts are left
    alone."""
    n_haps, mats = quad_case
    some = 0
    for n_rows in ROWS:
        mat, wts = mats[n_rows]
        what = "R=%d H=%d" % (n_rows, n_haps)
        st, bufs, ndist, nquad, used = _with_quads(lib, mat, wts, what)
        some += int((nquad > 0).sum())
        small_bytes = 2 * QUAD_CHUNK
        st0, bufs0, _, _ = _coded(lib, mat, wts, what)
        small, (used_s, _), nquad_s = _build_quads(lib, st0, n_rows, n_haps, small_bytes, what + " qrec_bytes=%d" % small_bytes)
        _check_coded(bufs0, what)
        lost = (nquad_s == 0) & (nquad > 0)
        assert numpy.array_equal(nquad_s[~lost], nquad[~lost]), what
        # the encoders reserve whole pieces whether or not they fit, the same number on every run: stats[0] of the short
        # run is what the full run used, "the size that suffices"
        assert used_s == used, what
        assert lost.any() == (used > small_bytes), what
        if n_rows == 700:
            assert lost.any() and used_s > small_bytes, what           # two pieces hold a dozen records, not hundreds
        qoff = small["qoff"].get(numpy.int64)
        kept = numpy.flatnonzero(nquad_s > 0)
        assert ((qoff[kept] >= 0) & (qoff[kept] + 2048 + 32 * nquad_s[kept] <= small_bytes)).all(), what
    assert some > 0


@pytest.mark.parametrize("tile,left_grid", [(3, 0), (1, 1), (3, 2 ** 31 - 1)])
@pytest.mark.parametrize("n_runs", [1, 4, 9])
def test_em_iter_coded_beside_a_quad_dictionary(lib, quad_case, n_runs, tile, left_grid):
    """mxm_em_iter_coded over quad records, byte-coded leftovers and wide rows, full tiles of three restarts and single
    ones, at both ends of mxm_set_coded_batch_tile and mxm_set_quad_left_grid; ws exactly mxm_workspace_bytes(R, H, B)."""
    assert lib.mxm_set_coded_batch_tile(tile) == 0 and lib.mxm_set_quad_left_grid(left_grid) == 0
    n_haps, mats = quad_case
    rng = numpy.random.default_rng(n_haps + n_runs)
    for n_rows in ROWS:
        mat, wts = mats[n_rows]
        what = "R=%d H=%d B=%d tile=%d left=%d" % (n_rows, n_haps, n_runs, tile, left_grid)
        st, bufs, _, _, _ = _with_quads(lib, mat, wts, what)
        props = rng.dirichlet([1.0] * n_haps, size=n_runs)
        done = (1,) if n_runs > 1 else ()
        raw = numpy.zeros(n_runs * 6, dtype=numpy.int32)
        raw[[6 * b for b in done]] = 1
        ws_bytes = lib.mxm_workspace_bytes(n_rows, n_haps, n_runs)
        run = {"w": guarded_from(wts, numpy.float64, 8, DEV), "props": guarded_from(props, numpy.float64, 8, DEV),
               "state": guarded_from(raw, numpy.int32, 8, DEV), "colsum": guarded(8 * n_runs * n_haps, 8, DEV),
               "ws": guarded(ws_bytes, 8, DEV, row_bytes=8 * (n_haps + 8))}
        assert lib.mxm_em_iter_coded(ctypes.byref(st), run["w"].ptr, run["props"].ptr, n_haps, n_runs, run["state"].ptr,
                                     run["colsum"].ptr, run["ws"].ptr, ws_bytes, _stream()) == 0, lib.mxm_last_error()
        _sync()
        _check_coded(bufs, what)
        _check_coded(run, what)
        assert numpy.array_equal(run["state"].get(numpy.int32), raw), what
        got = run["colsum"].get(numpy.float64, (n_runs, n_haps))
        for b in range(n_runs):
            if b in done:
                assert (got[b].view(numpy.uint8) == 0xFF).all(), "colsum row of finished restart %d was written (%s)" % (b, what)
                continue
            _, new = em_oracle.em_step(mat, wts, numpy.log(props[b]), numpy.empty_like(mat))
            assert numpy.abs(got[b] * props[b] - numpy.exp(new) * wts.sum()).max() <= 1e-12 * wts.sum(), (what, b)


@pytest.mark.parametrize("grid", [0, 1, 2 ** 31 - 1])
@pytest.mark.parametrize("n_runs,quads", [(1, False), (1, True), (4, True), (4, False)])
def test_em_loop_coded(lib, quad_case, n_runs, quads, grid):
    """mxm_em_loop_coded, three iterations with tolerance 0, over records alone (the one-launch loop at these sizes, at both
    ends of mxm_set_fused_coded_grid) and beside a quad dictionary; restart 1 of several arrives finished and is left
    alone.  The oracle's third step at the bound of the one-launch loops' tests (1e-9)."""
    from mixemt_amd import _lib
    assert lib.mxm_set_fused_coded_grid(grid) == 0
    n_haps, mats = quad_case
    rng = numpy.random.default_rng(n_haps + n_runs + 5)
    for n_rows in ROWS[1:]:
        mat, wts = mats[n_rows]
        what = "R=%d H=%d B=%d quads=%s grid=%d" % (n_rows, n_haps, n_runs, quads, grid)
        if quads:
            st, bufs, _, _, _ = _with_quads(lib, mat, wts, what)
        else:
            st, bufs, _, _ = _coded(lib, mat, wts, what)
        ln0 = numpy.log(rng.dirichlet([1.0] * n_haps, size=n_runs))
        done = (1,) if n_runs > 1 else ()
        raw = numpy.zeros(n_runs * 6, dtype=numpy.int32)
        raw[[6 * b for b in done]] = 1
        ws_bytes = lib.mxm_workspace_bytes(n_rows, n_haps, n_runs)
        run = {"w": guarded_from(wts, numpy.float64, 8, DEV), "props_cur": guarded_from(numpy.exp(ln0), numpy.float64, 8, DEV),
               "ln_cur": guarded_from(ln0, numpy.float64, 8, DEV), "ln_new": guarded_from(ln0, numpy.float64, 8, DEV),
               "colsum": guarded(8 * n_runs * n_haps, 8, DEV), "state": guarded_from(raw, numpy.int32, 8, DEV),
               "ws": guarded(ws_bytes, 8, DEV, row_bytes=8 * (n_haps + 8))}
        host = (_lib.EmState * n_runs)()
        assert lib.mxm_em_loop_coded(ctypes.byref(st), run["w"].ptr, n_haps, n_runs, run["props_cur"].ptr, run["ln_cur"].ptr,
                                     run["ln_new"].ptr, run["colsum"].ptr, run["state"].ptr, 0.0, 3, 2, run["ws"].ptr, ws_bytes,
                                     _stream(), host) == 0, lib.mxm_last_error()
        _sync()
        _check_coded(bufs, what)
        _check_coded(run, what)
        got_new = run["ln_new"].get(numpy.float64, ln0.shape)
        got_sum = run["colsum"].get(numpy.float64, ln0.shape)
        for b in range(n_runs):
            if b in done:
                assert (host[b].done, host[b].iters) == (1, 0) and numpy.array_equal(got_new[b], ln0[b]), (what, b)
                assert (got_sum[b].view(numpy.uint8) == 0xFF).all(), "colsum row of finished restart %d was written (%s)" % (b, what)
                continue
            assert (host[b].done, host[b].iters, host[b].error) == (2, 3, 0), (what, b)
            theta = ln0[b]
            for _ in range(3):
                _, theta = em_oracle.em_step(mat, wts, theta, numpy.empty_like(mat))
            assert numpy.abs(numpy.exp(got_new[b]) - numpy.exp(theta)).max() < 1e-9, (what, b)
