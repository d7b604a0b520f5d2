"""
The consumers and the small auxiliary kernels of include/mixemt_hip.h called through ctypes with every device pointer
guard-banded at its exact documented size (tests/_guarded.py): mxm_row_argmax_votes, mxm_first_seen, mxm_assign_reads,
mxm_gather_columns, mxm_fold_logaddexp, mxm_log_normalize, mxm_l1_exp_diff, mxm_add_scalar.  References: numpy.
Each matrix comes once at the doubles' own alignment with an odd stride and once at 16 bytes with an even one (the
vectorised forms).
"""
import ctypes

import numpy
import pytest

from _guarded_abi import load_lib, stream as _stream, sync as _sync
from _guarded import guarded, guarded_2d, guarded_from

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 257, 700)
WIDTHS = (66, 1026, 5408, 8192, 1, 3, 65, 8193)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _ld(width, align):
    """A stride larger than the width: odd excess at 8 bytes, the next even stride but one at 16."""
    return width + 3 if align == 8 else width + 2 + (width & 1)


@pytest.mark.parametrize("align", [8, 16])
@pytest.mark.parametrize("n_haps", WIDTHS)
def test_row_argmax_votes(lib, n_haps, align):
    """mixemt_hip.h: "best[r] = first index of max_h X[r][h]; votes[h] = sum_{r: best[r]==h} w[r]; votes[H] is overwritten
    (NULL = not wanted); w NULL = 1 ... ws / ws_bytes as for mxm_em_iter (mxm_workspace_bytes(R, H, 1)), only needed when
    votes != NULL" -- ties, NaNs, rows of -inf and a winner in the last column, the pad columns of X being NaN."""
    rng = numpy.random.default_rng(100 + n_haps + align)
    ldx = _ld(n_haps, align)
    for n_rows in ROWS:
        mat = rng.normal(-20.0, 5.0, size=(n_rows, n_haps))
        if n_haps > 1:
            for r in range(0, n_rows, 3):
                a, b = sorted(rng.choice(n_haps, size=2, replace=False))
                mat[r, a] = mat[r, b] = mat[r].max() + 1.0
            for r in range(1, n_rows, 7):
                mat[r, rng.choice(n_haps, size=2, replace=False)] = numpy.nan
        if n_rows > 5:
            mat[5, :] = -numpy.inf
        mat[0, n_haps - 1] = 1e9
        wts = rng.integers(1, 5, size=n_rows).astype(numpy.float64) + 0.25
        want = numpy.argmax(mat, axis=1)
        x_buf = guarded_2d(n_rows, n_haps, ldx, numpy.float64, align, DEV).put(mat)
        w_buf = guarded_from(wts, numpy.float64, 8, DEV)
        ws_bytes = lib.mxm_workspace_bytes(n_rows, n_haps, 1)
        ws = guarded(ws_bytes, 8, DEV, row_bytes=8 * (n_haps + 8))
        for weighted, with_votes in ((True, True), (False, True), (True, False)):
            best = guarded(4 * n_rows, 4, DEV)
            votes = guarded(8 * n_haps, 8, DEV)
            rc = lib.mxm_row_argmax_votes(x_buf.ptr, ldx, w_buf.ptr if weighted else None, n_rows, n_haps, best.ptr,
                                          votes.ptr if with_votes else None, ws.ptr if with_votes else None,
                                          ws_bytes if with_votes else 0, _stream())
            assert rc == 0, lib.mxm_last_error()
            _sync()
            what = "R=%d H=%d align=%d w=%s votes=%s" % (n_rows, n_haps, align, weighted, with_votes)
            x_buf.check("X " + what, pads="unchanged")
            for name, buf in (("w", w_buf), ("best", best), ("votes", votes), ("ws", ws)):
                buf.check(name + " " + what)
            assert numpy.array_equal(best.get(numpy.int32), want), what
            if with_votes:
                want_votes = numpy.zeros(n_haps)
                numpy.add.at(want_votes, want, wts if weighted else 1.0)
                assert numpy.array_equal(votes.get(numpy.float64), want_votes), what      # quarters: exact in any order
            else:
                assert (votes.get(numpy.uint8) == 0xFF).all(), what


@pytest.mark.parametrize("n_haps", WIDTHS + (20001,))
def test_first_seen(lib, n_haps):
    """mixemt_hip.h: "first[h] = the smallest r with best[r] == h, R if no row voted for h (device int64[H]) ... Entries of
    best outside [0, H) are ignored"."""
    rng = numpy.random.default_rng(200 + n_haps)
    for n_rows in ROWS + (3000,):
        best = rng.integers(0, min(n_haps, 40), size=n_rows).astype(numpy.int32) * max(1, n_haps // 40)
        best[rng.random(n_rows) < 0.1] = -1
        best[rng.random(n_rows) < 0.1] = n_haps
        best[n_rows // 2] = n_haps - 1
        want = numpy.full(n_haps, n_rows, dtype=numpy.int64)
        for r in range(n_rows - 1, -1, -1):
            if 0 <= best[r] < n_haps:
                want[best[r]] = r
        b_buf = guarded_from(best, numpy.int32, 4, DEV)
        first = guarded(8 * n_haps, 8, DEV)
        assert lib.mxm_first_seen(b_buf.ptr, n_rows, n_haps, first.ptr, _stream()) == 0, lib.mxm_last_error()
        _sync()
        b_buf.check("best R=%d H=%d" % (n_rows, n_haps))
        first.check("first R=%d H=%d" % (n_rows, n_haps))
        assert numpy.array_equal(first.get(numpy.int64), want), (n_rows, n_haps)


@pytest.mark.parametrize("n_haps,n_cols", [(66, 2), (1026, 3), (5408, 7), (8193, 16), (3, 2), (65, 5)])
def test_assign_reads(lib, n_haps, n_cols):
    """mixemt_hip.h: "v_c = X[r][c] - log_props[c] for the nC contributor columns cols[]; assigned[r] = ordinal (0..nC-1) of
    the largest v_c if it beats the runner-up by at least log_min_fold, else -1"; among equal values the larger column
    wins (numpy.argsort(...)[::-1], assemble.py:267-281)."""
    rng = numpy.random.default_rng(300 + n_haps)
    ldx = n_haps + 3
    fold = numpy.log(2.0)
    for n_rows in ROWS:
        mat = numpy.round(rng.normal(-10.0, 2.0, size=(n_rows, n_haps)), 1)
        cols = numpy.sort(rng.choice(n_haps, size=n_cols, replace=False)).astype(numpy.int32)
        cols[-1] = n_haps - 1                                  # the last column of a row, the last row's included
        cols = numpy.unique(cols).astype(numpy.int32)
        log_props = numpy.full(n_haps, numpy.nan)              # a column that is no contributor's is never looked at
        log_props[cols] = numpy.round(numpy.log(rng.dirichlet([1.0] * len(cols))), 1)
        val = mat[:, cols] - log_props[cols][None, :]
        want = numpy.empty(n_rows, dtype=numpy.int32)
        for r in range(n_rows):
            order = sorted(range(len(cols)), key=lambda i: (val[r, i], cols[i]), reverse=True)
            want[r] = order[0] if len(cols) >= 2 and val[r, order[0]] - val[r, order[1]] >= fold else -1
        x_buf = guarded_2d(n_rows, n_haps, ldx, numpy.float64, 8, DEV).put(mat)
        lp_buf = guarded_from(log_props, numpy.float64, 8, DEV)
        c_buf = guarded_from(cols, numpy.int32, 4, DEV)
        out = guarded(4 * n_rows, 4, DEV)
        assert lib.mxm_assign_reads(x_buf.ptr, ldx, lp_buf.ptr, c_buf.ptr, len(cols), n_rows, n_haps, fold, out.ptr,
                                    _stream()) == 0, lib.mxm_last_error()
        _sync()
        what = "R=%d H=%d nC=%d" % (n_rows, n_haps, len(cols))
        x_buf.check("X " + what, pads="unchanged")
        for name, buf in (("log_props", lp_buf), ("cols", c_buf), ("assigned", out)):
            buf.check(name + " " + what)
        assert numpy.array_equal(out.get(numpy.int32), want), what
        assert n_rows < 100 or ((want >= 0).any() and (want < 0).any()), what       # both outcomes are in the case


@pytest.mark.parametrize("n_haps,n_cols,ldo", [(66, 1, 4), (1026, 3, 4), (5408, 7, 8), (8193, 16, 19), (3, 3, 3), (65, 64, 67),
                                               (1, 1, 2), (8192, 100, 101)])
def test_gather_columns(lib, n_haps, n_cols, ldo):
    """mixemt_hip.h: "out[r][i] = M[r][cols[i]], i < nC; cols[] device int32, each in [0, H)"; columns [nC, ldo) of out are
    left alone."""
    rng = numpy.random.default_rng(400 + n_haps)
    ldm = n_haps + 3
    for n_rows in ROWS:
        mat = rng.normal(size=(n_rows, n_haps))
        cols = rng.integers(0, n_haps, size=n_cols).astype(numpy.int32)       # any order, repeats allowed
        cols[0] = n_haps - 1
        m_buf = guarded_2d(n_rows, n_haps, ldm, numpy.float64, 8, DEV).put(mat)
        c_buf = guarded_from(cols, numpy.int32, 4, DEV)
        out = guarded_2d(n_rows, n_cols, ldo, numpy.float64, 8, DEV)
        assert lib.mxm_gather_columns(m_buf.ptr, ldm, n_rows, n_haps, c_buf.ptr, n_cols, out.ptr, ldo, _stream()) == 0, \
            lib.mxm_last_error()
        _sync()
        what = "R=%d H=%d nC=%d" % (n_rows, n_haps, n_cols)
        m_buf.check("M " + what, pads="unchanged")
        c_buf.check("cols " + what)
        out.check("out " + what, pads="unchanged")
        assert numpy.array_equal(out.get(), mat[:, cols]), what


@pytest.mark.parametrize("align", [8, 16])
@pytest.mark.parametrize("n_haps,n_in", [(66, 1), (1026, 8), (5408, 2), (8192, 3), (1, 2), (3, 8), (65, 0), (8193, 1)])
def test_fold_logaddexp(lib, n_haps, n_in, align):
    """mixemt_hip.h: "acc[r][h] = logaddexp(... logaddexp(logaddexp(acc, in[0]), in[1]) ..., in[n_in-1]) + delta in that
    fixed order"; the pad columns of acc are left alone, those of the inputs never read."""
    rng = numpy.random.default_rng(500 + n_haps + align)
    lda = _ld(n_haps, align)
    delta = -numpy.log(3.0)
    for n_rows in ROWS:
        acc = rng.normal(-30.0, 10.0, size=(n_rows, n_haps))
        acc[rng.random(acc.shape) < 0.01] = -numpy.inf
        blocks = [rng.normal(-30.0, 10.0, size=(n_rows, n_haps)) - 700.0 * (k == 1) for k in range(n_in)]
        lds = [_ld(n_haps, align) + 2 * k for k in range(n_in)]
        a_buf = guarded_2d(n_rows, n_haps, lda, numpy.float64, align, DEV).put(acc)
        in_bufs = [guarded_2d(n_rows, n_haps, lds[k], numpy.float64, align, DEV).put(blocks[k]) for k in range(n_in)]
        ptrs = (ctypes.c_void_p * max(n_in, 1))(*[b.ptr for b in in_bufs])
        ld_in = (ctypes.c_int64 * max(n_in, 1))(*lds)
        assert lib.mxm_fold_logaddexp(a_buf.ptr, lda, ptrs, ld_in, n_in, n_rows, n_haps, delta, _stream()) == 0, \
            lib.mxm_last_error()
        _sync()
        what = "R=%d H=%d n_in=%d align=%d" % (n_rows, n_haps, n_in, align)
        a_buf.check("acc " + what, pads="unchanged")
        for k, buf in enumerate(in_bufs):
            buf.check("in[%d] %s" % (k, what), pads="unchanged")
        want = acc
        for blk in blocks:
            want = numpy.logaddexp(want, blk)
        want = want + delta
        got = a_buf.get()
        fin = numpy.isfinite(want)
        assert numpy.array_equal(numpy.isfinite(got), fin), what
        assert numpy.allclose(got[fin], want[fin], rtol=0, atol=1e-10), what           # the bound of the posterior fold's test


@pytest.mark.parametrize("n_haps", WIDTHS)
def test_log_normalize_and_l1_exp_diff(lib, n_haps):
    """mixemt_hip.h: "ln_new[h] = log(colsum[h]) - log(sum_h colsum[h])" and "l1_out[0] = sum_h |exp(a[h]) - exp(b[h])|":
    vectors of exactly H doubles, one double out."""
    rng = numpy.random.default_rng(600 + n_haps)
    sums = rng.random(n_haps) * 50.0 + 1e-6
    if n_haps > 2:
        sums[1] = 0.0                                                  # log(0) = -inf, as the reference's
    s_buf = guarded_from(sums, numpy.float64, 8, DEV)
    out = guarded(8 * n_haps, 8, DEV)
    assert lib.mxm_log_normalize(s_buf.ptr, n_haps, out.ptr, _stream()) == 0, lib.mxm_last_error()
    _sync()
    s_buf.check("colsum H=%d" % n_haps)
    out.check("ln_new H=%d" % n_haps)
    with numpy.errstate(divide="ignore"):
        want = numpy.log(sums) - numpy.log(sums.sum())
    got = out.get(numpy.float64)
    fin = numpy.isfinite(want)
    assert numpy.array_equal(numpy.isfinite(got), fin) and numpy.array_equal(got[~fin], want[~fin])
    # a sum of H <= 8193 positive terms in any order is good to (H - 1) * 2^-53 = 9.1e-13 relative, which is the absolute
    # error of its log; the two logs add a few ulp of values below 20 in magnitude
    assert numpy.allclose(got[fin], want[fin], rtol=0, atol=1e-12)
    a = numpy.log(rng.dirichlet([1.0] * n_haps))
    b = numpy.log(rng.dirichlet([1.0] * n_haps))
    a_buf, b_buf = guarded_from(a, numpy.float64, 8, DEV), guarded_from(b, numpy.float64, 8, DEV)
    l1 = guarded(8, 8, DEV)
    assert lib.mxm_l1_exp_diff(a_buf.ptr, b_buf.ptr, n_haps, l1.ptr, _stream()) == 0, lib.mxm_last_error()
    _sync()
    for name, buf in (("a", a_buf), ("b", b_buf), ("l1_out", l1)):
        buf.check("%s H=%d" % (name, n_haps))
    # proportions sum to 1 on either side: the result is at most 2, and a sum of H <= 8193 such terms in any order is good
    # to (H - 1) * 2^-53 * 2 = 1.8e-12
    assert abs(l1.get(numpy.float64)[0] - numpy.abs(numpy.exp(a) - numpy.exp(b)).sum()) <= 2e-12


@pytest.mark.parametrize("align", [8, 16])
@pytest.mark.parametrize("n_haps", WIDTHS)
def test_add_scalar_leaves_the_pad_columns_alone(lib, n_haps, align):
    """mixemt_hip.h: "x[i] += delta over an [R][ld] matrix's first H columns" -- the pad columns are unchanged."""
    rng = numpy.random.default_rng(700 + n_haps + align)
    ld = _ld(n_haps, align)
    delta = -numpy.log(7.0)
    for n_rows in ROWS:
        mat = rng.normal(-30.0, 10.0, size=(n_rows, n_haps))
        mat[rng.random(mat.shape) < 0.01] = -numpy.inf
        x_buf = guarded_2d(n_rows, n_haps, ld, numpy.float64, align, DEV).put(mat)
        assert lib.mxm_add_scalar(x_buf.ptr, ld, n_rows, n_haps, delta, _stream()) == 0, lib.mxm_last_error()
        _sync()
        x_buf.check("x R=%d H=%d align=%d" % (n_rows, n_haps, align), pads="unchanged")
        assert numpy.array_equal(x_buf.get(), mat + delta), (n_rows, n_haps, align)
