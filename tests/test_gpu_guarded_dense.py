"""
The dense EM entries of include/mixemt_hip.h called through ctypes with EVERY device pointer guard-banded at its exact
documented size (tests/_guarded.py): mxm_linearize(_f32), mxm_em_iter(_f32), mxm_em_step, mxm_m_finalize,
mxm_em_loop(_f32).  After each call and a synchronise (a) every guard, every "left alone" region and every "written as 0"
pad is as the header says, and (b) the values equal the oracle's at the tolerance the entry's existing test uses -- an
over-READ shows only there (the guards and an input's pad columns read as NaN).

Alignment: doubles are promised 8 bytes, so every buffer starts at an odd multiple of 8; the kernels that want 16-byte rows
(the "wide" forms) are reached by the same tests at an odd multiple of 16 with an even stride.
"""
import ctypes

import numpy
import pytest

from _guarded_abi import load_lib, stream as _stream, sync as _sync
from _guarded import guarded, guarded_2d, guarded_from
from oracle import em_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 257, 700)
H_LINEAR = (66, 1026, 5408, 8192)          # H % 4 == 2, the chunk-count edges, the streaming kernel's cap
H_ANY = (1, 3, 65, 8193)                   # the widths only the any-width kernels take
INT32_MAX = 2 ** 31 - 1
SENTINEL = 0xFF                            # an untouched double reads as NaN


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _matrix(rng, n_rows, n_haps):
    """Log likelihoods with a few -inf cells (wide matrices only) and a finite cell in every row."""
    mat = rng.normal(-20.0, 6.0, size=(n_rows, n_haps))
    if n_haps >= 66:
        mat[rng.random(mat.shape) < 0.002] = -numpy.inf
        mat[:, n_haps // 2] = -3.0
    return mat


def _strides(n_haps, align):
    """(ldm, ldp, ldo): strides larger than the width by an amount that is no multiple of the vector width (2 doubles) where
    the header allows an odd stride; the 16-byte variant uses even strides, which is what the wide kernels ask for."""
    even = n_haps + 2 + (n_haps & 1)
    if align == 16:
        return even, even, even
    return n_haps + 3, even, n_haps + 3


def _linear(mat):
    rowmax = mat.max(axis=1)
    rowmax = numpy.where(numpy.isfinite(rowmax), rowmax, 0.0)
    with numpy.errstate(under="ignore"):
        return numpy.exp(mat - rowmax[:, None]), rowmax


def _states(n_runs, done=()):
    """mxm_em_state[n_runs] (24 bytes each, 8-byte aligned), zeroed, with .done = 1 for the restarts in `done`."""
    raw = numpy.zeros(n_runs * 6, dtype=numpy.int32)
    for b in done:
        raw[6 * b] = 1
    return guarded_from(raw, numpy.int32, 8, DEV)


def _read_states(buf, n_runs):
    from mixemt_amd import _lib
    raw = buf.get(numpy.uint8).tobytes()
    return list((_lib.EmState * n_runs).from_buffer_copy(raw))


def _workspace(lib, n_rows, n_haps, n_runs):
    nbytes = lib.mxm_workspace_bytes(n_rows, n_haps, n_runs)
    return guarded(nbytes, 8, DEV, row_bytes=8 * (n_haps + 8)), nbytes


def _oracle_step(mat, wts, ln_props):
    with numpy.errstate(divide="ignore", invalid="ignore", under="ignore"):
        return em_oracle.em_step(mat, wts, ln_props, numpy.empty_like(mat))


def _is_sentinel(row):
    return bool((row.view(numpy.uint8) == SENTINEL).all())


# ---- mxm_linearize / mxm_linearize_f32 ------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [8, 16])
@pytest.mark.parametrize("n_haps", H_LINEAR + H_ANY)
def test_linearize_writes_its_rows_zeroes_its_pads_and_nothing_else(lib, n_haps, align):
    """mixemt_hip.h: "rowmax[r] = max_h M[r][h] (0 if not finite), P[r][h] = exp(M[r][h] - rowmax[r]); ldp must be even and
    >= H; pad columns [H, ldp) are written as 0" -- and the fp32-storage twin: "ldp (floats) a multiple of 4, pad columns 0"."""
    rng = numpy.random.default_rng(1000 + n_haps)
    ldm, ldp, _ = _strides(n_haps, align)
    ldp32 = (n_haps + 3) // 4 * 4 + 4
    for n_rows in ROWS:
        mat = _matrix(rng, n_rows, n_haps)
        if n_rows > 1:
            mat[n_rows // 2, :] = -numpy.inf                       # "0 if not finite"
        want, want_max = _linear(mat)
        src = guarded_2d(n_rows, n_haps, ldm, numpy.float64, align, DEV).put(mat)
        for dtype, ld in ((numpy.float64, ldp), (numpy.float32, ldp32)):
            lin = guarded_2d(n_rows, n_haps, ld, dtype, align if dtype is numpy.float64 else align // 2, DEV)
            rowmax = guarded(8 * n_rows, 8, DEV)
            entry = lib.mxm_linearize if dtype is numpy.float64 else lib.mxm_linearize_f32
            assert entry(src.ptr, ldm, n_rows, n_haps, lin.ptr, ld, rowmax.ptr, _stream()) == 0, lib.mxm_last_error()
            _sync()
            what = "%s R=%d H=%d" % (dtype.__name__, n_rows, n_haps)
            src.check("M " + what, pads="unchanged")
            lin.check("P " + what, pads="zero")
            rowmax.check("rowmax " + what)
            assert numpy.array_equal(rowmax.get(numpy.float64), want_max), what
            got = lin.get()
            if dtype is numpy.float64:
                assert numpy.allclose(got, want, rtol=1e-15, atol=0), what
            else:
                # an fp64 exp rounded to the nearest float: half a float ulp (2^-24 relative, 2^-150 absolute) on top of
                # the fp64 result's last bits, which can move the rounding by one more ulp at most
                with numpy.errstate(under="ignore", over="ignore"):
                    assert numpy.allclose(got, want.astype(numpy.float32), rtol=1.2e-7, atol=1.5e-45), what


# ---- mxm_em_iter: the streaming kernel ---------------------------------------------------------------------------------
def _check_em_iter(lib, rng, n_rows, n_haps, n_runs, align, storage="f64", linear=True, null_weights=False):
    ldm, ldp, _ = _strides(n_haps, align)
    mat = _matrix(rng, n_rows, n_haps)
    wts = rng.integers(1, 4, size=n_rows).astype(numpy.float64)
    if null_weights:
        wts[:] = 1.0
    props = rng.dirichlet([1.0] * n_haps, size=n_runs)
    done = (1,) if n_runs > 1 else ()
    lin, _ = _linear(mat)
    if storage == "f32":
        ldp = (n_haps + 3) // 4 * 4 + 4
        lin = lin.astype(numpy.float32)
    # P is mxm_linearize's output: its pad columns are DEFINED as 0 (an odd H reads the one beside its last column)
    p_buf = guarded_2d(n_rows, n_haps, ldp, lin.dtype, align if storage == "f64" else align // 2, DEV, pad=0).put(lin) \
        if linear else None
    m_buf = guarded_2d(n_rows, n_haps, ldm, numpy.float64, align, DEV).put(mat) if not linear else None
    w_buf = None if null_weights else guarded_from(wts, numpy.float64, 8, DEV)
    props_buf = guarded_from(props, numpy.float64, 8, DEV)
    with numpy.errstate(divide="ignore"):
        ln_buf = guarded_from(numpy.log(props), numpy.float64, 8, DEV)
    state = _states(n_runs, done)
    colsum = guarded(8 * n_runs * n_haps, 8, DEV)
    ws, ws_bytes = _workspace(lib, n_rows, n_haps, n_runs)
    w_ptr = None if w_buf is None else w_buf.ptr
    if storage == "f32":
        rc = lib.mxm_em_iter_f32(p_buf.ptr, ldp, w_ptr, props_buf.ptr, n_rows, n_haps, n_runs, state.ptr, colsum.ptr,
                                 ws.ptr, ws_bytes, _stream())
    else:
        rc = lib.mxm_em_iter(m_buf.ptr if m_buf else None, ldm if m_buf else 0, p_buf.ptr if p_buf else None,
                             ldp if p_buf else 0, w_ptr, props_buf.ptr, ln_buf.ptr, n_rows, n_haps, n_runs, state.ptr,
                             colsum.ptr, ws.ptr, ws_bytes, _stream())
    assert rc == 0, lib.mxm_last_error()
    _sync()
    what = "R=%d H=%d B=%d %s" % (n_rows, n_haps, n_runs, storage)
    for name, buf in (("P", p_buf), ("M", m_buf)):
        if buf is not None:
            buf.check(name + " " + what, pads="unchanged")
    for name, buf in (("w", w_buf), ("props", props_buf), ("ln_props", ln_buf), ("state", state), ("colsum", colsum),
                      ("ws", ws)):
        if buf is not None:
            buf.check(name + " " + what)
    assert [(s.done, s.iters, s.ticket, s.error) for s in _read_states(state, n_runs)] == \
        [(1 if b in done else 0, 0, 0, 0) for b in range(n_runs)], what          # const state: read, never written
    got = colsum.get(numpy.float64, (n_runs, n_haps))
    for b in range(n_runs):
        if b in done:
            assert _is_sentinel(got[b]), "colsum row of finished restart %d was written (%s)" % (b, what)
            continue
        if storage == "f32":
            # the same operation in fp64 over the float-rounded matrix the kernel streams
            lin64 = lin.astype(numpy.float64)
            want = ((wts / (lin64 @ props[b])) @ lin64) * props[b]
        else:
            _, new = _oracle_step(mat, wts, numpy.log(props[b]))
            want = numpy.exp(new) * wts.sum()
        assert numpy.abs(got[b] * props[b] - want).max() <= 1e-12 * wts.sum(), (what, b)


@pytest.mark.parametrize("n_runs", [1, 4, 5, 9])
@pytest.mark.parametrize("n_haps", H_LINEAR + (65,))
def test_em_iter_streaming_kernel(lib, n_haps, n_runs):
    """mixemt_hip.h: "colsum[b][h] = T_bh ...; restarts with state[b].done != 0 are skipped (their colsum is left
    untouched)"; ws is exactly mxm_workspace_bytes(R, H, B)."""
    rng = numpy.random.default_rng(2000 + 10 * n_haps + n_runs)
    for n_rows in ROWS:
        _check_em_iter(lib, rng, n_rows, n_haps, n_runs, 8 if n_rows != 257 else 16, null_weights=(n_rows == 1))


@pytest.mark.parametrize("tile,rows_per_wg", [(1, 1), (4, INT32_MAX), (1, INT32_MAX), (4, 1)])
@pytest.mark.parametrize("n_haps", [66, 8192])
def test_em_iter_workspace_at_the_ends_of_its_grid_setters(lib, n_haps, tile, rows_per_wg):
    """The workspace is sized by MXM_MAX_WG while the grid comes from the device and mxm_set_min_rows_per_wg /
    mxm_set_batch_tile: at the smallest and the largest value each setter accepts the partial rows stay inside it."""
    assert lib.mxm_set_batch_tile(tile) == 0 and lib.mxm_set_min_rows_per_wg(rows_per_wg) == 0
    rng = numpy.random.default_rng(2500 + n_haps + tile)
    for n_rows in (257, 700):
        _check_em_iter(lib, rng, n_rows, n_haps, 9, 8)


@pytest.mark.parametrize("n_runs", [1, 4])
@pytest.mark.parametrize("n_haps", H_ANY + (64, 66))
def test_em_iter_log_space_kernels(lib, n_haps, n_runs):
    """P == NULL: "otherwise streams M in log space and reads ln_props" -- the one-thread-per-row, the LDS and (at 8193)
    the widest any-width forms, M with an odd stride."""
    rng = numpy.random.default_rng(3000 + 10 * n_haps + n_runs)
    for n_rows in ROWS:
        _check_em_iter(lib, rng, n_rows, n_haps, n_runs, 8, linear=False)


@pytest.mark.parametrize("n_runs", [1, 5])
@pytest.mark.parametrize("n_haps", H_LINEAR)
def test_em_iter_f32_storage(lib, n_haps, n_runs):
    """mxm_em_iter_f32: "P is kept as float ... every product, row sum and column sum stays fp64.  ldp (floats) a multiple
    of 4, pad columns 0"."""
    rng = numpy.random.default_rng(4000 + 10 * n_haps + n_runs)
    for n_rows in ROWS:
        _check_em_iter(lib, rng, n_rows, n_haps, n_runs, 8 if n_rows != 257 else 16, storage="f32")


# ---- mxm_em_step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [8, 16])
@pytest.mark.parametrize("n_haps", H_LINEAR + H_ANY + (64,))
def test_em_step_posterior_and_sums(lib, n_haps, align):
    """mixemt_hip.h: "out[r][h] = (ln_props[h] + M[r][h]) - logsumexp_h(ln_props + M[r]); mode 0: store; mode 1: out =
    logaddexp(out, value); colsum (nullable): also the M-step sums"; out's pad columns are left alone; ws is exactly
    mxm_workspace_bytes(R, H, 1)."""
    rng = numpy.random.default_rng(5000 + n_haps + align)
    ldm, _, ldo = _strides(n_haps, align)
    for n_rows in ROWS:
        mat = _matrix(rng, n_rows, n_haps)
        wts = rng.integers(1, 4, size=n_rows).astype(numpy.float64)
        with numpy.errstate(divide="ignore"):
            lnp = numpy.log(rng.dirichlet([0.5] * n_haps, size=2))
        mix = [_oracle_step(mat, wts, lnp[k]) for k in range(2)]
        m_buf = guarded_2d(n_rows, n_haps, ldm, numpy.float64, align, DEV).put(mat)
        w_buf = guarded_from(wts, numpy.float64, 8, DEV)
        out = guarded_2d(n_rows, n_haps, ldo, numpy.float64, align, DEV)
        ws, ws_bytes = _workspace(lib, n_rows, n_haps, 1)
        what = "R=%d H=%d align=%d" % (n_rows, n_haps, align)
        for mode in (0, 1):
            lnp_buf = guarded_from(lnp[mode], numpy.float64, 8, DEV)
            colsum = guarded(8 * n_haps, 8, DEV)
            assert lib.mxm_em_step(m_buf.ptr, ldm, w_buf.ptr, lnp_buf.ptr, n_rows, n_haps, out.ptr, ldo, mode,
                                   colsum.ptr, ws.ptr, ws_bytes, _stream()) == 0, lib.mxm_last_error()
            _sync()
            for name, buf in (("w", w_buf), ("ln_props", lnp_buf), ("colsum", colsum), ("ws", ws)):
                buf.check("%s %s mode %d" % (name, what, mode))
            m_buf.check("M " + what, pads="unchanged")
            out.check("out " + what, pads="unchanged")
            with numpy.errstate(invalid="ignore"):
                want = mix[0][0] if mode == 0 else numpy.logaddexp(mix[0][0], mix[1][0])
            got = out.get()
            fin = numpy.isfinite(want)
            assert numpy.array_equal(numpy.isfinite(got), fin), (what, mode)
            assert numpy.allclose(got[fin], want[fin], rtol=0, atol=1e-10), (what, mode)
            sums = colsum.get(numpy.float64)
            assert numpy.allclose(sums / sums.sum(), numpy.exp(mix[mode][1]), rtol=0, atol=1e-13), (what, mode)
        # without the sums no workspace is needed at all
        assert lib.mxm_em_step(m_buf.ptr, ldm, None, lnp_buf.ptr, n_rows, n_haps, out.ptr, ldo, 0, None, None, 0,
                               _stream()) == 0, lib.mxm_last_error()
        _sync()
        out.check("out " + what, pads="unchanged")
        m_buf.check("M " + what, pads="unchanged")
        got = out.get()
        assert numpy.allclose(got[fin := numpy.isfinite(mix[1][0])], mix[1][0][fin], rtol=0, atol=1e-10), what


# ---- mxm_m_finalize -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_runs", [1, 4, 5, 9])
@pytest.mark.parametrize("n_haps", (1, 3, 65, 66, 5408, 8192, 8193))
def test_m_finalize_vectors_and_states(lib, n_haps, n_runs):
    """mixemt_hip.h: "ln_new = ln_cur + log(colsum) - log(sum_h props_cur * colsum); l1 = sum_h |exp(ln_new) - props_cur|;
    iters += 1; l1 < tol -> done = 1; else iters >= max_iter -> done = 2; else ln_cur := ln_new, props_cur := exp(ln_new)";
    a finished restart's rows and state are left alone; ticket is 0 between calls."""
    rng = numpy.random.default_rng(6000 + 10 * n_haps + n_runs)
    done = (1,) if n_runs > 1 else ()
    for tol, max_iter in ((0.0, 5), (0.0, 1), (1e9, 5)):
        props = rng.dirichlet([1.0] * n_haps, size=n_runs)
        ln_cur = numpy.log(props)
        sums = rng.random((n_runs, n_haps)) * 40.0 + 1e-3
        bufs = {"colsum": guarded_from(sums, numpy.float64, 8, DEV), "ln_cur": guarded_from(ln_cur, numpy.float64, 8, DEV),
                "ln_new": guarded(8 * n_runs * n_haps, 8, DEV), "props_cur": guarded_from(props, numpy.float64, 8, DEV),
                "state": _states(n_runs, done)}
        assert lib.mxm_m_finalize(bufs["colsum"].ptr, bufs["ln_cur"].ptr, bufs["ln_new"].ptr, bufs["props_cur"].ptr,
                                  n_haps, n_runs, tol, max_iter, bufs["state"].ptr, _stream()) == 0, lib.mxm_last_error()
        _sync()
        what = "H=%d B=%d tol=%g max_iter=%d" % (n_haps, n_runs, tol, max_iter)
        for name, buf in bufs.items():
            buf.check(name + " " + what)
        assert numpy.array_equal(bufs["colsum"].get(numpy.float64, sums.shape), sums), what
        got_cur = bufs["ln_cur"].get(numpy.float64, sums.shape)
        got_new = bufs["ln_new"].get(numpy.float64, sums.shape)
        got_props = bufs["props_cur"].get(numpy.float64, sums.shape)
        states = _read_states(bufs["state"], n_runs)
        for b in range(n_runs):
            st = states[b]
            if b in done:
                assert (st.done, st.iters, st.l1, st.ticket, st.error) == (1, 0, 0.0, 0, 0), (what, b)
                assert _is_sentinel(got_new[b]) and numpy.array_equal(got_cur[b], ln_cur[b]) and \
                    numpy.array_equal(got_props[b], props[b]), (what, b)
                continue
            want_new = ln_cur[b] + numpy.log(sums[b]) - numpy.log((props[b] * sums[b]).sum())
            want_l1 = numpy.abs(numpy.exp(want_new) - props[b]).sum()
            # a sum of H <= 8193 positive terms in any order is good to (H - 1) * 2^-53 = 9.1e-13 relative: that much in
            # the log of the total (plus a few ulp of logs below 20 in magnitude); the L1 norm (at most 2) inherits it once
            # through exp(ln_new), whose terms sum to 1, and twice through its own sum of H terms
            assert numpy.allclose(got_new[b], want_new, rtol=0, atol=1e-12), (what, b)
            assert abs(st.l1 - want_l1) <= 4e-12, (what, b)
            want_done = 1 if want_l1 < tol else (2 if 1 >= max_iter else 0)
            assert (st.done, st.iters, st.ticket, st.error) == (want_done, 1, 0, 0), (what, b)
            if want_done == 0:
                assert numpy.array_equal(got_cur[b], got_new[b]), (what, b)
                assert numpy.allclose(got_props[b], numpy.exp(want_new), rtol=0, atol=1e-13), (what, b)
            else:
                assert numpy.array_equal(got_cur[b], ln_cur[b]) and numpy.array_equal(got_props[b], props[b]), (what, b)


# ---- mxm_em_loop / mxm_em_loop_f32 ----------------------------------------------------------------------------------------
def _check_em_loop(lib, rng, n_rows, n_haps, n_runs, n_iter=3, storage="f64", linear=True, atol=1e-12):
    """max_iter = n_iter with tolerance 0: every running restart stops by max_iter with ln_new = log theta_n, the oracle's
    n-th step; restart 1 of several arrives finished and must be left alone, its sentinel colsum row included."""
    from mixemt_amd import _lib
    ldm, ldp, _ = _strides(n_haps, 8)
    mat = _matrix(rng, n_rows, n_haps)
    wts = rng.integers(1, 4, size=n_rows).astype(numpy.float64)
    inits = rng.dirichlet([1.0] * n_haps, size=n_runs)
    ln0 = numpy.log(inits)
    done = (1,) if n_runs > 1 else ()
    lin, _ = _linear(mat)
    if storage == "f32":
        ldp = (n_haps + 3) // 4 * 4 + 4
        lin = lin.astype(numpy.float32)
    p_buf = guarded_2d(n_rows, n_haps, ldp, lin.dtype, 8 if storage == "f64" else 4, DEV, pad=0).put(lin) if linear else None
    m_buf = guarded_2d(n_rows, n_haps, ldm, numpy.float64, 8, DEV).put(mat) if storage == "f64" else None
    w_buf = guarded_from(wts, numpy.float64, 8, DEV)
    vec = {"props_cur": guarded_from(numpy.exp(ln0), numpy.float64, 8, DEV), "ln_cur": guarded_from(ln0, numpy.float64, 8, DEV),
           "ln_new": guarded_from(ln0, numpy.float64, 8, DEV), "colsum": guarded(8 * n_runs * n_haps, 8, DEV),
           "state": _states(n_runs, done)}
    ws, ws_bytes = _workspace(lib, n_rows, n_haps, n_runs)
    host = (_lib.EmState * n_runs)()
    if storage == "f32":
        rc = lib.mxm_em_loop_f32(p_buf.ptr, ldp, w_buf.ptr, n_rows, n_haps, n_runs, vec["props_cur"].ptr, vec["ln_cur"].ptr,
                                 vec["ln_new"].ptr, vec["colsum"].ptr, vec["state"].ptr, 0.0, n_iter, 2, ws.ptr, ws_bytes,
                                 _stream(), host)
    else:
        rc = lib.mxm_em_loop(m_buf.ptr, ldm, p_buf.ptr if p_buf else None, ldp if p_buf else 0, w_buf.ptr, n_rows, n_haps,
                             n_runs, vec["props_cur"].ptr, vec["ln_cur"].ptr, vec["ln_new"].ptr, vec["colsum"].ptr,
                             vec["state"].ptr, 0.0, n_iter, 2, ws.ptr, ws_bytes, _stream(), host)
    assert rc == 0, lib.mxm_last_error()
    _sync()
    what = "R=%d H=%d B=%d %s%s" % (n_rows, n_haps, n_runs, storage, "" if linear else " log space")
    for name, buf in (("P", p_buf), ("M", m_buf)):
        if buf is not None:
            buf.check(name + " " + what, pads="unchanged")
    for name, buf in list(vec.items()) + [("w", w_buf), ("ws", ws)]:
        buf.check(name + " " + what)
    states = _read_states(vec["state"], n_runs)
    got_new = vec["ln_new"].get(numpy.float64, ln0.shape)
    got_cur = vec["ln_cur"].get(numpy.float64, ln0.shape)
    got_sum = vec["colsum"].get(numpy.float64, ln0.shape)
    for b in range(n_runs):
        assert (host[b].done, host[b].iters, host[b].error) == (states[b].done, states[b].iters, states[b].error), (what, b)
        if b in done:
            assert (states[b].done, states[b].iters) == (1, 0), (what, b)
            assert _is_sentinel(got_sum[b]), "colsum row of finished restart %d was written (%s)" % (b, what)
            assert numpy.array_equal(got_new[b], ln0[b]) and numpy.array_equal(got_cur[b], ln0[b]), (what, b)
            continue
        assert (states[b].done, states[b].iters, states[b].ticket, states[b].error) == (2, n_iter, 0, 0), (what, b)
        theta = ln0[b]
        for _ in range(n_iter):
            _, theta = _oracle_step(mat, wts, theta)
        assert numpy.abs(numpy.exp(got_new[b]) - numpy.exp(theta)).max() < atol, (what, b)


@pytest.mark.parametrize("schedule", [0, 2])
@pytest.mark.parametrize("n_rows,n_haps,n_runs", [(257, 66, 4), (700, 1026, 5), (257, 5408, 9), (1, 8192, 1), (700, 8192, 4)])
def test_em_loop_per_iteration_kernels(lib, n_rows, n_haps, n_runs, schedule):
    """mxm_em_loop through {mxm_em_iter; mxm_m_finalize} (mxm_set_loop_fused(0)) under the first and the last restart
    schedule of mxm_set_compact_restarts."""
    assert lib.mxm_set_loop_fused(0, 0) == 0 and lib.mxm_set_compact_restarts(schedule) == 0
    _check_em_loop(lib, numpy.random.default_rng(7000 + n_haps + n_runs), n_rows, n_haps, n_runs)


@pytest.mark.parametrize("n_rows,n_haps,n_runs", [(257, 3, 4), (700, 64, 1), (257, 8193, 1), (1, 1, 1)])
def test_em_loop_log_space(lib, n_rows, n_haps, n_runs):
    """P == NULL: the loop over the log-space kernels, M with an odd stride."""
    assert lib.mxm_set_loop_fused(0, 0) == 0
    _check_em_loop(lib, numpy.random.default_rng(7100 + n_haps), n_rows, n_haps, n_runs, linear=False)


@pytest.mark.parametrize("mode", [-1, 0, 2])
def test_em_loop_forms_at_1500_rows_of_66_columns(lib, mode):
    """The case the comment in mxm_workspace_bytes singles out: the transposed one-launch loop's partials are sized by R,
    not H, and outgrow the tile scratch of a narrow matrix.  Automatic (the transposed form), rows split (2) and the
    per-iteration kernels (0), each inside a workspace of exactly mxm_workspace_bytes(1500, 66, B) bytes."""
    assert lib.mxm_set_loop_fused(mode, 0) == 0
    rng = numpy.random.default_rng(7200)
    for n_runs in (1, 3):
        # the one-launch forms carry the proportions in another variable: the bound of tests/test_gpu_fused.py
        _check_em_loop(lib, rng, 1500, 66, n_runs, atol=1e-12 if mode == 0 else 1e-9)


@pytest.mark.parametrize("mode", [-1, 0])
@pytest.mark.parametrize("n_haps", [4, 8, 16])
def test_em_loop_narrow_form_at_1500_rows(lib, n_haps, mode):
    """The refinement EM's shape (a few contributor columns, log space): the narrow one-launch loop and the per-iteration
    kernels, the bound of tests/test_gpu_narrow_loop.py."""
    assert lib.mxm_set_loop_fused(mode, 0) == 0
    _check_em_loop(lib, numpy.random.default_rng(7300 + n_haps), 1500, n_haps, 1, linear=False)


@pytest.mark.parametrize("n_rows,n_haps,n_runs", [(257, 66, 1), (700, 1026, 4), (257, 8192, 1)])
def test_em_loop_f32_storage(lib, n_rows, n_haps, n_runs):
    """mxm_em_loop_f32 against the oracle at the bound of test_f32_storage_iterations_vs_oracle (float storage of P)."""
    _check_em_loop(lib, numpy.random.default_rng(7400 + n_haps), n_rows, n_haps, n_runs, n_iter=4, storage="f32", atol=2e-7)
