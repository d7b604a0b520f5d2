"""
The entries of include/mixemt_hip_support.h called through ctypes with every buffer guard-banded at its exact documented size
(tests/_guarded.py): mxm_em_loop_samples_narrow_masks and mxm_loglik_samples_masks.  The cohort of
tests/test_gpu_guarded_cohort.py (S = 3 ragged samples: one row; two full tiles; two tiles plus one row) with B = 3 fits per
sample, one slot unused: every per-fit table [S][B][ld] at ld in {4, 8, 16} with every sample's column count below ld --
entries past a sample's columns and the unused slot must keep their sentinel --, ll [S][B], n_eff [S], mask_host [S][B] and
state_host [S * B] guarded ON THE HOST.  A second cohort puts one sample past 9216 cells: E exactly B x c->R x ld doubles.  The
workspaces are exactly mxm_support_workspace_bytes, at the 16 bytes the entries ask for.  References: the loop of
tests/test_gpu_guarded_samples_runs.py on the masked-in columns, tests/_support_ref.py.  Values are compared, not only the guards.
"""
import ctypes

import numpy
import pytest

import _support_ref as ref
from _guarded import guarded, guarded_from
from _guarded_abi import DEV, check_all, is_sentinel, load_lib, read_states, states, stream, sync
from test_gpu_guarded_bootstrap import _coded
from test_gpu_guarded_cohort import LDS, _columns, _n_tiles, _rows
from test_gpu_guarded_samples_runs import _loop_reference

pytestmark = pytest.mark.gpu

FITS = 3


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _host_state(n):
    from mixemt_amd import _lib
    buf = guarded(n * ctypes.sizeof(_lib.EmState), 8, None)
    return buf, ctypes.cast(buf.ptr, ctypes.POINTER(_lib.EmState))


def _tables(rng, masks, ncol, ld):
    """theta0 / props0 [S][B][ld]: a start over every mask's columns, the sentinel everywhere else."""
    n, n_fits = masks.shape
    theta0 = numpy.frombuffer(b"\xff" * (8 * n * n_fits * ld), dtype=numpy.float64).reshape(n, n_fits, ld).copy()
    props0 = theta0.copy()
    for s in range(n):
        for b in range(n_fits):
            cols = ref.mask_columns(masks[s, b])
            if cols:
                theta0[s, b, cols] = numpy.log(rng.dirichlet([1.0] * len(cols)))
                props0[s, b, cols] = numpy.exp(theta0[s, b, cols])
    return theta0, props0


def _check_loop(got, host, row0, ncol, masks, sub, wts, theta0, n_iter, what):
    n, n_fits = masks.shape
    for s in range(n):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        for b in range(n_fits):
            e = s * n_fits + b
            cols = ref.mask_columns(masks[s, b])
            if not cols:
                assert (host[e].done, host[e].iters) == (0, 0), (what, s, b)
                assert all(is_sentinel(got[key][s, b]) for key in got), "the unused slot (%d, %d) was written (%s)" % (s, b, what)
                continue
            assert (host[e].done, host[e].iters) == (2, n_iter), (what, s, b)
            out = [c for c in range(k) if c not in cols]
            for key in got:
                assert is_sentinel(got[key][s, b, k:]), "%s past the %d columns of sample %d, fit %d was written (%s)" % (key, k, s, b, what)
            assert numpy.isneginf(got["ln_cur"][s, b, out]).all() and numpy.isneginf(got["ln_new"][s, b, out]).all(), (what, s, b)
            assert not got["props_cur"][s, b, out].any(), (what, s, b)
            theta_k, theta_n = _loop_reference(sub[lo:hi][:, cols], wts[lo:hi], theta0[s, b, cols], n_iter)
            assert numpy.abs(numpy.exp(got["ln_new"][s, b, cols]) - numpy.exp(theta_n)).max() < 1e-12, (what, s, b)
            assert numpy.abs(numpy.exp(got["ln_cur"][s, b, cols]) - numpy.exp(theta_k)).max() < 1e-12, (what, s, b)
            assert numpy.abs(got["props_cur"][s, b, cols] - numpy.exp(theta_k)).max() < 1e-12, (what, s, b)


@pytest.mark.parametrize("ld", LDS)
def test_loop_and_loglik(lib, ld):
    """mixemt_hip_support.h: "props_cur / ln_cur / ln_new [S][B][ld], state and state_host [S * B] (entry s * B + b)"; "mask_host
    [S][B] (host, uint32)"; "Mask 0 marks an unused slot: its outputs and its state are left alone"; "ll [S][B] (an unused
    slot's is left alone); n_eff [S]"; ws: mxm_support_workspace_bytes."""
    row0 = _rows(lib)
    n_samples, n_rows = len(row0) - 1, int(row0[-1])
    rng = numpy.random.default_rng(700 + ld)
    wts = rng.integers(0, 4, size=n_rows).astype(numpy.float64)
    wts[0] = 3.0
    st, bufs = _coded(n_rows)
    ncol, _ = _columns(rng, n_samples, 66, ld)                              # 1, 3 and ld - 1 columns
    # per sample: all its columns; its highest column alone (K = 1: the unused slot instead); the unused slot / an alternating mask
    masks = numpy.array([[1, 0, 0], [0b111, 0b100, 0], [(1 << (ld - 1)) - 1, 1 << (ld - 2), sum(1 << c for c in range(0, ld - 1, 2))]],
                        dtype=numpy.uint32)
    sub = numpy.full((n_rows, ld), numpy.nan)                                # columns past a sample's own: never read
    for s in range(n_samples):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        sub[lo:hi, :k] = rng.normal(-20.0, 6.0, size=(hi - lo, k))
    theta0, props0 = _tables(rng, masks, ncol, ld)
    ws_bytes = lib.mxm_support_workspace_bytes(_n_tiles(lib, row0), n_samples, FITS, ld)
    assert ws_bytes > 0
    state, raw = states(n_samples * FITS)
    mask_host = guarded_from(masks, numpy.uint32, 4, None)
    host_buf, host = _host_state(n_samples * FITS)
    run = {"M": guarded_from(sub, numpy.float64, 8, DEV), "w": guarded_from(wts, numpy.float64, 8, DEV),
           "props_cur": guarded_from(props0, numpy.float64, 8, DEV), "ln_cur": guarded_from(theta0, numpy.float64, 8, DEV),
           "ln_new": guarded_from(theta0, numpy.float64, 8, DEV), "state": state, "ws": guarded(ws_bytes, 16, DEV),
           "mask_host": mask_host, "state_host": host_buf}
    what = "ld=%d" % ld
    assert lib.mxm_em_loop_samples_narrow_masks(ctypes.byref(st), row0.ctypes.data, n_samples, 66, FITS, run["M"].ptr, ld,
                                                ncol.ctypes.data, mask_host.ptr, run["w"].ptr, run["props_cur"].ptr, run["ln_cur"].ptr,
                                                run["ln_new"].ptr, run["state"].ptr, 0.0, 3, 2, None, run["ws"].ptr, ws_bytes, stream(),
                                                host) == 0, lib.mxm_last_error()        # E = NULL: every sample fits LDS
    sync()
    check_all(bufs, what)
    check_all(run, what)
    assert numpy.array_equal(mask_host.get(numpy.uint32, masks.shape), masks)
    got = {k: run[k].get(numpy.float64, (n_samples, FITS, ld)) for k in ("props_cur", "ln_cur", "ln_new")}
    dev_states = read_states(state, n_samples * FITS)
    for e in range(n_samples * FITS):
        assert (host[e].done, host[e].iters, host[e].error) == (dev_states[e].done, dev_states[e].iters, dev_states[e].error), e
    _check_loop(got, host, row0, ncol, masks, sub, wts, theta0, 3, what)

    out = {"M": run["M"], "w": run["w"], "ln_props": run["ln_new"], "ll": guarded(8 * n_samples * FITS, 8, DEV),
           "n_eff": guarded(8 * n_samples, 8, DEV), "ws": guarded(ws_bytes, 16, DEV), "mask_host": mask_host}
    assert lib.mxm_loglik_samples_masks(ctypes.byref(st), row0.ctypes.data, n_samples, 66, FITS, out["M"].ptr, ld, ncol.ctypes.data,
                                        mask_host.ptr, out["w"].ptr, out["ln_props"].ptr, out["ll"].ptr, out["n_eff"].ptr, out["ws"].ptr,
                                        ws_bytes, stream()) == 0, lib.mxm_last_error()
    sync()
    check_all(bufs, what)
    check_all(out, what)
    assert numpy.array_equal(out["ln_props"].get(numpy.float64, (n_samples, FITS, ld)).view(numpy.int64), got["ln_new"].view(numpy.int64))
    ll = out["ll"].get(numpy.float64, (n_samples, FITS))
    n_eff = out["n_eff"].get(numpy.float64)
    for s in range(n_samples):
        lo, hi = int(row0[s]), int(row0[s + 1])
        assert abs(n_eff[s] - wts[lo:hi].sum()) <= 1e-12 * wts[lo:hi].sum(), (what, s)
        for b in range(FITS):
            if masks[s, b] == 0:
                assert is_sentinel(ll[s, b:b + 1]), "ll of the unused slot (%d, %d) was written (%s)" % (s, b, what)
            else:
                want = float(ref.exact_loglik(sub[lo:hi], got["ln_new"][s, b], wts[lo:hi], int(masks[s, b])))
                assert abs(ll[s, b] - want) <= 1e-12 * abs(want), (what, s, b, ll[s, b], want)


def test_a_sample_past_the_lds_cells_keeps_every_fit_in_its_own_slice_of_e(lib):
    """"E is exactly B x c->R x ld doubles, fit (s, b) owns the slice at (B * row0[s] + b * R_s) * ld ... NULL accepted when every
    sample has at most 9216 cells, refused otherwise": 5 rows x 2 columns beside 3073 rows x 3 columns (9219 cells) at ld = 4."""
    ld = 4
    row0 = numpy.array([0, 5, 5 + 3073], dtype=numpy.int64)
    n_rows = int(row0[-1])
    rng = numpy.random.default_rng(3073)
    wts = rng.integers(0, 4, size=n_rows).astype(numpy.float64)
    st, bufs = _coded(n_rows)
    ncol = numpy.array([2, 3], dtype=numpy.int32)
    masks = numpy.array([[0b11, 0, 0b10], [0b111, 0b101, 0b010]], dtype=numpy.uint32)
    sub = numpy.full((n_rows, ld), numpy.nan)
    sub[:5, :2] = rng.normal(-20.0, 6.0, size=(5, 2))
    sub[5:, :3] = rng.normal(-20.0, 6.0, size=(3073, 3))
    theta0, props0 = _tables(rng, masks, ncol, ld)
    ws_bytes = lib.mxm_support_workspace_bytes(_n_tiles(lib, row0), 2, FITS, ld)
    state, _ = states(2 * FITS)
    mask_host = guarded_from(masks, numpy.uint32, 4, None)
    host_buf, host = _host_state(2 * FITS)
    run = {"M": guarded_from(sub, numpy.float64, 8, DEV), "w": guarded_from(wts, numpy.float64, 8, DEV),
           "props_cur": guarded_from(props0, numpy.float64, 8, DEV), "ln_cur": guarded_from(theta0, numpy.float64, 8, DEV),
           "ln_new": guarded_from(theta0, numpy.float64, 8, DEV), "state": state, "E": guarded(8 * FITS * n_rows * ld, 8, DEV),
           "ws": guarded(ws_bytes, 16, DEV), "mask_host": mask_host, "state_host": host_buf}
    args = (ctypes.byref(st), row0.ctypes.data, 2, 66, FITS, run["M"].ptr, ld, ncol.ctypes.data, mask_host.ptr, run["w"].ptr,
            run["props_cur"].ptr, run["ln_cur"].ptr, run["ln_new"].ptr, run["state"].ptr, 0.0, 3, 2)
    assert lib.mxm_em_loop_samples_narrow_masks(*(args + (None, run["ws"].ptr, ws_bytes, stream(), host))) == -1     # no E: refused
    sync()
    assert numpy.array_equal(run["ln_new"].get(numpy.float64, theta0.shape).view(numpy.int64), theta0.view(numpy.int64))
    assert lib.mxm_em_loop_samples_narrow_masks(*(args + (run["E"].ptr, run["ws"].ptr, ws_bytes, stream(), host))) == 0, \
        lib.mxm_last_error()
    sync()
    check_all(bufs, "large")
    check_all(run, "large")
    lin = run["E"].get(numpy.float64, (FITS * n_rows, ld))
    assert is_sentinel(lin[:FITS * 5]), "the sample that fits LDS wrote E"
    for b in range(FITS):
        cols = ref.mask_columns(masks[1, b])
        part = lin[FITS * 5 + b * 3073:FITS * 5 + (b + 1) * 3073]
        big = sub[5:][:, cols]
        assert numpy.abs(part[:, cols] - numpy.exp(big - big.max(axis=1)[:, None])).max() < 1e-15, b
        assert not part[:, [c for c in range(ld) if c not in cols]].any(), b
    got = {k: run[k].get(numpy.float64, (2, FITS, ld)) for k in ("props_cur", "ln_cur", "ln_new")}
    _check_loop(got, host, row0, ncol, masks, sub, wts, theta0, 3, "large")
