"""
The entries of include/mixemt_hip_bootstrap.h called through ctypes with every device pointer guard-banded at its exact
documented size (tests/_guarded.py): mxm_bootstrap_weights, mxm_em_loop_samples_narrow_boot, mxm_bootstrap_summary.  The
cohort of tests/test_gpu_guarded_cohort.py (S = 3 ragged samples: one row; two full tiles; two tiles plus one row) with
B = 3 replicates per sample: wb exactly c->R x B doubles, every per-replicate table [S][B][ld] at ld in {4, 8, 16} with every
sample's column count below ld -- entries past a sample's columns must keep their sentinel --, lo / hi / mean / sd [S][ld],
flag [S].  A second cohort puts one sample past MXM_BOOTSTRAP_LDS_ROWS (the workspace's 32-bit counters) and past 9216 cells
(E exactly c->R x ld doubles).  The workspaces are exactly mxm_bootstrap_workspace_bytes, at the 16 bytes the entries ask for.
References: tests/_bootstrap_ref.py, oracle.em_oracle per (sample, replicate).  Values are compared, not only the guards.
"""
import ctypes
import math

import numpy
import pytest

import _bootstrap_ref as ref
from _guarded import guarded, guarded_from
from _guarded_abi import DEV, check_all, is_sentinel, load_lib, read_states, states, stream, sync
from test_gpu_guarded_cohort import LDS, _columns, _n_tiles, _rows
from test_gpu_guarded_samples_runs import _loop_reference

pytestmark = pytest.mark.gpu

BOOT = 3
SEED = 99
IDS = numpy.array([4000000000, 7, 0], dtype=numpy.uint32)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _coded(n_rows):
    """An mxm_coded over n_rows rows whose arrays are guarded and never read: no bootstrap entry reads a record."""
    from mixemt_amd import _lib
    bufs = {"rec": guarded(64, 16, DEV), "rec_off": guarded(8 * n_rows, 8, DEV), "ndist": guarded(4 * n_rows, 4, DEV)}
    return _lib.Coded(bufs["rec"].ptr, bufs["rec_off"].ptr, bufs["ndist"].ptr, n_rows, None, 0, None, 0, None, 0), bufs


def _weights(lib, st, row0, wts, ids, n_boot):
    """mxm_bootstrap_weights into guarded buffers -> (buffers, wb [R * B] as the entry left it)."""
    n_samples, n_rows = len(row0) - 1, int(row0[-1])
    ws_bytes = lib.mxm_bootstrap_workspace_bytes(_n_tiles(lib, row0), n_samples, n_boot, 0)
    assert ws_bytes > 0
    state, raw = states(n_samples)
    run = {"w": guarded_from(wts, numpy.float64, 8, DEV), "wb": guarded(8 * n_rows * n_boot, 8, DEV), "state": state,
           "ws": guarded(ws_bytes, 16, DEV)}
    assert lib.mxm_bootstrap_weights(ctypes.byref(st), row0.ctypes.data, n_samples, n_boot, run["w"].ptr, SEED, ids.ctypes.data,
                                     run["wb"].ptr, run["state"].ptr, run["ws"].ptr, ws_bytes, stream()) == 0, lib.mxm_last_error()
    sync()
    check_all(run, "weights")
    assert numpy.array_equal(state.get(numpy.int32), raw)                    # no error code, nothing else written
    assert numpy.array_equal(run["w"].get(numpy.float64), wts)
    return run, run["wb"].get(numpy.float64)


def _check_weights(row0, wts, ids, n_boot, wb):
    for s in range(len(row0) - 1):
        lo, hi = int(row0[s]), int(row0[s + 1])
        got = wb[n_boot * lo:n_boot * hi].reshape(n_boot, hi - lo)
        want = ref.resample_all(wts[lo:hi], SEED, int(ids[s]), n_boot)
        assert numpy.array_equal(got.view(numpy.int64), want.view(numpy.int64)), s


@pytest.mark.parametrize("ld", LDS)
def test_weights_loop_and_summary(lib, ld):
    """mixemt_hip_bootstrap.h: "the weights are wb[B * row0[s] + b * R_s + i] (... c->R x B doubles)"; the loop's "props_cur /
    ln_cur / ln_new [S][B][ld], state and state_host [S * B] (entry s * B + b)"; the summary's "x[s][b][k] ... ([S][B][ld]; the
    pad columns are not touched) ... lo / hi [S][ld] ... flag[s] (int32 [S])"; ws: mxm_bootstrap_workspace_bytes."""
    from mixemt_amd import _lib
    row0 = _rows(lib)
    n_samples, n_rows = len(row0) - 1, int(row0[-1])
    rng = numpy.random.default_rng(900 + ld)
    wts = rng.integers(0, 4, size=n_rows).astype(numpy.float64)
    wts[0] = 3.0                                                            # (the one-row sample needs a draw)
    st, bufs = _coded(n_rows)
    made, wb = _weights(lib, st, row0, wts, IDS, BOOT)
    _check_weights(row0, wts, IDS, BOOT, wb)
    check_all(bufs, "weights")

    ncol, _ = _columns(rng, n_samples, 66, ld)
    sub = numpy.full((n_rows, ld), numpy.nan)                                # columns past a sample's own: never read
    theta0 = numpy.frombuffer(b"\xff" * (8 * n_samples * BOOT * ld), dtype=numpy.float64).reshape(n_samples, BOOT, ld).copy()
    for s in range(n_samples):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        sub[lo:hi, :k] = rng.normal(-20.0, 6.0, size=(hi - lo, k))
        theta0[s, :, :k] = numpy.log(rng.dirichlet([1.0] * k))[None, :]      # one start for all of a sample's replicates
    props0 = theta0.copy()
    for s in range(n_samples):
        props0[s, :, :ncol[s]] = numpy.exp(theta0[s, :, :ncol[s]])
    ws_bytes = lib.mxm_bootstrap_workspace_bytes(_n_tiles(lib, row0), n_samples, BOOT, ld)
    state, _ = states(n_samples * BOOT)
    run = {"M": guarded_from(sub, numpy.float64, 8, DEV), "wb": made["wb"], "props_cur": guarded_from(props0, numpy.float64, 8, DEV),
           "ln_cur": guarded_from(theta0, numpy.float64, 8, DEV), "ln_new": guarded_from(theta0, numpy.float64, 8, DEV),
           "state": state, "ws": guarded(ws_bytes, 16, DEV)}
    host = (_lib.EmState * (n_samples * BOOT))()
    what = "ld=%d" % ld
    assert lib.mxm_em_loop_samples_narrow_boot(ctypes.byref(st), row0.ctypes.data, n_samples, 66, BOOT, run["M"].ptr, ld,
                                               ncol.ctypes.data, run["wb"].ptr, run["props_cur"].ptr, run["ln_cur"].ptr,
                                               run["ln_new"].ptr, run["state"].ptr, 0.0, 3, 2, None, run["ws"].ptr, ws_bytes, stream(),
                                               host) == 0, lib.mxm_last_error()       # E = NULL: every sample fits LDS
    sync()
    check_all(bufs, what)
    check_all(run, what)
    assert numpy.array_equal(run["wb"].get(numpy.float64).view(numpy.int64), wb.view(numpy.int64)), what     # read, not written
    got = {k: run[k].get(numpy.float64, (n_samples, BOOT, ld)) for k in ("props_cur", "ln_cur", "ln_new")}
    dev_states = read_states(state, n_samples * BOOT)
    for s in range(n_samples):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        for b in range(BOOT):
            e = s * BOOT + b
            assert (host[e].done, host[e].iters, host[e].error) == (dev_states[e].done, dev_states[e].iters, dev_states[e].error)
            assert (host[e].done, host[e].iters) == (2, 3), (what, s, b)
            for key in got:
                assert is_sentinel(got[key][s, b, k:]), "%s past the %d columns of sample %d, replicate %d was written (%s)" % (key, k, s, b, what)
            w_b = wb[BOOT * lo + b * (hi - lo):BOOT * lo + (b + 1) * (hi - lo)]
            theta_k, theta_n = _loop_reference(sub[lo:hi, :k], w_b, theta0[s, b, :k], 3)
            assert numpy.abs(numpy.exp(got["ln_new"][s, b, :k]) - numpy.exp(theta_n)).max() < 1e-12, (what, s, b)
            assert numpy.abs(numpy.exp(got["ln_cur"][s, b, :k]) - numpy.exp(theta_k)).max() < 1e-12, (what, s, b)
            assert numpy.abs(got["props_cur"][s, b, :k] - numpy.exp(theta_k)).max() < 1e-12, (what, s, b)

    out = {"ln_new": run["ln_new"], "state": state, "x": guarded(8 * n_samples * BOOT * ld, 8, DEV)}
    for name in ("lo", "hi", "mean", "sd"):
        out[name] = guarded(8 * n_samples * ld, 8, DEV)
    out["flag"] = guarded(4 * n_samples, 4, DEV)
    assert lib.mxm_bootstrap_summary(n_samples, BOOT, ld, ncol.ctypes.data, out["ln_new"].ptr, out["state"].ptr, 0.25, 0.9, out["x"].ptr,
                                     out["lo"].ptr, out["hi"].ptr, out["mean"].ptr, out["sd"].ptr, out["flag"].ptr, stream()) == 0, \
        lib.mxm_last_error()
    sync()
    check_all(out, what)
    assert numpy.array_equal(out["ln_new"].get(numpy.float64, (n_samples, BOOT, ld)).view(numpy.int64), got["ln_new"].view(numpy.int64))
    x = out["x"].get(numpy.float64, (n_samples, BOOT, ld))
    tabs = {name: out[name].get(numpy.float64, (n_samples, ld)) for name in ("lo", "hi", "mean", "sd")}
    assert out["flag"].get(numpy.int32).tolist() == [0] * n_samples
    bound = 4 * BOOT * 2.0 ** -53
    for s in range(n_samples):
        k = int(ncol[s])
        assert is_sentinel(x[s, :, k:]) and all(is_sentinel(t[s, k:]) for t in tabs.values()), (what, s)
        want_x = numpy.exp(got["ln_new"][s, :, :k])
        assert (numpy.abs(x[s, :, :k] - want_x) <= 2 * numpy.spacing(want_x)).all(), (what, s)
        for c in range(k):
            col = numpy.sort(x[s, :, c])
            assert tabs["lo"][s, c] == ref.quantile(col, 0.25) and tabs["hi"][s, c] == ref.quantile(col, 0.9), (what, s, c)
            exact = math.fsum(col) / BOOT
            assert abs(tabs["mean"][s, c] - exact) <= bound, (what, s, c)
            assert abs(tabs["sd"][s, c] - math.sqrt(math.fsum((col - exact) ** 2) / (BOOT - 1))) <= bound, (what, s, c)


def test_a_sample_past_the_lds_rows_and_past_the_lds_cells(lib):
    """"in LDS for a sample of at most MXM_BOOTSTRAP_LDS_ROWS rows, in 32-bit global counters in the workspace above it" and
    "E exactly c->R x ld doubles; NULL accepted when every sample has at most 9216 cells, refused otherwise": 5 rows x 2
    columns beside 8193 rows x 3 columns at ld = 4, B = 66 replicates (two rounds of the workspace's 64 counter rows)."""
    from mixemt_amd import _lib
    n_boot, ld = 66, 4
    row0 = numpy.array([0, 5, 5 + 8193], dtype=numpy.int64)
    n_rows = int(row0[-1])
    rng = numpy.random.default_rng(8193)
    wts = (rng.random(n_rows) < 0.05).astype(numpy.float64)                   # N of a few hundred: the references stay quick
    wts[:5] = (2, 0, 1, 0, 3)
    ids = numpy.array([5, 6], dtype=numpy.uint32)
    st, bufs = _coded(n_rows)
    made, wb = _weights(lib, st, row0, wts, ids, n_boot)
    _check_weights(row0, wts, ids, n_boot, wb)
    check_all(bufs, "large")
    ncol = numpy.array([2, 3], dtype=numpy.int32)
    sub = numpy.full((n_rows, ld), numpy.nan)
    sub[:5, :2] = rng.normal(-20.0, 6.0, size=(5, 2))
    sub[5:, :3] = rng.normal(-20.0, 6.0, size=(8193, 3))
    theta0 = numpy.frombuffer(b"\xff" * (8 * 2 * n_boot * ld), dtype=numpy.float64).reshape(2, n_boot, ld).copy()
    for s in range(2):
        theta0[s, :, :ncol[s]] = numpy.log(rng.dirichlet([1.0] * ncol[s]))[None, :]
    props0 = theta0.copy()
    for s in range(2):
        props0[s, :, :ncol[s]] = numpy.exp(theta0[s, :, :ncol[s]])
    ws_bytes = lib.mxm_bootstrap_workspace_bytes(_n_tiles(lib, row0), 2, n_boot, ld)
    state, _ = states(2 * n_boot)
    run = {"M": guarded_from(sub, numpy.float64, 8, DEV), "wb": made["wb"], "props_cur": guarded_from(props0, numpy.float64, 8, DEV),
           "ln_cur": guarded_from(theta0, numpy.float64, 8, DEV), "ln_new": guarded_from(theta0, numpy.float64, 8, DEV),
           "state": state, "E": guarded(8 * n_rows * ld, 8, DEV), "ws": guarded(ws_bytes, 16, DEV)}
    host = (_lib.EmState * (2 * n_boot))()
    args = (ctypes.byref(st), row0.ctypes.data, 2, 66, n_boot, run["M"].ptr, ld, ncol.ctypes.data, run["wb"].ptr, run["props_cur"].ptr,
            run["ln_cur"].ptr, run["ln_new"].ptr, run["state"].ptr, 0.0, 3, 2)
    assert lib.mxm_em_loop_samples_narrow_boot(*(args + (None, run["ws"].ptr, ws_bytes, stream(), host))) == -1     # no E: refused
    sync()
    assert numpy.array_equal(run["ln_new"].get(numpy.float64, theta0.shape).view(numpy.int64), theta0.view(numpy.int64))
    assert lib.mxm_em_loop_samples_narrow_boot(*(args + (run["E"].ptr, run["ws"].ptr, ws_bytes, stream(), host))) == 0, \
        lib.mxm_last_error()
    sync()
    check_all(bufs, "large")
    check_all(run, "large")
    lin = run["E"].get(numpy.float64, (n_rows, ld))
    assert is_sentinel(lin[:5]), "the sample that fits LDS wrote E"
    big = sub[5:, :3]
    assert numpy.abs(lin[5:, :3] - numpy.exp(big - big.max(axis=1)[:, None])).max() < 1e-15 and (lin[5:, 3] == 0.0).all()
    got_new = run["ln_new"].get(numpy.float64, (2, n_boot, ld))
    for s in range(2):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        for b in (0, 1, 63, 64, 65):
            assert (host[s * n_boot + b].done, host[s * n_boot + b].iters) == (2, 3), (s, b)
            w_b = wb[n_boot * lo + b * (hi - lo):n_boot * lo + (b + 1) * (hi - lo)]
            _, want = _loop_reference(sub[lo:hi, :k], w_b, theta0[s, b, :k], 3)
            assert numpy.abs(numpy.exp(got_new[s, b, :k]) - numpy.exp(want)).max() < 1e-12, (s, b)
            assert is_sentinel(got_new[s, b, k:]), (s, b)
