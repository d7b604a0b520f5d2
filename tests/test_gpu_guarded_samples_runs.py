"""
The entries of include/mixemt_hip_samples_runs.h called through ctypes with every device pointer guard-banded at its
exact documented size (tests/_guarded.py): mxm_votes_samples_runs, mxm_em_loop_samples_narrow_runs,
mxm_assign_reads_samples_runs.  The cohort of tests/test_gpu_guarded_cohort.py (S = 3 ragged samples: one row; two full
tiles; two tiles plus one row) with B = 3 runs per sample, every per-run table [S][B][...]; the reduced matrices come at
ld in {4, 8, 16} with every sample's column count below ld, and entries past a sample's columns must keep their
sentinel.  E is NULL where every sample fits LDS, and exactly c->R x ld doubles where one does not.  The workspaces are
exactly mxm_samples_runs_workspace_bytes, at the 16 bytes the entries ask for.
References: oracle.em_oracle per (sample, run), numpy restatements of the header's rules for the rest.  Values are
compared, not only the guards.
"""
import ctypes

import numpy
import pytest

from _guarded import guarded, guarded_from
from _guarded_abi import DEV, check_all, coded, is_sentinel, load_lib, read_states, states, stream, sync
from test_gpu_guarded_cohort import LDS, _columns, _matrix, _n_tiles, _rows, _step

pytestmark = pytest.mark.gpu

WIDTHS = (66, 1026)
RUNS = 3


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.fixture(scope="module", params=WIDTHS)
def cohort(request, lib):
    """Per width: row0, the concatenated matrix, weights -- made once, never written."""
    n_haps = request.param
    row0 = _rows(lib)
    rng = numpy.random.default_rng(700 + n_haps)
    n_rows = int(row0[-1])
    return n_haps, row0, _matrix(rng, n_rows, n_haps), rng.integers(1, 4, size=n_rows).astype(numpy.float64)


def _fold(terms):
    out = terms[0]
    for term in terms[1:]:
        out = numpy.logaddexp(out, term)
    return out


def test_votes_samples_runs(lib, cohort):
    """mixemt_hip_samples_runs.h: "lse_b = the row normaliser under run b's props / ln_props [S][B][H] ...; v_h = the fold
    over b, in run order starting from run 0, of logaddexp((ln_props[s][b][h] + M[r][h]) - lse_b); best[r] = the first index
    of the maximum ...  votes / counts (nullable) / first / state (nullable) as mxm_votes_samples.  lse (nullable) [R][B]
    receives the lse_b"; ws: mxm_samples_runs_workspace_bytes(n_tiles, S, B, 0)."""
    n_haps, row0, mat, wts = cohort
    n_samples, n_rows = len(row0) - 1, int(row0[-1])
    what = "H=%d" % n_haps
    st, bufs, _, _ = coded(lib, mat, wts, what)
    rng = numpy.random.default_rng(n_haps + 1)
    props = rng.dirichlet([1.0] * n_haps, size=(n_samples, RUNS))
    ln_props = numpy.log(props)
    ws_bytes = lib.mxm_samples_runs_workspace_bytes(_n_tiles(lib, row0), n_samples, RUNS, 0)
    assert ws_bytes > 0
    for with_all in (True, False):
        state, raw = states(n_samples)
        run = {"w": guarded_from(wts + 0.25, numpy.float64, 8, DEV), "ln_props": guarded_from(ln_props, numpy.float64, 8, DEV),
               "props": guarded_from(props, numpy.float64, 8, DEV), "best": guarded(4 * n_rows, 4, DEV),
               "votes": guarded(8 * n_samples * n_haps, 8, DEV), "counts": guarded(8 * n_samples * n_haps, 8, DEV),
               "first": guarded(8 * n_samples * n_haps, 8, DEV), "lse": guarded(8 * n_rows * RUNS, 8, DEV), "state": state,
               "ws": guarded(ws_bytes, 16, DEV)}
        opt = (lambda k: run[k].ptr) if with_all else (lambda k: None)
        assert lib.mxm_votes_samples_runs(ctypes.byref(st), row0.ctypes.data, n_samples, n_haps, RUNS, opt("w"), run["ln_props"].ptr,
                                          run["props"].ptr, bufs["rowmax"].ptr, run["best"].ptr, run["votes"].ptr, opt("counts"),
                                          run["first"].ptr, opt("lse"), opt("state"), run["ws"].ptr, ws_bytes, stream()) == 0, \
            lib.mxm_last_error()
        sync()
        check_all(bufs, what)
        check_all(run, what)
        assert numpy.array_equal(state.get(numpy.int32), raw), what                 # nothing raised, nothing else written
        best = run["best"].get(numpy.int32)
        votes = run["votes"].get(numpy.float64, (n_samples, n_haps))
        first = run["first"].get(numpy.int64, (n_samples, n_haps))
        exact = 0
        for s in range(n_samples):
            lo, hi = int(row0[s]), int(row0[s + 1])
            x = ln_props[s][:, None, :] + mat[lo:hi][None, :, :]                    # [B][R_s][H]
            top = x.max(axis=2)
            want_lse = top + numpy.log(numpy.exp(x - top[:, :, None]).sum(axis=2))   # [B][R_s]
            v = _fold([x[b] - want_lse[b][:, None] for b in range(RUNS)])
            mine = best[lo:hi]
            assert (mine >= 0).all() and (mine < n_haps).all(), (what, s)
            # the header's maximum, to the rounding of the fold (the first such index where numpy's own argmax agrees)
            assert (v[numpy.arange(hi - lo), mine] >= v.max(axis=1) - 1e-12).all(), (what, s)
            exact += int((mine == v.argmax(axis=1)).sum())
            w_s = wts[lo:hi] + 0.25 if with_all else numpy.ones(hi - lo)
            assert numpy.array_equal(votes[s], numpy.bincount(mine, weights=w_s, minlength=n_haps)), (what, s)    # quarters: exact
            want_first = numpy.full(n_haps, hi - lo, dtype=numpy.int64)
            for i in range(hi - lo - 1, -1, -1):
                want_first[mine[i]] = i
            assert numpy.array_equal(first[s], want_first), (what, s)
            if with_all:
                assert numpy.array_equal(run["counts"].get(numpy.int64, (n_samples, n_haps))[s], numpy.bincount(mine, minlength=n_haps))
                lse = run["lse"].get(numpy.float64, (n_rows, RUNS))[lo:hi]
                assert numpy.abs(lse - want_lse.T).max() < 1e-10, (what, s)
        assert exact >= n_rows - 1, (what, exact)
        if not with_all:
            assert is_sentinel(run["counts"].get(numpy.uint8)) and is_sentinel(run["lse"].get(numpy.uint8)), what


def _reduced(row0, mat, ncol, cols, ld):
    sub = numpy.full((int(row0[-1]), ld), numpy.nan)                          # columns past a sample's own: never read
    for s in range(len(row0) - 1):
        lo, hi = int(row0[s]), int(row0[s + 1])
        sub[lo:hi, :ncol[s]] = mat[lo:hi][:, cols[s, :ncol[s]]]
    return sub


def _thetas(rng, ncol, ld, n_runs):
    """[S][B][ld] log vectors: every byte past a sample's columns 0xFF."""
    n = len(ncol)
    theta = numpy.frombuffer(b"\xff" * (8 * n * n_runs * ld), dtype=numpy.float64).reshape(n, n_runs, ld).copy()
    for s in range(n):
        theta[s, :, :ncol[s]] = numpy.log(rng.dirichlet([1.0] * ncol[s], size=n_runs))
    return theta


def _loop_reference(sub, wts, theta0, n_iter):
    """(theta_k, theta_{k+1}) after n_iter iterations of em_oracle.em_step from theta0."""
    cur, before = theta0, theta0
    for _ in range(n_iter):
        before = cur
        _, cur = _step(sub, wts, cur)
    return before, cur


@pytest.mark.parametrize("ld", LDS)
def test_refine_and_assign_samples_runs(lib, cohort, ld):
    """mixemt_hip_samples_runs.h: mxm_em_loop_samples_narrow_runs "props_cur / ln_cur / ln_new [S][B][ld], state and
    state_host [S * B] (entry s * B + b) ...  a finished run is frozen while its siblings go on ...  a smaller sample is
    linearised in each workgroup's LDS and never touches E ...  NULL is accepted when every sample has at most 9216 cells";
    mxm_assign_reads_samples_runs "ln_theta / props [S][B][ld] ..., log_props [S][ld] ...; X_c = the fold over b, in run
    order, of logaddexp((ln_theta[s][b][c] + M[r][c]) - L_b), then + (-log B) ...; v_c = X_c - log_props[s][c] ...  post
    (nullable) [R][ld] receives X (-inf in the pad columns)"; ws: mxm_samples_runs_workspace_bytes(n_tiles, S, B, ld)."""
    from mixemt_amd import _lib
    n_haps, row0, mat, wts = cohort
    n_samples, n_rows = len(row0) - 1, int(row0[-1])
    what = "H=%d ld=%d" % (n_haps, ld)
    st, bufs, _, _ = coded(lib, mat, wts, what)
    rng = numpy.random.default_rng(n_haps + ld)
    ncol, cols = _columns(rng, n_samples, n_haps, ld)
    ws_bytes = lib.mxm_samples_runs_workspace_bytes(_n_tiles(lib, row0), n_samples, RUNS, ld)
    sub = _reduced(row0, mat, ncol, cols, ld)
    theta0 = _thetas(rng, ncol, ld, RUNS)
    props0 = theta0.copy()                                               # (the tails keep their 0xFF bytes)
    for s in range(n_samples):
        props0[s, :, :ncol[s]] = numpy.exp(theta0[s, :, :ncol[s]])
    frozen = 1 * RUNS + 1                                                # run 1 of sample 1 arrives finished
    state, raw = states(n_samples * RUNS, (frozen,))
    run = {"M": guarded_from(sub, numpy.float64, 8, DEV), "w": guarded_from(wts, numpy.float64, 8, DEV),
           "props_cur": guarded_from(props0, numpy.float64, 8, DEV), "ln_cur": guarded_from(theta0, numpy.float64, 8, DEV),
           "ln_new": guarded_from(theta0, numpy.float64, 8, DEV), "state": state, "ws": guarded(ws_bytes, 16, DEV)}
    host = (_lib.EmState * (n_samples * RUNS))()
    assert lib.mxm_em_loop_samples_narrow_runs(ctypes.byref(st), row0.ctypes.data, n_samples, n_haps, RUNS, run["M"].ptr, ld,
                                               ncol.ctypes.data, run["w"].ptr, run["props_cur"].ptr, run["ln_cur"].ptr,
                                               run["ln_new"].ptr, run["state"].ptr, 0.0, 3, 2, None, run["ws"].ptr, ws_bytes, stream(),
                                               host) == 0, lib.mxm_last_error()       # E = NULL: every sample fits LDS
    sync()
    check_all(bufs, what)
    check_all(run, what)
    assert numpy.array_equal(run["M"].get(numpy.uint8), numpy.ascontiguousarray(sub).view(numpy.uint8).reshape(-1)), what
    got = {k: run[k].get(numpy.float64, (n_samples, RUNS, ld)) for k in ("props_cur", "ln_cur", "ln_new")}
    dev_states = read_states(state, n_samples * RUNS)
    theta_k, theta_n = numpy.array(theta0), numpy.array(theta0)
    for s in range(n_samples):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        for b in range(RUNS):
            e = s * RUNS + b
            assert (host[e].done, host[e].iters, host[e].error) == (dev_states[e].done, dev_states[e].iters, dev_states[e].error)
            for key in got:
                assert is_sentinel(got[key][s, b, k:]), "%s past the %d columns of sample %d, run %d was written (%s)" % (key, k, s, b, what)
            if e == frozen:
                assert (host[e].done, host[e].iters) == (1, 0), what
                for key, start in (("props_cur", props0), ("ln_cur", theta0), ("ln_new", theta0)):
                    assert numpy.array_equal(got[key][s, b, :k], start[s, b, :k]), (what, key)
                continue
            assert (host[e].done, host[e].iters) == (2, 3), (what, s, b)
            theta_k[s, b, :k], theta_n[s, b, :k] = _loop_reference(sub[lo:hi, :k], wts[lo:hi], theta0[s, b, :k], 3)
            assert numpy.abs(numpy.exp(got["ln_new"][s, b, :k]) - numpy.exp(theta_n[s, b, :k])).max() < 1e-12, (what, s, b)
            assert numpy.abs(numpy.exp(got["ln_cur"][s, b, :k]) - numpy.exp(theta_k[s, b, :k])).max() < 1e-12, (what, s, b)
            assert numpy.abs(got["props_cur"][s, b, :k] - numpy.exp(theta_k[s, b, :k])).max() < 1e-12, (what, s, b)
    # the assignment under the runs' theta_k (the folded posterior's proportions) and the folded theta_{k+1} (the returned ones)
    log_folded = numpy.frombuffer(b"\xff" * (8 * n_samples * ld), dtype=numpy.float64).reshape(n_samples, ld).copy()
    perm = numpy.full((n_samples, ld), -1, dtype=numpy.int32)
    for s in range(n_samples):
        log_folded[s, :ncol[s]] = theta_n[s, :, :ncol[s]].sum(axis=0) / RUNS
        perm[s, :ncol[s]] = rng.permutation(ncol[s])
    props_k = theta_k.copy()
    for s in range(n_samples):
        props_k[s, :, :ncol[s]] = numpy.exp(theta_k[s, :, :ncol[s]])
    fold = numpy.log(2.0)
    for with_post in (True, False):
        asg = {"M": guarded_from(sub, numpy.float64, 8, DEV), "ln_theta": guarded_from(theta_k, numpy.float64, 8, DEV),
               "props": guarded_from(props_k, numpy.float64, 8, DEV), "log_props": guarded_from(log_folded, numpy.float64, 8, DEV),
               "assigned": guarded(4 * n_rows, 4, DEV), "post": guarded(8 * n_rows * ld, 8, DEV), "ws": guarded(ws_bytes, 16, DEV)}
        assert lib.mxm_assign_reads_samples_runs(ctypes.byref(st), row0.ctypes.data, n_samples, n_haps, RUNS, asg["M"].ptr, ld,
                                                 ncol.ctypes.data, perm.ctypes.data, asg["ln_theta"].ptr, asg["props"].ptr,
                                                 asg["log_props"].ptr, None, fold, asg["assigned"].ptr,
                                                 asg["post"].ptr if with_post else None, asg["ws"].ptr, ws_bytes, stream()) == 0, \
            lib.mxm_last_error()
        sync()
        check_all(bufs, what)
        check_all(asg, what)
        assigned = asg["assigned"].get(numpy.int32)
        post = asg["post"].get(numpy.float64, (n_rows, ld))
        if not with_post:
            assert is_sentinel(post), what
        seen = set()
        for s in range(n_samples):
            lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
            mix = _fold([_step(sub[lo:hi, :k], wts[lo:hi], theta_k[s, b, :k])[0] for b in range(RUNS)]) - numpy.log(RUNS)
            if with_post:
                assert numpy.abs(post[lo:hi, :k] - mix).max() < 1e-10, (what, s)
                assert numpy.isneginf(post[lo:hi, k:]).all(), (what, s)
            if k <= 1:
                assert (assigned[lo:hi] == 0).all(), (what, s)
                continue
            val = mix - log_folded[s, :k][None, :]
            order = numpy.argsort(val, axis=1, kind="stable")                     # ascending; among equals the later column last
            v1, v2 = val[numpy.arange(hi - lo), order[:, -1]], val[numpy.arange(hi - lo), order[:, -2]]
            clear = numpy.abs((v1 - v2) - fold) > 1e-9                            # a margin within rounding of the fold: either
            want = numpy.where(v1 - v2 >= fold, perm[s][order[:, -1]], -1)
            assert numpy.array_equal(assigned[lo:hi][clear], want[clear]) and clear.sum() >= hi - lo - 1, (what, s)
            seen.update((want[clear] >= 0).tolist())
        assert seen == {True, False}, what                                    # both outcomes are in the case


def test_the_loop_with_a_sample_that_needs_e(lib):
    """"for a sample of more than 9216 cells (R_s x ncol) it is formed ONCE per call by a pass of its own into E, which the B
    workgroups of the sample then only read; a smaller sample ... never touches E.  E: exactly c->R x ld doubles ([R][ld],
    the layout of M)": 5 rows x 2 columns beside 3073 rows x 3 columns at ld = 4; the unrefined assignment then takes
    lse [R][B]."""
    from mixemt_amd import _lib
    n_haps, ld, n_runs = 66, 4, 2
    row0 = numpy.array([0, 5, 5 + 3073], dtype=numpy.int64)
    n_rows = int(row0[-1])
    rng = numpy.random.default_rng(3073)
    vals = rng.normal(-20.0, 6.0, size=(n_rows, 9))
    mat = numpy.take_along_axis(vals, rng.integers(0, 9, size=(n_rows, n_haps)), axis=1)
    wts = rng.integers(1, 4, size=n_rows).astype(numpy.float64)
    what = "E"
    st, bufs, _, _ = coded(lib, mat, wts, what)
    ncol = numpy.array([2, 3], dtype=numpy.int32)
    cols = numpy.array([[3, 40, -1, -1], [1, 20, 65, -1]], dtype=numpy.int32)
    sub = _reduced(row0, mat, ncol, cols, ld)
    theta0 = _thetas(rng, ncol, ld, n_runs)
    props0 = theta0.copy()
    for s in range(2):
        props0[s, :, :ncol[s]] = numpy.exp(theta0[s, :, :ncol[s]])
    ws_bytes = lib.mxm_samples_runs_workspace_bytes(_n_tiles(lib, row0), 2, n_runs, ld)
    state, _ = states(2 * n_runs)
    run = {"M": guarded_from(sub, numpy.float64, 8, DEV), "w": guarded_from(wts, numpy.float64, 8, DEV),
           "props_cur": guarded_from(props0, numpy.float64, 8, DEV), "ln_cur": guarded_from(theta0, numpy.float64, 8, DEV),
           "ln_new": guarded_from(theta0, numpy.float64, 8, DEV), "state": state, "E": guarded(8 * n_rows * ld, 8, DEV),
           "ws": guarded(ws_bytes, 16, DEV)}
    host = (_lib.EmState * (2 * n_runs))()
    args = (ctypes.byref(st), row0.ctypes.data, 2, n_haps, n_runs, run["M"].ptr, ld, ncol.ctypes.data, run["w"].ptr,
            run["props_cur"].ptr, run["ln_cur"].ptr, run["ln_new"].ptr, run["state"].ptr, 0.0, 3, 2)
    assert lib.mxm_em_loop_samples_narrow_runs(*(args + (None, run["ws"].ptr, ws_bytes, stream(), host))) == -1     # no E: refused
    sync()
    assert numpy.array_equal(run["ln_new"].get(numpy.float64, theta0.shape).view(numpy.int64), theta0.view(numpy.int64))
    assert lib.mxm_em_loop_samples_narrow_runs(*(args + (run["E"].ptr, run["ws"].ptr, ws_bytes, stream(), host))) == 0, \
        lib.mxm_last_error()
    sync()
    check_all(bufs, what)
    check_all(run, what)
    lin = run["E"].get(numpy.float64, (n_rows, ld))
    assert is_sentinel(lin[:5]), "the sample that fits LDS wrote E"
    big = sub[5:, :3]
    assert numpy.abs(lin[5:, :3] - numpy.exp(big - big.max(axis=1)[:, None])).max() < 1e-15 and (lin[5:, 3] == 0.0).all()
    got_new = run["ln_new"].get(numpy.float64, (2, n_runs, ld))
    for s in range(2):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        for b in range(n_runs):
            assert (host[s * n_runs + b].done, host[s * n_runs + b].iters) == (2, 3), (s, b)
            _, want = _loop_reference(sub[lo:hi, :k], wts[lo:hi], theta0[s, b, :k], 3)
            assert numpy.abs(numpy.exp(got_new[s, b, :k]) - numpy.exp(want)).max() < 1e-12, (s, b)
            assert is_sentinel(got_new[s, b, k:]), (s, b)
    # the assignment with the caller's normalisers lse [R][B]: exactly R x B doubles
    theta_k = run["ln_cur"].get(numpy.float64, (2, n_runs, ld))
    log_folded = numpy.frombuffer(b"\xff" * (8 * 2 * ld), dtype=numpy.float64).reshape(2, ld).copy()
    perm = numpy.array([[1, 0, -1, -1], [2, 0, 1, -1]], dtype=numpy.int32)
    lse = numpy.empty((n_rows, n_runs))
    for s in range(2):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        log_folded[s, :k] = got_new[s, :, :k].sum(axis=0) / n_runs
        for b in range(n_runs):
            x = theta_k[s, b, :k][None, :] + sub[lo:hi, :k]
            lse[lo:hi, b] = x.max(axis=1) + numpy.log(numpy.exp(x - x.max(axis=1)[:, None]).sum(axis=1)) + 0.5      # (not the rows' own)
    asg = {"M": guarded_from(sub, numpy.float64, 8, DEV), "ln_theta": guarded_from(theta_k, numpy.float64, 8, DEV),
           "props": guarded(8 * 2 * n_runs * ld, 8, DEV), "log_props": guarded_from(log_folded, numpy.float64, 8, DEV),
           "lse": guarded_from(lse, numpy.float64, 8, DEV), "assigned": guarded(4 * n_rows, 4, DEV),
           "post": guarded(8 * n_rows * ld, 8, DEV), "ws": guarded(ws_bytes, 16, DEV)}
    assert lib.mxm_assign_reads_samples_runs(ctypes.byref(st), row0.ctypes.data, 2, n_haps, n_runs, asg["M"].ptr, ld, ncol.ctypes.data,
                                             perm.ctypes.data, asg["ln_theta"].ptr, asg["props"].ptr, asg["log_props"].ptr,
                                             asg["lse"].ptr, numpy.log(2.0), asg["assigned"].ptr, asg["post"].ptr, asg["ws"].ptr,
                                             ws_bytes, stream()) == 0, lib.mxm_last_error()
    sync()
    check_all(bufs, what)
    check_all(asg, what)
    assert is_sentinel(asg["props"].get(numpy.uint8))                    # (with lse given the props are not read: NaN would show)
    post = asg["post"].get(numpy.float64, (n_rows, ld))
    for s in range(2):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        want = _fold([(theta_k[s, b, :k][None, :] + sub[lo:hi, :k]) - lse[lo:hi, b][:, None] for b in range(n_runs)]) - numpy.log(n_runs)
        assert numpy.abs(post[lo:hi, :k] - want).max() < 1e-10 and numpy.isneginf(post[lo:hi, k:]).all(), s
    assert set(numpy.unique(asg["assigned"].get(numpy.int32))) <= {-1, 0, 1, 2}
