"""
The cohort entries of include/mixemt_hip.h, mixemt_hip_samples_finish.h and mixemt_hip_var_check.h called through ctypes
with every device pointer guard-banded at its exact documented size (tests/_guarded.py): mxm_em_iter_samples,
mxm_em_loop_samples, mxm_votes_samples, mxm_gather_columns_samples, mxm_em_loop_samples_narrow, mxm_assign_reads_samples,
mxm_check_variants_samples.  S = 3 ragged samples back to back: one row; two full tiles of mxm_samples_tile_rows(); two
tiles plus one row.  The reduced matrices come at ld in {4, 8, 16} with every sample's column count below ld; entries
past a sample's columns or candidates must keep their sentinel.  The workspaces are exactly
mxm_samples_workspace_bytes / mxm_samples_finish_workspace_bytes, at the 16 bytes those entries ask for.
References: oracle.em_oracle per sample for the passes and loops, numpy restatements of the headers' rules for the rest.
"""
import ctypes

import numpy
import pytest

from _guarded import guarded, guarded_from
from _guarded_abi import DEV, check_all, coded, is_sentinel, load_lib, read_states, states, stream, sync
from oracle import em_oracle

pytestmark = pytest.mark.gpu

WIDTHS = (66, 1026, 8192)
LDS = (4, 8, 16)


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _rows(lib):
    tile = lib.mxm_samples_tile_rows()
    return numpy.array([0, 1, 1 + 2 * tile, 2 + 4 * tile], dtype=numpy.int64)          # 1, 2 tiles, 2 tiles + 1 row


def _matrix(rng, n_rows, n_haps):
    """Rows of a few distinct values (byte codes), every seventh of about 300 where the width allows (16-bit codes)."""
    mat = numpy.empty((n_rows, n_haps))
    for r in range(n_rows):
        n_val = min(300, n_haps) if r % 7 == 3 else 9
        vals = rng.normal(-20.0, 6.0, size=n_val)
        idx = rng.integers(0, n_val, size=n_haps)
        idx[rng.permutation(n_haps)[:n_val]] = numpy.arange(n_val)
        mat[r] = vals[idx]
    return mat


@pytest.fixture(scope="module", params=WIDTHS)
def cohort(request, lib):
    """Per width: row0, the concatenated matrix, weights -- made once, never written."""
    n_haps = request.param
    row0 = _rows(lib)
    rng = numpy.random.default_rng(300 + n_haps)
    n_rows = int(row0[-1])
    return n_haps, row0, _matrix(rng, n_rows, n_haps), rng.integers(1, 4, size=n_rows).astype(numpy.float64)


def _n_tiles(lib, row0):
    return int(lib.mxm_samples_plan(row0.ctypes.data, len(row0) - 1, None, 0, None))


def _step(mat, wts, ln_props):
    with numpy.errstate(divide="ignore", invalid="ignore", under="ignore"):
        return em_oracle.em_step(mat, wts, ln_props, numpy.empty_like(mat))


# ---- the batched EM pass and loop -------------------------------------------------------------------------------------------
def test_em_iter_samples_and_em_loop_samples(lib, cohort):
    """mixemt_hip.h: "mxm_samples_workspace_bytes: scratch for a plan of n_tiles tiles: the tile table, one partial row of H
    doubles per tile, a fault word per tile"; "colsum[s][h] = T_sh as mxm_em_iter defines it, from sample s's rows under
    props[s].  Samples with state[s].done != 0 are skipped and their colsum rows left untouched"; mxm_em_loop_samples:
    "mxm_em_loop_coded over S samples ... state_host[S] receives the final states"."""
    from mixemt_amd import _lib
    n_haps, row0, mat, wts = cohort
    n_samples = len(row0) - 1
    what = "H=%d" % n_haps
    st, bufs, ndist, rest = coded(lib, mat, wts, what)
    assert len(rest) == 0 and (ndist > 256).any() == (n_haps >= 300)
    ws_bytes = lib.mxm_samples_workspace_bytes(_n_tiles(lib, row0), n_samples, n_haps)
    rng = numpy.random.default_rng(n_haps)
    props = rng.dirichlet([1.0] * n_haps, size=n_samples)
    for done in ((), (1,)):
        state, raw = states(n_samples, done)
        run = {"w": guarded_from(wts, numpy.float64, 8, DEV), "props": guarded_from(props, numpy.float64, 8, DEV), "state": state,
               "colsum": guarded(8 * n_samples * n_haps, 8, DEV), "ws": guarded(ws_bytes, 16, DEV, row_bytes=8 * (n_haps + 8))}
        assert lib.mxm_em_iter_samples(ctypes.byref(st), row0.ctypes.data, n_samples, run["w"].ptr, run["props"].ptr, n_haps,
                                       run["state"].ptr, run["colsum"].ptr, run["ws"].ptr, ws_bytes, stream()) == 0, lib.mxm_last_error()
        sync()
        check_all(bufs, what)
        check_all(run, what)
        assert numpy.array_equal(state.get(numpy.int32), raw), what                 # nothing raised, nothing else written
        got = run["colsum"].get(numpy.float64, (n_samples, n_haps))
        for s in range(n_samples):
            lo, hi = int(row0[s]), int(row0[s + 1])
            if s in done:
                assert is_sentinel(got[s]), "colsum row of finished sample %d was written (%s)" % (s, what)
                continue
            _, new = _step(mat[lo:hi], wts[lo:hi], numpy.log(props[s]))
            assert numpy.abs(got[s] * props[s] - numpy.exp(new) * wts[lo:hi].sum()).max() <= 1e-12 * wts[lo:hi].sum(), (what, s)
    # the loop: three iterations with tolerance 0; sample 1 arrives finished and is left alone
    ln0 = numpy.log(props)
    state, raw = states(n_samples, (1,))
    run = {"w": guarded_from(wts, numpy.float64, 8, DEV), "props_cur": guarded_from(props, numpy.float64, 8, DEV),
           "ln_cur": guarded_from(ln0, numpy.float64, 8, DEV), "ln_new": guarded_from(ln0, numpy.float64, 8, DEV),
           "colsum": guarded(8 * n_samples * n_haps, 8, DEV), "state": state,
           "ws": guarded(ws_bytes, 16, DEV, row_bytes=8 * (n_haps + 8))}
    host = (_lib.EmState * n_samples)()
    assert lib.mxm_em_loop_samples(ctypes.byref(st), row0.ctypes.data, n_samples, run["w"].ptr, n_haps, run["props_cur"].ptr,
                                   run["ln_cur"].ptr, run["ln_new"].ptr, run["colsum"].ptr, run["state"].ptr, 0.0, 3, 2,
                                   run["ws"].ptr, ws_bytes, stream(), host) == 0, lib.mxm_last_error()
    sync()
    check_all(bufs, what)
    check_all(run, what)
    got_new = run["ln_new"].get(numpy.float64, ln0.shape)
    got_sum = run["colsum"].get(numpy.float64, ln0.shape)
    dev_states = read_states(state, n_samples)
    for s in range(n_samples):
        lo, hi = int(row0[s]), int(row0[s + 1])
        assert (host[s].done, host[s].iters, host[s].error) == (dev_states[s].done, dev_states[s].iters, dev_states[s].error)
        if s == 1:
            assert (host[s].done, host[s].iters) == (1, 0) and numpy.array_equal(got_new[s], ln0[s]) and is_sentinel(got_sum[s]), what
            continue
        assert (host[s].done, host[s].iters, host[s].error) == (2, 3, 0), (what, s)
        theta = ln0[s]
        for _ in range(3):
            _, theta = _step(mat[lo:hi], wts[lo:hi], theta)
        assert numpy.abs(numpy.exp(got_new[s]) - numpy.exp(theta)).max() < 1e-12, (what, s)


# ---- the second half: votes, gather, refinement loop, assignment ------------------------------------------------------------
def test_votes_samples(lib, cohort):
    """mixemt_hip_samples_finish.h: "best[r] = first index of max_h (ln_props[s][h] + M[r][h]) for the rows of sample s;
    votes[s][h] = sum of w[r] (NULL: 1) over the sample's rows with best[r] == h; counts[s][h] (nullable) their number;
    first[s][h] = the smallest such row counted from the sample's first row, or R_s when there is none.  lse[r] (nullable)
    = rowmax[r] + log sum_h props[s][h] P[r][h]"; ws: mxm_samples_finish_workspace_bytes(n_tiles, S, 0)."""
    n_haps, row0, mat, wts = cohort
    n_samples, n_rows = len(row0) - 1, int(row0[-1])
    what = "H=%d" % n_haps
    st, bufs, _, _ = coded(lib, mat, wts, what)
    rng = numpy.random.default_rng(n_haps + 1)
    props = rng.dirichlet([1.0] * n_haps, size=n_samples)
    ln_props = numpy.log(props)
    ws_bytes = lib.mxm_samples_finish_workspace_bytes(_n_tiles(lib, row0), n_samples, 0)
    for with_all in (True, False):
        state, raw = states(n_samples)
        run = {"w": guarded_from(wts + 0.25, numpy.float64, 8, DEV), "ln_props": guarded_from(ln_props, numpy.float64, 8, DEV),
               "props": guarded_from(props, numpy.float64, 8, DEV), "best": guarded(4 * n_rows, 4, DEV),
               "votes": guarded(8 * n_samples * n_haps, 8, DEV), "counts": guarded(8 * n_samples * n_haps, 8, DEV),
               "first": guarded(8 * n_samples * n_haps, 8, DEV), "lse": guarded(8 * n_rows, 8, DEV), "state": state,
               "ws": guarded(ws_bytes, 16, DEV)}
        opt = (lambda k: run[k].ptr) if with_all else (lambda k: None)
        assert lib.mxm_votes_samples(ctypes.byref(st), row0.ctypes.data, n_samples, n_haps, opt("w"), run["ln_props"].ptr,
                                     opt("props"), bufs["rowmax"].ptr if with_all else None, run["best"].ptr, run["votes"].ptr,
                                     opt("counts"), run["first"].ptr, opt("lse"), opt("state"), run["ws"].ptr, ws_bytes,
                                     stream()) == 0, lib.mxm_last_error()
        sync()
        check_all(bufs, what)
        check_all(run, what)
        assert numpy.array_equal(state.get(numpy.int32), raw), what
        best = run["best"].get(numpy.int32)
        votes = run["votes"].get(numpy.float64, (n_samples, n_haps))
        first = run["first"].get(numpy.int64, (n_samples, n_haps))
        for s in range(n_samples):
            lo, hi = int(row0[s]), int(row0[s + 1])
            want = (ln_props[s][None, :] + mat[lo:hi]).argmax(axis=1)
            assert numpy.array_equal(best[lo:hi], want), (what, s)
            w_s = wts[lo:hi] + 0.25 if with_all else numpy.ones(hi - lo)
            assert numpy.array_equal(votes[s], numpy.bincount(want, weights=w_s, minlength=n_haps)), (what, s)    # quarters: exact
            want_first = numpy.full(n_haps, hi - lo, dtype=numpy.int64)
            for i in range(hi - lo - 1, -1, -1):
                want_first[want[i]] = i
            assert numpy.array_equal(first[s], want_first), (what, s)
            if with_all:
                assert numpy.array_equal(run["counts"].get(numpy.int64, (n_samples, n_haps))[s], numpy.bincount(want, minlength=n_haps))
                lse = run["lse"].get(numpy.float64)[lo:hi]
                x = ln_props[s][None, :] + mat[lo:hi]
                top = x.max(axis=1)
                assert numpy.abs(lse - (top + numpy.log(numpy.exp(x - top[:, None]).sum(axis=1)))).max() < 1e-10, (what, s)
        if not with_all:
            assert is_sentinel(run["counts"].get(numpy.uint8)) and is_sentinel(run["lse"].get(numpy.uint8)), what


def _columns(rng, n_samples, n_haps, ld):
    """Every sample's contributor columns, ascending, fewer than ld: 1, 3 and ld - 1 of them; the table's tail holds -1."""
    ncol = numpy.array([1, 3, ld - 1][:n_samples], dtype=numpy.int32)
    cols = numpy.full((n_samples, ld), -1, dtype=numpy.int32)
    for s in range(n_samples):
        cols[s, :ncol[s]] = numpy.sort(rng.choice(n_haps, size=ncol[s], replace=False))
    cols[n_samples - 1, ncol[-1] - 1] = n_haps - 1                       # the last column of a record
    return ncol, cols


@pytest.mark.parametrize("ld", LDS)
def test_gather_refine_and_assign_samples(lib, cohort, ld):
    """mixemt_hip_samples_finish.h: mxm_gather_columns_samples "out[r][i] = M[r][cols_host[s][i]] for i < ncol_host[s], -inf
    for ncol_host[s] <= i < ld.  out [R][ld]"; mxm_em_loop_samples_narrow "M [R][ld] (the gather's output), props_cur /
    ln_cur / ln_new [S][ld], state [S]: stop / resume / state as mxm_em_loop" -- the entries past a sample's columns are left
    alone, the columns of M past them never read, E untouched while every sample fits LDS; mxm_assign_reads_samples
    "assigned[r] = perm_host[s][c] of the best c when it beats the runner-up by log_min_fold, else -1; exactly equal values:
    the later column wins.  Samples with ncol <= 1 get 0 throughout.  post (nullable) [R][ld] receives X (-inf in the pad
    columns)"; ws: mxm_samples_finish_workspace_bytes(n_tiles, S, ld)."""
    from mixemt_amd import _lib
    n_haps, row0, mat, wts = cohort
    n_samples, n_rows = len(row0) - 1, int(row0[-1])
    what = "H=%d ld=%d" % (n_haps, ld)
    st, bufs, _, _ = coded(lib, mat, wts, what)
    rng = numpy.random.default_rng(n_haps + ld)
    ncol, cols = _columns(rng, n_samples, n_haps, ld)
    ws_bytes = lib.mxm_samples_finish_workspace_bytes(_n_tiles(lib, row0), n_samples, ld)
    # the gather
    out = guarded(8 * n_rows * ld, 8, DEV)
    ws = guarded(ws_bytes, 16, DEV)
    assert lib.mxm_gather_columns_samples(ctypes.byref(st), row0.ctypes.data, n_samples, n_haps, cols.ctypes.data, ncol.ctypes.data,
                                          ld, out.ptr, ws.ptr, ws_bytes, stream()) == 0, lib.mxm_last_error()
    sync()
    check_all(bufs, what)
    out.check("out " + what)
    ws.check("ws " + what)
    want_sub = numpy.full((n_rows, ld), -numpy.inf)
    for s in range(n_samples):
        lo, hi = int(row0[s]), int(row0[s + 1])
        want_sub[lo:hi, :ncol[s]] = mat[lo:hi][:, cols[s, :ncol[s]]]
    assert numpy.array_equal(out.get(numpy.float64, (n_rows, ld)), want_sub), what
    # the refinement loop over a reduced matrix whose columns past a sample's own are NaN: they are never read
    sub = want_sub.copy()
    sub[numpy.isinf(sub)] = numpy.nan
    theta0 = numpy.frombuffer(b"\xff" * (8 * n_samples * ld), dtype=numpy.float64).reshape(n_samples, ld).copy()
    for s in range(n_samples):
        theta0[s, :ncol[s]] = numpy.log(rng.dirichlet([1.0] * ncol[s]))
    props0 = theta0.copy()                                               # (the tail keeps its 0xFF bytes)
    for s in range(n_samples):
        props0[s, :ncol[s]] = numpy.exp(theta0[s, :ncol[s]])
    state, raw = states(n_samples)
    run = {"M": guarded_from(sub, numpy.float64, 8, DEV), "w": guarded_from(wts, numpy.float64, 8, DEV),
           "props_cur": guarded_from(props0, numpy.float64, 8, DEV), "ln_cur": guarded_from(theta0, numpy.float64, 8, DEV),
           "ln_new": guarded_from(theta0, numpy.float64, 8, DEV), "state": state, "E": guarded(8 * n_rows * ld, 8, DEV),
           "ws": guarded(ws_bytes, 16, DEV)}
    host = (_lib.EmState * n_samples)()
    assert lib.mxm_em_loop_samples_narrow(ctypes.byref(st), row0.ctypes.data, n_samples, n_haps, run["M"].ptr, ld, ncol.ctypes.data,
                                          run["w"].ptr, run["props_cur"].ptr, run["ln_cur"].ptr, run["ln_new"].ptr, run["state"].ptr,
                                          0.0, 3, 2, run["E"].ptr, run["ws"].ptr, ws_bytes, stream(), host) == 0, lib.mxm_last_error()
    sync()
    check_all(bufs, what)
    check_all(run, what)
    assert is_sentinel(run["E"].get(numpy.uint8)), what
    assert numpy.array_equal(run["M"].get(numpy.uint8), numpy.ascontiguousarray(sub).view(numpy.uint8).reshape(-1)), what
    got = {k: run[k].get(numpy.float64, (n_samples, ld)) for k in ("props_cur", "ln_cur", "ln_new")}
    theta_k = numpy.array(theta0)
    theta_n = numpy.array(theta0)
    for s in range(n_samples):
        lo, hi, k = int(row0[s]), int(row0[s + 1]), int(ncol[s])
        assert (host[s].done, host[s].iters) == (2, 3), (what, s)
        for key in got:
            assert is_sentinel(got[key][s, k:]), "%s past the %d columns of sample %d was written (%s)" % (key, k, s, what)
        cur = theta0[s, :k]
        for it in range(3):
            theta_k[s, :k] = cur
            _, cur = _step(want_sub[lo:hi, :k], wts[lo:hi], cur)
        theta_n[s, :k] = cur
        assert numpy.abs(numpy.exp(got["ln_new"][s, :k]) - numpy.exp(theta_n[s, :k])).max() < 1e-12, (what, s)
        assert numpy.abs(numpy.exp(got["ln_cur"][s, :k]) - numpy.exp(theta_k[s, :k])).max() < 1e-12, (what, s)
        assert numpy.abs(got["props_cur"][s, :k] - numpy.exp(theta_k[s, :k])).max() < 1e-12, (what, s)
    # the assignment under theta_k (the posterior's proportions) and theta_{k+1} (the returned ones)
    perm = numpy.full((n_samples, ld), -1, dtype=numpy.int32)
    for s in range(n_samples):
        perm[s, :ncol[s]] = rng.permutation(ncol[s])
    fold = numpy.log(2.0)
    for with_post in (True, False):
        asg = {"M": guarded_from(sub, numpy.float64, 8, DEV), "ln_theta": guarded_from(theta_k, numpy.float64, 8, DEV),
               "props": guarded_from(numpy.exp(theta_k), numpy.float64, 8, DEV), "log_props": guarded_from(theta_n, numpy.float64, 8, DEV),
               "assigned": guarded(4 * n_rows, 4, DEV), "post": guarded(8 * n_rows * ld, 8, DEV), "ws": guarded(ws_bytes, 16, DEV)}
        assert lib.mxm_assign_reads_samples(ctypes.byref(st), row0.ctypes.data, n_samples, n_haps, asg["M"].ptr, ld, ncol.ctypes.data,
                                            perm.ctypes.data, asg["ln_theta"].ptr, asg["props"].ptr, asg["log_props"].ptr, None, fold,
                                            asg["assigned"].ptr, asg["post"].ptr if with_post else None, asg["ws"].ptr, ws_bytes,
                                            stream()) == 0, lib.mxm_last_error()
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
            mix, _ = _step(want_sub[lo:hi, :k], wts[lo:hi], theta_k[s, :k])
            if with_post:
                assert numpy.abs(post[lo:hi, :k] - mix).max() < 1e-10, (what, s)
                assert numpy.isneginf(post[lo:hi, k:]).all(), (what, s)
            if k <= 1:
                assert (assigned[lo:hi] == 0).all(), (what, s)
                continue
            val = mix - theta_n[s, :k][None, :]
            order = numpy.argsort(val, axis=1, kind="stable")                     # ascending; among equals the later column last
            v1, v2 = val[numpy.arange(hi - lo), order[:, -1]], val[numpy.arange(hi - lo), order[:, -2]]
            clear = numpy.abs((v1 - v2) - fold) > 1e-9                            # a margin within rounding of the fold: either
            want = numpy.where(v1 - v2 >= fold, perm[s][order[:, -1]], -1)
            assert numpy.array_equal(assigned[lo:hi][clear], want[clear]) and clear.sum() >= hi - lo - 1, (what, s)
            seen.update((want[clear] >= 0).tolist())
        assert seen == {True, False}, what                                    # both outcomes are in the case


# ---- the variant check ------------------------------------------------------------------------------------------------------
def _variant_check_ref(counts, key_ptr, key, site, site_key, cand, min_var_reads, frac, var_fraction, has_count, var_count):
    """mixemt_hip_var_check.h, candidate by candidate -> [(keep, n_uniq, n_found)]."""
    claimed, out = set(), []
    for h in cand:
        keys = [int(k) for k in key[key_ptr[h]:key_ptr[h + 1]]]
        uniq = [k for k in keys if k not in claimed]
        found = []
        for k in uniq:
            pos, code = k // 4, k % 4
            seen = int(counts[pos, code]) + int(counts[pos, code + 7])
            total = int(counts[pos, 0:4].sum()) + int(counts[pos, 7:11].sum())
            if float(seen) >= max(min_var_reads, float(total) * frac):
                found.append(k)
        keep = len(uniq) == 0 or (has_count and len(found) >= var_count) or (len(uniq) > 0 and len(found) / len(uniq) >= var_fraction)
        if keep:
            claimed.update(found)
            own = {k // 4 for k in keys}
            claimed.update(int(sk) for p, sk in zip(site, site_key) if int(p) not in own and sk >= 0)
        out.append((int(keep), len(uniq), len(found)))
    return out


@pytest.mark.parametrize("has_count", [0, 1])
@pytest.mark.parametrize("ld", LDS)
def test_check_variants_samples(lib, ld, has_count):
    """mixemt_hip_var_check.h: "counts [S][L][16] the samples' pileups (device, 16-byte aligned); key_ptr [H + 1], key;
    site [n_sites], site_key [n_sites]; cand_host [S][ld], ncand_host [S]; keep [S][ld] uint8, n_uniq / n_found [S][ld] int32
    (both nullable): device; entries c >= ncand_host[s] are not written"."""
    rng = numpy.random.default_rng(40 + ld + has_count)
    n_samples, table_len, n_haps, n_sites = 3, 333, 24, 60
    site = numpy.sort(rng.choice(table_len - 1, size=n_sites - 1, replace=False)).astype(numpy.int32)
    site = numpy.append(site, table_len - 1).astype(numpy.int32)                  # a variant on the table's last position
    ref_code = rng.integers(-1, 4, size=n_sites)
    site_key = numpy.where(ref_code >= 0, site * 4 + ref_code, -1).astype(numpy.int32)
    key_ptr, key = [0], []
    for h in range(n_haps):
        at = numpy.sort(rng.choice(n_sites, size=int(rng.integers(0, 9)), replace=False))
        if h == n_haps - 1:
            at = numpy.union1d(at, [n_sites - 1])
        key.extend(int(site[i]) * 4 + int(rng.integers(0, 4)) for i in at)
        key_ptr.append(len(key))
    key_ptr, key = numpy.array(key_ptr, dtype=numpy.int32), numpy.array(key, dtype=numpy.int32)
    counts = rng.integers(0, 6, size=(n_samples, table_len, 16)).astype(numpy.uint32)
    counts[..., 14:] = 0xFFFFFFFF                                                 # the pad bins take no part
    ncand = numpy.array([1, 3, ld - 1], dtype=numpy.int32)
    cand = numpy.full((n_samples, ld), -1, dtype=numpy.int32)
    for s in range(n_samples):
        cand[s, :ncand[s]] = rng.choice(n_haps, size=ncand[s], replace=False)
    cand[2, 0] = n_haps - 1
    args = (2.0, 0.3, 0.5, has_count, 2)
    bufs = {"counts": guarded_from(counts, numpy.uint32, 16, DEV), "key_ptr": guarded_from(key_ptr, numpy.int32, 4, DEV),
            "key": guarded_from(key, numpy.int32, 4, DEV), "site": guarded_from(site, numpy.int32, 4, DEV),
            "site_key": guarded_from(site_key, numpy.int32, 4, DEV), "keep": guarded(n_samples * ld, 1, DEV),
            "n_uniq": guarded(4 * n_samples * ld, 4, DEV), "n_found": guarded(4 * n_samples * ld, 4, DEV)}
    for with_counts in (True, False):
        outs = {"keep": guarded(n_samples * ld, 1, DEV), "n_uniq": guarded(4 * n_samples * ld, 4, DEV),
                "n_found": guarded(4 * n_samples * ld, 4, DEV)}
        assert lib.mxm_check_variants_samples(bufs["counts"].ptr, n_samples, table_len, bufs["key_ptr"].ptr, bufs["key"].ptr, n_haps,
                                              bufs["site"].ptr, bufs["site_key"].ptr, n_sites, table_len - 1, cand.ctypes.data,
                                              ncand.ctypes.data, ld, args[0], args[1], args[2], args[3], args[4], outs["keep"].ptr,
                                              outs["n_uniq"].ptr if with_counts else None, outs["n_found"].ptr if with_counts else None,
                                              stream()) == 0, lib.mxm_last_error()
        sync()
        check_all(bufs, "ld=%d" % ld)
        check_all(outs, "ld=%d" % ld)
        keep = outs["keep"].get(numpy.uint8, (n_samples, ld))
        n_uniq, n_found = outs["n_uniq"].get(numpy.int32, (n_samples, ld)), outs["n_found"].get(numpy.int32, (n_samples, ld))
        kept = 0
        for s in range(n_samples):
            k = int(ncand[s])
            want = _variant_check_ref(counts[s], key_ptr, key, site, site_key, cand[s, :k], *args)
            assert [int(v) for v in keep[s, :k]] == [w[0] for w in want], (ld, s)
            assert (keep[s, k:] == 0xFF).all(), "keep past the %d candidates of sample %d was written" % (k, s)
            kept += sum(w[0] for w in want)
            if with_counts:
                assert [int(v) for v in n_uniq[s, :k]] == [w[1] for w in want] and [int(v) for v in n_found[s, :k]] == [w[2] for w in want]
                assert (n_uniq[s, k:] == -1).all() and (n_found[s, k:] == -1).all(), (ld, s)
            else:
                assert (n_uniq[s] == -1).all() and (n_found[s] == -1).all(), (ld, s)
        assert 0 < kept < int(ncand.sum()), ld
