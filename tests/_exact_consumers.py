"""
Extended-precision reference of the CONSUMERS of the posterior -- the row normaliser, the posterior of one run, the
logaddexp fold over runs, the contributor vote, the read assignment and the two small vector entries -- in the style of
tests/_exact.py: plain numpy in numpy.longdouble, CPU only, no device code and no use of the library.  It reads the bits the
kernels read (the fp64 log matrix -- dense, or what the records' log tables hold, which is the same bits: records are
lossless --, the fp64 ln_props / props, integer weights), so every difference is the kernel's own rounding.

    exact_row_lse(M, ln_props)            shift + log(pairwise sum of exp(a - shift)), a = ln p + M; an empty row: -inf
    exact_posterior(M, ln_props)          _exact.exact_posterior, reused
    exact_fold(blocks, delta)             logaddexp over the blocks in order, hi + log1p(exp(lo - hi)), + delta once
    exact_vote_values(M, ln_runs)         the values the vote maximises per row: ln p + M with one run (the normaliser drops
                                          out), the fold of the runs' posteriors with several
    top_two(V)                            (best column, best value, runner-up value) per row
    exact_assign_values(X, log_props)     v_c = X_c - log_props_c
    exact_labels(V, log_min_fold)         (label, margin m_r = v1 - v2) per row: the best column if m_r >= log_min_fold else -1
    exact_log_normalize(T)                log T - log sum T
    exact_l1_exp_diff(a, b)               sum_h |exp(a_h) - exp(b_h)|, each term without cancellation

Beside each stands its COMPARISON PASS, the same quantity in plain fp64 numpy (numpy.logaddexp chains, scipy's logsumexp
as oracle/em_oracle.py restates it): what seq_colsum is for the EM passes -- the error an honest fp64 implementation has.

The rule (no constant of its own):
    values      |got - exact| <= _exact.abs_bound(the comparison pass's largest error, exact values) = 8 max(own, u max |value|)
                over the entries whose exact value is finite; the pattern of -inf / NaN equals the reference's
    decisions   d = 2 x that bound (two values enter a gap): best[r] must be a column whose exact value is within d of the
                exact row maximum; assigned[r] must be the exact label unless |m_r - log_min_fold| <= d or m_r <= d.  Rows
                with more than one admissible answer are "undecided"; their share per case is at most UNDECIDED_CAP.
The mutants (kernel mistakes restated in numpy; tests/test_exact_consumers.py shows each outside the rule) are marked.
"""
import numpy

import _exact
from oracle import em_oracle

LD = _exact.LD
U = _exact.U
UNDECIDED_CAP = 0.01
SMALLEST_NORMAL = 2.0 ** -1022


def _ld(a):
    return numpy.asarray(a).astype(LD)


# ---------------------------------------------------------------- the reference
def exact_row_lse(M, ln_props):
    """logsumexp_h(ln_props[h] + M[r][h]) per row, long double; -inf for a row without a finite entry."""
    a = _ld(M) + _ld(ln_props)[None, :]
    m = a.max(axis=1)
    shift = numpy.where(numpy.isfinite(m), m, LD(0))
    with numpy.errstate(divide="ignore", invalid="ignore"):
        return shift + numpy.log(_exact._pairwise_sum(numpy.exp(a - shift[:, None]), axis=1))


def exact_posterior(M, ln_props, lse=None):
    """(ln_p + M) - lse_r; lse None: the exact normaliser (_exact.exact_posterior), else the caller's fp64 one."""
    if lse is None:
        return _exact.exact_posterior(M, ln_props)
    with numpy.errstate(invalid="ignore"):
        return (_ld(M) + _ld(ln_props)[None, :]) - _ld(lse)[:, None]


def _logaddexp_ld(a, b):
    hi, lo = numpy.maximum(a, b), numpy.minimum(a, b)
    with numpy.errstate(invalid="ignore", over="ignore"):
        out = hi + numpy.log1p(numpy.exp(lo - hi))
    return numpy.where(numpy.isneginf(hi), hi, out)        # (-inf, -inf): lo - hi is NaN


def exact_fold(blocks, delta=0.0):
    """logaddexp(...logaddexp(blocks[0], blocks[1])..., blocks[-1]) + delta: run order, long double, delta once."""
    acc = _ld(blocks[0])
    for blk in blocks[1:]:
        acc = _logaddexp_ld(acc, _ld(blk))
    return acc + LD(delta)


def exact_vote_values(M, ln_runs):
    """[R][H] long double: what best[r] is the argmax of.  ln_runs [B][H]."""
    ln_runs = numpy.atleast_2d(ln_runs)
    if len(ln_runs) == 1:
        return _ld(M) + _ld(ln_runs[0])[None, :]
    return exact_fold([_exact.exact_posterior(M, ln) for ln in ln_runs])


def top_two(V):
    """(column of the maximum, the maximum, the largest value of the OTHER columns) per row; one column: runner-up -inf."""
    V = numpy.asarray(V)
    idx = numpy.argmax(V, axis=1)
    rows = numpy.arange(len(V))
    v1 = V[rows, idx]
    if V.shape[1] < 2:
        return idx, v1, numpy.full(len(V), -numpy.inf, dtype=V.dtype)
    rest = numpy.array(V, copy=True)
    rest[rows, idx] = -numpy.inf
    return idx, v1, rest.max(axis=1)


def exact_assign_values(X, log_props):
    """v_c = X_c - log_props_c over the given columns (X [R][K], log_props [K]), long double."""
    return _ld(X) - _ld(log_props)[None, :]


def exact_labels(V, log_min_fold):
    """(label [R], margin [R]): label = the best column when v1 - v2 >= log_min_fold, else -1."""
    idx, v1, v2 = top_two(V)
    with numpy.errstate(invalid="ignore"):
        margin = v1 - v2
    return numpy.where(margin >= LD(log_min_fold), idx, -1), margin


def exact_log_normalize(T):
    T = _ld(T)
    with numpy.errstate(divide="ignore"):
        return numpy.log(T) - numpy.log(_exact._pairwise_sum(T, axis=0))


def exact_l1_exp_diff(a, b):
    """sum_h |exp(a_h) - exp(b_h)|, each term as exp(hi) * -expm1(lo - hi): the plain difference would cancel in long double
    too (a = 0 against the next fp64 number: 5e-324, not 0)."""
    a, b = _ld(a), _ld(b)
    hi, lo = numpy.maximum(a, b), numpy.minimum(a, b)
    with numpy.errstate(invalid="ignore"):
        terms = numpy.where(a == b, LD(0), numpy.exp(hi) * -numpy.expm1(lo - hi))
    return _exact._pairwise_sum(terms, axis=0)


# ---------------------------------------------------------------- the comparison passes: plain fp64
def cmp_row_lse(M, ln_props):
    with numpy.errstate(divide="ignore", invalid="ignore"):
        return em_oracle.logsumexp(numpy.asarray(M, dtype=numpy.float64) + numpy.asarray(ln_props, dtype=numpy.float64)[None, :], axis=1)


def cmp_posterior(M, ln_props, lse=None):
    a = numpy.asarray(M, dtype=numpy.float64) + numpy.asarray(ln_props, dtype=numpy.float64)[None, :]
    with numpy.errstate(invalid="ignore"):
        return a - (cmp_row_lse(M, ln_props) if lse is None else numpy.asarray(lse, dtype=numpy.float64))[:, None]


def cmp_fold(blocks, delta=0.0):
    acc = numpy.array(blocks[0], dtype=numpy.float64)
    for blk in blocks[1:]:
        acc = numpy.logaddexp(acc, numpy.asarray(blk, dtype=numpy.float64))
    return acc + delta


def cmp_vote_values(M, ln_runs):
    ln_runs = numpy.atleast_2d(ln_runs)
    if len(ln_runs) == 1:
        return numpy.asarray(M, dtype=numpy.float64) + ln_runs[0][None, :]
    return cmp_fold([cmp_posterior(M, ln) for ln in ln_runs])


def cmp_assign_values(X, log_props):
    return numpy.asarray(X, dtype=numpy.float64) - numpy.asarray(log_props, dtype=numpy.float64)[None, :]


def cmp_log_normalize(T):
    T = numpy.asarray(T, dtype=numpy.float64)
    with numpy.errstate(divide="ignore"):
        return numpy.log(T) - numpy.log(T.sum())


def cmp_l1_exp_diff(a, b):
    return numpy.abs(numpy.exp(numpy.asarray(a, dtype=numpy.float64)) - numpy.exp(numpy.asarray(b, dtype=numpy.float64))).sum()


# ---------------------------------------------------------------- restatements of the kernels' forms, and the mutants
LOG_REDO_BELOW = 2.0 ** -960


def fast_row_lse(M, ln_props, props, redo_below=LOG_REDO_BELOW):
    """The records kernels' normaliser in fp64 numpy: rowmax + log(sum_h props[h] exp(M - rowmax)), the row redone in log
    space (cmp_row_lse) where that sum is not finite or below `redo_below`.  redo_below = 0 is the MUTANT: the redo only
    at z == 0, which leaves the rows with a subnormal sum (a few mantissa bits) to the fast form."""
    M = numpy.asarray(M, dtype=numpy.float64)
    rowmax = M.max(axis=1)
    with numpy.errstate(invalid="ignore", divide="ignore", under="ignore"):
        z = (numpy.exp(M - rowmax[:, None]) * numpy.asarray(props, dtype=numpy.float64)[None, :]).sum(axis=1)
        fast = rowmax + numpy.log(z)
    redo = ~((z > 0 if redo_below == 0 else z >= redo_below) & (z < numpy.inf))
    return numpy.where(redo, cmp_row_lse(M, ln_props), fast), z


def mutant_fold_linear(blocks, delta=0.0):
    """MUTANT: the fold in linear space, log(exp a + exp b) without the shift."""
    acc = numpy.array(blocks[0], dtype=numpy.float64)
    with numpy.errstate(divide="ignore", under="ignore"):
        for blk in blocks[1:]:
            acc = numpy.log(numpy.exp(acc) + numpy.exp(numpy.asarray(blk, dtype=numpy.float64)))
    return acc + delta


def mutant_fold_delta_per_input(blocks, delta=0.0):
    """MUTANT: delta added once per input instead of once."""
    acc = numpy.array(blocks[0], dtype=numpy.float64)
    for blk in blocks[1:]:
        acc = numpy.logaddexp(acc, numpy.asarray(blk, dtype=numpy.float64)) + delta
    return acc


def labels_fp64(V, log_min_fold, runner_up_columns=None):
    """The assignment in fp64 on the values V [R][K].  runner_up_columns = K - 1 is the MUTANT that takes the runner-up
    from the first K - 1 columns only."""
    V = numpy.asarray(V, dtype=numpy.float64)
    idx, v1, v2 = top_two(V)
    if runner_up_columns is not None:
        rest = numpy.array(V[:, :runner_up_columns], copy=True)
        inside = idx < runner_up_columns
        rest[numpy.flatnonzero(inside), idx[inside]] = -numpy.inf
        v2 = rest.max(axis=1)
    with numpy.errstate(invalid="ignore"):
        return numpy.where((v1 - v2) >= log_min_fold, idx, -1)


def fast_posterior(M, ln_props, redo_below=LOG_REDO_BELOW):
    """(ln p + M) - fast_row_lse: the records posterior as the kernels form it (redo_below = 0: as they formed it)."""
    ln_props = numpy.asarray(ln_props, dtype=numpy.float64)
    lse, _ = fast_row_lse(M, ln_props, numpy.exp(ln_props), redo_below)
    with numpy.errstate(invalid="ignore"):
        return (numpy.asarray(M, dtype=numpy.float64) + ln_props[None, :]) - lse[:, None]


def strided_sum(x, lanes=1024):
    """A second honest sum, in the order of the one-workgroup vector kernels: lane t adds x[t], x[t + lanes], ... in turn,
    then the lanes are added as numpy adds them."""
    x = numpy.asarray(x, dtype=numpy.float64)
    pad = numpy.zeros(-len(x) % lanes)
    part = numpy.zeros(lanes)
    for chunk in numpy.concatenate([x, pad]).reshape(-1, lanes):
        part += chunk
    return part.sum()


def abs_exp_diff(a, b):
    """|exp(a) - exp(b)| term by term as mxm_l1_exp_diff forms it: exp(hi) * -expm1(lo - hi), no cancellation."""
    a, b = numpy.asarray(a, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    hi, lo = numpy.maximum(a, b), numpy.minimum(a, b)
    with numpy.errstate(invalid="ignore", under="ignore"):
        return numpy.where(a == b, 0.0, numpy.exp(hi) * -numpy.expm1(lo - hi))


def fold_by_hand(blocks, delta=0.0):
    """A second honest fold: hi + log1p(exp(lo - hi)) written out in fp64 (numpy.logaddexp is the comparison pass)."""
    acc = numpy.array(blocks[0], dtype=numpy.float64)
    for blk in blocks[1:]:
        hi, lo = numpy.maximum(acc, blk), numpy.minimum(acc, blk)
        with numpy.errstate(invalid="ignore"):
            acc = numpy.where(numpy.isneginf(hi), hi, hi + numpy.log1p(numpy.exp(lo - hi)))
    return acc + delta


def vote_reference(mat, ln_runs, fast=None):
    """(exact, comparison pass) values of the vote for ONE table of runs ln_runs [B][H]; fast = a redo threshold: the third
    return value is the kernels' own form restated (fast_posterior per run, folded by hand)."""
    exact, own = exact_vote_values(mat, ln_runs), cmp_vote_values(mat, ln_runs)
    if fast is None:
        return exact, own
    if len(ln_runs) == 1:
        return exact, own, numpy.asarray(mat, dtype=numpy.float64) + ln_runs[0][None, :]
    return exact, own, fold_by_hand([fast_posterior(mat, ln, fast) for ln in ln_runs])


def assign_samples_reference(M, sample_of, ncol, ln_theta, log_props, lse=None, delta=0.0):
    """The batched assignment's quantities for every row: M [R][ld], ln_theta [S][B][ld], log_props [S][ld], lse None (the
    normaliser over the sample's own columns) or [R][B] fp64.  -> (X, V) in long double and (X, V) of the comparison pass,
    each [R][ld] with -inf in the pad columns: X_c = fold_b((ln_theta_b,c + M_rc) - L_b) + delta, V_c = X_c - log_props_c."""
    n_rows, ld = M.shape
    out = [numpy.full((n_rows, ld), -numpy.inf, dtype=t) for t in (LD, LD, numpy.float64, numpy.float64)]
    for s in range(len(ncol)):
        idx = numpy.flatnonzero(sample_of == s)
        k, runs = int(ncol[s]), range(ln_theta.shape[1])
        sub = numpy.ascontiguousarray(M[idx, :k])
        given = [None if lse is None else lse[idx, b] for b in runs]
        X = exact_fold([exact_posterior(sub, ln_theta[s, b, :k], given[b]) for b in runs], delta)
        Xc = cmp_fold([cmp_posterior(sub, ln_theta[s, b, :k], given[b]) for b in runs], delta)
        out[0][idx, :k], out[1][idx, :k] = X, exact_assign_values(X, log_props[s, :k])
        out[2][idx, :k], out[3][idx, :k] = Xc, cmp_assign_values(Xc, log_props[s, :k])
    return out


# ---------------------------------------------------------------- the rule
def value_errors(got, exact, own):
    """-> (got's largest error, the comparison pass's, the bound) over the entries whose exact value is finite, after the
    check that got has the reference's pattern of -inf / NaN.  The comparison pass `own` is held to the pattern too."""
    exact = numpy.asarray(exact)
    e64 = exact.astype(numpy.float64)
    finite = numpy.isfinite(e64)
    for name, arr in (("the kernel's", got), ("the comparison pass's", own)):
        arr = numpy.asarray(arr, dtype=numpy.float64)
        assert arr.shape == e64.shape, (name, arr.shape, e64.shape)
        assert numpy.array_equal(numpy.isfinite(arr), finite), "%s finite entries are not the reference's" % name
        assert numpy.array_equal(numpy.isnan(arr), numpy.isnan(e64)), "%s NaNs are not the reference's" % name
        assert numpy.array_equal(numpy.isneginf(arr), numpy.isneginf(e64)), "%s -inf entries are not the reference's" % name
    if not finite.any():
        return 0.0, 0.0, _exact.abs_bound(0.0, e64)
    with numpy.errstate(invalid="ignore"):                 # (-inf - -inf outside `finite`)
        err = float(numpy.abs(_ld(got) - exact)[finite].max())
        mine = float(numpy.abs(_ld(own) - exact)[finite].max())
    return err, mine, _exact.abs_bound(mine, e64)


def inside(got, exact, own):
    """True / False for the value rule (a broken pattern counts as outside): what the mutant tests ask."""
    try:
        err, _, bound = value_errors(got, exact, own)
    except AssertionError:
        return False
    return err <= bound


def undecided_best(V_exact, d):
    """Rows in which a second column lies within d of the exact row maximum (or the row has no maximum: NaN / all -inf)."""
    _, v1, v2 = top_two(numpy.asarray(V_exact))
    with numpy.errstate(invalid="ignore"):
        return ~((v1 - v2) > LD(d))


def check_best(best, V_exact, d):
    """best[r] is a column whose exact value is within d of the exact row maximum -> the undecided rows (bool [R])."""
    V_exact = numpy.asarray(V_exact)
    best = numpy.asarray(best).astype(numpy.int64)
    assert best.shape == (len(V_exact),) and (best >= 0).all() and (best < V_exact.shape[1]).all(), "best outside 0 .. H - 1"
    rowmax = V_exact.max(axis=1)
    mine = V_exact[numpy.arange(len(V_exact)), best]
    decided = numpy.isfinite(rowmax.astype(numpy.float64))
    bad = numpy.flatnonzero(decided & ~(mine >= rowmax - LD(d)))
    assert len(bad) == 0, "rows %s: best is not within d = %.3g of the exact row maximum" % (bad[:8], d)
    return undecided_best(V_exact, d)


def undecided_labels(margin, log_min_fold, d):
    with numpy.errstate(invalid="ignore"):
        return ~((numpy.abs(margin - LD(log_min_fold)) > LD(d)) & (margin > LD(d)))


def check_labels(assigned, V_exact, log_min_fold, d):
    """assigned[r] (a column of V_exact, or -1) equals the exact label on every decided row -> the undecided rows."""
    want, margin = exact_labels(V_exact, log_min_fold)
    undecided = undecided_labels(margin, log_min_fold, d)
    bad = numpy.flatnonzero(~undecided & (numpy.asarray(assigned).astype(numpy.int64) != want))
    assert len(bad) == 0, "rows %s: assigned %s, exact %s, margins %s, log_min_fold %.17g, d %.3g" % (
        bad[:8], numpy.asarray(assigned)[bad[:8]], want[bad[:8]], margin[bad[:8]].astype(numpy.float64), log_min_fold, d)
    return undecided


def within_cap(undecided):
    return float(numpy.mean(undecided)) <= UNDECIDED_CAP if len(undecided) else True


def exact_votes(best, weights, n_haps):
    """(votes [H] as exact integers, counts [H], first-seen row [H] with R for "none") from the device's own best."""
    best = numpy.asarray(best).astype(numpy.int64)
    w = numpy.asarray(weights)
    assert numpy.array_equal(w, numpy.round(w)), "integer weights only: the sums are then exact in any order"
    votes = numpy.zeros(n_haps, dtype=numpy.int64)
    numpy.add.at(votes, best, w.astype(numpy.int64))
    counts = numpy.bincount(best, minlength=n_haps).astype(numpy.int64)
    first = numpy.full(n_haps, len(best), dtype=numpy.int64)
    numpy.minimum.at(first, best, numpy.arange(len(best), dtype=numpy.int64))
    return votes, counts, first
