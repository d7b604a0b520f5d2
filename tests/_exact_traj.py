"""
Extended-precision reference of an EM LOOP: K passes of tests/_exact.py chained through the LOG state, CPU only, no device
code and no use of the library.  What tests/_exact.py is to one pass, this is to what a loop carries from iteration k to
k + 1 (the log proportions, the linear proportions derived from them, the reported l1).

    exact_trajectory(X, ln0, w, K)     long double: ln_k, l1_k = sum_h |exp(ln_k) - exp(ln_{k-1})| and T_k for k = 1 .. K,
                                       from exact_colsum (X = P, the linearised matrix as the device holds it) or
                                       exact_colsum_log (X = M, log_space = True) and exact_finalize; p = exp(ln) is taken
                                       in long double, whose exponent range keeps e^-800 (and e^-11000) a normal number:
                                       the reference never underflows, it IS the log-space recurrence
    seq_trajectory(P, ln0, w, K)       the comparison pass: the same recurrence in plain fp64 (seq_colsum, a log state,
                                       p = exp(ln) per iteration); `mutant` selects one of three subtly wrong carries
    oracle_trajectory(M, ln0, w, K)    the comparison pass of the log-space forms: K steps of oracle.em_oracle.em_step

props0 (optional) are the linear proportions the FIRST pass reads, where a caller hands the kernel both arrays (props_cur
and ln_cur): reference and kernel then start from the same bits; from the second pass on p = exp(ln).

The rule (u = 2^-53; the maximum over the entries whose exact value is finite):

    max_h |ln_K - ln_exact,K|  <=  8 * max(err_seq(K), K * u * max(1, max_h |ln_exact,K|))             ln_bound
    |l1 - l1_exact,K|          <=  8 * max(the comparison pass's own l1 error, K * u * max |ln| + H * u)   l1_bound

K * u * max |ln|: every step adds two logarithms to ln and rounds the sum to a number of size |ln| (u |ln| per step); an
error d in ln_h is a relative error d of p_h, which moves Z_r by less than d and T -- hence the next ln -- by less than d
again (all terms are positive), so the errors of K steps add, they do not multiply.  H * u: the l1 sum of H terms of total
size <= 2.

deep_precondition(P, ln) replaces _exact.check_products where proportions are subnormal or zero in fp64: per row, the
products p_h P_rh below 2^-1000 sum to less than 2^-60 Z_r, i.e. what fp64 loses to gradual underflow is far below one
rounding of Z_r, and the existing bound on T stands.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy

import _exact
from _exact import LD, U

_POOL = ThreadPoolExecutor(max_workers=8)             # (numpy's long-double loops release the GIL)
ROW_BLOCK = 128


def _colsum(P, p, w):
    """exact_colsum; from 256 rows on over blocks of 128 rows side by side: Z_r belongs to its row alone, so T is the
    (pairwise, long-double) sum of the blocks' own T."""
    if P.shape[0] < 2 * ROW_BLOCK:
        return _exact.exact_colsum(P, p, w)
    w = numpy.asarray(w)
    parts = list(_POOL.map(lambda a: _exact.exact_colsum(P[a:a + ROW_BLOCK], p, w[a:a + ROW_BLOCK]), range(0, P.shape[0], ROW_BLOCK)))
    return _exact._pairwise_sum(numpy.stack(parts), axis=0)


MUTANTS =("carry_fp32", "last_not_renormalised", "last_log_lags")


class Trajectory(object):
    """ln[k], l1[k], T[k] for k = 0 .. K (entry 0: the start; l1[0] and T[0] are NaN)."""

    def __init__(self, ln0, n_steps, dtype):
        n_haps = len(ln0)
        self.ln = numpy.empty((n_steps + 1, n_haps), dtype=dtype)
        self.T = numpy.full((n_steps + 1, n_haps), numpy.nan, dtype=dtype)
        self.l1 = numpy.full(n_steps + 1, numpy.nan, dtype=dtype)
        self.ln[0] = ln0
        self.K = n_steps


def exact_trajectory(X, ln0, w, K, props0=None, log_space=False):
    """log_space: X = M.  Long double holds exp(M - rowmax) * exp(ln p) down to e^-11000 as a normal number, so the
    log-space pass is exact_colsum over E = exp(M - rowmax) taken ONCE in long double (the row shift cancels in T) -- the
    same T as exact_colsum_log's to long-double rounding, K times cheaper in exponentials; its first step is checked against
    exact_colsum_log itself in tests/test_exact_traj.py."""
    traj = Trajectory(numpy.asarray(ln0).astype(LD), K, LD)
    X = numpy.asarray(X)
    if log_space:
        rowmax = X.max(axis=1, keepdims=True)
        X = numpy.exp(X.astype(LD) - numpy.where(numpy.isfinite(rowmax), rowmax, 0.0).astype(LD))
        assert props0 is None
    else:
        X = X.astype(LD)                               # (once, not per step)
    p = numpy.exp(traj.ln[0]) if props0 is None else numpy.asarray(props0).astype(LD)
    for k in range(1, K + 1):
        T = _colsum(X, p, w)
        traj.T[k] = T
        traj.ln[k] = _exact.exact_finalize(T, traj.ln[k - 1], p)
        p_new = numpy.exp(traj.ln[k])
        traj.l1[k] = _exact._pairwise_sum(numpy.abs(p_new - p), axis=0)
        p = p_new
    return traj


def seq_trajectory(P, ln0, w, K, props0=None, mutant=None, colsum=_exact.seq_colsum):
    """
    Plain fp64: T = seq_colsum(P, p, w), tot = sum_h p_h T_h in sequential order, ln += log T - log tot, p = exp(ln).
    colsum = _exact.pairwise_colsum makes the second honest pass of tests/test_exact_traj.py.
    The three MUTANTS of tests/test_exact_traj.py (none of them is the comparison pass) carry something wrong from
    iteration k to k + 1, which is why each is right at K = 1:
      "carry_fp32"             p carried as p * T / tot, rounded to fp32, instead of exp(ln)
      "last_not_renormalised"  p carried as p * T / tot, the last column's as p * T
      "last_log_lags"          column H - 1 of the log state receives the PREVIOUS iteration's increment (none at k = 1 ...
                               where the right one is used: the first step has nothing to lag behind)
    """
    assert mutant is None or mutant in MUTANTS
    P = numpy.asarray(P)
    w = numpy.asarray(w, dtype=numpy.float64)
    traj = Trajectory(numpy.asarray(ln0, dtype=numpy.float64), K, numpy.float64)
    p = numpy.exp(traj.ln[0]) if props0 is None else numpy.asarray(props0, dtype=numpy.float64).copy()
    lag = None
    for k in range(1, K + 1):
        with numpy.errstate(divide="ignore", invalid="ignore", over="ignore"):
            T = colsum(P, p, w)
            tot = 0.0
            for term in p * T:
                tot += term
            step = numpy.log(T) - numpy.log(tot)
            if mutant == "last_log_lags":
                step[-1], lag = (step[-1] if lag is None else lag), step[-1]
            traj.T[k] = T
            traj.ln[k] = traj.ln[k - 1] + step
            p_new = numpy.exp(traj.ln[k])
            traj.l1[k] = numpy.abs(p_new - p).sum()
            if mutant == "carry_fp32":
                p_new = (p * T / tot).astype(numpy.float32).astype(numpy.float64)
            elif mutant == "last_not_renormalised":
                p_new = p * T / tot
                p_new[-1] = p[-1] * T[-1]
        p = p_new
    return traj


def oracle_trajectory(M, ln0, w, K):
    """K steps of oracle.em_oracle.em_step (fp64, log space); T_k recovered as sum_r w_r exp(post_rh - ln p_h)."""
    from oracle import em_oracle
    M = numpy.asarray(M)
    w = numpy.asarray(w, dtype=numpy.float64)
    traj = Trajectory(numpy.asarray(ln0, dtype=numpy.float64), K, numpy.float64)
    buf = numpy.empty_like(M)
    for k in range(1, K + 1):
        ln = traj.ln[k - 1]
        post, theta = em_oracle.em_step(M, w, ln, buf)
        traj.T[k] = (numpy.exp(post - ln[None, :]) * w[:, None]).sum(axis=0)
        traj.ln[k] = theta
        traj.l1[k] = numpy.abs(numpy.exp(theta) - numpy.exp(ln)).sum()
    return traj


# ---------------------------------------------------------------- the rule
def _finite(exact_ln):
    return numpy.isfinite(numpy.asarray(exact_ln).astype(numpy.float64))


def ln_error(got, exact_ln):
    """max_h |got_h - exact_h| where the exact value is finite; inf if `got` is not finite there."""
    ok = _finite(exact_ln)
    got = numpy.asarray(got)
    if not ok.any() or not numpy.isfinite(got[ok].astype(numpy.float64)).all():
        return float("inf")
    return float(numpy.abs(got.astype(LD) - numpy.asarray(exact_ln).astype(LD))[ok].max())


def ln_floor(exact_ln, k):
    """K * u * max(1, max |ln_exact,K|) -- the 1: p = exp(ln) is itself rounded, a relative error u of every proportion and
    so an absolute u in the next log, whatever the size of ln (it decides where max |ln| < 1 only: a single column)."""
    ok = _finite(exact_ln)
    return k * U * max(1.0, float(numpy.abs(numpy.asarray(exact_ln).astype(numpy.float64)[ok]).max()))


def ln_bound(err_seq, exact_ln, k):
    return _exact.TIGHT_MARGIN * max(float(err_seq), ln_floor(exact_ln, k))


def l1_bound(l1_err_seq, exact_ln, k):
    return _exact.TIGHT_MARGIN * max(float(l1_err_seq), ln_floor(exact_ln, k) + len(exact_ln) * U)


def seq_errors(exact, seq, k):
    """(the comparison pass's ln error, its l1 error) against the trajectory at step k."""
    return ln_error(seq.ln[k], exact.ln[k]), abs(float(LD(seq.l1[k]) - exact.l1[k]))


def inside_rule(got_ln, exact, seq, k):
    """-> (inside?, error, bound) of a state `got_ln` claimed to be ln_k."""
    err = ln_error(got_ln, exact.ln[k])
    bound = ln_bound(seq_errors(exact, seq, k)[0], exact.ln[k], k)
    return err <= bound, err, bound


# ---------------------------------------------------------------- the stop decision, from the reference
GAP = 1.5
TOL_MIN = 1e-9                                         # a tol the l1 bound itself (8 (K u max |ln| + H u) ~ 1e-11 at most here)
                                                       # reaches decides nothing: fp64's l1 of H terms does not fall below H u


def stop_point(l1, k_min=3):
    """
    (K*, tol) for `l1[0 .. K]` (entry 0 unused).  An iteration k is a USABLE stop if min_{j<k} l1_j > 1.5 l1_k (l1 is not
    monotone, and where it falls by a few per cent per iteration no tolerance separates two neighbours by that much);
    K* = the first usable k >= k_min (the carry taken with state that was itself carried), failing that the first
    usable k >= 2; tol = the geometric mean of l1_{K*} and that minimum -- a loop whose l1 is right to within a factor
    1.2 stops exactly there.  (None, None) when no iteration is usable.
    """
    l1 = numpy.asarray(l1).astype(numpy.float64)
    usable = [k for k in range(2, len(l1)) if float(l1[1:k].min()) > GAP * l1[k] and l1[k] * l1[1:k].min() >= TOL_MIN ** 2]
    if not usable:
        return None, None
    k = next((k for k in usable if k >= k_min), usable[0])
    return k, float(numpy.sqrt(l1[k] * l1[1:k].min()))


def stops_at(l1, tol):
    """The first k with l1_k < tol (None if there is none) and the margin of that decision: the smallest ratio by which an
    l1 on the way misses tol, on either side."""
    l1 = numpy.asarray(l1).astype(numpy.float64)
    for k in range(1, len(l1)):
        if l1[k] < tol:
            margin = min([tol / l1[k]] + [float(v) / tol for v in l1[1:k]])
            return k, margin
    return None, 0.0


def common_tol(l1_lists, k_min=2):
    """
    One tol for several restarts whose l1 are given up to max_iter = len - 1: restart b stops (done = 1) at the first k with
    l1_k < tol, or runs to max_iter (done = 2).  Every l1 on every restart's way misses tol by a factor sqrt(1.5) at least
    (stop_point's gap, split evenly over the two sides), every stop is at k_min or later, and the restarts end at as many
    DIFFERENT iterations as any tol allows (ties: the widest margin).  -> tol, [(iterations, done)].
    Candidates: every l1 value times and over sqrt(1.5) -- the ends of the intervals a tol is allowed in -- and the
    geometric means between neighbours of those.
    """
    values = numpy.concatenate([numpy.asarray(l).astype(numpy.float64)[1:] for l in l1_lists])
    values = values[values > 0]
    edges = numpy.sort(numpy.concatenate([values * numpy.sqrt(GAP), values / numpy.sqrt(GAP)]))
    best = None
    for tol in numpy.concatenate([numpy.sqrt(edges[:-1] * edges[1:]), edges * (1 + 1e-9), edges * (1 - 1e-9)]):
        ends, margin = [], float("inf")
        for l1 in l1_lists:
            l1 = numpy.asarray(l1).astype(numpy.float64)
            k, m = stops_at(l1, tol)
            if k is None:
                k, m, done = len(l1) - 1, float(l1[1:].min()) / tol, 2
            else:
                done = 1
            ends.append((k, done))
            margin = min(margin, m)
        if tol < TOL_MIN or margin < numpy.sqrt(GAP) * (1 + 1e-10) or min(k for k, _ in ends) < k_min:
            continue
        score = (len(set(k for k, _ in ends)), margin)
        if best is None or score > best[0]:
            best = (score, float(tol), ends)
    assert best is not None, "no tolerance separates the restarts' stops"
    return best[1], best[2]


# ---------------------------------------------------------------- the precondition of the "deep" vector
def deep_precondition(P, ln):
    """Per row: the products p_h P_rh below 2^-1000 sum to less than 2^-60 Z_r (long double).  -> min_r Z_r."""
    prod = numpy.asarray(P).astype(LD) * numpy.exp(numpy.asarray(ln).astype(LD))[None, :]
    z = _exact._pairwise_sum(prod, axis=1)
    lost = _exact._pairwise_sum(numpy.where(prod < LD(_exact.MIN_PRODUCT), prod, LD(0)), axis=1)
    assert (z > 0).all() and (lost < LD(2.0) ** -60 * z).all(), "underflowing products carry weight in some row's Z"
    return float(z.min())
