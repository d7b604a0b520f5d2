"""
Plain-numpy references for the contributor-support entries (include/mixemt_hip_support.h; assign.support_many), shared by
test_support_host.py and the GPU tests.  CPU only: no device code and no use of the library.
    subset_em      the refinement EM over a subset of the columns in fp64, in the loop's order of operations (linearise with
                   the shift over the masked-in columns, z, w / z, column sums, log update, l1 against the tolerance)
    exact_loglik   sum_r w_r log sum_{k in mask} p_k exp(M_rk) in numpy.longdouble with pairwise sums (tests/_exact.py)
    seq_loglik     the same formula -- the entry's, with its log-space redo -- in sequential fp64
    lrt_p / bic / aic   the statistics restated
"""
import math

import numpy

import _exact as ex

LD = ex.LD
LINEAR_MIN = 2.0 ** -960                # MXM_LSE_LINEAR_MIN (csrc/common.hpp)


def mask_columns(mask):
    return [k for k in range(32) if (int(mask) >> k) & 1]


def subset_em(M, w, mask, start, tol, max_iter):
    """-> (ln_cur, ln_new, iters, done) over the masked-in columns, in ascending column order; start: linear, one value per
    masked-in column."""
    cols = mask_columns(mask)
    x = numpy.asarray(M, dtype=numpy.float64)[:, cols]
    w = numpy.ones(x.shape[0]) if w is None else numpy.asarray(w, dtype=numpy.float64)
    m = x.max(axis=1, keepdims=True)
    with numpy.errstate(invalid="ignore"):
        e = numpy.exp(x - numpy.where(numpy.isfinite(m), m, 0.0))
    with numpy.errstate(divide="ignore"):
        lc = numpy.log(numpy.asarray(start, dtype=numpy.float64))
    p = numpy.exp(lc)
    ln_next, iters, done = lc.copy(), 0, 0
    while done == 0:
        z = numpy.zeros(x.shape[0])
        for k in range(len(cols)):
            z += p[k] * e[:, k]
        with numpy.errstate(divide="ignore", invalid="ignore"):
            c = numpy.where(z > 0, w / z, numpy.where(w != 0, numpy.nan, 0.0))
        T = (c[:, None] * e).sum(axis=0)
        tot = float((p * T).sum())
        with numpy.errstate(divide="ignore"):
            ln_next = lc + numpy.log(T) - math.log(tot)
        pn = numpy.exp(ln_next)
        l1 = float(numpy.abs(pn - p).sum())
        iters += 1
        done = 1 if l1 < tol else (2 if iters >= max_iter else 0)
        if done == 0:
            lc, p = ln_next, pn
    return lc, ln_next, iters, done


def exact_loglik(M, ln_props, w, mask):
    """The log-likelihood in long double from the BITS the kernel reads: M [R][ld], ln_props [ld], w [R] or None."""
    cols = mask_columns(mask)
    a = numpy.asarray(M)[:, cols].astype(LD) + numpy.asarray(ln_props)[cols].astype(LD)[None, :]
    w = numpy.ones(a.shape[0], dtype=LD) if w is None else numpy.asarray(w).astype(LD)
    keep = w != 0
    a, w = a[keep], w[keep]
    if a.shape[0] == 0:
        return LD(0.0)
    shift = a.max(axis=1)
    if numpy.isneginf(shift).any():
        return LD(-numpy.inf)
    lse = shift + numpy.log(ex._pairwise_sum(numpy.exp(a - shift[:, None]), axis=1))
    return ex._pairwise_sum(w * lse, axis=0)


def seq_loglik(M, ln_props, w, mask):
    """The entry's formula in fp64, every sum sequential: per row m = the maximum of M over the mask, z = sum p_k exp(M - m)
    column after column, m + log z -- or, where z is below 2^-960 or not finite, log sum exp(ln p_k + M - its maximum) + that
    maximum -- and ll += w_r x that, row after row."""
    cols = mask_columns(mask)
    x = numpy.asarray(M, dtype=numpy.float64)[:, cols]
    lnp = numpy.asarray(ln_props, dtype=numpy.float64)[cols]
    p = numpy.exp(lnp)
    w = numpy.ones(x.shape[0]) if w is None else numpy.asarray(w, dtype=numpy.float64)
    total = 0.0
    for r in range(x.shape[0]):
        if w[r] == 0:
            continue
        m = x[r].max()
        shift = m if numpy.isfinite(m) else 0.0
        z = 0.0
        for k in range(len(cols)):
            z += p[k] * math.exp(x[r, k] - shift) if x[r, k] > -numpy.inf else 0.0
        if z >= LINEAR_MIN and z < numpy.inf:
            term = shift + math.log(z)
        else:
            a = lnp + x[r]
            mm = a.max()
            if not numpy.isfinite(mm):
                return -numpy.inf
            s = 0.0
            for k in range(len(cols)):
                s += math.exp(a[k] - mm) if a[k] > -numpy.inf else 0.0
            term = math.log(s) + mm
        total += w[r] * term
    return total


def rel_ll(got, exact):
    """|got - exact| / |exact| as a float (inf when got is not finite)."""
    if not numpy.isfinite(got):
        return float("inf")
    return float(abs(LD(got) - exact) / abs(exact))


def lrt_p(lrt):
    """1/2 erfc(sqrt(max(lrt, 0) / 2)): the upper tail of 1/2 chi2_0 + 1/2 chi2_1."""
    return 0.5 * math.erfc(math.sqrt(max(lrt, 0.0) / 2.0))


def bic(ll, n_columns, n_eff):
    return -2.0 * ll + ((n_columns - 1) * math.log(n_eff) if n_columns > 1 else 0.0)


def aic(ll, n_columns):
    return -2.0 * ll + 2.0 * (n_columns - 1)
