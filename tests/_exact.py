"""
Extended-precision reference of one EM pass -- plain numpy in numpy.longdouble (x87: 64 mantissa bits, 2^11 times finer
than fp64), CPU only, no device code and no use of the library.  The inputs are the BITS the kernel under test reads (the
fp64 / fp32 linearised matrix as the device holds it, the fp64 proportions, the fp64 weights), so reference and kernel start
from identical numbers and every difference is the kernel's own rounding.

    exact_colsum(P, props, w)          T[B][H] of the linear forms:  Z_r = sum_h p_h P_rh,  T_h = sum_r (w_r / Z_r) P_rh
    exact_colsum_log(M, ln_props, w)   the same T from the log matrix (the log-space kernels: H <= 64, H > 8192)
    exact_finalize(T, ln_cur, props)   ln_new = ln_cur + log T - log sum_h props T
    exact_posterior(M, ln_props)       (ln_p + M) - logsumexp_h(ln_p + M)
    seq_colsum(P, props, w)            the comparison pass in fp64, least favourable (sequential) order
    check_products(P, props)           every non-zero p_h P_rh >= 2^-1000: no gradual underflow inside the bound

The bound (one rule for every form, u = 2^-53, rel(X) = max_h |X_h - T_h| / T_h; all terms are non-negative, so the sums
are perfectly conditioned):

    rel(T_gpu) <= 8 * max(rel(T_seq), 4u)      tight_bound    (T_seq: seq_colsum on the same inputs)
    rel(T_gpu) <= (R + H + 8) * u              derived_bound  (H products and H - 1 additions in Z, one division, one
                                                               product with w, one product and R - 1 additions in T:
                                                               first-order worst case of ANY summation order)

The sums here are pairwise in long double: at most log2(5408) + log2(700) + 4 < 30 roundings of 2^-64 each, 0.015 u.
"""
import numpy
import pytest

LD = numpy.longdouble
if numpy.finfo(LD).nmant < 63:                       # (pytest collects nothing from a helper module: the skip reaches the
    pytest.skip("numpy.longdouble is not wider than fp64 here", allow_module_level=True)   # importing test module)
assert numpy.finfo(LD).nmant >= 63

U = 2.0 ** -53
TIGHT_MARGIN = 8.0
TERM_FLOOR = 4.0 * U                                 # the four roundings of a single term (matters for H <= 2 only)
MIN_PRODUCT = 2.0 ** -1000


def _pairwise_sum(a, axis):
    """Sum along `axis` by halving (log2(n) roundings per result, whatever numpy's own reduction does on that axis)."""
    a = numpy.moveaxis(a, axis, 0)
    while a.shape[0] > 1:
        half = a.shape[0] // 2
        head = a[:half] + a[half:2 * half]
        a = head if a.shape[0] == 2 * half else numpy.concatenate([head, a[2 * half:]], axis=0)
    return a[0]


def _props2d(props):
    props = numpy.asarray(props)
    return props.reshape(1, -1) if props.ndim == 1 else props


def exact_colsum(P, props, w):
    """T[B][H] (long double) from the linearised matrix P[R][H] (fp64 or fp32 bits), props[B][H] or [H], w[R]."""
    P = numpy.asarray(P).astype(LD, copy=False)         # (a long-double matrix is taken as it is: the trajectory's K passes)
    w = numpy.asarray(w).astype(LD)
    p2 = _props2d(props)
    out = numpy.empty((p2.shape[0], P.shape[1]), dtype=LD)
    for b in range(p2.shape[0]):
        z = _pairwise_sum(P * p2[b].astype(LD)[None, :], axis=1)
        with numpy.errstate(divide="ignore", invalid="ignore"):
            c = w / z
        out[b] = _pairwise_sum(P * c[:, None], axis=0)
    return out if numpy.asarray(props).ndim == 2 else out[0]


def exact_colsum_log(M, ln_props, w):
    """The same T from the log matrix: exp(ln_p + M - shift) in long double, shift = the row maximum of ln_p + M."""
    M = numpy.asarray(M).astype(LD)
    w = numpy.asarray(w).astype(LD)
    l2 = _props2d(ln_props)
    out = numpy.empty((l2.shape[0], M.shape[1]), dtype=LD)
    for b in range(l2.shape[0]):
        a = M + l2[b].astype(LD)[None, :]
        shift = a.max(axis=1, keepdims=True)
        e = numpy.exp(a - shift)
        z = _pairwise_sum(e, axis=1)
        # exp(M - shift) = e / p: one long-double exp per cell instead of two
        out[b] = _pairwise_sum(e * (w / z)[:, None], axis=0) * numpy.exp(-l2[b].astype(LD))
    return out if numpy.asarray(ln_props).ndim == 2 else out[0]


def exact_finalize(T, ln_cur, props_cur):
    """ln_new = ln_cur + log T - log sum_h props_cur T (long double; -inf where T == 0)."""
    T = numpy.asarray(T).astype(LD)
    tot = _pairwise_sum(numpy.asarray(props_cur).astype(LD) * T, axis=-1)
    with numpy.errstate(divide="ignore"):
        return numpy.asarray(ln_cur).astype(LD) + numpy.log(T) - numpy.log(tot)[..., None]


def exact_posterior(M, ln_props):
    """(ln_p + M) - logsumexp_h(ln_p + M), long double."""
    a = numpy.asarray(M).astype(LD) + numpy.asarray(ln_props).astype(LD)[None, :]
    shift = a.max(axis=1, keepdims=True)
    lse = shift + numpy.log(_pairwise_sum(numpy.exp(a - shift), axis=1))[:, None]
    return a - lse


def seq_colsum(P, props, w, recip=None, skip_last=False, acc=numpy.float64):
    """
    The comparison pass, fp64 throughout: Z accumulated column by column, T row by row, no pairwise summation -- the
    error a plain fp64 implementation has in the least favourable order.  The keyword arguments make the three MUTANTS of
    tests/test_exact_ref.py (none of them is the comparison pass): recip = a dtype the reciprocal of Z is rounded to,
    skip_last = the last column left out of Z, acc = the type T is accumulated in.
    """
    P = numpy.asarray(P).astype(numpy.float64)
    props = numpy.asarray(props, dtype=numpy.float64)
    w = numpy.asarray(w, dtype=numpy.float64)
    n_rows, n_haps = P.shape
    z = numpy.zeros(n_rows)
    for h in range(n_haps - (1 if skip_last else 0)):
        z += props[h] * P[:, h]
    with numpy.errstate(divide="ignore", invalid="ignore"):
        c = w / z if recip is None else w * (1.0 / z).astype(recip).astype(numpy.float64)
    t = numpy.zeros(n_haps, dtype=acc)
    for r in range(n_rows):
        t += (c[r] * P[r]).astype(acc)
    return t.astype(numpy.float64)


def pairwise_colsum(P, props, w):
    """What numpy does by itself in fp64 (blocked / pairwise reductions): the second accepted pass of test_exact_ref."""
    P = numpy.asarray(P).astype(numpy.float64)
    z = (P * numpy.asarray(props, dtype=numpy.float64)[None, :]).sum(axis=1)
    return (P * (numpy.asarray(w, dtype=numpy.float64) / z)[:, None]).sum(axis=0)


def check_products(P, props):
    """Every non-zero p_h P_rh is a normal number with room to spare; returns the smallest one."""
    prod = numpy.asarray(P).astype(numpy.float64) * numpy.asarray(props, dtype=numpy.float64)[None, :]
    nz = prod[prod > 0]
    smallest = float(nz.min()) if nz.size else float("inf")
    assert smallest >= MIN_PRODUCT, "a product p_h * P_rh of %.3g would underflow gradually" % smallest
    return smallest


def rel_err(T, T_exact):
    """max_h |T_h - T_exact,h| / T_exact,h as a float (inf when a sum is not finite or a zero column is not zero)."""
    T = numpy.asarray(T).astype(LD)
    T_exact = numpy.asarray(T_exact).astype(LD)
    if not numpy.isfinite(T).all():
        return float("inf")
    zero = T_exact == 0
    if (T[zero] != 0).any():
        return float("inf")
    if zero.all():
        return 0.0
    return float((numpy.abs(T - T_exact)[~zero] / T_exact[~zero]).max())


def tight_bound(rel_seq):
    return TIGHT_MARGIN * max(rel_seq, TERM_FLOOR)


def derived_bound(n_rows, n_haps):
    return (n_rows + n_haps + 8) * U


def abs_bound(oracle_err, values):
    """Posterior and ln_new: 8 x max(the fp64 oracle's own largest error, u x max |value|), absolute."""
    finite = numpy.asarray(values)[numpy.isfinite(numpy.asarray(values, dtype=numpy.float64))]
    big = float(numpy.abs(finite).max()) if finite.size else 0.0
    return TIGHT_MARGIN * max(float(oracle_err), U * big)


def ulp_err(got, want_ld):
    """|got - want| in units of the last place of `want` rounded to got's type, maximum over the array."""
    got = numpy.asarray(got)
    want_ld = numpy.asarray(want_ld).astype(LD)
    near = want_ld.astype(got.dtype)
    spacing = numpy.spacing(numpy.abs(near)).astype(LD)
    ok = numpy.isfinite(near) & (near != 0)
    if not ok.any():
        return 0.0
    return float((numpy.abs(got.astype(LD) - want_ld)[ok] / spacing[ok]).max())
