"""
The trajectory reference (tests/_exact_traj.py) catches what it is for, on every (matrix, vector, K) of
tests/test_gpu_accuracy_loops.py -- CPU only:
  * at K = 1 it IS the one-pass reference, to the bit;
  * two honest fp64 loops, the sequential comparison pass and one over numpy's pairwise sums, are inside the rule at every K
    (the rule is satisfiable by the reference alone), l1 included; so is the fp64 oracle on the log-space widths;
  * three loops whose CARRY is subtly wrong are right at K = 1 and outside the rule at K = 3 -- the K each first fails at is
    asserted;
  * the "deep" vector is what its docstring says: subnormal and zero proportions, more of them crossing while the loop
    runs, no weight lost to underflow (deep_precondition), no zero sum;
  * the stop decision taken from the reference has the margin the GPU module relies on.
"""
import numpy
import pytest

import _accuracy_inputs as inputs
import _exact
import _exact_traj as traj

K_MAX = max(inputs.LOOP_STEPS)
FIRST_FAILURE = {"carry_fp32": 2, "last_not_renormalised": 2, "last_log_lags": 2}
NO_USABLE_STOP = {(66, "dirichlet"), (1025, "dirichlet"), (5408, "dirichlet"), (5408, "skewed")}


@pytest.fixture(scope="module")
def linear_cases(b17):
    """(label, vector, P, w, props, ln, exact trajectory, comparison pass) at the real widths, made once."""
    out = []
    for n_haps in inputs.LOOP_WIDTHS_REAL:
        label, mat, wts = inputs.loop_matrix(b17, n_haps)
        lin = inputs.linearise(mat)
        for vec, (props, ln) in inputs.loop_vectors(n_haps).items():
            exact = traj.exact_trajectory(lin, ln, wts, K_MAX, props0=props)
            seq = traj.seq_trajectory(lin, ln, wts, K_MAX, props0=props)
            out.append((label, vec, lin, wts, props, ln, exact, seq))
    return out


def test_one_step_is_the_one_pass_reference_to_the_bit(linear_cases):
    for label, vec, lin, wts, props, ln, exact, _ in linear_cases:
        T = _exact.exact_colsum(lin, props, wts)
        assert numpy.array_equal(exact.T[1], T), (label, vec)
        assert numpy.array_equal(exact.ln[1], _exact.exact_finalize(T, ln, props)), (label, vec)
        # without props0 the first pass reads exp(ln) in long double, and is exact_colsum of that
        p_ld = numpy.exp(ln.astype(_exact.LD))
        alone = traj.exact_trajectory(lin, ln, wts, 1)
        T = _exact.exact_colsum(lin, p_ld, wts)
        assert numpy.array_equal(alone.T[1], T) and numpy.array_equal(alone.ln[1], _exact.exact_finalize(T, ln, p_ld))


def test_honest_fp64_loops_are_inside_the_rule(linear_cases):
    for label, vec, lin, wts, props, ln, exact, seq in linear_cases:
        pair = traj.seq_trajectory(lin, ln, wts, K_MAX, props0=props, colsum=_exact.pairwise_colsum)
        for k in inputs.LOOP_STEPS:
            err_seq, l1_seq = traj.seq_errors(exact, seq, k)
            err_pair, l1_pair = traj.seq_errors(exact, pair, k)
            bound, l1_bound = traj.ln_bound(err_seq, exact.ln[k], k), traj.l1_bound(l1_seq, exact.ln[k], k)
            print("%-22s %-9s K=%-2d ln: seq %.3g, pairwise %.3g, floor %.3g | l1 %.3g: seq %.3g, pairwise %.3g, bound %.3g"
                  % (label, vec, k, err_seq, err_pair, traj.ln_floor(exact.ln[k], k), float(exact.l1[k]), l1_seq, l1_pair, l1_bound))
            assert err_seq <= bound and err_pair <= bound, (label, vec, k)
            assert l1_seq <= l1_bound and l1_pair <= l1_bound, (label, vec, k)
            for t in (seq, pair):
                assert _exact.rel_err(t.T[k], exact.T[k]) <= _exact.derived_bound(*lin.shape), (label, vec, k)


@pytest.mark.parametrize("n_haps", inputs.LOOP_WIDTHS_LOG)
def test_the_fp64_oracle_is_inside_the_rule_in_log_space(b17, n_haps):
    """The log-space widths: exact_colsum_log chained, against K steps of em_oracle.em_step (finite throughout, "deep"
    included: neither underflows)."""
    label, mat, wts = inputs.loop_matrix(b17, n_haps)
    for vec, (props, ln) in inputs.loop_vectors(n_haps).items():
        exact = traj.exact_trajectory(mat, ln, wts, K_MAX, log_space=True)
        # the trajectory takes exp(M - rowmax) once in long double: its first step is exact_colsum_log's, to long-double rounding
        direct = _exact.exact_finalize(_exact.exact_colsum_log(mat, ln, wts), ln, numpy.exp(ln.astype(_exact.LD)))
        assert traj.ln_error(exact.ln[1], direct) <= 8 * 2.0 ** -64 * float(numpy.abs(ln).max())
        own = traj.oracle_trajectory(mat, ln, wts, K_MAX)
        # the second honest pass: the linear recurrence in fp64 over numpy's pairwise sums, as the narrow kernels compute it
        second = traj.seq_trajectory(inputs.linearise(mat), ln, wts, K_MAX, colsum=_exact.pairwise_colsum)
        for k in inputs.LOOP_STEPS:
            err, l1_err = traj.seq_errors(exact, own, k)
            err2, l1_err2 = traj.seq_errors(exact, second, k)
            print("%-18s %-9s K=%-2d ln: oracle %.3g, linear fp64 pass %.3g, floor %.3g | l1: %.3g, %.3g"
                  % (label, vec, k, err, err2, traj.ln_floor(exact.ln[k], k), l1_err, l1_err2))
            assert numpy.isfinite(err) and numpy.isfinite(l1_err)            # (the comparison pass itself: finite, no more)
            assert err2 <= traj.ln_bound(err, exact.ln[k], k) and l1_err2 <= traj.l1_bound(l1_err, exact.ln[k], k)


def test_three_mutants_of_the_carry_are_outside_the_rule(linear_cases):
    seen = {m: set() for m in traj.MUTANTS}
    for label, vec, lin, wts, props, ln, exact, seq in linear_cases:
        for mutant in traj.MUTANTS:
            bad = traj.seq_trajectory(lin, ln, wts, 3, props0=props, mutant=mutant)
            inside = [traj.inside_rule(bad.ln[k], exact, seq, k) for k in (1, 2, 3)]
            first = next((k for k, (ok, _, _) in zip((1, 2, 3), inside) if not ok), None)
            print("%-22s %-9s %-22s first outside at K = %s; K = 3: error %.3g, bound %.3g" % (label, vec, mutant, first, inside[2][1], inside[2][2]))
            assert inside[0][0], (label, vec, mutant, "the first step carries nothing")
            assert not inside[2][0], (label, vec, mutant)
            seen[mutant].add(first)
    assert {m: sorted(s) for m, s in seen.items()} == {m: [k] for m, k in FIRST_FAILURE.items()}


def test_deep_vector_is_deep(linear_cases):
    tiny, denorm_min = numpy.log(numpy.finfo(numpy.float64).tiny), numpy.log(5e-324)
    for label, vec, lin, wts, props, ln, exact, seq in linear_cases:
        if vec != "deep":
            _exact.check_products(lin, props)              # (the existing inputs' guard still holds at 96 rows)
            continue
        n_haps = lin.shape[1]
        z_min = min(traj.deep_precondition(lin, exact.ln[k]) for k in (0, 1, 10, K_MAX))
        zero, sub = int((props == 0).sum()), int(((props > 0) & (props < numpy.finfo(numpy.float64).tiny)).sum())
        assert (ln[props == 0] < denorm_min).all() and (ln[props > 0] > denorm_min - 1.0).all()
        crossed = [int(((exact.ln[k] < denorm_min - 1.0) & (props > 0)).sum()) for k in (1, 10, K_MAX)]
        print("%-22s deep: %d subnormal, %d zero, %s more zero after 1 / 10 / %d iterations, min Z %.3g, min T %.3g"
              % (label, sub, zero, crossed, K_MAX, z_min, float(exact.T[1:].min())))
        assert sub >= n_haps // 8 and zero >= n_haps // 16
        assert crossed[2] > crossed[0] >= 0 and crossed[2] >= 1          # proportions cross -745 while the loop runs
        assert (exact.T[1:] > 0).all() and numpy.isfinite(exact.ln.astype(numpy.float64)).all()
        assert z_min >= 1e-3                               # (1.7e-3 .. 1.2e-2) every row keeps a supporter of weight: the documented limit is far
        with pytest.raises(AssertionError):
            _exact.check_products(lin, props)              # which is why this vector needs a precondition of its own


def test_stop_decision_has_its_margin(linear_cases):
    """K* and tol come from the reference's own l1.  Where l1 falls by a few per cent per iteration for all 40 of them, no
    iteration is 1.5 x below every earlier one: those pairs have no stop test, and which they are is pinned here."""
    without = set()
    for label, vec, lin, wts, props, ln, exact, seq in linear_cases:
        k_stop, tol = traj.stop_point(exact.l1)
        if k_stop is None:
            without.add((lin.shape[1], vec))
            continue
        l1 = exact.l1.astype(numpy.float64)
        print("%-22s %-9s K* = %d, tol = %.3g, l1 there %.3g, smallest before %.3g" % (label, vec, k_stop, tol, l1[k_stop], l1[1:k_stop].min()))
        assert 2 <= k_stop <= K_MAX and l1[1:k_stop].min() > traj.GAP * l1[k_stop]
        assert traj.stops_at(exact.l1, tol)[0] == k_stop == traj.stops_at(seq.l1, tol)[0]
    assert without == NO_USABLE_STOP
