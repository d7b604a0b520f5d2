"""
The consumers' extended-precision reference (tests/_exact_consumers.py) catches what it is for, on every input of the device
tests (tests/_consumer_inputs.py) -- CPU only:
  * the honest fp64 passes are inside the value rule: the comparison pass has the reference's pattern of -inf / NaN, and a
    SECOND honest pass per quantity (the kernels' own forms restated in numpy: the fast normaliser with its log-space redo
    below 2^-960, the fold written out by hand, the vector kernels' strided sums) is inside the bound the comparison pass
    sets;
  * four restated kernel mistakes are outside it on at least one input: the fast normaliser with the redo only at z == 0
    (what the kernels did before), a fold in linear space, a fold that adds delta once per input, an assignment that takes
    the runner-up from the first nC - 1 columns only;
  * every decision case of the device tests has at most 1 % undecided rows, from the reference alone.
"""
import numpy
import pytest

import _accuracy_inputs as inputs
import _consumer_inputs as cases
import _exact
import _exact_consumers as xc


def _inside(what, got, exact, own):
    err, mine, bound = xc.value_errors(got, exact, own)
    print("%-72s error %.3g, the comparison pass's %.3g, bound %.3g" % (what, err, mine, bound))
    assert err <= bound, (what, err, mine, bound)
    return bound


def _dense_matrices(b17):
    return [cases.orphan_matrix(b17, h, "few", 200) for h in (64, 65, 128)]


# ---------------------------------------------------------------- honest passes
@pytest.mark.parametrize("n_haps", cases.VECTOR_WIDTHS)
def test_small_vector_entries(n_haps):
    for name, T in cases.normalize_vectors(n_haps).items():
        with numpy.errstate(divide="ignore"):
            seq = numpy.log(T) - numpy.log(xc.strided_sum(T))
        _inside("log_normalize H=%d %s" % (n_haps, name), seq, xc.exact_log_normalize(T), xc.cmp_log_normalize(T))
    for name, (a, b) in cases.vector_pairs(n_haps).items():
        seq = xc.strided_sum(xc.abs_exp_diff(a, b))
        exact = xc.exact_l1_exp_diff(a, b)
        _inside("l1_exp_diff H=%d %s (exact %.3g)" % (n_haps, name, float(exact)), seq, exact, xc.cmp_l1_exp_diff(a, b))
        if name == "deep, below -745":
            assert seq == 0.0 and xc.cmp_l1_exp_diff(a, b) == 0.0 and 0 <= exact < n_haps * _exact.LD(2.0) ** -1074


@pytest.mark.parametrize("n_haps", cases.FOLD_WIDTHS)
def test_fold_by_hand_is_inside_and_two_mutants_are_outside(n_haps):
    caught = {"linear": 0, "delta": 0}
    for n_in in cases.FOLD_INPUTS:
        blocks = cases.fold_blocks(n_haps, n_in)
        for delta in (0.0, -float(numpy.log(n_in + 1.0))):
            exact, own = xc.exact_fold(blocks, delta), xc.cmp_fold(blocks, delta)
            _inside("fold H=%d n_in=%d delta=%.3g" % (n_haps, n_in, delta), xc.fold_by_hand(blocks, delta), exact, own)
            assert numpy.isneginf(exact[3].astype(numpy.float64)).all() and numpy.isfinite(exact[4].astype(numpy.float64)).all()
            caught["linear"] += not xc.inside(xc.mutant_fold_linear(blocks, delta), exact, own)
            if n_in >= 2 and delta != 0.0:
                caught["delta"] += not xc.inside(xc.mutant_fold_delta_per_input(blocks, delta), exact, own)
    print("H=%d: the linear fold is outside in %d cases of 8, delta per input in %d of 3" % (n_haps, caught["linear"], caught["delta"]))
    assert caught["linear"] == 8 and caught["delta"] == 3


def test_posteriors_and_the_fast_normaliser(b17):
    """The kernels' normaliser restated: with the redo below 2^-960 inside the rule on every matrix and vector, orphan rows
    included; with the redo at z == 0 only (the mutant) outside it wherever a row's linear sum is subnormal."""
    outside = []
    for label, mat, t_of in cases.vote_matrices(b17) + _dense_matrices(b17):
        n_haps = mat.shape[1]
        for kind in ("skewed", "deep"):
            ln = cases.run_vectors(n_haps, kind, 1)[0]
            props = numpy.exp(ln)
            exact_lse, own_lse = xc.exact_row_lse(mat, ln), xc.cmp_row_lse(mat, ln)
            lse, z = xc.fast_row_lse(mat, ln, props)
            _inside("row normaliser, %s, %s" % (label, kind), lse, exact_lse, own_lse)
            exact, own = xc.exact_posterior(mat, ln), xc.cmp_posterior(mat, ln)
            bound = _inside("posterior, %s, %s" % (label, kind), xc.fast_posterior(mat, ln), exact, own)
            old_lse, _ = xc.fast_row_lse(mat, ln, props, redo_below=0)
            window = (z > 0) & (z < xc.SMALLEST_NORMAL)
            miss = numpy.abs(old_lse.astype(_exact.LD) - exact_lse).astype(numpy.float64)
            if kind == "deep":
                for t in cases.ORPHAN_T:
                    rows = t_of == t
                    print("   orphans t = %g: %d rows, %d with 0 < z < 2^-1022, %d with z == 0; redo at z == 0 only misses the "
                          "normaliser by up to %.3g (median %.3g)" % (t, rows.sum(), (rows & window).sum(), (rows & (z == 0)).sum(),
                                                                       miss[rows].max(), numpy.median(miss[rows])))
                assert (z[t_of == -750.0] == 0).all() and numpy.isfinite(lse[t_of == -750.0]).all()
                assert (z[~numpy.isnan(t_of)] < xc.LOG_REDO_BELOW).all() and (z[numpy.isnan(t_of)] >= xc.LOG_REDO_BELOW).all()
                assert window[(t_of == -715.0) | (t_of == -738.0)].mean() > 0.5
            else:
                assert not window.any()
            if window.any():
                assert numpy.array_equal(old_lse[~window & (z >= xc.LOG_REDO_BELOW)], lse[~window & (z >= xc.LOG_REDO_BELOW)])
                if not xc.inside(xc.fast_posterior(mat, ln, redo_below=0), exact, own):
                    outside.append((label, float(miss[window].max()), bound))
    print("redo at z == 0 only is outside the rule on:", outside)
    assert len(outside) >= 3


def _vote_tables(n_haps, kind, n_runs):
    """The run tables a vote case sees: the runs in order (whole matrix, even samples) and reversed (odd samples)."""
    fwd = cases.run_vectors(n_haps, kind, n_runs)
    return [fwd] if n_runs == 1 else [fwd, numpy.ascontiguousarray(fwd[::-1])]


def test_vote_values_and_their_undecided_rows(b17):
    for label, mat, _ in cases.vote_matrices(b17):
        for kind in cases.VOTE_KINDS:
            for n_runs in (1, 2, 3):
                for order, table in enumerate(_vote_tables(mat.shape[1], kind, n_runs)):
                    what = "vote values, %s, %s, B = %d%s" % (label, kind, n_runs, ", reversed" if order else "")
                    exact, own, fast = xc.vote_reference(mat, table, fast=xc.LOG_REDO_BELOW)
                    d = 2.0 * _inside(what, fast, exact, own)
                    undecided = xc.check_best(numpy.argmax(own, axis=1), exact, d)
                    print("   undecided rows: %d of %d at d = %.3g" % (undecided.sum(), len(mat), d))
                    assert xc.within_cap(undecided), what
                    row0 = cases.sample_cuts(len(mat))
                    for s in range(len(row0) - 1):
                        if (s % 2) == order or n_runs == 1:
                            assert xc.within_cap(undecided[row0[s]:row0[s + 1]]), (what, s)


def test_a_vote_over_the_old_normaliser_elects_other_columns(b17):
    """What the window costs: with the redo at z == 0 only, the "mixed" runs (an orphan row's normaliser subnormal in one
    run, normal in the others) move the argmax of decided rows."""
    label, mat, t_of = cases.vote_matrices(b17)[0]
    table = cases.run_vectors(mat.shape[1], "mixed", 3)
    exact, own, old = xc.vote_reference(mat, table, fast=0)
    d = 2.0 * xc.value_errors(own, exact, own)[2]
    moved = numpy.flatnonzero(~xc.undecided_best(exact, d) & (numpy.argmax(old, axis=1) != numpy.argmax(exact, axis=1)))
    print("decided rows whose winner changes:", moved, "thresholds", t_of[moved])
    assert not xc.inside(old, exact, own)
    with pytest.raises(AssertionError):
        xc.check_best(numpy.argmax(old, axis=1), exact, d)


# ---------------------------------------------------------------- the assignment
def _fold_thresholds(margin):
    finite = margin[numpy.isfinite(margin.astype(numpy.float64))].astype(numpy.float64)
    return [float(numpy.log(2.0)), float(numpy.median(finite))]


@pytest.mark.parametrize("n_cols", [2, 3, 16])
def test_dense_assignment_and_the_short_runner_up(n_cols):
    for ascending in (True, False):
        X, log_props, cols = cases.dense_assign_case(n_cols, ascending)
        exact, own = xc.exact_assign_values(X[:, cols], log_props[cols]), xc.cmp_assign_values(X[:, cols], log_props[cols])
        d = 2.0 * _inside("mxm_assign_reads values, nC = %d, %s" % (n_cols, "ascending" if ascending else "any order"), own, exact, own)
        for lmf in _fold_thresholds(xc.exact_labels(exact, 0.0)[1]):
            undecided = xc.check_labels(xc.labels_fp64(own, lmf), exact, lmf, d)
            want = xc.exact_labels(exact, lmf)[0]
            print("   log_min_fold %.4g: %d undecided, %d unassigned of %d" % (lmf, undecided.sum(), (want < 0).sum(), len(want)))
            assert xc.within_cap(undecided) and 0 < (want < 0).sum() < len(want)
            with pytest.raises(AssertionError):            # the mutant: runner-up among the first nC - 1 columns
                xc.check_labels(xc.labels_fp64(own, lmf, runner_up_columns=n_cols - 1), exact, lmf, d)


@pytest.mark.parametrize("n_runs", [1, 2, 3])
@pytest.mark.parametrize("ld", [4, 8, 16])
def test_batched_assignment(ld, n_runs):
    batch = cases.assign_batch(ld, n_runs)
    delta = -float(numpy.log(float(n_runs))) if n_runs > 1 else 0.0
    for given in (False, True):
        lse = batch["lse"] if given else None
        X, V, Xc, Vc = xc.assign_samples_reference(batch["M"], batch["sample_of"], batch["ncol"], batch["ln_theta"], batch["log_props"],
                                                   lse, delta)
        what = "batched assignment ld = %d, B = %d, %s normaliser" % (ld, n_runs, "given" if given else "internal")
        _inside(what + ", post", Xc, X, Xc)
        d = 2.0 * _inside(what + ", values", Vc, V, Vc)
        for lmf in _fold_thresholds(xc.exact_labels(V, 0.0)[1]):
            undecided = xc.check_labels(xc.labels_fp64(Vc, lmf), V, lmf, d)
            want = xc.exact_labels(V, lmf)[0]
            print("   log_min_fold %.4g: %d undecided, %d unassigned of %d" % (lmf, undecided.sum(), (want < 0).sum(), len(want)))
            assert xc.within_cap(undecided) and 0 < (want < 0).sum() < len(want)
    if n_runs == 1:                                        # the internal normaliser in the kernels' form, deep samples included
        ln, M, sample_of = batch["ln_theta"][:, 0], batch["M"], batch["sample_of"]
        exact_all, _, own_all, _ = xc.assign_samples_reference(M, sample_of, batch["ncol"], batch["ln_theta"], batch["log_props"])
        for s, kind in enumerate(batch["kinds"]):
            k, idx = int(batch["ncol"][s]), numpy.flatnonzero(sample_of == s)
            sub = numpy.ascontiguousarray(M[idx, :k])
            _inside("   sample %d (%s, K = %d), the fast form" % (s, kind, k), xc.fast_posterior(sub, ln[s, :k]), exact_all[idx, :k],
                    own_all[idx, :k])
            z = xc.fast_row_lse(sub, ln[s, :k], numpy.exp(ln[s, :k]))[1]
            if kind == "deep" and len(idx) >= 37:
                assert (z == 0).any() and ((z > 0) & (z < xc.LOG_REDO_BELOW)).any()
            elif kind == "well":
                assert (z >= xc.LOG_REDO_BELOW).all()


def test_the_reference_itself():
    """Edges of the reference: an empty row's normaliser is -inf, the fold of (-inf, -inf) is -inf, exact votes."""
    mat = numpy.array([[-1.0, -2.0], [-numpy.inf, -numpy.inf]])
    lse = xc.exact_row_lse(mat, numpy.log([0.5, 0.5]))
    assert numpy.isneginf(float(lse[1])) and abs(float(lse[0]) - numpy.log(0.5 * numpy.exp(-1.0) + 0.5 * numpy.exp(-2.0))) < 1e-15
    assert numpy.isneginf(float(xc.exact_fold([numpy.array([-numpy.inf]), numpy.array([-numpy.inf])], 1.0)[0]))
    assert abs(float(xc.exact_fold([numpy.array([-800.0]), numpy.array([-800.0])])[0]) - (numpy.log(2.0) - 800.0)) < 1e-13
    votes, counts, first = xc.exact_votes([2, 0, 2], inputs.weights(3) * 0 + [3, 1, 4], 4)
    assert votes.tolist() == [1, 0, 7, 0] and counts.tolist() == [1, 0, 2, 0] and first.tolist() == [1, 3, 0, 3]
