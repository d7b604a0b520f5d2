"""
The extended-precision reference (tests/_exact.py) catches what it is for, on every input of the accuracy tests
(tests/_accuracy_inputs.py) -- CPU only:
  * two honest fp64 passes, numpy's pairwise one and the sequential comparison pass, are inside both bounds;
  * three subtly wrong passes are outside the tight one: (a) the reciprocal of Z rounded to fp32, (b) the last column left
    out of Z while its proportion is 1e-12, (c) T accumulated in fp32 -- and (b) moves the proportions by less than 1e-9,
    i.e. an absolute tolerance on the proportions cannot see it.
"""
import numpy
import pytest

import _accuracy_inputs as inputs
import _exact


@pytest.fixture(scope="module")
def cases(b17):
    """(label, vector name, P, props, w, exact T, rel(T_seq)) for every input and both proportion vectors, made once."""
    out = []
    for label, mat, wts in inputs.all_inputs(b17):
        lin = inputs.linearise(mat)
        for vec, (props, _) in inputs.prop_vectors(mat.shape[1]).items():
            smallest = _exact.check_products(lin, props)
            exact = _exact.exact_colsum(lin, props, wts)
            rel_seq = _exact.rel_err(_exact.seq_colsum(lin, props, wts), exact)
            print("%-18s %-9s smallest product %.2g, rel(T_seq) = %.1f u" % (label, vec, smallest, rel_seq / _exact.U))
            out.append((label, vec, lin, props, wts, exact, rel_seq))
    return out


def test_honest_fp64_passes_are_inside_both_bounds(cases):
    for label, vec, lin, props, wts, exact, rel_seq in cases:
        n_rows, n_haps = lin.shape
        rel_pair = _exact.rel_err(_exact.pairwise_colsum(lin, props, wts), exact)
        print("%-18s %-9s seq %.1f u, pairwise %.1f u, tight %.0f u, derived %d u"
              % (label, vec, rel_seq / _exact.U, rel_pair / _exact.U, _exact.tight_bound(rel_seq) / _exact.U, n_rows + n_haps + 8))
        for rel in (rel_seq, rel_pair):
            assert rel <= _exact.tight_bound(rel_seq), (label, vec)
            assert rel <= _exact.derived_bound(n_rows, n_haps), (label, vec)


def test_three_mutants_are_outside_the_tight_bound(cases):
    for label, vec, lin, props, wts, exact, rel_seq in cases:
        if lin.shape[1] == 1 and vec == "dirichlet":       # one column and p = 1: P = exp(M - rowmax) is 1 in every row, T = sum(w),
            continue                                       # every factor is exact in fp32 too -- nothing a mutant could get wrong
        bound = _exact.tight_bound(rel_seq)
        rel_a = _exact.rel_err(_exact.seq_colsum(lin, props, wts, recip=numpy.float32), exact)
        rel_c = _exact.rel_err(_exact.seq_colsum(lin, props, wts, acc=numpy.float32), exact)
        print("%-18s %-9s bound %.3g: fp32 reciprocal %.3g, fp32 sums %.3g" % (label, vec, bound, rel_a, rel_c))
        assert rel_a > bound and rel_c > bound, (label, vec)
        if vec != "skewed":                                # (b) is about p_last = 1e-12: the skewed vector's last entry
            continue
        assert abs(props[-1] / 1e-12 - 1.0) < 1e-14
        with numpy.errstate(invalid="ignore", divide="ignore"):
            mutant = _exact.seq_colsum(lin, props, wts, skip_last=True)
        rel_b = _exact.rel_err(mutant, exact)
        good = (props * exact.astype(numpy.float64))
        bad = props * mutant
        shift = numpy.abs(bad / bad.sum() - good / good.sum()).max()
        print("%-18s %-9s bound %.3g: column dropped %.3g, shift of the proportions %.3g" % (label, vec, bound, rel_b, shift))
        assert rel_b > bound, label
        if not label.startswith("few values"):             # on real rows PROPS_ATOL = 1e-9 cannot see it (a random matrix is not
            assert shift < 1e-9, label                     # explained by the skewed vector: there the proportions move visibly)


# ---------------------------------------------------------------- the instance sweep's rule (tests/test_gpu_instances.py)
def _edge_pass(lin, props, wts, drop_last=False, pad=None):
    """A sequential fp64 pass as a kernel with a wrong predicate on its last chunk would run it (the mutant pattern of
    tests/_exact_traj.py): drop_last = the class's last column is never visited (not in Z, its sum stays 0); pad = the
    value of ONE pad column behind the row that the pass reads as if it were a column (its proportion: the last one's)."""
    n_haps = lin.shape[1]
    if drop_last:
        out = numpy.zeros(n_haps)
        out[:-1] = _exact.seq_colsum(lin[:, :-1], props[:-1], wts)
        return out
    wide = numpy.concatenate([lin, numpy.full((len(lin), 1), pad)], axis=1)
    with numpy.errstate(invalid="ignore"):
        return _exact.seq_colsum(wide, numpy.append(props, props[-1]), wts)[:n_haps]


def test_edge_mutants_fail_the_rule_at_every_edge_width(b17):
    """At every (edge width, row count) at which tests/test_gpu_instances.py checks a colsum (_instances.colsum_shapes),
    on edge_rows of that shape: the honest sequential pass is inside both bounds; a pass that drops the last column, and one
    that reads one pad column too many (the pad holds NaN), are outside the tight bound -- under both proportion vectors,
    the skewed one (p_last = 1e-12) included."""
    import _instances as inst
    shapes = inst.colsum_shapes()
    assert shapes[0][0] == 65 and shapes[-1][0] == 8192 and set(r for _, r in shapes) == {3, 37, 64}
    assert set(w for w, _ in shapes) >= set(w for w in inst.edge_widths(inst.COLSUM_SITES))
    for n_haps, n_rows in shapes:
        label, mat = inputs.edge_rows(b17, n_haps, n_rows)
        wts = inputs.weights(n_rows)
        lin = inputs.linearise(mat)
        for vec, (props, _) in inputs.prop_vectors(n_haps).items():
            _exact.check_products(lin, props)
            exact = _exact.exact_colsum(lin, props, wts)
            rel_seq = _exact.rel_err(_exact.seq_colsum(lin, props, wts), exact)
            bound = _exact.tight_bound(rel_seq)
            assert rel_seq <= _exact.derived_bound(n_rows, n_haps), (label, vec)
            rel_drop = _exact.rel_err(_edge_pass(lin, props, wts, drop_last=True), exact)
            rel_pad = _exact.rel_err(_edge_pass(lin, props, wts, pad=numpy.nan), exact)
            assert rel_drop > bound and rel_pad > bound, (label, vec, rel_drop, rel_pad, bound)
        print("%-34s R=%-2d rel(T_seq) = %.1f u, bound %.1f u: last column dropped %.3g, NaN pad read %.3g"
              % (label, n_rows, rel_seq / _exact.U, bound / _exact.U, rel_drop, rel_pad))
