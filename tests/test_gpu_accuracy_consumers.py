"""
The consumers of the posterior against the extended-precision reference (tests/_exact_consumers.py): the second half of a
run, where a number turns into a decision -- a contributor, or a read's label.  The rest of the suite checks them against
goldens made with well-conditioned proportions, against each other (batched route against per-sample route, bit for bit) and
with absolute 1e-9 tolerances: a consumer that is wrong in the same way on both routes, in a regime the goldens never
visit, passes all of that.  Here every entry is held to ONE rule (u = 2^-53):

    values      post, lse, folded posteriors, mxm_log_normalize, mxm_l1_exp_diff:
                |got - exact| <= 8 max(the fp64 comparison pass's own largest error, u max |value|)   (_exact.abs_bound)
                over the entries whose exact value is finite; the pattern of -inf / NaN equals the reference's
    decisions   d = twice that bound for the values the decision is taken on.  best[r] is a column whose exact value lies
                within d of the exact row maximum; assigned[r] is the exact label unless |m_r - log_min_fold| <= d or the
                exact top-two gap m_r <= d.  Rows with more than one admissible answer are undecided: at most 1 % per case
                (tests/test_exact_consumers.py asserts it from the reference alone, on the same inputs)
    exact       votes, counts and first-seen rows recomputed from the device's own best and the integer weights: equal

Inputs: tests/_consumer_inputs.py -- among them ORPHAN ROWS, supported only by proportions below exp(-700) .. exp(-750): the
row normaliser taken in linear variables, rowmax + log(sum_h props[h] P[r][h]), is there a subnormal sum of a few mantissa
bits.  Until this module the kernels redid such a row in log space only at sum == 0.  Measured with the library built from
the commit before it: lse and post of mxm_em_step_coded / mxm_votes_samples(_runs) off by up to 0.186 on the orphan rows
(bound 1.2e-12), post of mxm_assign_reads_samples by up to 0.12 and of mxm_assign_reads_samples_runs by up to 0.56 on the
deep samples, and -- the error does not cancel once every run is shifted by its own normaliser -- the multi-run vote
electing a column outside d in 3 ("deep") and 4 ("mixed") decided rows of 400.  They now redo every row whose sum is below
2^-960 (csrc/common.hpp); rows with a normal sum kept their bits.  The module's second finding: mxm_l1_exp_diff took
|exp a - exp b| as the difference of two rounded exponentials, 16 u of the result off (bound 8 u) for two proportions near
0.6 a tenth apart; it now forms exp(hi) * -expm1(lo - hi).

MXM_ACCURACY_REPORT=<file> makes the module write its measured figures to <file>.consumers
(tools/accuracy_report.py -> profiles/accuracy/README.md).
"""
import ctypes
import os

import numpy
import pytest

import _accuracy_inputs as inputs
import _consumer_inputs as cases
import _exact
import _exact_consumers as xc
import test_gpu_accuracy as one_pass

pytestmark = pytest.mark.gpu

_rows = []
_kept = {}


def _record(entry, case, n_haps, n_rows, err, own, bound, undecided=None):
    _rows.append((entry, case, n_haps, n_rows, err, own, bound, undecided))
    print("%-34s %-58s H=%-5d R=%-4d error %s, the comparison pass's %s, bound %s%s"
          % (entry, case, n_haps, n_rows, *("-" if v is None else "%.3g" % v for v in (err, own, bound)),
             "" if undecided is None else ", %d undecided" % undecided))


def _values(entry, case, got, exact, own, n_haps, n_rows):
    """The value rule; -> the bound."""
    err, mine, bound = xc.value_errors(got, exact, own)
    _record(entry, case, n_haps, n_rows, err, mine, bound)
    assert err <= bound, (entry, case, err, mine, bound)
    return bound


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    _kept.clear()
    path = os.environ.get("MXM_ACCURACY_REPORT")
    if not path:
        return
    with open(path + ".consumers", "w") as out:
        out.write("| entry | case | H | R | error | comparison pass | bound | undecided rows |\n|---|---|---|---|---|---|---|---|\n")
        for entry, case, n_haps, n_rows, err, own, bound, undecided in _rows:
            cells = ["-" if v is None else "%.2g" % v for v in (err, own, bound)] + ["-" if undecided is None else "%d" % undecided]
            out.write("| %s | %s | %d | %d | %s |\n" % (entry, case, n_haps, n_rows, " | ".join(cells)))


def _gpu():
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream, require_gpu
    return torch, _lib, _lib.load(), require_gpu(), current_stream


# ---------------------------------------------------------------- mxm_log_normalize, mxm_l1_exp_diff
@pytest.mark.parametrize("n_haps", cases.VECTOR_WIDTHS)
def test_log_normalize_and_l1_exp_diff(n_haps):
    torch, _lib, lib, dev, stream = _gpu()
    for name, T in cases.normalize_vectors(n_haps).items():
        t_d = torch.from_numpy(T).to(dev)
        out = torch.full((n_haps,), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.mxm_log_normalize(t_d.data_ptr(), n_haps, out.data_ptr(), stream()), "mxm_log_normalize")
        _values("mxm_log_normalize", name, out.cpu().numpy(), xc.exact_log_normalize(T), xc.cmp_log_normalize(T), n_haps, 1)
    for name, (a, b) in cases.vector_pairs(n_haps).items():
        a_d, b_d = torch.from_numpy(numpy.ascontiguousarray(a)).to(dev), torch.from_numpy(numpy.ascontiguousarray(b)).to(dev)
        out = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.mxm_l1_exp_diff(a_d.data_ptr(), b_d.data_ptr(), n_haps, out.data_ptr(), stream()), "mxm_l1_exp_diff")
        got = out.cpu().numpy()
        _values("mxm_l1_exp_diff", name, got, numpy.atleast_1d(xc.exact_l1_exp_diff(a, b)), numpy.atleast_1d(xc.cmp_l1_exp_diff(a, b)),
                n_haps, 1)
        if name == "deep, below -745":
            assert got[0] == 0.0                           # every exp is exactly 0


# ---------------------------------------------------------------- mxm_fold_logaddexp
def _placed(torch, dev, block, ld, off):
    """`block` [R][H] as a device view with leading dimension ld whose first element is `off` doubles past a 16-byte
    boundary; the cells around it are NaN."""
    n_rows, n_haps = block.shape
    buf = torch.full((n_rows * ld + 2,), float("nan"), dtype=torch.float64, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n_rows * ld].view(n_rows, ld)
    view[:, :n_haps] = torch.from_numpy(block).to(dev)
    assert view.data_ptr() % 16 == 8 * off and view.stride(0) == ld
    return buf, view


def _fold_layouts(n_haps):
    """(name, lda, ld of input 0, offset of acc, offset of input 0): the 16-byte instance needs an even H, even leading
    dimensions and aligned pointers everywhere -- each of the three ways of breaking that forces the scalar one."""
    even = n_haps + (n_haps & 1)
    if n_haps & 1:
        return [("odd H", even, even, 0, 0), ("odd H, odd ld", n_haps, n_haps + 2, 0, 0)]
    return [("vectors", n_haps, n_haps + 2, 0, 0), ("odd ld of acc", n_haps + 1, n_haps, 0, 0),
            ("odd ld of an input", n_haps, n_haps + 1, 0, 0), ("acc 8 bytes off", n_haps, n_haps, 1, 0),
            ("an input 8 bytes off", n_haps + 2, n_haps, 0, 1)]


@pytest.mark.parametrize("n_in", cases.FOLD_INPUTS)
@pytest.mark.parametrize("n_haps", cases.FOLD_WIDTHS)
def test_fold_logaddexp(n_haps, n_in):
    torch, _lib, lib, dev, stream = _gpu()
    blocks = cases.fold_blocks(n_haps, n_in)
    for delta in (0.0, -float(numpy.log(n_in + 1.0))):
        exact, own = xc.exact_fold(blocks, delta), xc.cmp_fold(blocks, delta)
        for name, lda, ld0, off_acc, off0 in _fold_layouts(n_haps):
            keep, acc = _placed(torch, dev, blocks[0], lda, off_acc)
            ins = [_placed(torch, dev, blk, ld0 if k == 0 else n_haps + (n_haps & 1), off0 if k == 0 else 0) for k, blk in enumerate(blocks[1:])]
            ptrs = (ctypes.c_void_p * n_in)(*[v.data_ptr() for _, v in ins])
            lds = (ctypes.c_int64 * n_in)(*[v.stride(0) for _, v in ins])
            _lib.check(lib.mxm_fold_logaddexp(acc.data_ptr(), lda, ptrs, lds, n_in, cases.FOLD_ROWS, n_haps, delta, stream()),
                       "mxm_fold_logaddexp")
            got = acc[:, :n_haps].cpu().numpy()
            _values("mxm_fold_logaddexp", "n_in = %d, delta = %.3g, %s" % (n_in, delta, name), got, exact, own, n_haps, cases.FOLD_ROWS)
            assert torch.isnan(acc[:, n_haps:]).all()      # the pad columns are left alone


# ---------------------------------------------------------------- the posterior under "deep", orphan rows included
def _post_vectors(n_haps):
    return {"deep": cases.run_vectors(n_haps, "deep", 2), "skewed": cases.run_vectors(n_haps, "skewed", 1)}


def _orphan_figures(entry, case, got, exact, t_of, n_haps):
    """The error of the orphan rows per threshold, beside the ordinary rows' (recorded, not asserted: the value rule over the
    whole matrix is the assertion)."""
    with numpy.errstate(invalid="ignore"):
        err = numpy.abs(numpy.asarray(got).astype(_exact.LD) - exact).astype(numpy.float64)
    if err.ndim == 2:
        err = numpy.where(numpy.isfinite(err), err, 0.0).max(axis=1)
    groups = [("ordinary rows", numpy.isnan(t_of))] + [("orphans below %g" % t, t_of == t) for t in cases.ORPHAN_T]
    for name, rows in groups:
        _record(entry, "%s: %s" % (case, name), n_haps, int(rows.sum()), float(err[rows].max()), None, None)


@pytest.mark.parametrize("n_haps", [64, 65, 128])
def test_dense_posterior_deep(b17, n_haps):
    """mxm_em_step (log space throughout: these are pins)."""
    from mixemt_amd import em
    label, mat, t_of = cases.orphan_matrix(b17, n_haps, "few", 200)
    plan = em.EmPlan(numpy.array(mat), inputs.weights(len(mat)))
    ln = _post_vectors(n_haps)["deep"][0]
    got = em.posterior(plan, ln).cpu().numpy()
    exact = xc.exact_posterior(mat, ln)
    _values("mxm_em_step", "deep, " + label, got, exact, xc.cmp_posterior(mat, ln), n_haps, len(mat))
    _orphan_figures("mxm_em_step", "deep", got, exact, t_of, n_haps)
    assert numpy.isfinite(got[t_of == -750.0]).any(axis=1).all()


def _records(mat):
    """(records plan, CodedMatrix over it) of a log matrix; every row has a record."""
    import torch
    from mixemt_amd import preprocess
    key = id(mat)
    if key not in _kept:
        wts = inputs.weights(len(mat))
        plan = one_pass._coded_plan(numpy.array(mat), wts)
        assert plan.coded_rest == 0
        rest = torch.nonzero(plan.coded_ndist == 0).flatten()
        cm = preprocess.CodedMatrix(len(mat), mat.shape[1], *plan._coded_keep[:3], plan.rowmax, 0, rest, plan.mat[rest].contiguous())
        _kept[key] = (mat, plan, cm, wts)
    return _kept[key][1:]


@pytest.mark.parametrize("which", [0, 1], ids=["byte codes 128", "wide records 5408"])
def test_records_posterior_deep(b17, which):
    """mxm_em_step_coded mode 0 and mode 1 under "deep": the orphan rows' normaliser."""
    from mixemt_amd import em
    label, mat, t_of = cases.vote_matrices(b17)[which]
    n_haps = mat.shape[1]
    plan, cm, wts = _records(mat)
    assert which == 0 or plan.coded_wide > 0
    rec_plan = em.EmPlan(None, wts, records=cm)
    vecs = _post_vectors(n_haps)
    ln_a, ln_b, ln_s = vecs["deep"][0], vecs["deep"][1], vecs["skewed"][0]
    exact_a, own_a = xc.exact_posterior(mat, ln_a), xc.cmp_posterior(mat, ln_a)
    out = em.posterior(rec_plan, ln_a)
    got = out.cpu().numpy()
    _orphan_figures("mxm_em_step_coded, mode 0", "deep", got, exact_a, t_of, n_haps)
    assert numpy.isfinite(got[t_of == -750.0]).any(axis=1).all()          # the z == 0 redo the kernel always had
    _values("mxm_em_step_coded, mode 0", "deep, " + label, got, exact_a, own_a, n_haps, len(mat))
    for name, ln_2 in (("deep + deep", ln_b), ("deep + skewed", ln_s)):
        out = em.posterior(rec_plan, ln_a)
        out = em.posterior(rec_plan, ln_2, out=out, fold=True)
        exact = xc.exact_fold([exact_a, xc.exact_posterior(mat, ln_2)])
        own = xc.cmp_fold([own_a, xc.cmp_posterior(mat, ln_2)])
        _values("mxm_em_step_coded, mode 1", "%s, %s" % (name, label), out.cpu().numpy(), exact, own, n_haps, len(mat))


# ---------------------------------------------------------------- the votes
def _vote_ref(mat, table, key):
    """(exact values, bound, d) of one run table on one matrix, made once."""
    key = ("vote", id(mat)) + key
    if key not in _kept:
        exact, own = xc.vote_reference(mat, table)
        bound = xc.value_errors(own, exact, own)[2]
        _kept[key] = (mat, exact, bound, 2.0 * bound)
    return _kept[key][1:]


def _check_votes(entry, case, best, votes, counts, first, exact, d, wts, n_haps):
    undecided = xc.check_best(best, exact, d)
    _record(entry, case, n_haps, len(best), None, None, d, int(undecided.sum()))
    assert xc.within_cap(undecided), (entry, case, int(undecided.sum()))
    want_votes, want_counts, want_first = xc.exact_votes(best, wts, n_haps)
    assert numpy.array_equal(votes, want_votes.astype(numpy.float64)), (entry, case, "votes")
    if counts is not None:
        assert numpy.array_equal(counts, want_counts), (entry, case, "counts")
    if first is not None:
        assert numpy.array_equal(first, want_first), (entry, case, "first-seen rows")


@pytest.mark.parametrize("kind", cases.VOTE_KINDS)
@pytest.mark.parametrize("which", [0, 1], ids=["byte codes 128", "wide records 5408"])
def test_votes_from_records(b17, which, kind):
    """mxm_row_argmax_votes_coded with n_runs = 1, 2 and 3 over the whole matrix."""
    from mixemt_amd import assign
    label, mat, _ = cases.vote_matrices(b17)[which]
    n_haps = mat.shape[1]
    plan, cm, wts = _records(mat)
    for n_runs in (1, 2, 3):
        table = cases.run_vectors(n_haps, kind, n_runs)
        exact, _, d = _vote_ref(mat, table, (kind, n_runs, 0))
        best, votes = assign.row_argmax_votes_records(cm, table if n_runs > 1 else table[0], wts)
        _check_votes("mxm_row_argmax_votes_coded", "%s, B = %d, %s" % (kind, n_runs, label), best, votes, None, None, exact, d, wts, n_haps)


def _finish(mat):
    from mixemt_amd import em
    plan, cm, wts = _records(mat)
    row0 = cases.sample_cuts(len(mat))
    n = int(row0[-1])                                      # (the samples need not reach the matrix's last row)
    sub = cm.rows(0, n)
    return em.SampleFinish(sub.rec, sub.rec_off, sub.ndist, plan.wts[:n], sub.rowmax, row0, mat.shape[1]), row0, wts


@pytest.mark.parametrize("kind", cases.VOTE_KINDS)
@pytest.mark.parametrize("which", [0, 1], ids=["byte codes 128", "wide records 5408"])
def test_votes_of_samples(b17, which, kind):
    """mxm_votes_samples with lse and mxm_votes_samples_runs with lse (B = 2, 3) on samples of 1, 63, 64, 65 and 200 rows;
    the odd samples take the runs in reversed order."""
    label, mat, t_of = cases.vote_matrices(b17)[which]
    n_haps = mat.shape[1]
    fin, row0, wts = _finish(mat)
    n = len(row0) - 1
    for n_runs in (1, 2, 3):
        tables = cases.sample_run_vectors(n_haps, kind, n_runs, n)
        if n_runs == 1:
            entry = "mxm_votes_samples"
            best, votes, counts, first, lse, errors = fin.votes(tables[:, 0], want_lse=True)
        else:
            entry = "mxm_votes_samples_runs"
            best, votes, counts, first, lse, errors = fin.votes_runs(tables, want_lse=True)
        assert not any(errors)
        best, lse = best.cpu().numpy(), lse.cpu().numpy().reshape(int(row0[-1]), n_runs)
        for s in range(n):
            lo, hi = int(row0[s]), int(row0[s + 1])
            order = (s % 2) if n_runs > 1 else 0
            exact, _, d = _vote_ref(mat, tables[s], (kind, n_runs, order))
            case = "%s, B = %d, sample of %d rows, %s" % (kind, n_runs, hi - lo, label)
            _check_votes(entry, case, best[lo:hi], votes[s], counts[s], first[s], exact[lo:hi], d, wts[lo:hi], n_haps)
            for b in range(n_runs):
                sub = mat[lo:hi]
                _values(entry + ", lse", "%s, run %d" % (case, b), lse[lo:hi, b], xc.exact_row_lse(sub, tables[s, b]),
                        xc.cmp_row_lse(sub, tables[s, b]), n_haps, hi - lo)


# ---------------------------------------------------------------- the assignment
def _thresholds(V):
    margin = xc.exact_labels(V, 0.0)[1]
    finite = margin[numpy.isfinite(margin.astype(numpy.float64))].astype(numpy.float64)
    return [float(numpy.log(2.0)), float(numpy.median(finite))]


@pytest.mark.parametrize("ascending", [True, False], ids=["ascending", "any order"])
@pytest.mark.parametrize("n_cols", [2, 3, 16])
def test_assign_reads_dense(n_cols, ascending):
    """mxm_assign_reads on a dense X: the ordinal of the best column among cols[], or -1."""
    torch, _lib, lib, dev, stream = _gpu()
    X, log_props, cols = cases.dense_assign_case(n_cols, ascending)
    n_rows, n_haps = X.shape
    exact, own = xc.exact_assign_values(X[:, cols], log_props[cols]), xc.cmp_assign_values(X[:, cols], log_props[cols])
    d = 2.0 * xc.value_errors(own, exact, own)[2]
    x_d, lp_d, c_d = torch.from_numpy(X).to(dev), torch.from_numpy(log_props).to(dev), torch.from_numpy(cols).to(dev)
    for lmf in _thresholds(exact):
        assigned = torch.full((n_rows,), -7, dtype=torch.int32, device=dev)
        _lib.check(lib.mxm_assign_reads(x_d.data_ptr(), x_d.stride(0), lp_d.data_ptr(), c_d.data_ptr(), n_cols, n_rows, n_haps, lmf,
                                        assigned.data_ptr(), stream()), "mxm_assign_reads")
        undecided = xc.check_labels(assigned.cpu().numpy(), exact, lmf, d)
        _record("mxm_assign_reads", "nC = %d, %s, log_min_fold %.4g" % (n_cols, "ascending" if ascending else "any order", lmf),
                n_haps, n_rows, None, None, d, int(undecided.sum()))
        assert xc.within_cap(undecided)


def _assign_finish(n_rows_total, row0):
    """A SampleFinish over any records of the batch's row count (the assignment reads M, not the records)."""
    from mixemt_amd import em
    mat = inputs.few_values(n_rows_total, 128)
    plan, cm, wts = _records(mat)
    return em.SampleFinish(cm.rec, cm.rec_off, cm.ndist, plan.wts, cm.rowmax, row0, 128)


@pytest.mark.parametrize("n_runs", [1, 2, 3])
@pytest.mark.parametrize("ld", [4, 8, 16])
def test_assign_reads_of_samples(ld, n_runs):
    """mxm_assign_reads_samples (B = 1) and mxm_assign_reads_samples_runs (B = 2, 3): post and labels, with the internal
    normaliser and with a given lse, at log_min_fold = log 2 and at the median of the exact margins; K = 2, 3 (and 16), one
    well-conditioned sample and one whose every column is deep per K."""
    torch, _lib, lib, dev, stream = _gpu()
    batch = cases.assign_batch(ld, n_runs)
    row0, ncol, perm, sample_of = batch["row0"], batch["ncol"], batch["perm"], batch["sample_of"]
    n_rows = int(row0[-1])
    fin = _assign_finish(n_rows, row0)
    entry = "mxm_assign_reads_samples" + ("_runs" if n_runs > 1 else "")
    delta = -float(numpy.log(float(n_runs))) if n_runs > 1 else 0.0
    m_d = torch.from_numpy(batch["M"]).to(dev)
    for given in (False, True):
        X, V, Xc, Vc = xc.assign_samples_reference(batch["M"], sample_of, ncol, batch["ln_theta"], batch["log_props"],
                                                   batch["lse"] if given else None, delta)
        d = 2.0 * xc.value_errors(Vc, V, Vc)[2]
        lse_d = torch.from_numpy(batch["lse"] if n_runs > 1 else numpy.ascontiguousarray(batch["lse"][:, 0])).to(dev) if given else None
        for lmf in _thresholds(V):
            min_fold = float(numpy.exp(lmf))
            used = float(numpy.log(min_fold))              # the wrappers take min_fold and pass its logarithm
            if n_runs > 1:
                assigned, post = fin.assign_runs(m_d, ld, ncol, perm, batch["ln_theta"], batch["log_props"], lse_d, min_fold, want_post=True)
            else:
                assigned, post = fin.assign(m_d, ld, ncol, perm, batch["ln_theta"][:, 0], batch["log_props"], lse_d, min_fold, want_post=True)
            case = "ld = %d, B = %d, %s normaliser, log_min_fold %.4g" % (ld, n_runs, "given" if given else "internal", used)
            _values(entry + ", post", case, post.cpu().numpy(), X, Xc, ld, n_rows)
            got = assigned.cpu().numpy()
            column = numpy.full(n_rows, -1, dtype=numpy.int64)   # the label back to the column it names: perm is a permutation
            for s in range(len(ncol)):
                inverse = numpy.argsort(perm[s, :ncol[s]])
                rows = numpy.flatnonzero((sample_of == s) & (got >= 0))
                assert (got[rows] < ncol[s]).all()
                column[rows] = inverse[got[rows]]
            assert (got >= -1).all()
            undecided = xc.check_labels(column, V, used, d)
            _record(entry, case, ld, n_rows, None, None, d, int(undecided.sum()))
            assert xc.within_cap(undecided)
