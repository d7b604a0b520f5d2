"""
The host side of assign.finish_many (the batched second half of a cohort run): the column plan, the routing decision,
the draw order of the refinements' initial proportions, the argument checks -- and what the four C entry points say when
they refuse a call (every row is refused before the first HIP call, so no device is needed; the pointers that are not
NULL are never followed).
"""
import argparse
import ctypes

import numpy
import pytest

from mixemt_amd import _lib

PTR = 0x1000                 # "some pointer": never dereferenced by a row below


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import build
    build.build()
    return _lib.load()


def finish_args(**kw):
    args = argparse.Namespace(min_reads=10, contributors=None, var_check=False, min_var_reads=3, frac_var_reads=0.02,
                              var_count=None, var_fraction=0.5, refine_ests=True, min_fold=2.0, tolerance=0.0001,
                              max_iter=10000, init_alpha=1.0, n_multi=1, verbose=False)
    for key, val in kw.items():
        setattr(args, key, val)
    return args


# ---- the column plan ---------------------------------------------------------------------------------------------
def test_column_plan_keeps_both_orders():
    """The reduced matrix's columns ascend by haplogroup index (preprocess.py:247-251); ordinals follow the contributor
    table (descending proportion): perm maps the one to the other."""
    from mixemt_amd import assign
    haps = ["h%02d" % i for i in range(40)]
    index = {h: i for i, h in enumerate(haps)}
    contribs = [["hap1", "h30", 0.6], ["hap2", "h02", 0.3], ["hap3", "h17", 0.1]]
    cols, perm, names = assign._finish_columns(contribs, index)
    assert cols == [2, 17, 30] and perm == [1, 2, 0] and names == ["h02", "h17", "h30"]
    # ... which is what reduce_em_matrix keeps
    from mixemt_amd import preprocess
    _, want = preprocess.reduce_em_matrix(numpy.zeros((1, 40)), haps, contribs)
    assert names == want
    for k, con in enumerate(contribs):                    # column of contributor k -> k
        assert perm[cols.index(index[con[1]])] == k


@pytest.mark.parametrize("widths,ld", [([1], 4), ([4, 2], 4), ([5, 1], 8), ([8], 8), ([9, 3], 16), ([16, 1, 4], 16)])
def test_tables_pad_to_4_8_16_by_the_widest_batched_sample(widths, ld):
    from mixemt_amd import assign
    plans = [(list(range(10, 10 + k)), list(range(k))[::-1], ["x"] * k) for k in widths]
    got_ld, cols, ncol, perm = assign._finish_tables(plans)
    assert got_ld == ld and cols.shape == perm.shape == (len(widths), ld) and cols.dtype == perm.dtype == numpy.int32
    assert list(ncol) == widths
    for s, k in enumerate(widths):
        assert list(cols[s, :k]) == list(range(10, 10 + k)) and list(perm[s, :k]) == list(range(k))[::-1]
        assert not cols[s, k:].any() and not perm[s, k:].any()


def test_ld_comes_from_the_batched_samples_only():
    """A 17-contributor sample goes to the per-sample route and must not widen (or break) the batch's tables."""
    from mixemt_amd import assign
    small = (list(range(3)), [0, 1, 2], ["a", "b", "c"])
    wide = (list(range(17)), list(range(17)), ["x"] * 17)
    assert assign._finish_route(600, "batch", 1, 10 ** 6, 17, 17) == "single"
    assert assign._finish_tables([small])[0] == 4
    with pytest.raises(ValueError, match="at most 16"):
        assign._finish_tables([small, wide])


# ---- the routing decision ----------------------------------------------------------------------------------------
def test_routing_decision():
    from mixemt_amd import assign
    route = assign._finish_route
    assert route(600, "batch", 1, 1000) == "batch"
    assert route(600, "single", 1, 1000) == "single"               # its first EM ran on its own
    assert route(600, "batch", 2, 1000) == "single"                # the fold over several runs stays per sample
    assert route(1000, "batch", 1, 1000) == "batch" and route(1001, "batch", 1, 1000) == "single"
    assert route(64, "batch", 1, 64) == "batch" and route(65, "batch", 1, 64) == "single"
    assert route(600, "batch", 1, 1000, 16, 16) == "batch" and route(600, "batch", 1, 1000, 17, 17) == "single"
    assert route(600, "batch", 1, 1000, 3, 2) == "single"          # a haplogroup named twice
    assert assign.FINISH_KMAX == 16 and assign.FINISH_MAX_ROWS > 0


# ---- the draws ---------------------------------------------------------------------------------------------------
def test_refine_inits_are_drawn_sample_after_sample_for_refined_samples_only():
    from mixemt_amd import assign, em
    numpy.random.seed(11)
    got = assign._finish_inits([3, None, 1, 5], None, 1.0)
    numpy.random.seed(11)
    want = [em.init_props(3), None, em.init_props(1), em.init_props(5)]
    after = numpy.random.random()
    assert got[1] is None
    for g, w in zip(got, want):
        if w is not None:
            assert g.shape == (1, len(w)) and numpy.array_equal(g[0], w)
    numpy.random.seed(11)
    assign._finish_inits([3, None, 1, 5], None, 1.0)
    assert numpy.random.random() == after                  # nothing else was drawn
    # given ones are taken as they are, and checked against the reduced matrix's width
    given = [numpy.array([0.2, 0.3, 0.5]), None, numpy.array([1.0]), numpy.full(5, 0.2)]
    got = assign._finish_inits([3, None, 1, 5], given, 1.0)
    assert numpy.array_equal(got[0], given[0][None, :]) and got[1] is None
    with pytest.raises(ValueError, match=r"refine_inits\[0\] must hold 3"):
        assign._finish_inits([3, None, 1, 5], [numpy.ones(2), None, numpy.ones(1), numpy.ones(5)], 1.0)
    with pytest.raises(ValueError, match="one entry per sample"):
        assign._finish_inits([3, None], [numpy.ones(3)], 1.0)


# ---- the argument checks -----------------------------------------------------------------------------------------
def _records(rec, n_rows, n_haps=66):
    import torch
    from mixemt_amd import preprocess
    return preprocess.CodedMatrix(n_rows, n_haps, rec, torch.zeros(n_rows, dtype=torch.int64), torch.ones(n_rows, dtype=torch.int32),
                                  torch.zeros(n_rows, dtype=torch.float64), 0, torch.zeros(0, dtype=torch.int64),
                                  torch.zeros((0, n_haps), dtype=torch.float64))


def test_finish_many_refuses_before_it_touches_the_device():
    import torch
    from mixemt_amd import assign
    haps = ["h%02d" % i for i in range(66)]
    rec_a, rec_b = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    one, two, other = _records(rec_a, 5), _records(rec_a, 7), _records(rec_b, 7)
    res = [{"props": numpy.full(66, 1 / 66.0), "ln_theta_k": numpy.zeros((1, 66)), "route": "batch"}] * 2
    wts = [numpy.ones(5), numpy.ones(7)]
    with pytest.raises(ValueError, match="build_em_records_many"):
        assign.finish_many([(one, wts[0]), (other, wts[1])], res, haps, finish_args())
    with pytest.raises(ValueError, match="build_em_records_many"):
        assign.finish_many([(numpy.zeros((5, 66)), wts[0]), (two, wts[1])], res, haps, finish_args())
    with pytest.raises(ValueError, match="2 samples, 1 results"):
        assign.finish_many([(one, wts[0]), (two, wts[1])], res[:1], haps, finish_args())
    with pytest.raises(ValueError, match="needs obs="):
        assign.finish_many([(one, wts[0]), (two, wts[1])], res, haps, finish_args(var_check=True))
    with pytest.raises(ValueError, match="obs needs one entry per sample"):
        assign.finish_many([(one, wts[0]), (two, wts[1])], res, haps, finish_args(var_check=True), phylo=object(), obs=[None])
    with pytest.raises(ValueError, match="Unknown haplogroup 'nope'"):
        assign.finish_many([(one, wts[0]), (two, wts[1])], res, haps, finish_args(contributors="h01,nope"))
    with pytest.raises(ValueError, match="65 haplogroups for matrices of 66 columns"):
        assign.finish_many([(one, wts[0]), (two, wts[1])], res, haps[:65], finish_args())


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def test_symbols_are_exported_with_the_bound_signatures(lib):
    import os
    want = {"mxm_samples_finish_workspace_bytes": 3, "mxm_votes_samples": 17, "mxm_gather_columns_samples": 11,
            "mxm_em_loop_samples_narrow": 20, "mxm_assign_reads_samples": 18}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mixemt_hip_samples_finish.h")).read()
    for name, n_args in want.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == n_args, name
        assert ("%s(" % name) in header, name
    assert lib.mxm_version() == 603
    assert lib.mxm_samples_finish_workspace_bytes(0, 1, 4) == 0
    small, large = (lib.mxm_samples_finish_workspace_bytes(10, 3, ld) for ld in (4, 16))
    assert 0 < small <= large and small % 256 == 0


def _coded(**kw):
    c = _lib.Coded()
    c.rec, c.rec_off, c.ndist, c.R = PTR, PTR, PTR, 10
    for key, val in kw.items():
        setattr(c, key, val)
    return c


def _i64(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _i32(*vals):
    return (ctypes.c_int32 * len(vals))(*vals)


STATES = (_lib.EmState * 4)()


def _calls(lib, coded, row0, n_samples, width=128, ld=4, ncol=(2, 3), cols=(1, 2, 0, 0, 5, 6, 7, 0), perm=(1, 0, 0, 0, 2, 0, 1, 0)):
    """entry point -> a call of it on one batch description (only the entries a row names are ever called: the others
    would go on to the device with pointers that are not real)."""
    c, r0 = ctypes.byref(coded), _i64(*row0)
    nc, cs, pm = _i32(*ncol), _i32(*cols), _i32(*perm)
    return {
        "mxm_votes_samples": lambda: lib.mxm_votes_samples(c, r0, n_samples, width, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR,
                                                           PTR, PTR, 1 << 20, None),
        "mxm_gather_columns_samples": lambda: lib.mxm_gather_columns_samples(c, r0, n_samples, width, cs, nc, ld, PTR, PTR,
                                                                             1 << 20, None),
        "mxm_em_loop_samples_narrow": lambda: lib.mxm_em_loop_samples_narrow(c, r0, n_samples, width, PTR, ld, nc, PTR, PTR, PTR,
                                                                             PTR, PTR, 1e-4, 10, 4, PTR, PTR, 1 << 20, None, STATES),
        "mxm_assign_reads_samples": lambda: lib.mxm_assign_reads_samples(c, r0, n_samples, width, PTR, ld, nc, pm, PTR, PTR, PTR,
                                                                         None, 0.69, PTR, None, PTR, 1 << 20, None),
    }


ALL = ("mxm_votes_samples", "mxm_gather_columns_samples", "mxm_em_loop_samples_narrow", "mxm_assign_reads_samples")
WITH_LD = ALL[1:]
# (what, keyword arguments of _calls, the entries that refuse it, the message after "<entry>: ")
REFUSALS = [
    ("row0 not ascending", dict(row0=(0, 7, 4, 10), n_samples=3, ncol=(2, 3, 1), cols=(0,) * 12, perm=(0,) * 12), ALL,
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has -3 rows)"),
    ("an empty sample", dict(row0=(0, 4, 4, 10), n_samples=3, ncol=(2, 3, 1), cols=(0,) * 12, perm=(0,) * 12), ALL,
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has 0 rows)"),
    ("row0[S] != R", dict(row0=(0, 4, 9), n_samples=2), ALL, "%s: row0[S] = 9, the matrix has 10 rows"),
    ("a quad dictionary", dict(coded=_coded(qrec=PTR), row0=(0, 4, 10), n_samples=2), ALL,
     "%s: a quad dictionary is attached; the batched pass reads the records only"),
    ("a dense rest", dict(coded=_coded(R_rest=2), row0=(0, 4, 10), n_samples=2), ALL,
     "%s: 2 rows without a record (the dense rest): such a sample runs on its own"),
    ("ld = 5", dict(row0=(0, 4, 10), n_samples=2, ld=5), WITH_LD, "%s: ld = 5: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ld = 32", dict(row0=(0, 4, 10), n_samples=2, ld=32), WITH_LD, "%s: ld = 32: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ncol above ld", dict(row0=(0, 4, 10), n_samples=2, ncol=(2, 5)), WITH_LD, "%s: sample 1 has ncol = 5 outside [0, 4]"),
    ("ncol below 0", dict(row0=(0, 4, 10), n_samples=2, ncol=(-1, 3)), WITH_LD, "%s: sample 0 has ncol = -1 outside [0, 4]"),
    ("a column at H", dict(row0=(0, 4, 10), n_samples=2, cols=(1, 2, 0, 0, 5, 128, 7, 0)), ALL[1:2],
     "%s: sample 1, column 1: haplogroup index 128 outside [0, 128)"),
    ("a column below 0", dict(row0=(0, 4, 10), n_samples=2, cols=(-4, 2, 0, 0, 5, 6, 7, 0)), ALL[1:2],
     "%s: sample 0, column 0: haplogroup index -4 outside [0, 128)"),
    ("an ordinal at ncol", dict(row0=(0, 4, 10), n_samples=2, perm=(1, 2, 0, 0, 2, 0, 1, 0)), ALL[3:],
     "%s: sample 0, column 1: contributor ordinal 2 outside [0, 2)"),
]


@pytest.mark.parametrize("what,kw,entries,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_messages(lib, what, kw, entries, message):
    kw = dict(kw)
    coded = kw.pop("coded", _coded())
    calls = _calls(lib, coded, **kw)
    for name in entries:
        assert calls[name]() == -1, (what, name)
        want = message % name if "%s" in message else message
        assert lib.mxm_last_error().decode() == want, (what, name)
