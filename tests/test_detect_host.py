"""
The host side of assign.detect_many -- a bootstrap of the contributor DETECTION -- and of its C entries
(include/mixemt_hip_detect.h): the header against the binding table, every refusal of both entries (all made before the first
HIP call, so no device is needed; the pointers that are not NULL are never followed), detect_many's refusals and skip
reasons, the restated candidate rule (tests/_detect_ref.py) against the Python the reference runs, the summary arithmetic and
the report's text against hand-computed values, and the concavity claim the warm start rests on.
"""
import io
import os
import re

import numpy
import pytest

from mixemt_amd import _lib

import _detect_ref as ref
from test_samples_finish_host import PTR, _i32, _i64, _records, finish_args

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mixemt_hip_detect.h")
CAND, CHECK = "mxm_detect_candidates", "mxm_check_variants_entries"


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import build
    build.build()
    return _lib.load()


def declared():
    """{entry: number of parameters} of the header: test_guarded_complete.declared_entries' parse, over this header."""
    with open(HEADER) as fin:
        text = fin.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for decl in text.split(";"):
        found = re.search(r"\b(mxm_\w+)\s*\(([^)]*)\)", decl)
        if found and "typedef" not in decl.split(found.group(1))[0]:
            out[found.group(1)] = len(found.group(2).split(","))
    return out


def test_the_header_and_the_binding_table_name_the_same_entries(lib):
    names = declared()
    assert set(names) == set(_lib.DETECT_SIGNATURES) == {CAND, CHECK}
    for name, n_args in names.items():
        restype, argtypes = _lib.DETECT_SIGNATURES[name]
        assert len(argtypes) == n_args, name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    for table in (_lib.SIGNATURES, _lib.FINISH_SIGNATURES, _lib.VARCHECK_SIGNATURES, _lib.ASSEMBLE_SAMPLES_SIGNATURES,
                  _lib.STATS_SAMPLES_SIGNATURES, _lib.SAMPLES_RUNS_SIGNATURES, _lib.BOOTSTRAP_SIGNATURES, _lib.SUPPORT_SIGNATURES):
        assert not (set(names) & set(table))
    from test_guarded_complete import declared_entries
    assert not (set(names) & declared_entries())
    with open(HEADER) as fin:
        assert "MXM_VERSION 603: the version stays" in fin.read()
    with open(os.path.join(os.path.dirname(HEADER), "mixemt_hip.h")) as fin:
        assert '#include "mixemt_hip_detect.h"' in fin.read()
    assert lib.mxm_version() == 603 and _lib.ABI_VERSION == 603
    from mixemt_amd import assign, build
    assert HEADER in build.HDRS
    assert assign.DETECT_LD == 64
    # no size function: neither entry takes a workspace
    assert not hasattr(lib, "mxm_detect_workspace_bytes") or "mxm_detect_workspace_bytes" in names


# ---- the C ABI ---------------------------------------------------------------------------------------------------
def _cand_call(lib, E=2, H=70, ld=8, rows=(5, 7), votes=PTR, first=PTR, props=PTR, cand=PTR, ncand=PTR, cprop=PTR, no_rows=False):
    r = None if no_rows else _i64(*rows)
    return lib.mxm_detect_candidates(votes, first, r, props, None, E, H, 3.0, ld, cand, ncand, cprop, None)


LD_MESSAGE = "%s: ld = %d: the candidate tables' row stride must be 4, 8, 16, 32 or 64"
CAND_REFUSALS = [
    ("E < 0", dict(E=-1), CAND + ": E < 0 (-1)"),
    ("H = 0", dict(H=0), CAND + ": H = 0: at least one haplogroup is needed"),
    ("H < 0", dict(H=-4), CAND + ": H = -4: at least one haplogroup is needed"),
    ("ld = 0", dict(ld=0), LD_MESSAGE % (CAND, 0)),
    ("ld = 5", dict(ld=5), LD_MESSAGE % (CAND, 5)),
    ("ld = 128", dict(ld=128), LD_MESSAGE % (CAND, 128)),
    ("a negative row count", dict(rows=(5, -2)), CAND + ": entry 1 has -2 rows"),
] + [("no %s" % name, {name: None}, CAND + ": bad arguments (votes, first, rows_host, props, cand, ncand and cprop are required)")
     for name in ("votes", "first", "props", "cand", "ncand", "cprop")] + [
    ("no rows_host", dict(no_rows=True), CAND + ": bad arguments (votes, first, rows_host, props, cand, ncand and cprop are required)")]


@pytest.mark.parametrize("what,kw,message", CAND_REFUSALS, ids=[r[0] for r in CAND_REFUSALS])
def test_the_candidate_entry_refuses_before_any_pointer_is_followed(lib, what, kw, message):
    assert _cand_call(lib, **kw) == -1, what
    assert lib.mxm_last_error().decode() == message


def _check_call(lib, E=2, T=2, L=100, H=70, ld=8, table_of=(0, 1), counts=PTR, key_ptr=PTR, key=PTR, site=PTR, site_key=PTR, n_sites=3,
                max_pos=50, cand=PTR, ncand=PTR, keep=PTR, flag=PTR, no_table=False):
    t = None if no_table else _i32(*table_of)
    return lib.mxm_check_variants_entries(counts, T, L, key_ptr, key, H, site, site_key, n_sites, max_pos, t, E, cand, ncand, ld, 3.0,
                                          0.02, 0.5, 0, 0, keep, None, None, flag, None)


REQUIRED = CHECK + ": bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)"
LISTS = CHECK + ": bad arguments (table_of_host, cand, ncand and flag are required)"
CHECK_REFUSALS = [
    ("E < 0", dict(E=-1), CHECK + ": E < 0 (-1)"),
    ("ld = 6", dict(ld=6), LD_MESSAGE % (CHECK, 6)),
    ("ld = 2", dict(ld=2), LD_MESSAGE % (CHECK, 2)),
    ("T = 0", dict(T=0), CHECK + ": T = 0: at least one pileup table is needed"),
    ("no table_of_host", dict(no_table=True), LISTS),
    ("no cand", dict(cand=None), LISTS),
    ("no ncand", dict(ncand=None), LISTS),
    ("no flag", dict(flag=None), LISTS),
    ("a table at T", dict(table_of=(0, 2)), CHECK + ": entry 1: table 2 outside [0, 2)"),
    ("a negative table", dict(table_of=(-1, 0)), CHECK + ": entry 0: table -1 outside [0, 2)"),
    ("no counts", dict(counts=None), REQUIRED),
    ("no key_ptr", dict(key_ptr=None), REQUIRED),
    ("no key", dict(key=None), REQUIRED),
    ("no keep", dict(keep=None), REQUIRED),
    ("no site with sites", dict(site=None), REQUIRED),
    ("no site_key with sites", dict(site_key=None), REQUIRED),
    ("counts not aligned", dict(counts=PTR + 4), CHECK + ": counts must be 16-byte aligned"),
    ("L = 0", dict(L=0, max_pos=-1), CHECK + ": bad shape (L = 0, n_sites = 3, H = 70)"),
    ("n_sites < 0", dict(n_sites=-1), CHECK + ": bad shape (L = 100, n_sites = -1, H = 70)"),
    ("H = 0", dict(H=0), CHECK + ": bad shape (L = 100, n_sites = 3, H = 0)"),
    ("max_pos at L", dict(max_pos=100), CHECK + ": max_pos = 100: the tree's variants reach past the pileup (L = 100)"),
    ("L above the cap", dict(L=131073), CHECK + ": L = 131073: a sample's bitsets do not fit the kernel's LDS (L <= 131072)"),
]


@pytest.mark.parametrize("what,kw,message", CHECK_REFUSALS, ids=[r[0] for r in CHECK_REFUSALS])
def test_the_check_entry_refuses_before_any_pointer_is_followed(lib, what, kw, message):
    assert _check_call(lib, **kw) == -1, what
    assert lib.mxm_last_error().decode() == message


def test_no_entries_is_fine_and_launches_nothing(lib):
    assert _cand_call(lib, E=0, votes=None, cand=None, no_rows=True) == 0
    assert _check_call(lib, E=0, T=0, counts=None, no_table=True) == 0
    # ... but the shape is still judged
    assert _cand_call(lib, E=0, ld=5) == -1 and _check_call(lib, E=0, ld=5) == -1


# ---- detect_many's argument errors and skip reasons (all before a device is asked for) ------------------------------------
def _cohort():
    import torch
    rec = torch.zeros(64, dtype=torch.uint8)
    haps = ["h%02d" % i for i in range(66)]
    samples = [(_records(rec, 5), numpy.ones(5)), (_records(rec, 7), numpy.ones(7))]
    props = numpy.full(66, 1.0 / 66)
    results = [{"route": "batch", "props": props}, {"route": "batch", "props": props}]
    done = {"contribs": [["hap1", "h03", 0.7], ["hap2", "h01", 0.3]]}
    return samples, results, [done, dict(done)], haps


def test_detect_many_refuses_bad_arguments_before_it_touches_the_device():
    import torch
    from mixemt_amd import assign
    samples, results, finished, haps = _cohort()
    args = finish_args()
    for bad in (0, 1, 4097, -5):
        with pytest.raises(ValueError, match=r"detect_many: n_boot = %d: 2 \.\. 4096 replicates are taken" % bad):
            assign.detect_many(samples, results, finished, haps, args, n_boot=bad)
    for bad in (0.0, 1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match=r"detect_many: level = .* must lie in \(0, 1\)"):
            assign.detect_many(samples, results, finished, haps, args, level=bad)
    with pytest.raises(ValueError, match=r"one result of run_em_many and one of finish_many per sample are needed \(2 samples, 2 and 1"):
        assign.detect_many(samples, results, finished[:1], haps, args)
    with pytest.raises(ValueError, match=r"per sample are needed \(2 samples, 1 and 2"):
        assign.detect_many(samples, results[:1], finished, haps, args)
    with pytest.raises(ValueError, match="per sample are needed"):
        assign.detect_many([], [], [], haps, args)
    with pytest.raises(ValueError, match=r"sample_ids needs one id per sample \(2 samples, 3 ids\)"):
        assign.detect_many(samples, results, finished, haps, args, sample_ids=[1, 2, 3])
    with pytest.raises(ValueError, match="32-bit unsigned"):
        assign.detect_many(samples, results, finished, haps, args, sample_ids=[1, 2 ** 32])
    with pytest.raises(ValueError, match=r"inits needs one entry per sample \(2 samples, 1 entries\)"):
        assign.detect_many(samples, results, finished, haps, args, inits=[None])
    with pytest.raises(ValueError, match="the start of sample 1 must be 66 finite non-negative proportions"):
        assign.detect_many(samples, results, finished, haps, args, inits=[None, numpy.ones(65)])
    with pytest.raises(ValueError, match="the start of sample 0 must be"):
        assign.detect_many(samples, results, finished, haps, args, inits=[numpy.zeros(66), None])
    with pytest.raises(ValueError, match=r"above the budget of 1000 bytes \(max_bytes\): split the cohort or lower n_boot"):
        assign.detect_many(samples, results, finished, haps, args, n_boot=4, max_bytes=1000)
    with pytest.raises(ValueError, match="detect_many: weights do not match"):
        assign.detect_many([(samples[0][0], numpy.ones(4)), samples[1]], results, finished, haps, args)
    other = (_records(torch.zeros(64, dtype=torch.uint8), 7), numpy.ones(7))
    with pytest.raises(ValueError, match="detect_many: the samples must be views of ONE record buffer"):
        assign.detect_many([samples[0], other], results, finished, haps, args)
    with pytest.raises(ValueError, match="detect_many: 65 haplogroups for matrices of 66 columns"):
        assign.detect_many(samples, results, finished, haps[:65], args)
    # the variant check: a cohort pileup and a tree, nothing else
    checked = finish_args(var_check=True)
    for obs in (None, [object(), object()]):
        with pytest.raises(ValueError, match="args.var_check needs obs= an observe.CohortPileup"):
            assign.detect_many(samples, results, finished, haps, checked, obs=obs, phylo=object())
    from mixemt_amd import observe
    pile = observe.CohortPileup(torch.zeros((2, 40, 16), dtype=torch.int32), [40, 40])
    with pytest.raises(ValueError, match=r"the variant check needs phylo= \(or var_tables=\)"):
        assign.detect_many(samples, results, finished, haps, checked, obs=pile)
    with pytest.raises(ValueError, match=r"obs needs one table per sample \(2 samples, 3 tables\)"):
        assign.detect_many(samples, results, finished, haps, checked, phylo=object(),
                           obs=observe.CohortPileup(torch.zeros((3, 40, 16), dtype=torch.int32), [40] * 3))
    with pytest.raises(ValueError, match="a pileup of 131073 positions"):
        assign.detect_many(samples, results, finished, haps, checked, phylo=object(),
                           obs=observe.CohortPileup(torch.zeros((2, 131073, 16), dtype=torch.int32), [1, 1]))
    from test_var_check_host import toy_tree
    tables = assign.VarCheckTables.build(toy_tree(), list("ABCDEFGHI"))          # (9 haplogroups, no device)
    with pytest.raises(ValueError, match="var_tables must be built with a device for the samples' 66 haplogroups"):
        assign.detect_many(samples, results, finished, haps, checked, obs=pile, var_tables=tables)


def test_samples_that_do_not_take_part_are_skipped_with_a_reason():
    from mixemt_amd import assign
    samples, results, finished, haps = _cohort()
    skip = assign._detect_skip
    assert skip(samples[0], results[0], finish_args()) is None
    assert "did not run in the batch (route 'single')" in skip(samples[0], dict(results[0], route="single"), finish_args())
    assert "args.n_multi = 3" in skip(samples[0], results[0], finish_args(n_multi=3))
    assert "nothing to detect" in skip(samples[0], results[0], finish_args(contributors="h01,h02"))
    for bad in (numpy.array([1, 2, 0.5, 1, 1]), numpy.array([1, 2, -1, 1, 1]), numpy.array([1, 2, numpy.nan, 1, 1])):
        assert "not non-negative integers" in skip((samples[0][0], bad), results[0], finish_args())
    assert "a total in [1, 2^31)" in skip((samples[0][0], numpy.zeros(5)), results[0], finish_args())
    assert "a total in [1, 2^31)" in skip((samples[0][0], numpy.full(5, 2.0 ** 30)), results[0], finish_args())
    # a cohort in which nothing takes part never asks for a device
    single = [dict(r, route="single") for r in results]
    found, skipped = assign.detect_many(samples, single, finished, haps, finish_args())
    assert found == [None, None] and [s for s, _ in skipped] == [0, 1] and all("route 'single'" in why for _, why in skipped)
    found, skipped = assign.detect_many(samples, results, finished, haps, finish_args(contributors="h01"))
    assert found == [None, None] and all("nothing to detect" in why for _, why in skipped)
    one, why = assign.detect(samples[0][0], samples[0][1], single[0], finished[0], haps, finish_args())
    assert one is None and "route 'single'" in why


def test_chunks_are_contiguous_and_within_the_budget():
    from mixemt_amd import assign
    assert assign._detect_chunks([10, 10, 10, 10, 10], 30) == [(0, 3), (3, 5)]
    assert assign._detect_chunks([10, 30, 10], 30) == [(0, 1), (1, 2), (2, 3)]
    assert assign._detect_chunks([7] * 4, 7) == [(0, 1), (1, 2), (2, 3), (3, 4)] and assign._detect_chunks([7] * 4, 10 ** 6) == [(0, 4)]
    with pytest.raises(ValueError, match="one .sample, replicate. entry needs 31 bytes"):
        assign._detect_chunks([10, 31], 30)
    small, large = assign._detect_entry_bytes(33, 5408, 32), assign._detect_entry_bytes(600, 5408, 32)
    assert small >= 2 * 5408 * 8 + 56 * 5408 and large - small >= 17 * 5408 * 8          # tiles, then the vote's and loop's tables


# ---- the restated candidate rule against the Python the reference runs ------------------------------------------------------
def python_route(best, wts, props, min_reads):
    """assemble.py:115-123 and :85-86 as the package's host route runs them: (haplogroups in checking order, proportions)."""
    from mixemt_amd import assign
    votes = numpy.bincount(best, weights=wts, minlength=len(props))
    found = [int(h) for h in assign._first_seen_order(best) if votes[h] >= min_reads]
    contrib_prop = [[h, props[h]] for h in found]
    contrib_prop.sort(key=lambda con: con[1], reverse=True)
    return [c[0] for c in contrib_prop], [c[1] for c in contrib_prop]


def tables_of(best, wts, n_haps):
    votes = numpy.bincount(best, weights=wts, minlength=n_haps)
    first = numpy.full(n_haps, len(best), dtype=numpy.int64)
    for r in range(len(best) - 1, -1, -1):
        first[best[r]] = r
    return votes, first


CRAFTED = [
    # (what, best per row, weights, {haplogroup: proportion} (others 0.01), min_reads)
    ("two bit-equal proportions: first-seen order", [5, 2, 5, 2, 9], [1, 1, 1, 1, 3], {5: 0.25, 2: 0.25, 9: 0.5}, 2),
    ("three bit-equal proportions", [7, 7, 1, 1, 4, 4, 0], [1] * 7, {7: 0.2, 1: 0.2, 4: 0.2, 0: 0.4}, 1),
    ("three equal, seen in descending index", [9, 4, 1, 9, 4, 1], [1] * 6, {9: 0.3, 4: 0.3, 1: 0.3}, 2),
    ("a vote exactly equal to min_reads", [3, 3, 6, 6, 6], [1.5, 1.5, 1, 1, 1], {3: 0.6, 6: 0.4}, 3.0),
    ("a vote just under min_reads", [3, 3, 6, 6, 6], [1.5, 1.5, 1, 1, 1], {3: 0.6, 6: 0.4}, 3.0000000000000004),
    ("min_reads = 0: only row winners", [2, 2, 8], [1, 1, 1], {2: 0.5, 8: 0.3, 5: 0.9}, 0),
    ("min_reads = 0: a winner of weight-0 rows only", [2, 8, 2], [1, 0, 1], {2: 0.5, 8: 0.6}, 0),
    ("nobody reaches min_reads", [1, 2, 3], [1, 1, 1], {}, 2),
]


@pytest.mark.parametrize("what,best,wts,named,min_reads", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_the_restatement_is_the_references_sort_over_the_first_seen_order(what, best, wts, named, min_reads):
    n_haps = 12
    best, wts = numpy.asarray(best), numpy.asarray(wts, dtype=numpy.float64)
    props = numpy.full(n_haps, 0.01)
    for h, p in named.items():
        props[h] = p
    votes, first = tables_of(best, wts, n_haps)
    want = python_route(best, wts, props, min_reads)
    n, cand, cprop = ref.candidates(votes, first, len(best), props, min_reads, 8)
    assert n == len(want[0]) and cand == want[0] and cprop == want[1], what
    if what.startswith("min_reads = 0: only"):
        assert 5 not in cand and votes[5] >= min_reads            # enough votes for the rule, but it never won a row
    if what.startswith("a vote exactly"):
        assert cand == [3, 6] and votes[3] == min_reads
    if what.startswith("a vote just under"):
        assert cand == []
    if "three equal, seen in descending" in what:
        assert cand == [9, 4, 1]
    if "weight-0" in what:
        assert cand == [8, 2]


def test_the_restatement_poisons_and_overflows_as_the_header_says():
    votes, first = numpy.array([4.0, 0.0, 5.0, 6.0]), numpy.array([0, 9, 1, 2])
    props = numpy.array([0.1, 0.2, 0.3, 0.4])
    assert ref.candidates(votes, first, 9, props, 1, 4) == (3, [3, 2, 0], [0.4, 0.3, 0.1])
    assert ref.candidates(votes, first, 9, props, 1, 4, state=(1, 0))[0] == 3
    assert ref.candidates(votes, first, 9, props, 1, 4, state=(0, 0))[0] == -1
    assert ref.candidates(votes, first, 9, props, 1, 4, state=(1, 1))[0] == -1
    assert ref.candidates(numpy.array([4.0, numpy.nan, 5.0, 6.0]), first, 9, props, 1, 4)[0] == -1       # a NaN vote anywhere
    assert ref.candidates(votes, first, 9, numpy.array([0.1, numpy.nan, 0.3, 0.4]), 1, 4)[0] == 3          # ... not a candidate's
    assert ref.candidates(votes, first, 9, numpy.array([numpy.nan, 0.2, 0.3, 0.4]), 1, 4)[0] == -1
    assert ref.candidates(numpy.ones(6), numpy.arange(6), 6, numpy.ones(6), 1, 4) == (6, [], [])


# ---- the summary ----------------------------------------------------------------------------------------------------
HAPS = ["h%d" % i for i in range(8)]
CONTRIBS = [["hap1", "h3", 0.7], ["hap2", "h1", 0.28], ["hap3", "h6", 0.02]]


def hand_made():
    """Seven replicates; 64-wide tables as they leave the device."""
    cand = numpy.zeros((7, 64), dtype=numpy.int32)
    keep = numpy.zeros((7, 64), dtype=bool)
    lists = [([3, 1, 6], [1, 1, 1]), ([3, 1], [1, 1]), ([3, 1, 5], [1, 1, 0]), ([3, 1, 6], [1, 1, 0]), ([1, 3], [1, 1]), ([3], [1]),
             ([3, 1, 6], [1, 1, 1])]
    for b, (c, k) in enumerate(lists):
        cand[b, :len(c)], keep[b, :len(c)] = c, k
    ncand = numpy.array([3, 2, 3, 3, 2, -1, 3], dtype=numpy.int32)
    flag = numpy.array([0, 0, 0, 0, 0, 0, 2], dtype=numpy.int32)
    done = numpy.array([1, 1, 2, 1, 0, 1, 1], dtype=numpy.int32)
    return cand, ncand, keep, flag, done


def test_the_summary_against_hand_computed_values():
    from mixemt_amd import assign
    index = {h: i for i, h in enumerate(HAPS)}
    cand, ncand, keep, flag, done = hand_made()
    got = assign._detect_summary(cand, ncand, keep, flag, done, CONTRIBS, HAPS, index)
    # used: replicates 0 .. 3 (2 stopped by max_iter and counts); 4 did not finish, 5 is poisoned, 6 was flagged
    assert got["n_used"] == 4
    assert got["n_failed"] == {"the EM loop did not finish": 1, "poisoned: a NaN vote or proportion, or a loop error": 1,
                               "a candidate index outside the tree": 1}
    assert got["detection"] == [["h1", 4, 4, True, 0.28], ["h3", 4, 4, True, 0.7], ["h6", 2, 1, True, 0.02], ["h5", 1, 0, False, None]]
    assert got["set_sizes"] == {2: 3, 3: 1} and got["same_set"] == 1
    assert got["sets"] == [(["h1", "h3"], 3), (["h1", "h3", "h6"], 1)]
    assert got == ref.summary(cand, ncand, keep, flag, done, CONTRIBS, HAPS)
    # the check off: every candidate is kept
    off = assign._detect_summary(cand, ncand, None, numpy.zeros(7, dtype=numpy.int32), done, CONTRIBS, HAPS, index)
    assert off["n_used"] == 5 and all(row[1] == row[2] for row in off["detection"])
    assert off["sets"] == [(["h1", "h3", "h6"], 3), (["h1", "h3"], 1), (["h1", "h3", "h5"], 1)] and off["same_set"] == 3
    assert off == ref.summary(cand, ncand, None, numpy.zeros(7, dtype=numpy.int32), done, CONTRIBS, HAPS)
    # more than ten sets: the ten most frequent, ties by first occurrence; more than 64 candidates; a flag of 1
    many = numpy.zeros((14, 64), dtype=numpy.int32)
    many[:12, 0] = [7, 6, 5, 4, 3, 2, 1, 0, 7, 7, 2, 2]
    many[:12, 1] = [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    many[:12, 2] = [1, 1, 1, 1, 1, 1, 2, 2, 1, 1, 1, 1]
    n_many = numpy.array([3] * 12 + [65, 3], dtype=numpy.int32)
    f_many = numpy.array([0] * 13 + [1], dtype=numpy.int32)
    got = assign._detect_summary(many, n_many, None, f_many, numpy.ones(14), [], HAPS, index)
    assert got["n_used"] == 12 and got["n_failed"] == {"more than 64 candidates": 1, "the variant check left it alone (ncand)": 1}
    assert got["sets"] == [(["h0", "h1", "h2"], 5), (["h0", "h1", "h7"], 3), (["h0", "h1", "h6"], 1), (["h0", "h1", "h5"], 1),
                           (["h0", "h1", "h4"], 1), (["h0", "h1", "h3"], 1)]
    assert got["same_set"] == 0 and got == ref.summary(many, n_many, None, f_many, numpy.ones(14), [], HAPS)
    pairs = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6)]
    twelve = numpy.zeros((12, 64), dtype=numpy.int32)
    twelve[:, :2] = pairs
    got = assign._detect_summary(twelve, numpy.full(12, 2), None, numpy.zeros(12), numpy.ones(12), [], HAPS, index)
    assert got["sets"] == [(["h%d" % a, "h%d" % b], 1) for a, b in pairs[:10]] and got["set_sizes"] == {2: 12}
    assert got == ref.summary(twelve, numpy.full(12, 2), None, numpy.zeros(12), numpy.ones(12), [], HAPS)
    # no usable replicate: the estimate's rows with zero counts
    none = assign._detect_summary(cand[:1], numpy.array([-1]), None, numpy.zeros(1), numpy.ones(1), CONTRIBS, HAPS, index)
    assert none["n_used"] == 0 and none["detection"] == [["h1", 0, 0, True, 0.28], ["h3", 0, 0, True, 0.7], ["h6", 0, 0, True, 0.02]]
    assert none["sets"] == [] and none["set_sizes"] == {}


def test_the_reports_text():
    from mixemt_amd import assign, stats
    index = {h: i for i, h in enumerate(HAPS)}
    res = assign._detect_summary(*hand_made(), CONTRIBS, HAPS, index)
    res.update({"n_boot": 7, "var_check": "observed pileup"})
    out = io.StringIO()
    stats.report_detection_many(out, [{"contribs": CONTRIBS}, {"contribs": []}], [res, None], titles=["one", "two"])
    text = out.getvalue()
    first = text.split("\n")[0]
    assert "conditional on the OBSERVED pileup" in first and "stop rule" in first and "not the frequencies of the full pipeline" in first
    assert text == (stats.DETECTION_HEADER + "# one\n# 4 / 7 replicates used; variant check: observed pileup\n"
                    "haplogroup  candidate  kept    freq  estimate\n"
                    "        h1          4     4  1.0000    0.2800\n"
                    "        h3          4     4  1.0000    0.7000\n"
                    "        h6          2     1  0.2500    0.0200\n"
                    "        h5          1     0  0.0000         -\n"
                    "same_set\t1\nset_size\t2\t3\nset_size\t3\t1\nset\th1,h3\t3\nset\th1,h3,h6\t1\n"
                    "failed\tthe EM loop did not finish\t1\nfailed\tpoisoned: a NaN vote or proportion, or a loop error\t1\n"
                    "failed\ta candidate index outside the tree\t1\n"
                    "# two\n# skipped: no detection bootstrap\n")
    with pytest.raises(ValueError, match="one detection result"):
        stats.report_detection_many(io.StringIO(), [{"contribs": []}], [res, None])


# ---- the warm start ------------------------------------------------------------------------------------------------
def test_two_starts_reach_the_same_likelihood():
    """for fixed components the log-likelihood sum_r w_r log sum_h p_h P_rh is concave in p, so EM's fixed
    point does not depend on the start.  40 x 6, long double throughout."""
    rng = numpy.random.RandomState(5)
    lik = numpy.exp(rng.normal(0.0, 2.0, size=(40, 6))).astype(numpy.longdouble)
    wts = rng.randint(0, 4, size=40).astype(numpy.longdouble)

    def fit(p):
        p = numpy.asarray(p, dtype=numpy.longdouble)
        for _ in range(200000):
            mix = lik * p
            nxt = (wts[:, None] * mix / mix.sum(axis=1, keepdims=True)).sum(axis=0) / wts.sum()
            moved = numpy.abs(nxt - p).sum()
            p = nxt
            if moved < 1e-17:
                break
        return p, (wts * numpy.log((lik * p).sum(axis=1))).sum()

    p_a, ll_a = fit(numpy.full(6, 1.0 / 6))
    p_b, ll_b = fit(rng.dirichlet(numpy.ones(6) * 0.3) * (1 - 6e-6) + 1e-6)
    # EM never lowers the likelihood and both runs stopped moving: what is left is the rounding of a 40-term long double sum
    assert abs(ll_a - ll_b) <= 1e-12 * abs(ll_a), (ll_a, ll_b)
    assert numpy.abs(p_a - p_b).max() < 1e-6
