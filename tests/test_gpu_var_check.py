"""
The cohort's variant check on the device -- observe.observe_bases_many (one labelled pileup call for all samples),
mxm_check_variants_samples (csrc/var_check_kernels.hpp) and assign.finish_many(obs=CohortPileup) -- against the
reference's own contributor tables (g16), against assign.check_contrib_phy_vars over the same tables on the host (the
numbers it prints per candidate included), and against the per-sample route of finish_many.
"""
import argparse
import io
import os
import re
import sys

import numpy
import pytest

from conftest import ROOT, em_args, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_observe import _subset  # noqa: E402
from test_observe import VARIANTS, asm_args, g16_columns, want_contribs  # noqa: E402
from test_samples_finish_host import finish_args  # noqa: E402
from test_var_check_host import toy_tree  # noqa: E402

pytestmark = pytest.mark.gpu

TOY = list("ABCDEFGHI")
A, C, G, T = 0, 1, 2, 3           # forward bins; + 7: the reverse strand's


def host_check(phy, table, names, args):
    """[(kept, n_uniq, n_found), ...] of check_contrib_phy_vars over `table` ([L][16]), read from its verbose lines."""
    from mixemt_amd import assign, observe
    verbose = argparse.Namespace(**vars(args))
    verbose.verbose = True
    err, sys.stderr = sys.stderr, io.StringIO()
    try:
        kept = assign.check_contrib_phy_vars(phy, observe.ObservedBases(numpy.asarray(table).astype(numpy.uint32)),
                                             [[name, 0.0] for name in names], verbose)
        text = sys.stderr.getvalue()
    finally:
        sys.stderr = err
    out = []
    for line in text.split("\n"):
        m = re.match(r"(Keeping|Ignoring) '(.*)': (?:only )?(\d+)/(\d+) unique variant bases observed", line)
        if m:
            out.append((m.group(1) == "Keeping", m.group(2), int(m.group(4)), int(m.group(3))))
    assert [o[1] for o in out] == list(names) and [o[1] for o in out if o[0]] == [k[0] for k in kept]
    return [(o[0], o[2], o[3]) for o in out]


def device_check(counts, tab, haps_index, cands, args):
    """The same triples per sample from ONE mxm_check_variants_samples call; counts: numpy or device [S][L][16]."""
    import torch
    from mixemt_amd import assign
    if not isinstance(counts, torch.Tensor):
        counts = torch.from_numpy(numpy.ascontiguousarray(counts, dtype=numpy.int32)).cuda()
    keep, n_uniq, n_found = assign.check_variants_samples(counts, tab, [[haps_index[n] for n in names] for names in cands],
                                                          args, want_counts=True)
    assert keep.shape[1] in (4, 8, 16, 32, 64) and keep.shape == n_uniq.shape == n_found.shape
    for s, names in enumerate(cands):                       # entries past a sample's candidates are left as they were
        assert not keep[s, len(names):].any() and not n_uniq[s, len(names):].any() and not n_found[s, len(names):].any()
    return [[(bool(keep[s, i]), int(n_uniq[s, i]), int(n_found[s, i])) for i in range(len(names))]
            for s, names in enumerate(cands)]


@pytest.fixture(scope="module")
def cohort(b17):
    """g16, its even-numbered fragments and g16 again: their columns, ONE CohortPileup, the tree's tables."""
    from mixemt_amd import assign, observe
    refseq, phy, haps, _ = b17
    g = golden("g16_observe")
    cols = g16_columns(g)
    parts = [cols, _subset(cols, numpy.flatnonzero(cols.frag % 2 == 0)), cols]
    pileup = observe.observe_bases_many(parts, 30, 30, ref_len=len(refseq))
    tab = assign.VarCheckTables.build(phy, haps, pileup.counts.device)
    cand = sorted([int(c) for c in g["candidates"]], key=lambda c: g["props"][c], reverse=True)
    return {"g": g, "parts": parts, "pileup": pileup, "tab": tab, "names": [haps[c] for c in cand],
            "index": {h: i for i, h in enumerate(haps)}}


# ---- 1. the reference's tables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,kw", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_the_references_contributors_and_the_host_checks_numbers(cohort, b17, label, kw):
    _, phy, _, _ = b17
    names, pileup = cohort["names"], cohort["pileup"]
    args = asm_args(**kw)
    got = device_check(pileup.counts, cohort["tab"], cohort["index"], [names] * 3, args)
    want = [w[1] for w in want_contribs(cohort["g"], label)]
    for s in (0, 2):
        assert [n for n, (kept, _, _) in zip(names, got[s]) if kept] == want, (label, s)
    for s in range(3):
        assert got[s] == host_check(phy, pileup.host(s).counts, names, args), (label, s)
    if label == "default":
        assert not all(kept for kept, _, _ in got[0])             # the check drops a candidate: the branch under test


# ---- 2. the pileups ----------------------------------------------------------------------------------------------------
def test_every_samples_table_is_its_own_pileup(cohort, b17):
    from mixemt_amd import observe
    refseq = b17[0]
    pileup = cohort["pileup"]
    assert pileup.n_samples == 3 and tuple(pileup.counts.shape) == (3, pileup.L, 16) and pileup.L == max(pileup.lengths)
    assert (pileup.min_map_qual, pileup.min_base_qual) == (30, 30)
    tables = pileup.counts.cpu().numpy()
    for s, cols in enumerate(cohort["parts"][:2]):
        alone = observe.observe_bases(cols, 30, 30, ref_len=len(refseq))
        n = alone.counts.shape[0]
        assert n == pileup.lengths[s]
        assert numpy.array_equal(tables[s, :n].view(numpy.uint32), alone.counts) and not tables[s, n:].any(), s
        assert numpy.array_equal(pileup.host(s).counts, alone.counts)
    assert numpy.array_equal(tables[2], tables[0]) and tables[1].sum() < tables[0].sum()
    # an empty sample beside a real one, and one alone
    from test_var_check_host import empty_columns
    two = observe.observe_bases_many([empty_columns(), cohort["parts"][1]], 30, 30, ref_len=len(refseq))
    assert not two.counts[0].any() and numpy.array_equal(two.counts[1, :pileup.lengths[1]].cpu().numpy(), tables[1, :pileup.lengths[1]])
    assert two.lengths[0] == len(refseq)


# ---- 3. a sample's result does not depend on its batch ----------------------------------------------------------------------
def test_a_sample_is_the_same_bits_alone_first_or_last(cohort, b17):
    import torch
    from mixemt_amd import assign, observe
    names, idx = cohort["names"], cohort["index"]
    alone = observe.observe_bases_many(cohort["parts"][:1], 30, 30, ref_len=len(b17[0]))
    cand = [idx[n] for n in names]
    for kw in ({}, {"var_count": 1}):
        args = asm_args(**kw)
        one = assign.check_variants_samples(alone.counts, cohort["tab"], [cand], args, want_counts=True)
        three = assign.check_variants_samples(cohort["pileup"].counts, cohort["tab"], [cand, cand[::-1], cand], args,
                                              want_counts=True)
        for a, b in zip(one, three):
            assert a[0].tobytes() == b[0].tobytes() == b[2].tobytes()
    assert torch.equal(alone.counts[0], cohort["pileup"].counts[0, :alone.L])


# ---- 4. the kernel's edges on the toy tree --------------------------------------------------------------------------------
def table(L, cells):
    out = numpy.zeros((L, 16), dtype=numpy.int32)
    for (pos, b), n in cells.items():
        out[pos, b] = n
    return out


# (what, the table's cells, candidates, args, what the reference's rule gives: (kept, n_uniq, n_found) per candidate)
SHARED = {(0, G): 5, (1, T): 5}                                         # I found; of A's other two, 2T is found and 4T is not
TOY_CASES = [
    ("seen == min_var_reads, both strands", {(0, G): 2, (0, G + 7): 1}, ["I"], {}, [(True, 1, 1)]),
    ("seen one below min_var_reads", {(0, G): 2}, ["I"], {}, [(False, 1, 0)]),
    ("seen == total * frac_var_reads", {(0, G): 3, (0, A): 140, (0, T + 7): 7}, ["I"], {}, [(True, 1, 1)]),
    ("seen just under total * frac_var_reads", {(0, G): 3, (0, A): 141, (0, T + 7): 7}, ["I"], {}, [(False, 1, 0)]),
    ("n_found / n_uniq == var_fraction", SHARED, ["I", "A"], {}, [(True, 1, 1), (True, 2, 1)]),
    ("n_found / n_uniq under var_fraction", SHARED, ["I", "A"], {"var_fraction": 0.51}, [(True, 1, 1), (False, 2, 1)]),
    ("var_count = 0 keeps everything", {}, ["H", "A", "B"], {"var_count": 0}, [(True, 3, 0), (True, 3, 0), (True, 5, 0)]),
    ("var_count met below var_fraction", {(0, G): 5}, ["H"], {"var_count": 1}, [(True, 3, 1)]),
    ("all variants claimed: kept", {(0, G): 5, (2, T): 5, (4, T): 5}, ["H", "I"], {}, [(True, 3, 3), (True, 0, 0)]),
    ("a dropped candidate claims nothing", {(0, G): 5, (5, T): 5}, ["H", "F"], {}, [(False, 3, 1), (True, 4, 2)]),
    ("an ancestral base blocks a back-mutation", {(0, G): 5, (4, A): 50, (2, T): 5}, ["I", "C"], {}, [(True, 1, 1), (True, 2, 1)]),
    ("the back-mutation counted when nothing claims it", {(0, G): 5, (4, A): 50, (2, T): 5}, ["C"], {}, [(True, 4, 3)]),
    ("ncand == ld", SHARED, ["I", "A", "H", "F"], {}, None),
    ("five candidates: the next stride", SHARED, ["F", "I", "A", "H", "E"], {}, None),
]


@pytest.mark.parametrize("L", [9, 37])
def test_toy_tree_edges_against_the_host_check(L):
    from mixemt_amd import assign
    phy = toy_tree()
    tab = assign.VarCheckTables.build(phy, TOY, "cuda")
    index = {h: i for i, h in enumerate(TOY)}
    for what, cells, names, kw, want in TOY_CASES:
        args = asm_args(**kw)
        tbl = table(L, cells)
        got = device_check(tbl[None], tab, index, [names], args)[0]
        assert got == host_check(phy, tbl, names, args), what
        if want is not None:
            assert got == want, what
    # S = 3 with another number of candidates each (none; ld of them; one), every sample its own table
    args = asm_args()
    tables = [table(L, {(0, G): 9}), table(L, SHARED), table(L, {(0, G): 5, (2, T): 5, (4, T): 5})]
    cands = [[], ["I", "A", "H", "F"], ["H"]]
    got = device_check(numpy.stack(tables), tab, index, cands, args)
    assert got == [host_check(phy, t, names, args) for t, names in zip(tables, cands)] and got[0] == []
    assert got[2] == [(True, 3, 3)]
    # no candidate anywhere: nothing is launched, nothing is written
    assert device_check(numpy.stack(tables), tab, index, [[], [], []], args) == [[], [], []]


# ---- 5. more keys than the workgroup has threads -----------------------------------------------------------------------------
def test_a_custom_haplogroup_of_600_variants():
    from mixemt_amd import assign, phylotree
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    phy.add_custom_hap("custom", ["A%dC" % (1000 + 3 * i) for i in range(600)])
    haps = sorted(phy.hap_var)
    tab = assign.VarCheckTables.build(phy, haps, "cuda")
    h = haps.index("custom")
    assert tab.key_ptr_h[h + 1] - tab.key_ptr_h[h] == 600
    tbl = numpy.zeros((16569, 16), dtype=numpy.int32)
    for i in range(0, 600, 2):                                  # every other one: 300 found
        tbl[999 + 3 * i, [C, C + 7]] = [2, 1]
    index = {"custom": h}
    assert device_check(tbl[None], tab, index, [["custom"]], asm_args()) == [[(True, 600, 300)]]
    assert device_check(tbl[None], tab, index, [["custom"]], asm_args(var_fraction=0.5000001)) == [[(False, 600, 300)]]
    assert host_check(phy, tbl, ["custom"], asm_args(var_fraction=0.5000001)) == [(False, 600, 300)]


# ---- 6. finish_many ------------------------------------------------------------------------------------------------------
def test_finish_many_device_route_equals_the_per_sample_route(cohort, b17, monkeypatch):
    from mixemt_amd import alignments, assign, em, observe, preprocess
    refseq, phy, haps, tables = b17
    g, parts, pileup = cohort["g"], cohort["parts"], cohort["pileup"]
    encs = [alignments.encode_alignments(_subset(c, numpy.flatnonzero(c.ref_start >= 0)), tables.sites, len(refseq), 30, 30)
            for c in parts]
    cm, row0 = preprocess.build_em_records_many(tables, [(e.row_ptr, e.site, e.obs) for e in encs])
    samples = [(cm.rows(row0[s], row0[s + 1]), e.weights.astype(numpy.float64)) for s, e in enumerate(encs)]
    numpy.random.seed(int(g["seeds"][1]))
    results = em.run_em_many(samples, em_args())
    args = finish_args(var_check=True)

    def run(obs, **kw):
        numpy.random.seed(3)
        return assign.finish_many(samples, results, haps, finish_args(var_check=True, **kw), phylo=phy, obs=obs)

    dev = run(pileup)
    host = run([observe.observe_bases(c, 30, 30, ref_len=len(refseq)) for c in parts])
    for s, (a, b) in enumerate(zip(dev, host)):
        assert a["contribs"] == b["contribs"] and len(a["contribs"]) >= 1, s
        assert numpy.array_equal(a["row_label"], b["row_label"]) and list(a["vote_order"]) == list(b["vote_order"]), s
        assert a["refined"]["iters"] == b["refined"]["iters"], s
        assert a["refined"]["props"].tobytes() == b["refined"]["props"].tobytes(), s
        assert (a["var_check"], b["var_check"]) == ("device", "host") and a["route"] == b["route"], s
    assert [c[1] for c in dev[0]["contribs"]] == [w[1] for w in want_contribs(g, "default")]
    # reused tables: the same result
    numpy.random.seed(3)
    again = assign.finish_many(samples, results, haps, args, phylo=phy, obs=pileup, var_tables=cohort["tab"])
    assert [r["contribs"] for r in again] == [r["contribs"] for r in dev] and again[1]["var_check"] == "device"

    # verbose: the host's check, with the reference's lines
    err, sys.stderr = sys.stderr, io.StringIO()
    try:
        loud = run(pileup, verbose=True)
        text = sys.stderr.getvalue()
    finally:
        sys.stderr = err
    assert [r["var_check"] for r in loud] == ["host"] * 3 and text.startswith(str(g["verbose_text"]))
    assert [r["contribs"] for r in loud] == [r["contribs"] for r in dev]

    # given contributors switch the check off: nothing of it runs
    def never(*a, **k):
        raise AssertionError("the variant check ran")

    monkeypatch.setattr(assign, "check_variants_samples", never)
    monkeypatch.setattr(assign, "check_contrib_phy_vars", never)
    monkeypatch.setattr(pileup, "host", never)
    fixed = run(pileup, contributors="A12a")
    assert [r["var_check"] for r in fixed] == [None] * 3 and [c[1] for c in fixed[0]["contribs"]] == ["A12a"]


def test_finish_many_batch_route_samples_take_the_device_check(b17):
    """Samples on the batch route of both halves.  Alignment samples tend to hold a few rows without a record (the
    per-sample route), so the rows come from synth_reads and the pileups from synth_alignments of the same three
    contributors: what is compared is the two routes of the check over the same candidates and the same pileups."""
    from mixemt_amd import assign, em, observe, preprocess, synth
    refseq, phy, haps, tables = b17
    parts = [synth.synth_alignments(tables, refseq, n, seed=40 + s) for s, n in enumerate((300, 60, 450))]
    csr = [synth.synth_reads(tables, len(refseq), n, seed=50 + s)[:3] for s, n in enumerate((400, 90, 600))]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    samples = [(cm.rows(row0[s], row0[s + 1]), numpy.ones(int(row0[s + 1] - row0[s]))) for s in range(3)]
    numpy.random.seed(11)
    results = em.run_em_many(samples, em_args())
    pileup = observe.observe_bases_many(parts, 30, 30, ref_len=len(refseq))
    each = [observe.observe_bases(c, 30, 30, ref_len=len(refseq)) for c in parts]
    for kw in ({}, {"min_var_reads": 10}, {"refine_ests": False}):
        numpy.random.seed(3)
        dev = assign.finish_many(samples, results, haps, finish_args(var_check=True, **kw), phylo=phy, obs=pileup)
        numpy.random.seed(3)
        host = assign.finish_many(samples, results, haps, finish_args(var_check=True, **kw), phylo=phy, obs=each)
        for s, (a, b) in enumerate(zip(dev, host)):
            assert (a["route"], b["route"], a["var_check"], b["var_check"]) == ("batch", "batch", "device", "host"), (kw, s)
            assert a["contribs"] == b["contribs"] and numpy.array_equal(a["row_label"], b["row_label"]), (kw, s)
            if a["refined"] is not None:
                assert a["refined"]["props"].tobytes() == b["refined"]["props"].tobytes(), (kw, s)
    # the check off: neither route is named
    plain = assign.finish_many(samples, results, haps, finish_args(var_check=False), obs=pileup)
    assert [r["var_check"] for r in plain] == [None] * 3


# ---- 7. dynamic LDS above 64 KiB: the bitsets' last words ----------------------------------------------------------------------
def lds_bytes(L):
    """vchk_lds_bytes (csrc/var_check_kernels.hpp), restated: the `used` bitset over 4 L keys, `touched` over L positions,
    two tally words."""
    return ((4 * L + 31) // 32 + (L + 31) // 32 + 2) * 4


def long_reference_lengths():
    """(the cap MXM_VAR_CHECK_MAX_L, the first L whose workgroup needs more than 64 KiB): both run the opt-in path."""
    with open(os.path.join(ROOT, "include", "mixemt_hip_var_check.h")) as src:
        cap = int(re.search(r"#define\s+MXM_VAR_CHECK_MAX_L\s+(\d+)", src.read()).group(1))
    first = next(L for L in range(1, cap + 1) if lds_bytes(L) > 64 * 1024)
    assert lds_bytes(first - 1) <= 64 * 1024 < lds_bytes(first) < lds_bytes(cap) and first < cap
    return cap, first


def end_tree(L):
    """The toy tree with its last two variant positions (B's A8T, D's A9T) moved to the LAST two positions of a reference
    of L bases: two variant sites and two candidates' variants in the last word of both bitsets."""
    from mixemt_amd import phylotree
    rows = [r.replace("A8T", "A%dT" % (L - 1)).replace("A9T", "A%dT" % L) for r in phylotree.example_rows()]
    phy = phylotree.Phylotree(rows)
    phy.refseq = "A" * L
    assert sorted(phy.get_variant_pos())[-2:] == [L - 2, L - 1]
    return phy


def end_cases(L):
    """(what, cells, candidates, args) at the end of the reference; the expected triples are the host check's."""
    e1, e2 = L - 1, L - 2
    return [("the last position found", {(e1, T): 5}, ["D"], {"var_count": 1}),
            ("the last position missing", {(2, T): 5, (4, T): 5, (6, T): 5}, ["D"], {"var_fraction": 0.8}),
            ("both last positions, the shared ones claimed first", {(0, G): 5, (2, T): 5, (4, T): 5, (e2, T): 5, (e1, T): 5}, ["H", "B", "D"], {}),
            ("the last two sites claimed as ancestral", {(0, G): 5, (e2, A): 50, (e1, A + 7): 50}, ["I", "B", "D"], {}),
            ("seen == min_var_reads on the last row of the table", {(e1, T): 2, (e1, T + 7): 1, (e2, T + 7): 3}, ["D", "B"], {"var_count": 1})]


@pytest.mark.parametrize("which", [0, 1], ids=["the cap", "just above 64 KiB"])
def test_toy_tree_with_more_than_64k_of_lds(which):
    from mixemt_amd import assign
    L = long_reference_lengths()[which]
    phy = end_tree(L)
    tab = assign.VarCheckTables.build(phy, TOY, "cuda")
    assert tab.max_pos == L - 1
    index = {h: i for i, h in enumerate(TOY)}
    cases = [c[:4] for c in TOY_CASES if not ({"B", "D"} & set(c[2]))] + end_cases(L)
    for what, cells, names, kw in cases:
        args = asm_args(**kw)
        tbl = table(L, cells)
        got = device_check(tbl[None], tab, index, [names], args)[0]
        assert got == host_check(phy, tbl, names, args), (L, what)
    assert device_check(table(L, {(L - 1, T): 5})[None], tab, index, [["D"]], asm_args(var_count=1))[0] == [(True, 5, 1)]
    # S = 3, every sample its own table (8 MiB each at the cap) and its own number of candidates
    args = asm_args()
    picked = [end_cases(L)[2], end_cases(L)[3], ("one", {(L - 2, T): 9}, ["B"], {})]
    tables = [table(L, c[1]) for c in picked]
    got = device_check(numpy.stack(tables), tab, index, [c[2] for c in picked], args)
    assert got == [host_check(phy, t, c[2], args) for t, c in zip(tables, picked)]
