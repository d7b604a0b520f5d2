"""
The detection bootstrap on the device (include/mixemt_hip_detect.h; assign.detect_many):
  1. mxm_detect_candidates against the restated rule (tests/_detect_ref.py), bit for bit, on hand-made tables with no records;
  2. mxm_check_variants_entries over device lists against mxm_check_variants_samples over the same lists (the cohort and
     the toy tree of tests/test_gpu_var_check.py), shared tables, reversed tables and the three flag values;
  3. assign.detect_many end to end: every (sample, replicate) against the per-sample route under the replicate's weights --
     run_em_many([(cm_s, wb_sb)], inits=start) followed by finish_many with that sample's pileup.
"""
import ctypes
import os
import sys

import numpy
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _detect_ref as ref  # noqa: E402
from test_gpu_var_check import G, T, TOY, TOY_CASES, cohort, end_cases, end_tree, host_check, long_reference_lengths, table  # noqa: E402,F401
from test_observe import asm_args  # noqa: E402
from test_samples_finish_host import finish_args  # noqa: E402
from test_var_check_host import toy_tree  # noqa: E402

pytestmark = pytest.mark.gpu

F8, I8, I4 = numpy.float64, numpy.int64, numpy.int32


def sentinel(shape, dtype):
    out = numpy.empty(shape, dtype=dtype)
    out.view(numpy.uint8).reshape(-1)[:] = 0xFF
    return out


def is_sentinel(values):
    return bool((numpy.ascontiguousarray(values).view(numpy.uint8) == 0xFF).all())


# ---- 1. the candidate rule ------------------------------------------------------------------------------------------------
def make_entry(kind, n_haps, ld, rng):
    """One entry's (votes [H], first [H], R, props [H], state or None, min_reads is 3.0 throughout)."""
    n_rows = max(n_haps, 1) + 7
    votes, first = numpy.zeros(n_haps), numpy.full(n_haps, n_rows, dtype=I8)
    props = rng.dirichlet(numpy.ones(n_haps)) if n_haps > 1 else numpy.ones(1)
    want = {"random": min(n_haps, 3), "none": 0, "ties": min(n_haps, 3), "exactly ld": ld, "ld + 1": ld + 1, "nan vote": min(n_haps, 2),
            "error state": min(n_haps, 2), "not done": min(n_haps, 2), "nan prop": min(n_haps, 2), "below and at": min(n_haps, 4),
            "no row won": min(n_haps, 2)}[kind]
    winners = rng.permutation(n_haps)[:want]
    rows = rng.permutation(n_rows)[:want]
    first[winners] = rows
    votes[winners] = 3.0 + rng.integers(0, 5, size=want)
    state = (1, 0)
    if kind == "none":
        extra = rng.permutation(n_haps)[:min(n_haps, 5)]
        first[extra] = rng.permutation(n_rows)[:len(extra)]
        votes[extra] = 2.5                                          # they won rows, with too few reads
    elif kind == "ties" and want >= 2:
        props[winners] = props[winners[0]]                          # bit-equal: the order is first's
    elif kind == "nan vote":
        votes[int(rng.integers(0, n_haps))] = numpy.nan             # anywhere, a candidate or not
    elif kind == "error state":
        state = (1, 1)
    elif kind == "not done":
        state = (0, 0)
    elif kind == "nan prop":
        props[winners[-1]] = numpy.nan
    elif kind == "below and at" and want >= 2:
        votes[winners[0]] = 3.0                                     # exactly min_reads: a candidate
        votes[winners[1]] = numpy.nextafter(3.0, 0.0)               # one ulp below: not one
    elif kind == "no row won":
        others = [h for h in range(n_haps) if h not in set(winners.tolist())][:2]
        votes[others] = 50.0                                        # votes enough, first == R: not in the reference's table
    return votes, first, n_rows, props, state


KINDS = ["random", "none", "ties", "exactly ld", "ld + 1", "nan vote", "error state", "not done", "nan prop", "below and at", "no row won"]


def entries_for(n_haps, ld, seed):
    rng = numpy.random.default_rng(seed)
    kinds = [k for k in KINDS if not (k in ("exactly ld", "ld + 1") and n_haps < ld + 1)]
    return kinds, [make_entry(k, n_haps, ld, rng) for k in kinds]


def run_candidates(lib, entries, ld, with_state=True, min_reads=3.0):
    """One mxm_detect_candidates call over the entries -> (ncand [E], cand [E][ld], cprop [E][ld]); outputs start as 0xFF."""
    import torch
    from mixemt_amd import _lib
    n = len(entries)
    votes = torch.from_numpy(numpy.stack([e[0] for e in entries])).cuda()
    first = torch.from_numpy(numpy.stack([e[1] for e in entries])).cuda()
    props = torch.from_numpy(numpy.stack([e[3] for e in entries])).cuda()
    rows = numpy.array([e[2] for e in entries], dtype=I8)
    state = (_lib.EmState * n)()
    for i, e in enumerate(entries):
        state[i].done, state[i].error = e[4]
    state_d = torch.from_numpy(numpy.frombuffer(bytes(state), dtype=numpy.uint8).copy()).cuda()
    cand = torch.from_numpy(sentinel((n, ld), I4)).cuda()
    ncand = torch.from_numpy(sentinel(n, I4)).cuda()
    cprop = torch.from_numpy(sentinel((n, ld), F8)).cuda()
    rc = lib.mxm_detect_candidates(votes.data_ptr(), first.data_ptr(), rows.ctypes.data, props.data_ptr(),
                                   state_d.data_ptr() if with_state else None, n, votes.shape[1], min_reads, ld, cand.data_ptr(),
                                   ncand.data_ptr(), cprop.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mxm_last_error()
    rows[:] = -5                                                    # (class B: the table may change once the call has returned)
    torch.cuda.synchronize()
    return ncand.cpu().numpy(), cand.cpu().numpy(), cprop.cpu().numpy()


def check_against_the_restatement(entries, kinds, got, ld, with_state=True, min_reads=3.0):
    ncand, cand, cprop = got
    for i, (votes, first, n_rows, props, state) in enumerate(entries):
        n, want_c, want_p = ref.candidates(votes, first, n_rows, props, min_reads, ld, state if with_state else None)
        assert ncand[i] == n, (kinds[i], i, ncand[i], n)
        if 0 <= n <= ld:
            assert cand[i, :n].tolist() == want_c, (kinds[i], i)
            assert cprop[i, :n].tobytes() == numpy.array(want_p, dtype=F8).tobytes(), (kinds[i], i)
            assert is_sentinel(cand[i, n:]) and is_sentinel(cprop[i, n:]), "slots past ncand were written (%s)" % kinds[i]


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("ld", [4, 64])
@pytest.mark.parametrize("n_haps", [1, 65, 66, 5408])
def test_candidates_equal_the_restatement_bit_for_bit(lib, n_haps, ld):
    kinds, entries = entries_for(n_haps, ld, 1000 * ld + n_haps)
    assert len(entries) >= 9
    expect = {k: ref.candidates(*e[:4], 3.0, ld, e[4])[0] for k, e in zip(kinds, entries)}
    assert expect["nan vote"] == expect["error state"] == expect["not done"] == expect["nan prop"] == -1 and expect["none"] == 0
    if n_haps > ld + 1:
        assert expect["exactly ld"] == ld and expect["ld + 1"] == ld + 1
    check_against_the_restatement(entries, kinds, run_candidates(lib, entries, ld), ld)                 # E = 9 .. 11
    check_against_the_restatement(entries[:5], kinds[:5], run_candidates(lib, entries[:5], ld), ld)     # E = 5
    for i in range(len(entries)):                                                                       # E = 1
        check_against_the_restatement(entries[i:i + 1], kinds[i:i + 1], run_candidates(lib, entries[i:i + 1], ld), ld)
    # without a state the two entries it refused are candidates' lists like any other
    got = run_candidates(lib, entries, ld, with_state=False)
    check_against_the_restatement(entries, kinds, got, ld, with_state=False)
    assert got[0][kinds.index("error state")] >= 0 and got[0][kinds.index("not done")] >= 0


def test_the_ties_of_the_host_test_come_out_in_first_seen_order(lib):
    """The crafted cases of tests/test_detect_host.py through the kernel: Python's sort over the first-seen order."""
    from test_detect_host import CRAFTED, python_route, tables_of
    for what, best, wts, named, min_reads in CRAFTED:
        best, wts = numpy.asarray(best), numpy.asarray(wts, dtype=F8)
        props = numpy.full(12, 0.01)
        for h, p in named.items():
            props[h] = p
        votes, first = tables_of(best, wts, 12)
        ncand, cand, cprop = run_candidates(lib, [(votes, first, len(best), props, (1, 0))], 8, min_reads=float(min_reads))
        want = python_route(best, wts, props, min_reads)
        assert ncand[0] == len(want[0]) and cand[0, :ncand[0]].tolist() == want[0], what
        assert cprop[0, :ncand[0]].tobytes() == numpy.array(want[1], dtype=F8).tobytes(), what


def test_an_entry_is_the_same_bits_alone_first_and_last(lib):
    kinds, entries = entries_for(5408, 64, 77)
    for k in ("ties", "exactly ld", "ld + 1", "nan prop"):
        x = entries[kinds.index(k)]
        a, b = entries[kinds.index("random")], entries[kinds.index("none")]
        alone, head, tail = (run_candidates(lib, batch, 64) for batch in ([x], [x, a, b], [a, b, x]))
        n = alone[0][0]
        assert head[0][0] == tail[0][2] == n, k
        if 0 <= n <= 64:
            for t in (1, 2):
                assert alone[t][0, :n].tobytes() == head[t][0, :n].tobytes() == tail[t][2, :n].tobytes(), k


# ---- 2. the check over device lists --------------------------------------------------------------------------------------
def entries_check(counts, tab, cand_rows, ncand, table_of, args, ld):
    """One mxm_check_variants_entries call; cand_rows [E][ld] / ncand [E] go to the device as they are.  Outputs start
    as 0xFF.  -> keep [E][ld] uint8, n_uniq, n_found [E][ld] int32, flag [E]."""
    import torch
    from mixemt_amd import _lib
    lib = _lib.load()
    if not isinstance(counts, torch.Tensor):
        counts = torch.from_numpy(numpy.ascontiguousarray(counts, dtype=I4)).cuda()
    n = len(ncand)
    cand_d = torch.from_numpy(numpy.ascontiguousarray(cand_rows, dtype=I4)).cuda()
    ncand_d = torch.from_numpy(numpy.ascontiguousarray(ncand, dtype=I4)).cuda()
    keep = torch.from_numpy(sentinel((n, ld), numpy.uint8)).cuda()
    uniq, found = torch.from_numpy(sentinel((n, ld), I4)).cuda(), torch.from_numpy(sentinel((n, ld), I4)).cuda()
    flag = torch.from_numpy(sentinel(n, I4)).cuda()
    table_h = numpy.ascontiguousarray(table_of, dtype=I4)
    var_count = getattr(args, "var_count", None)
    rc = lib.mxm_check_variants_entries(counts.data_ptr(), int(counts.shape[0]), int(counts.shape[1]), tab.key_ptr.data_ptr(),
                                        tab.key.data_ptr(), tab.n_haps, tab.site.data_ptr(), tab.site_key.data_ptr(), len(tab.site_h),
                                        tab.max_pos, table_h.ctypes.data, n, cand_d.data_ptr(), ncand_d.data_ptr(), ld,
                                        float(args.min_var_reads), float(args.frac_var_reads), float(args.var_fraction),
                                        0 if var_count is None else 1, 0 if var_count is None else int(var_count), keep.data_ptr(),
                                        uniq.data_ptr(), found.data_ptr(), flag.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mxm_last_error()
    table_h[:] = 0
    torch.cuda.synchronize()
    return keep.cpu().numpy(), uniq.cpu().numpy(), found.cpu().numpy(), flag.cpu().numpy()


def lists_to_rows(lists, ld):
    rows = numpy.zeros((len(lists), ld), dtype=I4)
    for e, c in enumerate(lists):
        rows[e, :len(c)] = c
    return rows, numpy.array([len(c) for c in lists], dtype=I4)


def same_as_the_samples_entry(counts_for_samples, counts, tab, lists, table_of, args, what):
    """The entries call over `counts` / table_of against mxm_check_variants_samples over counts_for_samples [E][L][16]."""
    from mixemt_amd import assign
    want = assign.check_variants_samples(counts_for_samples, tab, lists, args, want_counts=True)
    ld = want[0].shape[1]
    rows, ncand = lists_to_rows(lists, ld)
    keep, uniq, found, flag = entries_check(counts, tab, rows, ncand, table_of, args, ld)
    assert flag.tolist() == [0] * len(lists), what
    for e, c in enumerate(lists):
        n = len(c)
        assert keep[e, :n].astype(bool).tolist() == want[0][e, :n].tolist(), (what, e)
        assert uniq[e, :n].tobytes() == want[1][e, :n].tobytes() and found[e, :n].tobytes() == want[2][e, :n].tobytes(), (what, e)
        assert is_sentinel(keep[e, n:]) and is_sentinel(uniq[e, n:]) and is_sentinel(found[e, n:]), (what, e)
    return keep


def test_the_check_over_device_lists_equals_the_samples_entry(cohort):      # noqa: F811
    counts, tab, idx = cohort["pileup"].counts, cohort["tab"], cohort["index"]
    cand = [idx[n] for n in cohort["names"]]
    assert len(cand) >= 3
    lists = [cand, cand[::-1], cand[1:]]
    for kw in ({}, {"var_count": 1}, {"min_var_reads": 10}):
        args = asm_args(**kw)
        keep = same_as_the_samples_entry(counts, counts, tab, lists, [0, 1, 2], args, "own tables %r" % (kw,))
        if not kw:
            assert not keep[0, :len(cand)].all() and keep[0, :len(cand)].any()          # the check drops one and keeps one
        # three entries over ONE table under different lists
        one = counts[1:2].expand(3, -1, -1).contiguous()
        same_as_the_samples_entry(one, counts, tab, lists, [1, 1, 1], args, "one table %r" % (kw,))
        # entries in reversed table order
        same_as_the_samples_entry(counts.flip(0).contiguous(), counts, tab, lists, [2, 1, 0], args, "reversed %r" % (kw,))
    # an empty list beside full ones: checked trivially
    same_as_the_samples_entry(counts, counts, tab, [cand, [], cand[:1]], [0, 1, 2], asm_args(), "an empty list")


def test_flags_leave_the_entry_alone_and_its_neighbours_intact(cohort):      # noqa: F811
    counts, tab, idx = cohort["pileup"].counts, cohort["tab"], cohort["index"]
    cand = [idx[n] for n in cohort["names"]]
    ld, args = 8, asm_args()
    assert len(cand) <= ld
    good, good_n = lists_to_rows([cand] * 5, ld)
    want = entries_check(counts, tab, good, good_n, [0] * 5, args, ld)
    assert want[3].tolist() == [0] * 5
    rows, ncand = good.copy(), good_n.copy()
    ncand[1], ncand[3] = -1, ld + 1                                 # a poisoned entry; one with too many candidates
    keep, uniq, found, flag = entries_check(counts, tab, rows, ncand, [0] * 5, args, ld)
    assert flag.tolist() == [0, 1, 0, 1, 0]
    rows[2, len(cand) - 1] = tab.n_haps                             # the first index that is no haplogroup
    rows[4, 0] = -1
    keep2, uniq2, found2, flag2 = entries_check(counts, tab, rows, good_n, [0] * 5, args, ld)
    assert flag2.tolist() == [0, 0, 2, 0, 2]
    for got, bad in (((keep, uniq, found), (1, 3)), ((keep2, uniq2, found2), (2, 4))):
        for e in range(5):
            for t in range(3):
                if e in bad:
                    assert is_sentinel(got[t][e]), "a flagged entry was written (%d)" % e
                else:
                    assert got[t][e].tobytes() == want[t][e].tobytes(), "the neighbour %d of a flagged entry changed" % e


def test_toy_tree_edges_through_the_entries_call():
    from mixemt_amd import assign
    L = 64
    phy = toy_tree()
    tab = assign.VarCheckTables.build(phy, TOY, "cuda")
    index = {h: i for i, h in enumerate(TOY)}
    for what, cells, names, kw, want in TOY_CASES:
        args = asm_args(**kw)
        tbl = table(L, cells)
        ld = 4 if len(names) <= 4 else 8
        rows, ncand = lists_to_rows([[index[n] for n in names]], ld)
        keep, uniq, found, flag = entries_check(tbl[None], tab, rows, ncand, [0], args, ld)
        got = [(bool(keep[0, i]), int(uniq[0, i]), int(found[0, i])) for i in range(len(names))]
        assert flag[0] == 0 and got == host_check(phy, tbl, names, args), what
        if want is not None:
            assert got == want, what
    # every case as an entry of ONE call, each over its own table
    args = asm_args()
    plain = [c for c in TOY_CASES if not c[3]]
    tables = numpy.stack([table(L, c[1]) for c in plain])
    rows, ncand = lists_to_rows([[index[n] for n in c[2]] for c in plain], 8)
    keep, uniq, found, flag = entries_check(tables, tab, rows, ncand, list(range(len(plain))), args, 8)
    for e, c in enumerate(plain):
        got = [(bool(keep[e, i]), int(uniq[e, i]), int(found[e, i])) for i in range(len(c[2]))]
        assert flag[e] == 0 and got == host_check(phy, tables[e], c[2], args), c[0]


@pytest.mark.parametrize("which", [0, 1], ids=["the cap", "just above 64 KiB"])
def test_entries_call_with_more_than_64k_of_lds(which):
    """check_variants_entries_kernel on the opt-in path (tests/test_gpu_var_check.py, section 7): the toy tree with variant
    sites and candidates' variants at the last two positions of a reference of L bases; three entries, each its own table."""
    from mixemt_amd import assign
    L = long_reference_lengths()[which]
    phy = end_tree(L)
    tab = assign.VarCheckTables.build(phy, TOY, "cuda")
    index = {h: i for i, h in enumerate(TOY)}
    cases = [c for c in end_cases(L) if not c[3]] + [("one", {(0, G): 9, (2, T): 9, (4, T): 9, (L - 2, T): 9, (L - 1, T + 7): 9}, ["B", "D", "H"], {})]
    assert len(cases) == 3
    args = asm_args()
    tables = numpy.stack([table(L, c[1]) for c in cases])
    rows, ncand = lists_to_rows([[index[n] for n in c[2]] for c in cases], 4)
    keep, uniq, found, flag = entries_check(tables, tab, rows, ncand, [0, 1, 2], args, 4)
    for e, c in enumerate(cases):
        got = [(bool(keep[e, i]), int(uniq[e, i]), int(found[e, i])) for i in range(len(c[2]))]
        assert flag[e] == 0 and got == host_check(phy, tables[e], c[2], args), (L, c[0])
        assert is_sentinel(keep[e, len(c[2]):])
    # ... and the argument-carrying cases one entry at a time
    for what, cells, names, kw in end_cases(L):
        if kw:
            tbl = table(L, cells)
            rows, ncand = lists_to_rows([[index[n] for n in names]], 4)
            keep, uniq, found, flag = entries_check(tbl[None], tab, rows, ncand, [0], asm_args(**kw), 4)
            got = [(bool(keep[0, i]), int(uniq[0, i]), int(found[0, i])) for i in range(len(names))]
            assert flag[0] == 0 and got == host_check(phy, tbl, names, asm_args(**kw)), (L, what)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------
N_BOOT, SEED, MIN_READS = 4, 12345, 2


@pytest.fixture(scope="module")
def small(b17):
    """Three small samples (33 rows: two tiles, the second of one row; a single row; 90 reads' rows), integer weights above 1
    among them, and a fourth whose weights are not integers; their pileups; the first EM's results and finish_many's."""
    from mixemt_amd import assign, em, observe, preprocess, synth
    refseq, phy, haps, tables = b17
    csr = [synth.synth_reads(tables, len(refseq), n, seed=60 + s)[:3] for s, n in enumerate((60, 9, 90, 40))]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    spans = [(row0[0], row0[0] + 33), (row0[1], row0[1] + 1), (row0[2], row0[3]), (row0[3], row0[4])]
    rng = numpy.random.default_rng(9)
    samples = []
    for s, (lo, hi) in enumerate(spans):
        wts = rng.integers(1, 4, size=int(hi - lo)).astype(F8)
        samples.append((cm.rows(int(lo), int(hi)), wts + 0.5 if s == 3 else wts))
    assert [m.n_rows for m, _ in samples][:2] == [33, 1]
    numpy.random.seed(21)
    results = em.run_em_many(samples, finish_args())
    assert [r["route"] for r in results] == ["batch"] * 4
    parts = [synth.synth_alignments(tables, refseq, n, seed=70 + s) for s, n in enumerate((200, 60, 300, 100))]
    pileup = observe.observe_bases_many(parts, 30, 30, ref_len=len(refseq))
    tab = assign.VarCheckTables.build(phy, haps, pileup.counts.device)
    finished = {}
    for checked in (False, True):
        args = finish_args(var_check=checked, min_reads=MIN_READS, refine_ests=False)
        finished[checked] = assign.finish_many(samples, results, haps, args, phylo=phy, obs=pileup, var_tables=tab)
    return {"samples": samples, "results": results, "pileup": pileup, "tab": tab, "finished": finished, "haps": haps, "phy": phy}


def detect(small, checked, **kw):
    from mixemt_amd import assign
    args = finish_args(var_check=checked, min_reads=MIN_READS)
    kw.setdefault("n_boot", N_BOOT)
    return assign.detect_many(small["samples"], small["results"], small["finished"][checked], small["haps"], args, seed=SEED,
                              obs=small["pileup"] if checked else None, phylo=small["phy"], var_tables=small["tab"] if checked else None,
                              **kw)


@pytest.fixture(scope="module")
def detected(small):
    return {checked: detect(small, checked) for checked in (False, True)}


def same_replicates(a, b, n, what):
    for key in ("cand", "ncand", "keep", "flag", "cand_props", "iters", "done", "props_boot"):
        assert numpy.ascontiguousarray(a[key][:n]).tobytes() == numpy.ascontiguousarray(b[key][:n]).tobytes(), (what, key)


def test_every_replicate_equals_the_per_sample_route(small, detected):
    import torch
    from mixemt_amd import assign, em, observe
    samples, results, haps, pileup = small["samples"], small["results"], small["haps"], small["pileup"]
    ids = [0, 1, 2]
    wts_d = {s: torch.from_numpy(samples[s][1]).cuda() for s in ids}
    wb, errors = assign._finish_batch(samples, wts_d, ids).boot_weights(N_BOOT, SEED, ids)
    assert not any(errors)
    wb = wb.cpu().numpy()
    row0 = numpy.concatenate([[0], numpy.cumsum([samples[s][0].n_rows for s in ids])])
    n_zero = 0
    for s in ids:
        cm, n_rows = samples[s][0], samples[s][0].n_rows
        start = numpy.asarray(results[s]["props"], dtype=F8)
        start = start / start.sum()
        one_table = observe.CohortPileup(pileup.counts[s:s + 1].contiguous(), [pileup.lengths[s]], 30, 30)
        for b in range(N_BOOT):
            w_sb = wb[N_BOOT * row0[s] + b * n_rows:N_BOOT * row0[s] + (b + 1) * n_rows].copy()
            assert w_sb.sum() == samples[s][1].sum()
            n_zero += int((w_sb == 0).sum())
            res = em.run_em_many([(cm, w_sb)], finish_args(), inits=[start])
            assert res[0]["route"] == "batch"
            for checked in (False, True):
                args = finish_args(var_check=checked, min_reads=MIN_READS, refine_ests=False)
                fin = assign.finish_many([(cm, w_sb)], res, haps, args, phylo=small["phy"], obs=one_table, var_tables=small["tab"])[0]
                got = detected[checked][0][s]
                n = int(got["ncand"][b])
                assert got["flag"][b] == 0 and 0 <= n <= 64, (s, b, checked)
                kept = [i for i in range(n) if got["keep"][b, i]]
                assert [haps[got["cand"][b, i]] for i in kept] == [con[1] for con in fin["contribs"]], (s, b, checked)
                want_p = numpy.array([con[2] for con in fin["contribs"]], dtype=F8)
                assert got["cand_props"][b, kept].tobytes() == want_p.tobytes(), (s, b, checked)
                assert (got["iters"][b], got["done"][b]) == (res[0]["iters"][0], res[0]["done"][0]), (s, b, checked)
                if not checked:
                    assert len(kept) == n
                # the estimate's columns: the replicate's wide-EM proportions there
                cols = [haps.index(con[1]) for con in small["finished"][checked][s]["contribs"]]
                assert got["props_boot"][b].tobytes() == numpy.asarray(res[0]["props"])[cols].tobytes(), (s, b, checked)
    assert n_zero > 0                                               # rows of resampled weight 0 stayed in the batch


def test_the_result_holds_what_the_docstring_says(small, detected):
    for checked in (False, True):
        found, skipped = detected[checked]
        assert found[3] is None and skipped == [(3, "its weights are not non-negative integers")]
        for s in range(3):
            res = found[s]
            contribs = small["finished"][checked][s]["contribs"]
            want = ref.summary(res["cand"], res["ncand"], res["keep"] if checked else None, res["flag"], res["done"], contribs, small["haps"])
            for key in want:
                assert res[key] == want[key], (checked, s, key)
            assert res["n_used"] + sum(res["n_failed"].values()) == N_BOOT and res["n_used"] == N_BOOT
            assert res["var_check"] == ("observed pileup" if checked else "off") and (res["seed"], res["n_boot"]) == (SEED, N_BOOT)
            assert res["columns"] == [c[1] for c in contribs] and res["props_boot"].shape == (N_BOOT, len(contribs))
            if 1 <= len(contribs) <= 16:
                assert res["summary"] == "mxm_bootstrap_summary"
                assert numpy.allclose(res["mean"], res["props_boot"].mean(axis=0), rtol=1e-12, atol=0)
                assert numpy.all(res["lo"] <= res["hi"]) and res["sd"].shape == (len(contribs),)
            else:
                assert "lo" not in res and res["summary"].startswith("omitted")
    # the single-row sample: every replicate is the sample itself
    one = detected[False][0][1]
    assert len(set(one["cand"][b, :one["ncand"][b]].tobytes() for b in range(N_BOOT))) == 1


def test_more_replicates_reproduce_the_first_ones(small, detected):
    for checked in (False, True):
        eight = detect(small, checked, n_boot=8)[0]
        for s in range(3):
            same_replicates(eight[s], detected[checked][0][s], N_BOOT, (checked, s))


def test_the_chunking_changes_nothing(small, detected, lib):
    from mixemt_amd import assign
    tile = int(lib.mxm_samples_tile_rows())
    m0 = small["samples"][0][0]
    row_bytes = m0.rec_off.element_size() + m0.ndist.element_size()
    needs = [assign._detect_entry_bytes(small["samples"][s][0].n_rows, len(small["haps"]), tile, row_bytes) for s in range(3) for _ in range(N_BOOT)]
    one_each = max(needs)
    assert assign._detect_chunks(needs, one_each) == [(e, e + 1) for e in range(3 * N_BOOT)]
    assert assign._detect_chunks(needs, assign.DETECT_BYTES) == [(0, 3 * N_BOOT)]
    for checked in (False, True):
        split = detect(small, checked, max_bytes=one_each)[0]
        for s in range(3):
            same_replicates(split[s], detected[checked][0][s], N_BOOT, (checked, s))
            assert split[s]["detection"] == detected[checked][0][s]["detection"]
            if "lo" in split[s]:
                assert split[s]["lo"].tobytes() == detected[checked][0][s]["lo"].tobytes()
    with pytest.raises(ValueError, match="split the cohort or lower n_boot"):
        detect(small, False, max_bytes=one_each - 1)


def test_a_skipped_sample_leaves_its_neighbours_unchanged(small, detected):
    from mixemt_amd import assign
    args = finish_args(min_reads=MIN_READS)
    three, skipped = assign.detect_many(small["samples"][:3], small["results"][:3], small["finished"][False][:3], small["haps"], args,
                                        n_boot=N_BOOT, seed=SEED)
    assert skipped == []
    for s in range(3):
        same_replicates(three[s], detected[False][0][s], N_BOOT, s)
    # weights on the device are checked by the weights entry: the same reason, the same neighbours
    import torch
    on_device = [(m, torch.from_numpy(w).cuda()) for m, w in small["samples"]]
    found, skipped = assign.detect_many(on_device, small["results"], small["finished"][False], small["haps"], args, n_boot=N_BOOT, seed=SEED)
    assert found[3] is None and skipped == [(3, "its weights are not non-negative integers")]
    for s in range(3):
        same_replicates(found[s], detected[False][0][s], N_BOOT, s)
    one, why = assign.detect(small["samples"][2][0], small["samples"][2][1], small["results"][2], small["finished"][False][2], small["haps"],
                             args, n_boot=N_BOOT, seed=SEED, sample_ids=2)
    assert why is None
    same_replicates(one, detected[False][0][2], N_BOOT, "detect")
