"""
The assembly stage of a cohort on the device (assemble.extend_assemblies_many, call_consensus_many,
write_consensus_seqs_many over an assign.CohortContribReads; mxm_new_variants_samples, mxm_extend_assign_samples): per sample
the batch gives what the sample gives alone through extend_assemblies / call_consensus_all / write_consensus_seqs, what the
numpy restatement (tests/_assemble_ref.py) gives, and -- g18 -- what the reference's own run gave.  Integers, strings and file
bytes: no tolerance anywhere.
"""
import ctypes
import json
import os
import sys
import tempfile

import numpy
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _assemble_ref  # noqa: E402
from test_assemble import CASES, g18_args, g18_contribs, g18_inputs, g18_start  # noqa: E402
from test_gpu_assemble import args_of, device_table, random_columns, random_labels, random_sources  # noqa: E402
from test_gpu_observe import _subset  # noqa: E402
from test_var_check_host import empty_columns  # noqa: E402

pytestmark = pytest.mark.gpu

REF_LEN = 3000
THREE = ["hap1", "hap2", "hap3", "unassigned"]
TWO = ["hap1", "hap2", "unassigned"]


def make_cohort(samples):
    """An assign.CohortContribReads from per-sample (cols, local label, names, keys): the labels made global by hand (what
    assign_reads_many derives from finish_many's results)."""
    import torch
    from mixemt_amd import alignments, assign
    cols_list = [s[0] for s in samples]
    joined, aln0 = alignments.concat_columns(cols_list)
    lab0 = numpy.zeros(len(samples) + 1, dtype=numpy.int64)
    glob = []
    for s, (_, label, names, _) in enumerate(samples):
        lab0[s + 1] = lab0[s] + len([n for n in names if n != "unassigned"]) + 1
        label = numpy.asarray(label, dtype=numpy.int64)
        glob.append(numpy.where(label >= 0, label + lab0[s], -1))
    labels = torch.from_numpy(numpy.concatenate(glob).astype(numpy.int32)).cuda()
    aln_sample = torch.from_numpy(numpy.repeat(numpy.arange(len(samples), dtype=numpy.int32), numpy.diff(aln0))).cuda()
    return assign.CohortContribReads(cols_list, joined, aln0, lab0, [s[2] for s in samples], [s[3] for s in samples], labels,
                                     aln_sample)


def random_sample(seed, n_src, n_aln):
    """As test_gpu_assemble.test_random_inputs_equal_the_restatement makes its input (the reference sequence's own letters
    play no part in the stage: only its length does)."""
    rng = numpy.random.default_rng(seed)
    _, srcs = random_sources(rng, REF_LEN, n_src)
    cols = random_columns(rng, n_aln, srcs, n_aln // 2)
    names = THREE if n_src == 3 else TWO
    return cols, random_labels(rng, cols, n_src), list(names), list(names)


@pytest.fixture(scope="module")
def cohort_inputs():
    """The seven samples, and per sample the restatement's final table and record (made once, never written)."""
    s0, s1, s2, s3 = random_sample(11, 3, 1500), random_sample(12, 2, 1500), random_sample(13, 3, 600), random_sample(14, 2, 400)
    samples = [s0, s1, s2, s3,
               (empty_columns(), numpy.zeros(0, dtype=numpy.int32), list(TWO), []),                # no alignments
               (s3[0], numpy.zeros(len(s3[0]), dtype=numpy.int32), ["hap1"], ["hap1"]),            # no 'unassigned' label
               (s0[0], numpy.where(s0[1] == 1, -1, s0[1]).astype(numpy.int32), list(THREE), list(THREE))]   # hap2 has no alignments
    a = args_of(cons_cov=2)
    refseq = "A" * REF_LEN
    want = []
    for cols, label, names, keys in samples:
        table = _assemble_ref.Table(cols, label, names, keys)
        record = []
        _assemble_ref.extend_assemblies(refseq, table, a, record)
        want.append((table, record))
    return refseq, a, samples, want


def test_the_random_cohort_is_not_degenerate(cohort_inputs):
    _, _, samples, want = cohort_inputs
    rounds = [len(record) for _, record in want]
    movers = [sum(1 for r in record if r[0] > 0) for _, record in want]
    print("rounds per sample:", rounds, "rounds with moves:", movers)
    assert sum(1 for m in movers if m >= 2) >= 3 and len(set(rounds[:4])) >= 2
    assert rounds[4:] == [1, 1, 1] and want[5][1][0][2] > 0 and want[6][1][0][:3] == (0, int((samples[6][1] == 3).sum()), 0)


@pytest.fixture(scope="module")
def extended(cohort_inputs):
    """The cohort after extend_assemblies_many, and every sample after extend_assemblies alone."""
    from mixemt_amd import assemble
    refseq, a, samples, _ = cohort_inputs
    cohort = make_cohort(samples)
    assert assemble.extend_assemblies_many(refseq, cohort, a, samples=range(len(samples))) is cohort
    alone = []
    for cols, label, names, keys in samples:
        cr = device_table(cols, label, names, keys)
        assemble.extend_assemblies(refseq, cr, a)
        alone.append(cr)
    return cohort, alone


def test_random_cohort_equals_the_restatement_and_the_samples_alone(cohort_inputs, extended):
    _, _, samples, want = cohort_inputs
    cohort, alone = extended
    for s, (table, record) in enumerate(want):
        got = cohort.sample(s)
        assert numpy.array_equal(got.labels.cpu().numpy(), table.label), s
        assert numpy.array_equal(got.joined.cpu().numpy(), table.joined), s
        assert list(got) == table.keys and cohort.rounds[s] == table.rounds == len(record), s
        assert cohort.round_log[s] == [tuple(r[:3]) for r in record], s
        assert numpy.array_equal(got.labels.cpu().numpy(), alone[s].labels.cpu().numpy()), s
        assert numpy.array_equal(got.joined.cpu().numpy(), alone[s].joined.cpu().numpy()), s
        assert list(got) == list(alone[s]) and got.rounds == alone[s].rounds, s


@pytest.mark.parametrize("strict", [True, False])
def test_random_cohort_consensus_strings(cohort_inputs, extended, strict):
    from mixemt_amd import assemble
    refseq, a, _, want = cohort_inputs
    cohort, alone = extended
    got = assemble.call_consensus_many(refseq, cohort, 1, a, strict=strict)
    for s, (table, _) in enumerate(want):
        assert got[s] == assemble.call_consensus_all(refseq, alone[s], 1, a, strict=strict), s
        assert list(got[s]) == table.keys, s
        for key in table.keys:
            assert got[s][key] == _assemble_ref.call_consensus(refseq, table, key, 1, a, strict), (s, key)
    assert got[4] == {"unassigned": ""} and len(got[0]["hap1"]) == REF_LEN


def test_default_samples_are_those_with_more_than_one_contributor(cohort_inputs):
    from mixemt_amd import assemble
    refseq, a, samples, want = cohort_inputs
    cohort = make_cohort(samples[2:6])
    assemble.extend_assemblies_many(refseq, cohort, a)
    assert cohort.rounds == [want[2][0].rounds, want[3][0].rounds, 1, 0]
    assert "unassigned" not in cohort.keys[3] and int((cohort.sample(3).joined > 0).sum()) == 0


def test_place_in_the_batch_and_order_inside_a_sample_do_not_matter(cohort_inputs):
    from mixemt_amd import assemble
    refseq, a, samples, want = cohort_inputs
    other, mine = samples[1], samples[2]
    table = want[2][0]
    rng = numpy.random.default_rng(5)
    perm = rng.permutation(len(mine[0]))
    shuffled = (_subset(mine[0], perm), mine[1][perm], mine[2], mine[3])
    strings = None
    for batch, at, order in (([mine], 0, None), ([mine, other], 0, None), ([other, mine], 1, None), ([other, shuffled], 1, perm)):
        cohort = make_cohort(batch)
        assemble.extend_assemblies_many(refseq, cohort, a)
        got = cohort.sample(at)
        idx = numpy.arange(len(perm)) if order is None else order
        assert numpy.array_equal(got.labels.cpu().numpy(), table.label[idx]), (len(batch), at)
        assert numpy.array_equal(got.joined.cpu().numpy(), table.joined[idx]), (len(batch), at)
        assert cohort.rounds[at] == table.rounds
        cons = assemble.call_consensus_many(refseq, cohort, 2, a)[at]
        loose = assemble.call_consensus_many(refseq, cohort, 1, a, strict=False)[at]
        if strings is None:
            strings = (cons, loose)
        assert cons == strings[0], (len(batch), at)
        if order is None:                                            # (the tie rule reads the list's order: not under a permutation)
            assert loose == strings[1], (len(batch), at)


# ---- g18: the reference's own run, three cases as one batch ----------------------------------------------------------------
@pytest.fixture(scope="module")
def g18():
    return g18_inputs()


@pytest.mark.parametrize("cons_cov", [2, 1000000])
def test_g18_cases_as_one_batch(g18, cons_cov, capsys):
    """g18's three cases over the same columns as ONE batch of three samples.  The stage takes one args for a batch and the
    golden's `nocall` case was run with cons_cov = 1000000, the other two with 2: the batch is run under either value, and
    under each every sample whose case has that value equals the reference's run in labels, joined, rounds, verbose text,
    the three consensus dictionaries and the FASTA file."""
    from mixemt_amd import assemble
    refseq, _, cols = g18
    g = golden("g18_assemble")
    starts = [g18_start(g, case) for case in CASES]
    mine = [k for k, case in enumerate(CASES) if int(g18_args(g, case).cons_cov) == cons_cov]
    assert mine == ([0, 1] if cons_cov == 2 else [2])
    a = g18_args(g, CASES[mine[0]], verbose=True)
    cohort = make_cohort([(cols, label, names, keys) for names, keys, label in starts])
    capsys.readouterr()
    assemble.extend_assemblies_many(refseq, cohort, a)
    err = capsys.readouterr().err
    a.verbose = False
    blocks = ["\nAssembly extension step...\n" + part for part in err.split("\nAssembly extension step...\n")[1:]]
    assert len(blocks) == 3 and "".join(blocks) == err
    cons = {item: assemble.call_consensus_many(refseq, cohort, min_cov, a, strict=strict)
            for item, min_cov, strict in (("strict_after", cons_cov, True), ("strict2_after", 2, True), ("loose_after", 1, False))}
    with tempfile.TemporaryDirectory() as tmp:
        prefixes = [os.path.join(tmp, case) for case in CASES]
        assemble.write_consensus_seqs_many(refseq, [g18_contribs(g, case) for case in CASES], cohort, a, prefixes)
        for k in mine:
            case = CASES[k]
            names = starts[k][0]
            got = cohort.sample(k)
            final_keys = str(g[case + "_keys"]).split("\n")
            want = numpy.array([names.index(final_keys[i]) if i >= 0 else -1 for i in g[case + "_aln_key"]])
            assert numpy.array_equal(got.labels.cpu().numpy(), want), case
            assert numpy.array_equal(got.joined.cpu().numpy(), g[case + "_aln_round"]), case
            assert [list(r) for r in cohort.round_log[k]] == g[case + "_rounds"].tolist(), case
            assert cohort.rounds[k] == len(g[case + "_rounds"]) and blocks[k] == str(g[case + "_verbose"]), case
            for item in cons:
                want_cons = json.loads(str(g["%s_%s" % (case, item)]))
                assert cons[item][k] == want_cons, (case, item)
            loose = json.loads(str(g[case + "_loose_after"]))
            contribs = g18_contribs(g, case)
            records = [(c[0], c[1], loose.get(c[0], "")) for c in contribs] + [("unassigned", "", loose["unassigned"])]
            with open(prefixes[k] + ".fa") as fin:
                assert fin.read() == assemble.format_fasta(records), case
            assert sorted(got) == final_keys, case


# ---- the C entries directly --------------------------------------------------------------------------------------------
def _alignments(seqs, frag, start=10):
    """len(seqs) alignments of 4 matched bases at `start`, mapq 60, no qualities."""
    from mixemt_amd.alignments import AlignmentColumns
    n = len(seqs)
    raw = numpy.frombuffer("".join(seqs).encode(), dtype=numpy.uint8)
    return AlignmentColumns([start] * n, [60] * n, frag, numpy.arange(n + 1), [(4 << 4)] * n, 4 * numpy.arange(n + 1), raw,
                            None, None, ["r%d" % i for i in range(max(frag) + 1)], [0] * n)


def _extend_direct(frag, newvar_words, label=(1, 3)):
    """Two samples (labels 0 = its contributor, 1 = its 'unassigned'; 2 and 3), one alignment each: ACAT and ACCT at 10."""
    import torch
    from mixemt_amd import _lib, observe
    lib = _lib.load()
    cols = _alignments(["ACAT", "ACCT"], list(frag))
    dcols = observe.DeviceColumns(cols)
    st = dcols.struct()
    frag_d = torch.tensor(list(frag), dtype=torch.int64).cuda()
    st.n_frag, st.frag = 2, frag_d.data_ptr()
    ref_len = 20
    newvar = numpy.full((2, ref_len, 4), -1, dtype=numpy.int8)
    for s, pos, base, owner in newvar_words:
        newvar[s, pos, "ACGT".index(base)] = owner
    newvar_d = torch.from_numpy(newvar.view(numpy.int32).reshape(2, ref_len)).cuda()
    lab = torch.tensor(list(label), dtype=torch.int32).cuda()
    joined = torch.zeros(2, dtype=torch.int32).cuda()
    sample = torch.tensor([0, 1], dtype=torch.int32).cuda()
    state = torch.zeros(2, dtype=torch.int32).cuda()
    owner = torch.zeros(2, dtype=torch.int32).cuda()
    moved = torch.zeros(2, dtype=torch.int32).cuda()
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)                   # noqa: E731
    rc = lib.mxm_extend_assign_samples(ctypes.byref(st), sample.data_ptr(), lab.data_ptr(), joined.data_ptr(), i32(1, 3),
                                       i32(0, 2), i32(0, 1, 2), 2, 4, 5, 30, 30, newvar_d.data_ptr(), ref_len,
                                       state.data_ptr(), owner.data_ptr(), moved.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.mxm_last_error()
    return lab.tolist(), joined.tolist(), owner.tolist(), moved.tolist(), state.tolist()


def test_a_fragment_shared_by_two_samples_never_moves_across_them():
    own = [(0, 12, "A", 0), (1, 12, "C", 0)]                          # each sample's variant, shown by its own alignment
    # two fragments: both move, each to its own sample's contributor
    assert _extend_direct((0, 1), own) == ([0, 2], [5, 5], [0, 2], [1, 1], [0, 2])
    # ONE fragment index for both: two owners, a conflict -- nothing moves
    assert _extend_direct((0, 0), own) == ([1, 3], [0, 0], [-1, -1], [0, 0], [-2, -1])
    # one fragment index, only sample 0's alignment shows a variant: sample 1's alignment does not follow it
    assert _extend_direct((0, 0), own[:1]) == ([0, 3], [5, 0], [0, -1], [1, 0], [0, -1])
    # a sample's alignment is looked up in its OWN row: with the rows swapped neither base is a variant
    assert _extend_direct((0, 1), [(1, 12, "A", 0), (0, 12, "C", 0)]) == ([1, 3], [0, 0], [-1, -1], [0, 0], [-1, -1])


def test_new_variants_samples_rows_counters_and_samples_without_participants():
    import torch
    from mixemt_amd import _lib
    lib = _lib.load()
    ref_len, ld = 300, 320                                            # (more than one block per sample; ld > ref_len)
    rng = numpy.random.default_rng(3)
    cons = rng.choice(numpy.frombuffer(b"ACGTN-X", dtype=numpy.uint8), size=(5, ld), p=[0.3, 0.25, 0.2, 0.15, 0.04, 0.03, 0.03])
    use, use_ptr = [4, 0, 2, 1, 3], [0, 3, 3, 5]                      # sample 1 takes no part
    cons_d = torch.from_numpy(cons).cuda()
    newvar = torch.full((3, ref_len), 7, dtype=torch.int32).cuda()
    n_new = torch.tensor([10, 20, 30], dtype=torch.int32).cuda()
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)                    # noqa: E731
    assert lib.mxm_new_variants_samples(cons_d.data_ptr(), ld, 5, i32(use), i32(use_ptr), 3, ref_len, newvar.data_ptr(),
                                        n_new.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0, lib.mxm_last_error()
    got = newvar.cpu().numpy().view(numpy.int8).reshape(3, ref_len, 4)
    counts = []
    for s in range(3):
        rows = use[use_ptr[s]:use_ptr[s + 1]]
        want = numpy.full((ref_len, 4), -1, dtype=numpy.int8)
        for pos in range(ref_len if rows else 0):
            col = [chr(cons[r, pos]) for r in rows]
            if all(c in "ACGT" for c in col):
                for k, c in enumerate(col):
                    if col.count(c) == 1:
                        want[pos, "ACGT".index(c)] = k
        assert numpy.array_equal(got[s], want), s
        counts.append(int((want >= 0).sum()))
    assert n_new.tolist() == [10 + counts[0], 20, 30 + counts[2]] and counts[0] > 0 and counts[2] > 0


# ---- errors --------------------------------------------------------------------------------------------------------------
def _small_cohort(bad_cigar):
    """Three samples of two alignments: one of hap1, one unassigned (sample 2's unassigned one with a CIGAR of 10 matches
    over 4 bases when bad_cigar)."""
    from mixemt_amd.alignments import AlignmentColumns
    samples = []
    for s in range(3):
        cols = _alignments(["ACGT", "ACGT"], [0, 1])
        if s == 2 and bad_cigar:
            cols = AlignmentColumns(cols.ref_start, cols.mapq, cols.frag, cols.cig_ptr, [4 << 4, 10 << 4], cols.seq_ptr, cols.seq,
                                    None, None, cols.names, [0, 0])
        samples.append((cols, numpy.array([0, 2], dtype=numpy.int32), list(TWO), ["hap1", "unassigned"]))
    return make_cohort(samples)


def test_errors_name_the_alignment_the_sample_and_too_many_contributors():
    import torch
    from mixemt_amd import assemble
    refseq = "ACGT" * 25
    cohort = _small_cohort(True)
    with pytest.raises(ValueError, match=r"failed \(-4\): mxm_extend_assign_samples: the CIGAR of alignment 5 runs past its sequence$"):
        assemble.extend_assemblies_many(refseq, cohort, args_of())
    cohort = _small_cohort(False)
    cohort.aln_sample[3] = 7
    with pytest.raises(ValueError, match=r"failed \(-1\): mxm_extend_assign_samples: alignment 3 has a sample outside \[0, 3\)$"):
        assemble.extend_assemblies_many(refseq, cohort, args_of())
    many = ["hap%d" % i for i in range(128)]
    cols = _alignments(["ACGT"], [0])
    crowd = make_cohort([(cols, numpy.array([0], dtype=numpy.int32), many + ["unassigned"], list(many))])
    with pytest.raises(ValueError, match="128 contributors take part, at most 127"):
        assemble.extend_assemblies_many(refseq, crowd, args_of())
    assert torch.cuda.is_available()


# ---- the route from finish_many's results --------------------------------------------------------------------------------
def test_assign_reads_many_equals_assign_reads_per_sample():
    """Hand-made finish_many results over real columns: the labels, names and keys of assign_reads per sample; with a
    CohortPileup that kept its columns nothing is uploaded again."""
    import torch
    from mixemt_amd import assign, observe
    a = args_of(min_fold=2.0)
    cols_list, finished, reads_list, want = [], [], [], []
    contribs = [["hap1", "A", 0.5], ["hap2", "B", 0.3], ["hap3", "C", 0.2]]
    for s, (seed, k) in enumerate(((21, 3), (22, 1), (23, 2))):
        rng = numpy.random.default_rng(seed)
        _, srcs = random_sources(rng, 1000, 2)
        cols = random_columns(rng, 200, srcs, 120)
        frags = rng.permutation(120)[:100]                           # 20 fragments are in no row
        reads = [[cols.names[f] for f in frags[i:i + 2]] for i in range(0, 100, 2)]
        row = rng.integers(-1, k, size=len(reads)).astype(numpy.int32) if k > 1 else numpy.zeros(len(reads), dtype=numpy.int32)
        fin = {"contribs": [list(c) for c in contribs[:k]], "row_label": row, "assigned": assign.AssignedReads(row, [c[0] for c in contribs[:k]])}
        # assign_reads' own rule, restated: the row's label (unassigned: the number of contributors) for every alignment of
        # the row's fragments, -1 for a fragment in no row
        frag_label = numpy.full(120, -1)
        for r, ids in enumerate(reads):
            for name in ids:
                frag_label[cols.names.index(name)] = (row[r] if row[r] >= 0 else k) if k > 1 else 0
        want.append(frag_label[cols.frag])
        cols_list.append(cols), finished.append(fin), reads_list.append(reads)
    pileup = observe.observe_bases_many(cols_list, 30, 30, ref_len=1000, keep_columns=True)
    assert pileup.dcols is not None and observe.observe_bases_many(cols_list, 30, 30, ref_len=1000).dcols is None
    for pile in (None, pileup):
        cohort = assign.assign_reads_many(cols_list, finished, reads_list, a, pileup=pile)
        assert cohort.lab0.tolist() == [0, 4, 6, 9] and (pile is None or cohort.device_columns() is pileup.dcols)
        for s in range(3):
            got = cohort.sample(s)
            assert numpy.array_equal(got.labels.cpu().numpy(), want[s]), s
            assert got.names == [c[0] for c in finished[s]["contribs"]] + (["unassigned"] if len(finished[s]["contribs"]) > 1 else [])
            assert list(got) == list(finished[s]["assigned"]), s
        assert torch.equal(cohort.aln_sample.cpu(), torch.repeat_interleave(torch.arange(3, dtype=torch.int32), 200))
    with pytest.raises(ValueError, match="split the cohort"):
        assign.assign_reads_many(cols_list, finished, reads_list, a, max_bytes=1000)
