"""
mixemt's `-x` / `-b` on the device (mixemt_amd.assemble over ContribReads) against the reference's own run (g18: strings,
integers and file bytes, no tolerance) and against the numpy restatement (tests/_assemble_ref.py) on randomised and
10^6-fragment inputs.
"""
import argparse
import io
import json
import os
import sys
import tempfile

import numpy
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _assemble_ref  # noqa: E402
import _pileup_ref  # noqa: E402
from test_assemble import CASES, g18_args, g18_contribs, g18_dicts, g18_inputs, g18_start  # noqa: E402
from test_gpu_observe import _subset  # noqa: E402

from conftest import golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    return g18_inputs()


def device_table(cols, label, names, keys, joined=None):
    import torch
    from mixemt_amd import assign
    cr = assign.ContribReads(cols, torch.from_numpy(numpy.ascontiguousarray(label, dtype=numpy.int32)).cuda(), names, keys)
    if joined is not None:
        cr.relabel(cr.labels, torch.from_numpy(numpy.ascontiguousarray(joined, dtype=numpy.int32)).cuda())
    return cr


def args_of(**kw):
    a = argparse.Namespace(min_mq=30, min_bq=30, cons_cov=2, verbose=False)
    for key, val in kw.items():
        setattr(a, key, val)
    return a


@pytest.mark.parametrize("case", CASES)
def test_g18_extension_consensus_and_files(inputs, case, capsys):
    from mixemt_amd import assemble, observe, stats
    refseq, phy, cols = inputs
    g = golden("g18_assemble")
    names, keys, label = g18_start(g, case)
    a = g18_args(g, case)
    contribs = g18_contribs(g, case)
    cr = device_table(cols, label, names, keys)
    before = assemble.call_consensus_all(refseq, cr, int(a.cons_cov), a, strict=True)
    assert before == json.loads(str(g[case + "_strict_before"]))
    for key in keys:
        assert assemble.call_consensus(refseq, cr, key, int(a.cons_cov), a) == before[key]
    # round by round with the public steps: each round's dict and counters
    step = device_table(cols, label, names, keys)
    step["unassigned"]
    dicts, rounds = g18_dicts(g, case), g[case + "_rounds"].tolist()
    for want_dict, (moved, n_un, n_new) in zip(dicts, rounds):
        assert step.count("unassigned") == n_un
        got = assemble.find_new_variants(refseq, step, a)
        assert got == want_dict and len(got) == n_new
        assemble.assign_reads_from_new_vars(step, got, a)
        assert n_un - step.count("unassigned") == moved
    # the loop itself, verbose
    a.verbose = True
    capsys.readouterr()
    out = assemble.extend_assemblies(refseq, cr, a)
    assert capsys.readouterr().err == str(g[case + "_verbose"])
    a.verbose = False
    assert out is cr and list(cr) == str(g[case + "_extend_keys"]).split("\n")
    final_keys = str(g[case + "_keys"]).split("\n")
    want = numpy.array([names.index(final_keys[k]) if k >= 0 else -1 for k in g[case + "_aln_key"]])
    assert numpy.array_equal(cr.labels.cpu().numpy(), want)
    assert numpy.array_equal(step.labels.cpu().numpy(), want)
    assert numpy.array_equal(cr.joined.cpu().numpy(), g[case + "_aln_round"])
    for item, min_cov, strict in (("strict_after", int(a.cons_cov), True), ("strict2_after", 2, True), ("loose_after", 1, False)):
        assert assemble.call_consensus_all(refseq, cr, min_cov, a, strict=strict) == json.loads(str(g["%s_%s" % (case, item)])), item
    loose = json.loads(str(g[case + "_loose_after"]))
    report = io.StringIO()
    stats.report_contributors(report, contribs, cr)
    assert report.getvalue() == str(g[case + "_report"])
    assert sorted(cr) == final_keys
    with tempfile.TemporaryDirectory() as tmp:
        a.cons_prefix = os.path.join(tmp, "cons")
        assemble.write_consensus_seqs(refseq, contribs, cr, a)
        records = [(c[0], c[1], loose.get(c[0], "")) for c in contribs] + [("unassigned", "", loose["unassigned"])]
        with open(a.cons_prefix + ".fa") as fin:
            assert fin.read() == assemble.format_fasta(records)
        if case == "default":
            L = observe.pileup_length(cols, 30, len(refseq))
            all_obs = observe.ObservedBases(_pileup_ref.from_triplets(g["trip_pos"], str(g["trip_key"]), g["trip_count"], L))
            a.stats_prefix, a.min_var_reads, a.frac_var_reads = os.path.join(tmp, "run"), 3, 0.02
            stats.write_statistics(phy, all_obs, contribs, cr, a)
            with open(a.stats_prefix + ".pos.tab") as fin:
                assert fin.read() == str(g["default_pos_tab"])
            with open(a.stats_prefix + ".obs.tab") as fin:
                assert fin.read() == str(g["default_obs_tab"])


def random_sources(rng, ref_len, n_src=3, every=37):
    """A random reference and n_src sequences that differ from it every `every` positions (each at its own offset)."""
    ref = rng.choice(list("ACGT"), size=ref_len)
    srcs = []
    for k in range(n_src):
        src = ref.copy()
        at = numpy.arange(5 + 11 * k, ref_len, every)
        src[at] = [{"A": "C", "C": "G", "G": "T", "T": "A"}[c] for c in ref[at]]
        srcs.append(src)
    return "".join(ref), srcs


def random_columns(rng, n, srcs, n_frag, no_qual=False, noise=0.003):
    """n alignments shed by the sources (a fragment's alignments by one source: fragment % len(srcs)) with every CIGAR
    operation, both strands, lower case, N and IUPAC characters, low qualities; some reach past the reference."""
    from mixemt_amd.alignments import AlignmentColumns
    ref_len = len(srcs[0])
    frag = rng.integers(0, n_frag, size=n)
    starts, cig, seqs, quals, hasq = [], [], [], [], []
    for i in range(n):
        ops = [(5, 3)] if rng.random() < 0.2 else []
        if rng.random() < 0.3:
            ops.append((4, int(rng.integers(1, 6))))
        for _k in range(int(rng.integers(1, 4))):
            ops.append((int(rng.choice([0, 7, 8])), int(rng.integers(1, 70))))
            ops.append((int(rng.choice([1, 2, 3, 6])), int(rng.integers(1, 7))))
        ops.append((0, int(rng.integers(1, 40))))
        rlen = sum(ln for op, ln in ops if op in (0, 2, 3, 7, 8))
        start = int(rng.integers(0, ref_len - rlen + 30)) if rng.random() > 0.02 else -1
        src = srcs[int(frag[i]) % len(srcs)]
        seq, r = [], max(start, 0)
        for op, ln in ops:
            if op in (0, 7, 8):
                seq.extend(src[numpy.minimum(numpy.arange(r, r + ln), ref_len - 1)])
            elif op in (1, 4):
                seq.extend(rng.choice(list("ACGT"), size=ln))
            if op in (0, 2, 3, 7, 8):
                r += ln
        seq = numpy.array(seq)
        flip = rng.random(len(seq)) < noise
        seq[flip] = rng.choice(list("ACGTNR"), size=int(flip.sum()))
        if rng.random() < 0.1:
            seq = numpy.char.lower(seq)
        starts.append(start)
        cig.append([(ln << 4) | op for op, ln in ops])
        seqs.append("".join(seq))
        quals.append(numpy.where(rng.random(len(seq)) < 0.1, 12, 35))
        hasq.append(0 if rng.random() < 0.2 else 1)
    seq = numpy.frombuffer("".join(seqs).encode(), dtype=numpy.uint8)
    return AlignmentColumns(starts, rng.choice([60, 30, 29, 0], size=n, p=[0.6, 0.2, 0.1, 0.1]), frag,
                            numpy.concatenate([[0], numpy.cumsum([len(c) for c in cig])]), numpy.concatenate(cig),
                            numpy.concatenate([[0], numpy.cumsum([len(q) for q in seqs])]), seq,
                            None if no_qual else numpy.concatenate(quals).astype(numpy.uint8), None if no_qual else hasq,
                            ["f%d" % i for i in range(n_frag)], rng.integers(0, 2, size=n))


def random_labels(rng, cols, n_src=3):
    """60 % of the fragments unassigned, the others with their source (2 % with another), 5 % of the alignments in no row."""
    f = cols.frag
    assigned = (f * 7919 % 10) < 4
    label = numpy.where(assigned, f % n_src, n_src)
    wrong = rng.random(len(f)) < 0.02
    label[wrong & assigned] = (label[wrong & assigned] + 1) % n_src
    label[rng.random(len(f)) < 0.05] = -1
    return label.astype(numpy.int32)


def compare_with_restatement(refseq, cols, label, names, keys, a, joined=None):
    """The whole interface, device against restatement; returns the device table after extension."""
    from mixemt_amd import assemble
    cr = device_table(cols, label, names, keys, joined)
    ref = _assemble_ref.Table(cols, label, names, keys, joined)
    for strict, min_cov in ((True, int(a.cons_cov)), (False, 1), (True, 1), (False, 3)):
        got = assemble.call_consensus_all(refseq, cr, min_cov, a, strict=strict)
        for key in keys:
            assert got[key] == _assemble_ref.call_consensus(refseq, ref, key, min_cov, a, strict), (key, strict, min_cov)
    assert assemble.find_new_variants(refseq, cr, a) == _assemble_ref.find_new_variants(refseq, ref, a)
    record = []
    _assemble_ref.extend_assemblies(refseq, ref, a, record)
    assemble.extend_assemblies(refseq, cr, a)
    assert numpy.array_equal(cr.labels.cpu().numpy(), ref.label)
    assert numpy.array_equal(cr.joined.cpu().numpy(), ref.joined)
    assert list(cr) == ref.keys
    for strict in (True, False):
        got = assemble.call_consensus_all(refseq, cr, 1, a, strict=strict)
        for key in ref.keys:
            assert got[key] == _assemble_ref.call_consensus(refseq, ref, key, 1, a, strict), (key, strict)
    return cr, record


@pytest.mark.parametrize("ref_len,no_qual", [(3000, False), (3000, True), (50000, False)])
def test_random_inputs_equal_the_restatement(ref_len, no_qual):
    """ref_len 3000: newvar in LDS; 50000 (200 KB of newvar): read from global memory.  Reads reach past ref_len (the
    table is longer than the reference)."""
    rng = numpy.random.default_rng(ref_len + no_qual)
    refseq, srcs = random_sources(rng, ref_len)
    n = ref_len // 2
    cols = random_columns(rng, n, srcs, n // 2, no_qual)
    names = ["hap1", "hap2", "hap3", "unassigned"]
    label = random_labels(rng, cols)
    a = args_of(cons_cov=2)
    cr, record = compare_with_restatement(refseq, cols, label, names, list(names), a)
    assert sum(r[0] for r in record) > 0
    # one participating contributor: every called position is its variant
    cr1, rec1 = compare_with_restatement(refseq, cols, numpy.where(label == 3, 3, numpy.where(label >= 0, 0, -1)), names,
                                         ["hap1", "unassigned"], a)
    assert rec1[0][2] > 0
    # a key without alignments: no new variants at all, nothing moves
    cr0, rec0 = compare_with_restatement(refseq, cols, numpy.where(label == 1, -1, label), names, list(names), a)
    assert [r[:3] for r in rec0] == [(0, int((label == 3).sum()), 0)] and (label == 1).any()
    # no 'unassigned' label at all (one contributor): extension must not fail
    compare_with_restatement(refseq, cols, numpy.zeros(n, dtype=numpy.int32), ["hap1"], ["hap1"], a)


def test_order_inside_a_batch_does_not_matter():
    """The same alignments permuted (within their joined batches the order key changes, the SET of owners does not):
    the same labels per alignment and the same strict consensus."""
    from mixemt_amd import assemble
    rng = numpy.random.default_rng(77)
    refseq, srcs = random_sources(rng, 4000, n_src=2)
    cols = random_columns(rng, 2500, srcs, 1200)
    names = ["hap1", "hap2", "unassigned"]
    label = random_labels(rng, cols, n_src=2)
    a = args_of(cons_cov=2)
    cr = device_table(cols, label, names, list(names))
    assemble.extend_assemblies(refseq, cr, a)
    perm = rng.permutation(len(cols))
    cr2 = device_table(_subset(cols, perm), label[perm], names, list(names))
    assemble.extend_assemblies(refseq, cr2, a)
    assert numpy.array_equal(cr2.labels.cpu().numpy(), cr.labels.cpu().numpy()[perm])
    assert numpy.array_equal(cr2.joined.cpu().numpy(), cr.joined.cpu().numpy()[perm])
    assert int((cr.joined > 0).sum()) > 0
    assert assemble.call_consensus_all(refseq, cr2, 2, a) == assemble.call_consensus_all(refseq, cr, 2, a)


def test_errors_name_the_alignment_and_too_many_contributors():
    import torch
    from mixemt_amd import assemble
    from test_gpu_observe import _one
    refseq = "ACGT" * 25
    bad = _one(10, [(0, 10)], "ACGT")                              # the CIGAR runs past the sequence
    cr = device_table(bad, numpy.array([1]), ["hap1", "unassigned"], ["hap1", "unassigned"])
    with pytest.raises(ValueError, match="mxm_extend_assign: the CIGAR of alignment 0 runs past its sequence"):
        assemble.assign_reads_from_new_vars(cr, {(12, "A"): "hap1"}, args_of())
    with pytest.raises(ValueError, match="is no contributor"):
        assemble.assign_reads_from_new_vars(cr, {(12, "A"): "hap7"}, args_of())
    many = ["hap%d" % i for i in range(130)]
    ok = _one(10, [(0, 4)], "ACGT")
    crm = device_table(ok, numpy.array([0]), many + ["unassigned"], many)
    with pytest.raises(ValueError, match="at most 127"):
        assemble.find_new_variants(refseq, crm, args_of())
    assert torch.cuda.is_available()


def _tied_then(cigar, seq):
    """Two sound alignments that disagree at position 12 (G against C: a tie for the majority consensus), then a third
    with `cigar` over `seq`; all of contributor hap1."""
    from mixemt_amd.alignments import AlignmentColumns
    seqs = ["ACGT", "ACCT", seq]
    cig = [[(0, 4)], [(0, 4)], cigar]
    raw = numpy.frombuffer("".join(seqs).encode(), dtype=numpy.uint8)
    return AlignmentColumns([10, 10, 10], [60, 60, 60], [0, 1, 2], numpy.cumsum([0] + [len(c) for c in cig]),
                            [(n << 4) | op for c in cig for op, n in c], numpy.cumsum([0] + [len(q) for q in seqs]), raw,
                            None, None, ["r0", "r1", "r2"], [0, 0, 0])


@pytest.mark.parametrize("cigar,what", [([(0, 10)], "runs past its sequence"), ([(0, 2), (9, 1)], "holds an unknown operation")])
def test_tie_rule_names_the_alignment_with_a_bad_cigar(cigar, what, monkeypatch):
    """mxm_first_observed's own CIGAR errors.  Through call_consensus the labelled pileup walks the same alignments first
    and is the one to report; with the tables counted from the two sound alignments (what a caller holding earlier
    tables has) the tie rule's walk is the first to meet alignment 2."""
    from mixemt_amd import assemble
    refseq = "ACGT" * 25
    names = ["hap1"]
    cols = _tied_then(cigar, "ACGT")
    cr = device_table(cols, numpy.zeros(3), names, names)
    with pytest.raises(ValueError, match=r"failed \(-4\): mxm_observe_bases_labelled: the CIGAR of alignment 2 " + what + "$"):
        assemble.call_consensus(refseq, cr, "hap1", 1, args_of(), strict=False)
    sound = device_table(_subset(cols, numpy.arange(2)), numpy.zeros(2), names, names)
    assert assemble.call_consensus(refseq, sound, "hap1", 1, args_of(), strict=False)[10:14] == "ACGT"    # G was seen first
    tables = assemble._tables
    monkeypatch.setattr(assemble, "_tables", lambda _cr, label, n, a, ref_len: tables(sound, label[:2].contiguous(), n, a, ref_len))
    with pytest.raises(ValueError, match=r"failed \(-4\): mxm_first_observed: the CIGAR of alignment 2 " + what + "$"):
        assemble.call_consensus(refseq, cr, "hap1", 1, args_of(), strict=False)


def test_extension_names_the_alignment_with_an_unknown_operation():
    from mixemt_amd import assemble
    from test_gpu_observe import _one
    bad = _one(10, [(0, 2), (9, 1)], "ACGT")
    cr = device_table(bad, numpy.array([1]), ["hap1", "unassigned"], ["hap1", "unassigned"])
    with pytest.raises(ValueError, match=r"failed \(-4\): mxm_extend_assign: the CIGAR of alignment 0 holds an unknown operation$"):
        assemble.assign_reads_from_new_vars(cr, {(12, "A"): "hap1"}, args_of())


def test_million_fragments_equal_the_restatement():
    from mixemt_amd import assemble, phylotree, preprocess, synth
    import gen_golden
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    tables = preprocess.HapVarTables.build(refseq, phy, sorted(phy.hap_var))
    cols = synth.synth_alignments(tables, refseq, 1000000, seed=1, private=gen_golden.g18_private(refseq, tables))
    # the contributor that shed each fragment is the generator's first draw; fragment names keep the original numbers.
    # One fragment in 200 is assigned to its contributor (a strict consensus needs unanimous reads: ~12x each), the rest
    # is unassigned -- the walk of the extension is over 99 % of the alignments -- and a few are in no row
    who = numpy.random.default_rng([1, 0xA11]).choice(len(synth.DEFAULT_PROPS), size=1000000,
                                                      p=numpy.asarray(synth.DEFAULT_PROPS, dtype=float))
    who_of = who[numpy.array([int(name[1:]) for name in cols.names])]
    f = cols.frag
    label = numpy.where(f % 50 == 49, -1, numpy.where(f % 200 == 0, who_of[f], 3)).astype(numpy.int32)
    names = ["hap1", "hap2", "hap3", "unassigned"]
    a = args_of(cons_cov=2)
    cr = device_table(cols, label, names, list(names))
    ref = _assemble_ref.Table(cols, label, names, list(names))
    got = assemble.find_new_variants(refseq, cr, a)
    assert got == _assemble_ref.find_new_variants(refseq, ref, a)
    moved = _assemble_ref.assign_reads_from_new_vars(ref, got, a)
    assemble.assign_reads_from_new_vars(cr, got, a)
    assert numpy.array_equal(cr.labels.cpu().numpy(), ref.label) and numpy.array_equal(cr.joined.cpu().numpy(), ref.joined)
    assert moved == int((ref.joined > 0).sum()) and moved > 100000 and len(got) >= 100
    for strict in (True, False):
        cons = assemble.call_consensus_all(refseq, cr, 2, a, strict=strict)
        for key in names:
            assert cons[key] == _assemble_ref.call_consensus(refseq, ref, key, 2, a, strict), (key, strict)
