"""
The variant check's CPU side against the reference's own run (g16, tools/gen_golden.py): the pileup's numpy restatement,
ObservedBases' queries, _check_contrib_phy_vars / get_contributors, get_ancestral, write_base_obs; the strand column of
the alignment front end.  The device pileup is tests/test_gpu_observe.py.
"""
import argparse
import hashlib
import io
import json
import os
import sys
import tempfile

import numpy
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pileup_ref  # noqa: E402


def g16_columns(g):
    from mixemt_amd.alignments import AlignmentColumns
    return AlignmentColumns(g["ref_start"], g["mapq"], g["frag"], g["cig_ptr"], g["cigar"], g["seq_ptr"], g["seq"],
                            g["qual"], g["has_qual"], str(g["names"]).split("\n"), g["is_reverse"])


def g16_table(g, L):
    return _pileup_ref.from_triplets(g["trip_pos"], str(g["trip_key"]), g["trip_count"], L)


@pytest.fixture(scope="module")
def phy():
    from mixemt_amd import phylotree
    refseq = phylotree.load_rsrs()
    return phylotree.load_build17(refseq)


def asm_args(**kw):
    args = argparse.Namespace(min_reads=10, contributors=None, var_check=True, min_fold=2.0, min_var_reads=3,
                              frac_var_reads=0.02, var_fraction=0.5, var_count=None, verbose=False)
    for key, val in kw.items():
        setattr(args, key, val)
    return args


VARIANTS = [("default", {}), ("var_count_1", {"var_count": 1}), ("var_fraction_0.9", {"var_fraction": 0.9}),
            ("min_var_reads_10", {"min_var_reads": 10})]


def want_contribs(g, label):
    return [line.split("\t") for line in str(g["contribs_" + label]).split("\n") if line]


def test_numpy_pileup_equals_the_reference_table():
    from mixemt_amd import observe
    g = golden("g16_observe")
    cols = g16_columns(g)
    L = observe.pileup_length(cols, 30, 16569)
    assert L == 16569 + 20                                   # one read runs 20 positions off the end
    assert numpy.array_equal(_pileup_ref.pileup(cols, L), g16_table(g, L))


def test_get_contributors_with_the_check_reproduces_the_reference(phy, monkeypatch):
    from mixemt_amd import assign, observe
    g = golden("g16_observe")
    haps = sorted(phy.hap_var)
    obs = observe.ObservedBases(g16_table(g, 16589))
    cand = [int(c) for c in g["candidates"]]
    monkeypatch.setattr(assign, "find_contribs_from_reads", lambda mat, wts, args: list(cand))
    for label, kw in VARIANTS:
        got = assign.get_contributors(phy, obs, haps, g["weights"], (g["props"], None), asm_args(**kw))
        want = want_contribs(g, label)
        assert [c[:2] for c in got] == [w[:2] for w in want], label
        assert [float(c[2]) for c in got] == [float(w[2]) for w in want], label
    # the default check drops a candidate: the branch this feature exists for
    assert len(want_contribs(g, "default")) < len(cand)
    # verbose lines as the reference writes them
    err, sys.stderr = sys.stderr, io.StringIO()
    try:
        assign.get_contributors(phy, obs, haps, g["weights"], (g["props"], None), asm_args(verbose=True))
        text = sys.stderr.getvalue()
    finally:
        sys.stderr = err
    assert text == str(g["verbose_text"])
    # -C overrides (and switches the check off); an unknown name is the reference's ValueError
    got = assign.get_contributors(phy, obs, haps, g["weights"], (g["props"], None), asm_args(contributors=haps[cand[2]]))
    assert [c[1] for c in got] == [haps[cand[2]]] and got[0][0] == "hap1"
    with pytest.raises(ValueError, match="Unknown haplogroup"):
        assign.get_contributors(phy, obs, haps, g["weights"], (g["props"], None), asm_args(contributors="nope"))


def test_get_ancestral_equals_the_reference(phy):
    g = golden("g16_observe")
    want = json.loads(str(g["ancestral"]))
    for hap, pairs in want.items():
        assert sorted(phy.get_ancestral(hap)) == [tuple(p) for p in pairs], hap


def test_write_base_obs_bytes(phy):
    from mixemt_amd import io as mio
    from mixemt_amd import observe
    g = golden("g16_observe")
    obs = observe.ObservedBases(g16_table(g, 16589))
    buf = io.StringIO()
    mio.write_base_obs(buf, obs, phy.refseq, prefix="s1")
    assert buf.getvalue() == str(g["base_obs"])
    # the generic path (any object with obs_at / obs_tab) writes the same bytes
    plain = argparse.Namespace(obs_at=obs.obs_at, obs_tab=obs.obs_tab)
    buf2 = io.StringIO()
    mio.write_base_obs(buf2, plain, phy.refseq[:300], prefix="s1")
    assert buf2.getvalue() == "".join(str(g["base_obs"]).splitlines(True)[:300])


def test_observed_bases_queries():
    from mixemt_amd import observe
    counts = numpy.zeros((4, 16), dtype=numpy.uint32)
    counts[1, [0, 4, 5, 6, 7, 12, 13]] = [5, 1, 2, 3, 4, 6, 7]          # A N other - a other' +
    obs = observe.ObservedBases(counts)
    assert obs.obs_at(1, "A") == 9 and obs.obs_at(1, "a", stranded=True) == (5, 4)
    assert obs.obs_at(1, "-") == 10 and obs.obs_at(1, "+", stranded=True) == (3, 7)
    assert obs.obs_at(1, "N") == 1 and obs.obs_at(1, "C") == 0 and obs.obs_at(9, "A") == 0
    assert obs.total_obs(1) == 9 and obs.total_obs(99) == 0
    assert obs.obs_at(1) == {"A": 9, "N": 1, "X": 8, "-": 10}
    assert obs.obs_at(1, stranded=True) == {"A": 5, "N": 1, "X": 2, "-": 3, "a": 4, "x": 6, "+": 7}
    assert obs.obs_tab[1] == obs.obs_at(1, stranded=True) and obs.obs_tab[0] == {} and obs.obs_tab[50] == {}
    assert list(obs.obs_tab) == [1] and 1 in obs.obs_tab and 2 not in obs.obs_tab
    for bad in ("Q", "x", "*"):
        with pytest.raises(ValueError, match="Bad base"):
            obs.obs_at(1, bad)


def test_synth_alignments_columns_unchanged_by_the_strand_column():
    """Digest of a seed-1 run of synth_alignments' columns taken before the strand column was added."""
    from mixemt_amd import phylotree, preprocess, synth
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    tables = preprocess.HapVarTables.build(refseq, phy, sorted(phy.hap_var))
    cols = synth.synth_alignments(tables, refseq, 3000, seed=1)
    h = hashlib.sha256()
    for name in ("ref_start", "mapq", "frag", "cig_ptr", "cigar", "seq_ptr", "seq", "qual", "has_qual"):
        h.update(getattr(cols, name).tobytes())
    h.update("\n".join(cols.names).encode())
    assert h.hexdigest() == "4ffd0aa40aff6ee773c6452f37ccb032e2c90c1d8d99645e89e4449acb30d046"
    mate = numpy.zeros(len(cols), dtype=bool)
    first = numpy.full(cols.n_frag, -1)
    for i, f in enumerate(cols.frag):                          # the later alignment of a fragment is not always the mate,
        if first[f] >= 0:                                      # but every fragment with two has one reverse
            mate[i] = True
        first[f] = i
    two = numpy.bincount(cols.frag, minlength=cols.n_frag) == 2
    rev_per_frag = numpy.bincount(cols.frag, weights=cols.is_reverse, minlength=cols.n_frag)
    assert (rev_per_frag[two] >= 1).all()
    single = ~two[cols.frag]
    assert 0.4 < cols.is_reverse[single].mean() < 0.6


def test_is_reverse_flows_through_the_front_end():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _bam_writer
    from _pileup_aln import PileupAln
    from mixemt_amd import alignments
    alns = [PileupAln("r%d" % i, 100 + i, 60, "ACGTACGTAC", [35] * 10, [(0, 10)], i % 3 == 0) for i in range(7)]
    cols = alignments.AlignmentColumns.from_alignments(alns)
    assert cols.is_reverse.tolist() == [1, 0, 0, 1, 0, 0, 1]
    # objects without the attribute: no column (all forward)
    from _fake_aln import FakeAln
    plain = alignments.AlignmentColumns.from_alignments([FakeAln("x", 5, 60, "ACGT", None, "4M")])
    assert plain.is_reverse is None
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s.bam")
        _bam_writer.write_bam(path, cols, flag=numpy.where(cols.is_reverse == 1, 0x10 | 0x1, 0x1))
        back = alignments.read_bam(path, n_threads=1)
    assert back.is_reverse.tolist() == cols.is_reverse.tolist()
    assert back.flag.tolist() == [0x11, 1, 1, 0x11, 1, 1, 0x11]
