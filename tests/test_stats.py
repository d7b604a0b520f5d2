"""
mixemt's `-t` tables and contributor report (mixemt_amd/stats.py) against the reference's own run (g17,
tools/gen_golden.py), with the pileups restated in numpy (tests/_pileup_ref.py) instead of the device's labelled call.
The device side is tests/test_gpu_stats.py.
"""
import argparse
import collections
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
from test_gpu_observe import _subset  # noqa: E402
from test_observe import g16_columns, g16_table  # noqa: E402

CASES = ("default", "unassigned", "one")


@pytest.fixture(scope="module")
def phy():
    from mixemt_amd import phylotree
    refseq = phylotree.load_rsrs()
    return phylotree.load_build17(refseq)


def stat_args(prefix=None):
    return argparse.Namespace(stats_prefix=prefix, min_mq=30, min_bq=30, min_var_reads=3, frac_var_reads=0.02)


def g17_contribs(g, case):
    return [[name, hap, float(prop)] for name, hap, prop in
            (line.split("\t") for line in str(g[case + "_contribs"]).split("\n") if line)]


def numpy_tables(cols, g, case, L):
    """The reference's per-key alignments (g17's aln_key) counted by the numpy restatement: key -> [L][16]."""
    keys = str(g[case + "_keys"]).split("\n")
    aln_key = g[case + "_aln_key"]
    return {key: _pileup_ref.pileup(_subset(cols, numpy.flatnonzero(aln_key == k)), L) for k, key in enumerate(keys)}


def test_g17_is_made_from_g16s_alignments():
    import hashlib
    g16, g17 = golden("g16_observe"), golden("g17_stats")
    cols = g16_columns(g16)
    h = hashlib.sha256()
    for name in ("ref_start", "mapq", "frag", "cig_ptr", "cigar", "seq_ptr", "seq", "qual", "has_qual", "is_reverse"):
        h.update(numpy.ascontiguousarray(getattr(cols, name)).tobytes())
    h.update("\n".join(cols.names).encode())
    assert h.hexdigest() == str(g17["columns_sha256"])
    assert [int(s) for s in g17["seeds"][:2]] == [int(s) for s in g16["seeds"]]


@pytest.mark.parametrize("case", CASES)
def test_write_variants_bytes(phy, case):
    from mixemt_amd import observe, stats
    g16, g17 = golden("g16_observe"), golden("g17_stats")
    all_obs = observe.ObservedBases(g16_table(g16, 16589))
    out = io.StringIO()
    stats.write_variants(out, phy, g17_contribs(g17, case), all_obs, stat_args())
    assert out.getvalue() == str(g17[case + "_pos_tab"])
    # the generic path (an object with the reference's obs_at / total_obs only) writes the same bytes
    if case == "default":
        plain = argparse.Namespace(obs_at=all_obs.obs_at, total_obs=all_obs.total_obs)
        out2 = io.StringIO()
        stats.write_variants(out2, phy, g17_contribs(g17, case), plain, stat_args())
        assert out2.getvalue() == out.getvalue()


@pytest.mark.parametrize("case", CASES)
def test_write_statistics_bytes(phy, case, monkeypatch):
    from mixemt_amd import observe, stats
    g16, g17 = golden("g16_observe"), golden("g17_stats")
    cols = g16_columns(g16)
    L = observe.pileup_length(cols, 30, len(phy.refseq))
    tables = numpy_tables(cols, g17, case, L)
    keys = str(g17[case + "_keys"]).split("\n")
    contrib_reads = {key: [] for key in reversed(keys)}          # (the file order comes from sorting the keys)
    seen = []

    def fake_tables(cr, ks, min_mq, min_bq, ref_len):
        seen.append((list(ks), min_mq, min_bq, ref_len))
        return {k: tables[k].astype(numpy.uint32) for k in ks}

    monkeypatch.setattr(stats, "contrib_tables", fake_tables)
    all_obs = observe.ObservedBases(g16_table(g16, 16589))
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "run")
        stats.write_statistics(phy, all_obs, g17_contribs(g17, case), contrib_reads, stat_args(prefix))
        with open(prefix + ".pos.tab") as fin:
            assert fin.read() == str(g17[case + "_pos_tab"])
        with open(prefix + ".obs.tab") as fin:
            assert fin.read() == str(g17[case + "_obs_tab"])
    assert seen == [(sorted(keys), 30, 30, len(phy.refseq))]


def test_the_cases_cover_their_branches():
    g17 = golden("g17_stats")
    keys = {case: str(g17[case + "_keys"]).split("\n") for case in CASES}
    names = {case: [c[0] for c in g17_contribs(g17, case)] for case in CASES}
    # default: >= 2 contributors with alignments, and unassigned ones
    assert len(names["default"]) >= 2 and "unassigned" in keys["default"]
    assert all((g17["default_aln_key"] == keys["default"].index(n)).any() for n in names["default"])
    # everything unassigned: the contributors are keys with no alignment (report_contributors made them)
    for n in names["unassigned"]:
        assert n in keys["unassigned"] and not (g17["unassigned_aln_key"] == keys["unassigned"].index(n)).any()
    # one contributor: no 'unassigned' key and no 'all<TAB>mix' block
    assert keys["one"] == names["one"] and len(names["one"]) == 1
    assert "\nall\tmix\t" not in str(g17["one_obs_tab"])
    # dropped fragments' alignments are in no table
    assert (g17["default_aln_key"] < 0).any()


def test_report_contributors_both_forms():
    from mixemt_amd import stats
    g17 = golden("g17_stats")
    for case in CASES:
        keys = str(g17[case + "_keys"]).split("\n")
        aln_key = g17[case + "_aln_key"]
        contrib_reads = {key: list(numpy.flatnonzero(aln_key == k)) for k, key in enumerate(keys)}
        contribs = g17_contribs(g17, case)
        # the reference's table was made before report_contributors added the zero-alignment keys
        reads = {key: val for key, val in contrib_reads.items() if val}
        dd = collections.defaultdict(list, reads)
        out = io.StringIO()
        stats.report_contributors(out, contribs, dd)
        assert out.getvalue() == str(g17[case + "_report"]), case
        assert sorted(dd) == keys

    class Tty(io.StringIO):
        def isatty(self):
            return True

    out = Tty()
    contribs = [["hap1", "H1a", 0.61234], ["hap10", "U5a1b1", 0.01]]
    stats.report_contributors(out, contribs, {"hap1": [0] * 1234, "hap10": [1] * 7})
    assert out.getvalue() == ("hap#   Haplogroup      Contribution   Reads\n"
                              "-------------------------------------------\n"
                              "hap1   H1a                   0.6123    1234\n"
                              "hap10  U5a1b1                0.0100       7\n")


def test_polymorphic_sites_against_the_reference_on_the_toy_tree():
    from mixemt_amd import phylotree
    toy = phylotree.example()
    want = json.loads(str(golden("g17_stats")["toy_polymorphic"]))
    assert len(want) == 14
    for key, sites in want.items():
        ref, haps = key.split("|")
        assert toy.polymorphic_sites(haps.split(","), ref) == sites, key
    toy.refseq = "A" * 10
    assert toy.polymorphic_sites(["A", "C"]) == want["AAAAAAAAAA|A,C"]


def _toy_obs(rows, L=10):
    from mixemt_amd import observe
    counts = numpy.zeros((L, 16), dtype=numpy.uint32)
    for pos, vals in rows.items():
        counts[pos, :len(vals)] = vals
    return observe.ObservedBases(counts)


def test_the_stale_threshold_of_the_reference():
    """write_variants' threshold comes from the LAST variant position of the contributors, not the row's."""
    from mixemt_amd import phylotree, stats
    toy = phylotree.example()
    toy.refseq = "A" * 10
    contribs = [["hap1", "B", 0.5], ["hap2", "D", 0.5]]       # D's last variant: A9T (position 8)
    # position 8: 1000 observations -> threshold max(3, 1000 * 0.02) = 20 for every row
    # position 2: A 10, T 10 -> 'variant' by its own threshold (3), 'sample_fixed' by the stale one
    # position 4: A 30, T 25 -> 'variant' by either
    obs = _toy_obs({8: [500, 0, 0, 500], 2: [10, 0, 0, 10], 4: [30, 0, 0, 25]})
    out = io.StringIO()
    stats.write_variants(out, toy, contribs, obs, stat_args())
    lines = out.getvalue().splitlines()
    assert len(lines) == 10
    assert lines[2] == "3\t10\t0\t0\t10\tfixed\tsample_fixed\tB:A3T,D:A3T"
    assert lines[4] == "5\t30\t0\t0\t25\tfixed\tvariant\tB:A5T,D:A5T"
    assert lines[8] == "9\t500\t0\t0\t500\tpolymorphic\tvariant\tD:A9T"
    assert lines[0] == "1\t0\t0\t0\t0\tfixed\tsample_fixed\tB:A1G,D:A1G"
    assert [ln.split("\t")[5] for ln in lines] == ["fixed"] * 5 + ["polymorphic"] * 4 + ["fixed"]
    # a per-position threshold would have called position 2 'variant'
    per_pos = max(3, obs.total_obs(2) * 0.02)
    assert obs.obs_at(2, "A") >= per_pos and obs.obs_at(2, "T") >= per_pos
    # contributors without variants: the reference's UnboundLocalError
    toy.add_custom_hap("Z", [])
    with pytest.raises(UnboundLocalError):
        stats.write_variants(io.StringIO(), toy, [["hap1", "Z", 1.0]], obs, stat_args())


def test_obs_tab_sorts_the_keys_as_strings(phy, monkeypatch):
    from mixemt_amd import observe, stats
    contribs = [["hap%d" % i, "H%d" % i, 1.0 / 11] for i in range(1, 11)]
    keys = ["unassigned"] + [c[0] for c in contribs] + ["stray"]

    def fake_tables(cr, ks, min_mq, min_bq, ref_len):
        return {k: numpy.full((ref_len, 16), i + 1, dtype=numpy.uint32) for i, k in enumerate(ks)}

    monkeypatch.setattr(stats, "contrib_tables", fake_tables)
    toy = argparse.Namespace(refseq="ACGT", hap_var={c[1]: ["A1G"] for c in contribs},
                             polymorphic_sites=lambda haps, ref=None: [])
    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "run")
        stats.write_statistics(toy, observe.ObservedBases(numpy.zeros((4, 16), numpy.uint32)), contribs,
                               {k: [] for k in keys}, stat_args(prefix))
        with open(prefix + ".obs.tab") as fin:
            lines = fin.read().splitlines()
    order = []
    for line in lines:
        if line.split("\t")[0] not in order:
            order.append(line.split("\t")[0])
    assert order == ["hap1", "hap10", "hap2", "hap3", "hap4", "hap5", "hap6", "hap7", "hap8", "hap9", "stray",
                     "unassigned", "all"]
    assert lines[0] == "hap1\tH1\t0\t2\t2\t2\t2\t14"
    assert lines[4] == "hap10\tH10\t0\t4\t4\t4\t4\t28"
    assert [ln.split("\t")[1] for ln in lines if ln.startswith(("stray", "unassigned", "all"))] == \
        ["unassigned"] * 8 + ["mix"] * 4
