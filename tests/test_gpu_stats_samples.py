"""
mixemt's `-t` tables for ALL samples of a cohort (stats.write_statistics_many, stats.report_contributors_many over an
assign.CohortContribReads and an observe.CohortPileup): the reference's own files for g17's three cases run as ONE batch over
g16's alignments, and per sample the files of stats.write_statistics over cohort.sample(s) and pileup.host(s) for a cohort of
synthetic samples on the real tree -- before and after the extension has moved labels in place, and in another order.
"""
import argparse
import io
import os
import sys

import numpy
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_assemble_samples import make_cohort  # noqa: E402
from test_observe import g16_columns  # noqa: E402
from test_stats import CASES, g17_contribs, stat_args  # noqa: E402
from test_var_check_host import empty_columns  # noqa: E402

pytestmark = pytest.mark.gpu


def read(path):
    with open(path, "rb") as fin:
        return fin.read()


@pytest.fixture(scope="module")
def phy():
    from mixemt_amd import phylotree
    return phylotree.load_build17(phylotree.load_rsrs())


def full_args():
    a = stat_args()
    a.cons_cov, a.verbose = 1, False
    return a


# ---- g17: the reference's files ---------------------------------------------------------------------------------------
def g17_sample(g16_cols, g17, case, keys_with_alignments_only=False):
    """(cols, local label, names, keys) of a g17 case: the labels made by hand from the reference's per-alignment keys."""
    keys = str(g17[case + "_keys"]).split("\n")
    aln_key = g17[case + "_aln_key"]
    contribs = g17_contribs(g17, case)
    names = [c[0] for c in contribs] + (["unassigned"] if len(contribs) > 1 else [])
    lut = numpy.array([names.index(k) for k in keys] + [-1], dtype=numpy.int32)       # (the last entry serves key -1)
    label = lut[aln_key]
    if keys_with_alignments_only:                                   # the keys before report_contributors looks any up
        keys = [k for i, k in enumerate(keys) if (aln_key == i).any()]
    return g16_cols, label, names, keys


def test_g17_cases_as_one_batch(phy, tmp_path):
    from mixemt_amd import observe, stats
    g16, g17 = golden("g16_observe"), golden("g17_stats")
    cols = g16_columns(g16)
    cohort = make_cohort([g17_sample(cols, g17, case) for case in CASES])
    pileup = observe.observe_bases_many([cols] * 3, 30, 30, ref_len=len(phy.refseq))
    contribs = [g17_contribs(g17, case) for case in CASES]
    prefixes = [str(tmp_path / case) for case in CASES]
    # the cap comes before any file
    with pytest.raises(ValueError, match=r"the pos.tab text of 3 samples takes \d+ bytes, above the cap of 1000 bytes "
                                         r"\(max_text_bytes\): split the cohort"):
        stats.write_statistics_many(phy, pileup, contribs, cohort, stat_args(), prefixes, max_text_bytes=1000)
    assert os.listdir(str(tmp_path)) == []
    sizes = stats.write_statistics_many(phy, pileup, contribs, cohort, stat_args(), prefixes)
    for s, case in enumerate(CASES):
        pos, obs = read(prefixes[s] + ".pos.tab"), read(prefixes[s] + ".obs.tab")
        assert pos == str(g17[case + "_pos_tab"]).encode(), case
        assert obs == str(g17[case + "_obs_tab"]).encode(), case
        assert sizes[s] == (len(pos), len(obs))
    assert sorted(os.listdir(str(tmp_path))) == sorted(c + ext for c in CASES for ext in (".obs.tab", ".pos.tab"))


def test_report_contributors_many_then_the_zero_tables(phy, tmp_path):
    """g17's 'unassigned' case as bin/mixemt runs it: the contributors have no alignments, the report's lookup makes them
    keys, and the tables of those keys are all zeros.  Beside it the default case, in one batch."""
    from mixemt_amd import observe, stats
    g16, g17 = golden("g16_observe"), golden("g17_stats")
    cols = g16_columns(g16)
    cases = ("unassigned", "default")
    cohort = make_cohort([g17_sample(cols, g17, case, keys_with_alignments_only=True) for case in cases])
    contribs = [g17_contribs(g17, case) for case in cases]
    assert cohort.keys[0] == ["unassigned"]
    out = io.StringIO()
    stats.report_contributors_many(out, contribs, cohort, titles=list(cases))
    assert out.getvalue() == "".join("# %s\n%s" % (case, str(g17[case + "_report"])) for case in cases)
    for s, case in enumerate(cases):
        assert sorted(cohort.keys[s]) == str(g17[case + "_keys"]).split("\n"), case
    assert cohort.keys[0] == ["unassigned"] + [c[0] for c in contribs[0]]
    pileup = observe.observe_bases_many([cols] * 2, 30, 30, ref_len=len(phy.refseq))
    prefixes = [str(tmp_path / case) for case in cases]
    stats.write_statistics_many(phy, pileup, contribs, cohort, stat_args(), prefixes)
    for s, case in enumerate(cases):
        assert read(prefixes[s] + ".pos.tab") == str(g17[case + "_pos_tab"]).encode(), case
        assert read(prefixes[s] + ".obs.tab") == str(g17[case + "_obs_tab"]).encode(), case
    name = contribs[0][0][0]
    zero_line = ("%s\t%s\t5\t0\t0\t0\t0\t0\n" % (name, contribs[0][0][1])).encode()
    assert zero_line in read(prefixes[0] + ".obs.tab")


# ---- a synthetic cohort on the real tree ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic(phy):
    """Seven samples: (cols, local label, names, keys) and their contributor tables."""
    from mixemt_amd import preprocess, synth
    refseq = phy.refseq
    haps = sorted(phy.hap_var)
    tables = preprocess.HapVarTables.build(refseq, phy, haps)
    hap_of = [haps[c] for c in synth.DEFAULT_CONTRIB]
    rng = numpy.random.default_rng(77)
    three, two = ["hap1", "hap2", "hap3", "unassigned"], ["hap1", "hap2", "unassigned"]
    con3 = [["hap1", hap_of[0], 0.5], ["hap2", hap_of[1], 0.3], ["hap3", hap_of[2], 0.2]]
    con2 = [["hap1", hap_of[2], 0.75], ["hap2", hap_of[0], 0.25]]
    from mixemt_amd.alignments import concat_columns

    def sourced(contrib, n_each, seed):
        """Alignments shed by ONE contributor each, joined: -> (columns, the contributor's ordinal per alignment).  The
        label follows the source (so the contributors' consensus sequences differ and the extension has something to
        move), three in ten are 'unassigned' and a few are in no table (-1)."""
        sets = [synth.synth_alignments(tables, refseq, n_each, seed=seed + k, contrib=(c, c, c)) for k, c in enumerate(contrib)]
        cols, aln0 = concat_columns(sets)
        label = numpy.repeat(numpy.arange(len(sets)), numpy.diff(aln0)).astype(numpy.int32)
        draw = rng.random(len(label))
        label[draw < 0.3] = len(sets)
        label[draw < 0.03] = -1
        return cols, label

    c3, c2 = synth.DEFAULT_CONTRIB, (synth.DEFAULT_CONTRIB[2], synth.DEFAULT_CONTRIB[0])
    parts = [sourced(c3, 300, 60), sourced(c2, 300, 70), sourced(c2, 150, 80), sourced(c3, 200, 90)]
    (parts[0], lab0), (parts[1], lab1), (parts[2], _), (parts[3], lab3) = parts
    assert (lab0 < 0).any() and (lab0 == 3).any()
    samples = [(parts[0], lab0, list(three), list(three)),
               (parts[1], lab1, list(two), ["unassigned", "hap2", "hap1"]),                      # (keys in another order)
               (empty_columns(), numpy.zeros(0, dtype=numpy.int32), list(two), []),              # no alignments, no keys
               (parts[2], numpy.zeros(len(parts[2]), dtype=numpy.int32), ["hap1"], ["hap1"]),    # no 'unassigned' label
               (parts[3], numpy.where(lab3 == 1, -1, lab3).astype(numpy.int32), list(three), list(three)),   # hap2 has no alignments
               (parts[1], numpy.full(len(parts[1]), -1, dtype=numpy.int32), [], []),            # no contributors
               (parts[2], rng.integers(0, 2, size=len(parts[2])).astype(numpy.int32), list(two), ["hap1", "hap2"])]
    contribs = [con3, con2, con2, [["hap1", hap_of[1], 1.0]], con3, [], con2]
    return samples, contribs


def batch(phy, samples, contribs, tmp, tag, extend=False):
    """The cohort's files under tmp/<tag>_<s> -> (cohort, pileup, prefixes, the returned list)."""
    from mixemt_amd import assemble, observe, stats
    cohort = make_cohort(samples)
    if extend:
        assemble.extend_assemblies_many(phy.refseq, cohort, full_args())
    pileup = observe.observe_bases_many([s[0] for s in samples], 30, 30, ref_len=len(phy.refseq))
    prefixes = [os.path.join(str(tmp), "%s_%d" % (tag, s)) for s in range(len(samples))]
    got = stats.write_statistics_many(phy, pileup, contribs, cohort, full_args(), prefixes)
    return cohort, pileup, prefixes, got


def check_against_the_samples_alone(phy, cohort, pileup, contribs, prefixes, got, tmp):
    from mixemt_amd import stats
    for s in range(cohort.n_samples):
        if not contribs[s]:
            assert got[s] is None and not os.path.exists(prefixes[s] + ".pos.tab") and not os.path.exists(prefixes[s] + ".obs.tab")
            continue
        alone = os.path.join(str(tmp), "alone_%d" % s)
        a = full_args()
        a.stats_prefix = alone
        stats.write_statistics(phy, pileup.host(s), contribs[s], cohort.sample(s), a)
        for ext in (".pos.tab", ".obs.tab"):
            assert read(prefixes[s] + ext) == read(alone + ext), (s, ext)
        assert got[s] == (os.path.getsize(alone + ".pos.tab"), os.path.getsize(alone + ".obs.tab")), s


def test_synthetic_cohort_equals_write_statistics_per_sample(phy, synthetic, tmp_path):
    samples, contribs = synthetic
    cohort, pileup, prefixes, got = batch(phy, samples, contribs, tmp_path, "many")
    check_against_the_samples_alone(phy, cohort, pileup, contribs, prefixes, got, tmp_path)
    # what the cases are there for
    assert read(prefixes[2] + ".obs.tab") == b"" and got[2][1] == 0 and got[2][0] > 16569 * 12      # no keys: an empty obs.tab
    assert b"\nall\tmix\t" not in read(prefixes[3] + ".obs.tab") and b"all\tmix\t" in read(prefixes[0] + ".obs.tab")
    hap2 = [line for line in read(prefixes[4] + ".obs.tab").split(b"\n") if line.startswith(b"hap2\t")]
    assert len(hap2) == 16569 and all(line.endswith(b"\t0\t0\t0\t0\t0") for line in hap2)
    assert b"\tvariant\t" in read(prefixes[0] + ".pos.tab") and b"\tpolymorphic\t" in read(prefixes[0] + ".pos.tab")


def test_synthetic_cohort_after_the_extension_moved_labels(phy, synthetic, tmp_path):
    samples, contribs = synthetic
    cohort, pileup, prefixes, got = batch(phy, samples, contribs, tmp_path, "ext", extend=True)
    assert sum(r[0] for log in cohort.round_log for r in log) > 0, "the extension moved nothing"
    check_against_the_samples_alone(phy, cohort, pileup, contribs, prefixes, got, tmp_path)


def test_the_place_in_the_batch_does_not_matter(phy, synthetic, tmp_path):
    samples, contribs = synthetic
    _, _, first, got = batch(phy, samples, contribs, tmp_path, "a")
    order = [4, 6, 0, 5, 2, 1, 3]
    _, _, second, got2 = batch(phy, [samples[s] for s in order], [contribs[s] for s in order], tmp_path, "b")
    for at, s in enumerate(order):
        assert got2[at] == got[s], s
        if got[s] is None:
            continue
        for ext in (".pos.tab", ".obs.tab"):
            assert read(second[at] + ext) == read(first[s] + ext), (s, ext)
