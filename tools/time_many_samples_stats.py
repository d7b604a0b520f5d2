#!/usr/bin/env python
"""
mixemt's `-t` tables of a cohort -- PREFIX.pos.tab and PREFIX.obs.tab of every sample -- two routes alternated in one process
over the same assign.assign_reads_many result and the same observe.observe_bases_many pileup, writing to the same temporary
directory:

    per sample   a loop of stats.write_statistics(phylo, pileup.host(s), contribs, cohort.sample(s), args)
    cohort       stats.write_statistics_many(phylo, pileup, contribs_list, cohort, args, prefixes)

    python tools/time_many_samples_stats.py [--sets 64,256,ragged] [--repeats 3] [--frags 960]

Samples: synth.synth_alignments(tables, refseq, frags, seed=SEED0 + s, private=gen_golden.g18_private(refseq, tables))
through alignments.encode_alignments; "ragged": 64 samples of 80 .. 7000 fragments (numpy.random.default_rng(5).integers).
The EM, finish_many, assign_reads_many, report_contributors_many and the pileups are shared and not timed (the pileup's host
copies of the per-sample route are downloaded before its clock starts).  Wall times end in a synchronise; the first round
warms both routes up and is not counted; the median, min and max of the others are reported, and for the cohort route the
split of one further run into host plan, pileup, block tables, sizes, write, download and file write (a synchronise per phase).  The tool asserts that
both routes write the same bytes.  No ratio is required: the cohort route is opt-in, and what it cannot avoid is the download
and the file write of the text itself, which the split shows.
"""
import argparse
import io
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch
import gen_golden
from mixemt_amd import alignments, assign, em, observe, phylotree, preprocess, stats, synth

SEED0 = 1000

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="64,256,ragged")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--frags", type=int, default=960)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
private = gen_golden.g18_private(refseq, tables)
args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False, min_reads=10, contributors=None,
                          var_check=False, refine_ests=True, min_fold=2.0, min_mq=30, min_bq=30, cons_cov=2, cons_prefix=None,
                          min_var_reads=3, frac_var_reads=0.02, stats_prefix=None)
print("device: %s; %d haplogroups" % (torch.cuda.get_device_name(0), len(haps)), flush=True)


def read(path):
    with open(path, "rb") as fin:
        return fin.read()


def measure(name, frags, tmp):
    cols = [synth.synth_alignments(tables, refseq, n, seed=SEED0 + s, private=private) for s, n in enumerate(frags)]
    encs = [alignments.encode_alignments(c, tables.sites, len(refseq), 30, 30) for c in cols]
    cm, row0 = preprocess.build_em_records_many(tables, [(e.row_ptr, e.site, e.obs) for e in encs])
    samples = [(cm.rows(row0[s], row0[s + 1]), e.weights.astype(numpy.float64)) for s, e in enumerate(encs)]
    reads = [e.read_ids for e in encs]
    numpy.random.seed(7)
    results = em.run_em_many(samples, args)
    fin = assign.finish_many(samples, results, haps, args, max_rows=10 ** 9, want_posterior=True)
    n = len(frags)
    contribs = [f["contribs"] for f in fin]
    pileup = observe.observe_bases_many(cols, 30, 30, ref_len=len(refseq), keep_columns=True)
    cohort = assign.assign_reads_many(cols, fin, reads, args, pileup=pileup)
    stats.report_contributors_many(io.StringIO(), contribs, cohort)
    all_obs = [pileup.host(s) for s in range(n)]
    each = [os.path.join(tmp, "%s_each_%d" % (name, s)) for s in range(n)]
    many = [os.path.join(tmp, "%s_many_%d" % (name, s)) for s in range(n)]
    t_cohort, t_each = [], []
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        sizes = stats.write_statistics_many(phy, pileup, contribs, cohort, args, many)
        torch.cuda.synchronize(); dt_c = time.perf_counter() - t0
        torch.cuda.synchronize(); t1 = time.perf_counter()
        for s in range(n):
            if contribs[s]:
                args.stats_prefix = each[s]
                stats.write_statistics(phy, all_obs[s], contribs[s], cohort.sample(s), args)
        torch.cuda.synchronize(); dt_e = time.perf_counter() - t1
        if rep:
            t_cohort.append(dt_c); t_each.append(dt_e)
    split = {}
    stats.write_statistics_many(phy, pileup, contribs, cohort, args, many, timings=split)
    same = sum(1 for s in range(n) if not contribs[s] or all(read(many[s] + ext) == read(each[s] + ext) for ext in (".pos.tab", ".obs.tab")))
    text = sum(a + b for a, b in (sz for sz in sizes if sz is not None))
    tc, te = numpy.median(t_cohort), numpy.median(t_each)
    print("set %-7s S = %3d, fragments %d .. %d, alignments %d, labels %d; %.1f MB of text in %d files"
          % (name, n, min(frags), max(frags), len(cohort.cols), cohort.n_labels, text / 1e6, 2 * sum(1 for sz in sizes if sz)))
    print("    both files equal for %d of %d samples" % (same, n))
    print("    cohort       %9.2f ms (min %.2f, max %.2f of %d)   %8.1f us per sample"
          % (tc * 1e3, min(t_cohort) * 1e3, max(t_cohort) * 1e3, len(t_cohort), tc * 1e6 / n))
    print("    per sample   %9.2f ms (min %.2f, max %.2f)          %8.1f us per sample"
          % (te * 1e3, min(t_each) * 1e3, max(t_each) * 1e3, te * 1e6 / n))
    print("    ratio cohort / per sample  %.4f" % (tc / te))
    print("    cohort split (one run, a synchronise per phase): " +
          ", ".join("%s %.2f ms" % (k, split[k] * 1e3) for k in ("plan", "pileup", "tables", "sizes", "write", "download", "files")), flush=True)
    if same != n:
        raise SystemExit("the two routes disagree")


with tempfile.TemporaryDirectory() as tmp_dir:
    for set_name in opts.sets.split(","):
        if set_name == "ragged":
            measure(set_name, [int(v) for v in numpy.random.default_rng(5).integers(80, 7001, size=64)], tmp_dir)
        else:
            measure(set_name, [opts.frags] * int(set_name), tmp_dir)
