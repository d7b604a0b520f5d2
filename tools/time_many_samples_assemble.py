#!/usr/bin/env python
"""
The third stage of a cohort run -- one label per alignment, `-x` (assembly extension) and `-b` (consensus FASTA) -- two
routes alternated in one process over the same assign.finish_many results:

    per sample   a loop of assign.assign_reads -> assemble.extend_assemblies -> assemble.write_consensus_seqs
    cohort       assign.assign_reads_many -> assemble.extend_assemblies_many -> assemble.write_consensus_seqs_many

    python tools/time_many_samples_assemble.py [--sets 64,256,ragged] [--repeats 5] [--frags 960]

Samples: synth.synth_alignments(tables, refseq, frags, seed=SEED0 + s, private=gen_golden.g18_private(refseq, tables)) --
the planted variants give the extension something to move -- through alignments.encode_alignments; "ragged": 64 samples of
80 .. 7000 fragments (numpy.random.default_rng(5).integers).  The first EM and finish_many are shared and not timed.  Both
routes pay their uploads of the alignments.  Wall times end in a synchronise; the first round warms both routes up and is
not counted; the median, min and max of the others are reported.  The tool asserts that both routes give the same labels,
joined rounds, round counts and FASTA files, and exits non-zero when at S = 64 the cohort route's median is not below the
per-sample route's (the per-sample route is the yardstick: no further margin, the cohort route is opt-in and must merely
not lose).
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch
import gen_golden
from mixemt_amd import alignments, assemble, assign, em, phylotree, preprocess, synth

SEED0 = 1000

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="64,256,ragged")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--frags", type=int, default=960)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
private = gen_golden.g18_private(refseq, tables)
args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False, min_reads=10, contributors=None,
                          var_check=False, refine_ests=True, min_fold=2.0, min_mq=30, min_bq=30, cons_cov=2, cons_prefix=None)
print("device: %s; %d haplogroups; %d planted variants" % (torch.cuda.get_device_name(0), len(haps), len(private)), flush=True)


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
    assert all(len(f["contribs"]) >= 1 and f["posterior"] is not None for f in fin), "a sample without contributors"
    extend = [s for s in range(n) if len(fin[s]["contribs"]) > 1]                  # bin/mixemt:329
    each_fa = [os.path.join(tmp, "%s_each_%d" % (name, s)) for s in range(n)]
    many_fa = [os.path.join(tmp, "%s_many_%d" % (name, s)) for s in range(n)]
    t_cohort, t_each = [], []
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        cohort = assign.assign_reads_many(cols, fin, reads, args)
        assemble.extend_assemblies_many(refseq, cohort, args)
        assemble.write_consensus_seqs_many(refseq, [f["contribs"] for f in fin], cohort, args, many_fa)
        torch.cuda.synchronize(); dt_c = time.perf_counter() - t0
        torch.cuda.synchronize(); t1 = time.perf_counter()
        each = []
        for s in range(n):
            f = fin[s]
            cr = assign.assign_reads(cols[s], f["contribs"], (f["refined"]["props"], f["posterior"]), f["sub_haps"], reads[s], args)
            if s in extend:
                assemble.extend_assemblies(refseq, cr, args)
            args.cons_prefix = each_fa[s]
            assemble.write_consensus_seqs(refseq, f["contribs"], cr, args)
            each.append(cr)
        torch.cuda.synchronize(); dt_e = time.perf_counter() - t1
        if rep:
            t_cohort.append(dt_c); t_each.append(dt_e)
    same = 0
    for s in range(n):
        got = cohort.sample(s)
        same += (torch.equal(got.labels, each[s].labels) and torch.equal(got.joined, each[s].joined) and got.rounds == each[s].rounds
                 and list(got) == list(each[s]) and read(many_fa[s] + ".fa") == read(each_fa[s] + ".fa"))
    rounds = [cohort.rounds[s] for s in extend] or [0]
    moved = sum(r[0] for s in extend for r in cohort.round_log[s])
    tc, te = numpy.median(t_cohort), numpy.median(t_each)
    print("set %-7s S = %3d, fragments %d .. %d, alignments %d, labels %d; %d samples extended, rounds %d .. %d (shared rounds: %d), "
          "%d alignments moved" % (name, n, min(frags), max(frags), len(cohort.cols), cohort.n_labels, len(extend),
                                   min(rounds), max(rounds), max(rounds), moved))
    print("    labels, joined, rounds, keys and FASTA files equal for %d of %d samples" % (same, n))
    print("    cohort       %9.2f ms (min %.2f, max %.2f of %d)   %8.1f us per sample"
          % (tc * 1e3, min(t_cohort) * 1e3, max(t_cohort) * 1e3, len(t_cohort), tc * 1e6 / n))
    print("    per sample   %9.2f ms (min %.2f, max %.2f)          %8.1f us per sample"
          % (te * 1e3, min(t_each) * 1e3, max(t_each) * 1e3, te * 1e6 / n))
    print("    ratio cohort / per sample  %.3f" % (tc / te), flush=True)
    if same != n:
        raise SystemExit("the two routes disagree")
    if name == "64" and not tc < te:
        raise SystemExit("acceptance: at S = 64 the cohort route's median must be below the per-sample route's")


with tempfile.TemporaryDirectory() as tmp_dir:
    for set_name in opts.sets.split(","):
        if set_name == "ragged":
            measure(set_name, [int(v) for v in numpy.random.default_rng(5).integers(80, 7001, size=64)], tmp_dir)
        else:
            measure(set_name, [opts.frags] * int(set_name), tmp_dir)
