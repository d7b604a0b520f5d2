#!/usr/bin/env python
"""
The second half of a cohort run WITH the variant check (mixemt's default), two routes alternated in one process over the
same records and the same em.run_em_many results:

    per sample   observe.observe_bases per sample (upload, pileup, read-back of the table), then
                 assign.finish_many(obs=[ObservedBases, ...]): check_contrib_phy_vars per sample on the host
    cohort       observe.observe_bases_many (one upload, one labelled pileup call, tables stay on the device), then
                 assign.finish_many(obs=CohortPileup): one mxm_check_variants_samples call

    python tools/time_many_samples_varcheck.py [--sets 64,256,ragged] [--repeats 5] [--frags 960]

Samples: synth.synth_alignments(tables, refseq, frags, seed=SEED0 + s) through alignments.encode_alignments; "ragged": 64
samples of 80 .. 7000 fragments (numpy.random.default_rng(5).integers).  Both routes pay their pileups and uploads; the
first EM is shared and not timed.  Wall times end in a synchronise; the first round warms both routes up and is not
counted.  The tree's VarCheckTables are built once (their time is printed) and handed to every cohort call, as a caller
with more than one cohort would.  Both routes draw their refinement inits from numpy.random.seed(7).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch
from mixemt_amd import alignments, assign, em, observe, phylotree, preprocess, synth

SEED0 = 1000

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="64,256,ragged")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--frags", type=int, default=960)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False, min_reads=10, contributors=None,
                          var_check=True, min_var_reads=3, frac_var_reads=0.02, var_fraction=0.5, var_count=None,
                          refine_ests=True, min_fold=2.0)
dev = torch.device("cuda")
t0 = time.perf_counter()
var_tables = assign.VarCheckTables.build(phy, haps, dev)
torch.cuda.synchronize()
print("device: %s; %d haplogroups; VarCheckTables.build %.1f ms (%d keys, once per tree)"
      % (torch.cuda.get_device_name(0), len(haps), (time.perf_counter() - t0) * 1e3, len(var_tables.key_h)), flush=True)


def measure(name, frags):
    cols = [synth.synth_alignments(tables, refseq, n, seed=SEED0 + s) for s, n in enumerate(frags)]
    encs = [alignments.encode_alignments(c, tables.sites, len(refseq), 30, 30) for c in cols]
    cm, row0 = preprocess.build_em_records_many(tables, [(e.row_ptr, e.site, e.obs) for e in encs])
    samples = [(cm.rows(row0[s], row0[s + 1]), e.weights.astype(numpy.float64)) for s, e in enumerate(encs)]
    numpy.random.seed(7)
    results = em.run_em_many(samples, args)
    rows = [m.n_rows for m, _ in samples]
    t_cohort, t_each, t_pile_c, t_pile_e = [], [], [], []
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        numpy.random.seed(7)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        pileup = observe.observe_bases_many(cols, 30, 30, ref_len=len(refseq))
        torch.cuda.synchronize(); t1 = time.perf_counter()
        many = assign.finish_many(samples, results, haps, args, phylo=phy, obs=pileup, var_tables=var_tables, max_rows=10 ** 9)
        torch.cuda.synchronize(); dt_c = time.perf_counter() - t0
        numpy.random.seed(7)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        obs = [observe.observe_bases(c, 30, 30, ref_len=len(refseq)) for c in cols]
        torch.cuda.synchronize(); t3 = time.perf_counter()
        each = assign.finish_many(samples, results, haps, args, phylo=phy, obs=obs, max_rows=10 ** 9)
        torch.cuda.synchronize(); dt_e = time.perf_counter() - t2
        if rep:
            t_cohort.append(dt_c); t_each.append(dt_e); t_pile_c.append(t1 - t0); t_pile_e.append(t3 - t2)
        del pileup, obs
    assert all(r["var_check"] == "device" for r in many) and all(r["var_check"] == "host" for r in each)
    same_tables = sum(a["contribs"] == b["contribs"] for a, b in zip(many, each))
    same_labels = sum(numpy.array_equal(a["row_label"], b["row_label"]) for a, b in zip(many, each))
    dropped = sum(len(pending) - len(r["contribs"]) for pending, r in
                  zip(([h for h in r["vote_order"] if r["votes"][h] >= args.min_reads] for r in many), many))
    tc, te = numpy.median(t_cohort), numpy.median(t_each)
    print("set %-7s S = %3d, fragments %d .. %d, rows %d .. %d (%d in all), contributors %d .. %d, candidates the check dropped: %d"
          % (name, len(frags), min(frags), max(frags), min(rows), max(rows), sum(rows), min(len(r["contribs"]) for r in many),
             max(len(r["contribs"]) for r in many), dropped))
    print("    contributor tables equal for %d, row labels equal for %d of %d samples; %d on the batch route"
          % (same_tables, same_labels, len(frags), sum(r["route"] == "batch" for r in many)))
    print("    cohort       %9.2f ms (min %.2f, max %.2f of %d)   of it the pileup %8.2f ms   %8.1f us per sample"
          % (tc * 1e3, min(t_cohort) * 1e3, max(t_cohort) * 1e3, len(t_cohort), numpy.median(t_pile_c) * 1e3, tc * 1e6 / len(frags)))
    print("    per sample   %9.2f ms (min %.2f, max %.2f)          of it the pileups %7.2f ms   %8.1f us per sample"
          % (te * 1e3, min(t_each) * 1e3, max(t_each) * 1e3, numpy.median(t_pile_e) * 1e3, te * 1e6 / len(frags)))
    print("    ratio cohort / per sample  %.3f" % (tc / te), flush=True)
    if same_tables != len(frags) or same_labels != len(frags):
        raise SystemExit("the two routes disagree")
    if name == "64" and not tc < te:
        raise SystemExit("acceptance: at S = 64 the cohort route's median must be below the per-sample route's")


for name in opts.sets.split(","):
    if name == "ragged":
        measure(name, [int(v) for v in numpy.random.default_rng(5).integers(80, 7001, size=64)])
    else:
        measure(name, [opts.frags] * int(name))
