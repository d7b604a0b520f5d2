#!/usr/bin/env python
"""
assign.finish_many (the batched second half of a cohort run: votes, contributors, refinement EM and read assignment of
all samples in batched device passes) against the Python loop of the existing per-sample functions over the same records
and the same em.run_em_many results, in one process, alternated, the same initial proportions.

    python tools/time_many_samples_finish.py [--sets 64,256,ragged] [--repeats 3] [--rows 600]
    python tools/time_many_samples_finish.py --sweep 600,4600,30000,100000      # S = 64 at each size: the table behind max_rows

Samples: synth.synth_reads(tables, ref_len, rows, seed=SEED0 + s), unit weights; "ragged": 64 samples of 50 .. 5000 rows
(numpy.random.default_rng(5).integers).  From 30 000 rows on the sweep builds eight distinct samples and lists each eight
times (views of the same records: the per-sample work is the same, the build is eight times shorter).
The per-sample loop, once per sample: assign.get_contributors_records -> preprocess.reduce_em_records -> em.run_em_ex on
R x K -> assign.update_contribs -> assign._assign_rows, and the labels' read-back.  Both routes draw their refinement
inits from numpy.random.seed(7): sample after sample, so they start from the same proportions.
Wall times include everything a caller pays once run_em_many's results exist.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch
from mixemt_amd import assign, em, phylotree, preprocess, synth

SEED0 = 1000

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="64,256,ragged")
ap.add_argument("--sweep", default="")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rows", type=int, default=600)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False, min_reads=10, contributors=None,
                          var_check=False, refine_ests=True, min_fold=2.0)
print("device: %s; %d haplogroups; tolerance %g, min_reads %d, min_fold %g"
      % (torch.cuda.get_device_name(0), len(haps), args.tolerance, args.min_reads, args.min_fold))


def per_sample_loop(views, wts, results):
    out = []
    for cm, w, res in zip(views, wts, results):
        contribs = assign.get_contributors_records(None, None, haps, w, res["props"], cm, res["ln_theta_k"], args)
        sub, names = preprocess.reduce_em_records(cm, haps, contribs)
        run = em.run_em_ex(sub, w, args)
        contribs = assign.update_contribs(contribs, (run["props"], run["read_mix"]), names)
        table, assigned = assign._assign_rows(contribs, (run["props"], run["read_mix"]), names, cm.n_rows, args.min_fold)
        label = numpy.zeros(cm.n_rows, dtype=numpy.int32) if assigned is None else assigned.cpu().numpy()
        out.append({"contribs": contribs, "iters": run["iters"], "props": run["props"], "row_label": label})
    return out


def measure(name, counts, distinct=None):
    distinct = len(counts) if distinct is None else distinct
    csr = [synth.synth_reads(tables, len(refseq), n, seed=SEED0 + s)[:3] for s, n in enumerate(counts[:distinct])]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    own = [cm.rows(row0[s], row0[s + 1]) for s in range(distinct)]
    numpy.random.seed(7)
    first = em.run_em_many([(v, numpy.ones(v.n_rows)) for v in own], args)
    views = [own[s % distinct] for s in range(len(counts))]
    results = [first[s % distinct] for s in range(len(counts))]
    wts = [numpy.ones(v.n_rows) for v in views]
    samples = list(zip(views, wts))
    t_batch, t_seq = [], []
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        numpy.random.seed(7)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        many = assign.finish_many(samples, results, haps, args, max_rows=10 ** 9)
        torch.cuda.synchronize(); dt_b = time.perf_counter() - t0
        numpy.random.seed(7)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        one = per_sample_loop(views, wts, results)
        torch.cuda.synchronize(); dt_s = time.perf_counter() - t0
        if rep:
            t_batch.append(dt_b); t_seq.append(dt_s)
    assert all(r["route"] == "batch" for r in many)
    same_iters = sum(a["refined"]["iters"] == b["iters"] for a, b in zip(many, one))
    same_tables = sum([c[:2] for c in a["contribs"]] == [c[:2] for c in b["contribs"]] for a, b in zip(many, one))
    dprops = max(float(numpy.abs(a["refined"]["props"] - b["props"]).max()) for a, b in zip(many, one))
    dlabel = sum(int((a["row_label"] != b["row_label"]).sum()) for a, b in zip(many, one))
    tb, ts = numpy.median(t_batch), numpy.median(t_seq)
    print("set %-7s S = %3d, rows %d .. %d (%d in all), contributors %d .. %d: tables equal for %d, iterations equal for %d of %d "
          "samples, max |props batch - per sample| %.2e, %d row labels differ"
          % (name, len(counts), min(counts), max(counts), sum(counts), min(len(r["contribs"]) for r in many),
             max(len(r["contribs"]) for r in many), same_tables, same_iters, len(counts), dprops, dlabel))
    print("    finish_many  %9.2f ms (min %.2f, max %.2f of %d)   %7.1f us per sample"
          % (tb * 1e3, min(t_batch) * 1e3, max(t_batch) * 1e3, len(t_batch), tb * 1e6 / len(counts)))
    print("    per sample   %9.2f ms (min %.2f, max %.2f)          %7.1f us per sample"
          % (ts * 1e3, min(t_seq) * 1e3, max(t_seq) * 1e3, ts * 1e6 / len(counts)))
    print("    ratio finish_many / per sample  %.3f" % (tb / ts), flush=True)
    return tb, ts


if opts.sweep:
    table = []
    for rows in (int(v) for v in opts.sweep.split(",")):
        tb, ts = measure("%d" % rows, [rows] * 64, distinct=8 if rows >= 30000 else None)
        table.append((rows, ts, tb))
    print("rows per sample | per-sample loop ms | finish_many ms | ratio")
    for rows, ts, tb in table:
        print("%15d | %18.2f | %14.2f | %.3f" % (rows, ts * 1e3, tb * 1e3, tb / ts))
else:
    for name in opts.sets.split(","):
        if name == "ragged":
            measure(name, [int(v) for v in numpy.random.default_rng(5).integers(50, 5001, size=64)])
        else:
            measure(name, [opts.rows] * int(name))
