#!/usr/bin/env python
"""
assign.finish_many(runs="batch") -- multi-run samples (mixemt's -M) kept on the batched second half of a cohort run --
against assign.finish_many(runs="single"), the default, which sends every sample of a multi-run through the per-sample
functions: the same records, the same em.run_em_many results, the same initial proportions, in one process, alternated.

    python tools/time_many_samples_runs.py [--sets 64,256,ragged] [--runs 3,10] [--repeats 3] [--rows 600]
    python tools/time_many_samples_runs.py --sweep 600,4600,30000 --runs 3      # S = 64 at each size

Samples as tools/time_many_samples_finish.py makes them: synth.synth_reads(tables, ref_len, rows, seed=SEED0 + s), unit
weights; "ragged": 64 samples of 50 .. 5000 rows (numpy.random.default_rng(5).integers).  From 30 000 rows on the sweep
builds eight distinct samples and lists each eight times.  Both routes draw their refinement inits from
numpy.random.seed(7): B vectors per sample, sample after sample, so they start from the same proportions.
The first round warms both routes up and is not counted; every timing has a synchronise at each end.  The tool asserts that
both routes give the same contributor tables, iteration counts and row labels.
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
ap.add_argument("--runs", default="3,10")
ap.add_argument("--sweep", default="")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rows", type=int, default=600)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
print("device: %s; %d haplogroups" % (torch.cuda.get_device_name(0), len(haps)))


def measure(name, counts, n_multi, distinct=None):
    args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=n_multi, verbose=False, min_reads=10,
                              contributors=None, var_check=False, refine_ests=True, min_fold=2.0)
    distinct = len(counts) if distinct is None else distinct
    csr = [synth.synth_reads(tables, len(refseq), n, seed=SEED0 + s)[:3] for s, n in enumerate(counts[:distinct])]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    own = [cm.rows(row0[s], row0[s + 1]) for s in range(distinct)]
    numpy.random.seed(7)
    first = em.run_em_many([(v, numpy.ones(v.n_rows)) for v in own], args)
    samples = [(own[s % distinct], numpy.ones(own[s % distinct].n_rows)) for s in range(len(counts))]
    results = [first[s % distinct] for s in range(len(counts))]
    times = {"batch": [], "single": []}
    out = {}
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        for route in ("batch", "single"):
            numpy.random.seed(7)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out[route] = assign.finish_many(samples, results, haps, args, max_rows=10 ** 9, runs=route)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            if rep:
                times[route].append(dt)
    many, one = out["batch"], out["single"]
    assert all(r["route"] == "batch" for r in many) and all(r["route"] == "single" for r in one)
    dprops = max(float(numpy.abs(a["refined"]["props"] - b["refined"]["props"]).max()) for a, b in zip(many, one))
    print("set %-7s S = %3d, B = %2d, rows %d .. %d (%d in all), contributors %d .. %d, iterations %d .. %d; "
          "max |props batch - single| %.2e"
          % (name, len(counts), n_multi, min(counts), max(counts), sum(counts), min(len(r["contribs"]) for r in many),
             max(len(r["contribs"]) for r in many), min(min(r["refined"]["iters"]) for r in many),
             max(max(r["refined"]["iters"]) for r in many), dprops), flush=True)
    for s, (a, b) in enumerate(zip(many, one)):
        assert [c[:2] for c in a["contribs"]] == [c[:2] for c in b["contribs"]], ("contributor tables differ", name, n_multi, s)
        assert list(a["refined"]["iters"]) == list(b["refined"]["iters"]), ("iteration counts differ", name, n_multi, s,
                                                                          a["refined"]["iters"], b["refined"]["iters"])
        assert numpy.array_equal(a["row_label"], b["row_label"]), ("row labels differ", name, n_multi, s,
                                                                   int((a["row_label"] != b["row_label"]).sum()))
    tb, ts = numpy.median(times["batch"]), numpy.median(times["single"])
    for route, label in (("batch", 'runs="batch" '), ("single", 'runs="single"')):
        t = times[route]
        print("    %s %9.2f ms (min %.2f, max %.2f of %d)   %7.1f us per sample"
              % (label, numpy.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, len(t), numpy.median(t) * 1e6 / len(counts)))
    print("    ratio batch / single  %.3f" % (tb / ts), flush=True)
    return tb, ts


runs = [int(v) for v in opts.runs.split(",")]
if opts.sweep:
    table = []
    for n_multi in runs:
        for rows in (int(v) for v in opts.sweep.split(",")):
            tb, ts = measure("%d" % rows, [rows] * 64, n_multi, distinct=8 if rows >= 30000 else None)
            table.append((n_multi, rows, ts, tb))
    print(' B | rows per sample | runs="single" ms | runs="batch" ms | ratio')
    for n_multi, rows, ts, tb in table:
        print("%2d | %15d | %16.2f | %15.2f | %.3f" % (n_multi, rows, ts * 1e3, tb * 1e3, tb / ts))
else:
    for name in opts.sets.split(","):
        for n_multi in runs:
            if name == "ragged":
                measure(name, [int(v) for v in numpy.random.default_rng(5).integers(50, 5001, size=64)], n_multi)
            else:
                measure(name, [opts.rows] * int(name), n_multi)
