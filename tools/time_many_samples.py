#!/usr/bin/env python
"""
em.run_em_many (ONE batched device loop over the samples' concatenated records: mxm_em_loop_samples) against a Python loop
of em.run_em_ex(records=...) over the same samples (the records route of storage="coded": mxm_em_loop_coded per sample),
in one process, interleaved, default tolerance / max_iter, the same initial proportions.

    python tools/time_many_samples.py [--sets 64,256,ragged] [--repeats 3] [--rows 600]

Samples: synth.synth_reads(tables, ref_len, rows, seed=SEED0 + s), unit weights; "ragged": 64 samples of 50 .. 5000 rows
(numpy.random.default_rng(5).integers).  Initial proportions: numpy.random.seed(7), then em.draw_inits_many.
Wall times include everything a caller pays after the records exist: plan / workspace, the loop, the read-back.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch
from mixemt_amd import em, phylotree, preprocess, synth

SEED0 = 1000

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="64,256,ragged")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rows", type=int, default=600)
ap.add_argument("--max-iter", type=int, default=10000)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=opts.max_iter, n_multi=1, verbose=False)
print("device: %s; %d haplogroups; tolerance %g, max_iter %d" % (torch.cuda.get_device_name(0), len(haps), args.tolerance, args.max_iter))

for name in opts.sets.split(","):
    if name == "ragged":
        counts = [int(v) for v in numpy.random.default_rng(5).integers(50, 5001, size=64)]
    else:
        counts = [opts.rows] * int(name)
    csr = [synth.synth_reads(tables, len(refseq), n, seed=SEED0 + s)[:3] for s, n in enumerate(counts)]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    views = [cm.rows(row0[s], row0[s + 1]) for s in range(len(counts))]
    wts = [numpy.ones(n) for n in counts]
    numpy.random.seed(7)
    inits = em.draw_inits_many(len(counts), len(haps))
    samples = list(zip(views, wts))
    t_batch, t_seq, t_seq_loop = [], [], []
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        many = em.run_em_many(samples, args, inits=inits)
        torch.cuda.synchronize(); dt_b = time.perf_counter() - t0
        torch.cuda.synchronize(); t0 = time.perf_counter()
        one = [em.run_em_ex(None, w, args, inits=i, want_read_mix=False, records=v) for v, w, i in zip(views, wts, inits)]
        torch.cuda.synchronize(); dt_s = time.perf_counter() - t0
        if rep:
            t_batch.append(dt_b); t_seq.append(dt_s); t_seq_loop.append(sum(r["loop_s"] for r in one))
    it_b = [r["iters"][0] for r in many]
    it_s = [r["iters"][0] for r in one]
    dprops = max(float(numpy.abs(a["props"] - b["props"]).max()) for a, b in zip(many, one))
    tb, ts, tl = numpy.median(t_batch), numpy.median(t_seq), numpy.median(t_seq_loop)
    print("set %-6s S = %3d, rows %d .. %d (%d in all, %d tiles): iterations batch / sequential equal for %d of %d samples, "
          "max |props batch - sequential| %.2e" % (name, len(counts), min(counts), max(counts), sum(counts),
                                                   sum(-(-n // 32) for n in counts), sum(a == b for a, b in zip(it_b, it_s)),
                                                   len(counts), dprops))
    print("    batch       %9.2f ms (min %.2f, max %.2f of %d)   longest sample %d iterations = passes   %7.1f us per pass"
          % (tb * 1e3, min(t_batch) * 1e3, max(t_batch) * 1e3, len(t_batch), max(it_b), tb * 1e6 / max(it_b)))
    print("    sequential  %9.2f ms (min %.2f, max %.2f; loops alone %.2f ms)   %d sample-iterations   %7.1f us per sample-iteration"
          % (ts * 1e3, min(t_seq) * 1e3, max(t_seq) * 1e3, tl * 1e3, sum(it_s), ts * 1e6 / sum(it_s)))
    print("    ratio batch / sequential  %.3f   (against the loops alone %.3f)" % (tb / ts, tb / tl))
