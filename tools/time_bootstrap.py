#!/usr/bin/env python
"""
assign.bootstrap_many -- all replicates of all samples in batched device passes -- against a loop over the replicates: B calls
of em.SampleFinish.em_loop (mxm_em_loop_samples_narrow, one workgroup per sample), each under weights resampled ON THE HOST
by the draw rule of include/mixemt_hip_bootstrap.h, then one mxm_bootstrap_summary over the loop's log proportions.  The same
records, the same assign.finish_many results, the same seed, in one process, alternated.

    python tools/time_bootstrap.py [--sets 1,64,ragged,big] [--boots 200,1000] [--repeats 3] [--rows 600]

Samples as tools/time_many_samples_runs.py makes them: synth.synth_reads(tables, ref_len, rows, seed=SEED0 + s), unit
weights (N_s = the sample's rows); "ragged": 64 samples of 50 .. 5000 rows (numpy.random.default_rng(5).integers); "big": one
sample of 10^5 rows.  The first round warms both routes up and is not counted; every timing has a synchronise at each end;
the median of the repeats is reported.  The loop's host resampling is timed inside the loop route, as a caller without the
batched entry would pay it, and also reported on its own.  The tool asserts that both routes give identical props_boot.
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
SEED = 7

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="1,64,ragged,big")
ap.add_argument("--boots", default="200,1000")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rows", type=int, default=600)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
print("device: %s; %d haplogroups" % (torch.cuda.get_device_name(0), len(haps)))


def host_resample(cum, total, n_rows, s_id, b):
    """Replicate b of one sample on the host: draw j = word j mod 4 of Philox4x64-10, key (SEED, 0), counter (j / 4 + 1, b,
    s_id, 0) -- numpy's generator from counter (0, b, s_id, 0) --, t = (u * N) >> 64, row = the number of prefix sums <= t."""
    gen = numpy.random.Philox(counter=numpy.array([0, b, s_id, 0], dtype=numpy.uint64), key=numpy.array([SEED, 0], dtype=numpy.uint64))
    u = gen.random_raw(total)
    n = numpy.uint64(total)
    at = ((u >> numpy.uint64(32)) * n + (((u & numpy.uint64(0xFFFFFFFF)) * n) >> numpy.uint64(32))) >> numpy.uint64(32)
    return numpy.bincount(numpy.searchsorted(cum, at.astype(numpy.int64), side="right"), minlength=n_rows).astype(numpy.float64)


def prepare(counts):
    """The cohort and the loop route's fixtures, as bootstrap_many makes its own: the reduced matrices and the starts."""
    args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False, min_reads=10,
                              contributors=None, var_check=False, refine_ests=True, min_fold=2.0)
    n = len(counts)
    csr = [synth.synth_reads(tables, len(refseq), rows, seed=SEED0 + s)[:3] for s, rows in enumerate(counts)]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    samples = [(cm.rows(row0[s], row0[s + 1]), numpy.ones(int(row0[s + 1] - row0[s]))) for s in range(n)]
    numpy.random.seed(7)
    results = em.run_em_many(samples, args)
    finished = assign.finish_many(samples, results, haps, args, max_rows=10 ** 9)
    assert all(f["refined"] is not None and 1 <= len(f["contribs"]) <= 16 for f in finished), "a sample would be skipped"
    hap_index = {}
    for i, hap in enumerate(haps):
        hap_index.setdefault(hap, i)
    plans = [assign._finish_columns(f["contribs"], hap_index) for f in finished]
    ld, cols, ncol, _ = assign._finish_tables(plans)
    wts_d = [torch.ones(s[0].n_rows, dtype=torch.float64, device="cuda") for s in samples]
    fin = assign._finish_batch(samples, wts_d, list(range(n)))
    mat = fin.gather(cols, ncol, ld)
    starts = [numpy.asarray(f["refined"]["props"], dtype=numpy.float64) for f in finished]
    cums = [numpy.cumsum(numpy.ones(c, dtype=numpy.int64)) for c in counts]
    return args, samples, finished, fin, mat, ld, ncol, starts, cums


def measure(name, counts, n_boot, made):
    args, samples, finished, fin, mat, ld, ncol, starts, cums = made
    n = len(counts)
    done = numpy.zeros((n * n_boot, 6), dtype=numpy.int32)
    done[:, 0] = 1
    state = torch.from_numpy(done.reshape(-1).view(numpy.int64).copy()).cuda()
    level = 0.95
    times = {"batch": [], "loop": [], "resample": []}
    out = {}
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        boots, skipped = assign.bootstrap_many(samples, finished, haps, args, n_boot=n_boot, seed=SEED, level=level,
                                               max_rows=10 ** 9, max_bytes=64 << 30)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        assert not skipped
        out["batch"] = boots
        torch.cuda.synchronize(); t0 = time.perf_counter()
        host = 0.0
        ln_all = numpy.empty((n, n_boot, ld))
        iters = numpy.empty((n, n_boot), dtype=numpy.int64)
        for b in range(n_boot):
            h0 = time.perf_counter()
            w_b = numpy.concatenate([host_resample(cums[s], counts[s], counts[s], s, b) for s in range(n)])
            host += time.perf_counter() - h0
            fin.wts.copy_(torch.from_numpy(w_b))
            _, ln_new, states = fin.em_loop(mat, ld, ncol, starts, args.tolerance, args.max_iter)
            ln_all[:, b] = ln_new
            iters[:, b] = [st[1] for st in states]
        x, lo, hi, _, _, _ = fin.boot_summary(n_boot, ld, ncol, torch.from_numpy(ln_all.reshape(n * n_boot, ld)).cuda(), state,
                                              (1.0 - level) / 2.0, (1.0 + level) / 2.0)
        torch.cuda.synchronize(); dl = time.perf_counter() - t0
        out["loop"] = (x, lo, hi, iters)
        if rep:
            times["batch"].append(dt); times["loop"].append(dl); times["resample"].append(host)
    x, lo, hi, iters = out["loop"]
    for s, boot in enumerate(out["batch"]):
        k = int(ncol[s])
        assert numpy.array_equal(boot["props_boot"].view(numpy.int64), numpy.ascontiguousarray(x[s, :, :k]).view(numpy.int64)), \
            ("props_boot differs between the routes", name, n_boot, s)
        assert numpy.array_equal(boot["iters"], iters[s]) and numpy.array_equal(boot["lo"], lo[s, :k]) and numpy.array_equal(boot["hi"], hi[s, :k])
    tb, tl, th = (numpy.median(times[k]) for k in ("batch", "loop", "resample"))
    widths = [float((b["hi"] - b["lo"]).max()) for b in out["batch"]]
    print("set %-6s S = %3d, B = %4d, rows %d .. %d (%d in all), contributors %d .. %d, iterations %d .. %d, widest 95 %% "
          "interval %.4f .. %.4f; props_boot identical"
          % (name, n, n_boot, min(counts), max(counts), sum(counts), int(ncol.min()), int(ncol.max()), int(iters.min()),
             int(iters.max()), min(widths), max(widths)), flush=True)
    for key, label in (("batch", "bootstrap_many   "), ("loop", "loop of em_loop  "), ("resample", "  of it: host resampling")):
        t = times[key]
        print("    %s %10.2f ms (min %.2f, max %.2f of %d)" % (label, numpy.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, len(t)))
    print("    ratio batch / loop %.3f   (against the loop without its host resampling: %.3f)" % (tb / tl, tb / (tl - th)), flush=True)
    return tb, tl, th


table = []
for name in opts.sets.split(","):
    if name == "ragged":
        counts = [int(v) for v in numpy.random.default_rng(5).integers(50, 5001, size=64)]
    elif name == "big":
        counts = [100000]
    else:
        counts = [opts.rows] * int(name)
    made = prepare(counts)
    for n_boot in (int(v) for v in opts.boots.split(",")):
        table.append((name, n_boot) + measure(name, counts, n_boot, made))
print("set    |    B | loop ms (host resampling) | bootstrap_many ms | ratio")
for name, n_boot, tb, tl, th in table:
    print("%-6s | %4d | %10.2f (%10.2f)   | %17.2f | %.3f" % (name, n_boot, tl * 1e3, th * 1e3, tb * 1e3, tb / tl))
