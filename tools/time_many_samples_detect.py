#!/usr/bin/env python
"""
assign.detect_many -- the detection bootstrap of a cohort in batched device passes -- against the loop a caller writes
today, per (sample, replicate): em.run_em_ex(records=cm, weights=wb_sb, inits=start, want_read_mix=False), then
assign.get_contributors_records with a per-sample observe.ObservedBases of the same pileup.  Both functions are the
package's own, unchanged; the loop is handed its resampled weights for nothing (they are drawn once by
mxm_bootstrap_weights and sliced on the device), as tools/time_bootstrap.py does.

    python tools/time_many_samples_detect.py [--sets 1,64,ragged,big] [--boot 200] [--loop-reps 8] [--repeats 2] [--rows 600]

Samples as tools/time_bootstrap.py makes them: synth.synth_reads(tables, ref_len, rows, seed=SEED0 + s), unit weights;
"ragged": 64 samples of 55 .. 4996 rows (numpy.random.default_rng(5).integers); "big": one sample of 10^5 rows at B = 64.
Pileups: synth.synth_alignments of min(rows, 3000) fragments per sample, one observe.observe_bases_many call.  The variant
check is ON (the reference's default) and args.min_reads = 10.
The loop runs the first --loop-reps replicates of every sample and its time is SCALED by B / loop-reps; the report says so.
The first round warms both routes up and is not counted; every timing has a synchronise at each end; the median of the repeats
is reported with its range.  A second, separate pass of detect_many with a synchronise around each stage gives the stages'
shares (EM loop, vote, the two new kernels); its total is not the time reported.  The tool counts the replicates, among those
both routes ran, whose kept sets differ and asserts that there are none after it has printed the times.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy
import torch
from mixemt_amd import _lib, assign, em, observe, phylotree, preprocess, synth

SEED0, SEED = 1000, 7

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="1,64,ragged,big")
ap.add_argument("--boot", type=int, default=200)
ap.add_argument("--loop-reps", type=int, default=8)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--rows", type=int, default=600)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
print("device: %s; %d haplogroups" % (torch.cuda.get_device_name(0), len(haps)))
args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False, min_reads=10, contributors=None,
                          var_check=True, min_var_reads=3, frac_var_reads=0.02, var_count=None, var_fraction=0.5, refine_ests=True,
                          min_fold=2.0)


def prepare(counts):
    n = len(counts)
    csr = [synth.synth_reads(tables, len(refseq), rows, seed=SEED0 + s)[:3] for s, rows in enumerate(counts)]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    samples = [(cm.rows(row0[s], row0[s + 1]), numpy.ones(int(row0[s + 1] - row0[s]))) for s in range(n)]
    parts = [synth.synth_alignments(tables, refseq, min(rows, 3000), seed=SEED0 + 500 + s) for s, rows in enumerate(counts)]
    pileup = observe.observe_bases_many(parts, 30, 30, ref_len=len(refseq))
    var_tables = assign.VarCheckTables.build(phy, haps, pileup.counts.device)
    numpy.random.seed(7)
    results = em.run_em_many(samples, args)
    assert all(r["route"] == "batch" for r in results)
    finished = assign.finish_many(samples, results, haps, args, phylo=phy, obs=pileup, var_tables=var_tables, max_rows=10 ** 9)
    return samples, results, finished, pileup, var_tables


def loop_route(samples, results, pileup, wb, n_boot, reps):
    """Per (sample, replicate b < reps): run_em_ex under the replicate's weights from the warm start, get_contributors_records.
    -> [[(kept haplogroups, iterations)]]"""
    row0 = numpy.concatenate([[0], numpy.cumsum([m.n_rows for m, _ in samples])])
    out = []
    for s, (cm, _) in enumerate(samples):
        start = numpy.asarray(results[s]["props"], dtype=numpy.float64)
        start = (start / start.sum()).reshape(1, -1)
        obs = pileup.host(s)
        got = []
        for b in range(reps):
            lo = n_boot * int(row0[s]) + b * cm.n_rows
            w_sb = wb[lo:lo + cm.n_rows]
            res = em.run_em_ex(None, w_sb, args, inits=start, want_read_mix=False, records=cm)
            contribs = assign.get_contributors_records(phy, obs, haps, w_sb, res["props"], cm, res["ln_theta_k"], args)
            got.append(([c[1] for c in contribs], res["iters"][0]))
        out.append(got)
    return out


def staged(fn, bucket, key):
    def timed(*a, **kw):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        out = fn(*a, **kw)
        torch.cuda.synchronize(); bucket[key] = bucket.get(key, 0.0) + time.perf_counter() - t0
        return out
    return timed


def shares(call):
    """One detect_many call with a synchronise around the EM loop, the vote and the two new entries -> {stage: seconds}."""
    lib, bucket = _lib.load(), {}
    keep = (em.SampleBatch.em_loop_device, em.SampleFinish.votes_device, lib.mxm_detect_candidates, lib.mxm_check_variants_entries,
            em.SampleFinish.boot_weights)
    em.SampleBatch.em_loop_device = staged(keep[0], bucket, "loop")
    em.SampleFinish.votes_device = staged(keep[1], bucket, "vote")
    lib.mxm_detect_candidates = staged(keep[2], bucket, "candidates")
    lib.mxm_check_variants_entries = staged(keep[3], bucket, "check")
    em.SampleFinish.boot_weights = staged(keep[4], bucket, "weights")
    try:
        torch.cuda.synchronize(); t0 = time.perf_counter()
        call()
        torch.cuda.synchronize(); bucket["total"] = time.perf_counter() - t0
    finally:
        em.SampleBatch.em_loop_device, em.SampleFinish.votes_device = keep[0], keep[1]
        lib.mxm_detect_candidates, lib.mxm_check_variants_entries, em.SampleFinish.boot_weights = keep[2], keep[3], keep[4]
    return bucket


def measure(name, counts, n_boot):
    samples, results, finished, pileup, var_tables = prepare(counts)
    reps = min(opts.loop_reps, n_boot)
    wts_d = {s: torch.ones(samples[s][0].n_rows, dtype=torch.float64, device="cuda") for s in range(len(samples))}
    wb, errors = assign._finish_batch(samples, wts_d, list(range(len(samples)))).boot_weights(n_boot, SEED, list(range(len(samples))))
    assert not any(errors)

    def call():
        return assign.detect_many(samples, results, finished, haps, args, n_boot=n_boot, seed=SEED, obs=pileup, phylo=phy,
                                  var_tables=var_tables, max_bytes=16 << 30)
    times = {"batch": [], "loop": []}
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        found, skipped = call()
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        assert not skipped
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loop = loop_route(samples, results, pileup, wb, n_boot, reps)
        torch.cuda.synchronize(); dl = time.perf_counter() - t0
        if rep:
            times["batch"].append(dt); times["loop"].append(dl * n_boot / reps)
    share = shares(call)
    differ, iters_b, iters_l, unused = 0, [], [], 0
    for s in range(len(samples)):
        res = found[s]
        iters_b.extend(res["iters"].tolist())
        unused += n_boot - res["n_used"]
        for b in range(reps):
            kept = [haps[res["cand"][b, i]] for i in range(max(int(res["ncand"][b]), 0)) if res["keep"][b, i]]
            differ += kept != loop[s][b][0]
            iters_l.append(loop[s][b][1])
    tb, tl = numpy.median(times["batch"]), numpy.median(times["loop"])
    first_iters = [r["iters"][0] for r in results]
    print("set %-6s S = %3d, B = %d, rows %d .. %d (%d in all); first EM (random start) %d .. %d iterations; warm-started replicates "
          "%d .. %d (median %d; the loop's, on its %d replicates per sample: %d .. %d); %d replicates not usable"
          % (name, len(counts), n_boot, min(counts), max(counts), sum(counts), min(first_iters), max(first_iters), min(iters_b),
             max(iters_b), int(numpy.median(iters_b)), reps, min(iters_l), max(iters_l), unused), flush=True)
    print("    detect_many                 %10.2f ms (min %.2f, max %.2f of %d)"
          % (tb * 1e3, min(times["batch"]) * 1e3, max(times["batch"]) * 1e3, len(times["batch"])))
    print("    loop, %d of %d replicates, SCALED by %g: %10.2f ms (min %.2f, max %.2f of %d)"
          % (reps, n_boot, n_boot / float(reps), tl * 1e3, min(times["loop"]) * 1e3, max(times["loop"]) * 1e3, len(times["loop"])))
    print("    ratio batch / loop %.3f; kept sets that differ on the %d replicates both ran: %d" % (tb / tl, reps * len(counts), differ))
    total = share["total"]
    print("    shares of a synchronised pass (%.2f ms): weights %.1f%%, EM loop %.1f%%, vote %.1f%%, candidates %.2f%%, check %.2f%%, "
          "host and the rest %.1f%%"
          % (total * 1e3, 100 * share.get("weights", 0) / total, 100 * share["loop"] / total, 100 * share["vote"] / total,
             100 * share["candidates"] / total, 100 * share.get("check", 0) / total,
             100 * (total - sum(v for k, v in share.items() if k != "total")) / total), flush=True)
    return len(counts), n_boot, tb, tl, differ


table = []
for name in opts.sets.split(","):
    n_boot = opts.boot
    if name == "ragged":
        counts = [int(v) for v in numpy.random.default_rng(5).integers(50, 5001, size=64)]
    elif name == "big":
        counts, n_boot = [100000], min(64, opts.boot)
    else:
        counts = [opts.rows] * int(name)
    table.append((name,) + measure(name, counts, n_boot))
print("set    |   S |   B | loop ms (scaled) | detect_many ms | ratio")
for name, n, n_boot, tb, tl, _ in table:
    print("%-6s | %3d | %3d | %16.2f | %14.2f | %.3f" % (name, n, n_boot, tl * 1e3, tb * 1e3, tb / tl))
assert sum(row[5] for row in table) == 0, "kept sets differ between detect_many and the loop"
print("identical kept sets on every replicate both routes ran")
