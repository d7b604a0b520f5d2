#!/usr/bin/env python
"""
assign.support_many -- all nested-model fits of all samples in two batched device passes -- against the loop a caller
would write without it: per (sample, model) one em.SampleFinish.gather at the model's columns, one em.SampleFinish.em_loop
(mxm_em_loop_samples_narrow, one workgroup) from the same uniform start, and a torch.logsumexp log-likelihood.  The same
records, the same assign.finish_many results, in one process, alternated.

    python tools/time_support.py [--sets 1,64,256,ragged,big] [--configs drop,add,all] [--repeats 3] [--rows 600]

Samples as tools/time_bootstrap.py makes them: synth.synth_reads(tables, ref_len, rows, seed=SEED0 + s), unit weights;
"ragged": 64 samples of 55 .. 4996 rows (numpy.random.default_rng(5).integers); "big": one sample of 10^5 rows.  The
contributors are FIXED (args.contributors) to the haplogroups the reads were drawn from, so that every sample has the
configuration's K: "drop" = K = 3, models="drop-one" (4 fits); "add" = K = 3, models="add-one", n_extra=4 (8 fits); "all" = K = 8,
models="all" (255 fits).  The first round warms both routes up and is not counted; every timing has a synchronise at each end;
the median of the repeats is reported with its range.  The tool asserts identical props bits and equal iteration counts, and
the two log-likelihoods within 2 (R + K + 8) u of one another, before it reports any time.
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
CONTRIB3, PROPS3 = synth.DEFAULT_CONTRIB, synth.DEFAULT_PROPS
CONTRIB8, PROPS8 = (10, 700, 1400, 2000, 2700, 3400, 4000, 4700), (0.3, 0.2, 0.15, 0.1, 0.1, 0.05, 0.05, 0.05)
CONFIGS = {"drop": (CONTRIB3, PROPS3, dict(models="drop-one")), "add": (CONTRIB3, PROPS3, dict(models="add-one", n_extra=4)),
           "all": (CONTRIB8, PROPS8, dict(models="all"))}

ap = argparse.ArgumentParser()
ap.add_argument("--sets", default="1,64,256,ragged,big")
ap.add_argument("--configs", default="drop,add,all")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--rows", type=int, default=600)
opts = ap.parse_args()
refseq = phylotree.load_rsrs(); phy = phylotree.load_build17(refseq); haps = sorted(phy.hap_var)
tables = preprocess.HapVarTables.build(refseq, phy, haps)
hap_index = {}
for i, hap in enumerate(haps):
    hap_index.setdefault(hap, i)
print("device: %s; %d haplogroups" % (torch.cuda.get_device_name(0), len(haps)))


def prepare(counts, contrib, props):
    """The cohort, finished with its contributors fixed, and one em.SampleFinish per sample for the loop route."""
    args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False, min_reads=10,
                              contributors=",".join(haps[c] for c in contrib), var_check=False, refine_ests=True, min_fold=2.0)
    n = len(counts)
    csr = [synth.synth_reads(tables, len(refseq), rows, seed=SEED0 + s, contrib=contrib, props=props)[:3] for s, rows in enumerate(counts)]
    cm, row0 = preprocess.build_em_records_many(tables, csr)
    samples = [(cm.rows(row0[s], row0[s + 1]), numpy.ones(int(row0[s + 1] - row0[s]))) for s in range(n)]
    numpy.random.seed(7)
    results = em.run_em_many(samples, args)
    finished = assign.finish_many(samples, results, haps, args, max_rows=10 ** 9)
    assert all(f["refined"] is not None and len(f["contribs"]) == len(contrib) for f in finished), "a sample would be skipped"
    wts_d = {s: torch.ones(samples[s][0].n_rows, dtype=torch.float64, device="cuda") for s in range(n)}
    singles = [assign._finish_batch(samples, wts_d, [s]) for s in range(n)]
    return args, samples, finished, singles


def loop_route(args, finished, singles, support):
    """Per (sample, model): gather at the model's columns, em_loop from the uniform start, logsumexp.  -> [[(props, ll, iters)]]"""
    out = []
    for s, fin in enumerate(singles):
        fits = []
        for model in support[s]["models"]:
            names = model["names"]
            k = len(names)
            ld = 4 if k <= 4 else (8 if k <= 8 else 16)
            cols = numpy.zeros((1, ld), dtype=numpy.int32)
            cols[0, :k] = [hap_index[h] for h in names]
            mat = fin.gather(cols, [k], ld)
            _, ln_new, states = fin.em_loop(mat, ld, [k], [numpy.full(k, 1.0 / k)], args.tolerance, args.max_iter)
            lnp = torch.from_numpy(ln_new[0, :k]).cuda()
            ll = float((fin.wts * torch.logsumexp(mat[:, :k] + lnp[None, :], dim=1)).sum())
            fits.append((numpy.exp(ln_new[0, :k]), ll, states[0][1]))
        out.append(fits)
    return out


def measure(name, config, counts, made):
    args, samples, finished, singles = made
    kw = CONFIGS[config][2]
    times = {"batch": [], "loop": []}
    for rep in range(opts.repeats + 1):                       # (the first round warms both routes up and is not counted)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        support, skipped = assign.support_many(samples, finished, haps, args, max_rows=10 ** 9, max_bytes=64 << 30, **kw)
        torch.cuda.synchronize(); dt = time.perf_counter() - t0
        assert not skipped
        torch.cuda.synchronize(); t0 = time.perf_counter()
        loop = loop_route(args, finished, singles, support)
        torch.cuda.synchronize(); dl = time.perf_counter() - t0
        if rep:
            times["batch"].append(dt); times["loop"].append(dl)
    n_fits, iters = len(support[0]["models"]), []
    for s in range(len(counts)):
        for model, (props, ll, n_iter) in zip(support[s]["models"], loop[s]):
            assert numpy.array_equal(model["props"].view(numpy.int64), props.view(numpy.int64)), ("props differ", name, config, s, model["names"])
            assert model["iters"] == n_iter, (name, config, s, model["names"], model["iters"], n_iter)
            assert abs(model["loglik"] - ll) <= 2 * (counts[s] + len(props) + 8) * 2.0 ** -53 * abs(ll), (name, config, s, model["loglik"], ll)
            iters.append(n_iter)
    tb, tl = numpy.median(times["batch"]), numpy.median(times["loop"])
    print("set %-6s %-4s S = %3d, %3d fits each, rows %d .. %d (%d in all), iterations %d .. %d; props identical, ll equal"
          % (name, config, len(counts), n_fits, min(counts), max(counts), sum(counts), min(iters), max(iters)), flush=True)
    for key, label in (("batch", "support_many        "), ("loop", "loop of (sample, fit)")):
        t = times[key]
        print("    %s %10.2f ms (min %.2f, max %.2f of %d)" % (label, numpy.median(t) * 1e3, min(t) * 1e3, max(t) * 1e3, len(t)))
    print("    ratio batch / loop %.3f" % (tb / tl), flush=True)
    return n_fits, tb, tl


table = []
for config in opts.configs.split(","):
    for name in opts.sets.split(","):
        if name == "ragged":
            counts = [int(v) for v in numpy.random.default_rng(5).integers(50, 5001, size=64)]
        elif name == "big":
            counts = [100000]
        else:
            counts = [opts.rows] * int(name)
        made = prepare(counts, CONFIGS[config][0], CONFIGS[config][1])
        table.append((name, config) + measure(name, config, counts, made))
        del made
print("set    | config | fits | loop ms | support_many ms | ratio")
for name, config, n_fits, tb, tl in table:
    print("%-6s | %-6s | %4d | %10.2f | %15.2f | %.3f" % (name, config, n_fits, tl * 1e3, tb * 1e3, tb / tl))
