#!/usr/bin/env python
"""
mixemt's `-t` output at --frags N synthetic fragments (synth_alignments, with strands), on the same columns as
tools/time_observe.py:
  - mxm_observe_bases_labelled (--labels K tables in one call) against mxm_observe_bases (one table), device time of the
    whole call (CUDA events, median of --reps);
  - the alignment labels of assign.assign_reads (alignment_labels: fragment -> row -> label, torch indexing) from a
    synthetic row grouping of the fragments (--rows-per-frag fragments per row on average) and a per-row result;
  - stats.write_statistics (the labelled call + the tables back + PREFIX.pos.tab + PREFIX.obs.tab) into a temp dir.
The labelled tables are checked against the unlabelled one (their sum, every alignment labelled).

    python tools/time_stats.py [--frags 1000000] [--labels 4] [--reps 5]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy
import torch

from mixemt_amd import _lib, assign, observe, phylotree, preprocess, stats, synth


def timed(fn, reps):
    fn()                                                  # warm-up (code object, scratch pool)
    times = []
    for _ in range(reps):
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        times.append(ev0.elapsed_time(ev1))
    return float(numpy.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--labels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows-per-frag", type=float, default=0.5)
    opts = ap.parse_args()
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    haps = sorted(phy.hap_var)
    tables = preprocess.HapVarTables.build(refseq, phy, haps)
    t0 = time.perf_counter()
    cols = synth.synth_alignments(tables, refseq, opts.frags, seed=1)
    sys.stderr.write("%d alignments of %d fragments, generated in %.1f s\n"
                     % (len(cols), cols.n_frag, time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    _lib.load()
    L = observe.pileup_length(cols, 30, len(refseq))
    dcols = observe.DeviceColumns(cols)
    K = opts.labels

    # labels: fragment f in row f // 2 (a row per two fragments, as de-duplication leaves them), rows round-robin over
    # K - 1 contributors and 'unassigned' (label K - 1); every 50th fragment in no row
    n_frag = cols.n_frag
    in_row = numpy.flatnonzero(numpy.arange(n_frag) % 50 != 49)
    per = max(1, int(round(1.0 / opts.rows_per_frag)))
    row_of = in_row // per
    n_rows = int(row_of.max()) + 1 if len(row_of) else 0
    order = numpy.argsort(row_of, kind="stable")
    ptr = numpy.zeros(n_rows + 1, dtype=numpy.int64)
    numpy.cumsum(numpy.bincount(row_of, minlength=n_rows), out=ptr[1:])
    group_frag = in_row[order].astype(numpy.int64)
    assigned = (numpy.arange(n_rows) % K).astype(numpy.int32)            # (K - 1 = 'unassigned' of assign_reads)
    frag_d = torch.from_numpy(cols.frag).cuda()
    ptr_d, gf_d, rl_d = torch.from_numpy(ptr).cuda(), torch.from_numpy(group_frag).cuda(), torch.from_numpy(assigned).cuda()
    labels = assign.alignment_labels(frag_d, ptr_d, gf_d, rl_d, n_frag)
    t_lab, lab_times = timed(lambda: assign.alignment_labels(frag_d, ptr_d, gf_d, rl_d, n_frag), opts.reps)

    one = torch.zeros((L, 16), dtype=torch.int32, device="cuda")
    many = torch.zeros((K, L, 16), dtype=torch.int32, device="cuda")
    t_one, one_times = timed(lambda: (one.zero_(), observe.count_bases(dcols, one)), opts.reps)
    t_many, many_times = timed(lambda: (many.zero_(), observe.count_bases_labelled(dcols, labels, many)), opts.reps)
    everyone = torch.zeros_like(labels)
    sums = torch.zeros((K, L, 16), dtype=torch.int32, device="cuda")
    observe.count_bases_labelled(dcols, (everyone + torch.arange(len(cols), device="cuda", dtype=torch.int32) % K)
                                 .contiguous(), sums)
    same = bool(torch.equal(sums.sum(dim=0), one))

    print("columns: %d alignments of %d fragments, L = %d; %d labels, %d rows, %d alignments in no row"
          % (len(cols), n_frag, L, K, n_rows, int((labels < 0).sum())))
    print("mxm_observe_bases (1 table, device, median of %d): %.3f ms  [%s]"
          % (opts.reps, t_one, " ".join("%.3f" % t for t in one_times)))
    print("mxm_observe_bases_labelled (%d tables, device, median of %d): %.3f ms  [%s]  = %.2fx"
          % (K, opts.reps, t_many, " ".join("%.3f" % t for t in many_times), t_many / t_one))
    print("alignment labels (alignment_labels, torch indexing, median of %d): %.3f ms  [%s]"
          % (opts.reps, t_lab, " ".join("%.3f" % t for t in lab_times)))
    print("labelled tables summed == unlabelled table: %s" % same)

    # the whole -t output: ContribReads over these labels -> write_statistics (labelled call, tables back, both files)
    contribs = [["hap%d" % (k + 1), haps[k * 997], 1.0 / (K - 1)] for k in range(K - 1)]
    names = [c[0] for c in contribs] + ["unassigned"]
    all_obs = observe.ObservedBases(one.cpu().numpy().view(numpy.uint32))
    args = argparse.Namespace(min_mq=30, min_bq=30, min_var_reads=3, frac_var_reads=0.02)
    walls = []
    with tempfile.TemporaryDirectory() as tmp:
        args.stats_prefix = os.path.join(tmp, "run")
        for _ in range(opts.reps):
            cr = assign.ContribReads(cols, labels, names, names, dcols)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stats.write_statistics(phy, all_obs, contribs, cr, args)
            walls.append((time.perf_counter() - t0) * 1e3)
        sizes = [os.path.getsize(args.stats_prefix + ext) for ext in (".pos.tab", ".obs.tab")]
        t0 = time.perf_counter()
        with open(os.devnull, "w") as out:
            stats.write_variants(out, phy, contribs, all_obs, args)
        t_var = (time.perf_counter() - t0) * 1e3
    print("write_statistics (labelled call + %d tables back + pos.tab %.1f MB + obs.tab %.1f MB), median of %d: "
          "%.1f ms  [%s]; of which write_variants alone %.1f ms"
          % (K, sizes[0] / 1e6, sizes[1] / 1e6, opts.reps, float(numpy.median(walls)),
             " ".join("%.1f" % t for t in walls), t_var))
    print("upload of the columns (host -> device, apart): %.1f ms" % (dcols.upload_s * 1e3))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
