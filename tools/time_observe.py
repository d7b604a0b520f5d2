#!/usr/bin/env python
"""
The pileup of the variant check (observe.observe_bases -> mxm_observe_bases) at --frags N synthetic fragments
(synth_alignments, with strands): the library call's device time (the median of --reps calls, CUDA events around it),
the host -> device upload of the columns (apart), and the numpy restatement's time (tests/_pileup_ref.py) as the
single-core yardstick.  The tables are compared.

    python tools/time_observe.py [--frags 1000000] [--reps 5] [--no-numpy]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy
import torch

from mixemt_amd import _lib, observe, phylotree, preprocess, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    opts = ap.parse_args()
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    tables = preprocess.HapVarTables.build(refseq, phy, sorted(phy.hap_var))
    t0 = time.perf_counter()
    cols = synth.synth_alignments(tables, refseq, opts.frags, seed=1)
    sys.stderr.write("%d alignments of %d fragments, %.1f MB of bases (+ qualities), generated in %.1f s\n"
                     % (len(cols), cols.n_frag, len(cols.seq) / 1e6, time.perf_counter() - t0))
    torch.zeros(1, device="cuda")
    _lib.load()
    L = observe.pileup_length(cols, 30, len(refseq))
    dcols = observe.DeviceColumns(cols)
    dcols = observe.DeviceColumns(cols)                 # (the second upload: allocator warm)
    counts = torch.zeros((L, 16), dtype=torch.int32, device="cuda")
    observe.count_bases(dcols, counts)                  # warm-up (code object, scratch pool)
    times = []
    for _ in range(opts.reps):
        counts.zero_()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        observe.count_bases(dcols, counts)
        ev1.record()
        torch.cuda.synchronize()
        times.append(ev0.elapsed_time(ev1))
    got = counts.cpu().numpy().astype(numpy.int64)
    print("pileup: %d observations, L = %d" % (int(got.sum()), L))
    print("mxm_observe_bases (device, median of %d): %.3f ms  [%s]" % (opts.reps, float(numpy.median(times)),
                                                                       " ".join("%.3f" % t for t in times)))
    print("upload of the columns (host -> device): %.1f ms for %.1f MB"
          % (dcols.upload_s * 1e3, sum(t.numel() * t.element_size() for t in (
              dcols.ref_start, dcols.mapq, dcols.cig_ptr, dcols.cigar, dcols.seq_ptr, dcols.seq, dcols.qual,
              dcols.has_qual, dcols.is_reverse) if t is not None) / 1e6))
    if not opts.no_numpy:
        import _pileup_ref
        t0 = time.perf_counter()
        want = _pileup_ref.pileup(cols, L)
        print("numpy restatement: %.1f ms" % ((time.perf_counter() - t0) * 1e3))
        print("tables equal: %s" % numpy.array_equal(got, want))
        if not numpy.array_equal(got, want):
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
