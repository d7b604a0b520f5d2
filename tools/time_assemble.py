#!/usr/bin/env python
"""
mixemt's `-x` (assembly extension) and `-b` (consensus FASTA) at --frags N synthetic fragments (synth_alignments with
planted private variants, tools/gen_golden.py's g18_private), on labels made as tests/test_gpu_assemble.py's million test
makes them: one fragment in --assigned-every goes to the contributor that shed it, the rest is unassigned.

  - one mxm_observe_bases_labelled call over the same columns (the yardstick: one alignment walk);
  - ONE extension round split into its parts: pileup / consensus / new variants / assign + move (device events around
    each, median of --reps, the labels restored before every repeat);
  - the whole extend_assemblies (rounds stated) and a round after the first (which counts only what moved);
  - write_consensus_seqs (host clock: pileup + consensus + tie rule + strings back + the file);
  - the numpy restatement (tests/_assemble_ref.py) of one round on the same host, with --numpy.

    python tools/time_assemble.py [--frags 1000000] [--reps 5] [--assigned-every 200] [--numpy]
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy
import torch

from mixemt_amd import _lib, assemble, assign, observe, phylotree, preprocess, synth


def timed(fn, reps, before=None):
    if before:
        before()
    fn()                                                  # warm-up
    times = []
    for _ in range(reps):
        if before:
            before()
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        fn()
        ev1.record()
        torch.cuda.synchronize()
        times.append(ev0.elapsed_time(ev1))
    return float(numpy.median(times)), " ".join("%.3f" % t for t in times)


def main():
    import gen_golden
    ap = argparse.ArgumentParser()
    ap.add_argument("--frags", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--assigned-every", type=int, default=200)
    ap.add_argument("--numpy", action="store_true", help="also time the numpy restatement of one round (minutes at 10^6)")
    opts = ap.parse_args()
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    haps = sorted(phy.hap_var)
    tables = preprocess.HapVarTables.build(refseq, phy, haps)
    cols = synth.synth_alignments(tables, refseq, opts.frags, seed=1, private=gen_golden.g18_private(refseq, tables))
    who = numpy.random.default_rng([1, 0xA11]).choice(len(synth.DEFAULT_PROPS), size=opts.frags,
                                                      p=numpy.asarray(synth.DEFAULT_PROPS, dtype=float))
    who_of = who[numpy.array([int(name[1:]) for name in cols.names])]
    f = cols.frag
    n_con = len(synth.DEFAULT_PROPS)
    label = numpy.where(f % 50 == 49, -1, numpy.where(f % opts.assigned_every == 0, who_of[f], n_con)).astype(numpy.int32)
    names = ["hap%d" % (k + 1) for k in range(n_con)] + ["unassigned"]
    torch.zeros(1, device="cuda")
    _lib.load()
    a = argparse.Namespace(min_mq=30, min_bq=30, cons_cov=2, verbose=False)
    dcols = observe.DeviceColumns(cols)
    start = torch.from_numpy(label).cuda()
    cr = assign.ContribReads(cols, start.clone(), names, list(names), dcols)
    ref_len = len(refseq)
    L = observe.pileup_length(cols, 30, ref_len)
    print("columns: %d alignments of %d fragments, L = %d; %d contributors with %s alignments, %d unassigned, %d in no row"
          % (len(cols), cols.n_frag, L, n_con, [cr.count(n) for n in names[:-1]], cr.count("unassigned"), int((label < 0).sum())))

    def reset():
        cr.relabel(start.clone(), torch.zeros_like(start))
        cr.rounds = 0

    # the yardstick: one labelled pileup of ALL alignments (4 tables)
    many = torch.zeros((len(names), L, 16), dtype=torch.int32, device="cuda")
    t_obs, s = timed(lambda: (many.zero_(), observe.count_bases_labelled(dcols, start, many)), opts.reps)
    print("mxm_observe_bases_labelled, every alignment, %d tables (median of %d): %.3f ms  [%s]" % (len(names), opts.reps, t_obs, s))

    # one round in parts
    use = list(range(n_con))
    pend = assemble._remap(start, use, len(names))
    counts = torch.zeros((n_con, L, 16), dtype=torch.int32, device="cuda")
    t_pile, s = timed(lambda: (counts.zero_(), observe.count_bases_labelled(dcols, pend, counts)), opts.reps)
    print("round 1 pileup (the contributors' %d alignments into %d tables): %.3f ms  [%s]"
          % (int((pend >= 0).sum()), n_con, t_pile, s))
    t_cons, s = timed(lambda: assemble._consensus_device(counts, ref_len, 2, True), opts.reps)
    print("mxm_consensus (%d x %d positions, strict): %.3f ms  [%s]" % (n_con, ref_len, t_cons, s))
    t_nv, s = timed(lambda: assemble._new_variants_device(refseq, cr, a, counts), opts.reps)
    nv = assemble._new_variants_device(refseq, cr, a, counts)
    print("consensus + mxm_new_variants (%d entries): %.3f ms  [%s]  (new variants alone: %.3f ms)" % (len(nv), t_nv, s, t_nv - t_cons))
    state = {"moved": torch.zeros(1, dtype=torch.int32, device="cuda")}
    t_asg, s = timed(lambda: assemble._extend_assign(cr, nv, a, state), opts.reps, before=reset)
    reset()
    state["moved"].zero_()
    assemble._extend_assign(cr, nv, a, state)
    moved1 = int(state["moved"].cpu()[0])
    print("mxm_extend_assign (walk of %d unassigned alignments + move of %d): %.3f ms  [%s]  = %.2fx the labelled pileup"
          % (int((start == n_con).sum()), moved1, t_asg, s, t_asg / t_obs))
    # a round after the first: counts only what moved
    pend2 = state["moved_owner"].clone()
    t_pile2, s = timed(lambda: observe.count_bases_labelled(dcols, pend2, counts), opts.reps)
    print("round 2 pileup (the %d alignments that moved, added to the tables): %.3f ms  [%s]  = %.2fx round 1's"
          % (moved1, t_pile2, s, t_pile2 / t_pile))

    # the whole extension
    walls, rounds = [], 0
    for _ in range(opts.reps + 1):
        reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assemble.extend_assemblies(refseq, cr, a)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        rounds = cr.rounds
    print("extend_assemblies, %d rounds, %d alignments left unassigned (host clock, median of %d after one warm-up): %.1f ms  [%s]"
          % (rounds, cr.count("unassigned"), opts.reps, float(numpy.median(walls[1:])), " ".join("%.1f" % t for t in walls[1:])))

    contribs = [[names[k], haps[synth.DEFAULT_CONTRIB[k]], synth.DEFAULT_PROPS[k]] for k in range(n_con)]
    walls = []
    with tempfile.TemporaryDirectory() as tmp:
        a.cons_prefix = os.path.join(tmp, "cons")
        for _ in range(opts.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assemble.write_consensus_seqs(refseq, contribs, cr, a)
            walls.append((time.perf_counter() - t0) * 1e3)
        size = os.path.getsize(a.cons_prefix + ".fa")
    print("write_consensus_seqs (%d sequences, %d bytes; host clock, median of %d after one warm-up): %.1f ms  [%s]"
          % (len(names), size, opts.reps, float(numpy.median(walls[1:])), " ".join("%.1f" % t for t in walls[1:])))

    if opts.numpy:
        import _assemble_ref
        table = _assemble_ref.Table(cols, label, names, list(names))
        t0 = time.perf_counter()
        nv_ref = _assemble_ref.find_new_variants(refseq, table, a)
        t1 = time.perf_counter()
        moved_ref = _assemble_ref.assign_reads_from_new_vars(table, nv_ref, a)
        t2 = time.perf_counter()
        print("numpy restatement, one round: find_new_variants %.2f s (%d entries), assign_reads_from_new_vars %.2f s (%d moved)"
              % (t1 - t0, len(nv_ref), t2 - t1, moved_ref))
        assert nv_ref == nv.as_dict() and moved_ref == moved1
    print("upload of the columns (host -> device, apart): %.1f ms" % (dcols.upload_s * 1e3))
    return 0


if __name__ == "__main__":
    sys.exit(main())
