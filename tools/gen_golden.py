#!/usr/bin/env python
"""
Golden-vector generator: runs ONLY in the build container, where the reference
is mounted at /root/reference.  It imports the reference's own modules (through
a package shim, because `import mixemt` pulls in pysam via assemble.py:22) and
records inputs + outputs of the hot path as small .npz fixtures under
tests/golden/.  Only the fixtures travel; no reference code does.

    python tools/gen_golden.py [--only g0,g1,...] [--out tests/golden]

Fixtures (SURVEY.md section 8 c):
    g0  Build-17 + RSRS tables: haplogroup order, sites, mut_prob, sparse markers
    g0b digests of the other shipped tree / flag combinations and of both reference sequences
    g1  9-haplogroup toy tree: signatures -> matrix, run_em for seeds x n_multi
    g2  Build 17: 32 synthetic rows -> full matrix; 1000 more rows -> row stats
    g3  em_step on 64 x 5408 (+ the two exact -inf cases of em_test.py:35-65)
    g4  run_em on 600 x 5408, n_multi = 1
    g5  run_em on the same matrix, n_multi = 3
    g6  refinement shape: 600 x 5 contributor columns
    g7  config 1: 1000 x 100
    g8  consumers of the result on the g4 run: contributor votes, read assignment, refinement
    g15 run_em on the g4 inputs stopped by max_iter = 5 and 25 (the loop's "never converged" exit, em.py:140-142)
    g9  run_em on 2400 x 5408 with de-duplication-style weights (repeats up to 400), n_multi = 1
    g10 build_em_matrix + run_em on 20 000 x 5408 (Zipf weights): the size at which the product
        leaves the one-launch loops / takes the row-dictionary branch of storage="auto".
        The reference's build runs in row blocks over worker processes (rows are independent,
        preprocess.py:188-191); its run_em is one process (hours).  --g10-rows N overrides.
    g11 front end: the reference's process_reads / reduce_reads / build_em_input
        (preprocess.py:99-139,163-174,201-227) on a few hundred synthetic alignments
        (tests/_fake_aln.py objects: mates, conflicting overlaps, low MQ / BQ, missing qualities,
        indels, soft clips, lower-case bases)
    g13 consumers of a MULTI-RUN result: the reference's _find_contribs_from_reads / get_contributors / assign_read_indexes
        (assemble.py:103-123, :284-334) on its own n_multi = 3 run of the g5 matrix (the logaddexp fold of three posteriors)
    g14 the unmixed sample: reduce_em_matrix to ONE contributor column -> run_em on 600 x 1 (n_multi 1 and 3) ->
        update_contribs -> assign_read_indexes with a single contributor (bin/mixemt:311-320)
    g12 on-disk formats: the bytes the reference's own dump_all writes (bin/mixemt:214-245) for a small run and what its
        load_prev (bin/mixemt:168-211) reads back from them
    g16 the variant check: the reference's ObservedBases (observe.py) over ~4 000 synthetic fragments with strands plus
        hand-made alignments (D, N, an H clip, non-ACGTN bases, an unplaced one, mapq / bq at the 29 / 30 edges) --
        tests/_pileup_aln.py objects --, its process_reads -> build_em_matrix -> run_em, get_contributors with the
        check on under four argument sets, write_base_obs bytes and get_ancestral of the candidates
    g17 mixemt's `-t` output: g16's alignments (make_g16_alignments, same seeds) through the reference's own pipeline on
        (get_contributors with the default check, reduce_em_matrix, refinement run_em, update_contribs), then its
        assemble.assign_reads over the alignment objects, stats.report_contributors and stats.write_statistics in
        bin/mixemt's order (bin/mixemt:296-338), for three cases: default, every row unassigned (a huge min_fold),
        one contributor (a min_reads that leaves one candidate)
    g18 mixemt's `-x` and `-b`: make_g18_alignments (synthetic fragments with PRIVATE variants planted in two contributors'
        sources, hand-made reads on the uncovered tail of the reference for ties and gaps) through the reference's
        pipeline as g17, then its own extend_assemblies / find_new_variants / call_consensus (both `strict`) /
        report_contributors / write_statistics over the alignment objects: per round the counters and the new-variant
        dict, the final key and the round of every alignment, the consensus strings, the verbose text and the files;
        plus a case where nothing is assigned (no contributor keys) and one whose cons_cov calls nothing.
        --cache DIR keeps the reference's matrix and EM result of g18 between runs of the generator.
    g19 the REFINED multi-run (-M 3): g13's contributor table (read from g13's file in --out) -> reduce_em_matrix -> run_em
        with n_multi = 3 on 600 x 3 -> update_contribs -> assign_read_indexes: the runs' inits, stops and folded
        proportions, the folded reduced posterior and every row's label
"""

import argparse
import hashlib
import io
import os
import re
import sys
import time
import types

import numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = "/root/reference"


def load_reference():
    pkg = types.ModuleType("mixemt")
    pkg.__path__ = [os.path.join(REF, "mixemt")]
    sys.modules["mixemt"] = pkg
    import mixemt.em
    import mixemt.phylotree
    import mixemt.preprocess
    return pkg


def ns(**kw):
    args = argparse.Namespace(init_alpha=1.0, tolerance=0.0001, max_iter=10000,
                              n_multi=1, verbose=False)
    for key, val in kw.items():
        setattr(args, key, val)
    return args


def sha(arr):
    return hashlib.sha256(numpy.ascontiguousarray(arr).tobytes()).hexdigest()


def ref_run_em(ref, mat, wts, seed, **kw):
    """Reference run_em with the iteration counts scraped from its -v output."""
    args = ns(verbose=True, **kw)
    numpy.random.seed(seed)
    inits = numpy.stack([numpy.random.dirichlet([args.init_alpha] * mat.shape[1])
                         for _ in range(args.n_multi)])
    numpy.random.seed(seed)
    err, sys.stderr = sys.stderr, io.StringIO()
    try:
        props, read_mix = ref.em.run_em(mat, wts, args)
        log = sys.stderr.getvalue()
    finally:
        sys.stderr = err
    iters = [int(x) for x in re.findall(r"Converged! \((\d+)\)", log)]
    assert len(iters) == args.n_multi, log[-200:]
    return props, read_mix, numpy.array(iters), inits


_G10 = None


def _g10_block(span):
    ref, refseq, phy, sigs, haps, quiet = _G10
    return ref.preprocess.build_em_matrix(refseq, phy, sigs[span[0]:span[1]], haps, quiet)


def make_g11_alignments(refseq, tables, n_frag=320, seed=1111):
    """
    Seeded alignments for g11: fragments of three contributors' sequences (the reference sequence with the
    contributor's expected base at every variant site), read length 80-150, with sequencing errors, indels, soft
    clips, lower-case bases, low mapping / base qualities, missing quality arrays, mates that overlap (some with a
    conflicting high-quality base at a variant site -> 'N' -> dropped, some whose conflict is a low-quality base),
    PCR-style duplicates (equal signatures -> weights > 1), and one fragment whose only site is conflicted away
    (empty signature).  -> (list of FakeAln, name of that fragment)
    """
    from _fake_aln import FakeAln
    rng = numpy.random.default_rng(seed)
    sites = numpy.asarray(tables.sites)
    seqs = []
    for col in (10, 2000, 4000):
        seq = numpy.frombuffer(refseq.encode(), dtype=numpy.uint8).copy()
        seq[sites] = tables.expected[:, col]
        seqs.append(seq)
    letters = numpy.frombuffer(b"ACGT", dtype=numpy.uint8)
    ref_len = len(refseq)

    def one(name, start, length, who, cigar_kind, mq, qual_kind, lower):
        src = seqs[who]
        if cigar_kind == "ins":
            a = int(rng.integers(10, length - 10)); k = int(rng.integers(1, 4))
            q = numpy.concatenate([src[start:start + a], rng.choice(letters, k), src[start + a:start + length - k]])
            cigar = "%dM%dI%dM" % (a, k, length - a - k)
        elif cigar_kind == "del":
            a = int(rng.integers(10, length - 10)); k = int(rng.integers(1, 6))
            q = numpy.concatenate([src[start:start + a], src[start + a + k:start + length + k]])
            cigar = "%dM%dD%dM" % (a, k, length - a)
        elif cigar_kind == "clip":
            k = int(rng.integers(2, 9))
            q = numpy.concatenate([rng.choice(letters, k), src[start:start + length - k]])
            cigar = "%dS%dM" % (k, length - k)
        else:
            q = src[start:start + length].copy()
            cigar = "%dM" % length
        q = q.copy()
        err = rng.random(q.size) < 0.004                          # sequencing errors
        q[err] = rng.choice(letters, int(err.sum()))
        text = q.tobytes().decode()
        if lower:
            text = text.lower()
        if qual_kind == "none":
            quals = None
        else:
            quals = rng.integers(31, 41, size=len(text)).tolist()
            if qual_kind == "low":
                for at in rng.choice(len(text), size=max(1, len(text) // 10), replace=False):
                    quals[int(at)] = int(rng.integers(2, 30))
        return FakeAln(name, int(start), int(mq), text, quals, cigar)

    alns = []
    for f in range(n_frag):
        name = "frag%04d" % f
        who = int(rng.choice(3, p=[0.6, 0.3, 0.1]))
        length = int(rng.integers(80, 151))
        # a third of the fragments start at one of a few fixed positions: equal signatures, weights > 1
        start = int(rng.choice([310, 2700, 7020, 11710, 16120])) if rng.random() < 0.33 else int(rng.integers(0, ref_len - 400))
        if rng.random() < 0.33:
            length = 120
        cigar_kind = str(rng.choice(["plain", "plain", "plain", "ins", "del", "clip"]))
        mq = int(rng.choice([60, 60, 60, 60, 42, 30, 29, 10, 0]))
        qual_kind = str(rng.choice(["ok", "ok", "ok", "low", "none"]))
        alns.append(one(name, start, length, who, cigar_kind, mq, qual_kind, rng.random() < 0.1))
        if rng.random() < 0.4:                                    # the mate, overlapping by 20-60 bases
            shift = length - int(rng.integers(20, 61))
            mate = one(name, start + shift, int(rng.integers(80, 151)), who, "plain", int(rng.choice([60, 60, 35, 12])),
                       str(rng.choice(["ok", "ok", "none"])), False)
            lo, hi = start + shift, start + length                # overlap on the reference
            inside = sites[(sites >= lo) & (sites < min(hi, lo + len(mate.query_sequence)))]
            if inside.size and rng.random() < 0.6:
                pos = int(inside[0]); at = pos - mate.reference_start
                was = mate.query_sequence[at]
                other = [c for c in "ACGT" if c != was.upper()][int(rng.integers(0, 3))]
                mate.query_sequence = mate.query_sequence[:at] + other + mate.query_sequence[at + 1:]
                if mate.query_qualities is not None:
                    # half of these conflicts are low-quality bases, which do not count (preprocess.py:122-123)
                    mate.query_qualities[at] = 5 if rng.random() < 0.5 else 38
            alns.append(mate)
    # one fragment whose only variant site is seen with two different high-quality bases: two 30-base mates
    # around the most isolated site of the tree (its neighbours are more than 20 bases away on both sides)
    gap = numpy.diff(sites)
    iso = numpy.minimum(gap[:-1], gap[1:])
    lone = int(sites[1:-1][int(iso.argmax())])
    assert iso.max() > 20
    first = one("lonely", lone - 15, 30, 0, "plain", 60, "ok", False)
    first.query_sequence = seqs[0][lone - 15:lone + 15].tobytes().decode()        # no sequencing error here
    first.query_qualities = [38] * 30
    base = first.query_sequence[15]
    flip = [c for c in "ACGT" if c != base][0]
    seq2 = seqs[0][lone - 10:lone + 20].tobytes().decode()
    second = FakeAln("lonely", lone - 10, 60, seq2[:10] + flip + seq2[11:], [38] * 30, "30M")
    alns.insert(len(alns) // 2, first)
    alns.append(second)
    order = rng.permutation(len(alns))                            # file order is not fragment order
    return [alns[i] for i in order], "lonely"


G16_SEED = 16          # synth_alignments seed of g16 (chosen so that the default check drops >= 1 candidate, keeps >= 2)
G16_EM_SEED = 7
G16_MIN_READS = 10


def make_g16_alignments(refseq, tables, n_frag=4000):
    """synth_alignments (with strands) + hand-made alignments for the pileup's edges -> (AlignmentColumns, objects)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pileup_aln import PileupAln, from_columns
    from mixemt_amd import synth
    from mixemt_amd.alignments import AlignmentColumns
    cols = synth.synth_alignments(tables, refseq, n_frag, seed=G16_SEED)
    alns = from_columns(cols)
    rng = numpy.random.default_rng(1616)

    def seq_at(start, n):
        return refseq[start:start + n]

    def q(n, v=38):
        return [v] * n

    M, I, D, N, S, H, P = 0, 1, 2, 3, 4, 5, 6
    extra = [
        # deletions and a reference skip, both strands
        PileupAln("h_del", 700, 60, seq_at(700, 40) + seq_at(745, 40), q(80), [(M, 40), (D, 5), (M, 40)], False),
        PileupAln("h_del_rev", 702, 60, seq_at(702, 30) + seq_at(735, 30), q(60), [(M, 30), (D, 3), (M, 30)], True),
        PileupAln("h_skip", 3000, 60, seq_at(3000, 30) + seq_at(3330, 30), q(60), [(M, 30), (N, 300), (M, 30)], False),
        PileupAln("h_skip_rev", 3010, 60, seq_at(3010, 20) + seq_at(3130, 20), q(40), [(M, 20), (N, 100), (M, 20)], True),
        # hard clip, soft clip, insertion, padding, '=' and 'X'
        PileupAln("h_clip", 5000, 60, "GGGG" + seq_at(5000, 50), q(54), [(H, 10), (S, 4), (M, 50), (H, 7)], False),
        PileupAln("h_ins", 5100, 60, seq_at(5100, 20) + "TT" + seq_at(5120, 20), q(42), [(M, 20), (I, 2), (P, 1), (M, 20)],
                  True),
        PileupAln("h_eqx", 5200, 60, seq_at(5200, 30), q(30), [(7, 20), (8, 10)], False),
        # characters other than ACGTN (and lower case) on both strands
        PileupAln("h_iupac", 9000, 60, "ACRYacgtnN*" + seq_at(9011, 29), q(40), [(M, 40)], False),
        PileupAln("h_iupac_rev", 9005, 60, "ryKM" + seq_at(9009, 26), q(30), [(M, 30)], True),
        # an unplaced alignment, and no quality array
        PileupAln("h_unplaced", -1, 60, seq_at(0, 30), q(30), [(M, 30)], False),
        PileupAln("h_noqual", 9100, 60, seq_at(9100, 30), None, [(M, 30)], True),
        # mapq and base quality at the 29 / 30 edges
        PileupAln("h_mq29", 9200, 29, seq_at(9200, 30), q(30), [(M, 30)], False),
        PileupAln("h_mq30", 9200, 30, seq_at(9200, 30), q(30), [(M, 30)], False),
        PileupAln("h_bq", 9300, 60, seq_at(9300, 40), [29, 30] * 20, [(M, 40)], False),
        PileupAln("h_bq_rev", 9300, 60, seq_at(9300, 40), [30, 29] * 20, [(M, 40)], True),
        # a read running off the end of the reference (the table grows past ref_len)
        PileupAln("h_end", len(refseq) - 20, 60, "ACGT" * 10, q(40), [(M, 40)], False),
    ]
    order = rng.permutation(len(alns) + len(extra))
    every = [(alns + extra)[k] for k in order]
    cols = AlignmentColumns.from_alignments(every)
    return cols, from_columns(cols)


G17_REFINE_SEED = 17   # numpy.random seed in front of g17's refinement run_em


def _columns_sha(cols):
    h = hashlib.sha256()
    for name in ("ref_start", "mapq", "frag", "cig_ptr", "cigar", "seq_ptr", "seq", "qual", "has_qual", "is_reverse"):
        h.update(numpy.ascontiguousarray(getattr(cols, name)).tobytes())
    h.update("\n".join(cols.names).encode())
    return h.hexdigest()


G18_SEED = 18          # synth_alignments seed of g18 (the section's asserts say what it was chosen for)
G18_CONS_COV = 2
G18_TAIL = 110         # the hand-made reads sit on the last G18_TAIL positions, which no synthetic read reaches


def g18_private(refseq, tables):
    """(contributor, position, base) of g18's planted variants: every 40 positions, off the Phylotree sites, for the
    first two contributors (20 apart: a read of the third contributor shows the reference base at both, which belongs
    to the OTHER contributor each time -- the fragments that see two owners), a base other than the reference's."""
    sites = set(int(p) for p in tables.sites)
    out = []
    for k, first in ((0, 200), (1, 220)):
        for pos in range(first, len(refseq) - 500, 40):
            if pos not in sites and refseq[pos] in "ACGT":
                out.append((k, pos, "ACGT"[("ACGT".index(refseq[pos]) + 1 + k) % 4]))
    return out


def make_g18_alignments(refseq, tables, n_frag=4000):
    """synth_alignments with planted private variants + hand-made reads on the tail -> (AlignmentColumns, objects)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _pileup_aln import PileupAln, from_columns
    from mixemt_amd import synth
    from mixemt_amd.alignments import AlignmentColumns
    cols = synth.synth_alignments(tables, refseq, n_frag, seed=G18_SEED, private=g18_private(refseq, tables))
    alns = from_columns(cols)
    rng = numpy.random.default_rng(1818)
    n = len(refseq)
    t0 = n - G18_TAIL
    M, D = 0, 2

    def edited(start, length, edits):
        seq = list(refseq[start:start + length])
        for pos, base in edits:
            seq[pos - start] = base
        return "".join(seq)

    def other(pos, step):
        return "ACGT"[("ACGT".index(refseq[pos]) + step) % 4] if refseq[pos] in "ACGT" else "A"

    sites = set(int(p) for p in tables.sites)
    extra = []
    # pairs of reads, one per strand, that disagree at five positions each (no Phylotree site: the pair shares its
    # signature, so its row): 1 : 1 ties, decided by the file order
    for k in range(6):
        start = t0 + 2 * k
        at = [p for p in range(start + 5 + k, start + 80, 3) if p not in sites][::5][:5]
        extra.append(PileupAln("t_tie%d" % k, start, 60, edited(start, 80, [(p, other(p, 1 + k % 3)) for p in at]), [38] * 80,
                               [(M, 80)], k % 2 == 0))
        extra.append(PileupAln("t_tie%d_b" % k, start, 60, edited(start, 80, [(p, other(p, 1 + (k + 1) % 3)) for p in at]),
                               [38] * 80, [(M, 80)], k % 2 == 1))
    # two reads with the same deletion over positions nothing else covers (a gap called at coverage 2), and one with a
    # deletion of its own under them (1 gap : 2 bases)
    for k in range(3):
        start = t0 + 1
        d0, dlen = (n - 12, 3) if k < 2 else (n - 18, 2)
        seq = refseq[start:d0] + refseq[d0 + dlen:d0 + dlen + 4]
        extra.append(PileupAln("t_gap%d" % k, start, 60, seq, [38] * len(seq), [(M, d0 - start), (D, dlen), (M, 4)], k == 1))
    order = rng.permutation(len(alns) + len(extra))
    every = [(alns + extra)[k] for k in order]
    cols = AlignmentColumns.from_alignments(every)
    return cols, from_columns(cols)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    ap.add_argument("--g10-rows", type=int, default=20000)
    ap.add_argument("--workers", type=int, default=6)
    ap.add_argument("--cache", default="", help="g18: keep the reference's matrix and EM result in this directory")
    opts = ap.parse_args()
    only = set(x for x in opts.only.split(",") if x)
    os.makedirs(opts.out, exist_ok=True)

    def want(name):
        return not only or name in only

    def save(name, **arrays):
        path = os.path.join(opts.out, name + ".npz")
        numpy.savez_compressed(path, **arrays)
        print("%-4s %8.1f KB  %s" % (name, os.path.getsize(path) / 1024.0, path))

    ref = load_reference()
    from mixemt_amd import phylotree as my_phy
    from mixemt_amd import preprocess as my_pre
    from mixemt_amd import synth

    refseq = my_phy.read_fasta_first(os.path.join(REF, "mixemt/ref/RSRS.mtDNA.fa"))
    with open(os.path.join(REF, "mixemt/phylotree/mtDNA_tree_Build_17.csv")) as fin:
        phy = ref.phylotree.Phylotree(fin, refseq=refseq, anon_haps=True)
    haps = sorted(phy.hap_var)
    # encoder only (host tables for the generator); checked against the reference in g0
    tables = my_pre.HapVarTables.build(refseq, phy, haps)
    quiet = ns()

    if want("g0"):
        hvb = ref.preprocess.HapVarBaseMatrix(refseq, phy)
        sites = numpy.array(phy.get_variant_pos(), dtype=numpy.int64)
        where = {int(p): k for k, p in enumerate(sites)}
        mh, ms, mb = [], [], []
        dense = numpy.empty((len(sites), len(haps)), dtype=numpy.uint8)
        dense[:, :] = numpy.array([ord(refseq[p]) for p in sites], dtype=numpy.uint8)[:, None]
        for j, hap in enumerate(haps):
            for pos, base in sorted(hvb.markers[hap].items()):
                mh.append(j); ms.append(where[pos]); mb.append(ord(base))
                dense[where[pos], j] = ord(base)
        mut = numpy.array([hvb.mut_prob[int(p)] for p in sites])
        save("g0_tables_b17",
             hap_names=numpy.array("\n".join(haps)),
             sites=sites, mut_prob=mut,
             marker_hap=numpy.array(mh, dtype=numpy.uint16),
             marker_site=numpy.array(ms, dtype=numpy.uint16),
             marker_base=numpy.array(mb, dtype=numpy.uint8),
             ref_codes=numpy.array([ord(refseq[p]) for p in sites], dtype=numpy.uint8),
             dense_sha256=numpy.array(sha(dense)),
             n_haps=numpy.array(len(haps)), n_sites=numpy.array(len(sites)))

    if want("g0b"):
        # the other shipped tree / flag combinations: digests of what the reference parses
        out = {}
        for tag, fn, kw in (("b16", "mtDNA_tree_Build_16.csv", dict(anon_haps=True)),
                            ("b17_named", "mtDNA_tree_Build_17.csv", dict(anon_haps=False)),
                            ("b17_stable", "mtDNA_tree_Build_17.csv", dict(anon_haps=True, rm_unstable=True)),
                            ("b17_strict", "mtDNA_tree_Build_17.csv",
                             dict(anon_haps=True, rm_unstable=True, rm_backmut=True))):
            with open(os.path.join(REF, "mixemt/phylotree", fn)) as fin:
                tree = ref.phylotree.Phylotree(fin, refseq=refseq, **kw)
            names = sorted(tree.hap_var)
            text = "\n".join("%s\t%s" % (n, ",".join(tree.hap_var[n])) for n in names)
            counts = "\n".join("%d\t%s" % (p, ",".join("%s=%d" % kv for kv in sorted(tree.variants[p].items())))
                               for p in sorted(tree.variants))
            out[tag + "_n_haps"] = numpy.array(len(names))
            out[tag + "_n_sites"] = numpy.array(len(tree.variants))
            out[tag + "_hap_var_sha256"] = numpy.array(hashlib.sha256(text.encode()).hexdigest())
            out[tag + "_variants_sha256"] = numpy.array(hashlib.sha256(counts.encode()).hexdigest())
        rcrs = my_phy.read_fasta_first(os.path.join(REF, "mixemt/ref/rCRS.mtDNA.fa"))
        out["rcrs_sha256"] = numpy.array(hashlib.sha256(rcrs.encode()).hexdigest())
        out["rsrs_sha256"] = numpy.array(hashlib.sha256(refseq.encode()).hexdigest())
        save("g0b_trees", **out)

    if want("g1"):
        toy = ref.phylotree.example()
        toy_ref = "AAAAAAAAA"
        reads = ["1:A,2:T,3:A", "2:T,3:A", "3:A,4:T,5:T", "5:T,6:A", "6:A,7:T",
                 "6:A,7:T,8:A", "7:T,8:A", "4:T,5:T", "1:A,2:T,3:T,4:T", "5:A,6:T,7:A,8:A"]
        thaps = list("ABCDEFGHI")
        mat = ref.preprocess.build_em_matrix(toy_ref, toy, reads, thaps, quiet)
        reads_b = ["1:A,2:C", "1:T,2:C", "3:T,4:T", "2:A,4:T"]     # preprocess_test.py:269
        mat_b = ref.preprocess.build_em_matrix(toy_ref, toy, reads_b, thaps, quiet)
        out = dict(reads=numpy.array("\n".join(reads)), reads_b=numpy.array("\n".join(reads_b)),
                   mat=mat, mat_b=mat_b)
        for n_multi in (1, 3):
            for seed in (1, 2, 3):
                props, mix, iters, inits = ref_run_em(ref, mat, numpy.ones(len(reads)), seed,
                                                      n_multi=n_multi, max_iter=1000)
                key = "m%d_s%d" % (n_multi, seed)
                out[key + "_props"] = props
                out[key + "_mix"] = mix
                out[key + "_iters"] = iters
                out[key + "_inits"] = inits
        save("g1_toy", **out)

    if want("g2"):
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 1032, seed=2)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        t0 = time.time()
        mat = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
        print("g2: reference built 1032 x %d in %.0f s" % (len(haps), time.time() - t0))
        save("g2_build_b17", row_ptr=row_ptr, site=site, obs=obs,
             mat32=mat[:32].copy(),
             row_sum=mat.sum(axis=1), row_min=mat.min(axis=1), row_max=mat.max(axis=1),
             row_argmax=mat.argmax(axis=1).astype(numpy.int32),
             col_sum=mat.sum(axis=0), mat_sha256=numpy.array(sha(mat)))

    if want("g3"):
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 64, seed=3)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        mat = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
        rng = numpy.random.default_rng(33)
        wts = rng.integers(1, 6, size=64).astype(numpy.int64)
        lnp = numpy.log(rng.dirichlet([1.0] * len(haps)))
        mix = numpy.empty_like(mat)
        mix, new_props = ref.em.em_step(mat, wts, lnp, mix)
        inf = float("inf")
        ident = numpy.array([[0.0, -inf, -inf], [-inf, 0.0, -inf], [-inf, -inf, 0.0]])
        p3 = numpy.log(numpy.array([0.6, 0.2, 0.2]))
        r1 = ref.em.em_step(ident, numpy.array([1, 1, 1]), p3, numpy.empty_like(ident))
        r2 = ref.em.em_step(ident, numpy.array([2, 1, 1]), p3, numpy.empty_like(ident))
        save("g3_em_step", row_ptr=row_ptr, site=site, obs=obs, mat_sha256=numpy.array(sha(mat)),
             wts=wts, lnp=lnp, mix_rows=mix[:8].copy(), mix_sha256=numpy.array(sha(mix)),
             mix_rowmax=mix.max(axis=1), mix_argmax=mix.argmax(axis=1).astype(numpy.int32),
             new_props=new_props,
             ident=ident, ident_lnp=p3, ident_mix1=r1[0], ident_new1=r1[1],
             ident_mix2=r2[0], ident_new2=r2[1])

    mat600 = None
    wts600 = None
    if want("g4") or want("g5") or want("g6") or want("g15"):
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 600, seed=4)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        t0 = time.time()
        mat600 = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
        print("g4-6: reference built 600 x %d in %.0f s" % (len(haps), time.time() - t0))
        wts600 = numpy.random.default_rng(44).integers(1, 4, size=600).astype(numpy.int64)
        common = dict(row_ptr=row_ptr, site=site, obs=obs, who=who, wts=wts600,
                      mat_sha256=numpy.array(sha(mat600)))

    def votes_of(mix, wts, n):
        best = mix.argmax(axis=1)
        votes = numpy.zeros(n)
        numpy.add.at(votes, best, wts)          # assemble.py:115-123
        return best.astype(numpy.int32), votes

    if want("g4"):
        t0 = time.time()
        props, mix, iters, inits = ref_run_em(ref, mat600, wts600, 7)
        print("g4: reference run_em %d iterations in %.0f s" % (iters[0], time.time() - t0))
        best, votes = votes_of(mix, wts600, len(haps))
        save("g4_run_em", props=props, iters=iters, inits=inits, mix_rows=mix[:4].copy(),
             mix_argmax=best, votes=votes, mix_rowmax=mix.max(axis=1),
             contributors=numpy.flatnonzero(votes >= 10).astype(numpy.int32), **common)

    if want("g15"):
        # the reference's own loop stopped by max_iter (em.py:140-142, "never converged": the vectors are flipped back
        # and the last step's results returned) after 5 and after 25 iterations of the g4 run: cheap enough for the
        # default CPU suite to pin the oracle's loop on a Build-17 matrix bit for bit, and a mid-run pin for the GPU loop
        out = {}
        for k in (5, 25):
            numpy.random.seed(7)
            props, mix = ref.em.run_em(mat600, wts600, ns(max_iter=k))
            out["props_%d" % k] = props
            out["mix_rows_%d" % k] = mix[:4].copy()
            out["mix_rowmax_%d" % k] = mix.max(axis=1)
            out["mix_argmax_%d" % k] = mix.argmax(axis=1).astype(numpy.int32)
        save("g15_run_em_max_iter", **out, **common)

    if want("g5"):
        t0 = time.time()
        props, mix, iters, inits = ref_run_em(ref, mat600, wts600, 11, n_multi=3)
        print("g5: reference run_em x3 %s iterations in %.0f s" % (iters, time.time() - t0))
        best, votes = votes_of(mix, wts600, len(haps))
        save("g5_run_em_multi", props=props, iters=iters, inits=inits, mix_rows=mix[:16].copy(),
             mix_argmax=best, votes=votes, mix_rowmax=mix.max(axis=1), **common)

    if want("g6"):
        contribs = [["hap1", haps[10], 0.6], ["hap2", haps[2000], 0.3], ["hap3", haps[4000], 0.1],
                    ["hap4", haps[11], 0.0], ["hap5", haps[3000], 0.0]]
        sub, names = ref.preprocess.reduce_em_matrix(mat600, haps, contribs)
        props, mix, iters, inits = ref_run_em(ref, sub, wts600, 5)
        save("g6_refine", cols=numpy.array([haps.index(n) for n in names], dtype=numpy.int32),
             props=props, iters=iters, inits=inits, mix=mix, **common)

    if want("g8"):
        # consumers of the EM result (assemble.py / stats.py); assemble imports pysam and Bio at
        # module level only for its writers, so empty stand-in modules are enough to import it
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        import mixemt.assemble
        import mixemt.stats
        if mat600 is None:
            row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 600, seed=4)
            sigs = synth.signatures(tables, row_ptr, site, obs)
            mat600 = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
            wts600 = numpy.random.default_rng(44).integers(1, 4, size=600).astype(numpy.int64)
        props, mix, iters, inits = ref_run_em(ref, mat600, wts600, 7)
        asm_args = ns(min_reads=10, contributors=None, var_check=False, min_fold=2.0)
        cons = ref.assemble._find_contribs_from_reads(mix, wts600, asm_args)
        contribs = ref.assemble.get_contributors(phy, None, haps, wts600, (props, mix), asm_args)
        reads_stub = [[str(i)] for i in range(600)]
        table = ref.assemble.assign_read_indexes(contribs, (props, mix), haps, reads_stub, 2.0)
        assigned = numpy.full(600, -2, dtype=numpy.int32)
        names = [c[0] for c in contribs]
        for key, idxs in table.items():
            assigned[sorted(idxs)] = -1 if key == "unassigned" else names.index(key)
        err, sys.stderr = sys.stderr, io.StringIO()
        try:
            ref.stats.report_read_votes(haps, mix, 10)
            vote_text = sys.stderr.getvalue()
        finally:
            sys.stderr = err
        # refinement on the contributor columns (bin/mixemt:311-320)
        sub, sub_names = ref.preprocess.reduce_em_matrix(mat600, haps, contribs)
        rprops, rmix, riters, rinits = ref_run_em(ref, sub, wts600, 13)
        refined = ref.assemble.update_contribs([list(c) for c in contribs], (rprops, rmix), sub_names)
        rtable = ref.assemble.assign_read_indexes(refined, (rprops, rmix), sub_names, reads_stub, 2.0)
        rassigned = numpy.full(600, -2, dtype=numpy.int32)
        for key, idxs in rtable.items():
            rassigned[sorted(idxs)] = -1 if key == "unassigned" else names.index(key)
        save("g8_consumers", contributors=numpy.array(cons, dtype=numpy.int32),
             contrib_names=numpy.array("\n".join(names)),
             contrib_haps=numpy.array("\n".join(c[1] for c in contribs)),
             contrib_props=numpy.array([c[2] for c in contribs]),
             assigned=assigned, vote_text=numpy.array(vote_text),
             refined_props=numpy.array([c[2] for c in refined]), refined_iters=riters,
             refined_inits=rinits, refined_assigned=rassigned,
             props=props, iters=iters)

    if want("g14"):
        # the commonest real input: an UNMIXED sample.  One contributor -> reduce_em_matrix keeps one column
        # (preprocess.py:247-251) and bin/mixemt:311-320 calls run_em on R x 1, then update_contribs and
        # assign_read_indexes with a single contributor (assemble.py:211-230, :284-334).
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        import mixemt.assemble
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 600, seed=4)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        m600 = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
        w600 = numpy.random.default_rng(44).integers(1, 4, size=600).astype(numpy.int64)
        one = [["hap1", haps[10], 1.0]]
        sub, sub_names = ref.preprocess.reduce_em_matrix(m600, haps, one)
        assert sub.shape == (600, 1)
        props1, mix1, iters1, inits1 = ref_run_em(ref, sub, w600, 13)
        refined = ref.assemble.update_contribs([list(c) for c in one], (props1, mix1), sub_names)
        table = ref.assemble.assign_read_indexes(refined, (props1, mix1), sub_names, [[str(i)] for i in range(600)], 2.0)
        assert list(table) == ["hap1"] and len(table["hap1"]) == 600
        # and three restarts of the same (the geometric mean of three [1.0] vectors)
        props3, mix3, iters3, inits3 = ref_run_em(ref, sub, w600, 13, n_multi=3)
        save("g14_single_contributor", row_ptr=row_ptr, site=site, obs=obs, wts=w600, col=numpy.array([10], dtype=numpy.int32),
             sub=sub, props=props1, mix=mix1, iters=iters1, inits=inits1, refined_props=numpy.array([c[2] for c in refined]),
             assigned=numpy.array(sorted(table["hap1"]), dtype=numpy.int32),
             props3=props3, mix3=mix3, iters3=iters3, inits3=inits3)

    if want("g9"):
        # 4x the g4 size, weights as reduce_reads leaves them (preprocess.py:218-220: fragments per
        # distinct signature -- mostly 1, a heavy tail of repeats up to a few hundred)
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 2400, seed=9)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        t0 = time.time()
        mat = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
        print("g9: reference built 2400 x %d in %.0f s" % (len(haps), time.time() - t0))
        rng = numpy.random.default_rng(99)
        wts = numpy.minimum(rng.zipf(1.6, size=2400), 400).astype(numpy.int64)
        t0 = time.time()
        props, mix, iters, inits = ref_run_em(ref, mat, wts, 17)
        print("g9: reference run_em %d iterations in %.0f s" % (iters[0], time.time() - t0))
        best, votes = votes_of(mix, wts, len(haps))
        save("g9_run_em_2400", row_ptr=row_ptr, site=site, obs=obs, who=who, wts=wts,
             mat_sha256=numpy.array(sha(mat)), mat_row_sum=mat.sum(axis=1),
             props=props, iters=iters, inits=inits, mix_rows=mix[:4].copy(),
             mix_argmax=best, mix_argmax_sha256=numpy.array(sha(best)), votes=votes,
             mix_rowmax=mix.max(axis=1), mix_row_lse_abs_max=numpy.array(
                 numpy.abs(numpy.log(numpy.exp(mix).sum(axis=1))).max()),
             contributors=numpy.flatnonzero(votes >= 10).astype(numpy.int32))


    if want("g10"):
        n10 = opts.g10_rows
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), n10, seed=10)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        t0 = time.time()
        import multiprocessing
        step = 250
        blocks = [(a, min(a + step, n10)) for a in range(0, n10, step)]
        global _G10
        _G10 = (ref, refseq, phy, sigs, haps, quiet)
        with multiprocessing.get_context("fork").Pool(opts.workers) as pool:
            parts = pool.map(_g10_block, blocks)
        mat = numpy.concatenate(parts, axis=0)
        del parts
        print("g10: reference built %d x %d in %.0f s (%d workers)"
              % (n10, len(haps), time.time() - t0, opts.workers), flush=True)
        rng = numpy.random.default_rng(1010)
        wts = numpy.minimum(rng.zipf(1.6, size=n10), 400).astype(numpy.int64)
        mat_sha = sha(mat)
        numpy.save("/tmp/g10_mat.npy", mat)           # scratch: lets a rerun skip the build
        t0 = time.time()
        props, mix, iters, inits = ref_run_em(ref, mat, wts, 23)
        print("g10: reference run_em %d iterations in %.0f s" % (iters[0], time.time() - t0), flush=True)
        best, votes = votes_of(mix, wts, len(haps))
        pick = numpy.arange(0, n10, max(n10 // 8, 1))[:8]
        save("g10_run_em_20k", n_rows=numpy.array(n10), synth_seed=numpy.array(10),
             csr_sha256=numpy.array(sha(row_ptr) + sha(site) + sha(obs)),
             wts=wts.astype(numpy.int16), mat_sha256=numpy.array(mat_sha),
             mat_row_sum=mat.sum(axis=1), props=props, iters=iters, inits=inits,
             mix_pick=pick, mix_rows=mix[pick].copy(),
             mix_argmax=best.astype(numpy.int16), mix_argmax_sha256=numpy.array(sha(best)), votes=votes,
             mix_rowmax=mix.max(axis=1),
             contributors=numpy.flatnonzero(votes >= 10).astype(numpy.int32))

    if want("g11"):
        # front end (row f-4) by a reference RUN: process_reads / reduce_reads / build_em_input on duck-typed
        # alignments (tests/_fake_aln.py implements the pysam attributes preprocess.py:99-139 touches)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import json
        from _fake_aln import FakeAln, FakeBam
        alns, empty_name = make_g11_alignments(refseq, tables)
        var_pos = phy.get_variant_pos()
        fe_args = ns(min_mq=30, min_bq=30)
        obs_all = ref.preprocess.process_reads(alns, var_pos, fe_args.min_mq, fe_args.min_bq)
        sigs_all = ref.preprocess.reduce_reads(obs_all)
        assert "" in sigs_all and sigs_all[""] == [empty_name], sigs_all.get("")
        # the reference itself dies on the fragment whose every site was conflicted away (int('') at :156-160) ...
        try:
            ref.preprocess.build_em_input(FakeBam(alns), refseq, phy, fe_args)
            died = ""
        except ValueError as exc:
            died = "ValueError: %s" % exc
        assert died, "the reference was expected to stop on the empty signature"
        # ... so the full comparison runs on the same alignments without that fragment
        kept = [a for a in alns if a.query_name != empty_name]
        t0 = time.time()
        mat, wts, hap_order, read_ids = ref.preprocess.build_em_input(FakeBam(kept), refseq, phy, fe_args)
        print("g11: reference build_em_input on %d alignments -> %d x %d in %.0f s"
              % (len(kept), mat.shape[0], mat.shape[1], time.time() - t0), flush=True)
        obs_kept = ref.preprocess.process_reads(kept, var_pos, fe_args.min_mq, fe_args.min_bq)
        sig_kept = ref.preprocess.reduce_reads(obs_kept)
        rows = sorted(sig_kept)
        save("g11_frontend",
             alns=numpy.array(json.dumps([[a.query_name, a.reference_start, a.mapping_quality, a.query_sequence,
                                           a.query_qualities, a.cigarstring] for a in alns])),
             empty_name=numpy.array(empty_name), min_mq=numpy.array(30), min_bq=numpy.array(30),
             read_obs=numpy.array(json.dumps({name: {str(p): b for p, b in sorted(o.items())}
                                              for name, o in sorted(obs_all.items())})),
             read_sigs=numpy.array(json.dumps({sig: ids for sig, ids in sorted(sigs_all.items())})),
             ref_died_with=numpy.array(died),
             signatures=numpy.array("\n".join(rows)), weights=numpy.asarray(wts, dtype=numpy.int64),
             read_ids=numpy.array(json.dumps(read_ids)), hap_sha256=numpy.array(
                 hashlib.sha256("\n".join(hap_order).encode()).hexdigest()),
             mat_sha256=numpy.array(sha(mat)), mat_row_sum=mat.sum(axis=1), mat_rows=mat[:3].copy())

    if want("g12"):
        # the -s / -l files, written and read back by the reference's own functions (bin/mixemt is a script: loaded as a
        # module; its main() sits behind the __main__ guard)
        import importlib.machinery
        import tempfile
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO", "pkg_resources"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        cli = importlib.machinery.SourceFileLoader("mixemt_cli", os.path.join(REF, "bin", "mixemt")).load_module()
        rng = numpy.random.default_rng(1212)
        io_haps = ["A12a", "B4'5", "H2a2a1", "L3e1a1a", "M9a'b", "R0", "U5b2a1a1"]
        io_reads = [["frag0001"], ["frag0002", "frag0007", "frag0100"], ["r/1", "r/2"], ["x"], ["y y", "z"]]
        io_em = rng.normal(-20.0, 7.0, size=(5, 7))
        io_mix = io_em - numpy.log(numpy.exp(io_em).sum(axis=1, keepdims=True))
        io_props = rng.dirichlet([1.0] * 7)
        out = {}
        with tempfile.TemporaryDirectory() as tmp:
            prefix = os.path.join(tmp, "run")
            cli.dump_all(prefix, io_haps, io_reads, io_em, (io_props, io_mix))
            for ext in ("haps", "reads", "em.npy", "mat.npy", "prop.npy"):
                with open("%s.%s" % (prefix, ext), "rb") as fin:
                    out["file_" + ext.replace(".", "_")] = numpy.frombuffer(fin.read(), dtype=numpy.uint8)
            haps2, reads2, wts2, init2, (props2, mat2) = cli.load_prev(prefix)
        import json
        save("g12_io_formats", haps=numpy.array("\n".join(io_haps)), reads=numpy.array(json.dumps(io_reads)),
             em=io_em, mix=io_mix, props=io_props, loaded_haps=numpy.array("\n".join(haps2)),
             loaded_reads=numpy.array(json.dumps(reads2)), loaded_wts=numpy.asarray(wts2), loaded_init=init2,
             loaded_props=props2, loaded_mat=mat2, **out)

    if want("g13"):
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        import mixemt.assemble
        import mixemt.stats
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 600, seed=4)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        mat = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
        wts = numpy.random.default_rng(44).integers(1, 4, size=600).astype(numpy.int64)
        t0 = time.time()
        props, mix, iters, inits = ref_run_em(ref, mat, wts, 11, n_multi=3)
        print("g13: reference run_em x3 %s iterations in %.0f s" % (iters, time.time() - t0), flush=True)
        asm_args = ns(min_reads=10, contributors=None, var_check=False, min_fold=2.0)
        cons = ref.assemble._find_contribs_from_reads(mix, wts, asm_args)
        contribs = ref.assemble.get_contributors(phy, None, haps, wts, (props, mix), asm_args)
        reads_stub = [[str(i)] for i in range(600)]
        table = ref.assemble.assign_read_indexes(contribs, (props, mix), haps, reads_stub, 2.0)
        names = [c[0] for c in contribs]
        assigned = numpy.full(600, -2, dtype=numpy.int32)
        for key, idxs in table.items():
            assigned[sorted(idxs)] = -1 if key == "unassigned" else names.index(key)
        err, sys.stderr = sys.stderr, io.StringIO()
        try:
            ref.stats.report_read_votes(haps, mix, 10)
            vote_text = sys.stderr.getvalue()
        finally:
            sys.stderr = err
        save("g13_consumers_multi", contributors=numpy.array(cons, dtype=numpy.int32),
             contrib_names=numpy.array("\n".join(names)), contrib_haps=numpy.array("\n".join(c[1] for c in contribs)),
             contrib_props=numpy.array([c[2] for c in contribs]), assigned=assigned, vote_text=numpy.array(vote_text),
             props=props, iters=iters, inits=inits, mat_sha256=numpy.array(sha(mat)))

    if want("g19"):
        # the REFINED multi-run: bin/mixemt:311-320 with -M 3 on g13's contributors.  The refinement depends on the reduced
        # matrix alone, so the first EM is not run again: the contributor table is g13's own.
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        import mixemt.assemble
        g13 = numpy.load(os.path.join(opts.out, "g13_consumers_multi.npz"))
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 600, seed=4)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        t0 = time.time()
        mat = ref.preprocess.build_em_matrix(refseq, phy, sigs, haps, quiet)
        assert sha(mat) == str(g13["mat_sha256"])
        wts = numpy.random.default_rng(44).integers(1, 4, size=600).astype(numpy.int64)
        contribs = [[n, h, float(p)] for n, h, p in zip(str(g13["contrib_names"]).split("\n"),
                                                        str(g13["contrib_haps"]).split("\n"), g13["contrib_props"])]
        sub, sub_names = ref.preprocess.reduce_em_matrix(mat, haps, contribs)
        props, mix, iters, inits = ref_run_em(ref, sub, wts, 23, n_multi=3)
        print("g19: matrix + refinement x3 %s iterations in %.0f s" % (iters, time.time() - t0), flush=True)
        refined = ref.assemble.update_contribs([list(c) for c in contribs], (props, mix), sub_names)
        table = ref.assemble.assign_read_indexes(refined, (props, mix), sub_names, [[str(i)] for i in range(600)], 2.0)
        names = [c[0] for c in refined]
        assigned = numpy.full(600, -2, dtype=numpy.int32)
        for key, idxs in table.items():
            assigned[sorted(idxs)] = -1 if key == "unassigned" else names.index(key)
        assert (assigned >= -1).all()
        with numpy.errstate(divide="ignore", invalid="ignore"):
            v = numpy.sort(mix - numpy.log(props), axis=1)
        print("g19: %s; stops %s; props %s (sum %.8f); assigned %s, unassigned %d; closest margin to log 2: %.3f"
              % (" / ".join(sub_names), [int(v) for v in iters], props, props.sum(), [int((assigned == k).sum()) for k in range(len(names))],
                 int((assigned < 0).sum()), numpy.abs((v[:, -1] - v[:, -2]) - numpy.log(2.0)).min()), flush=True)
        save("g19_refine_multi", cols=numpy.array([haps.index(n) for n in sub_names], dtype=numpy.int32), props=props,
             iters=iters, inits=inits, mix=mix, refined_props=numpy.array([c[2] for c in refined]),
             contrib_names=numpy.array("\n".join(names)), assigned=assigned, row_ptr=row_ptr, site=site, obs=obs, wts=wts)

    if want("g16"):
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        import mixemt.assemble
        import mixemt.observe
        import mixemt.stats
        cols, alns = make_g16_alignments(refseq, tables)
        t0 = time.time()
        obs = ref.observe.ObservedBases(alns, mapq=30, baseq=30)
        trip = [(pos, key, cnt) for pos in sorted(obs.obs_tab) for key, cnt in sorted(obs.obs_tab[pos].items())]
        read_obs = ref.preprocess.process_reads(alns, phy.get_variant_pos(), 30, 30)
        read_sigs = ref.preprocess.reduce_reads(read_obs)
        read_sigs.pop("", None)                      # (a fragment conflicted away: the reference dies on it, see g11)
        rows = sorted(read_sigs)
        wts = numpy.array([len(read_sigs[r]) for r in rows])
        mat = ref.preprocess.build_em_matrix(refseq, phy, rows, haps, quiet)
        props, mix, iters, inits = ref_run_em(ref, mat, wts, G16_EM_SEED)
        print("g16: pileup + matrix %d x %d + run_em in %.0f s" % (mat.shape[0], mat.shape[1], time.time() - t0), flush=True)
        base = dict(min_reads=G16_MIN_READS, contributors=None, var_check=True, min_fold=2.0, min_var_reads=3,
                    frac_var_reads=0.02, var_fraction=0.5, var_count=None)
        variants = [("default", {}), ("var_count_1", {"var_count": 1}), ("var_fraction_0.9", {"var_fraction": 0.9}),
                    ("min_var_reads_10", {"min_var_reads": 10})]
        cand = ref.assemble._find_contribs_from_reads(mix, wts, ns(**base))
        out = {}
        for label, kw in variants:
            a = ns(**dict(base, **kw))
            got = ref.assemble.get_contributors(phy, obs, haps, wts, (props, mix), a)
            out["contribs_" + label] = numpy.array("\n".join("%s\t%s\t%r" % (c[0], c[1], float(c[2])) for c in got))
        a = ns(**dict(base, verbose=True))
        err, sys.stderr = sys.stderr, io.StringIO()
        try:
            ref.assemble.get_contributors(phy, obs, haps, wts, (props, mix), a)
            verbose_text = sys.stderr.getvalue()
        finally:
            sys.stderr = err
        n_cand, n_kept = len(cand), len(str(out["contribs_default"]).split("\n"))
        print("g16: %d candidates, %d kept by the default check" % (n_cand, n_kept), flush=True)
        assert n_kept >= 2 and n_cand - n_kept >= 1, (n_cand, n_kept)
        buf = io.StringIO()
        ref.stats.write_base_obs(buf, obs, refseq, prefix="s1")
        ancestral = {haps[c]: sorted(phy.get_ancestral(haps[c])) for c in cand}
        import json
        save("g16_observe", ref_start=cols.ref_start, mapq=cols.mapq, frag=cols.frag, cig_ptr=cols.cig_ptr,
             cigar=cols.cigar, seq_ptr=cols.seq_ptr, seq=cols.seq, qual=cols.qual, has_qual=cols.has_qual,
             is_reverse=cols.is_reverse, names=numpy.array("\n".join(cols.names)),
             seeds=numpy.array([G16_SEED, G16_EM_SEED]), min_reads=numpy.array(G16_MIN_READS),
             trip_pos=numpy.array([t[0] for t in trip], dtype=numpy.int64),
             trip_key=numpy.array("".join(t[1] for t in trip)),
             trip_count=numpy.array([t[2] for t in trip], dtype=numpy.int64),
             candidates=numpy.array(cand, dtype=numpy.int32), props=props, iters=iters,
             signatures=numpy.array("\n".join(rows)), weights=wts.astype(numpy.int64),
             base_obs=numpy.array(buf.getvalue()), verbose_text=numpy.array(verbose_text),
             ancestral=numpy.array(json.dumps(ancestral)), **out)

    if want("g17"):
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        import collections
        import json
        import tempfile
        import mixemt.assemble
        import mixemt.observe
        import mixemt.stats
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from _pileup_aln import PileupBam
        cols, alns = make_g16_alignments(refseq, tables)
        t0 = time.time()
        obs = ref.observe.ObservedBases(alns, mapq=30, baseq=30)
        read_obs = ref.preprocess.process_reads(alns, phy.get_variant_pos(), 30, 30)
        read_sigs = ref.preprocess.reduce_reads(read_obs)
        read_sigs.pop("", None)
        rows = sorted(read_sigs)
        reads = [read_sigs[r] for r in rows]
        wts = numpy.array([len(r) for r in reads])
        mat = ref.preprocess.build_em_matrix(refseq, phy, rows, haps, quiet)
        props, mix, iters, inits = ref_run_em(ref, mat, wts, G16_EM_SEED)
        print("g17: pileup + matrix %d x %d + run_em in %.0f s" % (mat.shape[0], mat.shape[1], time.time() - t0), flush=True)
        votes = collections.Counter()
        for r, h in enumerate(numpy.argmax(mix, 1)):
            votes[int(h)] += int(wts[r])
        top = sorted(votes.values(), reverse=True)
        one_min_reads = top[1] + 1                    # leaves the most voted candidate alone
        base = dict(min_reads=G16_MIN_READS, contributors=None, var_check=True, min_fold=2.0, min_var_reads=3,
                    frac_var_reads=0.02, var_fraction=0.5, var_count=None, min_mq=30, min_bq=30)
        cases = [("default", {}), ("unassigned", {"min_fold": 1e300}), ("one", {"min_reads": one_min_reads})]
        names_of = [cols.names[int(f)] for f in cols.frag]
        out = {}
        for label, kw in cases:
            a = ns(**dict(base, **kw))
            contribs = ref.assemble.get_contributors(phy, obs, haps, wts, (props, mix), a)
            sub, sub_haps = ref.preprocess.reduce_em_matrix(mat, haps, contribs)
            numpy.random.seed(G17_REFINE_SEED)
            res = ref.em.run_em(sub, wts, a)
            contribs = ref.assemble.update_contribs(contribs, res, sub_haps)
            contrib_reads = ref.assemble.assign_reads(PileupBam(alns), contribs, res, sub_haps, reads, a)
            report = io.StringIO()
            ref.stats.report_contributors(report, contribs, contrib_reads)
            with tempfile.TemporaryDirectory() as tmp:
                a.stats_prefix = os.path.join(tmp, "run")
                ref.stats.write_statistics(phy, obs, contribs, contrib_reads, a)
                with open(a.stats_prefix + ".pos.tab") as fin:
                    pos_tab = fin.read()
                with open(a.stats_prefix + ".obs.tab") as fin:
                    obs_tab = fin.read()
            keys = sorted(contrib_reads)
            key_of = {}
            for k, key in enumerate(keys):
                for aln in contrib_reads[key]:
                    key_of[id(aln)] = k
            aln_key = numpy.array([key_of.get(id(aln), -1) for aln in alns], dtype=numpy.int32)
            n_un = len(contrib_reads.get("unassigned", []))
            print("g17 %-10s: %d contributors, keys %s, %d alignments unassigned, %d in no table"
                  % (label, len(contribs), keys, n_un, int((aln_key < 0).sum())), flush=True)
            if label == "default":
                assert len(contribs) >= 2 and n_un > 0
            elif label == "unassigned":
                assert len(contribs) >= 2 and all(len(contrib_reads[c[0]]) == 0 for c in contribs)
            else:
                assert len(contribs) == 1 and "unassigned" not in contrib_reads
            out[label + "_contribs"] = numpy.array("\n".join("%s\t%s\t%r" % (c[0], c[1], float(c[2])) for c in contribs))
            out[label + "_args"] = numpy.array(json.dumps(kw))
            out[label + "_report"] = numpy.array(report.getvalue())
            out[label + "_pos_tab"] = numpy.array(pos_tab)
            out[label + "_obs_tab"] = numpy.array(obs_tab)
            out[label + "_keys"] = numpy.array("\n".join(keys))
            out[label + "_aln_key"] = aln_key
        # polymorphic_sites (phylotree.py:276-315) on the 9-haplogroup toy tree, reference all 'A' and one other
        toy = ref.phylotree.Phylotree(my_phy.example_rows())
        poly = {}
        for ref_seq in ("A" * 10, "AGTAAAAAAA"):
            for hs in (["A"], ["F", "G"], ["A", "C"], ["B", "C", "D", "E"], ["I"], ["H", "B", "E"], ["C", "C"]):
                poly["%s|%s" % (ref_seq, ",".join(hs))] = toy.polymorphic_sites(hs, ref_seq)
        out["toy_polymorphic"] = numpy.array(json.dumps(poly))
        save("g17_stats", seeds=numpy.array([G16_SEED, G16_EM_SEED, G17_REFINE_SEED]),
             columns_sha256=numpy.array(_columns_sha(cols)), **out)

    if want("g18"):
        for name in ("pysam", "Bio", "Bio.Seq", "Bio.SeqRecord", "Bio.SeqIO"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["Bio"].SeqIO = sys.modules["Bio.SeqIO"]
        sys.modules["Bio.Seq"].Seq = object
        sys.modules["Bio.SeqRecord"].SeqRecord = object
        import collections
        import json
        import pickle
        import tempfile
        import mixemt.assemble
        import mixemt.observe
        import mixemt.stats
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from _pileup_aln import PileupBam
        asm = ref.assemble
        cols, alns = make_g18_alignments(refseq, tables)
        cols_sha = _columns_sha(cols)
        t0 = time.time()
        obs = ref.observe.ObservedBases(alns, mapq=30, baseq=30)
        read_obs = ref.preprocess.process_reads(alns, phy.get_variant_pos(), 30, 30)
        read_sigs = ref.preprocess.reduce_reads(read_obs)
        read_sigs.pop("", None)
        rows = sorted(read_sigs)
        reads = [read_sigs[r] for r in rows]
        wts = numpy.array([len(r) for r in reads])
        cache = os.path.join(opts.cache, "g18_%s.pkl" % cols_sha[:16]) if opts.cache else ""
        if cache and os.path.exists(cache):
            with open(cache, "rb") as fin:
                mat, props, mix = pickle.load(fin)
        else:
            mat = ref.preprocess.build_em_matrix(refseq, phy, rows, haps, quiet)
            props, mix, _, _ = ref_run_em(ref, mat, wts, G16_EM_SEED)
            if cache:
                with open(cache, "wb") as fout:
                    pickle.dump((mat, props, mix), fout)
        print("g18: pileup + matrix %d x %d + run_em in %.0f s" % (mat.shape[0], mat.shape[1], time.time() - t0), flush=True)
        base = dict(min_reads=G16_MIN_READS, contributors=None, var_check=True, min_fold=2.0, min_var_reads=3,
                    frac_var_reads=0.02, var_fraction=0.5, var_count=None, min_mq=30, min_bq=30, cons_cov=G18_CONS_COV)
        cases = [("default", {}), ("nokeys", {"min_fold": 1e300}), ("nocall", {"cons_cov": 10 ** 6})]
        index_of = {id(aln): i for i, aln in enumerate(alns)}
        out = {}

        def folded(alns_of):
            """[ref_len][6] counts A C G T other gap of a list, N dropped (what consensus_base sees), and per position
            the folded keys in first-observed order."""
            tab = ref.observe.ObservedBases(alns_of, 30, 30) if alns_of else None
            cnt, first = [], []
            for pos in range(len(refseq)):
                c = tab.obs_at(pos) if tab is not None else {}
                keys = [k for k in c if k != "N" and c[k] > 0]
                first.append(keys)
                cnt.append([c.get(b, 0) for b in "ACGT"] + [sum(c[k] for k in keys if k not in "ACGT-"), c.get("-", 0)])
            return numpy.array(cnt, dtype=numpy.int64), first

        for label, kw in cases:
            a = ns(**dict(base, **kw))
            contribs = asm.get_contributors(phy, obs, haps, wts, (props, mix), a)
            sub, sub_haps = ref.preprocess.reduce_em_matrix(mat, haps, contribs)
            numpy.random.seed(G17_REFINE_SEED)
            res = ref.em.run_em(sub, wts, a)
            contribs = asm.update_contribs(contribs, res, sub_haps)
            contrib_reads = asm.assign_reads(PileupBam(alns), contribs, res, sub_haps, reads, a)
            names = [c[0] for c in contribs]
            start_key = {id(aln): key for key in contrib_reads for aln in contrib_reads[key]}
            strict_before = {key: asm.call_consensus(refseq, contrib_reads[key], a.cons_cov, a, strict=True)
                             for key in list(contrib_reads)}
            # the reference's own loop, with its two steps recorded as they run
            rounds, dicts, moved_ids = [], [], []
            real_find, real_assign = asm.find_new_variants, asm.assign_reads_from_new_vars

            def rec_find(refseq_, cr, args_):
                got = real_find(refseq_, cr, args_)
                dicts.append(dict(got))
                return got

            def rec_assign(cr, new_variants, args_):
                before = [id(x) for x in cr["unassigned"]]
                cr = real_assign(cr, new_variants, args_)
                after = set(id(x) for x in cr["unassigned"])
                moved_ids.append([i for i in before if i not in after])
                rounds.append((len(before) - len(after), len(before), len(new_variants)))
                return cr

            a.verbose = True
            err, sys.stderr = sys.stderr, io.StringIO()
            asm.find_new_variants, asm.assign_reads_from_new_vars = rec_find, rec_assign
            try:
                contrib_reads = asm.extend_assemblies(refseq, contrib_reads, a)
                verbose_text = sys.stderr.getvalue()
            finally:
                sys.stderr = err
                asm.find_new_variants, asm.assign_reads_from_new_vars = real_find, real_assign
            a.verbose = False
            keys_after_extend = list(contrib_reads)
            strict_after = {key: asm.call_consensus(refseq, contrib_reads[key], a.cons_cov, a, strict=True)
                            for key in keys_after_extend}
            strict2_after = {key: asm.call_consensus(refseq, contrib_reads[key], 2, a, strict=True)
                             for key in keys_after_extend}
            loose_after = {key: asm.call_consensus(refseq, contrib_reads[key], 1, a, strict=False)
                           for key in keys_after_extend}
            report = io.StringIO()
            ref.stats.report_contributors(report, contribs, contrib_reads)
            with tempfile.TemporaryDirectory() as tmp:
                a.stats_prefix = os.path.join(tmp, "run")
                ref.stats.write_statistics(phy, obs, contribs, contrib_reads, a)
                with open(a.stats_prefix + ".pos.tab") as fin:
                    pos_tab = fin.read()
                with open(a.stats_prefix + ".obs.tab") as fin:
                    obs_tab = fin.read()
            keys = sorted(contrib_reads)
            key_of = {}
            for k, key in enumerate(keys):
                for aln in contrib_reads[key]:
                    key_of[id(aln)] = k
            aln_key = numpy.array([key_of.get(id(aln), -1) for aln in alns], dtype=numpy.int32)
            aln_round = numpy.zeros(len(alns), dtype=numpy.int32)
            for r, ids in enumerate(moved_ids):
                aln_round[[index_of[i] for i in ids]] = r + 1
            print("g18 %-8s: %d contributors, rounds (moved, unassigned, variants) %s" % (label, len(contribs), rounds), flush=True)

            if label == "default":
                assert len(contribs) >= 2
                moving = [r for r in rounds if r[0] > 0]
                assert len(moving) >= 2 and sum(r[0] for r in rounds) >= 50, rounds
                assert rounds[-1][0] == 0
                # a moved alignment below min_mq, or the mate of the one that showed the variant
                moved = numpy.flatnonzero(aln_round > 0)
                low = [i for i in moved if alns[i].mapping_quality < a.min_mq]
                print("g18: %d alignments moved, %d of them below min_mq" % (len(moved), len(low)), flush=True)
                assert low
                # a fragment that saw two owners in round 1: re-walk the first round's unassigned list
                seen = collections.defaultdict(set)
                first_un = [x for x in alns if start_key.get(id(x)) == "unassigned"]
                for aln in first_un:
                    if aln.mapping_quality >= a.min_mq:
                        for qpos, rpos in aln.get_aligned_pairs(matches_only=True):
                            if aln.query_qualities is None or aln.query_qualities[qpos] >= a.min_bq:
                                hit = dicts[0].get((rpos, aln.query_sequence[qpos].upper()))
                                if hit is not None:
                                    seen[aln.query_name].add(hit)
                n_conflict = sum(1 for v in seen.values() if len(v) > 1)
                print("g18: %d fragments with two owners in round 1" % n_conflict, flush=True)
                assert n_conflict >= 1
                # ties of the non-strict consensus, their winners, gaps
                n_tie = n_not_first = n_rev_first = n_gap = n_gap_lift = 0
                for key in keys_after_extend:
                    lst = contrib_reads[key]
                    if not lst:
                        continue
                    cnt, first = folded(lst)
                    stranded = ref.observe.ObservedBases(lst, 30, 30)
                    cons, cons2 = loose_after[key], strict2_after[key]
                    for pos in range(len(refseq)):
                        assert cons[pos] in "ACGTN-" and strict_after[key][pos] in "ACGTN-", (key, pos, cons[pos])
                        c = cnt[pos]
                        assert c[4] == 0, (key, pos)               # no character outside ACGTN- is observed at all
                        if cons[pos] == "-":
                            n_gap += 1
                        if cons2[pos] == "-" and c[:5].sum() < 2:
                            n_gap_lift += 1
                        top = c.max()
                        if top > 0 and (c == top).sum() > 1:
                            n_tie += 1
                            tied = [b for b, v in zip("ACGTX-", c) if v == top]
                            assert cons[pos] in tied
                            if cons[pos] != sorted(tied)[0]:
                                n_not_first += 1
                            raw = list(stranded.obs_tab[pos])      # stranded keys in the order they were first observed
                            lead = [k for k in raw if k.upper() in tied or (k == "+" and "-" in tied)]
                            if lead and (lead[0].islower() or lead[0] == "+"):
                                n_rev_first += 1
                print("g18: %d tied positions, %d won by a base that is not the alphabetically first, %d first seen on the "
                      "reverse strand; %d gap calls, %d where gaps make the coverage" % (n_tie, n_not_first, n_rev_first, n_gap,
                                                                                      n_gap_lift), flush=True)
                assert n_tie >= 5 and n_not_first >= 1 and n_rev_first >= 1 and n_gap >= 1 and n_gap_lift >= 1
            elif label == "nokeys":
                assert len(contribs) >= 2 and dicts == [{}] and rounds[0][0] == 0 and len(rounds) == 1
            else:
                assert all(len(d) == 0 for d in dicts) and len(rounds) == 1 and rounds[0][0] == 0

            out[label + "_contribs"] = numpy.array("\n".join("%s\t%s\t%r" % (c[0], c[1], float(c[2])) for c in contribs))
            out[label + "_args"] = numpy.array(json.dumps(dict(kw, cons_cov=a.cons_cov)))
            out[label + "_rounds"] = numpy.array(rounds, dtype=numpy.int64).reshape(-1, 3)
            for r, d in enumerate(dicts):
                items = sorted(d.items())
                out["%s_nv%d_pos" % (label, r)] = numpy.array([k[0] for k, _ in items], dtype=numpy.int64)
                out["%s_nv%d_base" % (label, r)] = numpy.array("".join(k[1] for k, _ in items))
                out["%s_nv%d_own" % (label, r)] = numpy.array([names.index(v) for _, v in items], dtype=numpy.int32)
            out[label + "_start_keys"] = numpy.array("\n".join(strict_before))
            out[label + "_start_key"] = numpy.array([list(strict_before).index(start_key[id(x)]) if id(x) in start_key else -1
                                                     for x in alns], dtype=numpy.int32)
            out[label + "_extend_keys"] = numpy.array("\n".join(keys_after_extend))
            out[label + "_keys"] = numpy.array("\n".join(keys))
            out[label + "_aln_key"] = aln_key
            out[label + "_aln_round"] = aln_round
            out[label + "_strict_before"] = numpy.array(json.dumps(strict_before))
            out[label + "_strict_after"] = numpy.array(json.dumps(strict_after))
            out[label + "_strict2_after"] = numpy.array(json.dumps(strict2_after))
            out[label + "_loose_after"] = numpy.array(json.dumps(loose_after))
            out[label + "_verbose"] = numpy.array(verbose_text)
            out[label + "_report"] = numpy.array(report.getvalue())
            if label == "default":
                out[label + "_pos_tab"] = numpy.array(pos_tab)
                out[label + "_obs_tab"] = numpy.array(obs_tab)
        trip = [(pos, key, cnt) for pos in sorted(obs.obs_tab) for key, cnt in sorted(obs.obs_tab[pos].items())]
        save("g18_assemble", seeds=numpy.array([G18_SEED, G16_EM_SEED, G17_REFINE_SEED]),
             columns_sha256=numpy.array(cols_sha), n_aln=numpy.array(len(cols)),
             trip_pos=numpy.array([t[0] for t in trip], dtype=numpy.int64),
             trip_key=numpy.array("".join(t[1] for t in trip)),
             trip_count=numpy.array([t[2] for t in trip], dtype=numpy.int64),
             signatures_sha256=numpy.array(hashlib.sha256("\n".join(rows).encode()).hexdigest()),
             props=props, **out)

    if want("g7"):
        cols = list(range(0, 5400, 54))
        sub_haps = [haps[c] for c in cols]
        contrib = (cols[10], cols[40], cols[80])
        row_ptr, site, obs, who = synth.synth_reads(tables, len(refseq), 1000, seed=1,
                                                    contrib=contrib)
        sigs = synth.signatures(tables, row_ptr, site, obs)
        mat = ref.preprocess.build_em_matrix(refseq, phy, sigs, sub_haps, quiet)
        wts = numpy.ones(1000, dtype=numpy.int64)
        props, mix, iters, inits = ref_run_em(ref, mat, wts, 7)
        save("g7_config1", cols=numpy.array(cols, dtype=numpy.int32), row_ptr=row_ptr, site=site,
             obs=obs, who=who, mat=mat, props=props, iters=iters, inits=inits, mix=mix)


if __name__ == "__main__":
    main()
