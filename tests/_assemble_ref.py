"""
A plain numpy restatement of mixemt's assembly stage (call_consensus, find_new_variants, assign_reads_from_new_vars,
extend_assemblies; the reference's assemble.py:431-585) over alignments.AlignmentColumns and one label per alignment,
written from the rules, for the tests of mixemt_amd.assemble:

  - a contributor's list is its alignments in (joined, index) order: assign_reads' in file order, then what each
    extension round appended;
  - consensus: strands folded, N observations dropped, total = A + C + G + T + other + gap; below min_cov 'N'; strict: the
    only observed character or 'N'; not strict: the most observed one, among equals the one observed first in the list;
    "" for a list without alignments; 'X' stands for a character other than ACGTN;
  - new variants: over the keys other than 'unassigned'; none when there is no such key or one of them has no alignment;
    a position is skipped when any of their strict consensus characters is not one of ACGT; a base is a new variant of
    the one contributor that has it;
  - assignment: unassigned alignments with mapq >= min_mq, bases under M / = / X with quality >= min_bq (or no
    qualities), upper-cased, looked up; a fragment with hits of exactly one contributor moves with all its unassigned
    alignments.
"""
import sys

import numpy

CHARS = "ACGTNX-"
_BIN = numpy.full(256, 5, dtype=numpy.int64)
for _i, _c in enumerate("ACGTN"):
    _BIN[ord(_c)] = _BIN[ord(_c.lower())] = _i


def observations(cols, idx, min_mq=30, min_bq=30):
    """(rpos, folded bin 0-6, alignment, is_base, passes) of every observation of the alignments idx that the pileup
    counts: bin 4 = N (a base below min_bq), 6 = gap; passes = a base whose quality is fine (or without qualities)."""
    idx = numpy.asarray(idx, dtype=numpy.int64)
    idx = idx[(cols.mapq[idx] >= min_mq) & (cols.ref_start[idx] >= 0)]
    empty = numpy.zeros(0, dtype=numpy.int64)
    if not len(idx):
        return empty, empty, empty, empty.astype(bool), empty.astype(bool)
    n_ops = (cols.cig_ptr[idx + 1] - cols.cig_ptr[idx]).astype(numpy.int64)
    own = numpy.repeat(numpy.arange(len(idx)), n_ops)
    first_op = numpy.cumsum(n_ops) - n_ops
    k = numpy.repeat(cols.cig_ptr[idx], n_ops) + numpy.arange(int(n_ops.sum())) - numpy.repeat(first_op, n_ops)
    op = (cols.cigar[k] & 15).astype(numpy.int64)
    ln = (cols.cigar[k] >> 4).astype(numpy.int64)
    qadv = numpy.where(numpy.isin(op, (0, 1, 4, 7, 8)), ln, 0)
    radv = numpy.where(numpy.isin(op, (0, 2, 3, 7, 8)), ln, 0)

    def start_of(adv):
        cum = numpy.cumsum(adv) - adv
        return cum - cum[first_op][own]

    q0 = start_of(qadv)
    r0 = cols.ref_start[idx][own] + start_of(radv)
    keep = numpy.flatnonzero(radv > 0)
    cnt = ln[keep]
    seg = numpy.repeat(keep, cnt)
    off = numpy.arange(int(cnt.sum())) - numpy.repeat(numpy.cumsum(cnt) - cnt, cnt)
    rpos = r0[seg] + off
    is_base = (op[seg] != 2) & (op[seg] != 3)
    aln = idx[own[seg]]
    bins = numpy.full(len(seg), 6, dtype=numpy.int64)
    qp = (cols.seq_ptr[aln] + q0[seg] + off)[is_base]
    b = _BIN[cols.seq[qp]]
    ok = numpy.ones(len(qp), dtype=bool)
    if cols.qual is not None:
        hq = numpy.ones(len(cols), dtype=bool) if cols.has_qual is None else cols.has_qual.astype(bool)
        ok = ~(hq[aln[is_base]] & (cols.qual[qp] < min_bq))
    b[~ok] = 4
    bins[is_base] = b
    passes = numpy.zeros(len(seg), dtype=bool)
    passes[is_base] = ok
    return rpos, bins, aln, is_base, passes


def consensus(cols, idx, joined, ref_len, min_cov, min_mq=30, min_bq=30, strict=True):
    """call_consensus of the list idx (alignment indexes; order (joined, index))."""
    idx = numpy.asarray(idx, dtype=numpy.int64)
    if not len(idx):
        return ""
    rpos, bins, aln, _, _ = observations(cols, idx, min_mq, min_bq)
    inside = rpos < ref_len
    rpos, bins, aln = rpos[inside], bins[inside], aln[inside]
    cnt = numpy.zeros((ref_len, 7), dtype=numpy.int64)
    numpy.add.at(cnt, (rpos, bins), 1)
    cnt[:, 4] = 0
    total = cnt.sum(axis=1)
    best = cnt.max(axis=1)
    pick = cnt.argmax(axis=1)
    called = (total > 0) & (total >= min_cov)
    out = numpy.full(ref_len, ord("N"), dtype=numpy.uint8)
    chars = numpy.frombuffer(CHARS.encode(), dtype=numpy.uint8)
    if strict:
        ok = called & (best == total)
        out[ok] = chars[pick[ok]]
        return out.tobytes().decode()
    out[called] = chars[pick[called]]
    tied = numpy.flatnonzero(called & ((cnt == best[:, None]).sum(axis=1) > 1))
    if len(tied):
        order = numpy.lexsort((aln, joined[aln]))                  # the list's order; stable within an alignment
        rp, bn = rpos[order], bins[order]
        at = numpy.isin(rp, tied)
        rp, bn = rp[at], bn[at]
        for pos in tied:
            cand = bn[rp == pos]
            cand = cand[(cand != 4) & (cnt[pos, cand] == best[pos])]
            out[pos] = chars[cand[0]]
    return out.tobytes().decode()


class Table(object):
    """The reference's contrib_reads as labels: names[label], keys in order, label[n_aln] (-1 in no list), joined."""

    def __init__(self, cols, label, names, keys, joined=None):
        self.cols = cols
        self.label = numpy.array(label, dtype=numpy.int64)
        self.names = list(names)
        self.keys = list(keys)
        self.joined = numpy.zeros(len(self.label), dtype=numpy.int64) if joined is None else numpy.array(joined)
        self.rounds = 0

    def rows(self, name):
        if name not in self.names:
            return numpy.zeros(0, dtype=numpy.int64)
        return numpy.flatnonzero(self.label == self.names.index(name))

    def lookup(self, name):
        if name not in self.keys:
            self.keys.append(name)
        return self.rows(name)


def call_consensus(refseq, table, name, min_cov, args, strict=True):
    return consensus(table.cols, table.lookup(name), table.joined, len(refseq), min_cov, args.min_mq, args.min_bq, strict)


def find_new_variants(refseq, table, args):
    names = [k for k in table.keys if k != "unassigned"]
    cons = {k: call_consensus(refseq, table, k, int(args.cons_cov), args, True) for k in names}
    if not cons or min(len(c) for c in cons.values()) == 0:
        return {}
    mat = numpy.array([numpy.frombuffer(cons[k].encode(), dtype=numpy.uint8) for k in names])
    out = {}
    good = numpy.flatnonzero(numpy.isin(mat, numpy.frombuffer(b"ACGT", dtype=numpy.uint8)).all(axis=0))
    for pos in good:
        col = mat[:, pos]
        for k, name in enumerate(names):
            if (col == col[k]).sum() == 1:
                out[(int(pos), chr(col[k]))] = name
    return out


def assign_reads_from_new_vars(table, new_variants, args):
    cols = table.cols
    table.lookup("unassigned")
    table.rounds += 1
    if "unassigned" not in table.names or not new_variants:
        return 0
    un = table.names.index("unassigned")
    owners = sorted(set(new_variants.values()), key=table.names.index)
    n_pos = max(p for p, _ in new_variants) + 1
    newvar = numpy.full((n_pos, 4), -1, dtype=numpy.int64)
    for (pos, base), name in new_variants.items():
        if base in "ACGT":
            newvar[pos, "ACGT".index(base)] = owners.index(name)
    idx = numpy.flatnonzero(table.label == un)
    rpos, bins, aln, is_base, passes = observations(cols, idx, args.min_mq, args.min_bq)
    sel = is_base & passes & (bins < 4) & (rpos < n_pos)
    own = newvar[rpos[sel], bins[sel]]
    hit = own >= 0
    frag = cols.frag[aln[sel][hit]]
    own = own[hit]
    n_frag = int(cols.frag.max()) + 1 if len(cols) else 0
    lo = numpy.full(n_frag, len(owners), dtype=numpy.int64)
    hi = numpy.full(n_frag, -1, dtype=numpy.int64)
    numpy.minimum.at(lo, frag, own)
    numpy.maximum.at(hi, frag, own)
    one = (hi >= 0) & (lo == hi)
    move = idx[one[cols.frag[idx]]]
    table.label[move] = [table.names.index(owners[k]) for k in lo[cols.frag[move]]]
    table.joined[move] = table.rounds
    return len(move)


def extend_assemblies(refseq, table, args, record=None):
    """The loop of assemble.py:549-585; record (a list) gets (moved, unassigned before, n_new_vars, dict) per round."""
    table.lookup("unassigned")
    last, unassigned, run = None, len(table.rows("unassigned")), 1
    if args.verbose:
        sys.stderr.write("\nAssembly extension step...\n")
    while last != unassigned:
        new_variants = find_new_variants(refseq, table, args)
        moved = assign_reads_from_new_vars(table, new_variants, args)
        last, unassigned = unassigned, unassigned - moved
        if record is not None:
            record.append((moved, last, len(new_variants), new_variants))
        if args.verbose:
            sys.stderr.write("  %d: %d/%d reads assigned using %d variants\n" % (run, last - unassigned, last, len(new_variants)))
        run += 1
    if args.verbose:
        sys.stderr.write("\n")
    return table
