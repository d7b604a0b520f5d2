"""
A vectorised numpy restatement of the pileup (mxm_observe_bases, observe.py:56-86), written from its semantics: every
reference position an M / = / X or D / N operation of a counted alignment (mapq >= min_mq, ref_start >= 0) covers gets one
count in counts[L][16] -- bins 0-6 forward A C G T N other '-', 7-13 reverse.  A base below min_bq (when the alignment
has qualities) counts as N; letters are upper-cased.  Assumes CIGARs the library accepts.
"""
import numpy

_BIN = numpy.full(256, 5, dtype=numpy.int64)
for _i, _c in enumerate("ACGTN"):
    _BIN[ord(_c)] = _BIN[ord(_c.lower())] = _i


def pileup(cols, L, min_mq=30, min_bq=30):
    n = len(cols)
    counts = numpy.zeros((L, 16), dtype=numpy.int64)
    if not n or not len(cols.cigar):
        return counts
    n_ops = numpy.diff(cols.cig_ptr)
    own = numpy.repeat(numpy.arange(n), n_ops)                 # alignment of every CIGAR op
    op = (cols.cigar & 15).astype(numpy.int64)
    ln = (cols.cigar >> 4).astype(numpy.int64)
    qadv = numpy.where(numpy.isin(op, (0, 1, 4, 7, 8)), ln, 0)
    radv = numpy.where(numpy.isin(op, (0, 2, 3, 7, 8)), ln, 0)

    def start_of(adv):                                          # exclusive prefix of adv within each alignment
        cum = numpy.cumsum(adv) - adv
        return cum - (numpy.cumsum(adv) - adv)[cols.cig_ptr[:-1]][own]

    q0 = start_of(qadv)
    r0 = cols.ref_start[own] + start_of(radv)
    keep = (cols.mapq[own] >= min_mq) & (cols.ref_start[own] >= 0) & (radv > 0)
    k = numpy.flatnonzero(keep)
    cnt = ln[k]
    seg = numpy.repeat(k, cnt)                                  # one entry per covered reference position
    off = numpy.arange(int(cnt.sum())) - numpy.repeat(numpy.cumsum(cnt) - cnt, cnt)
    rpos = r0[seg] + off
    match = op[seg] != 2
    match &= op[seg] != 3
    bins = numpy.full(len(seg), 6, dtype=numpy.int64)
    a = own[seg]
    qp = cols.seq_ptr[a] + q0[seg] + off
    qm = qp[match]
    b = _BIN[cols.seq[qm]]
    if cols.qual is not None:
        hq = numpy.ones(n, dtype=bool) if cols.has_qual is None else cols.has_qual.astype(bool)
        low = hq[a[match]] & (cols.qual[qm] < min_bq)
        b[low] = 4
    bins[match] = b
    if getattr(cols, "is_reverse", None) is not None:
        bins += 7 * cols.is_reverse[a].astype(numpy.int64)
    numpy.add.at(counts, (rpos, bins), 1)
    return counts


def from_triplets(pos, keys, count, L):
    """
    The reference's obs_tab as (pos, key, count) triplets -> counts[L][16].  Its keys carry the strand by their case; a
    character without case (say '*') is the same key on both strands and is taken as forward here (g16 has one only on
    a forward alignment).
    """
    counts = numpy.zeros((L, 16), dtype=numpy.int64)
    fwd = {c: i for i, c in enumerate("ACGTN")}
    for p, key, c in zip(pos, keys, count):
        if key == "-":
            b = 6
        elif key == "+":
            b = 13
        elif key in fwd:
            b = fwd[key]
        elif key.upper() in fwd:
            b = fwd[key.upper()] + 7
        else:
            b = 12 if key.islower() else 5
        counts[int(p), b] += int(c)
    return counts
