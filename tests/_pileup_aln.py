"""
Stand-in for pysam.AlignedSegment for the pileup (g16): get_aligned_pairs in both forms and is_reverse, over the
alignments of an alignments.AlignmentColumns (pysam is not installed here; tests/_fake_aln.py stays the front end's).

get_aligned_pairs(matches_only=False) is modelled on pysam's: M / = / X give (qpos, rpos), I and S (qpos, None),
D and N (None, rpos) -- pysam emits the reference-skip positions too when matches_only is False --, H and P nothing.
An unplaced alignment (reference_start < 0) has no aligned pairs.
"""

_OPS = "MIDNSHP=XB"


class PileupAln(object):
    def __init__(self, name, start, mq, seq, quals, cigartuples, is_reverse):
        self.query_name = name
        self.reference_start = start
        self.mapping_quality = mq
        self.query_sequence = seq
        self.query_qualities = quals
        self.cigartuples = cigartuples
        self.cigarstring = "".join("%d%s" % (n, _OPS[op]) for op, n in cigartuples)
        self.is_reverse = bool(is_reverse)

    def get_aligned_pairs(self, matches_only=False):
        pairs = []
        if self.reference_start is None or self.reference_start < 0:
            return pairs
        q, r = 0, self.reference_start
        for op, n in self.cigartuples:
            if op in (0, 7, 8):
                pairs.extend((q + i, r + i) for i in range(n))
                q += n
                r += n
            elif op in (1, 4):
                if not matches_only:
                    pairs.extend((q + i, None) for i in range(n))
                q += n
            elif op in (2, 3):
                if not matches_only:
                    pairs.extend((None, r + i) for i in range(n))
                r += n
        return pairs


class PileupBam(object):
    def __init__(self, alns):
        self.alns = list(alns)

    def fetch(self):
        return iter(self.alns)


def from_columns(cols):
    """alignments.AlignmentColumns -> list of PileupAln (strands from cols.is_reverse; None = forward)."""
    out = []
    for i in range(len(cols)):
        a, b = int(cols.seq_ptr[i]), int(cols.seq_ptr[i + 1])
        quals = None
        if cols.qual is not None and (cols.has_qual is None or cols.has_qual[i]):
            quals = cols.qual[a:b].tolist()
        cig = [(int(c) & 15, int(c) >> 4) for c in cols.cigar[int(cols.cig_ptr[i]):int(cols.cig_ptr[i + 1])]]
        rev = cols.is_reverse is not None and bool(cols.is_reverse[i])
        out.append(PileupAln(cols.names[int(cols.frag[i])], int(cols.ref_start[i]), int(cols.mapq[i]),
                             cols.seq[a:b].tobytes().decode("ascii"), quals, cig, rev))
    return out
