"""
The pileup of mixemt's variant check -- observe.ObservedBases (the reference's mixemt/observe.py), counted on the device:

    obs = observe_bases(cols, min_mq=30, min_bq=30, ref_len=len(refseq))     # cols: alignments.AlignmentColumns
    obs.counts                  uint32 [L][16]: per position the bins of mxm_observe_bases (BINS below)
    obs.obs_at(pos, base=None, stranded=False), obs.total_obs(pos)            the reference's queries (observe.py:88-145)
    obs.obs_tab[pos]            a Counter of the position's observations, as the reference's attribute holds them
    count_bases_labelled(dcols, label, counts)     one table per label in one call (stats.write_statistics' tables)
    observe_bases_many(cols_list, ...)             the pileups of a cohort's samples in one upload and one labelled call:
                                                   a CohortPileup whose tables stay on the device (assign.finish_many)

The reference walks pysam's get_aligned_pairs(matches_only=False) one tuple at a time (observe.py:56-86); here one
library call (mxm_observe_bases, csrc/observe_kernels.hpp) counts every alignment's bases and gaps into the table.
A character other than ACGTN is counted in the `other` bin of its strand: the reference keys it by the character itself;
here it appears as 'X' (forward) / 'x' (reverse) in obs_at(pos) and obs_tab, and in write_base_obs' totals.
A consensus (assemble.call_consensus) that such a character wins is 'X' too, and assemble.find_new_variants skips a
position where a participating consensus is 'X': no read's real character could be looked up under it.
"""

import collections
import collections.abc
import ctypes
import warnings

import numpy

from . import _lib
from ._dev import current_stream, require_gpu, torch

# bins of a row of the table: forward, then reverse, then two pad bins
BINS = "ACGTNX-acgtnx+"
_FWD = {c: i for i, c in enumerate("ACGTNX-")}


def pileup_length(cols, min_mq=30, ref_len=None):
    """L = max(ref_len, the largest reference end of an alignment that is counted), from the CIGARs on the host."""
    n = len(cols)
    end = 0
    if n:
        ops = cols.cigar & 15
        lens = (cols.cigar >> 4).astype(numpy.int64)
        lens[(ops != 0) & (ops != 2) & (ops != 3) & (ops != 7) & (ops != 8)] = 0      # ops that advance the reference
        cum = numpy.zeros(len(lens) + 1, dtype=numpy.int64)
        numpy.cumsum(lens, out=cum[1:])
        span = cum[cols.cig_ptr[1:]] - cum[cols.cig_ptr[:-1]]
        use = (cols.mapq >= min_mq) & (cols.ref_start >= 0)
        if use.any():
            end = int((cols.ref_start[use] + span[use]).max())
    return max(int(ref_len or 0), end)


class DeviceColumns(object):
    """AlignmentColumns uploaded for mxm_observe_bases (.upload_s: the host -> device copy's time)."""

    def __init__(self, cols, dev=None):
        import time
        dev = dev or require_gpu()
        t0 = time.perf_counter()

        def up(arr, dtype, view=None):
            if arr is None:
                return None
            arr = numpy.ascontiguousarray(arr, dtype=dtype)
            if view is not None:
                arr = arr.view(view)
            if arr.size == 0:
                arr = numpy.zeros(1, dtype=arr.dtype)               # (the ABI wants a pointer even when empty)
            with warnings.catch_warnings():                         # read_bam's columns are read-only views
                warnings.simplefilter("ignore", UserWarning)
                return torch.from_numpy(arr).to(dev)

        self.n_aln = len(cols)
        self.ref_start = up(cols.ref_start, numpy.int64)
        self.mapq = up(cols.mapq, numpy.int32)
        self.cig_ptr = up(cols.cig_ptr, numpy.int64)
        self.cigar = up(cols.cigar, numpy.uint32, numpy.int32)
        self.seq_ptr = up(cols.seq_ptr, numpy.int64)
        self.seq = up(cols.seq, numpy.uint8)
        self.qual = up(cols.qual, numpy.uint8)
        self.has_qual = up(cols.has_qual, numpy.uint8)
        self.is_reverse = up(getattr(cols, "is_reverse", None), numpy.uint8)
        torch.cuda.synchronize()
        self.upload_s = time.perf_counter() - t0

    def struct(self):
        def p(t):
            return None if t is None else t.data_ptr()

        return _lib.AlnColumns(self.n_aln, 0, p(self.ref_start), p(self.mapq), None, p(self.cig_ptr), p(self.cigar),
                               p(self.seq_ptr), p(self.seq), p(self.qual), p(self.has_qual))


def count_bases(dcols, counts, min_mq=30, min_bq=30):
    """
    mxm_observe_bases: add the pileup of the uploaded columns `dcols` to `counts` (a zeroed or earlier-filled int32
    device tensor [L][16]).  Raises ValueError with the library's message (a CIGAR that runs past its sequence or holds
    an unknown operation; an alignment past the table).
    """
    if counts.dim() != 2 or counts.shape[1] != 16 or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 [L][16] device tensor")
    lib = _lib.load()
    st = dcols.struct()
    rev = 0 if dcols.is_reverse is None else dcols.is_reverse.data_ptr()
    _lib.check(lib.mxm_observe_bases(ctypes.byref(st), rev, int(min_mq), int(min_bq), int(counts.shape[0]),
                                     counts.data_ptr(), current_stream()), "mxm_observe_bases")
    return counts


def count_bases_labelled(dcols, label, counts, min_mq=30, min_bq=30):
    """
    mxm_observe_bases_labelled: add each label's pileup to its table in ONE call -- alignment i with label[i] in
    [0, n_labels) into counts[label[i]], label[i] < 0 not counted.  label: int32 device tensor [n_aln]; counts: a zeroed
    or earlier-filled contiguous int32 device tensor [n_labels][L][16].  Raises ValueError with the library's message
    (as count_bases, and for a label >= n_labels).
    """
    if counts.dim() != 3 or counts.shape[2] != 16 or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 [n_labels][L][16] device tensor")
    if label.dtype != torch.int32 or label.dim() != 1 or not label.is_contiguous() or label.numel() < dcols.n_aln:
        raise ValueError("label must be a contiguous int32 device tensor with one entry per alignment")
    lib = _lib.load()
    st = dcols.struct()
    rev = 0 if dcols.is_reverse is None else dcols.is_reverse.data_ptr()
    _lib.check(lib.mxm_observe_bases_labelled(ctypes.byref(st), rev, label.data_ptr(), int(counts.shape[0]), int(min_mq),
                                              int(min_bq), int(counts.shape[1]), counts.data_ptr(), current_stream()),
               "mxm_observe_bases_labelled")
    return counts


def observe_bases(cols, min_mq=30, min_bq=30, ref_len=None):
    """ObservedBases(alns, mapq=min_mq, baseq=min_bq) of the reference for alignments held as columns."""
    dev = require_gpu()
    L = pileup_length(cols, min_mq, ref_len)
    dcols = DeviceColumns(cols, dev)
    counts = torch.zeros((L, 16), dtype=torch.int32, device=dev)
    count_bases(dcols, counts, min_mq, min_bq)
    obs = ObservedBases(counts.cpu().numpy().view(numpy.uint32), min_mq, min_bq)
    obs.upload_s = dcols.upload_s
    return obs


COHORT_PILEUP_BYTES = 1 << 30        # observe_bases_many's default budget for the [S][L][16] table


class CohortPileup(object):
    """
    The pileups of a cohort's samples in ONE device tensor (observe_bases_many):
        counts            int32 device tensor [S][L][16] in the bins of BINS; nothing is downloaded unless asked
        n_samples, L, min_map_qual, min_base_qual
        lengths           the samples' own pileup_length: rows of counts[s] past lengths[s] are zero
        host(s)           an ObservedBases over a host copy of table s (downloaded on first use, cached): every query
                          answers as observe_bases(cols_list[s]) does -- a position past the sample's own length has no
                          observations in either
        cols, dcols, aln0 None, or with observe_bases_many(keep_columns=True) the concatenated AlignmentColumns, their
                          DeviceColumns and the samples' first alignments (alignments.concat_columns): the upload kept for
                          assign.assign_reads_many
    """

    def __init__(self, counts, lengths, min_mq=30, min_bq=30):
        self.counts = counts
        self.n_samples, self.L = int(counts.shape[0]), int(counts.shape[1])
        self.lengths = [int(n) for n in lengths]
        self.min_map_qual, self.min_base_qual = min_mq, min_bq
        self.upload_s = 0.0
        self.cols = self.dcols = self.aln0 = None
        self._host = {}

    def __len__(self):
        return self.n_samples

    def host(self, s):
        s = int(s)
        if not 0 <= s < self.n_samples:
            raise IndexError("sample index out of range")
        got = self._host.get(s)
        if got is None:
            table = self.counts[s, :self.lengths[s]].cpu().numpy().view(numpy.uint32)
            got = self._host[s] = ObservedBases(table, self.min_map_qual, self.min_base_qual)
        return got


def observe_bases_many(cols_list, min_mq=30, min_bq=30, ref_len=None, max_bytes=COHORT_PILEUP_BYTES, keep_columns=False):
    """
    observe_bases for the samples of a cohort in one upload and ONE labelled pileup call (the label of an alignment is
    its sample): -> CohortPileup with counts [S][L][16], L = the largest pileup_length among the samples.  The table takes
    S * L * 64 bytes (272 MB for 256 samples at L = 16 589); above max_bytes (default 1 GiB) this raises ValueError and
    the caller splits the cohort -- nothing is chunked silently.
    keep_columns: the returned pileup also carries the concatenated columns, their upload and aln0 (CohortPileup.cols /
    .dcols / .aln0), so that assign.assign_reads_many does not upload again; by default the upload is freed with the call.
    """
    from .alignments import concat_columns
    cols_list = list(cols_list)
    if not cols_list:
        raise ValueError("observe_bases_many: no samples")
    lengths = [pileup_length(cols, min_mq, ref_len) for cols in cols_list]
    n, L = len(cols_list), max(lengths)
    need = n * L * 64
    if need > int(max_bytes):
        raise ValueError("observe_bases_many: %d samples x %d positions need %d bytes of pileup tables, above the budget of "
                         "%d bytes (max_bytes): split the cohort" % (n, L, need, int(max_bytes)))
    dev = require_gpu()
    joined, aln0 = concat_columns(cols_list)
    dcols = DeviceColumns(joined, dev)
    label = torch.from_numpy(numpy.repeat(numpy.arange(n, dtype=numpy.int32), numpy.diff(aln0))).to(dev)
    counts = torch.zeros((n, L, 16), dtype=torch.int32, device=dev)
    if len(joined) and L:
        count_bases_labelled(dcols, label, counts, min_mq, min_bq)
    pileup = CohortPileup(counts, lengths, min_mq, min_bq)
    pileup.upload_s = dcols.upload_s
    if keep_columns:
        pileup.cols, pileup.dcols, pileup.aln0 = joined, dcols, aln0
    return pileup


class ObservedBases(object):
    """
    The reference's ObservedBases over a counted table (observe.py:16-145): counts[L][16] uint32 in the bins of BINS.
    Positions past the table have no observations.
    """

    def __init__(self, counts, mapq=30, baseq=30):
        self.counts = numpy.asarray(counts)
        if self.counts.ndim != 2 or self.counts.shape[1] != 16:
            raise ValueError("counts must be [L][16]")
        self.min_map_qual = mapq
        self.min_base_qual = baseq
        self.obs_tab = _ObsTabView(self.counts)

    def _row(self, pos):
        pos = int(pos)
        if 0 <= pos < self.counts.shape[0]:
            return self.counts[pos]
        return None

    def obs_at(self, pos, base=None, stranded=False):
        """observe.py:88-132: a Counter (base None), an int, or a (forward, reverse) tuple; ValueError for a bad base."""
        row = self._row(pos)
        if base is None:
            out = collections.Counter()
            if row is None:
                return out
            if stranded:
                for i, key in enumerate(BINS):
                    if row[i]:
                        out[key] = int(row[i])
                return out
            for i, key in enumerate(BINS):
                if row[i]:
                    out["-" if key == "+" else key.upper()] += int(row[i])
            return out
        # (substring tests, as the reference's: '' or 'AC' pass the first and count nothing, '-+' the second)
        if base.upper() in "ACGTN":
            i = _FWD.get(base.upper())
        elif base in "-+":
            i = _FWD["-"]
        else:
            raise ValueError("Bad base: %s" % (base))
        fwd, rev = (0, 0) if row is None or i is None else (int(row[i]), int(row[i + 7]))
        if stranded:
            return (fwd, rev)
        return fwd + rev

    def total_obs(self, pos):
        """observe.py:134-145: A + C + G + T of both strands (not N, not gaps)."""
        row = self._row(pos)
        if row is None:
            return 0
        return int(row[0:4].sum(dtype=numpy.int64) + row[7:11].sum(dtype=numpy.int64))


class _ObsTabView(collections.abc.Mapping):
    """Read-only pos -> Counter view of the table (the reference's obs_tab); any position gives a Counter."""

    def __init__(self, counts):
        self._counts = counts

    def __getitem__(self, pos):
        out = collections.Counter()
        pos = int(pos)
        if 0 <= pos < self._counts.shape[0]:
            row = self._counts[pos]
            for i, key in enumerate(BINS):
                if row[i]:
                    out[key] = int(row[i])
        return out

    def _observed(self):
        return numpy.flatnonzero(self._counts[:, :14].any(axis=1))

    def __iter__(self):
        return (int(p) for p in self._observed())

    def __len__(self):
        return len(self._observed())

    def __contains__(self, pos):
        try:
            pos = int(pos)
        except (TypeError, ValueError):
            return False
        return 0 <= pos < self._counts.shape[0] and bool(self._counts[pos, :14].any())
