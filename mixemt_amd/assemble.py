"""
mixemt's assembled haplotypes -- `-x` (assembly extension) and `-b PREFIX` (consensus FASTA) -- over assign.assign_reads'
ContribReads (one int32 label per alignment, on the device); the reference's mixemt/assemble.py:396-585 with an
AlignedSegment list replaced by (contrib_reads, name):

    call_consensus(refseq, contrib_reads, name, min_cov, args, strict=True)     assemble.py:431-466  -> str
    call_consensus_all(refseq, contrib_reads, min_cov, args, strict=True)       every key, from ONE labelled pileup
    find_new_variants(refseq, contrib_reads, args)                              assemble.py:469-501  -> {(pos, base): name}
    assign_reads_from_new_vars(contrib_reads, new_variants, args)               assemble.py:504-546
    extend_assemblies(refseq, contrib_reads, args)                              assemble.py:549-585
    write_consensus_seqs(refseq, contribs, contrib_reads, args)                 assemble.py:396-428  -> PREFIX.fa

Every step is a pass over data that is already on the device: the per-contributor tables come from
observe.count_bases_labelled, the per-position rule from mxm_consensus, the bases one contributor has alone from
mxm_new_variants, the walk of the unassigned alignments and their move from mxm_extend_assign, the tie rule of the
majority consensus from mxm_first_observed (csrc/assemble_kernels.hpp).  A round of the extension brings two counters
back to the host.  All integer work: the labels and the strings are the same for any alignment order.

Reference rules kept:
  - the contributors that take part in find_new_variants are the KEYS of contrib_reads other than 'unassigned'; a key
    without alignments has the consensus "" and so there are no new variants at all;
  - positions run over len(refseq), even when the pileup is longer; args.cons_cov is used as an int;
  - gaps and characters other than ACGTN count towards the coverage and can be called ('-'; 'X' is this library's stand-in
    for the reference's own character, see observe.py); a position where a contributor's consensus is 'X' gives no new
    variant (the reference would offer the character itself, which only a read showing that same character could match);
  - the move of an unassigned fragment takes ALL its unassigned alignments, below min_mq too.
"""

import ctypes
import sys

import numpy

from . import _lib, observe
from ._dev import current_stream, require_gpu, torch

FASTA_WIDTH = 60


def _struct_with_frag(contrib_reads):
    """The uploaded columns as mxm_aln_columns with the fragment column filled in (mxm_extend_assign reads it)."""
    dcols = contrib_reads.device_columns()
    st = dcols.struct()
    frag = contrib_reads.device_frag()
    cols = contrib_reads.cols
    st.n_frag = max(len(cols.names), int(cols.frag.max()) + 1 if len(cols) else 0)
    st.frag = frag.data_ptr() if frag.numel() else None
    return st, frag


def _remap(labels, use, n_names):
    """labels -> the index of the label in `use` (-1 for every other label), int32 on the device."""
    lut = numpy.full(n_names + 1, -1, dtype=numpy.int32)            # (the last entry serves label -1)
    for k, lab in enumerate(use):
        lut[lab] = k
    lut_d = torch.from_numpy(lut).to(labels.device)
    return lut_d[labels.to(torch.int64)].contiguous()


def _pileup_length(contrib_reads, args, ref_len):
    """observe.pileup_length of the table's columns (a host pass over every CIGAR: kept per (min_mq, ref_len))."""
    cache = contrib_reads.__dict__.setdefault("_pileup_len", {})
    key = (int(args.min_mq), int(ref_len))
    if key not in cache:
        cache[key] = observe.pileup_length(contrib_reads.cols, args.min_mq, ref_len)
    return cache[key]


def _consensus_device(counts, ref_len, min_cov, strict, want_tied=False):
    """mxm_consensus over counts[n][L][16] -> (cons uint8 [n][ref_len], tied or None, number of tied positions)."""
    lib = _lib.load()
    n, L = int(counts.shape[0]), int(counts.shape[1])
    dev = counts.device
    cons = torch.empty((n, max(ref_len, 1)), dtype=torch.uint8, device=dev)[:, :ref_len].contiguous()
    tied = torch.zeros((n, ref_len), dtype=torch.uint8, device=dev) if want_tied else None
    n_tied = torch.zeros(1, dtype=torch.int32, device=dev) if want_tied else None
    _lib.check(lib.mxm_consensus(counts.data_ptr(), n, L, ref_len, int(min_cov), 1 if strict else 0, cons.data_ptr(),
                                 tied.data_ptr() if want_tied else None, n_tied.data_ptr() if want_tied else None,
                                 current_stream()), "mxm_consensus")
    return cons, tied, (int(n_tied.cpu()[0]) if want_tied else 0)


def _tables(contrib_reads, label, n, args, ref_len):
    """One labelled pileup: counts[n][L][16] of the alignments with label[i] in [0, n)."""
    L = _pileup_length(contrib_reads, args, ref_len)
    counts = torch.zeros((max(n, 1), L, 16), dtype=torch.int32, device=label.device)
    if len(contrib_reads.cols) and n:
        observe.count_bases_labelled(contrib_reads.device_columns(), label, counts, args.min_mq, args.min_bq)
    return counts


def call_consensus_all(refseq, contrib_reads, min_cov, args, strict=True, names=None):
    """
    call_consensus of every key of contrib_reads (or of `names`, each looked up -- which makes it a key) ->
    {name: str}: ONE labelled pileup and ONE mxm_consensus, plus mxm_first_observed when strict is False and some
    position is tied.  A name without alignments gets "" (assemble.py:460-462).
    """
    require_gpu()
    if names is None:
        names = list(contrib_reads)
    for name in names:
        contrib_reads[name]
    ref_len = len(refseq)
    have = [name for name in names if contrib_reads.count(name) > 0]
    out = {name: "" for name in names}
    if not have or ref_len == 0:
        return out
    use = [contrib_reads.label_of(name) for name in have]
    label = _remap(contrib_reads.labels, use, len(contrib_reads.names))
    counts = _tables(contrib_reads, label, len(use), args, ref_len)
    cons, tied, n_tied = _consensus_device(counts, ref_len, min_cov, strict, want_tied=not strict)
    if n_tied:
        lib = _lib.load()
        st = contrib_reads.device_columns().struct()
        _lib.check(lib.mxm_first_observed(ctypes.byref(st), label.data_ptr(), contrib_reads.joined.data_ptr(), len(use),
                                          int(args.min_mq), int(args.min_bq), ref_len, tied.data_ptr(), cons.data_ptr(),
                                          current_stream()), "mxm_first_observed")
    host = cons.cpu().numpy()
    for k, name in enumerate(have):
        out[name] = host[k].tobytes().decode("ascii")
    return out


def call_consensus(refseq, contrib_reads, name, min_cov, args, strict=True):
    """
    assemble.call_consensus (assemble.py:431-466) of contrib_reads[name]: per reference position 'N' below min_cov
    observations (N observations do not count; gaps and other characters do), else the observed base when all agree
    (strict) or the most observed one (not strict; among equal counts the one observed first in the list).  "" for a
    name without alignments.
    """
    return call_consensus_all(refseq, contrib_reads, min_cov, args, strict, names=[name])[name]


class NewVariants(object):
    """find_new_variants' result on the device: newvar int32 [ref_len] (four int8 owners per position, A C G T), the
    labels of the owners (use[k] = label of owner k), their names, and the counter of entries."""

    def __init__(self, newvar, use, names, counter):
        self.newvar, self.use, self.names, self.counter = newvar, list(use), list(names), counter

    def __len__(self):
        return int(self.counter.cpu()[0])

    def as_dict(self):
        """{(pos, base): name}, the reference's return value."""
        words = self.newvar.cpu().numpy().view(numpy.int8).reshape(-1, 4)
        pos, b = numpy.nonzero(words >= 0)
        return {(int(p), "ACGT"[c]): self.names[int(words[p, c])] for p, c in zip(pos, b)}


def _participants(contrib_reads):
    return [name for name in contrib_reads if name != "unassigned"]


def _new_variants_device(refseq, contrib_reads, args, counts=None):
    """find_new_variants on the device -> NewVariants.  counts: the participants' tables, already counted (the
    extension loop keeps them); None = count them here."""
    lib = _lib.load()
    dev = contrib_reads.labels.device
    ref_len = len(refseq)
    names = _participants(contrib_reads)
    use = [contrib_reads.label_of(name) for name in names]
    newvar = torch.full((max(ref_len, 1),), -1, dtype=torch.int32, device=dev)[:ref_len]
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    nv = NewVariants(newvar, use, names, counter)
    if len(names) > 127:
        raise ValueError("find_new_variants: %d contributors take part, at most 127" % len(names))
    # no contributors, or one whose consensus is "" (no alignments: min_cons_len is 0): no new variants
    if not names or ref_len == 0 or any(u is None or contrib_reads.count(n) == 0 for u, n in zip(use, names)):
        return nv
    if counts is None:
        counts = _tables(contrib_reads, _remap(contrib_reads.labels, use, len(contrib_reads.names)), len(use), args, ref_len)
    cons, _, _ = _consensus_device(counts, ref_len, int(args.cons_cov), True)
    rows = (ctypes.c_int32 * len(use))(*range(len(use)))
    _lib.check(lib.mxm_new_variants(cons.data_ptr(), ref_len, len(use), rows, len(use), ref_len, newvar.data_ptr(),
                                    counter.data_ptr(), current_stream()), "mxm_new_variants")
    return nv


def find_new_variants(refseq, contrib_reads, args):
    """
    assemble.find_new_variants (assemble.py:469-501): {(pos, base): contributor} for the bases ONE contributor's strict
    consensus (coverage args.cons_cov) has alone at a position every participating consensus calls.
    """
    require_gpu()
    return _new_variants_device(refseq, contrib_reads, args).as_dict()


def _variants_from_dict(contrib_reads, new_variants, ref_len=None):
    """A {(pos, base): name} dict as NewVariants (uploaded): for callers that made or edited the dict themselves."""
    dev = contrib_reads.labels.device
    names = sorted(set(new_variants.values()), key=lambda n: (contrib_reads.label_of(n) is None, str(n)))
    for name in names:
        if contrib_reads.label_of(name) is None:
            raise ValueError("assign_reads_from_new_vars: '%s' is no contributor of this table" % (name))
    if len(names) > 127:
        raise ValueError("assign_reads_from_new_vars: %d contributors own variants, at most 127" % len(names))
    n = max([int(p) for p, _ in new_variants] + [-1]) + 1 if ref_len is None else int(ref_len)
    words = numpy.full((max(n, 1), 4), -1, dtype=numpy.int8)
    for (pos, base), name in new_variants.items():
        if base in ("A", "C", "G", "T") and 0 <= int(pos) < n:      # (an upper-cased read base is one of these or no hit)
            words[int(pos), "ACGT".index(base)] = names.index(name)
    newvar = torch.from_numpy(words.view(numpy.int32).reshape(-1)).to(dev)[:n]
    counter = torch.tensor([len(new_variants)], dtype=torch.int32, device=dev)
    return NewVariants(newvar, [contrib_reads.label_of(name) for name in names], names, counter)


def _extend_assign(contrib_reads, nv, args, state):
    """mxm_extend_assign with the labels updated in place -> the device counter of moved alignments (accumulated in
    state['moved'])."""
    lib = _lib.load()
    un = contrib_reads.label_of("unassigned")
    n_aln = len(contrib_reads.cols)
    contrib_reads.rounds += 1
    if un is None or not n_aln or not nv.use:
        return
    st, frag = _struct_with_frag(contrib_reads)
    dev = contrib_reads.labels.device
    if state.get("frag_state") is None:
        state["frag_state"] = torch.empty(max(int(st.n_frag), 1), dtype=torch.int32, device=dev)
        state["moved_owner"] = torch.empty(n_aln, dtype=torch.int32, device=dev)
    rows = (ctypes.c_int32 * len(nv.use))(*nv.use)
    _lib.check(lib.mxm_extend_assign(ctypes.byref(st), contrib_reads.labels.data_ptr(), contrib_reads.joined.data_ptr(), un,
                                     len(contrib_reads.names), rows, len(nv.use), contrib_reads.rounds, int(args.min_mq),
                                     int(args.min_bq), nv.newvar.data_ptr(), int(nv.newvar.numel()),
                                     state["frag_state"].data_ptr(), state["moved_owner"].data_ptr(),
                                     state["moved"].data_ptr(), current_stream()), "mxm_extend_assign")


def assign_reads_from_new_vars(contrib_reads, new_variants, args):
    """
    assemble.assign_reads_from_new_vars (assemble.py:504-546): the unassigned fragments whose bases (mapq >= args.min_mq,
    quality >= args.min_bq or none) show new variants of exactly ONE contributor move to it, with all their unassigned
    alignments.  new_variants: find_new_variants' dict.  Returns contrib_reads, relabelled.
    """
    require_gpu()
    contrib_reads["unassigned"]
    nv = new_variants if isinstance(new_variants, NewVariants) else _variants_from_dict(contrib_reads, new_variants)
    state = {"moved": torch.zeros(1, dtype=torch.int32, device=contrib_reads.labels.device)}
    _extend_assign(contrib_reads, nv, args, state)
    contrib_reads.relabel(contrib_reads.labels)
    return contrib_reads


def extend_assemblies(refseq, contrib_reads, args):
    """
    assemble.extend_assemblies (assemble.py:549-585): rounds of find_new_variants -> assign_reads_from_new_vars until the
    number of unassigned alignments stops changing (one more round after the last move), with the reference's verbose
    lines on stderr.  The contributors' tables are counted once and then only ADDED to: a round after the first counts
    the alignments that moved in the round before.  Per round the two counters (moved, new variants) come back.
    """
    require_gpu()
    contrib_reads["unassigned"]                                      # (the reference's defaultdict gains the key here)
    dev = contrib_reads.labels.device
    ref_len = len(refseq)
    last_unassigned = None
    unassigned = contrib_reads.count("unassigned")
    run = 1
    if args.verbose:
        sys.stderr.write("\nAssembly extension step...\n")
    names = _participants(contrib_reads)
    use = [contrib_reads.label_of(name) for name in names]
    live = bool(names) and ref_len > 0 and all(u is not None and contrib_reads.count(n) > 0 for u, n in zip(use, names))
    counts = None
    state = {"moved": torch.zeros(1, dtype=torch.int32, device=dev)}
    pending = None                                                   # labels of the alignments not yet in the tables
    if live:
        pending = _remap(contrib_reads.labels, use, len(contrib_reads.names))
        L = _pileup_length(contrib_reads, args, ref_len)
        counts = torch.zeros((len(use), L, 16), dtype=torch.int32, device=dev)
    while last_unassigned != unassigned:
        if live and pending is not None and len(contrib_reads.cols):
            observe.count_bases_labelled(contrib_reads.device_columns(), pending, counts, args.min_mq, args.min_bq)
        nv = _new_variants_device(refseq, contrib_reads, args, counts)
        state["moved"].zero_()
        _extend_assign(contrib_reads, nv, args, state)
        moved, n_new = int(state["moved"].cpu()[0]), len(nv)
        # (the owners of mxm_extend_assign index nv.use, which is `use`: what moved is labelled for the tables as it is)
        pending = state.get("moved_owner") if moved else None
        last_unassigned = unassigned
        unassigned -= moved
        if args.verbose:
            sys.stderr.write("  %d: %d/%d reads assigned using %d variants\n"
                             % (run, last_unassigned - unassigned, last_unassigned, n_new))
        run += 1
    if args.verbose:
        sys.stderr.write("\n")
    contrib_reads.relabel(contrib_reads.labels)
    return contrib_reads


def format_fasta(records):
    """
    FASTA text of (id, description, sequence) records in the layout of Biopython's FASTA writer (SeqIO.write(...,
    'fasta'), which the reference calls): '>id description' ('>id' alone when the description is empty, the description
    alone when it already starts with the id), then the sequence in lines of 60; an empty sequence has no sequence line.
    This layout is taken from Biopython's documented writer, not from a run of it (Biopython is not a dependency).
    """
    out = []
    for rec_id, description, seq in records:
        rec_id = str(rec_id).replace("\n", " ").replace("\r", " ")
        description = str(description).replace("\n", " ").replace("\r", " ")
        if description and description.split(None, 1)[0] == rec_id:
            title = description
        elif description:
            title = "%s %s" % (rec_id, description)
        else:
            title = rec_id
        out.append(">%s\n" % title)
        out.extend(seq[i:i + FASTA_WIDTH] + "\n" for i in range(0, len(seq), FASTA_WIDTH))
    return "".join(out)


def write_consensus_seqs(refseq, contribs, contrib_reads, args):
    """
    assemble.write_consensus_seqs (assemble.py:396-428): args.cons_prefix + '.fa' with the majority consensus (min_cov 1,
    strict=False) of every contributor of `contribs` in order (id hap#, description the haplogroup; looking one up makes
    it a key, as report_contributors does), then of 'unassigned' when it is a key.  See format_fasta for the layout.
    """
    names = [con for con, _, _ in contribs]
    for name in names:
        contrib_reads[name]
    records = [(con, hap) for con, hap, _ in contribs]
    if "unassigned" in contrib_reads:
        names.append("unassigned")
        records.append(("unassigned", ""))
    seqs = call_consensus_all(refseq, contrib_reads, 1, args, strict=False, names=names)
    with open("%s.fa" % (args.cons_prefix), "w") as fa_out:
        fa_out.write(format_fasta((rec_id, desc, seqs[rec_id]) for rec_id, desc in records))


# ---- the assembly stage of a cohort: -x and -b for ALL samples in shared rounds (assign.CohortContribReads) -----------------
def _cohort_tables(cohort, args, ref_len, who):
    """(L, zeroed counts[n_labels][L][16]) of a cohort, within its byte budget."""
    from .assign import _cohort_budget
    cache = cohort.__dict__.setdefault("_pileup_len", {})
    key = (int(args.min_mq), int(ref_len))
    if key not in cache:
        cache[key] = observe.pileup_length(cohort.cols, args.min_mq, ref_len)
    L = cache[key]
    _cohort_budget(who, cohort.n_labels, L, cohort.max_bytes)
    return L, torch.zeros((max(cohort.n_labels, 1), L, 16), dtype=torch.int32, device=cohort.labels.device)


def _cohort_struct(cohort):
    """The cohort's uploaded columns as mxm_aln_columns with the fragment column (mxm_extend_assign_samples reads it)."""
    st = cohort.device_columns().struct()
    frag = cohort.device_frag()
    st.n_frag = cohort.n_frag
    st.frag = frag.data_ptr() if frag.numel() else None
    return st


def _i32(values):
    return (ctypes.c_int32 * max(len(values), 1))(*values)


def extend_assemblies_many(refseq, cohort, args, samples=None):
    """
    extend_assemblies for the samples `samples` of an assign.CohortContribReads (default: those with more than one
    contributor, bin/mixemt:329) in SHARED rounds: a round for all samples that are still moving is one labelled pileup
    call that adds the pending alignments to counts[n_labels][L][16], one mxm_consensus, one mxm_new_variants_samples, one
    mxm_extend_assign_samples, and one read-back of two counters per sample.  Per sample the labels, joined, keys and rounds
    are those of extend_assemblies on the sample alone: its participants are its keys other than 'unassigned'; when one of
    them has no alignments there are no new variants at all; at least one round is run; after its first round without a
    move the sample is FROZEN (no 'unassigned' label and no participants are handed to the kernels), so nothing of it can
    change while others run on; joined is the sample's own round number.  With args.verbose every sample's stderr text is
    collected and written sample after sample, each block what its own extend_assemblies call writes.
    The tables take n_labels x L x 64 bytes: ValueError above the cohort's max_bytes (assign.assign_reads_many).
    Returns cohort, relabelled in place.
    """
    require_gpu()
    lib = _lib.load()
    n = cohort.n_samples
    ref_len = len(refseq)
    if samples is None:
        samples = [s for s in range(n) if cohort.n_contribs(s) > 1]
    samples = sorted(set(int(s) for s in samples))
    if any(not 0 <= s < n for s in samples):
        raise IndexError("extend_assemblies_many: sample index out of range")
    if not samples:
        return cohort
    dev = cohort.labels.device
    count = cohort.counts()
    use_of, un_of, unassigned, text = {}, {}, {}, {}
    for s in samples:
        if "unassigned" not in cohort.keys[s]:
            cohort.keys[s].append("unassigned")                      # (the reference's defaultdict gains the key here)
        names = [name for name in cohort.keys[s] if name != "unassigned"]
        if len(names) > 127:
            raise ValueError("find_new_variants: %d contributors take part, at most 127" % len(names))
        use = [cohort.label_of(s, name) for name in names]
        live = bool(names) and ref_len > 0 and all(u is not None and count[u] > 0 for u in use)
        use_of[s] = use if live else []
        un_of[s] = cohort.label_of(s, "unassigned")
        unassigned[s] = int(count[un_of[s]]) if un_of[s] is not None else 0
        text[s] = ["\nAssembly extension step...\n"]
    L, counts = _cohort_tables(cohort, args, ref_len, "extend_assemblies_many")
    n_aln = len(cohort.cols)
    lut = numpy.full(cohort.n_labels + 1, -1, dtype=numpy.int32)     # (the last entry serves label -1)
    for s in samples:
        for u in use_of[s]:
            lut[u] = u
    pending = torch.from_numpy(lut).to(dev)[cohort.labels.to(torch.int64)].contiguous() if n_aln else None
    cons = torch.empty((max(cohort.n_labels, 1), max(ref_len, 1)), dtype=torch.uint8, device=dev)
    newvar = torch.full((n, max(ref_len, 1)), -1, dtype=torch.int32, device=dev)
    counters = torch.zeros((2, n), dtype=torch.int32, device=dev)   # [0]: new variants, [1]: moved alignments
    frag_state = torch.empty(max(cohort.n_frag, 1), dtype=torch.int32, device=dev)
    moved_owner = torch.empty(max(n_aln, 1), dtype=torch.int32, device=dev)
    st = _cohort_struct(cohort)
    dcols = cohort.device_columns()
    active = list(samples)
    run = 1
    while active:
        use_ptr, use, un = [0], [], [-1] * n
        for s in range(n):
            if s in active:
                use.extend(use_of[s])
                un[s] = -1 if un_of[s] is None else un_of[s]
            use_ptr.append(len(use))
        counters.zero_()
        if use and n_aln:
            if pending is not None:
                observe.count_bases_labelled(dcols, pending, counts, args.min_mq, args.min_bq)
            _lib.check(lib.mxm_consensus(counts.data_ptr(), cohort.n_labels, L, ref_len, int(args.cons_cov), 1, cons.data_ptr(),
                                         None, None, current_stream()), "mxm_consensus")
            _lib.check(lib.mxm_new_variants_samples(cons.data_ptr(), cons.stride(0), cohort.n_labels, _i32(use), _i32(use_ptr),
                                                    n, ref_len, newvar.data_ptr(), counters[0].data_ptr(), current_stream()),
                       "mxm_new_variants_samples")
            if any(un[s] >= 0 and use_ptr[s + 1] > use_ptr[s] for s in range(n)):
                _lib.check(lib.mxm_extend_assign_samples(ctypes.byref(st), cohort.aln_sample.data_ptr(), cohort.labels.data_ptr(),
                                                         cohort.joined.data_ptr(), _i32(un), _i32(use), _i32(use_ptr), n,
                                                         cohort.n_labels, run, int(args.min_mq), int(args.min_bq),
                                                         newvar.data_ptr(), ref_len, frag_state.data_ptr(),
                                                         moved_owner.data_ptr(), counters[1].data_ptr(), current_stream()),
                           "mxm_extend_assign_samples")
        got = counters.cpu().numpy()                                 # ONE read-back per round: two counters per sample
        any_moved = False
        for s in list(active):
            n_new, moved = int(got[0, s]), int(got[1, s])
            cohort.rounds[s] += 1
            cohort.round_log[s].append((moved, unassigned[s], n_new))
            text[s].append("  %d: %d/%d reads assigned using %d variants\n" % (run, moved, unassigned[s], n_new))
            unassigned[s] -= moved
            any_moved = any_moved or moved > 0
            if not moved:
                active.remove(s)                                     # frozen: its labels, joined and rounds stay
        # (moved_owner holds global labels, -1 for what did not move: the labels of the next additive pileup as they are)
        pending = moved_owner if any_moved else None
        run += 1
    if args.verbose:
        for s in samples:
            sys.stderr.write("".join(text[s]) + "\n")
    return cohort


def call_consensus_many(refseq, cohort, min_cov, args, strict=True):
    """
    call_consensus_all for every sample of an assign.CohortContribReads -> one {name: str} per sample over the sample's
    keys: ONE labelled pileup over the global labels, ONE mxm_consensus, ONE mxm_first_observed when strict is False and
    some position is tied (the global labels are its tables; its scratch takes the tables' size again), ONE download.  The
    strings equal call_consensus_all of cohort.sample(s); a name without alignments gives "".
    """
    require_gpu()
    ref_len = len(refseq)
    out = [{name: "" for name in keys} for keys in cohort.keys]
    count = cohort.counts()
    if ref_len == 0 or not len(cohort.cols) or not count.any():
        return out
    lib = _lib.load()
    L, counts = _cohort_tables(cohort, args, ref_len, "call_consensus_many")
    observe.count_bases_labelled(cohort.device_columns(), cohort.labels, counts, args.min_mq, args.min_bq)
    cons, tied, n_tied = _consensus_device(counts, ref_len, min_cov, strict, want_tied=not strict)
    if n_tied:
        st = cohort.device_columns().struct()
        _lib.check(lib.mxm_first_observed(ctypes.byref(st), cohort.labels.data_ptr(), cohort.joined.data_ptr(), cohort.n_labels,
                                          int(args.min_mq), int(args.min_bq), ref_len, tied.data_ptr(), cons.data_ptr(),
                                          current_stream()), "mxm_first_observed")
    host = cons.cpu().numpy()
    for s, keys in enumerate(cohort.keys):
        for name in keys:
            lab = cohort.label_of(s, name)
            if lab is not None and count[lab] > 0:
                out[s][name] = host[lab].tobytes().decode("ascii")
    return out


def write_consensus_seqs_many(refseq, contribs_list, cohort, args, prefixes):
    """
    write_consensus_seqs for every sample of an assign.CohortContribReads: prefixes[s] + '.fa' holds what
    write_consensus_seqs(refseq, contribs_list[s], cohort.sample(s), args) writes under that prefix -- the majority
    consensus (min_cov 1, strict=False) of every contributor in order (looking one up makes it a key of the sample), then
    of 'unassigned' when it is a key -- from ONE call_consensus_many.  args.cons_prefix is not read.
    """
    if len(contribs_list) != cohort.n_samples or len(prefixes) != cohort.n_samples:
        raise ValueError("write_consensus_seqs_many: one contributor table and one prefix per sample are needed")
    records = []
    for s, contribs in enumerate(contribs_list):
        for con, _, _ in contribs:
            if con not in cohort.keys[s]:
                cohort.keys[s].append(con)
        recs = [(con, hap) for con, hap, _ in contribs]
        if "unassigned" in cohort.keys[s]:
            recs.append(("unassigned", ""))
        records.append(recs)
    seqs = call_consensus_many(refseq, cohort, 1, args, strict=False)
    for s, recs in enumerate(records):
        with open("%s.fa" % (prefixes[s]), "w") as fa_out:
            fa_out.write(format_fasta((rec_id, desc, seqs[s][rec_id]) for rec_id, desc in recs))
