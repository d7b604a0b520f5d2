"""
The pileup and the assembly kernels of include/mixemt_hip.h called through ctypes with every device pointer -- the arrays
inside mxm_aln_columns included -- guard-banded at its exact documented size (tests/_guarded.py): mxm_observe_bases,
mxm_observe_bases_labelled, mxm_consensus, mxm_new_variants, mxm_first_observed, mxm_extend_assign.  References:
tests/_pileup_ref.py for the tables, numpy restatements of the header's rules for the consensus and the new variants,
tests/_assemble_ref.py for the tie rule and the extension.  The alignments are the long D / N operations of
test_long_reads_and_gaps_cross_windows (past the kernel's window: its global-atomic path), with qualities on half of
them, plus one that ends on the table's last position; L is no multiple of 512.
"""
import ctypes

import numpy
import pytest

import _pileup_ref
from _guarded_abi import load_lib, stream as _stream, sync as _sync
from _guarded import guarded, guarded_from

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_LABELS = 4


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _columns(alns):
    """[(start, [(op, n)], seq, qualities or None, mapq, reverse)] -> AlignmentColumns."""
    from mixemt_amd.alignments import AlignmentColumns
    raw = [numpy.frombuffer(a[2].encode(), dtype=numpy.uint8) for a in alns]
    cig = [numpy.array([(n << 4) | op for op, n in a[1]], dtype=numpy.uint32) for a in alns]
    qual = numpy.concatenate([numpy.asarray(a[3] if a[3] is not None else [0] * len(a[2]), dtype=numpy.uint8) for a in alns])
    return AlignmentColumns([a[0] for a in alns], [a[4] for a in alns], numpy.arange(len(alns)),
                            numpy.concatenate([[0], numpy.cumsum([len(c) for c in cig])]), numpy.concatenate(cig),
                            numpy.concatenate([[0], numpy.cumsum([len(r) for r in raw])]), numpy.concatenate(raw), qual,
                            numpy.array([a[3] is not None for a in alns], dtype=numpy.uint8),
                            ["r%d" % i for i in range(len(alns))], [a[5] for a in alns])


def _long_alignments(seed, n_aln=300):
    rng = numpy.random.default_rng(seed)
    alns = []
    for _ in range(n_aln):
        start = int(rng.integers(0, 4000))
        ops = [(0, int(rng.integers(50, 900))), (2, int(rng.integers(1, 700))), (0, int(rng.integers(10, 300))),
               (3, int(rng.integers(1, 1500))), (1, 5), (4, 3), (0, int(rng.integers(1, 200)))]
        qlen = sum(n for op, n in ops if op in (0, 1, 4))
        seq = "".join(rng.choice(list("ACGTNacgtR"), size=qlen))
        qual = rng.integers(20, 41, size=qlen) if rng.random() < 0.5 else None
        alns.append((start, ops, seq, qual, int(rng.choice([60, 60, 60, 30, 29, 0])), int(rng.integers(0, 2))))
    alns.append((-1, [(0, 4)], "ACGT", None, 60, 0))                       # unplaced: skipped
    end = max(a[0] + sum(n for op, n in a[1] if op in (0, 2, 3, 7, 8)) for a in alns if a[4] >= 30)
    table_len = end + 1 if (end + 1) % 512 else end + 2
    alns.append((table_len - 10, [(7, 4), (8, 6)], "ACGTACGTAC", None, 60, 1))        # ends on the last position
    assert table_len % 512 != 0
    return alns, table_len


class DeviceAln:
    """AlignmentColumns uploaded array by array into guarded buffers of exactly n, n + 1, n_cigar and n_bases elements."""

    def __init__(self, cols):
        self.n = len(cols)
        self.bufs = {"ref_start": guarded_from(cols.ref_start, numpy.int64, 8, DEV), "mapq": guarded_from(cols.mapq, numpy.int32, 4, DEV),
                     "cig_ptr": guarded_from(cols.cig_ptr, numpy.int64, 8, DEV), "cigar": guarded_from(cols.cigar, numpy.uint32, 4, DEV),
                     "seq_ptr": guarded_from(cols.seq_ptr, numpy.int64, 8, DEV), "seq": guarded_from(cols.seq, numpy.uint8, 1, DEV),
                     "qual": guarded_from(cols.qual, numpy.uint8, 1, DEV), "has_qual": guarded_from(cols.has_qual, numpy.uint8, 1, DEV),
                     "is_reverse": guarded_from(cols.is_reverse, numpy.uint8, 1, DEV)}
        from mixemt_amd import _lib
        b = self.bufs
        self.struct = _lib.AlnColumns(self.n, 0, b["ref_start"].ptr, b["mapq"].ptr, None, b["cig_ptr"].ptr, b["cigar"].ptr,
                                      b["seq_ptr"].ptr, b["seq"].ptr, b["qual"].ptr, b["has_qual"].ptr)

    def check(self, what):
        for name, buf in self.bufs.items():
            buf.check("%s (%s)" % (name, what))


def _empty_tables(n_tables, table_len):
    """counts[n_tables][L][16] uint32, exactly: zeroed, with bins 14-15 ("pad, left alone") holding 0xFFFFFFFF."""
    init = numpy.zeros((n_tables, table_len, 16), dtype=numpy.uint32)
    init[:, :, 14:] = 0xFFFFFFFF
    return guarded_from(init, numpy.uint32, 4, DEV)


def _check_tables(buf, want, times, what):
    got = buf.get(numpy.uint32, want.shape[:-1] + (16,))
    assert (got[..., 14:] == 0xFFFFFFFF).all(), "bins 14-15 were written (%s)" % what
    assert numpy.array_equal(got[..., :14].astype(numpy.int64), times * want[..., :14]), what


@pytest.fixture(scope="module")
def pile():
    """The alignments, the table length, random labels and the reference's tables: made once, never written."""
    alns, table_len = _long_alignments(5)
    cols = _columns(alns)
    rng = numpy.random.default_rng(6)
    label = rng.integers(-1, N_LABELS, size=len(cols)).astype(numpy.int32)
    label[-1] = N_LABELS - 1                                # the alignment on the last position, in the last table
    want = _pileup_ref.pileup(cols, table_len, 30, 30)
    per = numpy.stack([_pileup_ref.pileup(_subset(cols, numpy.flatnonzero(label == k)), table_len, 30, 30) for k in range(N_LABELS)])
    assert want[table_len - 1].sum() > 0 and per[N_LABELS - 1, table_len - 1].sum() > 0 and want[:, 6].sum() > 10000
    return cols, table_len, label, want, per


def _subset(cols, idx):
    from mixemt_amd.alignments import AlignmentColumns
    idx = numpy.asarray(idx, dtype=numpy.int64)
    cig = [cols.cigar[cols.cig_ptr[i]:cols.cig_ptr[i + 1]] for i in idx]
    seq = [cols.seq[cols.seq_ptr[i]:cols.seq_ptr[i + 1]] for i in idx]
    qual = [cols.qual[cols.seq_ptr[i]:cols.seq_ptr[i + 1]] for i in idx]
    cat = lambda parts, dt: numpy.concatenate(parts).astype(dt) if parts else numpy.zeros(0, dtype=dt)      # noqa: E731
    return AlignmentColumns(cols.ref_start[idx], cols.mapq[idx], numpy.arange(len(idx)),
                            numpy.concatenate([[0], numpy.cumsum([len(c) for c in cig])]).astype(numpy.int64), cat(cig, numpy.uint32),
                            numpy.concatenate([[0], numpy.cumsum([len(s) for s in seq])]).astype(numpy.int64), cat(seq, numpy.uint8),
                            cat(qual, numpy.uint8), cols.has_qual[idx], ["r%d" % i for i in idx], cols.is_reverse[idx])


def test_observe_bases_accumulates_into_exactly_its_table(lib, pile):
    """mixemt_hip.h: "counts[L][16] (uint32, ZEROED by the caller, accumulated into) per reference position: bins 0-6 forward
    ..., 7-13 reverse ..., 14-15 pad (left alone)"; a second call adds the same counts again."""
    cols, table_len, _, want, _ = pile
    dev = DeviceAln(cols)
    counts = _empty_tables(1, table_len)
    for times in (1, 2):
        assert lib.mxm_observe_bases(ctypes.byref(dev.struct), dev.bufs["is_reverse"].ptr, 30, 30, table_len, counts.ptr,
                                     _stream()) == 0, lib.mxm_last_error()
        _sync()
        dev.check("mxm_observe_bases")
        counts.check("counts")
        _check_tables(counts, want[None], times, "L=%d call %d" % (table_len, times))


def test_observe_bases_labelled_fills_exactly_n_labels_tables(lib, pile):
    """mixemt_hip.h: "alignment i with label[i] (DEVICE int32[n_aln]) in [0, n_labels) is counted ... into table
    counts[label[i]][L][16] (uint32, n_labels tables back to back ...); label[i] < 0: not counted"."""
    cols, table_len, label, _, per = pile
    dev = DeviceAln(cols)
    lab = guarded_from(label, numpy.int32, 4, DEV)
    counts = _empty_tables(N_LABELS, table_len)
    assert lib.mxm_observe_bases_labelled(ctypes.byref(dev.struct), dev.bufs["is_reverse"].ptr, lab.ptr, N_LABELS, 30, 30,
                                          table_len, counts.ptr, _stream()) == 0, lib.mxm_last_error()
    _sync()
    dev.check("mxm_observe_bases_labelled")
    lab.check("label")
    counts.check("counts")
    _check_tables(counts, per, 1, "L=%d, %d tables" % (table_len, N_LABELS))


@pytest.mark.parametrize("short_by", [1, 7, 600])
def test_an_alignment_past_the_table_is_minus_1_and_nothing_is_written_outside(lib, pile, short_by):
    """mixemt_hip.h: "Returns 0, -1 (bad arguments, or an alignment reaching position L or beyond) ...; after -1 / -4 the
    table's contents are unspecified" -- but it is the table alone that may have been written."""
    cols, table_len, label, _, _ = pile
    dev = DeviceAln(cols)
    lab = guarded_from(label, numpy.int32, 4, DEV)
    short = table_len - short_by
    counts = _empty_tables(1, short)
    assert lib.mxm_observe_bases(ctypes.byref(dev.struct), dev.bufs["is_reverse"].ptr, 30, 30, short, counts.ptr, _stream()) == -1
    assert b"reaches past the table (L = %d)" % short in lib.mxm_last_error()
    _sync()
    dev.check("past the table")
    counts.check("counts of %d positions for alignments that reach %d" % (short, table_len))
    assert (counts.get(numpy.uint32, (short, 16))[:, 14:] == 0xFFFFFFFF).all()
    tables = _empty_tables(N_LABELS, short)
    assert lib.mxm_observe_bases_labelled(ctypes.byref(dev.struct), dev.bufs["is_reverse"].ptr, lab.ptr, N_LABELS, 30, 30, short,
                                          tables.ptr, _stream()) == -1
    _sync()
    dev.check("past the table, labelled")
    lab.check("label")
    tables.check("%d tables of %d positions for alignments that reach %d" % (N_LABELS, short, table_len))
    assert (tables.get(numpy.uint32, (N_LABELS, short, 16))[..., 14:] == 0xFFFFFFFF).all()


# ---- mxm_consensus / mxm_new_variants -------------------------------------------------------------------------------------
def _consensus_ref(per, ref_len, min_cov, strict):
    """The header's rule per (table, position): strands folded, N ignored, total = A + C + G + T + other + gap."""
    n_labels, table_len = per.shape[:2]
    folded = numpy.zeros((n_labels, ref_len, 7), dtype=numpy.int64)
    use = min(table_len, ref_len)
    folded[:, :use] = per[:, :use, 0:7] + per[:, :use, 7:14]
    cand = folded[..., [0, 1, 2, 3, 5, 6]]                               # A C G T other gap, in the order ties are listed
    total = cand.sum(axis=2)
    best = cand.max(axis=2)
    at_best = cand == best[..., None]
    first = at_best.argmax(axis=2)
    chars = numpy.frombuffer(b"ACGTX-", dtype=numpy.uint8)[first]
    called = (total > 0) & (total >= min_cov)
    if strict:
        cons = numpy.where(called & (best == total), chars, ord("N")).astype(numpy.uint8)
        return cons, numpy.zeros_like(cons)
    cons = numpy.where(called, chars, ord("N")).astype(numpy.uint8)
    bits = numpy.array([1, 2, 4, 8, 32, 64], dtype=numpy.int64)
    mask = (at_best * bits).sum(axis=2)
    tied = numpy.where(called & (at_best.sum(axis=2) > 1), mask, 0).astype(numpy.uint8)
    return cons, tied


@pytest.mark.parametrize("strict", [1, 0])
@pytest.mark.parametrize("extra,min_cov", [(0, 1), (37, 3), (-100, 2)])
def test_consensus_and_new_variants(lib, pile, strict, extra, min_cov):
    """mixemt_hip.h, mxm_consensus: "counts[n_labels][L][16] ... 16-byte aligned -> cons[n_labels][ref_len] uint8 ...;
    tied[n_labels][ref_len] (nullable) ...; n_tied (nullable): + the tied positions.  Positions >= L have no observations";
    mxm_new_variants: "rows[n_use] (HOST int32: rows of cons[n_rows][ld], ld >= ref_len).  newvar[ref_len] (DEVICE): one
    32-bit word per position holding four int8 owners ...; n_new: + the (position, base) entries"."""
    _, table_len, _, _, per = pile
    ref_len = table_len + extra
    low = per.copy()
    low[:, ::3] = numpy.minimum(low[:, ::3], 1)                          # every third position: counts of 0 / 1, hence ties
    tables = numpy.zeros((N_LABELS, table_len, 16), dtype=numpy.uint32)
    tables[..., :14] = low[..., :14]
    tables[..., 14:] = 0xFFFFFFFF                                        # a consensus that adds the pad bins in would show
    c_buf = guarded_from(tables, numpy.uint32, 16, DEV)
    cons = guarded(N_LABELS * ref_len, 1, DEV)
    tied = guarded(N_LABELS * ref_len, 1, DEV)
    n_tied = guarded_from([5], numpy.uint32, 4, DEV)
    assert lib.mxm_consensus(c_buf.ptr, N_LABELS, table_len, ref_len, min_cov, strict, cons.ptr, tied.ptr, n_tied.ptr,
                             _stream()) == 0, lib.mxm_last_error()
    _sync()
    for name, buf in (("counts", c_buf), ("cons", cons), ("tied", tied), ("n_tied", n_tied)):
        buf.check("%s ref_len=%d L=%d" % (name, ref_len, table_len))
    want_cons, want_tied = _consensus_ref(low, ref_len, min_cov, strict)
    got_cons = cons.get(numpy.uint8, (N_LABELS, ref_len))
    assert numpy.array_equal(got_cons, want_cons)
    assert numpy.array_equal(tied.get(numpy.uint8, (N_LABELS, ref_len)), want_tied)
    assert int(n_tied.get(numpy.uint32)[0]) == 5 + int((want_tied != 0).sum()) and (strict or (want_tied != 0).any())
    # without the optional outputs
    again = guarded(N_LABELS * ref_len, 1, DEV)
    assert lib.mxm_consensus(c_buf.ptr, N_LABELS, table_len, ref_len, min_cov, strict, again.ptr, None, None, _stream()) == 0
    _sync()
    again.check("cons alone")
    assert numpy.array_equal(again.get(numpy.uint8), got_cons.reshape(-1))
    # find_new_variants over rows 3 and 1 of a padded cons[n_rows][ld]
    ld = ref_len + 5
    padded = numpy.full((N_LABELS, ld), 0xFF, dtype=numpy.uint8)
    padded[:, :ref_len] = want_cons
    p_buf = guarded_from(padded, numpy.uint8, 1, DEV)
    for use in ([3, 1], [2], [0, 1, 2, 3]):
        rows = (ctypes.c_int32 * len(use))(*use)
        newvar = guarded(4 * ref_len, 4, DEV)
        n_new = guarded_from([11], numpy.uint32, 4, DEV)
        assert lib.mxm_new_variants(p_buf.ptr, ld, N_LABELS, rows, len(use), ref_len, newvar.ptr, n_new.ptr, _stream()) == 0, \
            lib.mxm_last_error()
        _sync()
        for name, buf in (("cons", p_buf), ("newvar", newvar), ("n_new", n_new)):
            buf.check("%s rows=%r" % (name, use))
        sub = want_cons[use]                                             # [n_use][ref_len]
        base = numpy.full(sub.shape, -1, dtype=numpy.int64)
        for k, ch in enumerate(b"ACGT"):
            base[sub == ch] = k
        skip = (base < 0).any(axis=0)
        want = numpy.full((ref_len, 4), -1, dtype=numpy.int8)
        for k in range(4):
            has = base == k
            only = has.sum(axis=0) == 1
            want[only & ~skip, k] = has.argmax(axis=0)[only & ~skip]
        assert numpy.array_equal(newvar.get(numpy.int8, (ref_len, 4)), want), use
        assert int(n_new.get(numpy.uint32)[0]) == 11 + int((want >= 0).sum()), use


# ---- mxm_first_observed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, -100])
def test_first_observed_settles_the_ties_in_list_order(lib, pile, extra):
    """mixemt_hip.h, mxm_first_observed: "the order key of alignment i is (joined[i], i) ...; keeps the smallest key per
    (table, tied position, folded bin) and writes the bin with the smallest one into cons[n_labels][ref_len] where tied[.] is
    set" -- tied is only read, untied positions keep their character, and an alignment that runs past ref_len (extra < 0)
    touches nothing outside the two tables.  Reference: tests/_assemble_ref.py's non-strict consensus of each label's list."""
    import _assemble_ref
    cols, table_len, label, _, per = pile
    ref_len = table_len + extra
    joined = numpy.random.default_rng(8).integers(0, 3, size=len(cols)).astype(numpy.int32)
    tables = numpy.zeros((N_LABELS, table_len, 16), dtype=numpy.uint32)
    tables[..., :14] = per[..., :14]
    c_buf = guarded_from(tables, numpy.uint32, 16, DEV)
    cons = guarded(N_LABELS * ref_len, 1, DEV)
    tied = guarded(N_LABELS * ref_len, 1, DEV)
    assert lib.mxm_consensus(c_buf.ptr, N_LABELS, table_len, ref_len, 1, 0, cons.ptr, tied.ptr, None, _stream()) == 0, \
        lib.mxm_last_error()
    _sync()
    tied_before, cons_before = tied.get(numpy.uint8), cons.get(numpy.uint8)
    assert (tied_before != 0).sum() > 100
    dev = DeviceAln(cols)
    lab, jn = guarded_from(label, numpy.int32, 4, DEV), guarded_from(joined, numpy.int32, 4, DEV)
    assert lib.mxm_first_observed(ctypes.byref(dev.struct), lab.ptr, jn.ptr, N_LABELS, 30, 30, ref_len, tied.ptr, cons.ptr,
                                  _stream()) == 0, lib.mxm_last_error()
    _sync()
    dev.check("mxm_first_observed")
    for name, buf in (("counts", c_buf), ("label", lab), ("joined", jn), ("tied", tied), ("cons", cons)):
        buf.check("%s ref_len=%d" % (name, ref_len))
    assert numpy.array_equal(tied.get(numpy.uint8), tied_before)
    got = cons.get(numpy.uint8, (N_LABELS, ref_len))
    untied = (tied_before == 0).reshape(N_LABELS, ref_len)
    assert numpy.array_equal(got[untied], cons_before.reshape(N_LABELS, ref_len)[untied])
    for k in range(N_LABELS):
        want = _assemble_ref.consensus(cols, numpy.flatnonzero(label == k), joined.astype(numpy.int64), ref_len, 1, 30, 30, strict=False)
        assert got[k].tobytes().decode() == want, k


# ---- mxm_extend_assign ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, -100])
def test_extend_assign_moves_the_fragments_with_one_owner(lib, pile, extra):
    """mixemt_hip.h, mxm_extend_assign: "(1) every alignment with label == unassigned, mapq >= min_mq and a place is walked
    (M / = / X only) ...; its upper-cased character is looked up in newvar[ref_len] ... folded into frag_state[n_frag] ...:
    -1 none, k one owner, -2 several.  (2) Every alignment with label == unassigned -- below min_mq too -- whose fragment has
    ONE owner k gets label rows[k] and joined = round; moved_owner[n_aln] (nullable) = k or -1; n_moved: + the alignments
    moved.  Alignments with another label are never touched."  Mates share a fragment here; extra < 0: alignments run past
    newvar's end.  Reference: the rule of tests/_assemble_ref.py's assign_reads_from_new_vars over the same table."""
    import _assemble_ref
    cols, table_len, label, _, _ = pile
    n_aln, ref_len = len(cols), table_len + extra
    rng = numpy.random.default_rng(11)
    frag = (numpy.arange(n_aln) // 2).astype(numpy.int64)
    n_frag = int(frag.max()) + 1
    unassigned, rows, this_round = 3, [2, 0], 7
    owners = numpy.full((ref_len, 4), -1, dtype=numpy.int8)
    marked = rng.random((ref_len, 4)) < 0.004
    owners[marked] = rng.integers(0, 2, size=int(marked.sum()))
    joined = rng.integers(0, 3, size=n_aln).astype(numpy.int32)
    # the rule
    idx = numpy.flatnonzero(label == unassigned)
    rpos, bins, aln, is_base, passes = _assemble_ref.observations(cols, idx, 30, 30)
    sel = is_base & passes & (bins < 4) & (rpos < ref_len)
    own = owners[rpos[sel], bins[sel]].astype(numpy.int64)
    hit = own >= 0
    lo, hi = numpy.full(n_frag, 2, dtype=numpy.int64), numpy.full(n_frag, -1, dtype=numpy.int64)
    numpy.minimum.at(lo, frag[aln[sel][hit]], own[hit])
    numpy.maximum.at(hi, frag[aln[sel][hit]], own[hit])
    want_state = numpy.where(hi < 0, -1, numpy.where(lo == hi, lo, -2)).astype(numpy.int32)
    move = idx[want_state[frag[idx]] >= 0]
    want_label, want_joined = label.copy(), joined.copy()
    want_label[move] = numpy.array(rows, dtype=numpy.int32)[want_state[frag[move]]]
    want_joined[move] = this_round
    want_owner = numpy.full(n_aln, -1, dtype=numpy.int32)
    want_owner[move] = want_state[frag[move]]
    assert len(move) > 5 and (want_state == -2).any() and (cols.mapq[move] < 30).any()
    # the device
    dev = DeviceAln(cols)
    bufs = {"frag": guarded_from(frag, numpy.int64, 8, DEV), "label": guarded_from(label, numpy.int32, 4, DEV),
            "joined": guarded_from(joined, numpy.int32, 4, DEV), "newvar": guarded_from(owners, numpy.int8, 4, DEV),
            "frag_state": guarded(4 * n_frag, 4, DEV), "moved_owner": guarded(4 * n_aln, 4, DEV),
            "n_moved": guarded_from([9], numpy.uint32, 4, DEV)}
    dev.struct.frag, dev.struct.n_frag = bufs["frag"].ptr, n_frag
    host_rows = (ctypes.c_int32 * len(rows))(*rows)
    assert lib.mxm_extend_assign(ctypes.byref(dev.struct), bufs["label"].ptr, bufs["joined"].ptr, unassigned, N_LABELS, host_rows,
                                 len(rows), this_round, 30, 30, bufs["newvar"].ptr, ref_len, bufs["frag_state"].ptr,
                                 bufs["moved_owner"].ptr, bufs["n_moved"].ptr, _stream()) == 0, lib.mxm_last_error()
    _sync()
    dev.check("mxm_extend_assign")
    for name, buf in bufs.items():
        buf.check("%s ref_len=%d" % (name, ref_len))
    assert numpy.array_equal(bufs["frag_state"].get(numpy.int32), want_state)
    assert numpy.array_equal(bufs["label"].get(numpy.int32), want_label)
    assert numpy.array_equal(bufs["joined"].get(numpy.int32), want_joined)
    assert numpy.array_equal(bufs["moved_owner"].get(numpy.int32), want_owner)
    assert int(bufs["n_moved"].get(numpy.uint32)[0]) == 9 + len(move)
