"""
The device pileup (mxm_observe_bases, csrc/observe_kernels.hpp) against the reference's ObservedBases table (g16) and
the numpy restatement (tests/_pileup_ref.py), and the variant check on the records route.
"""
import argparse
import ctypes
import os
import sys
import tempfile

import numpy
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pileup_ref  # noqa: E402
from test_observe import asm_args, g16_columns, g16_table, want_contribs  # noqa: E402

pytestmark = pytest.mark.gpu


def _subset(cols, idx):
    """Columns of the alignments idx (in that order)."""
    from mixemt_amd.alignments import AlignmentColumns

    def ragged(ptr, data):
        lens = numpy.diff(ptr)[idx]
        new_ptr = numpy.zeros(len(idx) + 1, dtype=numpy.int64)
        numpy.cumsum(lens, out=new_ptr[1:])
        gather = numpy.repeat(ptr[:-1][idx], lens) + numpy.arange(int(lens.sum())) - numpy.repeat(new_ptr[:-1], lens)
        return new_ptr, data[gather]

    cig_ptr, cigar = ragged(cols.cig_ptr, cols.cigar)
    seq_ptr, seq = ragged(cols.seq_ptr, cols.seq)
    qual = None if cols.qual is None else ragged(cols.seq_ptr, cols.qual)[1]
    return AlignmentColumns(cols.ref_start[idx], cols.mapq[idx], cols.frag[idx], cig_ptr, cigar, seq_ptr, seq, qual,
                            None if cols.has_qual is None else cols.has_qual[idx], cols.names,
                            None if cols.is_reverse is None else cols.is_reverse[idx])


def test_device_pileup_equals_the_reference_table():
    import torch
    from mixemt_amd import observe
    g = golden("g16_observe")
    cols = g16_columns(g)
    obs = observe.observe_bases(cols, 30, 30, ref_len=16569)
    assert obs.counts.shape == (16589, 16)
    want = g16_table(g, 16589)
    assert numpy.array_equal(obs.counts.astype(numpy.int64), want)
    assert not obs.counts[:, 14:].any()
    # shuffled, and split over two calls into one table: the same bits
    perm = numpy.random.default_rng(5).permutation(len(cols))
    counts = torch.zeros((16589, 16), dtype=torch.int32, device="cuda")
    for part in (perm[: len(perm) // 3], perm[len(perm) // 3:]):
        observe.count_bases(observe.DeviceColumns(_subset(cols, part)), counts, 30, 30)
    assert numpy.array_equal(counts.cpu().numpy().astype(numpy.int64), want)


def test_bam_route_equals_the_column_route():
    import _bam_writer
    from mixemt_amd import alignments, observe, phylotree, preprocess, synth
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    tables = preprocess.HapVarTables.build(refseq, phy, sorted(phy.hap_var))
    cols = synth.synth_alignments(tables, refseq, 3000, seed=9)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "s.bam")
        _bam_writer.write_bam(path, cols, flag=cols.is_reverse.astype(numpy.int64) * 0x10)
        back = alignments.read_bam(path, n_threads=2)
        from_bam = observe.observe_bases(back, 30, 30, ref_len=len(refseq))
    from_cols = observe.observe_bases(cols, 30, 30, ref_len=len(refseq))
    assert from_bam.counts.sum() > 0 and numpy.array_equal(from_bam.counts, from_cols.counts)


def test_million_fragments_equal_the_numpy_restatement():
    from mixemt_amd import observe, phylotree, preprocess, synth
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    tables = preprocess.HapVarTables.build(refseq, phy, sorted(phy.hap_var))
    cols = synth.synth_alignments(tables, refseq, 1000000, seed=1)
    obs = observe.observe_bases(cols, 30, 30, ref_len=len(refseq))
    want = _pileup_ref.pileup(cols, obs.counts.shape[0], 30, 30)
    assert int(want.sum()) > 10 ** 8
    assert numpy.array_equal(obs.counts.astype(numpy.int64), want)


def _one(start, cigar, seq, mapq=60, rev=0):
    from mixemt_amd.alignments import AlignmentColumns
    raw = numpy.frombuffer(seq.encode(), dtype=numpy.uint8)
    return AlignmentColumns([start], [mapq], [0], [0, len(cigar)], [(n << 4) | op for op, n in cigar], [0, len(raw)],
                            raw, None, None, ["r"], [rev])


def test_table_grows_past_ref_len_and_empty_inputs_give_zeros():
    from mixemt_amd import observe
    from mixemt_amd.alignments import AlignmentColumns
    obs = observe.observe_bases(_one(95, [(0, 10)], "ACGTNRacgt", rev=1), ref_len=100)
    assert obs.counts.shape == (105, 16)
    assert obs.obs_at(104, "t", stranded=True) == (0, 1) and obs.obs_at(99, "N", stranded=True) == (0, 1)
    assert obs.obs_at(100, stranded=True) == {"x": 1}
    empty = AlignmentColumns([], [], [], [0], [], [0], numpy.zeros(0, numpy.uint8), None, None, [])
    assert observe.observe_bases(empty, ref_len=50).counts.shape == (50, 16)
    assert not observe.observe_bases(empty, ref_len=50).counts.any()
    filtered = observe.observe_bases(_one(10, [(0, 4)], "ACGT", mapq=29), ref_len=50)
    unplaced = observe.observe_bases(_one(-1, [(0, 4)], "ACGT"), ref_len=50)
    assert not filtered.counts.any() and not unplaced.counts.any()


def test_bad_cigar_is_minus_4_with_the_message():
    import torch
    from mixemt_amd import _lib, observe
    lib = _lib.load()
    for cigar, what in (([(0, 10)], "runs past its sequence"), ([(0, 2), (9, 1)], "unknown operation")):
        dcols = observe.DeviceColumns(_one(10, cigar, "ACGT"))
        counts = torch.zeros((64, 16), dtype=torch.int32, device="cuda")
        st = dcols.struct()
        rc = lib.mxm_observe_bases(ctypes.byref(st), None, 30, 30, 64, counts.data_ptr(), None)
        assert rc == -4
        assert what in lib.mxm_last_error().decode()
        with pytest.raises(ValueError, match=what):
            observe.count_bases(dcols, counts)
    # a table too short for the alignment: -1, nothing written out of bounds
    dcols = observe.DeviceColumns(_one(60, [(0, 4)], "ACGT"))
    counts = torch.zeros((62, 16), dtype=torch.int32, device="cuda")
    st = dcols.struct()
    assert lib.mxm_observe_bases(ctypes.byref(st), None, 30, 30, 62, counts.data_ptr(), None) == -1


def test_records_route_with_the_check_gives_the_reference_contributors():
    from mixemt_amd import alignments, assign, em, observe, phylotree, preprocess
    g = golden("g16_observe")
    refseq = phylotree.load_rsrs()
    phy = phylotree.load_build17(refseq)
    haps = sorted(phy.hap_var)
    tables = preprocess.HapVarTables.build(refseq, phy, haps)
    cols = g16_columns(g)
    # the EM input without the unplaced alignment (the stand-in gives it no aligned pairs; the front end is not what is
    # under test here, and a BAM file's unplaced records never reach it)
    placed = _subset(cols, numpy.flatnonzero(cols.ref_start >= 0))
    enc = alignments.encode_alignments(placed, tables.sites, len(refseq), 30, 30)
    assert enc.signatures() == [s for s in str(g["signatures"]).split("\n") if s]
    cm = preprocess.build_em_records_device(tables, enc.row_ptr, enc.site, enc.obs)
    args = argparse.Namespace(init_alpha=1.0, tolerance=1e-4, max_iter=10000, n_multi=1, verbose=False)
    import torch
    numpy.random.seed(int(g["seeds"][1]))
    wts = torch.from_numpy(enc.weights).to(device="cuda", dtype=torch.float64)
    res = em.run_em_ex(None, wts, args, want_read_mix=False, records=cm)
    assert numpy.abs(res["props"] - g["props"]).max() < 1e-6
    obs = observe.observe_bases(cols, 30, 30, ref_len=len(refseq))
    got = assign.get_contributors_records(phy, obs, haps, enc.weights, res["props"], cm, res["ln_theta_k"], asm_args())
    want = want_contribs(g, "default")
    assert [c[:2] for c in got] == [w[:2] for w in want]
    assert numpy.allclose([c[2] for c in got], [float(w[2]) for w in want], rtol=0, atol=1e-6)
