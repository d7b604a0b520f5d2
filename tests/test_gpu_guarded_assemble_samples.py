"""
The two entries of include/mixemt_hip_assemble_samples.h called through the library handle with every device buffer at its
exact documented size between red zones (tests/_guarded.py): label, joined, moved_owner, aln_sample [n_aln], frag_state
[n_frag], newvar [S][ref_len], n_new / n_moved [S], cons [n_rows][ld], and the alignments' columns.  Shapes: ref_len no
multiple of a block, a last sample without alignments, ld > ref_len.  References: the header's rules restated in numpy
(the extension over tests/_assemble_ref.py's observations, as tests/test_gpu_guarded_alignments.py does for one sample).
"""
import ctypes

import numpy
import pytest

import _assemble_ref
from _guarded import guarded, guarded_from
from _guarded_abi import DEV, load_lib, stream, sync
from test_gpu_guarded_alignments import DeviceAln, _columns, _long_alignments

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _i32(values):
    return (ctypes.c_int32 * max(len(values), 1))(*values)


def test_new_variants_samples(lib):
    """ "cons [n_rows][ld] DEVICE uint8 ...; ld >= ref_len", "newvar [S][ref_len] DEVICE uint32 ...; owner k is the k-th
    participant OF THAT SAMPLE", "n_new [S] DEVICE uint32, ADDED to", "an EMPTY range: ... its newvar row is set to all -1
    and its counter is left alone"."""
    ref_len, ld, n_rows = 777, 801, 7
    assert ref_len % 256 and ld > ref_len
    rng = numpy.random.default_rng(8)
    cons = rng.choice(numpy.frombuffer(b"ACGTN-X", dtype=numpy.uint8), size=(n_rows, ld), p=[0.3, 0.25, 0.2, 0.15, 0.04, 0.03, 0.03])
    cons[:, ref_len:] = 0xFF                                         # the pad columns take no part
    use, use_ptr = [6, 0, 2, 5, 3, 1], [0, 3, 6, 6]                   # the last sample takes no part
    bufs = {"cons": guarded_from(cons, numpy.uint8, 1, DEV), "newvar": guarded(4 * 3 * ref_len, 4, DEV),
            "n_new": guarded_from([5, 6, 7], numpy.uint32, 4, DEV)}
    assert lib.mxm_new_variants_samples(bufs["cons"].ptr, ld, n_rows, _i32(use), _i32(use_ptr), 3, ref_len, bufs["newvar"].ptr,
                                        bufs["n_new"].ptr, stream()) == 0, lib.mxm_last_error()
    sync()
    for name, buf in bufs.items():
        buf.check(name)
    got = bufs["newvar"].get(numpy.int8, (3, ref_len, 4))
    n_new = bufs["n_new"].get(numpy.uint32)
    for s in range(3):
        rows = use[use_ptr[s]:use_ptr[s + 1]]
        want = numpy.full((ref_len, 4), -1, dtype=numpy.int8)
        for pos in range(ref_len if rows else 0):
            col = [chr(cons[r, pos]) for r in rows]
            if all(c in "ACGT" for c in col):
                for k, c in enumerate(col):
                    if col.count(c) == 1:
                        want[pos, "ACGT".index(c)] = k
        assert numpy.array_equal(got[s], want), s
        assert int(n_new[s]) == 5 + s + int((want >= 0).sum()) and (s == 2 or (want >= 0).any()), s


def test_extend_assign_samples(lib):
    """ "aln_sample [n_aln] DEVICE int32", "label, joined [n_aln] DEVICE int32, updated in place", "newvar [S][ref_len]",
    "frag_state [n_frag] DEVICE int32 scratch, reset by the call", "moved_owner [n_aln] ... the GLOBAL label an alignment
    moved to, or -1", "n_moved [S] DEVICE uint32, ADDED to".  Two samples of mates that share a fragment and a last sample
    without alignments; sample 1's table differs from sample 0's; alignments run past the end of a newvar row."""
    alns, table_len = _long_alignments(5)
    cols = _columns(alns)
    n_aln, ref_len, n_samples, this_round = len(cols), table_len - 100, 3, 4
    assert ref_len % 256
    rng = numpy.random.default_rng(12)
    sample = (numpy.arange(n_aln) >= 150).astype(numpy.int32)
    frag = (numpy.arange(n_aln) // 2).astype(numpy.int64)
    n_frag = int(frag.max()) + 1
    lab0 = numpy.array([0, 3, 6])                                     # per sample: two contributors, then 'unassigned'
    local = rng.integers(-1, 3, size=n_aln)
    label = numpy.where(local >= 0, local + lab0[sample], -1).astype(numpy.int32)
    joined = rng.integers(0, 3, size=n_aln).astype(numpy.int32)
    use, use_ptr, un = [1, 0, 3, 4, 6], [0, 2, 4, 5], [2, 5, 8]       # (sample 0's owners in the other order)
    owners = numpy.full((n_samples, ref_len, 4), -1, dtype=numpy.int8)
    for s in range(2):
        marked = rng.random((ref_len, 4)) < 0.004
        owners[s][marked] = rng.integers(0, 2, size=int(marked.sum()))
    owners[2] = 0                                                     # nobody looks a base up here
    # the rule, per sample over its own unassigned alignments and its own row
    want_state = numpy.full(n_frag, -1, dtype=numpy.int32)
    want_label, want_joined = label.copy(), joined.copy()
    want_owner = numpy.full(n_aln, -1, dtype=numpy.int32)
    moved = [0, 0, 0]
    for s in range(2):
        idx = numpy.flatnonzero((sample == s) & (label == un[s]))
        rpos, bins, aln, is_base, passes = _assemble_ref.observations(cols, idx, 30, 30)
        sel = is_base & passes & (bins < 4) & (rpos < ref_len)
        own = owners[s][rpos[sel], bins[sel]].astype(numpy.int64)
        hit = own >= 0
        lo, hi = numpy.full(n_frag, 2, dtype=numpy.int64), numpy.full(n_frag, -1, dtype=numpy.int64)
        numpy.minimum.at(lo, frag[aln[sel][hit]], own[hit])
        numpy.maximum.at(hi, frag[aln[sel][hit]], own[hit])
        rows = numpy.array(use[use_ptr[s]:use_ptr[s + 1]], dtype=numpy.int32)
        state = numpy.where(hi < 0, -1, numpy.where(lo == hi, rows[numpy.minimum(lo, 1)], -2)).astype(numpy.int32)
        mine = numpy.unique(frag[sample == s])
        want_state[mine] = state[mine]
        move = idx[state[frag[idx]] >= 0]
        want_label[move] = state[frag[move]]
        want_joined[move] = this_round
        want_owner[move] = state[frag[move]]
        moved[s] = len(move)
        assert (cols.mapq[move] < 30).any(), s                     # (alignments below min_mq move with their fragment)
    assert moved[0] > 2 and moved[1] > 2 and (want_state == -2).any()
    dev = DeviceAln(cols)
    bufs = {"frag": guarded_from(frag, numpy.int64, 8, DEV), "aln_sample": guarded_from(sample, numpy.int32, 4, DEV),
            "label": guarded_from(label, numpy.int32, 4, DEV), "joined": guarded_from(joined, numpy.int32, 4, DEV),
            "newvar": guarded_from(owners, numpy.int8, 4, DEV), "frag_state": guarded(4 * n_frag, 4, DEV),
            "moved_owner": guarded(4 * n_aln, 4, DEV), "n_moved": guarded_from([9, 8, 7], numpy.uint32, 4, DEV)}
    dev.struct.frag, dev.struct.n_frag = bufs["frag"].ptr, n_frag
    assert lib.mxm_extend_assign_samples(ctypes.byref(dev.struct), bufs["aln_sample"].ptr, bufs["label"].ptr, bufs["joined"].ptr,
                                         _i32(un), _i32(use), _i32(use_ptr), n_samples, 9, this_round, 30, 30, bufs["newvar"].ptr,
                                         ref_len, bufs["frag_state"].ptr, bufs["moved_owner"].ptr, bufs["n_moved"].ptr,
                                         stream()) == 0, lib.mxm_last_error()
    sync()
    dev.check("mxm_extend_assign_samples")
    for name, buf in bufs.items():
        buf.check(name)
    assert numpy.array_equal(bufs["frag_state"].get(numpy.int32), want_state)
    assert numpy.array_equal(bufs["label"].get(numpy.int32), want_label)
    assert numpy.array_equal(bufs["joined"].get(numpy.int32), want_joined)
    assert numpy.array_equal(bufs["moved_owner"].get(numpy.int32), want_owner)
    assert bufs["n_moved"].get(numpy.uint32).tolist() == [9 + moved[0], 8 + moved[1], 7]
    # a frozen sample: nothing of it is walked or moved, moved_owner is -1 throughout
    bufs["label"].put(label)
    bufs["joined"].put(joined)
    assert lib.mxm_extend_assign_samples(ctypes.byref(dev.struct), bufs["aln_sample"].ptr, bufs["label"].ptr, bufs["joined"].ptr,
                                         _i32([-1, 5, -1]), _i32(use), _i32(use_ptr), n_samples, 9, this_round, 30, 30,
                                         bufs["newvar"].ptr, ref_len, bufs["frag_state"].ptr, bufs["moved_owner"].ptr,
                                         bufs["n_moved"].ptr, stream()) == 0, lib.mxm_last_error()
    sync()
    for name, buf in bufs.items():
        buf.check(name + " (sample 0 frozen)")
    first = sample == 0
    assert numpy.array_equal(bufs["label"].get(numpy.int32)[first], label[first])
    assert numpy.array_equal(bufs["joined"].get(numpy.int32)[first], joined[first])
    assert (bufs["moved_owner"].get(numpy.int32)[first] == -1).all()
    assert numpy.array_equal(bufs["label"].get(numpy.int32)[~first], want_label[~first])
    assert bufs["n_moved"].get(numpy.uint32).tolist() == [9 + moved[0], 8 + 2 * moved[1], 7]
