"""
The host side of the cohort's assembly stage: the two C entries of include/mixemt_hip_assemble_samples.h -- their binding and
what they say when they refuse a call (every row is refused before the first HIP call, so no device is needed; pointers that
are not NULL are never followed) -- the global label plan of assign.assign_reads_many against assign_reads' own rule,
CohortContribReads.sample(s) on host tensors, and the byte budget.
The kernels: tests/test_gpu_assemble_samples.py.
"""
import argparse
import ctypes
import os
import re
import sys

import numpy
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_var_check_host import empty_columns  # noqa: E402

from mixemt_amd import _lib  # noqa: E402

PTR = 0x1000                 # "some pointer": never dereferenced by a row below
NEW, EXT = "mxm_new_variants_samples", "mxm_extend_assign_samples"


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import build
    build.build()
    return _lib.load()


def header_text():
    with open(os.path.join(ROOT, "include", "mixemt_hip_assemble_samples.h")) as fin:
        return fin.read()


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_the_headers_names_are_bound_and_exported(lib):
    raw = header_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mxm_\w+)\s*\(", text)))
    assert declared == sorted(_lib.ASSEMBLE_SAMPLES_SIGNATURES) == sorted([NEW, EXT])
    assert len(lib.mxm_new_variants_samples.argtypes) == len(_lib.ASSEMBLE_SAMPLES_SIGNATURES[NEW][1]) == 10
    assert len(lib.mxm_extend_assign_samples.argtypes) == len(_lib.ASSEMBLE_SAMPLES_SIGNATURES[EXT][1]) == 18
    for name in declared:
        assert name not in _lib.SIGNATURES and name not in _lib.FINISH_SIGNATURES and name not in _lib.VARCHECK_SIGNATURES
    assert '#include "mixemt_hip_assemble_samples.h"' in open(os.path.join(ROOT, "include", "mixemt_hip.h")).read()
    assert int(re.search(r"#define\s+MXM_ASSEMBLE_SAMPLES_MAX_USE\s+(\d+)", text).group(1)) == 127
    from mixemt_amd import build
    assert any(h.endswith("mixemt_hip_assemble_samples.h") for h in build.HDRS)
    assert lib.mxm_version() == 603 == _lib.ABI_VERSION
    # the header says why it stands apart, that the version stays, and which entry waits
    assert "MXM_VERSION 603: the version stays" in raw and "_lib.ASSEMBLE_SAMPLES_SIGNATURES" in raw
    assert raw.count("Refused with -1 WITHOUT touching the device") == 2 and "not meant to be captured" in raw
    blob = open(build.build(), "rb").read()
    for kernel in (b"new_variants_samples_kernel", b"extend_walk_samples_kernel", b"extend_move_samples_kernel"):
        assert kernel in blob


def _i32(vals):
    return None if vals is None else (ctypes.c_int32 * max(len(vals), 1))(*vals)


def call_new(lib, cons=PTR, ld=100, n_rows=6, use=(0, 1, 2, 4, 5), use_ptr=(0, 3, 3, 5), S=3, ref_len=100, newvar=PTR,
             n_new=PTR):
    return lib.mxm_new_variants_samples(cons, ld, n_rows, _i32(use), _i32(use_ptr), S, ref_len, newvar, n_new, None)


def columns(n_aln=5, n_frag=4, frag=PTR, seq=PTR):
    return _lib.AlnColumns(n_aln, n_frag, PTR, PTR, frag, PTR, PTR, PTR, seq, None, None)


def call_ext(lib, cols="default", aln_sample=PTR, label=PTR, joined=PTR, un=(3, -1, 6), use=(0, 1, 2, 4, 5), use_ptr=(0, 3, 3, 5),
             S=3, n_labels=7, rnd=1, newvar=PTR, ref_len=100, frag_state=PTR, moved_owner=None, n_moved=PTR):
    st = columns() if cols == "default" else cols
    return lib.mxm_extend_assign_samples(None if st is None else ctypes.byref(st), aln_sample, label, joined, _i32(un), _i32(use),
                                         _i32(use_ptr), S, n_labels, rnd, 30, 30, newvar, ref_len, frag_state, moved_owner,
                                         n_moved, None)


MANY = tuple(range(128))
NEW_REFUSALS = [
    ("S below 0", dict(S=-1), "S < 0 (-1)"),
    ("ref_len below 0", dict(ref_len=-1), "bad shape (ref_len = -1, ld = 100, n_rows = 6)"),
    ("ld below ref_len", dict(ld=99), "bad shape (ref_len = 100, ld = 99, n_rows = 6)"),
    ("n_rows below 0", dict(n_rows=-2), "bad shape (ref_len = 100, ld = 100, n_rows = -2)"),
    ("no offsets", dict(use_ptr=None), "bad arguments (use_ptr_host is required)"),
    ("offsets start below 0", dict(use_ptr=(-1, 3, 3, 5)), "use_ptr_host[0] = -1 is negative"),
    ("offsets decrease", dict(use_ptr=(0, 3, 2, 5)), "use_ptr_host decreases at sample 1 (2 after 3)"),
    ("128 participants", dict(use=MANY, use_ptr=(0, 0, 128, 128), n_rows=200),
     "sample 1 has 128 participants, at most 127 (an owner is an int8)"),
    ("no participants' table", dict(use=None), "bad arguments (use_host is required)"),
    ("a row at n_rows", dict(use=(0, 1, 6, 4, 5)), "sample 0: participant 6 outside [0, 6)"),
    ("a row below 0", dict(use=(0, 1, 2, 4, -5)), "sample 2: participant -5 outside [0, 6)"),
    ("no cons", dict(cons=None), "bad arguments (cons, newvar and n_new are required)"),
    ("no newvar", dict(newvar=None), "bad arguments (cons, newvar and n_new are required)"),
    ("no counter", dict(n_new=None), "bad arguments (cons, newvar and n_new are required)"),
]

NEED = "bad arguments (label, joined, frag, aln_sample, frag_state, newvar and n_moved are required)"
EXT_REFUSALS = [
    ("no columns", dict(cols=None), "bad arguments"),
    ("n_aln below 0", dict(cols=columns(n_aln=-1)), "bad arguments"),
    ("too many alignments", dict(cols=columns(n_aln=2 ** 31)), "more than 2^31 - 1 alignments (2147483648)"),
    ("a column missing", dict(cols=columns(seq=None)), "ref_start, mapq, cig_ptr, cigar, seq_ptr and seq are required"),
    ("S below 0", dict(S=-1), "S < 0 (-1)"),
    ("n_labels below 0", dict(n_labels=-1), "bad shape (n_labels = -1, ref_len = 100, n_frag = 4, round = 1)"),
    ("ref_len below 0", dict(ref_len=-5), "bad shape (n_labels = 7, ref_len = -5, n_frag = 4, round = 1)"),
    ("n_frag below 0", dict(cols=columns(n_frag=-1)), "bad shape (n_labels = 7, ref_len = 100, n_frag = -1, round = 1)"),
    ("round below 0", dict(rnd=-1), "bad shape (n_labels = 7, ref_len = 100, n_frag = 4, round = -1)"),
    ("no unassigned table", dict(un=None), "bad arguments (unassigned_host is required)"),
    ("no offsets", dict(use_ptr=None), "bad arguments (use_ptr_host is required)"),
    ("offsets start below 0", dict(use_ptr=(-2, 3, 3, 5)), "use_ptr_host[0] = -2 is negative"),
    ("offsets decrease", dict(use_ptr=(0, 3, 5, 4)), "use_ptr_host decreases at sample 2 (4 after 5)"),
    ("128 participants", dict(use=MANY, use_ptr=(0, 128, 128, 128), n_labels=200),
     "sample 0 has 128 participants, at most 127 (an owner is an int8)"),
    ("no participants' table", dict(use=None), "bad arguments (use_host is required)"),
    ("a participant at n_labels", dict(use=(0, 1, 2, 4, 7)), "sample 2: participant 7 outside [0, 7)"),
    ("a participant below 0", dict(use=(-1, 1, 2, 4, 5)), "sample 0: participant -1 outside [0, 7)"),
    ("an unassigned label at n_labels", dict(un=(3, 7, 6)), "sample 1: unassigned label 7 outside [0, 7)"),
    ("no labels", dict(label=None), NEED),
    ("no joined", dict(joined=None), NEED),
    ("no fragment column", dict(cols=columns(frag=None)), NEED),
    ("no samples of the alignments", dict(aln_sample=None), NEED),
    ("no counter", dict(n_moved=None), NEED),
    ("no fragment states", dict(frag_state=None), NEED),
    ("no newvar", dict(newvar=None), NEED),
]


@pytest.mark.parametrize("what,kw,message", NEW_REFUSALS, ids=[r[0] for r in NEW_REFUSALS])
def test_new_variants_samples_refusals_and_their_messages(lib, what, kw, message):
    assert call_new(lib, **kw) == -1, what
    assert lib.mxm_last_error() == ("%s: %s" % (NEW, message)).encode(), what


@pytest.mark.parametrize("what,kw,message", EXT_REFUSALS, ids=[r[0] for r in EXT_REFUSALS])
def test_extend_assign_samples_refusals_and_their_messages(lib, what, kw, message):
    assert call_ext(lib, **kw) == -1, what
    assert lib.mxm_last_error() == ("%s: %s" % (EXT, message)).encode(), what


def test_nothing_to_do_is_not_an_error(lib):
    """No sample, no position, no participant, no alignment: 0 before the device is looked at (the pointers are not real)."""
    assert call_new(lib, S=0, use=None, use_ptr=None) == 0
    assert call_new(lib, ref_len=0, ld=0) == 0
    assert call_new(lib, use=(), use_ptr=(0, 0, 0, 0)) == 0
    assert call_new(lib, use=(9, 9), use_ptr=(2, 2, 2, 2), cons=None) == 0       # (a table whose first offset is not 0)
    assert call_ext(lib, cols=columns(n_aln=0), label=None, joined=None, n_moved=None) == 0
    assert call_ext(lib, cols=columns(n_aln=0), S=0, un=None, use=None, use_ptr=None) == 0


# ---- the global label plan ------------------------------------------------------------------------------------------
def _finished(contribs, row_label):
    """What finish_many returns for a sample, as far as assign_reads_many reads it."""
    from mixemt_amd import assign
    names = [c[0] for c in contribs]
    return {"contribs": contribs, "row_label": numpy.asarray(row_label, dtype=numpy.int32),
            "assigned": assign.AssignedReads(numpy.asarray(row_label, dtype=numpy.int32), names)}


def _cohort_dicts():
    three = [["hap1", "A", 0.5], ["hap2", "B", 0.3], ["hap3", "C", 0.2]]
    return [_finished(three, [0, 2, -1, 2, -1, 0]),                  # hap2 gets no row: it is no key
            _finished([["hap1", "D", 1.0]], [0, 0, 0]),              # one contributor: no 'unassigned' label
            _finished([], []),                                       # no contributor at all
            _finished(three[:2], [1, 1, 0, 1])]                      # two contributors, nothing unassigned


def test_global_label_plan_follows_assign_reads_own_rule():
    from mixemt_amd import assign
    fin = _cohort_dicts()
    n_rows = [6, 3, 2, 4]
    lab0, names, keys, rows = assign._cohort_label_plan(fin, n_rows)
    assert lab0.tolist() == [0, 4, 6, 7, 10] and lab0.dtype == numpy.int64
    for s, f in enumerate(fin):
        contribs = f["contribs"]
        k = len(contribs)
        # assign_reads (assign.py): names = the contributors, then 'unassigned' with two or more; the label of a row is its
        # contributor's ordinal or, unassigned, the number of contributors; the keys are the AssignedReads' in its order
        want_names = [c[0] for c in contribs] + (["unassigned"] if k > 1 else [])
        assert names[s] == want_names, s
        assert rows[s].dtype == numpy.int32 and len(rows[s]) == n_rows[s]
        if k > 1:
            local = numpy.where(f["row_label"] >= 0, f["row_label"], k)
            assert numpy.array_equal(rows[s], lab0[s] + local), s
            assert keys[s] == list(f["assigned"]), s
        assert lab0[s + 1] - lab0[s] == k + 1                        # the 'unassigned' slot is always reserved
    assert keys[0] == ["hap1", "hap3", "unassigned"] and keys[3] == ["hap1", "hap2"]
    assert rows[1].tolist() == [4, 4, 4] and keys[1] == ["hap1"] and names[1] == ["hap1"]
    assert rows[2].tolist() == [-1, -1] and keys[2] == [] and names[2] == []
    with pytest.raises(ValueError, match="sample 0 has 5 rows of fragments and 6 row labels"):
        assign._cohort_label_plan(fin, [5, 3, 2, 4])
    with pytest.raises(ValueError, match="sample 3 has a row label >= its 2 contributors"):
        assign._cohort_label_plan(fin[:3] + [_finished(fin[3]["contribs"], [1, 2, 0, 1])], n_rows)


class FakeColumns(object):
    """What ContribReads and CohortContribReads read of their columns without a device: frag, names and the length."""

    def __init__(self, frag, names):
        self.frag, self.names = numpy.array(frag, dtype=numpy.int64), list(names)

    def __len__(self):
        return len(self.frag)


def test_sample_round_trips_the_labels():
    import torch
    from mixemt_amd import assign
    fin = _cohort_dicts()
    lab0, names, keys, _ = assign._cohort_label_plan(fin, [6, 3, 2, 4])
    parts = [FakeColumns(f, ["r%d" % i for i in range(max(f) + 1)] if f else []) for f in ([0, 1, 1, 2], [0, 0], [], [1, 0, 2])]
    joined_cols = FakeColumns([0, 1, 1, 2, 3, 3, 5, 4, 6], ["n%d" % i for i in range(7)])
    aln0 = [0, 4, 6, 6, 9]
    local = [[0, 3, -1, 2], [0, -1], [], [1, 0, 1]]
    glob = torch.tensor([int(lab0[s]) + v if v >= 0 else -1 for s, part in enumerate(local) for v in part], dtype=torch.int32)
    sample_of = torch.tensor([0] * 4 + [1] * 2 + [3] * 3, dtype=torch.int32)
    cohort = assign.CohortContribReads(parts, joined_cols, aln0, lab0, names, keys, glob, sample_of)
    assert (cohort.n_samples, cohort.n_labels, cohort.n_frag, len(cohort)) == (4, 10, 7, 4)
    assert [cohort.n_contribs(s) for s in range(4)] == [3, 1, 0, 2] and cohort.rounds == [0, 0, 0, 0]
    assert cohort.label_of(0, "unassigned") == 3 and cohort.label_of(1, "unassigned") is None and cohort.label_of(3, "hap2") == 8
    assert cohort.counts().tolist() == [1, 0, 1, 1, 1, 0, 0, 1, 2, 0]
    cohort.joined[2], cohort.joined[7] = 4, 2
    cohort.rounds[3] = 5
    for s in range(4):
        cr = cohort.sample(s)
        assert cr.labels.tolist() == local[s] and cr.labels.dtype == torch.int32, s
        assert cr.names == names[s] and list(cr) == keys[s] and cr.cols is parts[s], s
        back = torch.where(cr.labels >= 0, cr.labels + int(lab0[s]), cr.labels)
        assert back.tolist() == glob[aln0[s]:aln0[s + 1]].tolist(), s
    assert cohort.sample(0).joined.tolist() == [0, 0, 4, 0] and cohort.sample(3).joined.tolist() == [0, 2, 0]
    assert cohort.sample(3).rounds == 5 and cohort.sample(0).count("unassigned") == 1 and cohort.sample(0).count("hap2") == 0
    # a copy: a key looked up on the sample's table, or new labels given to it, leave the cohort alone
    one = cohort.sample(0)
    one["hap2"]
    one.labels[0] = 1
    assert "hap2" in one and cohort.keys[0] == ["hap1", "hap3", "unassigned"] and int(cohort.labels[0]) == 0
    with pytest.raises(IndexError):
        cohort.sample(4)


def test_assign_reads_many_names_its_budget_and_its_arguments():
    from mixemt_amd import assign
    fin = _cohort_dicts()[:2]
    cols = [empty_columns(), empty_columns()]
    reads = [[[]] * 6, [[]] * 3]
    args = argparse.Namespace(min_mq=30)
    assert assign.COHORT_TABLES_BYTES == 4 << 30
    pile = argparse.Namespace(cols=argparse.Namespace(), aln0=numpy.array([0, 0, 0, 0]), dcols=None)
    with pytest.raises(ValueError, match="the pileup's columns are not those of cols_list"):
        assign.assign_reads_many(cols, fin, reads, args, pileup=pile)
    with pytest.raises(ValueError, match=r"\(2 samples, 1 results, 2 lists\)"):
        assign.assign_reads_many(cols, fin[:1], reads, args)
    # six labels (3 + 1 and 1 + 1) over a pileup of 50 positions: raised before any device is asked for
    from mixemt_amd.alignments import AlignmentColumns
    raw = numpy.frombuffer(b"ACGT", dtype=numpy.uint8)
    cols[0] = AlignmentColumns([46], [60], [0], [0, 1], [4 << 4], [0, 4], raw, None, None, ["p"])
    with pytest.raises(ValueError, match=r"assign_reads_many: 6 labels x 50 positions need 19200 bytes of pileup tables, "
                                         r"above the budget of 19199 bytes \(max_bytes\): split the cohort"):
        assign.assign_reads_many(cols, fin, reads, args, max_bytes=19199)
    assert "split the cohort" in assign.assign_reads_many.__doc__ and "same size again" in assign.assign_reads_many.__doc__
