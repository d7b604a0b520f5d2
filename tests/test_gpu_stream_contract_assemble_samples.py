"""
The stream contract of the two entries of include/mixemt_hip_assemble_samples.h on a side stream that is still BUSY when the
library is called (tests/_busy_stream.py; the checks of tests/test_gpu_stream_contract.py, whose table of cases names the
older headers' entries and stays as it is):
  mxm_new_variants_samples    class B: uploads host tables into stream-ordered memory, only enqueues, not captured -- it
                              returns with the gate behind the delay still pending, and its result is right once the stream
                              has drained;
  mxm_extend_assign_samples   class C: its header says that it waits.
Both: the busy run's outputs equal the quiet run's bit for bit, with the host tables in pageable and in pinned memory,
overwritten with another problem's tables as soon as the call returns.
"""
import ctypes
import os

import numpy
import pytest

import _busy_stream as bs
import _stream_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

I4, U1 = numpy.int32, numpy.uint8
WAITS = "HOST, blocking: like mxm_extend_assign this entry waits for its work on `stream` and reads the error word"


def _ptr(arr):
    return arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def new_variants_case(lib):
    rng = numpy.random.default_rng(31)
    n_rows, ref_len, ld = 6, 3001, 3008
    letters = numpy.frombuffer(b"ACGTN", dtype=U1)
    cons = letters[rng.choice(5, size=(n_rows, ld), p=[0.3, 0.25, 0.2, 0.2, 0.05])]
    other = letters[rng.choice(5, size=(n_rows, ld), p=[0.3, 0.25, 0.2, 0.2, 0.05])]
    use, use_other = numpy.array([0, 1, 2, 3, 4], dtype=I4), numpy.array([5, 4, 3, 2, 1], dtype=I4)
    use_ptr, ptr_other = numpy.array([0, 2, 2, 5], dtype=I4), numpy.array([0, 1, 4, 5], dtype=I4)
    bufs = {"cons": cons, "newvar": bs.sentinel((3, ref_len), numpy.uint32), "n_new": numpy.array([11, 12, 13], dtype=numpy.uint32)}

    def call(p, h, stream):
        return lib.mxm_new_variants_samples(p["cons"], ld, n_rows, _ptr(h["use_host"]), _ptr(h["use_ptr_host"]), 3, ref_len,
                                            p["newvar"], p["n_new"], stream)
    return bs.Case("mxm_new_variants_samples", "S=3, one sample without participants", "B", call, bufs,
                   {"cons": other, "n_new": numpy.array([99, 98, 97], dtype=numpy.uint32)}, ["newvar", "n_new"],
                   host={"use_host": (use, use_other), "use_ptr_host": (use_ptr, ptr_other)})


def extend_assign_case(lib):
    cols, label, table_len, dec = sc.alignments()
    n_aln, n_frag = len(label), 750
    rng = numpy.random.default_rng(32)
    sample = (cols.frag >= n_frag // 2).astype(I4)                    # a fragment's alignments are one sample's
    to_global = lambda lab: numpy.where(lab >= 0, lab + 4 * sample, -1).astype(I4)        # noqa: E731
    owners = numpy.full((2, table_len, 4), -1, dtype=numpy.int8)
    for s, n_use in enumerate((3, 2)):
        marked = rng.random(owners[s].shape) < 0.02
        owners[s][marked] = rng.integers(0, n_use, size=int(marked.sum()))
    joined = rng.integers(0, 3, size=n_aln).astype(I4)
    bufs = sc._aln_bufs(cols, with_frag=True)
    bufs.update({"aln_sample": sample, "label": to_global(label), "joined": joined, "newvar": owners,
                 "frag_state": bs.sentinel(n_frag, I4), "moved_owner": bs.sentinel(n_aln, I4),
                 "n_moved": numpy.array([9, 8], dtype=numpy.uint32)})
    decoy = {k: dec[k] for k in ("seq", "qual", "mapq")}
    decoy["label"] = to_global(dec["label"])
    decoy["joined"] = (2 - joined).astype(I4)
    decoy["n_moved"] = numpy.array([1000, 2000], dtype=numpy.uint32)
    host = {"unassigned_host": (numpy.array([3, 7], dtype=I4), numpy.array([-1, 7], dtype=I4)),
            "use_host": (numpy.array([2, 0, 1, 4, 6], dtype=I4), numpy.array([1, 2, 0, 6, 5], dtype=I4)),
            "use_ptr_host": (numpy.array([0, 3, 5], dtype=I4), numpy.array([0, 2, 5], dtype=I4))}

    def call(p, h, stream):
        st = sc._aln_struct(p, cols, n_frag)
        return lib.mxm_extend_assign_samples(ctypes.byref(st), p["aln_sample"], p["label"], p["joined"], _ptr(h["unassigned_host"]),
                                             _ptr(h["use_host"]), _ptr(h["use_ptr_host"]), 2, 8, 7, 30, 30, p["newvar"], table_len,
                                             p["frag_state"], p["moved_owner"], p["n_moved"], stream)
    return bs.Case("mxm_extend_assign_samples", "1500 alignments of 750 fragments, two samples", "C", call, bufs, decoy,
                   ["label", "joined", "frag_state", "moved_owner", "n_moved"], host=host)


BUILDERS = {"mxm_new_variants_samples": new_variants_case, "mxm_extend_assign_samples": extend_assign_case}
_prepared = {}


@pytest.fixture(scope="module")
def lib():
    return bs.load_lib()


def prepared(lib, entry):
    """(case, staging tensors, the quiet run's outputs), made once per entry; the quiet run is also the warm-up."""
    if entry not in _prepared:
        case = BUILDERS[entry](lib)
        staged = bs.Staged(case)
        _prepared[entry] = (case, staged, bs.quiet_run(lib, staged))
    return _prepared[entry]


def test_the_header_says_which_entry_waits():
    with open(os.path.join(ROOT, "include", "mixemt_hip_assemble_samples.h")) as fin:
        text = " ".join(fin.read().replace(" * ", " ").split())
    assert WAITS in text
    assert "The call only enqueues on `stream`; nothing is waited for." in text and "not meant to be captured" in text


@pytest.mark.parametrize("entry", sorted(BUILDERS))
def test_quiet_run_reproduces_itself_and_the_decoy_changes_it(lib, entry):
    case, staged, want = prepared(lib, entry)
    assert bs.same(case, bs.quiet_run(lib, staged), want) is None, case.id
    decoyed = bs.quiet_run(lib, staged, decoys=True)
    assert any(not numpy.array_equal(decoyed[k], want[k]) for k in want), "%s: the decoy does not change the output" % case.id
    counter = "n_moved" if entry == "mxm_extend_assign_samples" else "n_new"
    counted = want[counter].view(numpy.uint32).astype(numpy.int64) - case.bufs[counter].astype(numpy.int64)
    assert counted.max() > 0 and counted.min() >= 0, (case.id, counted)                   # (something was counted)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("entry", sorted(BUILDERS))
def test_busy_stream(lib, entry, pinned):
    case, staged, want = prepared(lib, entry)
    outs, snaps, host_ms, pending = bs.busy_run(lib, staged, pinned)
    print("%s: class %s, %.3f ms of host time, gate %s at return" % (case.id, case.klass, host_ms, "pending" if pending else "passed"))
    bad = bs.same(case, outs, want)
    assert bad is None, "%s: output %r differs from the quiet run's" % (case.id, bad)
    for name in case.outs:
        assert numpy.array_equal(snaps[name], outs[name]), "%s: %r changed after the snapshot that follows the call" % (case.id, name)
    if case.klass == "B":
        assert pending, "%s only enqueues by its header, but the %g ms delay ahead of it had passed when it returned" % (
            case.id, case.delay_ms)
        assert host_ms < case.delay_ms / 2, "%s only enqueues by its header, but took %.1f ms of host time" % (case.id, host_ms)
    else:
        assert not pending, "%s waits by its header (\"%s ...\"), but returned with the stream's work pending" % (case.id, WAITS)
