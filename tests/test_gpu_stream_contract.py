"""
The second convention of include/mixemt_hip.h -- "`stream` is a hipStream_t ...; every call only enqueues work on it unless
stated otherwise" -- for every entry that takes a stream, on a side stream that is still BUSY when the library is called
(tests/_busy_stream.py; the cases: tests/_stream_cases.py).  Everywhere else in the suite the stream is idle at the call,
so a kernel or memset launched on nullptr, a host read of a device value that is not there yet, a silent synchronise or
work on a private stream without its event still give right answers there.  One parametrised test per check:

  * the quiet run reproduces itself bit for bit, and the quiet run on the decoys gives another output (a decoy that
    cannot change the result proves nothing);
  * the busy run (until the copies behind the delay arrive, every input with a payload holds its decoy and every other
    buffer -- offsets, codes, row lists -- is itself), host arrays in pageable memory: outputs equal the quiet run's, the
    snapshots enqueued straight after the call equal the final outputs (nothing of the call lands behind its place in
    the stream), and for an entry that must only enqueue (classes A and B) the gate behind the 200 ms delay is still
    pending at return and the call took less than half the delay of host time;
  * the same with the host arrays in pinned memory (where a host-to-device copy really is asynchronous), overwritten
    with another problem's tables as soon as the call returns;
  * class A: the call captured into a graph on one stream and replayed once;
  * two side streams from one host thread, each with its own buffers and workspace, both behind their delays.
"""
import numpy
import pytest

import _busy_stream as bs
import _stream_cases as sc

pytestmark = pytest.mark.gpu

IDS = sc.ids()
_prepared = {}


@pytest.fixture(scope="module")
def lib():
    handle = bs.load_lib()
    yield handle
    sc.close_exchange()


def prepared(lib, index):
    """(case, staging tensors, the quiet run's outputs): made once per case; the quiet run is also the warm-up that keeps
    lazy code-object loading out of the busy call."""
    if index not in _prepared:
        case = sc.TABLE[index][3](lib)
        staged = bs.Staged(case)
        _prepared[index] = (case, staged, bs.quiet_run(lib, staged))
    return _prepared[index]


def agree(case, got, want, what):
    bad = bs.same(case, case.canon(got), case.canon(want))
    assert bad is None, "%s: output %r differs from the quiet run's (%s)" % (case.id, bad, what)


@pytest.mark.parametrize("index", range(len(sc.TABLE)), ids=IDS)
def test_quiet_run_reproduces_itself_and_the_decoy_changes_it(lib, index):
    case, staged, want = prepared(lib, index)
    again = bs.quiet_run(lib, staged)
    bad = bs.same(case, case.canon(again), case.canon(want))
    assert bad is None, "%s: output %r of a second quiet run differs" % (case.id, bad)
    decoyed, real = case.canon(bs.quiet_run(lib, staged, decoys=True)), case.canon(want)
    assert any(not numpy.array_equal(decoyed[k], real[k]) for k in real), "%s: the decoy does not change the output" % case.id


def check_busy(lib, index, pinned):
    case, staged, want = prepared(lib, index)
    outs, snaps, host_ms, pending = bs.busy_run(lib, staged, pinned)
    what = "busy stream, %s host arrays" % ("pinned" if pinned else "pageable")
    print("%s: class %s, %.3f ms of host time, gate %s at return (%s)" % (case.id, case.klass, host_ms,
                                                                       "pending" if pending else "passed", what))
    agree(case, outs, want, what)
    for name in case.outs:
        assert numpy.array_equal(snaps[name], outs[name]), \
            "%s: %r changed after the snapshot that follows the call on its stream (%s)" % (case.id, name, what)
    if case.klass in ("A", "B"):
        assert pending, "%s only enqueues by its header, but the %g ms delay ahead of it had passed when it returned" % (
            case.id, case.delay_ms)
        assert host_ms < case.delay_ms / 2, "%s only enqueues by its header, but took %.1f ms of host time" % (case.id, host_ms)


@pytest.mark.parametrize("index", range(len(sc.TABLE)), ids=IDS)
def test_busy_stream(lib, index):
    check_busy(lib, index, pinned=False)


WITH_HOST_ARRAYS = [i for i, (entry, _, _, _) in enumerate(sc.TABLE) if entry in sc.HOST_ARRAY_ENTRIES]


@pytest.mark.parametrize("index", WITH_HOST_ARRAYS, ids=[IDS[i] for i in WITH_HOST_ARRAYS])
def test_busy_stream_with_pinned_host_arrays(lib, index):
    case = prepared(lib, index)[0]
    assert case.host, "%s takes host arrays: its case must name them" % case.id
    check_busy(lib, index, pinned=True)


def test_every_case_with_host_arrays_is_listed(lib):
    """HOST_ARRAY_ENTRIES is what selects the pinned runs without building a case: it must be the truth."""
    for index, (entry, _, _, _) in enumerate(sc.TABLE):
        assert bool(prepared(lib, index)[0].host) == (entry in sc.HOST_ARRAY_ENTRIES), IDS[index]


CLASS_A = [i for i, (_, _, klass, _) in enumerate(sc.TABLE) if klass == "A"]


@pytest.mark.parametrize("index", CLASS_A, ids=[IDS[i] for i in CLASS_A])
def test_captured_and_replayed(lib, index):
    case, staged, want = prepared(lib, index)
    agree(case, bs.graph_run(lib, staged), want, "captured on one stream, replayed once")


TWO_STREAMS = ("mxm_em_iter", "mxm_em_iter_coded", "mxm_observe_bases_labelled", "mxm_check_variants_samples")


@pytest.mark.parametrize("entry", TWO_STREAMS)
def test_two_side_streams_from_one_thread(lib, entry):
    """The workspace, the stream-ordered pools and the tuning snapshot: the same case on two side streams, each with its
    own buffers, both behind their delays so that the work overlaps.  (The one-launch loops stay out: two persistent
    grids that each want the whole chip would only starve each other into the documented give-up route.)"""
    import torch
    index = next(i for i, row in enumerate(sc.TABLE) if row[0] == entry)
    case, staged, want = prepared(lib, index)
    runs = [bs.BusyRun(lib, staged), bs.BusyRun(lib, staged)]
    for run in runs:
        run.stage()
    torch.cuda.synchronize()
    for run in runs:
        run.enqueue_delay()
    for run in runs:
        run.call()
    for k, run in enumerate(runs):
        outs, snaps = run.finish()
        agree(case, outs, want, "stream %d of two" % k)
        for name in case.outs:
            assert numpy.array_equal(snaps[name], outs[name]), (case.id, name, k)
