"""
The stream contract of the entries of include/mixemt_hip_bootstrap.h on a side stream that is still BUSY when the library is
called (tests/_busy_stream.py; the checks of tests/test_gpu_stream_contract.py, whose table of cases names the older
headers' entries and stays as it is):
  mxm_bootstrap_weights, mxm_bootstrap_summary   class B: upload host tables on every call (row0_host and s_id_host;
                              ncol_host), only enqueue, not captured -- they return with the gate behind the delay still
                              pending, and their results are right once the stream has drained;
  mxm_em_loop_samples_narrow_boot                class C: it waits, and its header says so.
All three: the busy run's outputs equal the quiet run's bit for bit, with the host tables in pageable and in pinned memory,
overwritten with another problem's tables as soon as the call returns.  S = 3 samples of 33, 64 and 600 rows, B = 5.
"""
import ctypes
import os

import numpy
import pytest

import _bootstrap_ref as ref
import _busy_stream as bs
import _stream_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

BOOT = 5
SEED = 41
F8, I4, I8, U4 = numpy.float64, numpy.int32, numpy.int64, numpy.uint32
IDS, IDS_OTHER = numpy.array([9, 4000000000, 2], dtype=U4), numpy.array([1, 2, 3], dtype=U4)
LOOP_SENTENCE = ("mxm_em_loop_samples_narrow_boot blocks the calling thread (one read-back of the states per launch); state_host "
                 "receives the final states")


def _ws(lib, ld):
    n = max(int(lib.mxm_samples_plan(row0.ctypes.data, 3, None, 0, None)) for row0 in (sc.ROW0, sc.ROW0_OTHER))
    return int(lib.mxm_bootstrap_workspace_bytes(n, 3, BOOT, ld))


def _weights(rec):
    return numpy.random.default_rng(42).integers(0, 4, size=rec.R).astype(F8)


def _replicates(rec):
    """wb [R * B] of the real problem, from the reference."""
    wts = _weights(rec)
    return numpy.concatenate([ref.resample_all(wts[int(lo):int(hi)], SEED, int(IDS[s]), BOOT).reshape(-1)
                              for s, (lo, hi) in enumerate(zip(sc.ROW0[:-1], sc.ROW0[1:]))])


def _thetas(seed):
    rng = numpy.random.default_rng(seed)
    theta = numpy.full((3, BOOT, sc.LD), -numpy.inf)
    for s in range(3):
        theta[s, :, :sc.NCOL[s]] = numpy.log(rng.dirichlet([1.0] * sc.NCOL[s], size=BOOT))
    return theta


def weights_case(lib):
    rec = sc.records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    wts = _weights(rec)
    nbytes = _ws(lib, 0)
    bufs.update({"w": wts, "wb": bs.sentinel(rec.R * BOOT, F8), "state": sc.states(3)})
    decoy = {"w": bs.nan_like(wts)}                                         # (the records are not read: their decoy would change nothing)

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_bootstrap_weights(ctypes.byref(st), h["row0_host"].ctypes.data, 3, BOOT, p["w"], SEED, h["s_id_host"].ctypes.data,
                                         p["wb"], p["state"], p["ws"], nbytes, stream)
    return bs.Case("mxm_bootstrap_weights", "S=3 B=5", "B", call, bufs, decoy, ["wb", "state"], scratch={"ws": nbytes},
                   host={"row0_host": (sc.ROW0, sc.ROW0_OTHER), "s_id_host": (IDS, IDS_OTHER)})


def loop_case(lib):
    rec = sc.records(lib, "samples 66")
    bufs, _ = rec.bufs()
    sub, theta, wb = sc._reduced(rec), _thetas(35), _replicates(rec)
    nbytes = _ws(lib, sc.LD)
    bufs.update({"M": sub, "wb": wb, "props_cur": numpy.exp(theta), "ln_cur": theta, "ln_new": theta.copy(),
                 "state": sc.states(3 * BOOT), "E": bs.sentinel((rec.R, sc.LD), F8)})
    decoy = {"M": bs.nan_like(sub), "wb": bs.nan_like(wb), "props_cur": bs.nan_like(theta), "ln_cur": bs.nan_like(theta),
             "ln_new": bs.nan_like(theta), "state": sc.stopped(3 * BOOT)}

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_em_loop_samples_narrow_boot(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, BOOT, p["M"], sc.LD,
                                                   h["ncol_host"].ctypes.data, p["wb"], p["props_cur"], p["ln_cur"], p["ln_new"],
                                                   p["state"], 0.0, 5, 2, p["E"], p["ws"], nbytes, stream, sc._state_ptr(h))
    return bs.Case("mxm_em_loop_samples_narrow_boot", "S=3 B=5 ld=8", "C", call, bufs, decoy,
                   ["props_cur", "ln_cur", "ln_new", "state", "E"], scratch={"ws": nbytes},
                   host={"row0_host": (sc.ROW0, sc.ROW0_OTHER), "ncol_host": (sc.NCOL, numpy.array([1, 1, 1], dtype=I4))},
                   host_outs=sc._state_host(3 * BOOT))


def summary_case(lib):
    theta = _thetas(36)
    bufs = {"ln_new": theta, "state": sc.stopped(3 * BOOT), "x": bs.sentinel((3, BOOT, sc.LD), F8), "flag": bs.sentinel(3, I4)}
    for name in ("lo", "hi", "mean", "sd"):
        bufs[name] = bs.sentinel((3, sc.LD), F8)
    decoy = {"ln_new": bs.nan_like(theta)}

    def call(p, h, stream):
        return lib.mxm_bootstrap_summary(3, BOOT, sc.LD, h["ncol_host"].ctypes.data, p["ln_new"], p["state"], 0.025, 0.975, p["x"],
                                         p["lo"], p["hi"], p["mean"], p["sd"], p["flag"], stream)
    return bs.Case("mxm_bootstrap_summary", "S=3 B=5 ld=8", "B", call, bufs, decoy, ["x", "lo", "hi", "mean", "sd", "flag"],
                   host={"ncol_host": (sc.NCOL, sc.NCOL_OTHER)})


BUILDERS = {"mxm_bootstrap_weights": weights_case, "mxm_em_loop_samples_narrow_boot": loop_case, "mxm_bootstrap_summary": summary_case}
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


def test_the_header_says_which_entries_enqueue_and_that_the_loop_blocks():
    with open(os.path.join(ROOT, "include", "mixemt_hip_bootstrap.h")) as fin:
        text = " ".join(fin.read().replace(" * ", " ").split())
    assert text.count("STREAM: the entry only enqueues") == 2
    assert "may be changed as soon as the call has returned" in text and "Not meant to be captured" in text
    assert "class B like its siblings, not meant to be captured" in text
    assert LOOP_SENTENCE in text


@pytest.mark.parametrize("entry", sorted(BUILDERS))
def test_quiet_run_reproduces_itself_and_the_decoy_changes_it(lib, entry):
    case, staged, want = prepared(lib, entry)
    assert bs.same(case, bs.quiet_run(lib, staged), want) is None, case.id
    decoyed = bs.quiet_run(lib, staged, decoys=True)
    assert any(not numpy.array_equal(decoyed[k], want[k]) for k in want), "%s: the decoy does not change the output" % case.id
    from mixemt_amd import _lib
    if case.klass == "C":                                         # the loop ran: five iterations of every replicate, E untouched
        states = (_lib.EmState * (3 * BOOT)).from_buffer_copy(want["host:state_host"].tobytes())
        assert [(st.done, st.iters) for st in states] == [(2, 5)] * (3 * BOOT)
        assert (want["E"] == 0xFF).all()
    elif entry == "mxm_bootstrap_weights":                        # the reference's weights, no error code
        rec = sc.records(lib, "samples 66")
        assert numpy.array_equal(want["wb"].view(I8), _replicates(rec).view(I8)) and not want["state"].any()     # (outputs come as bytes)
    else:
        assert want["flag"].view(I4).tolist() == [0, 0, 0] and not numpy.isnan(want["lo"].view(F8).reshape(3, sc.LD)[2, :7]).any()


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
        assert not pending, "%s blocks by its header (%r), but returned with the delay ahead of it pending" % (case.id, LOOP_SENTENCE)
