"""
The stream contract of the entries of include/mixemt_hip_samples_runs.h on a side stream that is still BUSY when the library
is called (tests/_busy_stream.py; the checks of tests/test_gpu_stream_contract.py, whose table of cases names the older
headers' entries and stays as it is):
  mxm_votes_samples_runs, mxm_assign_reads_samples_runs   class B: upload host tables on every call, only enqueue, not
                              captured -- they return with the gate behind the delay still pending, and their results
                              are right once the stream has drained;
  mxm_em_loop_samples_narrow_runs                         class C: it waits, and its header says so.
All three: the busy run's outputs equal the quiet run's bit for bit, with the host tables in pageable and in pinned memory,
overwritten with another problem's tables as soon as the call returns.  S = 3 samples of 33, 64 and 600 rows, B = 3.
"""
import ctypes
import os

import numpy
import pytest

import _busy_stream as bs
import _stream_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

RUNS = 3
F8, I4, I8 = numpy.float64, numpy.int32, numpy.int64
LOOP_SENTENCE = ("mxm_em_loop_samples_narrow_runs blocks the calling thread (one read-back of the states per launch); state_host "
                 "receives the final states")


def _ws(lib, ld):
    n = max(int(lib.mxm_samples_plan(row0.ctypes.data, 3, None, 0, None)) for row0 in (sc.ROW0, sc.ROW0_OTHER))
    return int(lib.mxm_samples_runs_workspace_bytes(n, 3, RUNS, ld))


def _thetas(seed):
    rng = numpy.random.default_rng(seed)
    theta = numpy.zeros((3, RUNS, sc.LD))
    for s in range(3):
        theta[s, :, :sc.NCOL[s]] = numpy.log(rng.dirichlet([1.0] * sc.NCOL[s], size=RUNS))
    return theta


def votes_case(lib):
    rec = sc.records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    props = sc.props_of(rec.H, 3 * RUNS, 31).reshape(3, RUNS, rec.H)
    nbytes = _ws(lib, 0)
    bufs.update({"w": rec.wts + 0.25, "ln_props": numpy.log(props), "props": props, "rowmax": rec.rowmax,
                 "best": bs.sentinel(rec.R, I4), "votes": bs.sentinel((3, rec.H), F8), "counts": bs.sentinel((3, rec.H), I8),
                 "first": bs.sentinel((3, rec.H), I8), "lse": bs.sentinel((rec.R, RUNS), F8), "state": sc.states(3)})
    decoy.update({"w": bs.nan_like(rec.wts), "ln_props": bs.nan_like(props), "props": bs.nan_like(props),
                  "rowmax": bs.nan_like(rec.rowmax)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_votes_samples_runs(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, RUNS, p["w"], p["ln_props"], p["props"],
                                          p["rowmax"], p["best"], p["votes"], p["counts"], p["first"], p["lse"], p["state"], p["ws"],
                                          nbytes, stream)
    return bs.Case("mxm_votes_samples_runs", "S=3 B=3 with counts and lse", "B", call, bufs, decoy,
                   ["best", "votes", "counts", "first", "lse", "state"], scratch={"ws": nbytes},
                   host={"row0_host": (sc.ROW0, sc.ROW0_OTHER)})


def assign_case(lib):
    rec = sc.records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    sub, theta_k = sc._reduced(rec), _thetas(32)
    log_props = _thetas(33)[:, 0, :].copy()
    nbytes = _ws(lib, sc.LD)
    rng = numpy.random.default_rng(34)
    perm, other = numpy.zeros((3, sc.LD), dtype=I4), numpy.zeros((3, sc.LD), dtype=I4)
    for s in range(3):
        perm[s, :sc.NCOL[s]] = rng.permutation(sc.NCOL[s])
        other[s, :sc.NCOL[s]] = perm[s, :sc.NCOL[s]][::-1]
    bufs.update({"M": sub, "ln_theta": theta_k, "props": numpy.exp(theta_k), "log_props": log_props,
                 "assigned": bs.sentinel(rec.R, I4), "post": bs.sentinel((rec.R, sc.LD), F8)})
    decoy.update({"M": bs.nan_like(sub), "ln_theta": bs.nan_like(theta_k), "props": bs.nan_like(theta_k),
                  "log_props": bs.nan_like(log_props)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_assign_reads_samples_runs(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, RUNS, p["M"], sc.LD,
                                                 h["ncol_host"].ctypes.data, h["perm_host"].ctypes.data, p["ln_theta"], p["props"],
                                                 p["log_props"], None, numpy.log(2.0), p["assigned"], p["post"], p["ws"], nbytes, stream)
    return bs.Case("mxm_assign_reads_samples_runs", "S=3 B=3 ld=8 with the posterior", "B", call, bufs, decoy, ["assigned", "post"],
                   scratch={"ws": nbytes}, host={"row0_host": (sc.ROW0, sc.ROW0_OTHER), "ncol_host": (sc.NCOL, sc.NCOL),
                                                 "perm_host": (perm, other)})


def loop_case(lib):
    rec = sc.records(lib, "samples 66")
    bufs, decoy = rec.bufs()
    sub, theta = sc._reduced(rec), _thetas(35)
    nbytes = _ws(lib, sc.LD)
    bufs.update({"M": sub, "w": rec.wts, "props_cur": numpy.exp(theta), "ln_cur": theta, "ln_new": theta.copy(),
                 "state": sc.states(3 * RUNS), "E": bs.sentinel((rec.R, sc.LD), F8)})
    decoy.update({"M": bs.nan_like(sub), "w": bs.nan_like(rec.wts), "props_cur": bs.nan_like(theta), "ln_cur": bs.nan_like(theta),
                  "ln_new": bs.nan_like(theta), "state": sc.stopped(3 * RUNS)})

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_em_loop_samples_narrow_runs(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, RUNS, p["M"], sc.LD,
                                                   h["ncol_host"].ctypes.data, p["w"], p["props_cur"], p["ln_cur"], p["ln_new"],
                                                   p["state"], 0.0, 5, 2, p["E"], p["ws"], nbytes, stream, sc._state_ptr(h))
    return bs.Case("mxm_em_loop_samples_narrow_runs", "S=3 B=3 ld=8", "C", call, bufs, decoy,
                   ["props_cur", "ln_cur", "ln_new", "state", "E"], scratch={"ws": nbytes},
                   host={"row0_host": (sc.ROW0, sc.ROW0_OTHER), "ncol_host": (sc.NCOL, numpy.array([1, 1, 1], dtype=I4))},
                   host_outs=sc._state_host(3 * RUNS))


BUILDERS = {"mxm_votes_samples_runs": votes_case, "mxm_assign_reads_samples_runs": assign_case,
            "mxm_em_loop_samples_narrow_runs": loop_case}
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
    with open(os.path.join(ROOT, "include", "mixemt_hip_samples_runs.h")) as fin:
        text = " ".join(fin.read().replace(" * ", " ").split())
    assert "mxm_votes_samples_runs and mxm_assign_reads_samples_runs only enqueue" in text
    assert "may be changed as soon as the call has returned" in text and "None of the three is meant to be captured" in text
    assert LOOP_SENTENCE in text


@pytest.mark.parametrize("entry", sorted(BUILDERS))
def test_quiet_run_reproduces_itself_and_the_decoy_changes_it(lib, entry):
    case, staged, want = prepared(lib, entry)
    assert bs.same(case, bs.quiet_run(lib, staged), want) is None, case.id
    decoyed = bs.quiet_run(lib, staged, decoys=True)
    assert any(not numpy.array_equal(decoyed[k], want[k]) for k in want), "%s: the decoy does not change the output" % case.id
    if case.klass == "C":                                         # the loop ran: five iterations of every run, E untouched
        from mixemt_amd import _lib
        states = (_lib.EmState * (3 * RUNS)).from_buffer_copy(want["host:state_host"].tobytes())
        assert [(st.done, st.iters) for st in states] == [(2, 5)] * (3 * RUNS)
        assert (want["E"] == 0xFF).all()


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
