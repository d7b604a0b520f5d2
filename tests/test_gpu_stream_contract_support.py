"""
The stream contract of the entries of include/mixemt_hip_support.h on a side stream that is still BUSY when the library is
called (tests/_busy_stream.py; the checks of tests/test_gpu_stream_contract.py, whose table of cases names the older
headers' entries and stays as it is):
  mxm_loglik_samples_masks           class B: uploads host tables on every call (row0_host, ncol_host, mask_host), only
                                     enqueues, not captured -- it returns with the gate behind the delay still pending, and
                                     its results are right once the stream has drained;
  mxm_em_loop_samples_narrow_masks   class C: it waits, and its header says so.
Both: the busy run's outputs equal the quiet run's bit for bit, with the host tables in pageable and in pinned memory,
overwritten with another problem's tables as soon as the call returns.  S = 3 samples of 33, 64 and 600 rows, B = 4 fits.
"""
import ctypes
import os

import numpy
import pytest

import _busy_stream as bs
import _stream_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

FITS = 4
F8, I4, U4 = numpy.float64, numpy.int32, numpy.uint32
# sc.NCOL = (1, 3, 7) columns: the full set, two subsets and an unused slot; the decoy's masks fit the decoy's columns (1, 1, 1)
MASKS = numpy.array([[1, 0, 0, 0], [0b111, 0b011, 0, 0b100], [0b1111111, 0b0101010, 0b1000000, 0b0111111]], dtype=U4)
MASKS_OTHER = numpy.array([[1, 1, 1, 1]] * 3, dtype=U4)
LOOP_SENTENCE = ("mxm_em_loop_samples_narrow_masks blocks the calling thread (one read-back of the states per launch); state_host "
                 "receives the final states")


def _ws(lib):
    n = max(int(lib.mxm_samples_plan(row0.ctypes.data, 3, None, 0, None)) for row0 in (sc.ROW0, sc.ROW0_OTHER))
    return int(lib.mxm_support_workspace_bytes(n, 3, FITS, sc.LD))


def _weights(rec):
    return numpy.random.default_rng(43).integers(1, 4, size=rec.R).astype(F8)


def _thetas(seed):
    """log proportions [S][B][ld] over every mask's columns, -inf elsewhere."""
    rng = numpy.random.default_rng(seed)
    theta = numpy.full((3, FITS, sc.LD), -numpy.inf)
    for s in range(3):
        for b in range(FITS):
            cols = [k for k in range(sc.LD) if (int(MASKS[s, b]) >> k) & 1]
            if cols:
                theta[s, b, cols] = numpy.log(rng.dirichlet([1.0] * len(cols)))
    return theta


HOST = {"row0_host": (sc.ROW0, sc.ROW0_OTHER), "ncol_host": (sc.NCOL, numpy.array([1, 1, 1], dtype=I4)), "mask_host": (MASKS, MASKS_OTHER)}


def loop_case(lib):
    rec = sc.records(lib, "samples 66")
    bufs, _ = rec.bufs()
    sub, theta, wts = sc._reduced(rec), _thetas(51), _weights(rec)
    nbytes = _ws(lib)
    bufs.update({"M": sub, "w": wts, "props_cur": numpy.exp(theta), "ln_cur": theta, "ln_new": theta.copy(),
                 "state": sc.states(3 * FITS), "E": bs.sentinel((FITS * rec.R, sc.LD), F8)})
    decoy = {"M": bs.nan_like(sub), "w": bs.nan_like(wts), "props_cur": bs.nan_like(theta), "ln_cur": bs.nan_like(theta),
             "ln_new": bs.nan_like(theta), "state": sc.stopped(3 * FITS)}

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_em_loop_samples_narrow_masks(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, FITS, p["M"], sc.LD,
                                                    h["ncol_host"].ctypes.data, h["mask_host"].ctypes.data, p["w"], p["props_cur"],
                                                    p["ln_cur"], p["ln_new"], p["state"], 0.0, 5, 2, p["E"], p["ws"], nbytes, stream,
                                                    sc._state_ptr(h))
    return bs.Case("mxm_em_loop_samples_narrow_masks", "S=3 B=4 ld=8", "C", call, bufs, decoy,
                   ["props_cur", "ln_cur", "ln_new", "state", "E"], scratch={"ws": nbytes}, host=HOST, host_outs=sc._state_host(3 * FITS))


def loglik_case(lib):
    rec = sc.records(lib, "samples 66")
    bufs, _ = rec.bufs()
    sub, theta, wts = sc._reduced(rec), _thetas(52), _weights(rec)
    nbytes = _ws(lib)
    bufs.update({"M": sub, "w": wts, "ln_props": theta, "ll": bs.sentinel((3, FITS), F8), "n_eff": bs.sentinel(3, F8)})
    decoy = {"M": bs.nan_like(sub), "w": bs.nan_like(wts), "ln_props": bs.nan_like(theta)}

    def call(p, h, stream):
        st = rec.struct(p)
        return lib.mxm_loglik_samples_masks(ctypes.byref(st), h["row0_host"].ctypes.data, 3, rec.H, FITS, p["M"], sc.LD,
                                            h["ncol_host"].ctypes.data, h["mask_host"].ctypes.data, p["w"], p["ln_props"], p["ll"],
                                            p["n_eff"], p["ws"], nbytes, stream)
    return bs.Case("mxm_loglik_samples_masks", "S=3 B=4 ld=8", "B", call, bufs, decoy, ["ll", "n_eff"], scratch={"ws": nbytes}, host=HOST)


BUILDERS = {"mxm_em_loop_samples_narrow_masks": loop_case, "mxm_loglik_samples_masks": loglik_case}
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


def test_the_header_says_which_entry_enqueues_and_that_the_loop_blocks():
    with open(os.path.join(ROOT, "include", "mixemt_hip_support.h")) as fin:
        text = " ".join(fin.read().replace(" * ", " ").split())
    assert text.count("STREAM: the entry only enqueues") == 1
    assert "may be changed as soon as the call has returned" in text and "Not meant to be captured" in text
    assert LOOP_SENTENCE in text


@pytest.mark.parametrize("entry", sorted(BUILDERS))
def test_quiet_run_reproduces_itself_and_the_decoy_changes_it(lib, entry):
    case, staged, want = prepared(lib, entry)
    assert bs.same(case, bs.quiet_run(lib, staged), want) is None, case.id
    decoyed = bs.quiet_run(lib, staged, decoys=True)
    assert any(not numpy.array_equal(decoyed[k], want[k]) for k in want), "%s: the decoy does not change the output" % case.id
    from mixemt_amd import _lib
    if case.klass == "C":                                         # the loop ran: five iterations of every used fit, E untouched
        states = (_lib.EmState * (3 * FITS)).from_buffer_copy(want["host:state_host"].tobytes())
        assert [(st.done, st.iters) for st in states] == [(2, 5) if m else (0, 0) for m in MASKS.reshape(-1)]
        assert (want["E"] == 0xFF).all()
    else:                                                         # the used slots hold a log-likelihood, the unused the sentinel
        ll = want["ll"].view(F8).reshape(3, FITS)
        assert numpy.array_equal(numpy.isfinite(ll), MASKS != 0) and (want["ll"].view(numpy.uint8).reshape(3, FITS, 8)[MASKS == 0] == 0xFF).all()
        rec = sc.records(lib, "samples 66")
        wts = _weights(rec)
        assert want["n_eff"].view(F8).tolist() == [wts[int(lo):int(hi)].sum() for lo, hi in zip(sc.ROW0[:-1], sc.ROW0[1:])]


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
