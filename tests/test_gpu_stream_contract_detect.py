"""
The stream contract of the entries of include/mixemt_hip_detect.h on a side stream that is still BUSY when the library is
called (tests/_busy_stream.py; the checks of tests/test_gpu_stream_contract.py, whose table of cases names the older
headers' entries and stays as it is):
  mxm_detect_candidates        class B: uploads rows_host into stream-ordered memory of its own, only enqueues;
  mxm_check_variants_entries   class B: uploads table_of_host likewise, only enqueues.
Both return with the gate behind the delay still pending, their results are right once the stream has drained and equal the
quiet run's bit for bit, with the host table in pageable and in pinned memory, overwritten with another problem's table as
soon as the call returns.  E = 6 entries over H = 66 haplogroups; E = 5 entries over the toy tree's three pileups.
"""
import os

import numpy
import pytest

import _busy_stream as bs
import _stream_cases as sc
from conftest import ROOT
from test_gpu_detect import entries_for
from test_gpu_var_check import TOY, table
from test_observe import asm_args
from test_var_check_host import toy_tree

pytestmark = pytest.mark.gpu

F8, I8, I4, U1 = numpy.float64, numpy.int64, numpy.int32, numpy.uint8
LD, H = 8, 66
G, T = 2, 3


def candidates_case(lib):
    kinds, entries = entries_for(H, LD, 5)
    keep = [kinds.index(k) for k in ("random", "ties", "none", "below and at", "no row won", "exactly ld")]
    entries = [entries[i] for i in keep]
    n = len(entries)
    other = entries_for(H, LD, 6)[1][:n]                                        # another valid problem: the integer decoys
    votes, first, props = (numpy.stack([e[i] for e in entries]) for i in (0, 1, 3))
    rows = numpy.array([e[2] for e in entries], dtype=I8)
    bufs = {"votes": votes, "first": first, "props": props, "state": sc.stopped(n), "cand": bs.sentinel((n, LD), I4),
            "ncand": bs.sentinel(n, I4), "cprop": bs.sentinel((n, LD), F8)}
    decoy = {"votes": bs.nan_like(votes), "props": bs.nan_like(props), "first": numpy.stack([e[1] for e in other]),
             "state": sc.states(n)}                                             # (done = 0: every entry refused)

    def call(p, h, stream):
        return lib.mxm_detect_candidates(p["votes"], p["first"], h["rows_host"].ctypes.data, p["props"], p["state"], n, H, 3.0, LD,
                                         p["cand"], p["ncand"], p["cprop"], stream)
    return bs.Case("mxm_detect_candidates", "E=6 H=66 ld=8", "B", call, bufs, decoy, ["cand", "ncand", "cprop"],
                   host={"rows_host": (rows, numpy.zeros(n, dtype=I8))})


def check_case(lib):
    from mixemt_amd import assign
    tab = assign.VarCheckTables.build(toy_tree(), TOY)
    index = {h: i for i, h in enumerate(TOY)}
    L = 37
    tables = numpy.stack([table(L, {(0, G): 5, (1, T): 5}), table(L, {(0, G): 5, (2, T): 5, (4, T): 5}), table(L, {(0, G): 9})])
    lists = [["I", "A", "H", "F"], ["H", "I"], [], ["H"], ["I", "A"]]
    n = len(lists)
    cand, other = numpy.zeros((n, LD), dtype=I4), numpy.zeros((n, LD), dtype=I4)
    for e, names in enumerate(lists):
        cand[e, :len(names)] = [index[x] for x in names]
        other[e, :len(names)] = [index[x] for x in names[::-1]]
    ncand = numpy.array([len(x) for x in lists], dtype=I4)
    args = asm_args()
    bufs = {"counts": tables.astype(I4), "key_ptr": tab.key_ptr_h, "key": tab.key_h, "site": tab.site_h, "site_key": tab.site_key_h,
            "cand": cand, "ncand": ncand, "keep": bs.sentinel((n, LD), U1), "n_uniq": bs.sentinel((n, LD), I4),
            "n_found": bs.sentinel((n, LD), I4), "flag": bs.sentinel(n, I4)}
    decoy = {"counts": numpy.zeros_like(bufs["counts"]), "cand": other, "ncand": numpy.zeros(n, dtype=I4)}

    def call(p, h, stream):
        return lib.mxm_check_variants_entries(p["counts"], 3, L, p["key_ptr"], p["key"], len(TOY), p["site"], p["site_key"],
                                              len(tab.site_h), tab.max_pos, h["table_of_host"].ctypes.data, n, p["cand"], p["ncand"], LD,
                                              float(args.min_var_reads), float(args.frac_var_reads), float(args.var_fraction), 0, 0,
                                              p["keep"], p["n_uniq"], p["n_found"], p["flag"], stream)
    return bs.Case("mxm_check_variants_entries", "E=5 T=3 ld=8", "B", call, bufs, decoy, ["keep", "n_uniq", "n_found", "flag"],
                   host={"table_of_host": (numpy.array([0, 1, 2, 1, 0], dtype=I4), numpy.array([2, 2, 0, 0, 1], dtype=I4))})


BUILDERS = {"mxm_detect_candidates": candidates_case, "mxm_check_variants_entries": check_case}
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


def test_the_header_says_that_both_entries_only_enqueue():
    with open(os.path.join(ROOT, "include", "mixemt_hip_detect.h")) as fin:
        text = " ".join(fin.read().replace(" * ", " ").split())
    assert text.count("STREAM: both entries only enqueue") == 1
    assert "may be changed as soon as it has" in text and "Not meant to be captured" in text


@pytest.mark.parametrize("entry", sorted(BUILDERS))
def test_quiet_run_reproduces_itself_and_the_decoy_changes_it(lib, entry):
    case, staged, want = prepared(lib, entry)
    assert bs.same(case, bs.quiet_run(lib, staged), want) is None, case.id
    decoyed = bs.quiet_run(lib, staged, decoys=True)
    assert any(not numpy.array_equal(decoyed[k], want[k]) for k in want), "%s: the decoy does not change the output" % case.id
    if entry == "mxm_detect_candidates":
        assert want["ncand"].view(I4).tolist() == [3, 3, 0, 3, 2, 8] and decoyed["ncand"].view(I4).tolist() == [-1] * 6
    else:
        assert want["flag"].view(I4).tolist() == [0] * 5
        keep = want["keep"].reshape(5, LD)
        assert keep[0, :4].tolist() == [1, 1, 0, 0] or keep[0, :4].any()             # the lists were checked against their tables
        assert (keep[2] == 0xFF).all() and (keep[1, 2:] == 0xFF).all()


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
    assert pending, "%s only enqueues by its header, but the %g ms delay ahead of it had passed when it returned" % (case.id, case.delay_ms)
    assert host_ms < case.delay_ms / 2, "%s only enqueues by its header, but took %.1f ms of host time" % (case.id, host_ms)
