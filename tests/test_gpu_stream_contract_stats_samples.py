"""
The stream contract of the two enqueuing entries of include/mixemt_hip_stats_samples.h on a side stream that is still BUSY when
the library is called (tests/_busy_stream.py; the checks of tests/test_gpu_stream_contract.py, whose table of cases names
the older headers' entries and stays as it is):
  mxm_stats_text_sizes, mxm_stats_text_write    class B: upload host tables into stream-ordered memory, only enqueue, not
                              captured -- they return with the gate behind the delay still pending, and their results are
                              right once the stream has drained.
Both: the busy run's outputs equal the quiet run's bit for bit, with the host tables (the table pointers, the prefixes and
their offsets) in pageable and in pinned memory, overwritten with another problem's tables as soon as the call returns.
"""
import ctypes
import os

import numpy
import pytest

import _busy_stream as bs
from conftest import ROOT
from test_gpu_stats_text import TILE, make_tables, want_lines

pytestmark = pytest.mark.gpu

N_POS, N_BLOCKS = 2 * TILE + 41, 3
PREFIXES, OTHER_PREFIXES = [b"hap1\tL3e1b\t", b"", b"all\tmix\t"], [b"x\t", b"unassigned\tunassigned\t", b""]


def _inputs(seed):
    rng = numpy.random.default_rng(seed)
    tables = numpy.stack([t for t in make_tables(rng, 1, N_POS, 0) + make_tables(rng, 1, N_POS, 0)])
    return tables                                                     # [2][n_pos][16]: blocks 0 and 2 (block 1 is NULL)


def _prefix_arrays(prefixes):
    raw = numpy.zeros(64, dtype=numpy.uint8)
    joined = b"".join(prefixes)
    raw[:len(joined)] = numpy.frombuffer(joined, dtype=numpy.uint8)
    return raw, numpy.concatenate([[0], numpy.cumsum([len(p) for p in prefixes])]).astype(numpy.int64)


def _host(n_pos_bytes):
    """The host tables: (real, decoy) pairs; the table pointers are made from the run's device pointers -- the decoy names the
    blocks' tables the other way round and makes another block NULL."""
    raw, ptr = _prefix_arrays(PREFIXES)
    raw2, ptr2 = _prefix_arrays(OTHER_PREFIXES)

    def tables(p):
        a, b = p["tables"], p["tables"] + n_pos_bytes
        return numpy.array([a, 0, b], dtype=numpy.uint64), numpy.array([0, b, a], dtype=numpy.uint64)
    return {"table_host": tables, "prefix_host": (raw, raw2), "prefix_ptr_host": (ptr, ptr2)}


def _struct(h):
    from mixemt_amd import _lib
    return _lib.StatsText(0, N_BLOCKS, N_POS, h["table_host"].ctypes.data, h["prefix_host"].ctypes.data,
                          h["prefix_ptr_host"].ctypes.data)


def _want(tables):
    blocks = [tables[0], None, tables[1]]
    lines = [want_lines(0, blocks[b], N_POS, PREFIXES[b]) for b in range(N_BLOCKS)]
    sizes = [sum(len(x) for x in block[lo:lo + TILE]) for block in lines for lo in range(0, N_POS, TILE)]
    return b"".join(b"".join(block) for block in lines), numpy.concatenate([[0], numpy.cumsum(sizes)]).astype(numpy.int64)


def sizes_case(lib):
    tables, other = _inputs(51), _inputs(52)
    n_tiles = lib.mxm_stats_text_tiles(N_BLOCKS, N_POS)
    bufs = {"tables": tables, "tile_off": bs.sentinel(n_tiles + 1, numpy.int64)}

    def call(p, h, stream):
        st = _struct(h)
        return lib.mxm_stats_text_sizes(ctypes.byref(st), p["tile_off"], stream)
    case = bs.Case("mxm_stats_text_sizes", "kind 0, three blocks, the middle one NULL", "B", call, bufs, {"tables": other},
                   ["tile_off"], host=_host(N_POS * 64))
    case.want = {"tile_off": _want(tables)[1]}
    return case


def write_case(lib):
    tables, other = _inputs(53), _inputs(54)
    text, off = _want(tables)
    bufs = {"tables": tables, "tile_off": off, "out": bs.sentinel(len(text), numpy.uint8), "err": numpy.zeros(1, dtype=numpy.uint32)}

    def call(p, h, stream):
        st = _struct(h)
        return lib.mxm_stats_text_write(ctypes.byref(st), p["tile_off"], p["out"], len(text), p["err"], stream)
    case = bs.Case("mxm_stats_text_write", "kind 0, three blocks, the middle one NULL", "B", call, bufs, {"tables": other},
                   ["out", "err"], host=_host(N_POS * 64))
    case.want = {"out": numpy.frombuffer(text, dtype=numpy.uint8), "err": numpy.zeros(1, dtype=numpy.uint32)}
    return case


BUILDERS = {"mxm_stats_text_sizes": sizes_case, "mxm_stats_text_write": write_case}
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


def test_the_header_says_that_both_only_enqueue():
    with open(os.path.join(ROOT, "include", "mixemt_hip_stats_samples.h")) as fin:
        text = " ".join(fin.read().replace(" * ", " ").split())
    assert text.count("The call only enqueues on `stream`; nothing is waited for") == 2
    assert text.count("not meant to be captured") == 2 and "read before the call returns" in text


@pytest.mark.parametrize("entry", sorted(BUILDERS))
def test_quiet_run_is_right_reproduces_itself_and_the_decoy_changes_it(lib, entry):
    case, staged, want = prepared(lib, entry)
    for name, value in case.want.items():
        assert numpy.array_equal(want[name].view(value.dtype), value), (case.id, name)       # the restatement's bytes
    assert bs.same(case, bs.quiet_run(lib, staged), want) is None, case.id
    decoyed = bs.quiet_run(lib, staged, decoys=True)
    assert any(not numpy.array_equal(decoyed[k], want[k]) for k in want), "%s: the decoy does not change the output" % case.id


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
    assert pending, "%s only enqueues by its header, but the %g ms delay ahead of it had passed when it returned" % (
        case.id, case.delay_ms)
    assert host_ms < case.delay_ms / 2, "%s only enqueues by its header, but took %.1f ms of host time" % (case.id, host_ms)
