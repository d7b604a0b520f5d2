"""
The two enqueuing entries of include/mixemt_hip_stats_samples.h called through the library handle with every device buffer at
its exact documented size between red zones (tests/_guarded.py): tile_off [n_tiles + 1], out [out_bytes], err (one uint32),
poly [n_blocks][n_pos], thr [n_blocks], tail, tail_ptr [n_blocks * n_pos + 1], and every table at EXACTLY n_pos rows ("rows at
or past n_pos are never read").  n_pos is no multiple of the tile; one table is NULL.  Reference: the restatement of
tests/test_gpu_stats_text.py.
"""
import ctypes

import numpy
import pytest

from _guarded import guarded, guarded_from
from _guarded_abi import DEV, load_lib, stream, sync
from test_gpu_stats_text import TILE, make_kind1, make_tables, want_lines

pytestmark = pytest.mark.gpu

N_POS, N_BLOCKS = 2 * TILE + 77, 3


@pytest.fixture(scope="module")
def lib():
    return load_lib()


def _struct(kind, tables):
    from mixemt_amd import _lib
    ptrs = (ctypes.c_void_p * N_BLOCKS)(*[None if t is None else t.ptr for t in tables])
    return _lib.StatsText(kind, N_BLOCKS, N_POS, ctypes.cast(ptrs, ctypes.c_void_p)), [ptrs]


def _run(lib, st, bufs, total_want):
    n_tiles = lib.mxm_stats_text_tiles(N_BLOCKS, N_POS)
    assert n_tiles == N_BLOCKS * 3 and N_POS % TILE
    bufs["tile_off"] = guarded(8 * (n_tiles + 1), 8, DEV)
    assert lib.mxm_stats_text_sizes(ctypes.byref(st), bufs["tile_off"].ptr, stream()) == 0, lib.mxm_last_error()
    sync()
    for name, buf in bufs.items():
        buf.check(name + " (sizes)")
    off = bufs["tile_off"].get(numpy.int64)
    assert int(off[-1]) == total_want and int(off[0]) == 0 and (numpy.diff(off) > 0).all()
    bufs["out"] = guarded(total_want, 1, DEV)                                # an odd address: nothing assumes an alignment
    bufs["err"] = guarded_from([0], numpy.uint32, 4, DEV)
    assert lib.mxm_stats_text_write(ctypes.byref(st), bufs["tile_off"].ptr, bufs["out"].ptr, total_want, bufs["err"].ptr,
                                    stream()) == 0, lib.mxm_last_error()
    sync()
    for name, buf in bufs.items():
        buf.check(name + " (write)")
    assert bufs["err"].get(numpy.uint32).tolist() == [0]
    return bufs["out"].get(numpy.uint8).tobytes()


def _tables(rng):
    """The tables at exactly n_pos rows, 16-byte aligned, the middle one NULL."""
    host = make_tables(rng, N_BLOCKS, N_POS, extra_rows=0)
    assert host[1] is None and all(t is None or t.shape == (N_POS, 16) for t in host)
    return host, [None if t is None else guarded_from(t, numpy.uint32, 16, DEV) for t in host]


def test_obs_lines(lib):
    """ "table_host ... DEVICE pointers, 16-byte aligned, to [>= n_pos][16] uint32; NULL: a table of zeros", "tile_off
    [n_tiles + 1] DEVICE int64, written", "out [out_bytes] DEVICE uint8 ... no alignment of out or of a tile is assumed"."""
    host, dev = _tables(numpy.random.default_rng(21))
    prefixes = [b"", b"p" * 64, b"all\tmix\t"]
    st, keep = _struct(0, dev)
    ptr = numpy.array([0, 0, 64, 72], dtype=numpy.int64)
    raw = numpy.frombuffer(b"".join(prefixes), dtype=numpy.uint8)
    st.prefix_host, st.prefix_ptr_host = raw.ctypes.data, ptr.ctypes.data
    want = b"".join(b"".join(want_lines(0, host[b], N_POS, prefixes[b])) for b in range(N_BLOCKS))
    bufs = {"table %d" % b: t for b, t in enumerate(dev) if t is not None}
    assert _run(lib, st, bufs, len(want)) == want


def test_pos_lines(lib):
    """ "poly [n_blocks][n_pos] uint8", "thr [n_blocks]", "tail ... the tails' bytes", "tail_ptr [n_blocks * n_pos + 1]"."""
    rng = numpy.random.default_rng(22)
    host, dev = _tables(rng)
    poly, thr, tails = make_kind1(rng, N_BLOCKS, N_POS)
    tails[2][N_POS - 1] = b"the-last-line's-tail"                           # the CSR's last entry is used
    lens = numpy.zeros(N_BLOCKS * N_POS + 1, dtype=numpy.int64)
    for b in range(N_BLOCKS):
        for pos in tails[b]:
            lens[b * N_POS + pos + 1] = len(tails[b][pos])
    raw = [tails[b][pos] for b in range(N_BLOCKS) for pos in sorted(tails[b])]
    bufs = {"table %d" % b: t for b, t in enumerate(dev) if t is not None}
    bufs.update({"poly": guarded_from(poly, numpy.uint8, 1, DEV), "thr": guarded_from(thr, numpy.float64, 8, DEV),
                 "tail": guarded_from(numpy.frombuffer(b"".join(raw), dtype=numpy.uint8), numpy.uint8, 1, DEV),
                 "tail_ptr": guarded_from(numpy.cumsum(lens), numpy.int64, 8, DEV)})
    st, keep = _struct(1, dev)
    st.poly, st.thr, st.tail, st.tail_ptr = bufs["poly"].ptr, bufs["thr"].ptr, bufs["tail"].ptr, bufs["tail_ptr"].ptr
    want = b"".join(b"".join(want_lines(1, host[b], N_POS, poly=poly[b], thr=thr[b], tails=tails[b])) for b in range(N_BLOCKS))
    assert want.endswith(b"\tthe-last-line's-tail\n")
    assert _run(lib, st, bufs, len(want)) == want
