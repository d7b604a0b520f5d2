"""
The formatter kernels of include/mixemt_hip_stats_samples.h (csrc/stats_text_kernels.hpp) through the C ABI against a
restatement of the two line formats with Python's %d: every position digit edge (n_pos = 10 001), counts at every digit
edge up to 2^32 - 1, a row of fourteen bins of 2^32 - 1 (total 60 129 542 130), pad bins and rows past n_pos filled with
0xFFFFFFFF, NULL tables, an empty prefix and one of exactly MXM_STATS_MAX_PREFIX bytes, thresholds equal to a count, long
tails across a tile edge, tile_off at the tile edges, and an output one byte too short.
"""
import ctypes

import numpy
import pytest

pytestmark = pytest.mark.gpu

TILE, MAX_PREFIX = 256, 64
FULL = 0xFFFFFFFF
EDGES = numpy.array([0] + [v for d in range(1, 10) for v in (10 ** d - 1, 10 ** d)] + [FULL], dtype=numpy.uint32)
N_POS = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 10001]
NULLS = {1: (), 3: (1,), 7: (0, 3, 6)}                     # NULL tables: none; the middle; first, in the middle and last
THR = [100.0, 2.5, 3.0, 1e9, 0.0, 4294967295.0, 7.0]      # (100, 2.5 and 3 meet the rows made for them below)


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import _lib
    return _lib.load()


def make_tables(rng, n_blocks, n_pos, extra_rows=5):
    """Per block None or uint32 [n_pos + extra][16]: digit-edge counts, pad bins and the rows past n_pos all ones, the
    threshold rows at 0..5 and the row of fourteen full bins at the end (where n_pos has room for them)."""
    tables = []
    for b in range(n_blocks):
        if b in NULLS[n_blocks]:
            tables.append(None)
            continue
        t = EDGES[rng.integers(0, len(EDGES), size=(n_pos + extra_rows, 16))]
        small = rng.random(n_pos + extra_rows) < 0.5                # half the rows: small counts, as real pileups have
        t[small] = rng.integers(0, 120, size=(int(small.sum()), 16))
        if n_pos >= 8:
            t[0:6] = 0
            t[0, [0, 7, 1]] = 60, 40, 100                           # A = 60 + 40 = C = 100: two bases AT a threshold of 100
            t[1, [0, 1, 8]] = 100, 90, 9                            # A = 100, C = 99: exactly one base at 100
            t[2, [2, 3]] = 3, 2                                     # 3 and 2 against 2.5: one base
            t[3, [2, 10]] = 3, 3                                    # 3 and 3 against 2.5 and against 3: two bases
            t[4, [0, 1, 2, 3]] = 2, 2, 2, 2                         # nothing reaches 2.5
            t[5, [4, 5, 6, 11, 12, 13]] = 1000                      # N, X and gaps count for the total only
            t[n_pos - 1, :14] = FULL                                # total 14 * (2^32 - 1)
        t[:, 14:] = FULL
        t[n_pos:] = FULL
        tables.append(numpy.ascontiguousarray(t))
    return tables


def make_kind1(rng, n_blocks, n_pos):
    poly = (rng.random((n_blocks, n_pos)) < 0.3).astype(numpy.uint8)
    thr = numpy.array([THR[b % len(THR)] for b in range(n_blocks)], dtype=numpy.float64)
    tails = []
    for b in range(n_blocks):
        mine = {}
        for pos in numpy.flatnonzero(rng.random(n_pos) < 0.04):
            mine[int(pos)] = ",".join("H%d:A%dG" % (k, pos + 1) for k in range(int(rng.integers(1, 4)))).encode()
        if n_pos > TILE and b != 1:
            mine[TILE - 1] = bytes(rng.integers(65, 91, size=1000, dtype=numpy.uint8))      # the last line of a tile
            mine[TILE] = bytes(rng.integers(97, 123, size=1000, dtype=numpy.uint8))         # the first line of the next
        tails.append(mine)
    return poly, thr, tails


def want_lines(kind, table, n_pos, prefix=b"", poly=None, thr=None, tails=None):
    tab = numpy.zeros((n_pos, 16), dtype=numpy.int64) if table is None else table[:n_pos].astype(numpy.int64)
    acgt = tab[:, 0:4] + tab[:, 7:11]
    if kind == 0:
        total = tab[:, :14].sum(axis=1)
        return [prefix + b"%d\t%d\t%d\t%d\t%d\t%d\n" % (pos, a, c, g, t, tot)
                for pos, (a, c, g, t), tot in zip(range(n_pos), acgt.tolist(), total.tolist())]
    variant = (acgt.astype(numpy.float64) >= thr).sum(axis=1) > 1
    return [b"%d\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n" % (pos + 1, a, c, g, t, b"polymorphic" if poly[pos] else b"fixed",
                                                b"variant" if var else b"sample_fixed", tails.get(pos, b""))
            for pos, (a, c, g, t), var in zip(range(n_pos), acgt.tolist(), variant.tolist())]


class Problem(object):
    """One text on the device: the struct, what it points to, and the restatement's lines per block."""

    def __init__(self, lib, kind, n_blocks, n_pos, seed):
        import torch
        from mixemt_amd import stats
        rng = numpy.random.default_rng(seed)
        self.kind, self.n_blocks, self.n_pos = kind, n_blocks, n_pos
        self.tables = make_tables(rng, n_blocks, n_pos)
        self.dev = [None if t is None else torch.from_numpy(t.view(numpy.int32)).cuda() for t in self.tables]
        ptrs = [None if t is None else t.data_ptr() for t in self.dev]
        if kind == 0:
            pool = [b"", bytes(rng.integers(33, 127, size=MAX_PREFIX, dtype=numpy.uint8)), b"hap1\tL3e1b\t", b"all\tmix\t"]
            self.prefixes = [pool[b % len(pool)] for b in range(n_blocks)]
            self.st, self.keep, self.n_tiles = stats._stats_text(lib, 0, n_pos, ptrs, prefixes=self.prefixes)
            self.lines = [want_lines(0, self.tables[b], n_pos, self.prefixes[b]) for b in range(n_blocks)]
        else:
            self.poly, self.thr, self.tails = make_kind1(rng, n_blocks, n_pos)
            lens = numpy.zeros(n_blocks * n_pos + 1, dtype=numpy.int64)
            raw = []
            for b in range(n_blocks):
                for pos in sorted(self.tails[b]):
                    lens[b * n_pos + pos + 1] = len(self.tails[b][pos])
                    raw.append(self.tails[b][pos])
            self.tail_ptr = numpy.cumsum(lens)
            self.tail = numpy.frombuffer(b"".join(raw) or b"\0", dtype=numpy.uint8).copy()
            self.st, self.keep, self.n_tiles = stats._stats_text(
                lib, 1, n_pos, ptrs, poly=torch.from_numpy(self.poly).cuda(), thr=torch.from_numpy(self.thr).cuda(),
                tail=torch.from_numpy(self.tail).cuda(), tail_ptr=torch.from_numpy(self.tail_ptr).cuda())
            self.lines = [want_lines(1, self.tables[b], n_pos, poly=self.poly[b], thr=self.thr[b], tails=self.tails[b])
                          for b in range(n_blocks)]
        self.text = b"".join(b"".join(block) for block in self.lines)
        # the tiles' first bytes: the cumulative line lengths at the tile edges of every block
        sizes = [sum(len(line) for line in block[lo:lo + TILE]) for block in self.lines for lo in range(0, n_pos, TILE)]
        self.tile_off = numpy.concatenate([[0], numpy.cumsum(sizes)]).astype(numpy.int64)

    def sizes(self, lib):
        import torch
        off = torch.full((self.n_tiles + 1,), -1, dtype=torch.int64, device="cuda")
        rc = lib.mxm_stats_text_sizes(ctypes.byref(self.st), off.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mxm_last_error()
        return off

    def write(self, lib, off, out_bytes, shift=0, room=None):
        """The text at an address `shift` bytes off a 256-byte boundary, in a buffer of 0xAA bytes with `room` bytes (default
        out_bytes) and as many again behind it -> (the whole buffer behind the shift as numpy, the error word)."""
        import torch
        room = out_bytes if room is None else room
        buf = torch.full((shift + 2 * room + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        rc = lib.mxm_stats_text_write(ctypes.byref(self.st), off.data_ptr(), buf.data_ptr() + shift, out_bytes, err.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.mxm_last_error()
        torch.cuda.synchronize()
        return buf[shift:].cpu().numpy(), int(err.item())


def check(lib, kind, n_blocks, n_pos, seed, shift):
    p = Problem(lib, kind, n_blocks, n_pos, seed)
    assert p.n_tiles == n_blocks * ((n_pos + TILE - 1) // TILE) == len(p.tile_off) - 1
    off = p.sizes(lib)
    assert numpy.array_equal(off.cpu().numpy(), p.tile_off)
    total = len(p.text)
    got, err = p.write(lib, off, total, shift=shift)
    assert err == 0
    assert got[:total].tobytes() == p.text
    assert (got[total:] == 0xAA).all()                                 # nothing at or past out + out_bytes
    return p, off


@pytest.mark.parametrize("kind", [0, 1], ids=["obs", "pos"])
@pytest.mark.parametrize("n_pos", N_POS)
def test_three_blocks_at_every_size(lib, kind, n_pos):
    p, _ = check(lib, kind, 3, n_pos, 100 + n_pos + kind, shift=1 + n_pos % 3)
    if n_pos >= 8:
        assert b"\t60129542130\n" in p.text if kind == 0 else b"\t8589934590\t" in p.text
    if n_pos == 10001 and kind == 0:
        for edge in (9, 10, 99, 100, 999, 1000, 9999, 10000):          # every position digit edge, 0-based
            assert p.lines[2][edge].startswith(p.prefixes[2] + b"%d\t" % edge)
        assert len(p.prefixes[1]) == MAX_PREFIX and p.prefixes[0] == b"" and p.lines[1][0].startswith(p.prefixes[1] + b"0\t")
    if n_pos == 10001 and kind == 1:
        assert p.lines[0][9998].startswith(b"9999\t") and p.lines[0][9999].startswith(b"10000\t")
    if kind == 1 and n_pos >= 8:
        # thr 100 (block 0): two bases AT the threshold are a variant, one is not; thr 3 (block 2): 3 and 3
        assert p.lines[0][0].split(b"\t")[1:7] == [b"100", b"100", b"0", b"0", b"polymorphic" if p.poly[0][0] else b"fixed", b"variant"]
        assert p.lines[0][1].split(b"\t")[1:7:5] == [b"100", b"sample_fixed"] and p.lines[0][1].split(b"\t")[2] == b"99"
        assert p.lines[2][3].split(b"\t")[6] == b"variant" and p.lines[2][2].split(b"\t")[6] == b"sample_fixed"
    if kind == 1 and n_pos > TILE:
        assert len(p.tails[0][TILE - 1]) == len(p.tails[0][TILE]) == 1000
        assert any(b"\t\n" in line for line in p.lines[0][:50])         # empty tails


@pytest.mark.parametrize("kind", [0, 1], ids=["obs", "pos"])
@pytest.mark.parametrize("n_blocks", [1, 7])
def test_one_and_seven_blocks(lib, kind, n_blocks):
    """One block; seven with NULL tables first, in the middle and last (a NULL table is a table of zeros); thresholds 2.5
    against 2 and 3 (block 1 of seven)."""
    p, _ = check(lib, kind, n_blocks, 2 * TILE + 3, 7 * n_blocks + kind, shift=3)
    if n_blocks == 7:
        assert p.tables[0] is None and p.tables[3] is None and p.tables[6] is None
        if kind == 0:
            assert p.lines[0][0] == p.prefixes[0] + b"0\t0\t0\t0\t0\t0\n"
        else:
            assert p.lines[0][0].split(b"\t")[:5] == [b"1", b"0", b"0", b"0", b"0"]
            assert p.thr[1] == 2.5
            assert [p.lines[1][r].split(b"\t")[6] for r in (2, 3, 4)] == [b"sample_fixed", b"variant", b"sample_fixed"]


def test_an_output_one_byte_short_skips_the_last_tile_whole(lib):
    for kind in (0, 1):
        p = Problem(lib, kind, 3, 2 * TILE + 3, 40 + kind)
        off = p.sizes(lib)
        total = len(p.text)
        got, err = p.write(lib, off, total - 1, shift=1, room=total)
        last = int(p.tile_off[-2])
        assert err == 1
        assert got[:last].tobytes() == p.text[:last]                   # every other tile is there
        assert (got[last:] == 0xAA).all()                              # the last tile: not one byte of it, nothing past the end
        # an output of no bytes at all: every tile is skipped
        got, err = p.write(lib, off, 0, shift=0, room=total)
        assert err == 1 and (got == 0xAA).all()


def test_nothing_to_format_still_writes_the_first_offset(lib):
    import torch
    from mixemt_amd import _lib
    for st in (_lib.StatsText(0, 0, 100), _lib.StatsText(1, 0, 100), _lib.StatsText(0, 3, 0)):
        off = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        assert lib.mxm_stats_text_sizes(ctypes.byref(st), off.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        assert off.tolist() == [0, -1]
