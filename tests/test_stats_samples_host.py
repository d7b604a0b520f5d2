"""
The host side of the cohort's `-t` tables: the three C entries of include/mixemt_hip_stats_samples.h -- their binding and what
they say when they refuse a call (every row is refused before the first HIP call, so no device is needed; device pointers
are never followed) --, the block plan of stats.write_statistics_many on hand-made cohorts, what it derives from the
contributors for pos.tab, and its errors, which come before any file exists.
The kernels: tests/test_gpu_stats_text.py; the files: tests/test_gpu_stats_samples.py.
"""
import argparse
import ctypes
import io
import os
import re

import numpy
import pytest

from conftest import ROOT

from mixemt_amd import _lib

PTR = 0x1000                 # "some device pointer": 16-byte aligned, never dereferenced by a row below
TILES, SIZES, WRITE = "mxm_stats_text_tiles", "mxm_stats_text_sizes", "mxm_stats_text_write"


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import build
    build.build()
    return _lib.load()


def header_text():
    with open(os.path.join(ROOT, "include", "mixemt_hip_stats_samples.h")) as fin:
        return fin.read()


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_the_headers_names_are_bound_and_exported(lib):
    raw = header_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mxm_\w+)\s*\(", text)))
    assert declared == sorted(_lib.STATS_SAMPLES_SIGNATURES) == sorted([TILES, SIZES, WRITE])
    assert len(lib.mxm_stats_text_tiles.argtypes) == 2 and len(lib.mxm_stats_text_sizes.argtypes) == 3
    assert len(lib.mxm_stats_text_write.argtypes) == 6
    for name in declared:
        assert not any(name in table for table in (_lib.SIGNATURES, _lib.FINISH_SIGNATURES, _lib.VARCHECK_SIGNATURES,
                                                   _lib.ASSEMBLE_SAMPLES_SIGNATURES))
    assert '#include "mixemt_hip_stats_samples.h"' in open(os.path.join(ROOT, "include", "mixemt_hip.h")).read()
    assert int(re.search(r"#define\s+MXM_STATS_TILE_LINES\s+(\d+)", text).group(1)) == 256
    assert int(re.search(r"#define\s+MXM_STATS_MAX_PREFIX\s+(\d+)", text).group(1)) == 64
    from mixemt_amd import build
    assert any(h.endswith("mixemt_hip_stats_samples.h") for h in build.HDRS)
    assert lib.mxm_version() == 603 == _lib.ABI_VERSION
    assert "MXM_VERSION 603: the version stays" in raw and "_lib.STATS_SAMPLES_SIGNATURES" in raw
    assert raw.count("Refused with -1 WITHOUT touching the device") == 2 and raw.count("not meant to be captured") == 2
    # the struct of the binding has the header's fields in the header's order
    body = re.search(r"typedef struct mxm_stats_text \{(.*?)\} mxm_stats_text;", text, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in _lib.StatsText._fields_]
    assert ctypes.sizeof(_lib.StatsText) == 16 + 7 * 8
    blob = open(build.build(), "rb").read()
    for kernel in (b"stats_text_sizes_kernel", b"stats_text_scan_kernel", b"stats_text_write_kernel"):
        assert kernel in blob


def test_tiles(lib):
    assert lib.mxm_stats_text_tiles(0, 100) == 0 and lib.mxm_stats_text_tiles(5, 0) == 0
    assert [lib.mxm_stats_text_tiles(3, n) for n in (1, 255, 256, 257, 16569)] == [3, 3, 3, 6, 195]
    assert lib.mxm_stats_text_tiles(-1, 5) == -1 and lib.mxm_stats_text_tiles(1, -5) == -1
    assert lib.mxm_stats_text_tiles(1, 2 ** 31 - 2) == 2 ** 23 and lib.mxm_stats_text_tiles(1, 2 ** 31 - 1) == -1
    assert lib.mxm_stats_text_tiles(2 ** 31 - 1, 256) == 2 ** 31 - 1 and lib.mxm_stats_text_tiles(2 ** 31 - 1, 257) == -1


def text(kind=0, n_blocks=3, n_pos=1000, tables=(PTR, 0, PTR), prefix=b"hap1\tA\tall\tmix\t", prefix_ptr=(0, 7, 7, 15),
         poly=PTR, thr=PTR, tail=PTR, tail_ptr=PTR):
    """(struct, what it points to)."""
    keep = []
    st = _lib.StatsText(kind, n_blocks, n_pos)
    if tables is not None:
        arr = (ctypes.c_void_p * max(len(tables), 1))(*[t or None for t in tables])
        keep.append(arr)
        st.table_host = ctypes.cast(arr, ctypes.c_void_p)
    if kind != 1:
        if prefix is not None:
            buf = ctypes.create_string_buffer(prefix, max(len(prefix), 1))
            keep.append(buf)
            st.prefix_host = ctypes.cast(buf, ctypes.c_void_p)
        if prefix_ptr is not None:
            ptr = (ctypes.c_int64 * len(prefix_ptr))(*prefix_ptr)
            keep.append(ptr)
            st.prefix_ptr_host = ctypes.cast(ptr, ctypes.c_void_p)
    else:
        st.poly, st.thr, st.tail, st.tail_ptr = poly, thr, tail, tail_ptr
    return st, keep


def call(lib, entry, st="default", tile_off=PTR, out=PTR, out_bytes=100, err=PTR, **kw):
    if st == "default":
        st, keep = text(**kw)
    ref = None if st is None else ctypes.byref(st)
    if entry == SIZES:
        return lib.mxm_stats_text_sizes(ref, tile_off, None)
    return lib.mxm_stats_text_write(ref, tile_off, out, out_bytes, err, None)


LONG = b"x" * 65
NEED1 = "bad arguments (poly, thr and tail_ptr are required)"
TOO_MANY = "more than the tile index holds (n_pos <= 2^31 - 2, at most 2^31 - 1 tiles of 256 lines)"
SHARED_REFUSALS = [
    ("no struct", dict(st=None), "bad arguments (the mxm_stats_text is required)"),
    ("n_blocks below 0", dict(n_blocks=-1), "bad shape (n_blocks = -1, n_pos = 1000)"),
    ("n_pos below 0", dict(n_pos=-7), "bad shape (n_blocks = 3, n_pos = -7)"),
    ("kind 2", dict(kind=2), "unknown kind 2 (0: obs.tab lines, 1: pos.tab lines)"),
    ("kind -1", dict(kind=-1), "unknown kind -1 (0: obs.tab lines, 1: pos.tab lines)"),
    ("n_pos above an int32", dict(n_pos=2 ** 31 - 1), "3 blocks of 2147483647 lines are " + TOO_MANY),
    ("too many tiles", dict(n_blocks=2 ** 31 - 1, n_pos=257), "2147483647 blocks of 257 lines are " + TOO_MANY),
    ("no tables", dict(tables=None), "bad arguments (table_host is required)"),
    ("a table off a 16-byte boundary", dict(tables=(PTR, 0, PTR + 8)), "the table of block 2 is not 16-byte aligned"),
    ("no prefix offsets", dict(prefix_ptr=None), "bad arguments (prefix_ptr_host is required)"),
    ("prefix offsets start below 0", dict(prefix_ptr=(-1, 7, 7, 15)), "prefix_ptr_host[0] = -1 is negative"),
    ("prefix offsets decrease", dict(prefix_ptr=(0, 7, 6, 15)), "prefix_ptr_host decreases at block 1 (6 after 7)"),
    ("a prefix of 65 bytes", dict(prefix=LONG, prefix_ptr=(0, 0, 65, 65)),
     "block 1 has a prefix of 65 bytes, at most 64 (the lines are staged in LDS)"),
    ("no prefix bytes", dict(prefix=None), "bad arguments (prefix_host is required)"),
    ("kind 1 without flags", dict(kind=1, poly=None), NEED1),
    ("kind 1 without thresholds", dict(kind=1, thr=None), NEED1),
    ("kind 1 without tail offsets", dict(kind=1, tail_ptr=None), NEED1),
]
SIZES_REFUSALS = SHARED_REFUSALS + [
    ("no tile_off", dict(tile_off=None), "bad arguments (tile_off is required)"),
    ("no tile_off, nothing to do", dict(tile_off=None, n_blocks=0, tables=()), "bad arguments (tile_off is required)"),
]
WRITE_REFUSALS = SHARED_REFUSALS + [
    ("out_bytes below 0", dict(out_bytes=-1), "out_bytes < 0 (-1)"),
    ("no out", dict(out=None), "bad arguments (out is NULL with out_bytes = 100)"),
    ("no tile_off", dict(tile_off=None), "bad arguments (tile_off and err are required)"),
    ("no error word", dict(err=None, kind=1), "bad arguments (tile_off and err are required)"),
]


@pytest.mark.parametrize("what,kw,message", SIZES_REFUSALS, ids=[r[0] for r in SIZES_REFUSALS])
def test_sizes_refusals_and_their_messages(lib, what, kw, message):
    assert call(lib, SIZES, **kw) == -1, what
    assert lib.mxm_last_error() == ("%s: %s" % (SIZES, message)).encode(), what


@pytest.mark.parametrize("what,kw,message", WRITE_REFUSALS, ids=[r[0] for r in WRITE_REFUSALS])
def test_write_refusals_and_their_messages(lib, what, kw, message):
    assert call(lib, WRITE, **kw) == -1, what
    assert lib.mxm_last_error() == ("%s: %s" % (WRITE, message)).encode(), what


def test_the_header_lists_every_refusal():
    flat = " ".join(header_text().replace(" * ", " ").split())
    for phrase in ("t NULL", "n_blocks < 0 or n_pos < 0", "a kind other than 0 and 1", "more than 2^31 - 1 tiles", "tile_off NULL",
                   "table_host NULL", "not 16-byte aligned", "prefix_ptr_host NULL", "prefix_ptr_host[0] < 0",
                   "a prefix_ptr_host that decreases", "more than MXM_STATS_MAX_PREFIX bytes", "prefix_host NULL with prefix bytes",
                   "poly, thr or tail_ptr NULL", "out_bytes < 0", "out NULL with out_bytes > 0", "err NULL",
                   "tile_off[0] = 0 is still written"):
        assert phrase in flat, phrase


def test_writing_nothing_is_not_an_error(lib):
    """No block or no line: mxm_stats_text_write returns 0 before the device is looked at (the pointers are not real); an
    empty prefix table needs no prefix bytes.  (mxm_stats_text_sizes still writes tile_off[0]: tests/test_gpu_stats_text.py.)"""
    assert call(lib, WRITE, n_blocks=0, tables=None, prefix=None, prefix_ptr=None) == 0
    assert call(lib, WRITE, n_pos=0, tables=None, prefix=None, prefix_ptr=None, out=None, out_bytes=0) == 0
    assert call(lib, WRITE, kind=1, n_blocks=0, poly=None, thr=None, tail_ptr=None, tail=None) == 0


# ---- the block plan -------------------------------------------------------------------------------------------------
class FakeColumns(object):
    def __init__(self, frag, names):
        self.frag, self.names = numpy.array(frag, dtype=numpy.int64), list(names)

    def __len__(self):
        return len(self.frag)


def hand_made_cohort():
    """Four samples on host tensors: three contributors of which hap2 has no key; one contributor whose 'unassigned' key has
    no label; no contributor at all; ten contributors (hap10 sorts before hap2)."""
    import torch
    from mixemt_amd import assign
    ten = ["hap%d" % i for i in range(1, 11)]
    names = [["hap1", "hap2", "hap3", "unassigned"], ["hap1"], [], ten + ["unassigned"]]
    keys = [["unassigned", "hap3", "hap1"], ["hap1", "unassigned"], [], list(reversed(ten))]
    lab0 = [0, 4, 6, 7, 18]
    parts = [FakeColumns([0, 1], ["a", "b"]), FakeColumns([0], ["c"]), FakeColumns([], []), FakeColumns([0], ["d"])]
    cols = FakeColumns([0, 1, 2, 3], ["a", "b", "c", "d"])
    labels = torch.tensor([0, 3, 4, 16], dtype=torch.int32)
    sample_of = torch.tensor([0, 0, 1, 3], dtype=torch.int32)
    cohort = assign.CohortContribReads(parts, cols, [0, 2, 3, 3, 4], lab0, names, keys, labels, sample_of)
    contribs = [[["hap1", "A1", 0.5], ["hap2", "B2", 0.3], ["hap3", "C3", 0.2]], [["hap1", "D4", 1.0]], [],
                [[name, "H%d" % i, 0.1] for i, name in enumerate(ten)]]
    return cohort, contribs


def test_block_plan_order_prefixes_and_null_tables():
    from mixemt_amd import stats
    cohort, contribs = hand_made_cohort()
    plan = stats._stats_block_plan(contribs, cohort)
    assert plan[2] is None                                            # no contributors: no files
    # keys sorted as strings; hap2 is no key, so it has no block; more than one key: 'all<TAB>mix' last
    assert plan[0] == [(b"hap1\tA1\t", ("label", 0)), (b"hap3\tC3\t", ("label", 2)), (b"unassigned\tunassigned\t", ("label", 3)),
                       (b"all\tmix\t", ("all", 0))]
    # one contributor and an 'unassigned' key the sample has no label for: a table of zeros (NULL); two keys, so 'all'
    assert plan[1] == [(b"hap1\tD4\t", ("label", 4)), (b"unassigned\tunassigned\t", None), (b"all\tmix\t", ("all", 1))]
    order = [p[0].split(b"\t")[0].decode() for p in plan[3]]
    assert order == sorted("hap%d" % i for i in range(1, 11)) + ["all"] and order[:3] == ["hap1", "hap10", "hap2"]
    assert plan[3][1] == (b"hap10\tH9\t", ("label", 7 + 9))
    # one key only: no 'all<TAB>mix' block
    cohort.keys[1] = ["hap1"]
    assert stats._stats_block_plan(contribs, cohort)[1] == [(b"hap1\tD4\t", ("label", 4))]
    # a key that is no contributor is labelled 'unassigned'
    cohort.keys[1] = ["hap1", "hap7"]
    assert stats._stats_block_plan(contribs, cohort)[1][1] == (b"hap7\tunassigned\t", None)


def test_report_contributors_many_adds_the_keys_and_writes_the_tables():
    from mixemt_amd import stats
    cohort, contribs = hand_made_cohort()
    before = [list(k) for k in cohort.keys]
    out = io.StringIO()
    stats.report_contributors_many(out, contribs, cohort, titles=["s0", "s1", "s2", "s3"])
    assert cohort.keys[0] == before[0] + ["hap2"] and cohort.keys[1:] == before[1:]
    want = io.StringIO()
    for s, title in enumerate(["s0", "s1", "s2", "s3"]):
        want.write("# %s\n" % title)
        stats.report_contributors(want, contribs[s], cohort.sample(s))
    assert out.getvalue() == want.getvalue() and "hap1\tA1\t0.5000\t1\n" in out.getvalue()
    assert "hap2\tB2\t0.3000\t0\n" in out.getvalue() and "hap10\tH9\t0.1000\t1\n" in out.getvalue()

    class Tty(io.StringIO):
        def isatty(self):
            return True

    tty, want_tty = Tty(), Tty()
    stats.report_contributors_many(tty, contribs, cohort)
    for s in range(4):
        stats.report_contributors(want_tty, contribs[s], cohort.sample(s))
    assert tty.getvalue() == want_tty.getvalue() and tty.getvalue().count("Haplogroup") == 4
    with pytest.raises(ValueError, match="one contributor table"):
        stats.report_contributors_many(out, contribs[:3], cohort)
    with pytest.raises(ValueError, match="one title"):
        stats.report_contributors_many(out, contribs, cohort, titles=["a"])


class ToyPhylo(object):
    refseq = "ACGTACGTAC"
    hap_var = {"A": ["A1G", "C6T"], "B": ["C6T", "G3A"], "N": []}

    def polymorphic_sites(self, haps):
        return [0, 2] if len(haps) > 1 else []


def test_pos_plan_follows_write_variants_loop():
    from mixemt_amd import stats
    poly, tails, last = stats._stats_pos_plan(ToyPhylo(), [["hap1", "A", 0.6], ["hap2", "B", 0.4]], 10)
    assert poly.tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0] and poly.dtype == numpy.uint8
    assert tails == {0: b"A:A1G", 5: b"A:C6T,B:C6T", 2: b"B:G3A"} and last == 2      # (the LAST variant of the loop, not the largest)
    assert stats._stats_pos_plan(ToyPhylo(), [["hap1", "N", 1.0]], 10)[2] is None
    # positions outside the reference take no part in the table
    assert stats._stats_pos_plan(ToyPhylo(), [["hap1", "A", 1.0]], 3)[1] == {0: b"A:A1G"}


def test_errors_come_before_any_file(tmp_path):
    """A wrong number of tables or prefixes, and a sample whose contributors have no variant: raised before the device is
    asked for and before any file exists."""
    from mixemt_amd import stats
    cohort, contribs = hand_made_cohort()
    args = argparse.Namespace(min_mq=30, min_bq=30, min_var_reads=3, frac_var_reads=0.02)
    prefixes = [str(tmp_path / ("s%d" % s)) for s in range(4)]
    pile = argparse.Namespace(n_samples=4, L=10)
    with pytest.raises(ValueError, match=r"\(4 samples, 4 tables, 4 contributor tables, 3 prefixes\)"):
        stats.write_statistics_many(ToyPhylo(), pile, contribs, cohort, args, prefixes[:3])
    with pytest.raises(ValueError, match=r"\(4 samples, 3 tables, 4 contributor tables, 4 prefixes\)"):
        stats.write_statistics_many(ToyPhylo(), argparse.Namespace(n_samples=3, L=10), contribs, cohort, args, prefixes)
    with pytest.raises(ValueError, match=r"\(4 samples, 4 tables, 2 contributor tables, 4 prefixes\)"):
        stats.write_statistics_many(ToyPhylo(), pile, contribs[:2], cohort, args, prefixes)
    with pytest.raises(ValueError, match="the pileup has 9 positions, the reference 10"):
        stats.write_statistics_many(ToyPhylo(), argparse.Namespace(n_samples=4, L=9), contribs, cohort, args, prefixes)
    toy = [[["hap1", "A", 0.5], ["hap2", "B", 0.3], ["hap3", "A", 0.2]], [["hap1", "N", 1.0]], [], []]
    with pytest.raises(ValueError, match="sample 1: its contributors have no variant at all"):
        stats.write_statistics_many(ToyPhylo(), pile, toy, cohort, args, prefixes)
    assert os.listdir(str(tmp_path)) == []
    assert "split the cohort" in stats.write_statistics_many.__doc__ and stats.MAX_TEXT_BYTES == 2 << 30
