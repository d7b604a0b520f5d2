"""
The HOST entries of include/mixemt_hip.h that write into caller-sized host buffers -- mxm_encode_signatures (`cap`),
mxm_samples_plan (`cap`), mxm_aln_fetch, mxm_aln_fetch_fragments, mxm_bam_fetch_names -- with every output a guard-banded
numpy buffer (tests/_guarded.py) of exactly the size the header or the entry's *_sizes_of reports, and with a `cap` that
is one too small where the entry takes one.  No GPU.
"""
import ctypes

import numpy
import pytest

import _bam_writer as bw
from _guarded import guarded, guarded_from
from mixemt_amd import _lib, alignments, synth


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _check_all(bufs, what):
    for name, buf in bufs.items():
        buf.check("%s (%s)" % (name, what))


# ---- mxm_encode_signatures ------------------------------------------------------------------------------------------------
def _signatures(rng, n_rows, ref_len, sites):
    sigs, want_site, want_obs, row_ptr = [], [], [], [0]
    for _ in range(n_rows):
        picked = numpy.sort(rng.choice(len(sites), size=int(rng.integers(1, 9)), replace=False))
        items = []
        for k in picked:
            base = "ACGT"[int(rng.integers(0, 4))] if rng.random() > 0.1 else "AC"           # not one character: obs 0
            items.append("%d:%s" % (sites[k], base))
            want_site.append(k)
            want_obs.append(ord(base) if len(base) == 1 else 0)
        sigs.append(",".join(items))
        row_ptr.append(len(want_site))
    return sigs, numpy.array(row_ptr, dtype=numpy.int64), numpy.array(want_site, dtype=numpy.uint16), \
        numpy.array(want_obs, dtype=numpy.uint8)


@pytest.mark.parametrize("n_rows", [1, 257, 700])
def test_encode_signatures_fills_exactly_cap_and_stops_one_short(lib, n_rows):
    """mixemt_hip.h: "row_ptr[R+1], site[cap], obs[cap] outputs ... Returns the number of observations written (>= 0), or
    -(r + 1) when signature r needs the caller's slow path: ... or more than `cap` observations"."""
    rng = numpy.random.default_rng(n_rows)
    ref_len = 16569
    sites = numpy.sort(rng.choice(ref_len, size=900, replace=False))
    sites[-1] = ref_len - 1
    site_of_pos = numpy.full(ref_len, -1, dtype=numpy.int32)
    site_of_pos[sites] = numpy.arange(len(sites), dtype=numpy.int32)
    sigs, want_ptr, want_site, want_obs = _signatures(rng, n_rows, ref_len, sites)
    text = ("\n".join(sigs) + "\n").encode("ascii")
    off = numpy.zeros(n_rows + 1, dtype=numpy.int64)
    numpy.cumsum([len(s) + 1 for s in sigs], out=off[1:])
    nnz = int(want_ptr[-1])
    for cap in (nnz, nnz - 1):
        bufs = {"row_ptr": guarded(8 * (n_rows + 1), 8), "site": guarded(2 * cap, 2), "obs": guarded(cap, 1)}
        got = lib.mxm_encode_signatures(text, off.ctypes.data, n_rows, site_of_pos.ctypes.data, ref_len, bufs["row_ptr"].ptr,
                                        bufs["site"].ptr, bufs["obs"].ptr, cap)
        _check_all(bufs, "R=%d cap=%d" % (n_rows, cap))
        if cap == nnz:
            assert got == nnz
            assert numpy.array_equal(bufs["row_ptr"].get(numpy.int64), want_ptr)
            assert numpy.array_equal(bufs["site"].get(numpy.uint16), want_site)
            assert numpy.array_equal(bufs["obs"].get(numpy.uint8), want_obs)
        else:
            assert got == -n_rows                           # the LAST signature is the one that no longer fits
            assert numpy.array_equal(bufs["site"].get(numpy.uint16), want_site[:cap])
            assert numpy.array_equal(bufs["obs"].get(numpy.uint8), want_obs[:cap])
            assert numpy.array_equal(bufs["row_ptr"].get(numpy.int64)[:n_rows], want_ptr[:n_rows])


# ---- mxm_samples_plan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [(1,), (1, 64, 65), (32, 33, 1, 700), (257,)])
def test_samples_plan_fills_exactly_cap_and_refuses_one_short(lib, rows):
    """mixemt_hip.h: "cuts every sample into tiles of at most MXM_SAMPLES_TILE_ROWS consecutive rows of that sample -- full
    tiles, then the remainder ...  Returns the number of tiles (-1: ... or cap too small); tiles_host[cap] (nullable: count
    only) receives the tiles in sample order, tile0_host[S + 1] (nullable) each sample's first tile"."""
    tile_rows = lib.mxm_samples_tile_rows()
    n_samples = len(rows)
    row0 = numpy.zeros(n_samples + 1, dtype=numpy.int64)
    numpy.cumsum(rows, out=row0[1:])
    want, want0 = [], [0]
    for s, n in enumerate(rows):
        for first in range(0, n, tile_rows):
            want.append((s, min(tile_rows, n - first), int(row0[s]) + first))
        want0.append(len(want))
    assert lib.mxm_samples_plan(row0.ctypes.data, n_samples, None, 0, None) == len(want)      # count only
    tiles = guarded(16 * len(want), 8)
    tile0 = guarded(4 * (n_samples + 1), 4)
    assert lib.mxm_samples_plan(row0.ctypes.data, n_samples, tiles.ptr, len(want), tile0.ptr) == len(want)
    tiles.check("tiles_host")
    tile0.check("tile0_host")
    got = (_lib.SampleTile * len(want)).from_buffer_copy(tiles.get(numpy.uint8).tobytes())
    assert [(t.sample, t.count, t.first) for t in got] == want
    assert list(tile0.get(numpy.int32)) == want0
    short = guarded(16 * (len(want) - 1), 8)
    tile0 = guarded(4 * (n_samples + 1), 4)
    assert lib.mxm_samples_plan(row0.ctypes.data, n_samples, short.ptr, len(want) - 1, tile0.ptr) == -1
    assert b"room for %d tiles" % (len(want) - 1) in lib.mxm_last_error()
    short.check("tiles_host one tile short")
    tile0.check("tile0_host one tile short")


# ---- mxm_aln_fetch / mxm_aln_fetch_fragments ------------------------------------------------------------------------------
def test_aln_fetch_into_buffers_of_exactly_the_reported_sizes(lib, b17):
    """mixemt_hip.h: "sizes via mxm_aln_sizes_of, copies via mxm_aln_fetch* (NULL = not wanted)": row_ptr[n_rows+1],
    site[nnz], obs[nnz], weights[n_rows], group_ptr[n_rows+1], group_frag[n_grouped], dropped[n_dropped],
    text[text_bytes], text_off[n_rows+1]; frag_id[n_frag_seen], frag_ptr[n_frag_seen+1], site / obs [frag_nnz]."""
    refseq, phy, haps, tables = b17
    cols = synth.synth_alignments(tables, refseq, 300, seed=5)
    want = alignments.encode_alignments(cols, tables.sites, len(refseq), 30, 30)
    sites = numpy.ascontiguousarray(tables.sites, dtype=numpy.int64)
    site_of_pos = numpy.full(len(refseq), -1, dtype=numpy.int32)
    site_of_pos[sites] = numpy.arange(len(sites), dtype=numpy.int32)
    st, keep = cols.struct()
    handle = ctypes.c_void_p()
    assert lib.mxm_aln_encode(ctypes.byref(st), site_of_pos.ctypes.data, len(refseq), sites.ctypes.data, len(sites), 30, 30, 2,
                              ctypes.byref(handle)) == 0, lib.mxm_last_error()
    try:
        sz = _lib.AlnSizes()
        assert lib.mxm_aln_sizes_of(handle, ctypes.byref(sz)) == 0
        assert sz.n_rows > 100 and sz.nnz > sz.n_rows and sz.n_grouped >= sz.n_rows and sz.frag_nnz > 0
        bufs = {"row_ptr": guarded(8 * (sz.n_rows + 1), 8), "site": guarded(2 * sz.nnz, 2), "obs": guarded(sz.nnz, 1),
                "weights": guarded(8 * sz.n_rows, 8), "group_ptr": guarded(8 * (sz.n_rows + 1), 8),
                "group_frag": guarded(8 * sz.n_grouped, 8), "dropped": guarded(8 * sz.n_dropped, 8),
                "text": guarded(sz.text_bytes, 1), "text_off": guarded(8 * (sz.n_rows + 1), 8)}
        order = ["row_ptr", "site", "obs", "weights", "group_ptr", "group_frag", "dropped", "text", "text_off"]
        assert lib.mxm_aln_fetch(handle, *[bufs[k].ptr for k in order]) == 0, lib.mxm_last_error()
        _check_all(bufs, "all wanted")
        assert numpy.array_equal(bufs["row_ptr"].get(numpy.int64), want.row_ptr)
        assert numpy.array_equal(bufs["site"].get(numpy.uint16), want.site)
        assert numpy.array_equal(bufs["obs"].get(numpy.uint8), want.obs)
        assert numpy.array_equal(bufs["weights"].get(numpy.int64), want.weights)
        text = bufs["text"].get(numpy.uint8).tobytes().decode("ascii")
        assert text.split("\n")[:-1] == want.signatures() and text.endswith("\n")
        text_off = bufs["text_off"].get(numpy.int64)
        assert text_off[0] == 0 and text_off[-1] == sz.text_bytes and (numpy.diff(text_off) > 0).all()
        group_ptr = bufs["group_ptr"].get(numpy.int64)
        assert group_ptr[0] == 0 and group_ptr[-1] == sz.n_grouped
        assert numpy.array_equal(numpy.diff(group_ptr), want.weights)
        assert sorted(bufs["group_frag"].get(numpy.int64).tolist() + bufs["dropped"].get(numpy.int64).tolist()) == \
            sorted(set(int(f) for f in bufs["group_frag"].get(numpy.int64)) | set(int(f) for f in bufs["dropped"].get(numpy.int64)))
        # one output at a time, the others not wanted: each copy stays inside its own buffer
        for k in order:
            one = guarded(bufs[k].nbytes, bufs[k].align)
            assert lib.mxm_aln_fetch(handle, *[one.ptr if name == k else None for name in order]) == 0
            one.check(k + " alone")
            assert numpy.array_equal(one.get(numpy.uint8), bufs[k].get(numpy.uint8)), k
        frag = {"frag_id": guarded(8 * sz.n_frag_seen, 8), "frag_ptr": guarded(8 * (sz.n_frag_seen + 1), 8),
                "site": guarded(2 * sz.frag_nnz, 2), "obs": guarded(sz.frag_nnz, 1)}
        assert lib.mxm_aln_fetch_fragments(handle, frag["frag_id"].ptr, frag["frag_ptr"].ptr, frag["site"].ptr,
                                           frag["obs"].ptr) == 0, lib.mxm_last_error()
        _check_all(frag, "fragments")
        frag_ptr = frag["frag_ptr"].get(numpy.int64)
        assert frag_ptr[0] == 0 and frag_ptr[-1] == sz.frag_nnz and (numpy.diff(frag_ptr) >= 0).all()
        # process_reads' own result through the binding's plain buffers: the same fragments, sites and bases
        names = cols.names
        got_obs = {}
        f_id, f_site, f_obs = frag["frag_id"].get(numpy.int64), frag["site"].get(numpy.uint16), frag["obs"].get(numpy.uint8)
        for k, f in enumerate(f_id):
            a, b = int(frag_ptr[k]), int(frag_ptr[k + 1])
            got_obs[names[int(f)]] = {int(sites[s]): chr(o) for s, o in zip(f_site[a:b], f_obs[a:b])}
        assert got_obs == want.read_obs(tables.sites)
    finally:
        lib.mxm_aln_free(handle)
        del keep


# ---- mxm_bam_fetch_names --------------------------------------------------------------------------------------------------
def test_bam_fetch_names_into_buffers_of_exactly_the_reported_sizes(lib, b17, tmp_path):
    """mixemt_hip.h: "names[names_bytes] / name_off[n_frag+1]: the fragments' read names back to back; ref_id[n_aln],
    flag[n_aln] ...; NULL = not wanted"."""
    refseq, phy, haps, tables = b17
    cols = synth.synth_alignments(tables, refseq, 200, seed=9)
    path = str(tmp_path / "reads.bam")
    flags = (numpy.arange(len(cols)) % 7 * 16).astype(numpy.int64).tolist()
    bw.write_bam(path, cols, flag=flags, ref_id=[0] * len(cols), block_bytes=4096, level=1)
    want = alignments.read_bam(path)
    handle = ctypes.c_void_p()
    assert lib.mxm_bam_read(path.encode(), 2, ctypes.byref(handle)) == 0, lib.mxm_last_error()
    try:
        sz = _lib.BamSizes()
        assert lib.mxm_bam_sizes_of(handle, ctypes.byref(sz)) == 0
        assert sz.n_aln == len(cols) and sz.n_frag == cols.n_frag and sz.names_bytes > sz.n_frag
        bufs = {"names": guarded(sz.names_bytes, 1), "name_off": guarded(8 * (sz.n_frag + 1), 8),
                "ref_id": guarded(4 * sz.n_aln, 4), "flag": guarded(2 * sz.n_aln, 2)}
        order = ["names", "name_off", "ref_id", "flag"]
        assert lib.mxm_bam_fetch_names(handle, *[bufs[k].ptr for k in order]) == 0, lib.mxm_last_error()
        _check_all(bufs, "all wanted")
        name_off = bufs["name_off"].get(numpy.int64)
        names = bufs["names"].get(numpy.uint8).tobytes()
        assert name_off[0] == 0 and name_off[-1] == sz.names_bytes
        got_names = [names[int(name_off[i]):int(name_off[i + 1])].decode("ascii") for i in range(sz.n_frag)]
        assert got_names == list(want.names)
        assert numpy.array_equal(bufs["ref_id"].get(numpy.int32), want.ref_id)
        assert numpy.array_equal(bufs["flag"].get(numpy.uint16), want.flag) and bufs["flag"].get(numpy.uint16).tolist() == flags
        for k in order:
            one = guarded(bufs[k].nbytes, bufs[k].align)
            assert lib.mxm_bam_fetch_names(handle, *[one.ptr if name == k else None for name in order]) == 0
            one.check(k + " alone")
            assert numpy.array_equal(one.get(numpy.uint8), bufs[k].get(numpy.uint8)), k
    finally:
        lib.mxm_bam_free(handle)
