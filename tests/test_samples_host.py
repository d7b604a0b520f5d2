"""
Host side of the batched loop over many samples (mxm_samples_plan, the binding table, run_em_many's init draws):
no device work, runs on a CPU box.
"""
import ctypes

import numpy

from mixemt_amd import _lib, em


def _plan(lib, row0):
    row0 = numpy.ascontiguousarray(row0, dtype=numpy.int64)
    n_samples = len(row0) - 1
    ptr = row0.ctypes.data_as(ctypes.c_void_p)
    n = lib.mxm_samples_plan(ptr, n_samples, None, 0, None)
    if n < 0:
        return n, None, None
    tiles = (_lib.SampleTile * n)()
    tile0 = (ctypes.c_int32 * (n_samples + 1))()
    assert lib.mxm_samples_plan(ptr, n_samples, tiles, n, tile0) == n
    return n, [(t.sample, t.first, t.count) for t in tiles], list(tile0)


def test_tile_plan_covers_every_row_once_and_never_spans_samples():
    lib = _lib.load()
    k = lib.mxm_samples_tile_rows()
    assert 1 <= k <= 64
    rng = numpy.random.default_rng(3)
    counts = [1, 2, k - 1, k, k + 1, 2 * k + 1, 600, 5000] + [int(v) for v in rng.integers(1, 4 * k, size=20)]
    row0 = numpy.concatenate([[0], numpy.cumsum(counts)])
    n, tiles, tile0 = _plan(lib, row0)
    assert n == sum(-(-c // k) for c in counts) and tile0[0] == 0 and tile0[-1] == n
    seen = numpy.zeros(row0[-1], dtype=numpy.int64)
    for i, (sample, first, count) in enumerate(tiles):
        assert 1 <= count <= k
        assert row0[sample] <= first and first + count <= row0[sample + 1]          # inside ONE sample
        assert tile0[sample] <= i < tile0[sample + 1]                               # ... whose tiles are contiguous
        seen[first:first + count] += 1
    assert (seen == 1).all()
    assert [t[0] for t in tiles] == sorted(t[0] for t in tiles)                     # sample order, rows ascending
    assert all(a[1] < b[1] for a, b in zip(tiles, tiles[1:]))


def test_tile_plan_depends_on_the_samples_own_row_count_only():
    lib = _lib.load()
    k = lib.mxm_samples_tile_rows()

    def cut(row0, s):
        _, tiles, tile0 = _plan(lib, row0)
        return [(first - row0[s], count) for _, first, count in tiles[tile0[s]:tile0[s + 1]]]

    for rows in (1, k - 1, k, k + 1, 2 * k + 1, 601):
        alone = cut([0, rows], 0)
        assert alone == [(i * k, min(k, rows - i * k)) for i in range(-(-rows // k))]
        assert cut([0, 7, 7 + rows, 7 + rows + 3 * k], 1) == alone                  # between two others
        assert cut([0, 1000, 1000 + rows], 1) == alone                              # last
        assert cut([0, rows, rows + 5], 0) == alone                                 # first


def test_tile_plan_refuses_empty_samples_and_descending_offsets():
    lib = _lib.load()
    for row0 in ([0, 5, 5, 9], [0, 9, 5, 12], [1, 5], [0]):
        n, _, _ = _plan(lib, row0) if len(row0) > 1 else (lib.mxm_samples_plan(None, 0, None, 0, None), None, None)
        assert n == -1 and lib.mxm_last_error()
    row0 = numpy.array([0, 40, 80], dtype=numpy.int64)
    tiles = (_lib.SampleTile * 1)()
    assert lib.mxm_samples_plan(row0.ctypes.data_as(ctypes.c_void_p), 2, tiles, 1, None) == -1      # no room


def test_binding_declares_the_samples_exports():
    lib = _lib.load()
    for name in ("mxm_samples_plan", "mxm_samples_workspace_bytes", "mxm_em_iter_samples", "mxm_em_loop_samples",
                 "mxm_samples_tile_rows"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == lib.mxm_version()
    assert ctypes.sizeof(_lib.SampleTile) == 16
    # the tile table, the samples' first tiles, a fault word and a partial row of H doubles per tile
    assert lib.mxm_samples_workspace_bytes(19, 1, 5408) >= 19 * (16 + 4 + 5408 * 8) + 2 * 4
    assert lib.mxm_samples_workspace_bytes(0, 1, 5408) == 0
    assert hasattr(em, "run_em_many") and hasattr(em, "SampleBatch")


def test_run_em_many_draws_inits_as_a_loop_of_run_em_would():
    """Sample after sample, n_multi draws each, from numpy's global legacy stream (em.py:23-36, :123)."""
    n_haps = 37
    numpy.random.seed(11)
    want = [numpy.stack([numpy.random.dirichlet([1.0] * n_haps) for _ in range(3)]) for _ in range(4)]
    numpy.random.seed(11)
    got = em.draw_inits_many(4, n_haps, n_multi=3, alpha=1.0)
    assert len(got) == 4 and all(numpy.array_equal(a, b) for a, b in zip(got, want))
    # sample 2 alone, at the same position of the stream, reproduces its own draw
    numpy.random.seed(11)
    em.draw_inits_many(2, n_haps, n_multi=3)
    assert numpy.array_equal(em.draw_inits_many(1, n_haps, n_multi=3)[0], want[2])
    # alpha = inf: the uniform start, no draw consumed
    numpy.random.seed(11)
    flat = em.draw_inits_many(2, n_haps, alpha=float("inf"))
    assert all(numpy.array_equal(f, numpy.full((1, n_haps), 1.0 / n_haps)) for f in flat)
    assert numpy.array_equal(em.draw_inits_many(1, n_haps)[0], want[0][:1])
