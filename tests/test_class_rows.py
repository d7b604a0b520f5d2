"""
The generators of tests/_class_rows.py do what they say, for every parameter set tests/test_gpu_class_edges.py uses: this
module is what makes that one's "exactly 256" mean exactly 256.  CPU only; a generator that misses its target by one
fails here.
"""
import numpy
import pytest

import _class_rows as cr


def _int_label(label):
    return not isinstance(label, str)


# ---------------------------------------------------------------- A. rows with D distinct values
@pytest.mark.parametrize("layout", ["runs", "shuffled"])
@pytest.mark.parametrize("n_haps", cr.ENCODER_WIDTHS + (cr.ENCODER_ODD_WIDTH,))
def test_encoder_rows_hold_exactly_their_number_of_values(n_haps, layout):
    mat, labels = cr.encoder_matrix(n_haps, layout)
    assert mat.shape == (len(labels), n_haps) and numpy.isfinite(mat[[_int_label(v) for v in labels]]).all()
    for row, label in zip(mat, labels):
        if _int_label(label):
            assert cr.n_distinct(row) == label
            assert cr.expected_ndist(row) == (label if label <= 1024 else 0)
    same_as_previous = (cr.bits(mat)[:, 1:] == cr.bits(mat)[:, :-1]).mean(axis=1)
    for share, label in zip(same_as_previous, labels):
        if _int_label(label) and label <= 258:
            # runs: at most one change per value; shuffled: the dominant value's pairs only (0.85^2 on average)
            assert (share >= 1.0 - label / (n_haps - 1.0)) if layout == "runs" else (share < 0.9 or label == 1)
    if n_haps == cr.ENCODER_ODD_WIDTH:
        assert sorted(labels) == [256, 256, 257, 257]
        return
    # every class limit from both sides, the limit rows named for the argmax, 33 rows with wide rows at 31 and 32
    assert len(labels) == 33 and set(cr.ENCODER_D) <= set(labels) and set(cr.ENCODER_LIMIT_D) <= set(cr.ENCODER_D)
    assert all(256 < labels[r] <= 1024 for r in (31, 32))
    assert [v for v in labels if isinstance(v, str)] == list(cr.ENCODER_SPECIAL)
    assert mat.flags.writeable is False


@pytest.mark.parametrize("n_haps", cr.ENCODER_WIDTHS)
def test_special_rows_are_what_their_names_say(n_haps):
    mat, labels = cr.encoder_matrix(n_haps, "runs")
    rows = {label: row for row, label in zip(mat, labels) if isinstance(label, str)}
    assert cr.n_distinct(rows["collide256"]) == 256 and cr.n_distinct(rows["collide1024"]) == 1024
    assert len(set(cr.encoder_slot(rows["collide256"], 1024))) == 1
    assert len(set(cr.encoder_slot(rows["collide1024"], 4096))) == 1
    for name in ("collide256", "collide1024"):
        assert numpy.isfinite(rows[name]).all() and rows[name].min() >= -60.0 and rows[name].max() <= 0.0
    zeros = rows["zeros"]
    assert cr.n_distinct(zeros) == 256 and len(numpy.unique(zeros)) == 255          # by value the two zeros are one
    assert (zeros == 0).any() and numpy.signbit(zeros[zeros == 0]).any() and not numpy.signbit(zeros[zeros == 0]).all()
    nans = rows["nans"]
    payloads = numpy.unique(cr.bits(nans[numpy.isnan(nans)]))
    assert len(payloads) == 2 and -1 not in payloads and cr.n_distinct(nans) == 9 and cr.expected_ndist(nans) == 9
    neginf = rows["neginf"]
    assert (neginf == -numpy.inf).sum() == n_haps // 3 and cr.expected_ndist(neginf) == 6
    ones = rows["allones"]
    assert (cr.bits(ones) == -1).sum() == 1 and cr.n_distinct(ones) == 9 and cr.expected_ndist(ones) == 0
    assert numpy.isfinite(numpy.delete(ones, numpy.flatnonzero(cr.bits(ones) == -1))).all()


@pytest.mark.parametrize("n,slots", [(256, 1024), (1024, 4096)])
def test_colliding_keys_share_one_slot(n, slots):
    keys = cr.colliding_keys(n, slots)
    assert keys.shape == (n,) and len(numpy.unique(cr.bits(keys))) == n
    assert numpy.isfinite(keys).all() and keys.min() >= -60.0 and keys.max() <= 0.0
    assert len(set(cr.encoder_slot(keys, slots))) == 1
    # the restated slot function on one key, in Python integers
    key = int(cr.bits(keys[:1])[0]) & ((1 << 64) - 1)
    want = (((key ^ (key >> 29)) * 0x9E3779B97F4A7C15 & ((1 << 64) - 1)) >> 40) & (slots - 1)
    assert int(cr.encoder_slot(keys[:1], slots)[0]) == want


# ---------------------------------------------------------------- B. rows with Q distinct quads
@pytest.mark.parametrize("n_haps", cr.QUAD_WIDTHS)
def test_quad_rows_hold_exactly_their_values_and_quads(n_haps):
    pool = cr.quad_pool(n_haps)
    classes = cr.quad_classes(n_haps)
    assert set(q for _, q in classes) == {1, 255, 256, 257, n_haps // 4}
    assert set(d for d, _ in classes) == {4, 64, 256}
    for d, q in classes:
        row = pool[(d, q)]
        assert row.shape == (n_haps,) and cr.n_distinct(row) == d and cr.n_quads(row) == q, (d, q)
    assert cr.n_distinct(pool["wide"]) == 300 and cr.n_distinct(pool["none"]) == 1025
    with pytest.raises(AssertionError):
        cr.rows_with_quads(n_haps, 4, [257], 1)                   # four values make 256 quadruples, not 257
    with pytest.raises(AssertionError):
        cr.rows_with_quads(n_haps, 64, [15], 1)                   # 64 values do not fit 15 quads


@pytest.mark.parametrize("n_rows", cr.QUAD_ROW_COUNTS)
@pytest.mark.parametrize("n_haps", cr.QUAD_WIDTHS)
def test_quad_matrices_interleave_the_classes(n_haps, n_rows):
    mat, kinds = cr.quad_matrix(n_haps, n_rows)
    assert mat.shape == (n_rows, n_haps) and len(kinds) == n_rows
    for i, (row, kind) in enumerate(zip(mat, kinds)):
        if kind == "wide":
            assert i % 4 == 2 and cr.n_distinct(row) == 300
        elif kind == "none":
            assert i % 4 == 3 and cr.n_distinct(row) == 1025
        else:
            d, q = kind
            assert i % 4 == (0 if q <= 256 else 1) and cr.n_distinct(row) == d and cr.n_quads(row) == q
    if n_rows == 130:                                             # every class occurs
        assert set(k for k in kinds if not isinstance(k, str)) == set(cr.quad_classes(n_haps))


def test_the_last_row_is_a_quad_row_once_and_a_row_without_a_record_once():
    last = {n: cr.quad_matrix(1028, n)[1][-1] for n in cr.QUAD_ROW_COUNTS}
    assert last[64] == "none" and not isinstance(last[65], str) and last[65][1] <= 256


# ---------------------------------------------------------------- C. tables with K masks and E marker entries
@pytest.mark.parametrize("dyadic", [False, True])
@pytest.mark.parametrize("part", ["short", "long"])
@pytest.mark.parametrize("n_haps", cr.MARKER_WIDTHS)
def test_marker_rows_have_the_intended_facts(n_haps, part, dyadic):
    tables, (row_ptr, site, obs), case_of_row = cr.marker_input(n_haps, part, dyadic)
    cases = cr.marker_case_list(n_haps, part)
    assert tables.lut() is not None and tables.n_haps == n_haps
    assert (tables.sparse()["maj"] == cr.REF_BASE).all()
    seen = []
    for r, c in enumerate(case_of_row):
        sl = slice(row_ptr[r], row_ptr[r + 1])
        if c < 0:
            assert row_ptr[r + 1] - row_ptr[r] == cr.FILLER_SITES
            continue
        assert case_of_row[r - 1] in (c, -1) and case_of_row[r + 1] in (c, -1)        # limit rows: never first, never last
        if case_of_row[r - 1] == c:
            assert numpy.array_equal(site[sl], site[row_ptr[r - 1]:row_ptr[r]])       # ... and each one twice, side by side
            continue
        n, n_masks, n_entries, n_values = cr.row_facts(tables, site[sl], obs[sl])
        want_n, want_k, want_e = cases[c]
        assert (n, n_masks) == (want_n, want_k), (cases[c], n, n_masks)
        if want_e is not None:
            assert n_entries == want_e, (cases[c], n_entries)
        elif 64 < n <= 128:
            assert n_entries <= cr.LONG_MAX_ENTRIES, (cases[c], n_entries)            # the MASKS decide this row's class
        if dyadic:
            sizes = set(len(p) for p in cr._patterns(want_n, want_k + 1))
            assert n_values == len(sizes) <= 5                                         # one exact sum per pattern size
        else:
            assert n_values == want_k + 1                                              # one value per mask
        seen.append(c)
    assert seen == list(range(len(cases)))
    wanted = cr.MARKER_SHORT if part == "short" else cr.MARKER_LONG
    assert [(n, k) for n, k, e in cases if e is None] == wanted
    entries = [(n, k, e) for n, k, e in cases if e is not None]
    if part == "short":
        assert entries == cr.MARKER_ENTRIES_SHORT
    else:
        assert entries == (cr.MARKER_ENTRIES_LONG if n_haps >= 5408 else [])


def test_the_issues_counts_with_2050_haplogroups():
    """64 / 128 sites, haplogroups dealt round-robin: exactly K + 1 masks for every K + 1 at a class limit; as many
    values as masks with generic terms, three values with dyadic ones (sizes 0, 1, 2)."""
    for n_patterns in (256, 257, 353, 354, 705, 706, 1024, 1025):
        for n_sites in (64, 128):
            for dyadic in (False, True):
                tables = cr.counting_tables(2050, n_sites, n_patterns, dyadic)
                row_ptr, site, obs = cr.all_reference_rows([numpy.arange(n_sites)])
                n, n_masks, n_entries, n_values = cr.row_facts(tables, site, obs)
                assert (n, n_masks + 1) == (n_sites, n_patterns)
                assert n_values == (3 if dyadic else n_patterns)
                assert tables.lut() is not None


def test_extra_carriers_add_entries_and_no_masks():
    base = cr.row_facts(cr.counting_tables(5408, 128, 101, False, 0), numpy.arange(128), numpy.full(128, cr.REF_BASE))
    more = cr.row_facts(cr.counting_tables(5408, 128, 101, False, 4000), numpy.arange(128), numpy.full(128, cr.REF_BASE))
    assert base[:2] == more[:2] == (128, 100) and more[2] == base[2] + 4000 and base[3] == more[3] == 101
    with pytest.raises(AssertionError):
        cr.counting_tables(2050, 128, 101, False, 5020)           # (not enough haplogroups: the long E cases need 5408)
    with pytest.raises(AssertionError, match="majority"):
        cr.counting_tables(64, 4, 16, False, None)                # every site on half the haplogroups


def test_marker_class_names_the_documented_limits():
    assert [cr.marker_class(n, k, 0) for n, k in ((64, 352), (64, 353), (65, 704), (65, 705), (128, 704), (129, 1))] == \
        ["short", "fallback", "long", "fallback", "long", "fallback"]
    assert cr.marker_class(128, 100, 5120) == "long" and cr.marker_class(128, 100, 5121) == "fallback"
    assert cr.marker_class(64, 100, 99999) == "short"            # the short instance walks on: no entry limit
    assert cr.marker_class(65, 10, 10, long_rows=False) == "fallback" and cr.marker_class(64, 10, 10, long_rows=False) == "short"
