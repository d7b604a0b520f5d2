"""
Rows made to order for the class limits of the four producers (tests/test_class_rows.py checks every generator on the
CPU, tests/test_gpu_class_edges.py feeds them to the device).  Host only, numpy only.

  producer                         counts                                            limits
  mxm_encode_rows                  D  distinct bit patterns of a row                 256 (byte codes), 1024 (16-bit codes)
  mxm_build_quads (both encoders)  Q  distinct aligned quads of a byte-coded row     256
  marker build, dense and records  n  observed sites, K distinct non-zero flip       64 / 128 sites, 352 / 704 masks,
                                   masks, E marker entries of the row                5120 entries (long instance)

    rows_with_values(H, d_list, seed, layout)       row i holds exactly d_list[i] distinct bit patterns
    rows_with_quads(H, d, q_list, seed)             ... exactly d values and exactly q_list[i] distinct aligned quads
    special_rows(H, seed)                           the encoder's odd inputs: colliding keys, both zeros, NaNs, -inf, all ones
    counting_tables(H, n_sites, n_patterns, ...)    HapVarTables whose all-reference row has exactly n_patterns - 1 masks
    join_tables(blocks)                             several of them side by side (one block of sites each)
    row_facts(tables, row_sites, row_obs)           (n, K, E, n_values) of a CSR row, from tables.sparse() and the C oracle
    colliding_keys(n, slots, seed)                  n doubles that encode_one_row's slot function sends to ONE slot
"""
import functools
import itertools
import math
import struct

import numpy

ALL_ONES = struct.unpack("<d", b"\xff" * 8)[0]          # the encoder's empty marker: a row that holds it gets no record
REF_BASE, DER_BASE = ord("A"), ord("G")


def bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


def n_distinct(row):
    """Distinct BIT PATTERNS of a row (+0.0 and -0.0 are two, NaN payloads count each)."""
    return len(numpy.unique(bits(row)))


def n_quads(row):
    """Distinct aligned groups of four columns, by bit pattern (the row's width is a multiple of 4)."""
    return len(numpy.unique(bits(row).reshape(-1, 4), axis=0))


def _run_lengths(rng, n_items, n_cells):
    """Every item at least once, the rest dealt as real rows deal them: one item holds most of the row."""
    assert 1 <= n_items <= n_cells, (n_items, n_cells)
    share = numpy.full(n_items, 0.15 / max(1, n_items - 1))
    share[0] = 0.85 if n_items > 1 else 1.0
    return 1 + rng.multinomial(n_cells - n_items, share / share.sum())


def _distinct_normals(rng, n):
    vals = rng.normal(-20.0, 6.0, size=n)
    while len(numpy.unique(vals.view(numpy.int64))) != n:               # (2^-50 per pair: the loop is for the record)
        vals = rng.normal(-20.0, 6.0, size=n)
    return vals


def row_from_values(vals, H, rng, layout="runs"):
    """A row of H cells that holds every one of `vals`: in runs (a value's cells are neighbours, the runs in random order
    -- the encoder's "same as my previous column" shortcut serves most cells) or fully shuffled (it serves almost none)."""
    vals = numpy.asarray(vals, dtype=numpy.float64)
    counts = _run_lengths(rng, len(vals), H)
    order = rng.permutation(len(vals))
    row = numpy.repeat(vals[order], counts[order])
    if layout == "shuffled":
        row = row[rng.permutation(H)]
    else:
        assert layout == "runs", layout
    return row


def rows_with_values(H, d_list, seed, layout="runs"):
    """Dense fp64 log matrix [len(d_list)][H]: row i holds exactly d_list[i] distinct bit patterns, each at least once;
    values N(-20, 6)."""
    rng = numpy.random.default_rng(seed)
    mat = numpy.empty((len(d_list), H))
    for i, d in enumerate(d_list):
        mat[i] = row_from_values(_distinct_normals(rng, int(d)), H, rng, layout)
    return mat


def rows_with_quads(H, d, q_list, seed):
    """[len(q_list)][H]: row i holds exactly d <= 256 distinct values and exactly q_list[i] distinct aligned quads
    (ceil(d / 4) <= q <= min(H / 4, d^4)); the quads come in runs, one of them holding most of the row."""
    assert H % 4 == 0 and 1 <= d <= 256, (H, d)
    rng = numpy.random.default_rng(seed)
    n_pos = H // 4
    n_cover = (d + 3) // 4
    mat = numpy.empty((len(q_list), H))
    for i, q in enumerate(q_list):
        q = int(q)
        assert n_cover <= q <= n_pos and q <= d ** 4, (d, q, n_pos)
        vals = _distinct_normals(rng, d)
        # the first ceil(d / 4) quadruples use every value; the others are drawn from all d^4, without repeats
        cover = [tuple((4 * k + e) % d for e in range(4)) for k in range(n_cover)]
        chosen = set(cover)
        if d ** 4 <= 65536:
            every = [c for c in itertools.product(range(d), repeat=4) if c not in chosen]
            for k in rng.permutation(len(every))[:q - n_cover]:
                chosen.add(every[k])
        else:
            while len(chosen) < q:
                chosen.add(tuple(int(v) for v in rng.integers(0, d, size=4)))
        quads = numpy.array(sorted(chosen), dtype=numpy.int64)[rng.permutation(q)]
        counts = _run_lengths(rng, q, n_pos)
        mat[i] = vals[numpy.repeat(quads, counts, axis=0)].reshape(-1)
    return mat


# ---------------------------------------------------------------- the encoder's hash
def encoder_slot(keys, slots):
    """RESTATED from csrc/coded_kernels.hpp (encode_one_row): ((key ^ key >> 29) * 0x9E3779B97F4A7C15 >> 40) & (slots - 1)
    on the 64-bit pattern of the value.  Nothing asserted about a colliding row depends on it: when the kernel's hash
    changes, such a row stays a valid input and only stops being the longest probe chain."""
    key = numpy.ascontiguousarray(keys, dtype=numpy.float64).view(numpy.uint64)
    mixed = (key ^ (key >> numpy.uint64(29))) * numpy.uint64(0x9E3779B97F4A7C15)        # (wraps modulo 2^64, as in C)
    return ((mixed >> numpy.uint64(40)) & numpy.uint64(slots - 1)).astype(numpy.int64)


@functools.lru_cache(maxsize=None)
def _colliding(n, slots, seed):
    rng = numpy.random.default_rng(seed)
    pool = numpy.unique(rng.uniform(-60.0, 0.0, size=max(3_000_000, 5 * n * slots // 4 + 1_000_000)))
    slot = encoder_slot(pool, slots)
    best = int(numpy.bincount(slot, minlength=slots).argmax())
    keys = pool[slot == best]
    assert len(keys) >= n, (len(keys), n)
    keys = keys[:n].copy()
    keys.setflags(write=False)
    return keys


def colliding_keys(n, slots, seed=0):
    """n distinct finite doubles in [-60, 0] that share one slot of a `slots`-entry table under encoder_slot."""
    return _colliding(int(n), int(slots), int(seed))


def special_rows(H, seed):
    """{name: row[H]} -- valid inputs of mxm_encode_rows that are not N(-20, 6) draws:
      collide256 / collide1024   256 / 1024 values in one hash slot (tables of 1024 / 4096 slots): D = 256 / 1024
      zeros                      +0.0 and -0.0 beside 254 other values: D = 256 only if the two zeros count as two
      nans                       two NaNs of different payloads (neither all ones) beside 7 values: D = 9
      neginf                     -inf in a third of the columns beside 5 values: D = 6
      allones                    the pattern 0xFFFFFFFFFFFFFFFF once beside 8 values: no record (the table's empty marker)
    """
    rng = numpy.random.default_rng(seed)
    rows = {}
    rows["collide256"] = row_from_values(colliding_keys(256, 1024), H, rng)
    if H >= 1024:
        rows["collide1024"] = row_from_values(colliding_keys(1024, 4096), H, rng, "shuffled")
    rows["zeros"] = row_from_values(numpy.concatenate([[0.0, -0.0], _distinct_normals(rng, 254)]), H, rng)
    nans = numpy.array([0x7FF8000000000001, 0xFFF0000000ABCDEF], dtype=numpy.uint64).view(numpy.float64)
    rows["nans"] = row_from_values(numpy.concatenate([nans, _distinct_normals(rng, 7)]), H, rng, "shuffled")
    neginf = row_from_values(_distinct_normals(rng, 5), H, rng)
    neginf[rng.permutation(H)[:H // 3]] = -numpy.inf
    assert n_distinct(neginf) == 6
    rows["neginf"] = neginf
    ones = row_from_values(_distinct_normals(rng, 8), H, rng)
    uniq, count = numpy.unique(ones, return_counts=True)
    most = numpy.flatnonzero(ones == uniq[count.argmax()])
    ones[most[len(most) // 2]] = ALL_ONES                   # one cell of the row's most frequent value
    rows["allones"] = ones
    return rows


def expected_ndist(row):
    """mxm_encode_rows' class of a row, from its bit patterns alone: D up to 1024, 0 (no record) beyond or with the
    all-ones pattern in it."""
    b = bits(row)
    d = len(numpy.unique(b))
    return 0 if (d > 1024 or (b == -1).any()) else d


# ---------------------------------------------------------------- tables whose rows hold a chosen number of masks
def _patterns(n_sites, n_patterns):
    """The empty set, every single site, every pair, every triple, ... of range(n_sites): the first n_patterns of them.
    The subsets of one size are taken with a fixed stride through their lexicographic list, so that a part of them does
    not lean on the first sites (the first 127 pairs of 128 sites in lexicographic order all hold site 0)."""
    out = []
    for size in range(n_sites + 1):
        combos = list(itertools.combinations(range(n_sites), size))
        stride = max(1, int(len(combos) * 0.618))
        while math.gcd(stride, len(combos)) != 1:
            stride += 1
        for k in range(len(combos)):
            out.append(combos[k * stride % len(combos)])
            if len(out) == n_patterns:
                return out
    raise ValueError("%d sites have only %d subsets" % (n_sites, len(out)))


def counting_tables(H, n_sites, n_patterns, dyadic=False, extra_carriers=None, seed=0):
    """
    preprocess.HapVarTables over n_sites sites, reference base A everywhere, in which haplogroup h carries the derived base
    G at the sites of ITS pattern (a subset of the sites; _patterns).  A row that observes A at every site then holds
    exactly n_patterns - 1 distinct non-zero flip masks (K), one per non-empty pattern.
      extra_carriers None: the haplogroups are dealt round-robin over the patterns (h -> pattern h % n_patterns).
      extra_carriers m >= 0: haplogroup h < n_patterns carries pattern h, the next m haplogroups repeat the single-site
        patterns in turn, all others carry nothing.  Each repeat adds ONE marker entry (E) and no mask.
      dyadic: lhit = -0.25 and lmiss = -8.0 at every site -- all sums exact, a row holds one value per pattern SIZE;
        otherwise mu ~ U(1e-4, 0.3) per site and a row holds one value per mask.
    The carriers of a site stay below H / 2, so the reference base remains the majority base (asserted).
    """
    from mixemt_amd import preprocess
    assert n_patterns <= H, (n_patterns, H)
    pats = _patterns(n_sites, n_patterns)
    if extra_carriers is None:
        of_hap = numpy.arange(H) % n_patterns
    else:
        n_single = min(n_sites, n_patterns - 1)
        assert n_single >= 1 and n_patterns + extra_carriers <= H, (n_patterns, extra_carriers, H)
        of_hap = numpy.zeros(H, dtype=numpy.int64)
        of_hap[:n_patterns] = numpy.arange(n_patterns)
        of_hap[n_patterns:n_patterns + extra_carriers] = 1 + numpy.arange(extra_carriers) % n_single
    carries = numpy.zeros((n_patterns, n_sites), dtype=bool)
    for k, combo in enumerate(pats):
        carries[k, list(combo)] = True
    lde = (H + 15) // 16 * 16
    expected = numpy.zeros((n_sites, lde), dtype=numpy.uint8)
    expected[:, :H] = numpy.where(carries[of_hap].T, DER_BASE, REF_BASE)
    assert int((expected[:, :H] == DER_BASE).sum(axis=1).max()) < H / 2.0, "the reference base must stay the majority"
    if dyadic:
        lhit, lmiss = numpy.full(n_sites, -0.25), numpy.full(n_sites, -8.0)
    else:
        mu = numpy.random.default_rng(seed).uniform(1e-4, 0.3, size=n_sites)
        lhit, lmiss = numpy.log(1.0 - mu), numpy.log(mu / 3.0)
    names = ["h%d" % h for h in range(H)]
    return preprocess.HapVarTables(numpy.arange(n_sites, dtype=numpy.int64), expected, lhit, lmiss, names, H)


def join_tables(blocks):
    """Tables over the blocks' sites one after the other (block b's site s becomes site offset[b] + s) -> (tables,
    offset[len(blocks) + 1]).  A row that observes one block's sites has that block's masks and marker entries."""
    from mixemt_amd import preprocess
    H = blocks[0].n_haps
    assert all(b.n_haps == H for b in blocks)
    offset = numpy.concatenate([[0], numpy.cumsum([len(b.sites) for b in blocks])]).astype(numpy.int64)
    assert offset[-1] <= 65536
    expected = numpy.concatenate([b.expected for b in blocks], axis=0)
    lhit = numpy.concatenate([b.lhit for b in blocks])
    lmiss = numpy.concatenate([b.lmiss for b in blocks])
    return preprocess.HapVarTables(numpy.arange(offset[-1], dtype=numpy.int64), expected, lhit, lmiss,
                                   list(blocks[0].haplogroups), H), offset


def all_reference_rows(site_lists):
    """CSR (row_ptr int64, site uint16, obs uint8) of rows that observe the reference base at the given site indexes."""
    lens = [len(s) for s in site_lists]
    row_ptr = numpy.concatenate([[0], numpy.cumsum(lens)]).astype(numpy.int64)
    site = numpy.concatenate([numpy.asarray(s, dtype=numpy.int64) for s in site_lists]).astype(numpy.uint16)
    return row_ptr, site, numpy.full(len(site), REF_BASE, dtype=numpy.uint8)


def row_facts(tables, row_sites, row_obs):
    """
    (n, K, E, n_values) of one CSR row, on the host:
      n         observed sites
      K         distinct non-zero columns of the flip matrix F[j][h] = (obs_j == expected(h, s_j)) != (obs_j == maj(s_j))
      E         sum of the marker-list lengths (tables.sparse()'s mk_ptr) of the row's sites
      n_values  distinct bit patterns of the row as the C oracle builds it
    """
    from oracle import c_oracle
    row_sites = numpy.asarray(row_sites, dtype=numpy.int64)
    row_obs = numpy.asarray(row_obs, dtype=numpy.uint8)
    sp = tables.sparse()
    H = tables.n_haps
    exp = tables.expected[row_sites, :H]
    flips = (exp == row_obs[:, None]) != (sp["maj"][row_sites] == row_obs)[:, None]
    cols = numpy.unique(numpy.packbits(flips, axis=0).T, axis=0)
    n_masks = int(cols.any(axis=1).sum())
    n_entries = int((sp["mk_ptr"][row_sites + 1] - sp["mk_ptr"][row_sites]).sum())
    row = c_oracle.build_em_matrix(tables.expected, tables.lhit, tables.lmiss, numpy.array([0, len(row_sites)]),
                                   row_sites.astype(numpy.uint16), row_obs, H)
    return len(row_sites), n_masks, n_entries, n_distinct(row[0])


# ---------------------------------------------------------------- the inputs of tests/test_gpu_class_edges.py
# A. the dense encoder: one matrix per width and layout, 33 rows -- every class limit from both sides, the odd inputs,
# and the limits again, so that encode_wide_rows_kernel's chunk boundary (32 rows) falls between two wide rows (31, 32)
ENCODER_WIDTHS = (1028, 2050, 5408)              # the smallest width with 257 quads; H % 4 == 2; Build 17
ENCODER_ODD_WIDTH = 5409                         # Build 17 + 1: encode_one_row's odd-width tail, D in {256, 257} only
ENCODER_D = (1, 2, 255, 256, 257, 258, 1023, 1024, 1025)
ENCODER_D_AGAIN = (256, 257, 255, 1023, 1024, 258, 2, 1, 1025, 256, 257, 1024, 1023, 255, 1025, 256, 257, 1024)
ENCODER_LIMIT_D = (255, 256, 257, 1023, 1024)
ENCODER_SPECIAL = ("collide256", "collide1024", "zeros", "nans", "neginf", "allones")
ENCODER_NAN_ROWS = ("nans", "allones")


@functools.lru_cache(maxsize=None)
def encoder_matrix(H, layout):
    """(matrix, labels): label = the row's D for a counted row, the name for a special one.  Never written to."""
    if H == ENCODER_ODD_WIDTH:
        d_list = (256, 257, 257, 256)
        mat, labels = rows_with_values(H, d_list, H, layout), list(d_list)
    else:
        special = special_rows(H, H + 1)
        mat = numpy.concatenate([rows_with_values(H, ENCODER_D, H, layout),
                                 numpy.stack([special[name] for name in ENCODER_SPECIAL]),
                                 rows_with_values(H, ENCODER_D_AGAIN, H + 2, layout)])
        labels = list(ENCODER_D) + list(ENCODER_SPECIAL) + list(ENCODER_D_AGAIN)
    mat.setflags(write=False)
    return mat, tuple(labels)


# B. the quad encoders: value rows of every (d, Q) class, interleaved with rows that have no quads
QUAD_WIDTHS = (1028, 5408)
QUAD_ROW_COUNTS = (1, 63, 64, 65, 130)           # the wave-per-row encoder fetches sizes 64 rows at a time


def quad_classes(H):
    """[(d, Q)]: Q = 1 needs one quadruple repeated (d = 4); d = 4 has only 4^4 = 256 quadruples, so it stops there."""
    out = [(4, 1), (4, 255), (4, 256)]
    for d in (64, 256):
        out += [(d, 255), (d, 256), (d, 257), (d, H // 4)]
    return out


@functools.lru_cache(maxsize=None)
def quad_pool(H):
    """{(d, Q): row} for quad_classes(H), plus "wide" (300 values) and "none" (1025 values: no record)."""
    pool = {}
    for d in (4, 64, 256):
        qs = [q for dd, q in quad_classes(H) if dd == d]
        rows = rows_with_quads(H, d, qs, 7 * H + d)
        for q, row in zip(qs, rows):
            pool[(d, q)] = row
    other = rows_with_values(H, (300, 1025), 7 * H + 1)
    pool["wide"], pool["none"] = other[0], other[1]
    for row in pool.values():
        row.setflags(write=False)
    return pool


def quad_matrix(H, n_rows):
    """(matrix, kinds): rows in the fixed pattern quad row, Q > 256 row, wide row, row without a record, ...; the quad
    rows and the Q > 256 rows each cycle through their classes.  kinds[i] = (d, Q), "wide" or "none"."""
    pool = quad_pool(H)
    small = [k for k in quad_classes(H) if k[1] <= 256]
    large = [k for k in quad_classes(H) if k[1] > 256]
    kinds = []
    for i in range(n_rows):
        kinds.append([small[(i // 4) % len(small)], large[(i // 4) % len(large)], "wide", "none"][i % 4])
    return numpy.stack([pool[k] for k in kinds]), kinds


# C. the marker build: (n, K) of every case; (n, K, E) where the marker entries are the point
MARKER_SHORT = [(n, K) for n in (10, 63, 64) for K in (254, 255, 256, 351, 352, 353)]
MARKER_LONG = [(n, K) for n in (65, 127, 128) for K in (255, 256, 703, 704, 705, 1023, 1024)] + [(129, 300)]
MARKER_ENTRIES_SHORT = [(64, 100, 1024), (64, 100, 1025)]
MARKER_ENTRIES_LONG = [(128, 100, 4096), (128, 100, 4097), (128, 100, 5120), (128, 100, 5121)]   # (H = 5408 only: see below)
MARKER_WIDTHS = (2050, 5408)
FILLER_SITES = 10
LONG_MAX_ENTRIES = 5120                          # mxm_set_sparse_long_entries' default


def marker_case_list(H, part):
    """The (n, K, E or None) cases of one matrix.  E cases put every pattern on one haplogroup and repeat single-site
    patterns on further ones, one marker entry each: 1 + K + (E - E0) haplogroups -- with single-site repeats the four
    long cases need up to 5122, which H = 2050 does not have (repeating larger patterns would fit, several entries per
    haplogroup; counting_tables keeps the one-entry step that hits E and E + 1 alike)."""
    if part == "short":
        return [(n, K, None) for n, K in MARKER_SHORT] + list(MARKER_ENTRIES_SHORT)
    assert part == "long", part
    return [(n, K, None) for n, K in MARKER_LONG] + (list(MARKER_ENTRIES_LONG) if H >= 5408 else [])


@functools.lru_cache(maxsize=None)
def marker_input(H, part, dyadic):
    """(tables, (row_ptr, site, obs), case_of_row): a filler row of 10 sites, then every case TWICE (two limit rows are
    neighbours), a filler row, the next case twice, ...; case_of_row[r] = index into marker_case_list or -1 (filler)."""
    cases = marker_case_list(H, part)
    blocks = [counting_tables(H, FILLER_SITES, 12, dyadic, None, 5)]
    for i, (n, K, E) in enumerate(cases):
        if E is None:
            # round-robin over all haplogroups where the row then stays within the long instance's 5120 marker entries
            # (H = 2050: ~3000); with 5408 haplogroups it would not (~8000: every long row would leave by its ENTRIES and
            # no mask limit would be met), so there every pattern sits on one haplogroup (~2 K entries)
            sizes = numpy.array([len(p) for p in _patterns(n, K + 1)])
            dealt = int(sizes[numpy.arange(H) % (K + 1)].sum())
            once = None if (n <= 64 or dealt <= LONG_MAX_ENTRIES) else 0
            blocks.append(counting_tables(H, n, K + 1, dyadic, once, 100 + i))
        else:
            base = sum(len(p) for p in _patterns(n, K + 1))
            blocks.append(counting_tables(H, n, K + 1, dyadic, E - base, 100 + i))
    tables, offset = join_tables(blocks)
    filler = numpy.arange(offset[0], offset[1])
    site_lists, case_of_row = [filler], [-1]
    for i in range(len(cases)):
        sites = numpy.arange(offset[i + 1], offset[i + 2])
        site_lists += [sites, sites, filler]
        case_of_row += [i, i, -1]
    return tables, all_reference_rows(site_lists), tuple(case_of_row)


def marker_class(n, K, E, long_rows=True, long_entries=LONG_MAX_ENTRIES):
    """Where the documented limits put a row: "short" (n <= 64, K <= 352), "long" (65 <= n <= 128, K <= 704,
    E <= 5120) or "fallback"."""
    if n <= 64:
        return "short" if K <= 352 else "fallback"
    if n <= 128 and long_rows:
        return "long" if (K <= 704 and E <= long_entries) else "fallback"
    return "fallback"


def mask_values(tables, row_sites, row_obs, oracle_row):
    """The row's value under each of its distinct flip masks (the zero mask included), sorted by bit pattern: what a
    record made by the marker kernel holds in its log table -- one entry per MASK, so equal sums repeat."""
    row_sites = numpy.asarray(row_sites, dtype=numpy.int64)
    row_obs = numpy.asarray(row_obs, dtype=numpy.uint8)
    exp = tables.expected[row_sites, :tables.n_haps]
    flips = (exp == row_obs[:, None]) != (tables.sparse()["maj"][row_sites] == row_obs)[:, None]
    _, first = numpy.unique(numpy.packbits(flips, axis=0).T, axis=0, return_index=True)
    return numpy.sort(bits(numpy.asarray(oracle_row)[first]))
