"""
The host side of the cohort's variant check on the device: the tree's tables (assign.VarCheckTables) against hap_var /
get_ancestral and the reference's own ancestral lists (g16), alignments.concat_columns against the numpy pileup, the C
entry's binding and what it says when it refuses a call (every row is refused before the first HIP call, so no device is
needed; pointers that are not NULL are never followed), and finish_many's argument checks for a CohortPileup.
The kernel itself: tests/test_gpu_var_check.py.
"""
import ctypes
import json
import os
import re
import sys

import numpy
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pileup_ref  # noqa: E402
from test_gpu_observe import _subset  # noqa: E402
from test_observe import g16_columns  # noqa: E402
from test_samples_finish_host import _records, finish_args  # noqa: E402

from mixemt_amd import _lib  # noqa: E402

PTR = 0x1000                 # "some pointer": never dereferenced by a row below
NAME = "mxm_check_variants_samples"


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import build
    build.build()
    return _lib.load()


def toy_tree(ref="AAAAAAAAA"):
    """A tree of its own (the session's `toy` is shared and has no reference sequence)."""
    from mixemt_amd import phylotree
    phy = phylotree.example()
    phy.refseq = ref
    return phy


def empty_columns():
    from mixemt_amd.alignments import AlignmentColumns
    return AlignmentColumns([], [], [], [0], [], [0], numpy.zeros(0, numpy.uint8), None, None, [])


def three_samples(g):
    cols = g16_columns(g)
    return [cols, _subset(cols, numpy.flatnonzero(cols.frag % 2 == 0)), empty_columns()]


# ---- the tables ----------------------------------------------------------------------------------------------------
def _decode(keys):
    return set((int(k) >> 2, "ACGT"[int(k) & 3]) for k in keys)


def test_tables_hold_hap_var_and_the_ancestral_bases(b17):
    from mixemt_amd import assign
    from mixemt_amd.phylotree import der_allele, pos_from_var
    _, phy, haps, _ = b17
    g = golden("g16_observe")
    tab = assign.VarCheckTables.build(phy, haps)
    assert tab.n_haps == len(haps) and tab.phylo is phy and tab.key_ptr is None            # (no device asked for)
    assert tab.key_ptr_h.dtype == tab.key_h.dtype == tab.site_h.dtype == tab.site_key_h.dtype == numpy.int32
    assert len(tab.key_h) == tab.key_ptr_h[-1] == 279179 and int(numpy.diff(tab.key_ptr_h).max()) == 68
    assert list(tab.site_h) == phy.get_variant_pos() and tab.max_pos == max(phy.get_variant_pos())
    ancestral = json.loads(str(g["ancestral"]))
    picked = [int(c) for c in g["candidates"]] + [0, 1, 77, 2500, len(haps) - 1] + [haps.index(h) for h in ancestral]
    for h in picked:
        own = tab.key_h[tab.key_ptr_h[h]:tab.key_ptr_h[h + 1]]
        assert list(own) == sorted(set(own.tolist())), haps[h]                                # distinct, ascending
        assert _decode(own) == set((pos_from_var(v), der_allele(v)) for v in phy.hap_var[haps[h]]), haps[h]
        touched = set(int(k) >> 2 for k in own)
        rest = [int(k) for p, k in zip(tab.site_h, tab.site_key_h) if int(p) not in touched]
        assert all(k >= 0 for k in rest)
        assert sorted(_decode(rest)) == sorted(phy.get_ancestral(haps[h])), haps[h]
        if haps[h] in ancestral:
            assert sorted(_decode(rest)) == [tuple(p) for p in ancestral[haps[h]]], haps[h]


def test_tables_of_an_edited_tree():
    from mixemt_amd import assign
    haps = list("ABCDEFGHI")
    phy = toy_tree()
    tab = assign.VarCheckTables.build(phy, haps)
    assert list(tab.site_h) == list(range(9)) and list(tab.site_key_h) == [4 * p for p in range(9)] and tab.max_pos == 8
    assert _decode(tab.key_h[tab.key_ptr_h[2]:tab.key_ptr_h[3]]) == {(0, "G"), (2, "T"), (4, "A"), (5, "T")}      # C: T5A
    # a custom haplogroup is in the tables of a build made after it was added
    phy.add_custom_hap("Z", ["A2C", "A9G", "A2C"])
    tab = assign.VarCheckTables.build(phy, haps + ["Z"])
    assert tab.n_haps == 10 and _decode(tab.key_h[tab.key_ptr_h[9]:]) == {(1, "C"), (8, "G")}
    # an ignored site leaves both tables
    phy.ignore_sites("9")                                       # (D = G + A9T merges into 'G/D')
    tab = assign.VarCheckTables.build(phy, sorted(phy.hap_var))
    assert tab.n_haps == 8 and 8 not in tab.site_h and tab.max_pos == 7 and all(int(k) >> 2 != 8 for k in tab.key_h)
    # a reference base outside ACGT: no key for the site
    tab = assign.VarCheckTables.build(toy_tree("AANAAAAAA"), haps)
    assert list(tab.site_key_h) == [0, 4, -1, 12, 16, 20, 24, 28, 32]
    # a derived allele outside ACGT: no tables (the caller takes the host route)
    phy = toy_tree()
    phy.add_custom_hap("Z", ["A3N"])
    assert assign.VarCheckTables.build(phy, haps + ["Z"]) is None
    assert assign.VarCheckTables.build(phy, haps) is not None


# ---- concat_columns ------------------------------------------------------------------------------------------------
def test_concat_columns_keeps_every_samples_pileup():
    from mixemt_amd import alignments, observe
    g = golden("g16_observe")
    parts = three_samples(g)
    joined, aln0 = alignments.concat_columns(parts)
    assert aln0.dtype == numpy.int64 and list(aln0) == [0, len(parts[0]), len(parts[0]) + len(parts[1]), len(joined)]
    assert len(parts[1]) > 0 and aln0[2] == aln0[3]
    assert list(joined.names) == list(parts[0].names) + list(parts[1].names)
    L = max(observe.pileup_length(c, 30, 16569) for c in parts)
    for s, cols in enumerate(parts):
        idx = numpy.arange(aln0[s], aln0[s + 1])
        own = _subset(joined, idx)
        assert numpy.array_equal(_pileup_ref.pileup(own, L), _pileup_ref.pileup(cols, L)), s
        assert [joined.names[f] for f in joined.frag[idx]] == [cols.names[f] for f in cols.frag], s
    frags = [set(joined.frag[aln0[s]:aln0[s + 1]].tolist()) for s in range(3)]
    assert frags[0] and frags[1] and not (frags[0] & frags[1])
    assert numpy.array_equal(joined.is_reverse, numpy.concatenate([parts[0].is_reverse, parts[1].is_reverse]))
    assert numpy.array_equal(joined.has_qual, numpy.concatenate([parts[0].has_qual, parts[1].has_qual]))
    with pytest.raises(ValueError, match="no samples"):
        alignments.concat_columns([])


def test_concat_columns_fills_an_absent_strand_or_quality_column_with_zeros():
    from mixemt_amd import alignments
    from mixemt_amd.alignments import AlignmentColumns
    raw = numpy.frombuffer(b"ACGT", dtype=numpy.uint8)
    plain = AlignmentColumns([5], [60], [0], [0, 1], [4 << 4], [0, 4], raw, None, None, ["p"])
    full = AlignmentColumns([7, 9], [60, 60], [0, 0], [0, 1, 2], [4 << 4, 4 << 4], [0, 4, 8], numpy.tile(raw, 2),
                            numpy.full(8, 35, numpy.uint8), [1, 1], ["q"], [1, 0])
    joined, aln0 = alignments.concat_columns([plain, empty_columns(), full])
    assert list(aln0) == [0, 1, 1, 3] and list(joined.is_reverse) == [0, 1, 0] and list(joined.has_qual) == [0, 1, 1]
    assert list(joined.qual) == [0] * 4 + [35] * 8 and list(joined.frag) == [0, 1, 1] and list(joined.names) == ["p", "q"]
    assert list(joined.cig_ptr) == [0, 1, 2, 3] and list(joined.seq_ptr) == [0, 4, 8, 12]
    alone, _ = alignments.concat_columns([plain])
    assert alone.is_reverse is None and alone.qual is None and alone.has_qual is None


# ---- the C ABI -----------------------------------------------------------------------------------------------------
def test_the_headers_names_are_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "mixemt_hip_var_check.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(mxm_\w+)\s*\(", text)))
    assert declared == sorted(_lib.VARCHECK_SIGNATURES) == [NAME]
    for name in declared:
        assert len(getattr(lib, name).argtypes) == len(_lib.VARCHECK_SIGNATURES[name][1]) == 22
        assert name not in _lib.SIGNATURES and name not in _lib.FINISH_SIGNATURES
    assert '#include "mixemt_hip_var_check.h"' in open(os.path.join(ROOT, "include", "mixemt_hip.h")).read()
    assert int(re.search(r"#define\s+MXM_VAR_CHECK_MAX_L\s+(\d+)", text).group(1)) == 131072
    from mixemt_amd import assign, build
    assert assign.VAR_CHECK_MAX_L == 131072 and any(h.endswith("mixemt_hip_var_check.h") for h in build.HDRS)
    assert lib.mxm_version() == 603


def _i32(*vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _call(lib, counts=PTR, S=2, L=100, key_ptr=PTR, key=PTR, H=50, site=PTR, site_key=PTR, n_sites=7, max_pos=99,
          cand=(1, 2, 0, 0, 49, 0, 0, 0), ncand=(2, 1), ld=4, keep=PTR):
    return lib.mxm_check_variants_samples(counts, S, L, key_ptr, key, H, site, site_key, n_sites, max_pos,
                                          None if cand is None else _i32(*cand), None if ncand is None else _i32(*ncand), ld,
                                          3.0, 0.02, 0.5, 0, 0, keep, None, None, None)


REFUSALS = [
    ("S below 0", dict(S=-1), "S < 0 (-1)"),
    ("ld = 5", dict(ld=5), "ld = 5: the candidate tables' row stride must be 4, 8, 16, 32 or 64"),
    ("ld = 128", dict(ld=128), "ld = 128: the candidate tables' row stride must be 4, 8, 16, 32 or 64"),
    ("ld = 0", dict(ld=0), "ld = 0: the candidate tables' row stride must be 4, 8, 16, 32 or 64"),
    ("no candidate table", dict(cand=None), "bad arguments (cand_host and ncand_host are required)"),
    ("no candidate counts", dict(ncand=None), "bad arguments (cand_host and ncand_host are required)"),
    ("ncand above ld", dict(ncand=(2, 5)), "sample 1 has ncand = 5 outside [0, 4]"),
    ("ncand below 0", dict(ncand=(-1, 1)), "sample 0 has ncand = -1 outside [0, 4]"),
    ("a candidate at H", dict(cand=(1, 50, 0, 0, 49, 0, 0, 0)), "sample 0, candidate 1: haplogroup index 50 outside [0, 50)"),
    ("a candidate below 0", dict(cand=(1, 2, 0, 0, -3, 0, 0, 0)), "sample 1, candidate 0: haplogroup index -3 outside [0, 50)"),
    ("no counts", dict(counts=None),
     "bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)"),
    ("no keys", dict(key=None), "bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)"),
    ("no key offsets", dict(key_ptr=None),
     "bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)"),
    ("no keep", dict(keep=None), "bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)"),
    ("sites without their keys", dict(site_key=None),
     "bad arguments (counts, key_ptr, key and keep are required, site and site_key with n_sites > 0)"),
    ("counts off the 16-byte grid", dict(counts=PTR + 4), "counts must be 16-byte aligned"),
    ("L = 0", dict(L=0, max_pos=-1), "bad shape (L = 0, n_sites = 7)"),
    ("n_sites below 0", dict(n_sites=-2), "bad shape (L = 100, n_sites = -2)"),
    ("max_pos at L", dict(max_pos=100), "max_pos = 100: the tree's variants reach past the pileup (L = 100)"),
    ("L above the cap", dict(L=131073, max_pos=16000), "L = 131073: a sample's bitsets do not fit the kernel's LDS (L <= 131072)"),
]


@pytest.mark.parametrize("what,kw,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_messages(lib, what, kw, message):
    assert _call(lib, **kw) == -1, what
    assert lib.mxm_last_error() == ("%s: %s" % (NAME, message)).encode(), what


def test_nothing_to_do_is_not_an_error(lib):
    """No sample, or no candidate in any: 0 before the device is looked at (the pointers are not real)."""
    assert _call(lib, S=0, cand=None, ncand=None) == 0
    assert _call(lib, ncand=(0, 0)) == 0
    assert _call(lib, S=1, ncand=(0,), cand=(7, 7, 7, 7), site=None, site_key=None, n_sites=0) == 0


# ---- finish_many's checks for a CohortPileup --------------------------------------------------------------------------
def test_finish_many_refuses_a_cohort_pileup_that_does_not_fit():
    import torch
    from mixemt_amd import assign, observe
    haps = ["h%02d" % i for i in range(66)]
    rec = torch.zeros(64, dtype=torch.uint8)
    samples = [(_records(rec, 5), numpy.ones(5)), (_records(rec, 7), numpy.ones(7))]
    res = [{"props": numpy.full(66, 1 / 66.0), "ln_theta_k": numpy.zeros((1, 66)), "route": "batch"}] * 2
    two = observe.CohortPileup(torch.zeros((2, 4, 16), dtype=torch.int32), [4, 4])
    one = observe.CohortPileup(torch.zeros((1, 4, 16), dtype=torch.int32), [4])
    assert (two.n_samples, two.L, two.min_map_qual, two.min_base_qual, len(one)) == (2, 4, 30, 30, 1)
    args = finish_args(var_check=True)
    with pytest.raises(ValueError, match=r"obs needs one entry per sample \(2 samples, 1 entries\)"):
        assign.finish_many(samples, res, haps, args, phylo=toy_tree(), obs=one)
    with pytest.raises(ValueError, match="needs phylo="):
        assign.finish_many(samples, res, haps, args, obs=two)
    tab = assign.VarCheckTables.build(toy_tree(), list("ABCDEFGHI"))
    with pytest.raises(ValueError, match="var_tables was built for 9 haplogroups, the samples have 66"):
        assign.finish_many(samples, res, haps, args, phylo=toy_tree(), obs=two, var_tables=tab)
    # host(s): a lazily downloaded, cached ObservedBases over the sample's own rows
    table = torch.zeros((2, 4, 16), dtype=torch.int32)
    table[1, 2, 0], table[1, 2, 7] = 5, 2
    pile = observe.CohortPileup(table, [4, 3])
    assert pile.host(1) is pile.host(1) and pile.host(1).obs_at(2, "A") == 7 and pile.host(0).total_obs(2) == 0
    assert pile.host(1).counts.shape == (3, 16) and pile.host(1).obs_at(3, "A") == 0
    with pytest.raises(IndexError):
        pile.host(2)


def test_observe_bases_many_names_its_budget():
    from mixemt_amd import observe
    with pytest.raises(ValueError, match=r"2 samples x 50 positions need 6400 bytes .* budget of 6399 bytes \(max_bytes\)"):
        observe.observe_bases_many([empty_columns(), empty_columns()], ref_len=50, max_bytes=6399)
    with pytest.raises(ValueError, match="no samples"):
        observe.observe_bases_many([])
    assert observe.COHORT_PILEUP_BYTES == 1 << 30
