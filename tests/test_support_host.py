"""
The host side of assign.support_many -- nested-model likelihood fits that say whether a contributor is supported -- and of
its C entries (include/mixemt_hip_support.h): the header against the binding table, the size function, every refusal (all
made before the first HIP call, so no device is needed; the pointers that are not NULL are never followed), the model lists
and masks, the statistics against hand-computed values, the skipping reasons, the report's text, and a self-check of the
reference the GPU tests compare against (tests/_support_ref.py), which is also the concavity claim checked on the CPU.
"""
import ctypes
import io
import math
import os
import re

import numpy
import pytest

from mixemt_amd import _lib

import _support_ref as ref
from test_samples_finish_host import PTR, _coded, _i32, _i64, _records, finish_args

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mixemt_hip_support.h")
SIZE, LOOP, LOGLIK = "mxm_support_workspace_bytes", "mxm_em_loop_samples_narrow_masks", "mxm_loglik_samples_masks"
BOTH = (LOOP, LOGLIK)


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import build
    build.build()
    return _lib.load()


def declared():
    """{entry: number of parameters} of the header: test_guarded_complete.declared_entries' parse, over this header."""
    with open(HEADER) as fin:
        text = fin.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    out = {}
    for decl in text.split(";"):
        found = re.search(r"\b(mxm_\w+)\s*\(([^)]*)\)", decl)
        if found and "typedef" not in decl.split(found.group(1))[0]:
            out[found.group(1)] = len(found.group(2).split(","))
    return out


def test_the_header_and_the_binding_table_name_the_same_entries(lib):
    names = declared()
    assert set(names) == set(_lib.SUPPORT_SIGNATURES) == {SIZE, LOOP, LOGLIK}
    for name, n_args in names.items():
        restype, argtypes = _lib.SUPPORT_SIGNATURES[name]
        assert len(argtypes) == n_args, name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    # none of them is in another table
    for table in (_lib.SIGNATURES, _lib.FINISH_SIGNATURES, _lib.VARCHECK_SIGNATURES, _lib.ASSEMBLE_SAMPLES_SIGNATURES,
                  _lib.STATS_SAMPLES_SIGNATURES, _lib.SAMPLES_RUNS_SIGNATURES, _lib.BOOTSTRAP_SIGNATURES):
        assert not (set(names) & set(table))
    # the loop is the runs loop with mask_host as one more argument, after ncol_host
    runs = _lib.SAMPLES_RUNS_SIGNATURES["mxm_em_loop_samples_narrow_runs"]
    mine = _lib.SUPPORT_SIGNATURES[LOOP]
    assert mine[0] == runs[0] and mine[1][:8] + mine[1][9:] == runs[1] and len(mine[1]) == len(runs[1]) + 1
    with open(HEADER) as fin:
        text = fin.read()
    assert "MXM_VERSION 603: the version stays" in text
    assert re.search(r"^#define MXM_SUPPORT_MAX_FITS 256$", text, flags=re.M)
    from test_guarded_complete import declared_entries
    assert not (set(names) & declared_entries())
    with open(os.path.join(os.path.dirname(HEADER), "mixemt_hip.h")) as fin:
        assert '#include "mixemt_hip_support.h"' in fin.read()
    assert lib.mxm_version() == 603 and _lib.ABI_VERSION == 603
    from mixemt_amd import assign, build
    assert HEADER in build.HDRS
    assert assign.SUPPORT_MAX_FITS == 256


def test_the_size_function_is_monotone_and_refuses_what_the_entries_refuse(lib):
    size = lib.mxm_support_workspace_bytes
    assert size(10, 3, 1, 4) > 0 and size(10, 3, 1, 4) % 256 == 0
    for n_fits in (0, 257, -3):
        assert size(10, 3, n_fits, 4) == 0
    assert size(0, 3, 2, 4) == 0 and size(10, 0, 2, 4) == 0 and size(10, 3, 2, -1) == 0
    base = (10, 3, 2, 4)
    for arg, values in ((0, (1, 10, 11, 1000, 10 ** 6)), (1, (1, 3, 4, 500, 65535)), (2, (1, 2, 64, 65, 256)), (3, (0, 4, 8, 16))):
        got = []
        for v in values:
            args = list(base)
            args[arg] = v
            got.append(size(*args))
        assert all(a <= b for a, b in zip(got, got[1:])) and got[0] > 0, (arg, got)
    # the one-run workspace and a 32-bit mask per (sample, fit)
    assert size(10, 3, 256, 16) >= lib.mxm_samples_finish_workspace_bytes(10, 3, 16) + 4 * 3 * 256


# ---- the C ABI ---------------------------------------------------------------------------------------------------
BIG_WS = 1 << 22


def _calls(lib, coded, row0, n_samples, n_fits=2, width=128, ld=4, ncol=(2, 3), masks=(1, 3, 7, 0, 0, 0), ws=PTR, ws_bytes=BIG_WS):
    """entry point -> a call of it on one batch description (every row below is refused before a pointer is followed)."""
    c, r0 = ctypes.byref(coded), _i64(*row0)
    nc = _i32(*ncol)
    mk = (ctypes.c_uint32 * max(len(masks), 1))(*masks) if masks is not None else None
    states = (_lib.EmState * (4 * 256))()
    return {
        LOOP: lambda: lib.mxm_em_loop_samples_narrow_masks(c, r0, n_samples, width, n_fits, PTR, ld, nc, mk, PTR, PTR, PTR, PTR, PTR,
                                                           1e-4, 10, 4, PTR, ws, ws_bytes, None, states),
        LOGLIK: lambda: lib.mxm_loglik_samples_masks(c, r0, n_samples, width, n_fits, PTR, ld, nc, mk, PTR, PTR, PTR, PTR, ws,
                                                     ws_bytes, None),
    }


FITS_MESSAGE = "%%s: B = %d fits per sample: 1 .. 256 are taken"
GOOD = dict(row0=(0, 4, 10), n_samples=2)
# (what, keyword arguments of _calls, the message after "<entry>: ")
REFUSALS = [
    ("B = 0", dict(GOOD, n_fits=0), FITS_MESSAGE % 0),
    ("B = 257", dict(GOOD, n_fits=257), FITS_MESSAGE % 257),
    ("B = -1", dict(GOOD, n_fits=-1), FITS_MESSAGE % -1),
    ("row0 not ascending", dict(row0=(0, 7, 4, 10), n_samples=3, ncol=(2, 3, 1)),
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has -3 rows)"),
    ("an empty sample", dict(row0=(0, 4, 4, 10), n_samples=3, ncol=(2, 3, 1)),
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has 0 rows)"),
    ("row0[S] != R", dict(row0=(0, 4, 9), n_samples=2), "%s: row0[S] = 9, the matrix has 10 rows"),
    ("a quad dictionary", dict(GOOD, coded=_coded(qrec=PTR)), "%s: a quad dictionary is attached; the batched pass reads the records only"),
    ("a dense rest", dict(GOOD, coded=_coded(R_rest=2)), "%s: 2 rows without a record (the dense rest): such a sample runs on its own"),
    ("no samples", dict(row0=(0, 4, 10), n_samples=0), "%s: bad arguments (S = 0; 1 .. 65535 samples)"),
    ("ld = 5", dict(GOOD, ld=5), "%s: ld = 5: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ld = 32", dict(GOOD, ld=32), "%s: ld = 32: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ncol above ld", dict(GOOD, ncol=(2, 5)), "%s: sample 1 has ncol = 5 outside [0, 4]"),
    ("ncol below 0", dict(GOOD, ncol=(-1, 3)), "%s: sample 0 has ncol = -1 outside [0, 4]"),
    ("a workspace that is not 16-byte aligned", dict(GOOD, ws=PTR + 8), "%s: workspace too small (or not 16-byte aligned)"),
    ("a short workspace", dict(GOOD, ws_bytes=255), "%s: workspace too small (or not 16-byte aligned)"),
    ("no workspace", dict(GOOD, ws=None), "%s: workspace too small (or not 16-byte aligned)"),
    ("no masks", dict(GOOD, masks=None), "%s: bad arguments (mask_host missing)"),
    ("a bit at ncol", dict(GOOD, masks=(1, 4, 7, 0)), "%s: sample 0, fit 1: mask 0x4 has a bit at or above ncol = 2"),
    ("a bit above ncol", dict(GOOD, masks=(1, 3, 7, 0x80000001)), "%s: sample 1, fit 1: mask 0x80000001 has a bit at or above ncol = 3"),
    ("a mask for a sample without columns", dict(GOOD, ncol=(0, 3), masks=(0, 1, 7, 0)),
     "%s: sample 0, fit 1: mask 0x1 has a bit at or above ncol = 0"),
]


@pytest.mark.parametrize("what,kw,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_messages(lib, what, kw, message):
    kw = dict(kw)
    coded = kw.pop("coded", _coded())
    calls = _calls(lib, coded, **kw)
    for name in BOTH:
        assert calls[name]() == -1, (what, name)
        want = message % name if "%s" in message else message
        assert lib.mxm_last_error().decode() == want, (what, name)


def test_a_workspace_one_byte_short_is_refused(lib):
    n_tiles = int(lib.mxm_samples_plan(_i64(0, 4, 10), 2, None, 0, None))
    need = lib.mxm_support_workspace_bytes(n_tiles, 2, 2, 4)
    assert need > lib.mxm_samples_finish_workspace_bytes(n_tiles, 2, 4)
    for name in BOTH:
        assert _calls(lib, _coded(), ws_bytes=need - 1, **GOOD)[name]() == -1
        assert lib.mxm_last_error().decode() == "%s: workspace too small (or not 16-byte aligned)" % name


def test_the_loop_refuses_a_large_sample_without_e(lib):
    """The header: "NULL accepted when every sample has at most 9216 cells, refused otherwise" -- judged on R_s x ncol[s],
    whatever the masks hold."""
    coded = _coded(R=3100)
    c, r0, nc = ctypes.byref(coded), _i64(0, 20, 3100), _i32(2, 3)                # 3080 x 3 = 9240 cells
    masks = (ctypes.c_uint32 * 4)(1, 3, 1, 0)                                     # (sample 1's one fit has ONE column)
    states = (_lib.EmState * 4)()
    assert lib.mxm_em_loop_samples_narrow_masks(c, r0, 2, 128, 2, PTR, 4, nc, masks, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 4, None, PTR,
                                                BIG_WS, None, states) == -1
    assert lib.mxm_last_error().decode() == "mxm_em_loop_samples_narrow_masks: a sample of more than 9216 cells needs the global copy E"


# ---- support_many's model lists and masks ------------------------------------------------------------------------
def _cohort():
    import torch
    rec = torch.zeros(64, dtype=torch.uint8)
    haps = ["h%02d" % i for i in range(66)]
    samples = [(_records(rec, 5), numpy.ones(5)), (_records(rec, 7), numpy.ones(7))]
    done = {"contribs": [["hap1", "h30", 0.6], ["hap2", "h02", 0.3], ["hap3", "h17", 0.1]], "sub_haps": ["h02", "h17", "h30"],
            "vote_order": ["h30", "h40", "h02", "h05", "h17", "h50"], "refined": {"props": numpy.array([0.3, 0.1, 0.6])}}
    return samples, [done, dict(done)], haps


def _plan(done, haps, models, n_extra=0, extra=None):
    from mixemt_amd import assign
    return assign._support_plan(done, {h: i for i, h in enumerate(haps)}, models, n_extra, extra)


def test_model_lists_and_masks():
    _, (done, _), haps = _cohort()
    # the columns ascend by haplogroup index: h02 = bit 0, h17 = bit 1, h30 = bit 2; the fits follow the CONTRIBUTOR order
    cols, names, masks, fits, extras, cut = _plan(done, haps, "drop-one")
    assert cols == [2, 17, 30] and names == ["h02", "h17", "h30"] and extras == [] and cut == []
    assert masks == [0b111, 0b011, 0b110, 0b101]
    assert fits == [("h02", "h17", "h30"), ("h02", "h17"), ("h17", "h30"), ("h02", "h30")]
    # extras: the first n_extra of the vote order that are not contributors (h40, h05), each added to the full set
    cols, names, masks, fits, extras, cut = _plan(done, haps, "add-one", n_extra=2)
    assert extras == ["h40", "h05"] and cols == [2, 5, 17, 30, 40] and names == ["h02", "h05", "h17", "h30", "h40"]
    assert masks == [0b01101, 0b00101, 0b01100, 0b01001, 0b11101, 0b01111]
    assert fits[4] == ("h02", "h17", "h30", "h40") and fits[5] == ("h02", "h05", "h17", "h30")
    # finish_many's vote_order holds haplogroup INDEXES: the same plan
    from mixemt_amd import assign
    by_index = dict(done, vote_order=[30, 40, 2, 5, 17, 50])
    assert assign._support_plan(by_index, {h: i for i, h in enumerate(haps)}, "add-one", 2, None, haps) == (cols, names, masks, fits, extras, cut)
    # drop-one gathers the extras too but fits none of them; extra= names them
    assert _plan(done, haps, "drop-one", n_extra=2)[2] == [0b01101, 0b00101, 0b01100, 0b01001]
    assert _plan(done, haps, "add-one", extra=["h50", "h30", "h50"])[4] == ["h50"]           # a contributor and a repeat: dropped
    # all: the full set first, then every other non-empty subset of the contributors, 2^K - 1 in all
    masks = _plan(done, haps, "all")[2]
    assert masks[0] == 0b111 and sorted(masks) == list(range(1, 8)) and len(masks) == 7
    # explicit: in the caller's order, over the contributors and any other haplogroup it names
    cols, names, masks, fits, extras, cut = _plan(done, haps, [("h30",), ("h17", "h02"), ("h30", "h61")])
    assert names == ["h02", "h17", "h30", "h61"] and masks == [0b0100, 0b0011, 0b1100] and extras == ["h61"]
    assert fits == [("h30",), ("h02", "h17"), ("h30", "h61")]
    # K = 1: the full fit only (nothing to leave out); add-one still adds
    one = dict(done, contribs=[["hap1", "h30", 1.0]], sub_haps=["h30"])
    assert _plan(one, haps, "drop-one")[2] == [1] and _plan(one, haps, "all")[2] == [1]
    assert _plan(one, haps, "add-one", n_extra=1)[2] == [0b01, 0b11]
    # a name that is not a haplogroup
    for bad in (dict(models="add-one", extra=["nope"]), dict(models=[("h30", "nope")])):
        with pytest.raises(ValueError, match="support_many: Unknown haplogroup 'nope'"):
            _plan(done, haps, **bad)
    with pytest.raises(ValueError, match="models must be 'drop-one', 'add-one', 'all' or a list"):
        _plan(done, haps, "drop-two")
    with pytest.raises(ValueError, match="at least one haplogroup, each named once"):
        _plan(done, haps, [("h30", "h30")])


def test_extras_are_truncated_at_16_columns_and_all_is_refused_above_8():
    _, (done, _), haps = _cohort()
    many = [["hap%d" % (i + 1), "h%02d" % (2 * i), 1 / 14.0] for i in range(14)]
    wide = dict(done, contribs=many, sub_haps=sorted(c[1] for c in many), vote_order=["h%02d" % i for i in range(66)])
    cols, names, masks, fits, extras, cut = _plan(wide, haps, "add-one", n_extra=4)
    assert extras == ["h01", "h03"] and cut == ["h05", "h07"] and len(cols) == 16
    assert len(masks) == 1 + 14 + 2 and all(m < (1 << 16) for m in masks) and masks[0] == sum(1 << names.index(c[1]) for c in many)
    with pytest.raises(ValueError, match=r"models='all' enumerates every subset: at most 8 contributors, not 14"):
        _plan(wide, haps, "all")
    nine = dict(done, contribs=many[:9], sub_haps=sorted(c[1] for c in many[:9]))
    with pytest.raises(ValueError, match="at most 8 contributors, not 9"):
        _plan(nine, haps, "all")
    assert len(_plan(dict(done, contribs=many[:8], sub_haps=sorted(c[1] for c in many[:8])), haps, "all")[2]) == 255
    with pytest.raises(ValueError, match=r"needs more than 16 candidate columns \(h63 left out\)"):
        _plan(wide, haps, [tuple(c[1] for c in many) + ("h61", "h62", "h63")])


def test_support_many_refuses_bad_arguments_before_it_touches_the_device():
    from mixemt_amd import assign
    samples, finished, haps = _cohort()
    args = finish_args()
    with pytest.raises(ValueError, match=r"one result of finish_many per sample is needed \(2 samples, 1 results\)"):
        assign.support_many(samples, finished[:1], haps, args)
    with pytest.raises(ValueError, match=r"one result of finish_many per sample"):
        assign.support_many([], [], haps, args)
    with pytest.raises(ValueError, match=r"models needs one list of name tuples per sample \(2 samples, 1 lists\)"):
        assign.support_many(samples, finished, haps, args, models=[[("h30",)]])
    with pytest.raises(ValueError, match=r"extra needs one list of names per sample \(2 samples, 3 lists\)"):
        assign.support_many(samples, finished, haps, args, extra=[[], [], []])
    with pytest.raises(ValueError, match=r"above the budget of 100 bytes \(max_bytes\): split the cohort or ask for fewer models"):
        assign.support_many(samples, finished, haps, args, max_bytes=100)
    with pytest.raises(ValueError, match="weights do not match"):
        assign.support_many([(samples[0][0], numpy.ones(4)), samples[1]], finished, haps, args)
    with pytest.raises(ValueError, match="Unknown haplogroup 'nope'"):
        assign.support_many(samples, finished, haps, args, models="add-one", extra=[["nope"], []])
    import torch
    other = (_records(torch.zeros(64, dtype=torch.uint8), 7), numpy.ones(7))
    with pytest.raises(ValueError, match="support_many: the samples must be views of ONE record buffer"):
        assign.support_many([samples[0], other], finished, haps, args)
    with pytest.raises(ValueError, match="support_many: 65 haplogroups for matrices of 66 columns"):
        assign.support_many(samples, finished, haps[:65], args)
    # the starts are deterministic: nothing above (or in the plan) advances numpy's global stream
    numpy.random.seed(3)
    want = numpy.random.random()
    numpy.random.seed(3)
    _plan(finished[0], haps, "add-one", n_extra=2)
    assert numpy.random.random() == want


def test_samples_that_do_not_take_part_are_skipped_with_a_reason():
    """Decided on the host: a cohort in which nothing takes part never asks for a device."""
    from mixemt_amd import assign
    samples, finished, haps = _cohort()
    skip = assign._support_skip
    assert skip(samples[0], finished[0], 1000) is None
    assert "no refined result" in skip(samples[0], dict(finished[0], refined=None), 1000)
    assert "more than max_rows = 4" in skip(samples[0], finished[0], 4)
    many = [["hap%d" % i, "h%02d" % i, 1 / 17.0] for i in range(17)]
    assert "17 contributors" in skip(samples[0], dict(finished[0], contribs=many, sub_haps=[c[1] for c in many]), 1000)
    assert "0 contributors" in skip(samples[0], dict(finished[0], contribs=[], sub_haps=[]), 1000)
    twice = [["hap1", "h30", 0.6], ["hap2", "h30", 0.4]]
    assert "named twice" in skip(samples[0], dict(finished[0], contribs=twice, sub_haps=["h30", "h30"]), 1000)
    # any non-negative finite weights take part: no integer condition here
    assert skip((samples[0][0], numpy.array([0.5, 2.25, 0.0, 1e-3, 7.0])), finished[0], 1000) is None
    for bad in (numpy.array([1, 2, -1, 1, 1.0]), numpy.array([1, 2, numpy.nan, 1, 1]), numpy.array([1, 2, numpy.inf, 1, 1])):
        assert "not non-negative finite numbers" in skip((samples[0][0], bad), finished[0], 1000)
    unrefined = [dict(f, refined=None) for f in finished]
    got, skipped = assign.support_many(samples, unrefined, haps, finish_args())
    assert got == [None, None] and [s for s, _ in skipped] == [0, 1] and all("no refined result" in why for _, why in skipped)
    one, why = assign.support(samples[0][0], samples[0][1], unrefined[0], haps, finish_args())
    assert one is None and "no refined result" in why


# ---- the statistics ----------------------------------------------------------------------------------------------
def test_the_statistics_against_hand_computed_values():
    from mixemt_amd import assign
    # P(chi2_1 > 3.841458820694124) = 0.05, so half of it; P(chi2_1 > 1) = erfc(1 / sqrt 2) = 0.31731050786291...
    assert abs(assign.support_lrt_p(3.841458820694124) - 0.025) < 1e-15
    assert abs(assign.support_lrt_p(1.0) - 0.15865525393145707) < 1e-15
    assert assign.support_lrt_p(0.0) == 0.5 and assign.support_lrt_p(-1e-7) == 0.5 and assign.support_lrt_p(-3.0) == 0.5
    assert assign.support_lrt_p(2 * 745.0) == 0.0                      # far out: underflows to 0, not an error
    for lrt in (-2.0, 0.0, 0.3, 1.0, 9.5, 40.0):
        assert assign.support_lrt_p(lrt) == ref.lrt_p(lrt)
    # ll = -1000 over 3 columns and 1198 reads: bic = 2000 + 2 log 1198 (log 1198 = 7.08841), aic = 2004
    assert ref.bic(-1000.0, 3, 1198.0) == 2000.0 + 2 * math.log(1198.0) and abs(ref.bic(-1000.0, 3, 1198.0) - 2014.17682) < 1e-5
    assert ref.aic(-1000.0, 3) == 2004.0 and ref.bic(-5.0, 1, 10.0) == 10.0 and ref.aic(-5.0, 1) == 10.0


def test_report_support_many_writes_contributors_extras_and_the_best_model():
    from mixemt_amd import stats
    _, finished, _ = _cohort()
    sup = {"drop": [["hap1", "h30", 0.6, 812.25, 1.5e-179], ["hap2", "h02", 0.3, 40.0, 1.27e-10], ["hap3", "h17", 0.1, -1e-7, 0.5]],
           "add": [["h40", 0.0123, 2.5, 0.0569]],
           "models": [{"names": ("h02", "h17", "h30"), "bic": 2014.17668}, {"names": ("h02", "h30"), "bic": 2010.5}], "best_bic": 1}
    out = io.StringIO()
    stats.report_support_many(out, finished, [sup, None], titles=["a", "b"])
    assert out.getvalue() == ("# a\nhap1\th30\t0.6000\t812.2500\t1.5e-179\nhap2\th02\t0.3000\t40.0000\t1.27e-10\n"
                              "hap3\th17\t0.1000\t-0.0000\t0.5\nadd\th40\t0.0123\t2.5000\t0.0569\nbest_bic\th02,h30\t2010.5000\n"
                              "# b\nhap1\th30\t0.6000\tNA\tNA\nhap2\th02\t0.3000\tNA\tNA\nhap3\th17\t0.1000\tNA\tNA\n")
    with pytest.raises(ValueError, match="one support result"):
        stats.report_support_many(io.StringIO(), finished, [sup])


# ---- the reference of the GPU tests: a self-check, and the concavity claim on the CPU -----------------------------
def _mixture(rng, n_rows, props, signal=4.0):
    """Log-likelihood rows of reads drawn from a mixture: column k is `signal` nats better on the reads of component k."""
    who = rng.choice(len(props), size=n_rows, p=props)
    mat = rng.normal(-30.0, 1.0, size=(n_rows, len(props)))
    mat[numpy.arange(n_rows), who] += signal
    return mat


def test_the_maximum_does_not_depend_on_the_start_and_a_nested_fit_is_never_better():
    rng = numpy.random.default_rng(17)
    mat = _mixture(rng, 400, [0.6, 0.3, 0.1])
    w = rng.integers(1, 4, size=400).astype(numpy.float64)
    lls = {}
    for mask in (0b111, 0b011, 0b101, 0b110):
        k = bin(mask).count("1")
        got = []
        for start in (numpy.full(k, 1.0 / k), rng.dirichlet([0.5] * k)):
            _, ln_new, iters, done = ref.subset_em(mat, w, mask, start, 1e-12, 100000)
            assert done == 1 and iters > 3
            full = numpy.full(3, -numpy.inf)
            full[ref.mask_columns(mask)] = ln_new
            got.append(ref.exact_loglik(mat, full, w, mask))
        # both starts reach the same maximum: the log-likelihood is concave in the proportions
        assert abs(got[0] - got[1]) <= 1e-9 * abs(got[0]), (mask, got)
        lls[mask] = got[0]
    for mask in (0b011, 0b101, 0b110):
        assert lls[mask] <= lls[0b111], (mask, lls)
        assert 2 * float(lls[0b111] - lls[mask]) > 10.0                     # and every true contributor is missed when left out


def test_exact_and_sequential_loglik_agree_and_handle_the_edge_rows():
    rng = numpy.random.default_rng(4)
    mat = _mixture(rng, 300, [0.5, 0.5, 0.0][:2] + [0.0])[:, :3]
    lnp = numpy.log(numpy.array([0.25, 0.7, 0.05]))
    w = rng.integers(0, 5, size=300).astype(numpy.float64)
    for mask in (0b111, 0b101, 0b010):
        exact, seq = ref.exact_loglik(mat, lnp, w, mask), ref.seq_loglik(mat, lnp, w, mask)
        assert ref.rel_ll(seq, exact) < 300 * 2.0 ** -53
        plain = float((w * numpy.log(numpy.exp(mat[:, ref.mask_columns(mask)] + lnp[ref.mask_columns(mask)]).sum(axis=1))).sum())
        assert abs(plain - float(exact)) < 1e-9 * abs(plain)
    # a row of weight 0 may hold anything; a weighted row without a finite masked-in cell gives -inf; the redo rule
    edge = mat.copy()
    edge[5] = -numpy.inf
    w5 = w.copy()
    w5[5] = 0
    assert numpy.isfinite(float(ref.exact_loglik(edge, lnp, w5, 0b111))) and numpy.isfinite(ref.seq_loglik(edge, lnp, w5, 0b111))
    w5[5] = 2
    assert ref.exact_loglik(edge, lnp, w5, 0b111) == -numpy.inf and ref.seq_loglik(edge, lnp, w5, 0b111) == -numpy.inf
    edge[5] = (-numpy.inf, -40.0, -numpy.inf)
    assert ref.seq_loglik(edge, lnp, w5, 0b101) == -numpy.inf and numpy.isfinite(ref.seq_loglik(edge, lnp, w5, 0b111))
    deep = numpy.log(numpy.array([1e-300, 1.0 - 1e-300, 1e-300]))
    far = mat.copy()
    far[7] = (-1300.0, 0.0, -1305.0)                                          # masked-in ln p + M near -2000: the linear sum is 0
    exact, seq = ref.exact_loglik(far, deep, w5 * 0 + 1, 0b101), ref.seq_loglik(far, deep, w5 * 0 + 1, 0b101)
    assert numpy.isfinite(seq) and ref.rel_ll(seq, exact) < 300 * 2.0 ** -53
