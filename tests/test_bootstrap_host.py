"""
The host side of assign.bootstrap_many -- bootstrap intervals for the refined proportions of a cohort -- and of its C
entries (include/mixemt_hip_bootstrap.h): the header against the binding table, the size function, every refusal (all made
before the first HIP call, so no device is needed; the pointers that are not NULL are never followed), bootstrap_many's
argument errors, and the two references the GPU tests compare against: a plain-Python Philox4x64-10 (tests/_bootstrap_ref.py)
against numpy's and the Random123 known answer, and the quantile formula against numpy.quantile.
"""
import ctypes
import io
import os
import re

import numpy
import pytest

from mixemt_amd import _lib

import _bootstrap_ref as ref
from test_samples_finish_host import PTR, _coded, _i32, _i64, _records, finish_args

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mixemt_hip_bootstrap.h")
SIZE, WEIGHTS, LOOP, SUMMARY = ("mxm_bootstrap_workspace_bytes", "mxm_bootstrap_weights", "mxm_em_loop_samples_narrow_boot",
                                "mxm_bootstrap_summary")
BATCHED = (WEIGHTS, LOOP)
ALL = (WEIGHTS, LOOP, SUMMARY)
WITH_LD = (LOOP, SUMMARY)


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
    assert set(names) == set(_lib.BOOTSTRAP_SIGNATURES) == {SIZE, WEIGHTS, LOOP, SUMMARY}
    for name, n_args in names.items():
        restype, argtypes = _lib.BOOTSTRAP_SIGNATURES[name]
        assert len(argtypes) == n_args, name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    # none of them is in another table
    for table in (_lib.SIGNATURES, _lib.FINISH_SIGNATURES, _lib.VARCHECK_SIGNATURES, _lib.ASSEMBLE_SAMPLES_SIGNATURES,
                  _lib.STATS_SAMPLES_SIGNATURES, _lib.SAMPLES_RUNS_SIGNATURES):
        assert not (set(names) & set(table))
    # the loop is the runs loop, parameter for parameter; the size function is the runs one's
    assert _lib.BOOTSTRAP_SIGNATURES[LOOP] == _lib.SAMPLES_RUNS_SIGNATURES["mxm_em_loop_samples_narrow_runs"]
    assert _lib.BOOTSTRAP_SIGNATURES[SIZE] == _lib.SAMPLES_RUNS_SIGNATURES["mxm_samples_runs_workspace_bytes"]
    with open(HEADER) as fin:
        text = fin.read()
    assert "MXM_VERSION 603: the version stays" in text
    assert re.search(r"^#define MXM_BOOTSTRAP_MAX 4096$", text, flags=re.M)
    assert re.search(r"^#define MXM_BOOTSTRAP_LDS_ROWS 8192$", text, flags=re.M)
    # the main header only includes it, the version stays, and the four pinned headers do not declare its entries
    from test_guarded_complete import declared_entries
    assert not (set(names) & declared_entries())
    with open(os.path.join(os.path.dirname(HEADER), "mixemt_hip.h")) as fin:
        assert '#include "mixemt_hip_bootstrap.h"' in fin.read()
    assert lib.mxm_version() == 603 and _lib.ABI_VERSION == 603
    from mixemt_amd import assign, build
    assert HEADER in build.HDRS
    assert assign.BOOTSTRAP_MAX == 4096


def test_the_size_function_is_monotone_and_refuses_what_the_entries_refuse(lib):
    size = lib.mxm_bootstrap_workspace_bytes
    assert size(10, 3, 2, 4) > 0 and size(10, 3, 2, 4) % 256 == 0
    for n_boot in (0, 1, 4097, -3):
        assert size(10, 3, n_boot, 4) == 0
    assert size(0, 3, 2, 4) == 0 and size(10, 0, 2, 4) == 0 and size(10, 3, 2, -1) == 0
    base = (10, 3, 2, 4)
    for arg, values in ((0, (1, 10, 11, 1000, 10 ** 6)), (1, (1, 3, 4, 500, 65535)), (2, (2, 3, 64, 65, 1000, 4096)), (3, (0, 4, 8, 16))):
        got = []
        for v in values:
            args = list(base)
            args[arg] = v
            got.append(size(*args))
        assert all(a <= b for a, b in zip(got, got[1:])) and got[0] > 0, (arg, got)
    # the one-run workspace, a prefix sum per row the plan can hold, and the counters of min(B, 64) replicates of them
    rows = 10 * 32
    assert size(10, 3, 5, 16) >= lib.mxm_samples_finish_workspace_bytes(10, 3, 16) + 4 * rows + 4 * 5 * rows
    assert size(10, 3, 4096, 16) == size(10, 3, 64, 16)


# ---- the C ABI ---------------------------------------------------------------------------------------------------
BIG_WS = 1 << 22


def _calls(lib, coded, row0, n_samples, n_boot=100, width=128, ld=4, ncol=(2, 3), ws=PTR, ws_bytes=BIG_WS, q=(0.025, 0.975), w=PTR):
    """entry point -> a call of it on one batch description (only the entries a row names are ever called: the others
    would go on to the device with pointers that are not real)."""
    c, r0 = ctypes.byref(coded), _i64(*row0)
    nc = _i32(*ncol)
    ids = (ctypes.c_uint32 * 8)(*range(8))
    states = (_lib.EmState * (4 * 4096))()
    return {
        WEIGHTS: lambda: lib.mxm_bootstrap_weights(c, r0, n_samples, n_boot, w, 7, ids, PTR, PTR, ws, ws_bytes, None),
        LOOP: lambda: lib.mxm_em_loop_samples_narrow_boot(c, r0, n_samples, width, n_boot, PTR, ld, nc, w, PTR, PTR, PTR, PTR, 1e-4,
                                                          10, 4, PTR, ws, ws_bytes, None, states),
        SUMMARY: lambda: lib.mxm_bootstrap_summary(n_samples, n_boot, ld, nc, PTR, PTR, q[0], q[1], PTR, PTR, PTR, PTR, PTR, PTR,
                                                   None),
    }


BOOT_MESSAGE = "%%s: B = %d replicates per sample: 2 .. 4096 are taken"
GOOD = dict(row0=(0, 4, 10), n_samples=2)
# (what, keyword arguments of _calls, the entries that refuse it, the message after "<entry>: ")
REFUSALS = [
    ("B = 0", dict(GOOD, n_boot=0), ALL, BOOT_MESSAGE % 0),
    ("B = 1", dict(GOOD, n_boot=1), ALL, BOOT_MESSAGE % 1),
    ("B = 4097", dict(GOOD, n_boot=4097), ALL, BOOT_MESSAGE % 4097),
    ("row0 not ascending", dict(row0=(0, 7, 4, 10), n_samples=3, ncol=(2, 3, 1)), BATCHED,
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has -3 rows)"),
    ("an empty sample", dict(row0=(0, 4, 4, 10), n_samples=3, ncol=(2, 3, 1)), BATCHED,
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has 0 rows)"),
    ("row0[S] != R", dict(row0=(0, 4, 9), n_samples=2), BATCHED, "%s: row0[S] = 9, the matrix has 10 rows"),
    ("a quad dictionary", dict(GOOD, coded=_coded(qrec=PTR)), BATCHED,
     "%s: a quad dictionary is attached; the batched pass reads the records only"),
    ("a dense rest", dict(GOOD, coded=_coded(R_rest=2)), BATCHED,
     "%s: 2 rows without a record (the dense rest): such a sample runs on its own"),
    ("no samples", dict(row0=(0, 4, 10), n_samples=0), ALL, "%s: bad arguments (S = 0; 1 .. 65535 samples)"),
    ("ld = 5", dict(GOOD, ld=5), WITH_LD, "%s: ld = 5: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ld = 32", dict(GOOD, ld=32), WITH_LD, "%s: ld = 32: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ncol above ld", dict(GOOD, ncol=(2, 5)), WITH_LD, "%s: sample 1 has ncol = 5 outside [0, 4]"),
    ("ncol below 0", dict(GOOD, ncol=(-1, 3)), WITH_LD, "%s: sample 0 has ncol = -1 outside [0, 4]"),
    ("a workspace that is not 16-byte aligned", dict(GOOD, ws=PTR + 8), BATCHED, "%s: workspace too small (or not 16-byte aligned)"),
    ("a short workspace", dict(GOOD, ws_bytes=255), BATCHED, "%s: workspace too small (or not 16-byte aligned)"),
    ("no workspace", dict(GOOD, ws=None), BATCHED, "%s: workspace too small (or not 16-byte aligned)"),
    ("no weights", dict(GOOD, w=None), (WEIGHTS,), "%s: bad arguments (w, s_id_host, wb and state are required)"),
    ("no replicate weights", dict(GOOD, w=None), (LOOP,), "%s: bad arguments"),
    ("a quantile above 1", dict(GOOD, q=(0.025, 1.5)), (SUMMARY,), "%s: the quantiles 0.025 and 1.5 must lie in [0, 1]"),
    ("a quantile that is NaN", dict(GOOD, q=(float("nan"), 0.5)), (SUMMARY,), "%s: the quantiles nan and 0.5 must lie in [0, 1]"),
]


@pytest.mark.parametrize("what,kw,entries,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_and_their_messages(lib, what, kw, entries, message):
    kw = dict(kw)
    coded = kw.pop("coded", _coded())
    calls = _calls(lib, coded, **kw)
    for name in entries:
        assert calls[name]() == -1, (what, name)
        want = message % name if "%s" in message else message
        assert lib.mxm_last_error().decode() == want, (what, name)


def test_a_workspace_one_byte_short_is_refused(lib):
    n_tiles = int(lib.mxm_samples_plan(_i64(0, 4, 10), 2, None, 0, None))
    for name, ld in ((WEIGHTS, 0), (LOOP, 4)):
        need = lib.mxm_bootstrap_workspace_bytes(n_tiles, 2, 100, ld)
        assert _calls(lib, _coded(), ws_bytes=need - 1, **GOOD)[name]() == -1
        assert lib.mxm_last_error().decode() == "%s: workspace too small (or not 16-byte aligned)" % name


def test_the_loop_refuses_a_large_sample_without_e(lib):
    """The header: "NULL accepted when every sample has at most 9216 cells, refused otherwise"."""
    coded = _coded(R=3100)
    c, r0, nc = ctypes.byref(coded), _i64(0, 20, 3100), _i32(2, 3)                # 3080 x 3 = 9240 cells
    states = (_lib.EmState * 6)()
    assert lib.mxm_em_loop_samples_narrow_boot(c, r0, 2, 128, 3, PTR, 4, nc, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 4, None, PTR, BIG_WS,
                                               None, states) == -1
    assert lib.mxm_last_error().decode() == "mxm_em_loop_samples_narrow_boot: a sample of more than 9216 cells needs the global copy E"


# ---- bootstrap_many's argument errors (all raised before a device is asked for) -------------------------------------------
def _cohort():
    import torch
    rec = torch.zeros(64, dtype=torch.uint8)
    haps = ["h%02d" % i for i in range(66)]
    samples = [(_records(rec, 5), numpy.ones(5)), (_records(rec, 7), numpy.ones(7))]
    done = {"contribs": [["hap1", "h03", 0.7], ["hap2", "h01", 0.3]], "sub_haps": ["h01", "h03"],
            "refined": {"props": numpy.array([0.3, 0.7])}}
    return samples, [done, dict(done)], haps


def test_bootstrap_many_refuses_bad_arguments_before_it_touches_the_device():
    from mixemt_amd import assign
    samples, finished, haps = _cohort()
    args = finish_args()
    for bad in (0, 1, 4097, -5):
        with pytest.raises(ValueError, match=r"n_boot = %d: 2 \.\. 4096 replicates are taken" % bad):
            assign.bootstrap_many(samples, finished, haps, args, n_boot=bad)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"level = .* must lie in \(0, 1\)"):
            assign.bootstrap_many(samples, finished, haps, args, level=bad)
    with pytest.raises(ValueError, match=r"one result of finish_many per sample is needed \(2 samples, 1 results\)"):
        assign.bootstrap_many(samples, finished[:1], haps, args)
    with pytest.raises(ValueError, match=r"one result of finish_many per sample"):
        assign.bootstrap_many([], [], haps, args)
    with pytest.raises(ValueError, match=r"sample_ids needs one id per sample \(2 samples, 3 ids\)"):
        assign.bootstrap_many(samples, finished, haps, args, sample_ids=[1, 2, 3])
    with pytest.raises(ValueError, match="32-bit unsigned"):
        assign.bootstrap_many(samples, finished, haps, args, sample_ids=[1, 2 ** 32])
    with pytest.raises(ValueError, match=r"above the budget of 1000 bytes \(max_bytes\): split the cohort or lower n_boot"):
        assign.bootstrap_many(samples, finished, haps, args, n_boot=100, max_bytes=1000)
    with pytest.raises(ValueError, match="weights do not match"):
        assign.bootstrap_many([(samples[0][0], numpy.ones(4)), samples[1]], finished, haps, args)
    # the matrices, under the function's own name: views of one record buffer, as wide as the haplogroup list
    import torch
    other = (_records(torch.zeros(64, dtype=torch.uint8), 7), numpy.ones(7))
    with pytest.raises(ValueError, match="bootstrap_many: the samples must be views of ONE record buffer"):
        assign.bootstrap_many([samples[0], other], finished, haps, args)
    with pytest.raises(ValueError, match="bootstrap_many: 65 haplogroups for matrices of 66 columns"):
        assign.bootstrap_many(samples, finished, haps[:65], args)


def test_samples_that_do_not_take_part_are_skipped_with_a_reason():
    """Decided on the host: a cohort in which nothing takes part never asks for a device."""
    from mixemt_amd import assign
    samples, finished, haps = _cohort()
    skip = assign._bootstrap_skip
    assert skip(samples[0], finished[0], 1000) is None
    assert "no refined result" in skip(samples[0], dict(finished[0], refined=None), 1000)
    assert "more than max_rows = 4" in skip(samples[0], finished[0], 4)
    many = [["hap%d" % i, "h%02d" % i, 1 / 17.0] for i in range(17)]
    assert "17 contributors" in skip(samples[0], dict(finished[0], contribs=many, sub_haps=[c[1] for c in many]), 1000)
    assert "0 contributors" in skip(samples[0], dict(finished[0], contribs=[], sub_haps=[]), 1000)
    for bad in (numpy.array([1, 2, 0.5, 1, 1]), numpy.array([1, 2, -1, 1, 1]), numpy.array([1, 2, numpy.nan, 1, 1])):
        assert "not non-negative integers" in skip((samples[0][0], bad), finished[0], 1000)
    assert "a total in [1, 2^31)" in skip((samples[0][0], numpy.zeros(5)), finished[0], 1000)
    assert "a total in [1, 2^31)" in skip((samples[0][0], numpy.full(5, 2.0 ** 30)), finished[0], 1000)
    unrefined = [dict(f, refined=None) for f in finished]
    boots, skipped = assign.bootstrap_many(samples, unrefined, haps, finish_args())
    assert boots == [None, None] and [s for s, _ in skipped] == [0, 1] and all("no refined result" in why for _, why in skipped)
    one, why = assign.bootstrap(samples[0][0], samples[0][1], unrefined[0], haps, finish_args())
    assert one is None and "no refined result" in why


def test_report_intervals_many_writes_one_line_per_contributor():
    from mixemt_amd import stats
    _, finished, _ = _cohort()
    boots = [{"intervals": [["hap1", "h03", 0.7, 0.65, 0.74961, 0.025], ["hap2", "h01", 0.3, 0.25039, 0.35, float("nan")]]}, None]
    out = io.StringIO()
    stats.report_intervals_many(out, finished, boots, titles=["a", "b"])
    assert out.getvalue() == ("# a\nhap1\th03\t0.7000\t0.6500\t0.7496\t0.0250\nhap2\th01\t0.3000\t0.2504\t0.3500\tnan\n"
                              "# b\nhap1\th03\t0.7000\tNA\tNA\tNA\nhap2\th01\t0.3000\tNA\tNA\tNA\n")
    with pytest.raises(ValueError, match="one bootstrap result"):
        stats.report_intervals_many(io.StringIO(), finished, boots[:1])


# ---- the references of the GPU tests ---------------------------------------------------------------------------------
def test_plain_python_philox_equals_the_known_answers_and_numpy():
    # Random123's kat_vectors: philox4x64-10, counter and key all zero; all ones
    assert ref.philox4x64([0, 0, 0, 0], [0, 0]) == [0x16554d9eca36314c, 0xdb20fe9d672d0fdc, 0xd7e772cee186176b, 0x7e68b68aec7ba23b]
    ones = (1 << 64) - 1
    assert ref.philox4x64([ones] * 4, [ones] * 2) == [0x87b092c3013fe90b, 0x438c3c67be8d0224, 0x9cc7d7c69cd777b6, 0xa09caebf594f0ba0]
    for seed, s_id, b, n in ((0, 0, 0, 9), (12345, 7, 3, 64), (2 ** 63 + 5, 2 ** 32 - 1, 4095, 13), (1, 2, 3, 0), (1, 2, 3, 1)):
        assert ref.stream(seed, s_id, b, n) == ref.numpy_stream(seed, s_id, b, n), (seed, s_id, b, n)


def test_the_draw_rule_counts_every_draw_and_never_draws_a_row_of_weight_zero():
    w = numpy.array([0, 3, 0, 0, 1, 2 ** 20, 0], dtype=numpy.float64)
    for b in range(3):
        counts = ref.resample(w, 11, 5, b)
        assert counts.sum() == w.sum() and not counts[w == 0].any()
    # the reference's vectorised upper half against Python's integers, at the ends of both ranges
    words = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, (1 << 64) - 1] + ref.stream(3, 1, 4, 57)
    for total in (1, 2, 5, 1198, (1 << 20) + 1, (1 << 31) - 1):
        assert ref.mulhi(words, total).tolist() == [(u * total) >> 64 for u in words], total
    # the rule itself, on words chosen by hand: N = 6 over (1, 0, 2, 3); t = (u * 6) >> 64
    words = [0, (1 << 64) // 6, (1 << 64) // 6 + 1, (1 << 63), (1 << 64) - 1, (1 << 64) // 2 - 1]          # t = 0, 0, 1, 3, 5, 2
    assert ref.resample([1, 0, 2, 3], 0, 0, 0, words=words).tolist() == [2.0, 0.0, 2.0, 2.0]


def test_the_quantile_formula_is_numpys_linear_method():
    rng = numpy.random.RandomState(5)
    for n in (2, 3, 64, 1000, 4096):
        x = numpy.sort(rng.random_sample(n))
        for q in (0.0, 0.025, 0.05, 0.5, 0.95, 0.975, 1.0):
            want = numpy.quantile(x, q, method="linear")
            got = ref.quantile(x, q)
            assert abs(got - want) <= 2 * numpy.spacing(want), (n, q)
    assert ref.quantile([0.25, 0.75], 0.5) == 0.5 and ref.quantile([0.25], 0.3) == 0.25
