"""
The host side of finish_many(runs="batch") -- the batched second half of a cohort run for samples of several EM runs
(mixemt's -M) -- and of its C entries (include/mixemt_hip_samples_runs.h): the header against the binding table, the
routing decision with and without the keyword, the size function, and every refusal (all made before the first HIP
call, so no device is needed; the pointers that are not NULL are never followed).
"""
import ctypes
import os
import re

import numpy
import pytest

from mixemt_amd import _lib

from test_samples_finish_host import PTR, _coded, _i32, _i64, _records, finish_args

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mixemt_hip_samples_runs.h")
VOTES, LOOP, ASSIGN = "mxm_votes_samples_runs", "mxm_em_loop_samples_narrow_runs", "mxm_assign_reads_samples_runs"
ALL = (VOTES, LOOP, ASSIGN)
WITH_LD = (LOOP, ASSIGN)


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
    assert set(names) == set(_lib.SAMPLES_RUNS_SIGNATURES) == set(ALL) | {"mxm_samples_runs_workspace_bytes"}
    for name, n_args in names.items():
        restype, argtypes = _lib.SAMPLES_RUNS_SIGNATURES[name]
        assert len(argtypes) == n_args, name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype == restype, name
    # one more parameter than the one-run form each: B
    for name, one_run in ((VOTES, "mxm_votes_samples"), (LOOP, "mxm_em_loop_samples_narrow"), (ASSIGN, "mxm_assign_reads_samples"),
                          ("mxm_samples_runs_workspace_bytes", "mxm_samples_finish_workspace_bytes")):
        assert names[name] == len(_lib.FINISH_SIGNATURES[one_run][1]) + 1, name
    with open(HEADER) as fin:
        text = fin.read()
    assert re.search(r"^#define MXM_SAMPLES_RUNS_MAX 64$", text, flags=re.M)
    # the main header only includes it, the version stays, and the four pinned headers do not declare its entries
    from test_guarded_complete import declared_entries
    assert not (set(names) & declared_entries())
    with open(os.path.join(os.path.dirname(HEADER), "mixemt_hip.h")) as fin:
        assert '#include "mixemt_hip_samples_runs.h"' in fin.read()
    assert lib.mxm_version() == 603
    from mixemt_amd import build
    assert HEADER in build.HDRS


def test_the_size_function_is_monotone_and_refuses_what_the_entries_refuse(lib):
    size = lib.mxm_samples_runs_workspace_bytes
    assert size(10, 3, 2, 4) > 0 and size(10, 3, 2, 4) % 256 == 0
    for n_runs in (0, 1, 65, -3):
        assert size(10, 3, n_runs, 4) == 0
    assert size(0, 3, 2, 4) == 0 and size(10, 0, 2, 4) == 0 and size(10, 3, 2, -1) == 0
    base = (10, 3, 2, 4)
    for arg, values in ((0, (1, 10, 11, 1000, 10 ** 6)), (1, (1, 3, 4, 500, 65535)), (2, (2, 3, 10, 64)), (3, (0, 4, 8, 16))):
        got = []
        for v in values:
            args = list(base)
            args[arg] = v
            got.append(size(*args))
        assert all(a <= b for a, b in zip(got, got[1:])) and got[0] > 0, (arg, got)
    # never less than the one-run workspace: the layout is shared
    assert size(10, 3, 5, 16) >= lib.mxm_samples_finish_workspace_bytes(10, 3, 16)


# ---- the routing decision ----------------------------------------------------------------------------------------
def test_routing_decision_with_and_without_the_keyword():
    from mixemt_amd import assign
    route = assign._finish_route
    assert assign.FINISH_RUNS_MAX == 64
    for n_multi in (2, 3, 64):
        assert route(600, "batch", n_multi, 1000) == "single"                       # the default: today's behaviour
        assert route(600, "batch", n_multi, 1000, runs="single") == "single"
        assert route(600, "batch", n_multi, 1000, runs="batch") == "batch"
        assert route(600, "batch", n_multi, 1000, 16, 16, runs="batch") == "batch"
    assert route(600, "batch", 65, 1000, runs="batch") == "single"                  # above the cap
    assert route(600, "single", 3, 1000, runs="batch") == "single"                  # its first EM ran on its own
    assert route(1001, "batch", 3, 1000, runs="batch") == "single" and route(1000, "batch", 3, 1000, runs="batch") == "batch"
    assert route(600, "batch", 3, 1000, 17, 17, runs="batch") == "single"           # more than 16 contributors
    assert route(600, "batch", 3, 1000, 3, 2, runs="batch") == "single"             # a haplogroup named twice
    assert route(600, "batch", 1, 1000, runs="batch") == "batch" and route(600, "batch", 1, 1000) == "batch"
    with pytest.raises(ValueError, match="runs must be 'single' or 'batch'"):
        route(600, "batch", 3, 1000, runs="both")


def test_finish_many_refuses_another_keyword_before_it_touches_the_device():
    import torch
    from mixemt_amd import assign
    haps = ["h%02d" % i for i in range(66)]
    rec = torch.zeros(64, dtype=torch.uint8)
    samples = [(_records(rec, 5), numpy.ones(5)), (_records(rec, 7), numpy.ones(7))]
    res = [{"props": numpy.full(66, 1 / 66.0), "ln_theta_k": numpy.zeros((3, 66)), "route": "batch"}] * 2
    for bad in ("both", "", None, "Batch"):
        with pytest.raises(ValueError, match="runs must be 'single' or 'batch'"):
            assign.finish_many(samples, res, haps, finish_args(n_multi=3), runs=bad)


def test_inits_of_several_runs_are_drawn_sample_after_sample():
    """[B][K_s] per refined sample, sample s's B draws before sample s + 1's; nothing for a sample that is not refined."""
    from mixemt_amd import assign, em
    numpy.random.seed(19)
    got = assign._finish_inits([3, None, 1, 5], None, 1.0, 3)
    numpy.random.seed(19)
    want = [numpy.stack([em.init_props(k) for _ in range(3)]) if k else None for k in (3, None, 1, 5)]
    after = numpy.random.random()
    assert got[1] is None and all(numpy.array_equal(g, w) for g, w in zip(got, want) if w is not None)
    assert [g.shape for g in got if g is not None] == [(3, 3), (3, 1), (3, 5)]
    numpy.random.seed(19)
    assign._finish_inits([3, None, 1, 5], None, 1.0, 3)
    assert numpy.random.random() == after
    with pytest.raises(ValueError, match=r"refine_inits\[0\] must hold 3"):
        assign._finish_inits([3], [numpy.ones(3) / 3], 1.0, 3)                  # one run's worth where three are needed


# ---- the C ABI ---------------------------------------------------------------------------------------------------
BIG_WS = 1 << 20


def _calls(lib, coded, row0, n_samples, n_runs=3, width=128, ld=4, ncol=(2, 3), perm=(1, 0, 0, 0, 2, 0, 1, 0), ws=PTR, ws_bytes=BIG_WS):
    """entry point -> a call of it on one batch description (only the entries a row names are ever called: the others
    would go on to the device with pointers that are not real)."""
    c, r0 = ctypes.byref(coded), _i64(*row0)
    nc, pm = _i32(*ncol), _i32(*perm)
    states = (_lib.EmState * (4 * 64))()
    return {
        VOTES: lambda: lib.mxm_votes_samples_runs(c, r0, n_samples, width, n_runs, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR,
                                                  ws, ws_bytes, None),
        LOOP: lambda: lib.mxm_em_loop_samples_narrow_runs(c, r0, n_samples, width, n_runs, PTR, ld, nc, PTR, PTR, PTR, PTR, PTR, 1e-4,
                                                          10, 4, PTR, ws, ws_bytes, None, states),
        ASSIGN: lambda: lib.mxm_assign_reads_samples_runs(c, r0, n_samples, width, n_runs, PTR, ld, nc, pm, PTR, PTR, PTR, None, 0.69,
                                                          PTR, None, ws, ws_bytes, None),
    }


RUNS_MESSAGE = "%%s: B = %d runs per sample: 2 .. 64 are taken (one run: the entries of mixemt_hip_samples_finish.h)"
GOOD = dict(row0=(0, 4, 10), n_samples=2)
# (what, keyword arguments of _calls, the entries that refuse it, the message after "<entry>: ")
REFUSALS = [
    ("B = 0", dict(GOOD, n_runs=0), ALL, RUNS_MESSAGE % 0),
    ("B = 1", dict(GOOD, n_runs=1), ALL, RUNS_MESSAGE % 1),
    ("B = 65", dict(GOOD, n_runs=65), ALL, RUNS_MESSAGE % 65),
    ("row0 not ascending", dict(row0=(0, 7, 4, 10), n_samples=3, ncol=(2, 3, 1), perm=(0,) * 12), ALL,
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has -3 rows)"),
    ("an empty sample", dict(row0=(0, 4, 4, 10), n_samples=3, ncol=(2, 3, 1), perm=(0,) * 12), ALL,
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has 0 rows)"),
    ("row0[S] != R", dict(row0=(0, 4, 9), n_samples=2), ALL, "%s: row0[S] = 9, the matrix has 10 rows"),
    ("a quad dictionary", dict(GOOD, coded=_coded(qrec=PTR)), ALL,
     "%s: a quad dictionary is attached; the batched pass reads the records only"),
    ("a dense rest", dict(GOOD, coded=_coded(R_rest=2)), ALL,
     "%s: 2 rows without a record (the dense rest): such a sample runs on its own"),
    ("ld = 5", dict(GOOD, ld=5), WITH_LD, "%s: ld = 5: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ld = 32", dict(GOOD, ld=32), WITH_LD, "%s: ld = 32: the reduced matrix's row stride must be 4, 8 or 16"),
    ("ncol above ld", dict(GOOD, ncol=(2, 5)), WITH_LD, "%s: sample 1 has ncol = 5 outside [0, 4]"),
    ("ncol below 0", dict(GOOD, ncol=(-1, 3)), WITH_LD, "%s: sample 0 has ncol = -1 outside [0, 4]"),
    ("an ordinal at ncol", dict(GOOD, perm=(1, 2, 0, 0, 2, 0, 1, 0)), (ASSIGN,),
     "%s: sample 0, column 1: contributor ordinal 2 outside [0, 2)"),
    ("an ordinal below 0", dict(GOOD, perm=(1, 0, 0, 0, 2, -1, 1, 0)), (ASSIGN,),
     "%s: sample 1, column 1: contributor ordinal -1 outside [0, 3)"),
    ("a workspace that is not 16-byte aligned", dict(GOOD, ws=PTR + 8), ALL, "%s: workspace too small (or not 16-byte aligned)"),
    ("a short workspace", dict(GOOD, ws_bytes=255), ALL, "%s: workspace too small (or not 16-byte aligned)"),
    ("no workspace", dict(GOOD, ws=None), ALL, "%s: workspace too small (or not 16-byte aligned)"),
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
    for name, ld in ((VOTES, 0), (LOOP, 4), (ASSIGN, 4)):
        need = lib.mxm_samples_runs_workspace_bytes(n_tiles, 2, 3, ld)
        assert _calls(lib, _coded(), ws_bytes=need - 1, **GOOD)[name]() == -1
        assert lib.mxm_last_error().decode() == "%s: workspace too small (or not 16-byte aligned)" % name


def test_the_loop_refuses_a_large_sample_without_e(lib):
    """The header: "NULL is accepted when every sample has at most 9216 cells, and refused otherwise"."""
    coded = _coded(R=3100)
    c, r0, nc = ctypes.byref(coded), _i64(0, 20, 3100), _i32(2, 3)                # 3080 x 3 = 9240 cells
    states = (_lib.EmState * 6)()
    assert lib.mxm_em_loop_samples_narrow_runs(c, r0, 2, 128, 3, PTR, 4, nc, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 4, None, PTR, BIG_WS,
                                               None, states) == -1
    assert lib.mxm_last_error().decode() == "mxm_em_loop_samples_narrow_runs: a sample of more than 9216 cells needs the global copy E"
