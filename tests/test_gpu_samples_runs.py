"""
finish_many(runs="batch"): the batched second half of a cohort run for samples of SEVERAL EM runs (mixemt's -M;
mxm_votes_samples_runs, mxm_em_loop_samples_narrow_runs, mxm_assign_reads_samples_runs).  Every sample must come out as
the per-sample functions leave it -- the reference's goldens g13 / g19 / g14 per sample, the existing per-sample route
and the one-run entries on small shapes -- and with the same BITS whatever else shares the batch.
"""
import ctypes

import numpy
import pytest

from conftest import em_args, golden
from test_gpu_samples_finish import BAND, PROPS_ATOL, _few_values, _per_sample, _records_of, _same_as_per_sample, _vote_text, finish_args

pytestmark = pytest.mark.gpu


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.int64)


# ---- the low level: both loop entries through ctypes, every array kept -------------------------------------------------------
def _low(samples, wts=None):
    import torch
    from mixemt_amd import assign
    wts = [w for _, w in samples] if wts is None else wts
    return assign._finish_batch(samples, [torch.from_numpy(numpy.asarray(w, dtype=numpy.float64)).cuda() for w in wts],
                                list(range(len(samples))))


def _loop(low, mat, ld, ncol, inits, n_runs, tol, max_iter, check_every, with_e=True, resume=None):
    """mxm_em_loop_samples_narrow_runs (n_runs >= 2) or mxm_em_loop_samples_narrow (n_runs None: inits[s] is ONE vector).
    -> {ln_cur, ln_new, props_cur: numpy [S][B][ld] ([S][ld]), states: [(done, iters, l1 bits)] per entry, E, dev}."""
    import torch
    from mixemt_amd import _lib, em
    from mixemt_amd._dev import current_stream
    n, runs = low.n_entries, (n_runs or 1)
    ncol = numpy.ascontiguousarray(ncol, dtype=numpy.int32)
    if resume is None:
        p0 = numpy.zeros((n, runs, ld))
        for s in range(n):
            p0[s, :, :ncol[s]] = numpy.asarray(inits[s], dtype=numpy.float64).reshape(runs, ncol[s])
        ln0, p0 = em.log_inits(p0.reshape(n * runs, ld))
        dev = {"props_cur": torch.from_numpy(p0).cuda(), "ln_cur": torch.from_numpy(ln0).cuda(), "ln_new": torch.from_numpy(ln0).cuda(),
               "state": em.new_state(n * runs, low.dev),
               "E": torch.full((low.n_rows, ld), -7.0, dtype=torch.float64, device=low.dev) if with_e else None}
    else:
        dev = resume
    host = (_lib.EmState * (n * runs))()
    e_ptr = dev["E"].data_ptr() if dev["E"] is not None else None
    head = (ctypes.byref(low.coded), low.row0_ptr, n, low.n_haps)
    tail = (mat.data_ptr(), ld, ncol.ctypes.data, low.wts.data_ptr(), dev["props_cur"].data_ptr(), dev["ln_cur"].data_ptr(),
            dev["ln_new"].data_ptr(), dev["state"].data_ptr(), float(tol), int(max_iter), int(check_every), e_ptr, low.ws.data_ptr(),
            low.ws_bytes, current_stream(), host)
    if n_runs:
        rc = low.lib.mxm_em_loop_samples_narrow_runs(*(head + (n_runs,) + tail))
    else:
        rc = low.lib.mxm_em_loop_samples_narrow(*(head + tail))
    assert rc == 0, low.lib.mxm_last_error()
    shape = (n, runs, ld) if n_runs else (n, ld)
    out = {k: dev[k].cpu().numpy().reshape(shape) for k in ("props_cur", "ln_cur", "ln_new")}
    out["states"] = [(st.done, st.iters, int(numpy.float64(st.l1).view(numpy.int64))) for st in host]
    raw = dev["state"].cpu().numpy().tobytes()
    assert [(st.done, st.iters) for st in (_lib.EmState * (n * runs)).from_buffer_copy(raw)] == [st[:2] for st in out["states"]]
    out["E"] = None if dev["E"] is None else dev["E"].cpu().numpy()
    out["dev"] = dev
    return out


def _runs_equal_the_one_run_entry(low, mat, ld, ncol, inits, n_runs, tol, max_iter, check_every, what):
    """Run b of every sample against that sample through mxm_em_loop_samples_narrow from init b: every output, to the bit."""
    got = _loop(low, mat, ld, ncol, inits, n_runs, tol, max_iter, check_every)
    for b in range(n_runs):
        one = _loop(low, mat, ld, ncol, [numpy.atleast_2d(init)[b] for init in inits], None, tol, max_iter, check_every)
        for s in range(low.n_entries):
            k = int(ncol[s])
            for key in ("ln_cur", "ln_new", "props_cur"):
                assert numpy.array_equal(_bits(got[key][s, b, :k]), _bits(one[key][s, :k])), (what, key, s, b)
            assert got["states"][s * n_runs + b] == one["states"][s], (what, s, b, got["states"][s * n_runs + b], one["states"][s])
    return got


# ---- the reference's goldens, with g9's 2400 rows in the same batch ---------------------------------------------------------
@pytest.fixture(scope="module")
def pins(b17):
    """g4's 600 rows and g9's 2400 rows as ONE records matrix and their first EM with THREE runs each in one batch (made
    once, shared, never written to): the g4 sample from g5's inits, which are g13's."""
    from mixemt_amd import em, preprocess
    refseq, phy, haps, tables = b17
    g4, g5, g9 = golden("g4_run_em"), golden("g5_run_em_multi"), golden("g9_run_em_2400")
    cm, row0 = preprocess.build_em_records_many(tables, [(g["row_ptr"], g["site"], g["obs"]) for g in (g4, g9)])
    assert list(row0) == [0, 600, 3000] and cm.rest_rows.numel() == 0
    samples = [(cm.rows(0, 600), g4["wts"]), (cm.rows(600, 3000), g9["wts"])]
    rng = numpy.random.default_rng(919)
    inits9 = numpy.concatenate([numpy.atleast_2d(g9["inits"])[:1], rng.dirichlet([1.0] * len(haps), size=2)])
    results = em.run_em_many(samples, em_args(n_multi=3), inits=[g5["inits"], inits9])
    assert [r["route"] for r in results] == ["batch", "batch"] and results[0]["ln_theta_k"].shape == (3, len(haps))
    return {"g4": g4, "g5": g5, "g9": g9, "cm": cm, "samples": samples, "results": results, "haps": haps}


def test_g13_unrefined_multi_run_in_a_batch(pins):
    """The reference's consumers of its own n_multi = 3 run (golden g13): vote, contributors and all 600 labels."""
    from mixemt_amd import assign
    g13, haps = golden("g13_consumers_multi"), pins["haps"]
    assert numpy.array_equal(g13["inits"], pins["g5"]["inits"])
    args = finish_args(refine_ests=False, n_multi=3)
    assert [r["route"] for r in assign.finish_many(pins["samples"], pins["results"], haps, args)] == ["single", "single"]
    got = assign.finish_many(pins["samples"], pins["results"], haps, args, runs="batch")
    assert [r["route"] for r in got] == ["batch", "batch"] and all(r["refined"] is None for r in got)
    me = got[0]
    print("contributors", me["contribs"], "g9:", len(got[1]["contribs"]))
    assert _vote_text(haps, me["vote_order"], me["votes"]) == str(g13["vote_text"])
    assert [c[0] for c in me["contribs"]] == str(g13["contrib_names"]).split("\n")
    assert [c[1] for c in me["contribs"]] == str(g13["contrib_haps"]).split("\n")
    err = numpy.abs(numpy.array([c[2] for c in me["contribs"]]) - g13["contrib_props"]).max()
    print("max |props - g13.contrib_props|", err)
    assert err <= 1e-9
    differ = numpy.flatnonzero(me["row_label"] != g13["assigned"])
    print("labels that differ from g13:", differ)
    assert me["row_label"].shape == (600,) and len(differ) == 0
    assert got[1]["row_label"].shape == (2400,)


def test_g19_refined_multi_run_in_a_batch(pins):
    """bin/mixemt:311-320 with -M 3 (golden g19, made by the reference): the three runs stop apart, after 41, 50 and 46
    iterations."""
    from mixemt_amd import assign
    g13, g19, haps = golden("g13_consumers_multi"), golden("g19_refine_multi"), pins["haps"]
    assert numpy.array_equal(g19["row_ptr"], pins["g4"]["row_ptr"]) and numpy.array_equal(g19["wts"], pins["g4"]["wts"])
    plain = assign.finish_many(pins["samples"], pins["results"], haps, finish_args(refine_ests=False, n_multi=3), runs="batch")
    k9 = len(plain[1]["contribs"])
    inits = [g19["inits"], numpy.random.default_rng(7).dirichlet([1.0] * k9, size=3) if k9 else None]
    got = assign.finish_many(pins["samples"], pins["results"], haps, finish_args(n_multi=3), refine_inits=inits, runs="batch",
                             want_posterior=True)
    assert [r["route"] for r in got] == ["batch", "batch"]
    me = got[0]
    assert me["sub_haps"] == [haps[int(c)] for c in g19["cols"]]
    assert [c[:2] for c in me["contribs"]] == [c[:2] for c in plain[0]["contribs"]]
    assert [c[1] for c in me["contribs"]] == str(g13["contrib_haps"]).split("\n")
    print("refined iterations", me["refined"]["iters"], "golden", list(g19["iters"]), "done", me["refined"]["done"])
    assert [int(v) for v in g19["iters"]] == [41, 50, 46]
    assert me["refined"]["iters"] == [41, 50, 46] and me["refined"]["done"] == [1, 1, 1]
    assert me["refined"]["inits"].shape == (3, 3) and me["refined"]["ln_theta_k"].shape == (3, 3) == me["refined"]["ln_theta_next"].shape
    err = numpy.abs(me["refined"]["props"] - g19["props"]).max()
    err2 = numpy.abs(numpy.array([c[2] for c in me["contribs"]]) - g19["refined_props"]).max()
    print("max |props - g19.props|", err, "max |contributor props - g19.refined_props|", err2)
    assert err <= 1e-9 and err2 <= 1e-9
    differ = numpy.flatnonzero(me["row_label"] != g19["assigned"])
    print("labels that differ from g19:", differ)
    assert me["row_label"].shape == (600,) and len(differ) == 0
    mix = me["posterior"].cpu().numpy()
    assert mix.shape == g19["mix"].shape == (600, 3)
    assert numpy.array_equal(numpy.isneginf(mix), numpy.isneginf(g19["mix"]))
    fin = ~numpy.isneginf(g19["mix"])
    assert numpy.isfinite(mix[fin]).all()
    print("max |posterior - g19.mix|", numpy.abs(mix[fin] - g19["mix"][fin]).max())
    assert numpy.abs(mix[fin] - g19["mix"][fin]).max() <= 1e-9
    if k9:
        assert len(got[1]["refined"]["iters"]) == 3 and got[1]["row_label"].shape == (2400,)


def test_g14_three_runs_of_the_unmixed_sample(pins):
    """Three runs on 600 x 1 (golden g14's inits3 / iters3 / props3): the draws, the stops and the fold exactly."""
    from mixemt_amd import assign
    g14, haps = golden("g14_single_contributor"), pins["haps"]
    assert numpy.array_equal(g14["row_ptr"], pins["g4"]["row_ptr"]) and numpy.array_equal(g14["wts"], pins["g4"]["wts"])
    numpy.random.seed(13)
    res = assign.finish_many(pins["samples"][:1], pins["results"][:1], haps,
                             finish_args(contributors=haps[int(g14["col"][0])], n_multi=3), runs="batch")[0]
    assert res["route"] == "batch" and [c[:2] for c in res["contribs"]] == [["hap1", haps[int(g14["col"][0])]]]
    assert res["refined"]["inits"].shape == (3, 1) and numpy.array_equal(res["refined"]["inits"], g14["inits3"])
    assert res["refined"]["iters"] == [int(v) for v in g14["iters3"]] and res["refined"]["done"] == [1, 1, 1]
    assert list(res["refined"]["props"]) == list(g14["props3"]) and [c[2] for c in res["contribs"]] == list(g14["props3"])
    assert list(res["assigned"]) == ["hap1"] and sorted(res["assigned"]["hap1"]) == list(range(600))
    assert not res["row_label"].any()


# ---- stops ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g19_loop(pins):
    """The g4 sample reduced to g19's three columns beside the g9 sample reduced to five: (low, mat, ld, ncol, inits)."""
    g19 = golden("g19_refine_multi")
    low = _low(pins["samples"])
    ld = 8
    cols = numpy.zeros((2, ld), dtype=numpy.int32)
    cols[0, :3] = g19["cols"]
    cols[1, :5] = [7, 300, 1999, 4000, 5400]
    ncol = numpy.array([3, 5], dtype=numpy.int32)
    inits = [g19["inits"], numpy.random.default_rng(3).dirichlet([1.0] * 5, size=3)]
    return low, low.gather(cols, ncol, ld), ld, ncol, inits


@pytest.mark.parametrize("check_every", [1, 16])
def test_runs_that_stop_in_different_chunks_equal_the_one_run_entry(g19_loop, check_every):
    """g19's runs stop after 41, 50 and 46 iterations: with read-backs every 16 iterations run 1 goes on for a launch after
    its siblings have stopped, with one per iteration for nine.  Each run must equal the one-run entry from its init --
    which was never launched again after ITS stop -- to the bit: a stopped run's ln_*, props, iters and l1 do not move.
    A further call on the finished states changes nothing either."""
    low, mat, ld, ncol, inits = g19_loop
    got = _runs_equal_the_one_run_entry(low, mat, ld, ncol, inits, 3, 1e-4, 10000, check_every, "check_every %d" % check_every)
    assert [st[:2] for st in got["states"][:3]] == [(1, 41), (1, 50), (1, 46)]
    assert len({(st[1] - 1) // 16 for st in got["states"][:3]}) > 1                   # (they do stop in different chunks)
    again = _loop(low, mat, ld, ncol, None, 3, 1e-4, 10000, check_every, resume=got["dev"])
    assert again["states"] == got["states"]
    for key in ("ln_cur", "ln_new", "props_cur"):
        assert numpy.array_equal(_bits(again[key]), _bits(got[key])), key
    assert (got["E"][:600] == -7.0).all() and (got["E"][600:, :5] != -7.0).all()       # 600 x 3 fits LDS, 2400 x 5 does not


def test_max_iter_stops_some_runs_while_their_siblings_converge(g19_loop):
    low, mat, ld, ncol, inits = g19_loop
    got = _runs_equal_the_one_run_entry(low, mat, ld, ncol, inits, 3, 1e-4, 45, 16, "max_iter 45")
    assert [st[:2] for st in got["states"][:3]] == [(1, 41), (2, 45), (2, 45)]
    full = _loop(low, mat, ld, ncol, inits, 3, 1e-4, 10000, 16)
    for key in ("ln_cur", "ln_new", "props_cur"):                                     # the converged run is the unlimited call's
        assert numpy.array_equal(_bits(got[key][0, 0]), _bits(full[key][0, 0])), key


# ---- small shapes: entry against entry, and against the per-sample route ----------------------------------------------------
SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 257]          # tile = 32 rows, assignment block = 64 threads
RUNS_OF = {1: 2, 2: 3, 4: 5, 5: 2, 8: 3, 9: 5, 16: 2}          # K -> B: every ld with and without pad columns, B in {2, 3, 5}


@pytest.fixture(scope="module", params=[66, 128, 5408])
def small(request):
    """Samples of SIZES rows in one batch (weights with 0 and > 1) and, per B, their first EM with B runs (made on demand,
    once)."""
    from mixemt_amd import _lib, em
    n_haps = request.param
    assert _lib.load().mxm_samples_tile_rows() == 32
    rng = numpy.random.default_rng(5200 + n_haps)
    mats = [_few_values(rng, rows, n_haps, 9) for rows in SIZES]
    wts = [rng.integers(0, 5, size=len(m)).astype(numpy.float64) for m in mats]
    for w in wts:
        w[0] = max(w[0], 2.0)
    assert any((w == 0).any() for w in wts) and any((w > 1).any() for w in wts)
    cm, row0 = _records_of(mats)
    samples = [(cm.rows(row0[i], row0[i + 1]), wts[i]) for i in range(len(mats))]
    first = {}

    def results(n_runs):
        if n_runs not in first:
            inits = [numpy.random.default_rng(n_haps + 31 * n_runs + s).dirichlet([1.0] * n_haps, size=n_runs) for s in range(len(mats))]
            first[n_runs] = em.run_em_many(samples, em_args(max_iter=40, n_multi=n_runs), inits=inits)
            assert all(r["route"] == "batch" for r in first[n_runs])
        return first[n_runs]
    return {"samples": samples, "results": results, "haps": ["h%04d" % i for i in range(n_haps)], "n_haps": n_haps}


@pytest.mark.parametrize("n_runs", [2, 3, 5])
def test_votes_equal_the_per_sample_multi_run_vote(small, n_runs):
    """best, first-seen order and integer-weight votes: exactly those of mxm_row_argmax_votes_coded with n_runs = B on the
    sample's own records, row for row; lse[r][b] is the run's normaliser."""
    import torch
    from mixemt_amd import assign
    samples, results = small["samples"], small["results"](n_runs)
    low = _low(samples)
    ln_props = numpy.stack([r["ln_theta_k"] for r in results])
    best, votes, counts, first, lse, errors = low.votes_runs(ln_props, want_lse=True)
    best = best.cpu().numpy()
    assert not any(errors) and lse.shape == (low.n_rows, n_runs) and torch.isfinite(lse).all()
    one_run = low.votes(ln_props[:, 1], want_lse=True)[4]                         # the one-run entry under run 1's proportions
    assert numpy.array_equal(_bits(lse[:, 1].cpu().numpy()), _bits(one_run.cpu().numpy()))
    for s, ((cm, w), res) in enumerate(zip(samples, results)):
        lo, hi = int(low.row0[s]), int(low.row0[s + 1])
        want_best, want_votes = assign.row_argmax_votes_records(cm, res["ln_theta_k"], w)
        assert numpy.array_equal(best[lo:hi], want_best), s
        assert numpy.array_equal(votes[s], want_votes)                         # integer weights: exact in any order
        assert numpy.array_equal(counts[s], numpy.bincount(want_best, minlength=cm.n_haps))
        order, _ = assign.vote_table_from_records(cm, res["ln_theta_k"], None)
        mine = numpy.flatnonzero(first[s] < cm.n_rows)
        assert numpy.array_equal(mine[numpy.argsort(first[s][mine], kind="stable")], order)


def _against_the_per_sample_route(samples, results, haps, cols, n_runs, rng, what, max_iter=300):
    from mixemt_amd import assign
    n_contribs = len(cols)
    args = finish_args(contributors=",".join(haps[int(c)] for c in cols), max_iter=max_iter, n_multi=n_runs)
    inits = [rng.dirichlet([1.0] * n_contribs, size=n_runs) for _ in samples]
    got = assign.finish_many(samples, results, haps, args, refine_inits=inits, runs="batch", want_posterior=True)
    assert [r["route"] for r in got] == ["batch"] * len(samples)
    for s, ((cm, w), res) in enumerate(zip(samples, results)):
        where = "%s: sample %d of %d rows" % (what, s, cm.n_rows)
        want = _per_sample(cm, w, res, haps, args, inits[s])
        assert not (numpy.abs(want["margin"] - numpy.log(args.min_fold)) <= BAND).any(), where      # (the seed leaves the band empty)
        _same_as_per_sample(got[s], want, args.min_fold, where)
        assert numpy.array_equal(got[s]["row_label"], want["row_label"]), where                    # ... so no label may differ
        assert len(got[s]["refined"]["iters"]) == n_runs and got[s]["refined"]["inits"].shape == (n_runs, n_contribs)
        post, ref = got[s]["posterior"].cpu().numpy(), want["run"]["read_mix"].cpu().numpy()
        assert post.shape == ref.shape == (cm.n_rows, n_contribs)
        assert numpy.array_equal(numpy.isneginf(post), numpy.isneginf(ref)), where
        fin = numpy.isfinite(ref)
        err = numpy.abs(post[fin] - ref[fin]).max() if fin.any() else 0.0
        assert numpy.isfinite(post[fin]).all() and err <= 1e-9, (where, err)
    return got, inits


@pytest.mark.parametrize("n_contribs", sorted(RUNS_OF))
def test_small_shapes_against_the_one_run_entry_and_the_per_sample_route(small, n_contribs):
    n_runs = RUNS_OF[n_contribs]
    samples, results, haps = small["samples"], small["results"](n_runs), small["haps"]
    rng = numpy.random.default_rng(small["n_haps"] + 100 * n_contribs)
    cols = numpy.sort(rng.choice(len(haps), size=n_contribs, replace=False))
    what = "H %d, K %d, B %d" % (small["n_haps"], n_contribs, n_runs)
    got, inits = _against_the_per_sample_route(samples, results, haps, cols, n_runs, rng, what)
    print(what, "iterations", [r["refined"]["iters"] for r in got])
    # the loop entry against the one-run entry, from the same inits
    low = _low(samples)
    ld = 4 if n_contribs <= 4 else (8 if n_contribs <= 8 else 16)
    table = numpy.zeros((len(samples), ld), dtype=numpy.int32)
    table[:, :n_contribs] = cols
    ncol = numpy.full(len(samples), n_contribs, dtype=numpy.int32)
    mat = low.gather(table, ncol, ld)
    for check_every in (1, 16):
        loop = _runs_equal_the_one_run_entry(low, mat, ld, ncol, inits, n_runs, 1e-4, 300, check_every, what)
        for s, r in enumerate(got):                                               # ... and finish_many reports that loop
            assert r["refined"]["iters"] == [st[1] for st in loop["states"][s * n_runs:(s + 1) * n_runs]]
            assert numpy.array_equal(_bits(r["refined"]["ln_theta_next"]), _bits(loop["ln_new"][s, :, :n_contribs]))


@pytest.mark.parametrize("n_contribs,rows,n_runs", [(3, (3072, 3073), 3), (16, (576, 577), 2)])
def test_either_side_of_the_lds_limit(n_contribs, rows, n_runs):
    """9216 cells: the sample that still fits is linearised in every workgroup's LDS, the one row larger reads the copy E that
    one pass made for all its runs -- and a batch without such a sample takes no E at all."""
    from mixemt_amd import em
    rng = numpy.random.default_rng(9216 + n_contribs)
    n_haps = 66
    assert rows[0] * n_contribs == 9216
    mats = [_few_values(rng, n, n_haps, 9) for n in rows]
    wts = [rng.integers(0, 4, size=len(m)).astype(numpy.float64) for m in mats]
    cm, row0 = _records_of(mats)
    samples = [(cm.rows(row0[i], row0[i + 1]), wts[i]) for i in range(2)]
    results = em.run_em_many(samples, em_args(max_iter=20, n_multi=n_runs), inits=[rng.dirichlet([1.0] * n_haps, size=n_runs) for _ in mats])
    haps = ["h%04d" % i for i in range(n_haps)]
    cols = numpy.sort(rng.choice(n_haps, size=n_contribs, replace=False))
    what = "K %d, rows %s" % (n_contribs, rows)
    got, inits = _against_the_per_sample_route(samples, results, haps, cols, n_runs, rng, what, max_iter=60)
    low = _low(samples)
    ld = 4 if n_contribs <= 4 else 16
    table = numpy.zeros((2, ld), dtype=numpy.int32)
    table[:, :n_contribs] = cols
    ncol = numpy.full(2, n_contribs, dtype=numpy.int32)
    mat = low.gather(table, ncol, ld)
    for check_every in (1, 16):
        loop = _runs_equal_the_one_run_entry(low, mat, ld, ncol, inits, n_runs, 1e-4, 60, check_every, what)
        assert (loop["E"][:rows[0]] == -7.0).all()                                # the sample that fits never touches E
        dense = mat.cpu().numpy()[rows[0]:, :n_contribs]
        want_e = numpy.exp(dense - dense.max(axis=1)[:, None])
        assert numpy.abs(loop["E"][rows[0]:, :n_contribs] - want_e).max() <= 1e-15 and (loop["E"][rows[0]:, n_contribs:] == 0.0).all()
    # the first sample alone: no E is needed ...
    alone = _low(samples[:1])
    one = _loop(alone, mat[:rows[0]], ld, ncol[:1], inits[:1], n_runs, 1e-4, 60, 16, with_e=False)
    assert one["states"] == loop["states"][:n_runs]
    # ... the second alone without one is refused before anything runs
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream
    import torch
    second = _low(samples[1:])
    state = em.new_state(n_runs, second.dev)
    vec = torch.zeros((n_runs, ld), dtype=torch.float64, device=second.dev)
    host = (_lib.EmState * n_runs)()
    assert second.lib.mxm_em_loop_samples_narrow_runs(ctypes.byref(second.coded), second.row0_ptr, 1, n_haps, n_runs,
                                                      mat[rows[0]:].data_ptr(), ld, ncol[1:].ctypes.data, second.wts.data_ptr(),
                                                      vec.data_ptr(), vec.data_ptr(), vec.data_ptr(), state.data_ptr(), 1e-4, 60, 16,
                                                      None, second.ws.data_ptr(), second.ws_bytes, current_stream(), host) == -1
    assert b"needs the global copy E" in second.lib.mxm_last_error()


# ---- the same bits alone, first, last and twice -----------------------------------------------------------------------------
def test_a_multi_run_sample_is_the_same_bits_alone_first_or_last(pins):
    from mixemt_amd import assign
    haps, g5 = pins["haps"], pins["g5"]
    me, mine = pins["samples"][0], pins["results"][0]
    others = [pins["samples"][1]] + [(pins["samples"][0][0], g5["wts"] + 1)] * 3
    theirs = [pins["results"][1]] + [pins["results"][0]] * 3

    def run_fixed(samples, results):
        low = _low(samples)
        best, votes, counts, first, lse, errors = low.votes_runs(numpy.stack([r["ln_theta_k"] for r in results]), want_lse=True)
        assert not any(errors)
        plain = assign.finish_many(samples, results, haps, finish_args(refine_ests=False, n_multi=3), runs="batch")
        inits = []
        for r in plain:                                                            # three different starts per sample, fixed
            base = numpy.linspace(1.0, 2.0, len(r["contribs"]))
            starts = numpy.stack([base, base[::-1], base ** 2]) if len(base) else None
            inits.append(None if starts is None else starts / starts.sum(axis=1, keepdims=True))
        out = assign.finish_many(samples, results, haps, finish_args(n_multi=3), refine_inits=inits, runs="batch", want_posterior=True)
        assert [r["route"] for r in out] == ["batch"] * len(samples)
        return low.row0, best.cpu().numpy(), votes, counts, first, out, lse.cpu().numpy(), plain

    alone = run_fixed([me], [mine])
    first_of = run_fixed([me] + others, [mine] + theirs)
    last_of = run_fixed(others + [me], theirs + [mine])
    again = run_fixed(others + [me], theirs + [mine])
    for got, at in ((first_of, 0), (last_of, 4)):
        lo, hi = int(got[0][at]), int(got[0][at + 1])
        assert numpy.array_equal(got[1][lo:hi], alone[1])                                          # best
        assert numpy.array_equal(_bits(got[6][lo:hi]), _bits(alone[6]))                             # lse [R][B]
        assert numpy.array_equal(_bits(got[2][at]), _bits(alone[2][0]))                             # votes
        assert numpy.array_equal(got[3][at], alone[3][0]) and numpy.array_equal(got[4][at], alone[4][0])      # counts, first
        assert numpy.array_equal(got[7][at]["row_label"], alone[7][0]["row_label"])                 # unrefined labels
        a, b = got[5][at], alone[5][0]
        assert a["refined"]["iters"] == b["refined"]["iters"] and len(a["refined"]["iters"]) == 3
        for key in ("ln_theta_k", "ln_theta_next", "props"):
            assert numpy.array_equal(_bits(a["refined"][key]), _bits(b["refined"][key])), key
        assert numpy.array_equal(a["row_label"], b["row_label"])
        assert numpy.array_equal(_bits(a["posterior"].cpu().numpy()), _bits(b["posterior"].cpu().numpy()))
    for a, b in zip(last_of[5], again[5]):                # two runs of the same batch
        assert a["refined"]["iters"] == b["refined"]["iters"]
        for key in ("ln_theta_k", "ln_theta_next"):
            assert numpy.array_equal(_bits(a["refined"][key]), _bits(b["refined"][key])), key
        assert numpy.array_equal(a["row_label"], b["row_label"])
    assert numpy.array_equal(last_of[1], again[1]) and numpy.array_equal(_bits(last_of[2]), _bits(again[2]))


# ---- edges ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge():
    """Three samples of 40, 70 and 33 rows at H = 128 with two identical columns, and their first EM with two runs."""
    from mixemt_amd import em
    rng = numpy.random.default_rng(61)
    n_haps = 128
    mats = [_few_values(rng, rows, n_haps, 7) for rows in (40, 70, 33)]
    for m in mats:
        m[:, 90] = m[:, 12]
    wts = [rng.integers(1, 4, size=len(m)).astype(numpy.float64) for m in mats]
    cm, row0 = _records_of(mats)
    samples = [(cm.rows(row0[i], row0[i + 1]), wts[i]) for i in range(3)]
    results = em.run_em_many(samples, em_args(max_iter=20, n_multi=2), inits=[rng.dirichlet([1.0] * n_haps, size=2) for _ in mats])
    return {"samples": samples, "results": results, "haps": ["h%04d" % i for i in range(n_haps)]}


def test_exactly_equal_columns_still_go_to_the_later_column(edge):
    """Two identical columns from equal inits stay identical to the bit in every run, so the fold of the runs is an exact tie in
    every row; with min_fold = 1 the tie decides the label: the later column, through perm, whichever order they are named in."""
    from mixemt_amd import assign
    samples, results, haps = edge["samples"], edge["results"], edge["haps"]
    for named in ("h0012,h0090", "h0090,h0012"):
        args = finish_args(contributors=named, min_fold=1.0, max_iter=50, n_multi=2)
        inits = [numpy.array([[0.5, 0.5], [0.5, 0.5]])] * 3
        got = assign.finish_many(samples, results, haps, args, refine_inits=inits, runs="batch")
        for s, (view, w) in enumerate(samples):
            want = _per_sample(view, w, results[s], haps, args, inits[s])
            assert (want["margin"] == 0.0).all()                          # exact ties throughout
            later = [c[1] for c in want["contribs"]].index("h0090")
            assert (want["row_label"] == later).all()
            assert got[s]["route"] == "batch" and numpy.array_equal(got[s]["row_label"], want["row_label"]), (named, s)
            assert got[s]["refined"]["props"][0] == got[s]["refined"]["props"][1]


def test_a_row_without_a_record_poisons_its_own_sample_only(edge):
    from mixemt_amd import assign, em, preprocess
    samples, results, haps = edge["samples"], edge["results"], edge["haps"]
    ln_props = numpy.stack([r["ln_theta_k"] for r in results])
    good = _low(samples)
    best, votes, counts, first, lse, errors = good.votes_runs(ln_props, want_lse=True)
    assert errors == [False, False, False]
    ndist = good.ndist.clone()
    at = int(good.row0[1]) + 7
    ndist[at] = 0                                             # forged in a copy: the row is never dereferenced
    bad = em.SampleFinish(good.rec, good.rec_off, ndist, good.wts, good.rowmax, good.row0, good.n_haps)
    best2, votes2, counts2, first2, lse2, errors2 = bad.votes_runs(ln_props, want_lse=True)
    assert errors2 == [False, True, False] and numpy.isnan(votes2[1]).all()
    assert int(best2[at]) == -1 and numpy.isnan(lse2[at].cpu().numpy()).all()
    for s in (0, 2):
        lo, hi = int(good.row0[s]), int(good.row0[s + 1])
        assert numpy.array_equal(best2[lo:hi].cpu().numpy(), best[lo:hi].cpu().numpy())
        assert numpy.array_equal(_bits(lse2[lo:hi].cpu().numpy()), _bits(lse[lo:hi].cpu().numpy()))
        assert numpy.array_equal(_bits(votes2[s]), _bits(votes[s]))
        assert numpy.array_equal(first2[s], first[s]) and numpy.array_equal(counts2[s], counts[s])
    cm1 = samples[1][0]
    forged = preprocess.CodedMatrix(cm1.n_rows, cm1.n_haps, cm1.rec, cm1.rec_off, ndist[int(good.row0[1]):int(good.row0[2])],
                                    cm1.rowmax, cm1.used, cm1.rest_rows, cm1.m_rest)
    with pytest.raises(ValueError, match="sample 1 has a row without a record"):
        assign.finish_many([samples[0], (forged, samples[1][1]), samples[2]], results, haps,
                           finish_args(contributors="%s,%s" % (haps[1], haps[2]), n_multi=2), runs="batch")


def test_a_sample_without_contributors_beside_a_normal_one_draws_no_inits(pins):
    from mixemt_amd import assign, em
    haps, g5 = pins["haps"], pins["g5"]
    few = (pins["cm"].rows(0, 5), numpy.ones(5))          # total weight 5 < min_reads
    res_few = em.run_em_many([few], em_args(max_iter=30, n_multi=3), inits=[g5["inits"]])[0]
    numpy.random.seed(13)
    got = assign.finish_many([few, pins["samples"][0]], [res_few, pins["results"][0]], haps, finish_args(n_multi=3), runs="batch")
    assert got[0]["contribs"] == [] and got[0]["refined"] is None and got[0]["route"] == "batch"
    assert len(got[0]["assigned"]) == 0 and got[0]["row_label"].shape == (0,) and len(got[0]["vote_order"]) >= 1
    numpy.random.seed(13)
    alone = assign.finish_many(pins["samples"][:1], pins["results"][:1], haps, finish_args(n_multi=3), runs="batch")[0]
    assert got[1]["route"] == alone["route"] == "batch" and len(got[1]["contribs"]) == 3 and got[1]["contribs"] == alone["contribs"]
    assert numpy.array_equal(got[1]["row_label"], alone["row_label"])
    assert got[1]["refined"]["inits"].shape == (3, 3)
    assert numpy.array_equal(got[1]["refined"]["inits"], alone["refined"]["inits"])          # the empty sample drew nothing


def test_fall_backs_and_the_default(edge):
    """17 contributors leave the batch with the same keys; runs="single" is the default, and with one run the keyword changes
    nothing."""
    from mixemt_amd import assign, em
    samples, results, haps = edge["samples"], edge["results"], edge["haps"]
    rng = numpy.random.default_rng(17)
    two = finish_args(contributors="%s,%s" % (haps[3], haps[40]), max_iter=50, n_multi=2)
    inits2 = [rng.dirichlet([1.0] * 2, size=2) for _ in samples]
    batch = assign.finish_many(samples, results, haps, two, refine_inits=inits2, runs="batch")
    assert [r["route"] for r in batch] == ["batch"] * 3
    cols17 = rng.choice(len(haps), size=17, replace=False)
    args17 = finish_args(contributors=",".join(haps[int(c)] for c in cols17), max_iter=50, n_multi=2)
    inits17 = [rng.dirichlet([1.0] * 17, size=2) for _ in samples]
    got = assign.finish_many(samples, results, haps, args17, refine_inits=inits17, runs="batch")
    assert [r["route"] for r in got] == ["single"] * 3 and all(set(r) == set(batch[0]) for r in got)
    for s, (cm, w) in enumerate(samples):
        _same_as_per_sample(got[s], _per_sample(cm, w, results[s], haps, args17, inits17[s]), args17.min_fold, "17 contributors")
    # rows above max_rows leave it too, sample by sample
    capped = assign.finish_many(samples, results, haps, two, refine_inits=inits2, runs="batch", max_rows=40)
    assert [r["route"] for r in capped] == ["batch", "single", "batch"]
    for s in range(3):
        assert capped[s]["refined"]["iters"] == batch[s]["refined"]["iters"]
        assert numpy.array_equal(capped[s]["row_label"], batch[s]["row_label"])
    # the default is runs="single": today's result, unchanged
    default = assign.finish_many(samples, results, haps, two, refine_inits=inits2)
    named = assign.finish_many(samples, results, haps, two, refine_inits=inits2, runs="single")
    assert [r["route"] for r in default] == [r["route"] for r in named] == ["single"] * 3
    for a, b, c in zip(default, named, batch):
        assert a["contribs"] == b["contribs"] and numpy.array_equal(a["row_label"], b["row_label"])
        assert a["refined"]["iters"] == b["refined"]["iters"] == c["refined"]["iters"]
        assert numpy.array_equal(_bits(a["refined"]["props"]), _bits(b["refined"]["props"]))
        assert numpy.abs(a["refined"]["props"] - c["refined"]["props"]).max() < PROPS_ATOL
    # one run: the keyword changes nothing, bit for bit
    res1 = em.run_em_many(samples, em_args(max_iter=20), inits=[r["inits"][:1] for r in results])
    one = finish_args(contributors=two.contributors, max_iter=50)
    inits1 = [i[0] for i in inits2]
    a = assign.finish_many(samples, res1, haps, one, refine_inits=inits1)
    b = assign.finish_many(samples, res1, haps, one, refine_inits=inits1, runs="batch")
    for x, y in zip(a, b):
        assert x["route"] == y["route"] == "batch" and x["refined"]["iters"] == y["refined"]["iters"]
        assert numpy.array_equal(_bits(x["refined"]["ln_theta_next"]), _bits(y["refined"]["ln_theta_next"]))
        assert numpy.array_equal(x["row_label"], y["row_label"])
