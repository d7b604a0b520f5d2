"""
The batched second half of a cohort run (assign.finish_many; mxm_votes_samples, mxm_gather_columns_samples,
mxm_em_loop_samples_narrow, mxm_assign_reads_samples): every sample must come out as the per-sample functions leave it
-- the reference's goldens g8 / g14 / g6 per sample, the existing per-sample route on small shapes, and the same BITS
whatever else shares the batch.
"""
import argparse
import collections
import ctypes

import numpy
import pytest

from conftest import em_args, golden

pytestmark = pytest.mark.gpu

PROPS_ATOL = 1e-9            # the project's own bar for proportions (tests/test_gpu_samples.py)
BAND = 1e-9                  # a row label may differ only where the top-two margin is this close to log(min_fold)


def finish_args(**kw):
    args = argparse.Namespace(min_reads=10, contributors=None, var_check=False, min_var_reads=3, frac_var_reads=0.02,
                              var_count=None, var_fraction=0.5, refine_ests=True, min_fold=2.0, tolerance=0.0001,
                              max_iter=10000, init_alpha=1.0, n_multi=1, verbose=False)
    for key, val in kw.items():
        setattr(args, key, val)
    return args


@pytest.fixture(scope="module")
def pins(b17):
    """g4's 600 rows and g9's 2400 rows as ONE records matrix and their first EM in one batch (made once, shared, never
    written to)."""
    from mixemt_amd import em, preprocess
    refseq, phy, haps, tables = b17
    g4, g9 = golden("g4_run_em"), golden("g9_run_em_2400")
    cm, row0 = preprocess.build_em_records_many(tables, [(g["row_ptr"], g["site"], g["obs"]) for g in (g4, g9)])
    assert list(row0) == [0, 600, 3000] and cm.rest_rows.numel() == 0
    samples = [(cm.rows(0, 600), g4["wts"]), (cm.rows(600, 3000), g9["wts"])]
    results = em.run_em_many(samples, em_args(), inits=[g4["inits"], g9["inits"]])
    assert [r["route"] for r in results] == ["batch", "batch"]
    return {"g4": g4, "g9": g9, "cm": cm, "samples": samples, "results": results, "haps": haps}


def _vote_text(haps, order, votes):
    """stats.report_read_votes' text (stats.py:34-45) from a vote table."""
    counter = collections.Counter()
    for h in order:
        counter[int(h)] = int(votes[h])
    text = "\nTop 10 haplogroups by read probabilities...\n"
    for hap_i, count in counter.most_common(10):
        text += "%s\t%d\n" % (haps[hap_i], count)
    return text + "\n"


def test_g8_in_a_batch(pins):
    """The reference's consumers of the g4 run (golden g8), with g9's 2400 rows in the same batch."""
    from mixemt_amd import assign
    g8, haps = golden("g8_consumers"), pins["haps"]
    samples, results = pins["samples"], pins["results"]
    plain = assign.finish_many(samples, results, haps, finish_args(refine_ests=False))
    assert [r["route"] for r in plain] == ["batch", "batch"] and all(r["refined"] is None for r in plain)
    me = plain[0]
    print("contributors", me["contribs"], "g9:", len(plain[1]["contribs"]))
    assert [c[0] for c in me["contribs"]] == str(g8["contrib_names"]).split("\n")
    assert [c[1] for c in me["contribs"]] == str(g8["contrib_haps"]).split("\n")
    cols = {haps.index(c[1]) for c in me["contribs"]}
    assert [int(h) for h in me["vote_order"] if int(h) in cols] == [int(c) for c in g8["contributors"]]      # first-seen order
    err = numpy.abs(numpy.array([c[2] for c in me["contribs"]]) - g8["contrib_props"]).max()
    print("max |props - g8.contrib_props|", err)
    assert err < PROPS_ATOL
    assert me["row_label"].shape == (600,) and numpy.array_equal(me["row_label"], g8["assigned"])
    assert _vote_text(haps, me["vote_order"], me["votes"]) == str(g8["vote_text"])
    assert me["sub_haps"] == [haps[c] for c in sorted(cols)]
    # refined, with the reference's own draw for the g4 sample
    inits = [g8["refined_inits"][0], numpy.full(len(plain[1]["contribs"]), 1.0 / max(1, len(plain[1]["contribs"])))]
    res = assign.finish_many(samples, results, haps, finish_args(), refine_inits=inits)
    me = res[0]
    assert [r["route"] for r in res] == ["batch", "batch"]
    assert [c[:2] for c in me["contribs"]] == [c[:2] for c in plain[0]["contribs"]]
    print("refined iterations", me["refined"]["iters"], "golden", list(g8["refined_iters"]))
    assert me["refined"]["iters"] == [int(v) for v in g8["refined_iters"]] and me["refined"]["done"] == [1]
    err = numpy.abs(numpy.array([c[2] for c in me["contribs"]]) - g8["refined_props"]).max()
    print("max |refined props - g8.refined_props|", err)
    assert err < PROPS_ATOL
    assert numpy.array_equal(me["row_label"], g8["refined_assigned"])
    names = [c[0] for c in me["contribs"]]
    for k, name in enumerate(names):                      # the AssignedReads is the labels' table, in contributor order
        assert numpy.array_equal(me["assigned"].rows(name), numpy.flatnonzero(me["row_label"] == k))
    assert me["assigned"].count("unassigned") == int((me["row_label"] < 0).sum())
    assert res[1]["row_label"].shape == (2400,) and res[1]["refined"]["done"] == [1]


def test_g14_the_unmixed_sample(pins):
    """One contributor: still refined on 600 x 1 (bin/mixemt:311-320; golden g14 pins the iteration count)."""
    from mixemt_amd import assign
    g14, haps = golden("g14_single_contributor"), pins["haps"]
    assert numpy.array_equal(g14["row_ptr"], pins["g4"]["row_ptr"]) and numpy.array_equal(g14["wts"], pins["g4"]["wts"])
    numpy.random.seed(13)
    res = assign.finish_many(pins["samples"][:1], pins["results"][:1], haps, finish_args(contributors=haps[int(g14["col"][0])]))[0]
    assert res["route"] == "batch" and [c[:2] for c in res["contribs"]] == [["hap1", haps[int(g14["col"][0])]]]
    assert numpy.array_equal(res["refined"]["inits"], g14["inits"])
    assert res["refined"]["iters"] == [int(v) for v in g14["iters"]] and res["refined"]["done"] == [1]
    assert [c[2] for c in res["contribs"]] == list(g14["refined_props"])
    assert list(res["assigned"]) == ["hap1"] and sorted(res["assigned"]["hap1"]) == list(g14["assigned"])
    assert not res["row_label"].any()


def test_g6_five_columns(pins):
    from mixemt_amd import assign
    g6, haps = golden("g6_refine"), pins["haps"]
    assert numpy.array_equal(g6["row_ptr"], pins["g4"]["row_ptr"]) and numpy.array_equal(g6["wts"], pins["g4"]["wts"])
    names = [haps[int(c)] for c in g6["cols"]]
    res = assign.finish_many(pins["samples"][:1], pins["results"][:1], haps, finish_args(contributors=",".join(names[::-1])),
                             refine_inits=[g6["inits"][0]], want_posterior=True)[0]
    assert res["route"] == "batch" and res["sub_haps"] == names            # ascending haplogroup index, whatever was asked
    print("iterations", res["refined"]["iters"], "golden", list(g6["iters"]))
    assert res["refined"]["iters"] == [int(v) for v in g6["iters"]]
    err = numpy.abs(res["refined"]["props"] - g6["props"]).max()
    print("max |props - g6.props|", err)
    assert err < PROPS_ATOL
    mix = res["posterior"].cpu().numpy()
    assert mix.shape == g6["mix"].shape
    assert numpy.array_equal(numpy.isneginf(mix), numpy.isneginf(g6["mix"]))
    fin = numpy.isfinite(mix) & numpy.isfinite(g6["mix"])
    assert numpy.array_equal(fin, ~numpy.isneginf(g6["mix"]))
    print("max |posterior - g6.mix|", numpy.abs(mix[fin] - g6["mix"][fin]).max())
    assert numpy.abs(mix[fin] - g6["mix"][fin]).max() < 1e-9


def test_a_sample_is_the_same_bits_alone_first_or_last(pins):
    import torch
    from mixemt_amd import assign
    haps, g5 = pins["haps"], golden("g5_run_em_multi")
    me, mine = pins["samples"][0], pins["results"][0]
    others = [pins["samples"][1]] + [(pins["samples"][0][0], g5["wts"])] * 3
    theirs = [pins["results"][1]] + [pins["results"][0]] * 3
    args = finish_args()

    def run_fixed(samples, results):
        low = assign._finish_batch(samples, [torch.from_numpy(numpy.asarray(w, dtype=numpy.float64)).cuda() for _, w in samples],
                                   list(range(len(samples))))
        best, votes, counts, first, _, errors = low.votes(numpy.stack([r["ln_theta_k"][0] for r in results]))
        assert not any(errors)
        plain = assign.finish_many(samples, results, haps, finish_args(refine_ests=False))
        inits = [numpy.full(len(r["contribs"]), 1.0 / len(r["contribs"])) for r in plain]
        out = assign.finish_many(samples, results, haps, args, refine_inits=inits)
        return low.row0, best.cpu().numpy(), votes, counts, first, out

    alone = run_fixed([me], [mine])
    first_of = run_fixed([me] + others, [mine] + theirs)
    last_of = run_fixed(others + [me], theirs + [mine])
    again = run_fixed(others + [me], theirs + [mine])
    for got, at in ((first_of, 0), (last_of, 4)):
        lo, hi = int(got[0][at]), int(got[0][at + 1])
        assert numpy.array_equal(got[1][lo:hi], alone[1])                                          # best
        assert numpy.array_equal(got[2][at].view(numpy.int64), alone[2][0].view(numpy.int64))      # votes
        assert numpy.array_equal(got[3][at], alone[3][0]) and numpy.array_equal(got[4][at], alone[4][0])      # counts, first
        a, b = got[5][at], alone[5][0]
        assert a["refined"]["iters"] == b["refined"]["iters"]
        for key in ("ln_theta_k", "ln_theta_next", "props"):                                        # the loop's own log vectors
            assert numpy.array_equal(a["refined"][key].view(numpy.int64), b["refined"][key].view(numpy.int64)), key
        assert numpy.array_equal(a["row_label"], b["row_label"])
    for a, b in zip(last_of[5], again[5]):                # two runs of the same batch
        assert a["refined"]["iters"] == b["refined"]["iters"]
        for key in ("ln_theta_k", "ln_theta_next"):
            assert numpy.array_equal(a["refined"][key].view(numpy.int64), b["refined"][key].view(numpy.int64)), key
        assert numpy.array_equal(a["row_label"], b["row_label"])
    assert numpy.array_equal(last_of[1], again[1]) and numpy.array_equal(last_of[2].view(numpy.int64), again[2].view(numpy.int64))


# ---- small shapes against the per-sample route ---------------------------------------------------------------------
def _few_values(rng, rows, n_haps, n_vals):
    """A matrix whose rows hold at most n_vals distinct values (so that they code)."""
    vals = rng.normal(-25.0, 8.0, size=(rows, n_vals))
    return numpy.take_along_axis(vals, rng.integers(0, n_vals, size=(rows, n_haps)), axis=1)


def _records_of(mats):
    """Dense matrices back to back as ONE records matrix; returns (cm, row0)."""
    import torch
    from mixemt_amd import em, preprocess
    n_rows, n_haps = sum(len(m) for m in mats), mats[0].shape[1]
    plan = em.EmPlan(torch.from_numpy(numpy.concatenate(mats)).cuda(), numpy.ones(n_rows), storage="coded", keep_log_matrix=False)
    rec, rec_off, ndist = plan._coded_keep[:3]
    assert plan.coded_rest == 0
    cm = preprocess.CodedMatrix(n_rows, n_haps, rec, rec_off, ndist, plan.rowmax, int(rec.numel()),
                                torch.zeros(0, dtype=torch.int64, device=rec.device),
                                torch.zeros((0, n_haps), dtype=torch.float64, device=rec.device))
    cm._plan = plan                                       # (keeps the buffers alive)
    return cm, numpy.concatenate([[0], numpy.cumsum([len(m) for m in mats])])


def _per_sample(cm, wts, res, haps, args, init):
    """The existing per-sample route: get_contributors_records -> reduce_em_records -> run_em_ex -> _assign_rows."""
    from mixemt_amd import assign, em, preprocess
    contribs = assign.get_contributors_records(None, None, haps, wts, res["props"], cm, res["ln_theta_k"], args)
    order, votes = assign.vote_table_from_records(cm, res["ln_theta_k"], None)
    if not contribs:
        return {"contribs": [], "vote_order": order, "votes": votes}
    sub, names = preprocess.reduce_em_records(cm, haps, contribs)
    run = em.run_em_ex(sub, wts, args, inits=None if init is None else numpy.atleast_2d(init))
    contribs = assign.update_contribs(contribs, (run["props"], run["read_mix"]), names)
    table, assigned = assign._assign_rows(contribs, (run["props"], run["read_mix"]), names, cm.n_rows, args.min_fold)
    label = numpy.zeros(cm.n_rows, dtype=numpy.int32) if assigned is None else assigned.cpu().numpy()
    # the margin of every row, restated from assemble.py:284-334 on the per-sample posterior
    margin = numpy.full(cm.n_rows, numpy.inf)
    if len(contribs) > 1:
        with numpy.errstate(divide="ignore", invalid="ignore"):
            v = numpy.sort(run["read_mix"].cpu().numpy() - numpy.log(run["props"]), axis=1)
            margin = v[:, -1] - v[:, -2]
    return {"contribs": contribs, "vote_order": order, "votes": votes, "sub_haps": names, "run": run, "row_label": label,
            "margin": margin, "assigned": table}


def _same_as_per_sample(got, want, min_fold, what):
    assert [c[:2] for c in got["contribs"]] == [c[:2] for c in want["contribs"]], what
    assert [int(h) for h in got["vote_order"]] == [int(h) for h in want["vote_order"]], what
    assert numpy.array_equal(got["votes"], want["votes"]), what
    if not want["contribs"]:
        return
    assert got["sub_haps"] == want["sub_haps"], what
    assert got["refined"]["iters"] == want["run"]["iters"] and got["refined"]["done"] == want["run"]["done"], \
        (what, got["refined"]["iters"], want["run"]["iters"])
    err = numpy.abs(got["refined"]["props"] - want["run"]["props"]).max()
    assert err < PROPS_ATOL, (what, err)
    assert numpy.abs(numpy.array([c[2] for c in got["contribs"]]) - numpy.array([c[2] for c in want["contribs"]])).max() < PROPS_ATOL
    differ = numpy.flatnonzero(got["row_label"] != want["row_label"])
    near = numpy.abs(want["margin"][differ] - numpy.log(min_fold)) <= BAND
    assert near.all() and len(differ) <= 0.01 * len(want["row_label"]), (what, differ[:10], want["margin"][differ][:10])


@pytest.fixture(scope="module", params=[66, 128, 5408])
def small(request):
    """Samples of 1, 2, 63, 64, 65, 513 and 2 x tile + 1 rows in one batch (weights with 0 and > 1; at the width that has
    room for them, a sample with 16-bit-coded rows), and their first EM."""
    from mixemt_amd import _lib, em
    n_haps = request.param
    tile = _lib.load().mxm_samples_tile_rows()
    rng = numpy.random.default_rng(4100 + n_haps)
    sizes = [1, 2, 63, 64, 65, 513, 2 * tile + 1]
    mats = [_few_values(rng, rows, n_haps, 9) for rows in sizes]
    if n_haps >= 1024:
        wide = _few_values(rng, tile + 3, n_haps, 9)
        wide[0::2] = _few_values(rng, len(wide[0::2]), n_haps, 600)
        assert all(256 < len(numpy.unique(row)) <= 1024 for row in wide[0::2])
        mats.insert(3, wide)
    wts = [rng.integers(0, 5, size=len(m)).astype(numpy.float64) for m in mats]
    for w in wts:
        w[0] = max(w[0], 2.0)
    assert any((w == 0).any() for w in wts) and any((w > 1).any() for w in wts)
    cm, row0 = _records_of(mats)
    if n_haps >= 1024:
        nd = cm.ndist_host()[row0[3]:row0[4]]
        assert (nd[0::2] > 256).all()                     # the wide rows did get 16-bit codes
    samples = [(cm.rows(row0[i], row0[i + 1]), wts[i]) for i in range(len(mats))]
    inits = [rng.dirichlet([1.0] * n_haps)[None, :] for _ in mats]
    results = em.run_em_many(samples, em_args(max_iter=40), inits=inits)
    assert all(r["route"] == "batch" for r in results)
    haps = ["h%04d" % i for i in range(n_haps)]
    return {"samples": samples, "results": results, "haps": haps, "rng_seed": 77 + n_haps, "cm": cm, "row0": row0}


def test_votes_equal_the_per_sample_vote(small):
    """best, first-seen order and integer-weight votes: exactly those of mxm_row_argmax_votes_coded per sample."""
    import torch
    from mixemt_amd import assign
    samples, results = small["samples"], small["results"]
    low = assign._finish_batch(samples, [torch.from_numpy(w).cuda() for _, w in samples], list(range(len(samples))))
    best, votes, counts, first, lse, errors = low.votes(numpy.stack([r["ln_theta_k"][0] for r in results]), want_lse=True)
    best = best.cpu().numpy()
    assert not any(errors) and torch.isfinite(lse).all()
    for s, ((cm, w), res) in enumerate(zip(samples, results)):
        lo, hi = int(low.row0[s]), int(low.row0[s + 1])
        want_best, want_votes = assign.row_argmax_votes_records(cm, res["ln_theta_k"], w)
        assert numpy.array_equal(best[lo:hi], want_best)
        assert numpy.array_equal(votes[s], want_votes)                     # integer weights: exact in any order
        assert numpy.array_equal(counts[s], numpy.bincount(want_best, minlength=cm.n_haps))
        seen, where = numpy.unique(want_best, return_index=True)
        want_first = numpy.full(cm.n_haps, cm.n_rows)
        want_first[seen] = where
        assert numpy.array_equal(first[s], want_first)
        order, _ = assign.vote_table_from_records(cm, res["ln_theta_k"], None)
        mine = numpy.flatnonzero(first[s] < cm.n_rows)
        assert numpy.array_equal(mine[numpy.argsort(first[s][mine], kind="stable")], order)


@pytest.mark.parametrize("n_contribs", [1, 2, 3, 16])
def test_small_shapes_against_the_per_sample_route(small, n_contribs):
    from mixemt_amd import assign
    samples, results, haps = small["samples"], small["results"], small["haps"]
    rng = numpy.random.default_rng(small["rng_seed"] + n_contribs)
    cols = rng.choice(len(haps), size=n_contribs, replace=False)
    args = finish_args(contributors=",".join(haps[int(c)] for c in cols), max_iter=300)
    inits = [rng.dirichlet([1.0] * n_contribs) for _ in samples]
    got = assign.finish_many(samples, results, haps, args, refine_inits=inits)
    assert [r["route"] for r in got] == ["batch"] * len(samples)
    for s, ((cm, w), res) in enumerate(zip(samples, results)):
        want = _per_sample(cm, w, res, haps, args, inits[s])
        assert not (numpy.abs(want["margin"] - numpy.log(args.min_fold)) <= BAND).any()      # (the seed leaves the band empty)
        _same_as_per_sample(got[s], want, args.min_fold, "sample %d of %d rows, K = %d" % (s, cm.n_rows, n_contribs))
        print("rows %d K %d: iterations %s, assigned %s" % (cm.n_rows, n_contribs, got[s]["refined"]["iters"], got[s]["assigned"]))


def test_exactly_equal_columns_go_to_the_later_column_as_in_the_per_sample_route():
    """Two identical columns from equal inits stay identical to the bit, so every row is an exact tie; with min_fold = 1 the
    tie decides the label: the later (larger haplogroup) column wins in assign_reads_kernel, and so it must here, through
    perm, whichever order the contributors are named in."""
    from mixemt_amd import assign, em
    rng = numpy.random.default_rng(31)
    n_haps = 128
    mats = [_few_values(rng, rows, n_haps, 7) for rows in (40, 70)]
    for m in mats:
        m[:, 90] = m[:, 12]
    wts = [rng.integers(1, 4, size=len(m)).astype(numpy.float64) for m in mats]
    cm, row0 = _records_of(mats)
    samples = [(cm.rows(row0[i], row0[i + 1]), wts[i]) for i in range(2)]
    results = em.run_em_many(samples, em_args(max_iter=20), inits=[rng.dirichlet([1.0] * n_haps)[None, :] for _ in mats])
    haps = ["h%04d" % i for i in range(n_haps)]
    for named in ("h0012,h0090", "h0090,h0012"):
        args = finish_args(contributors=named, min_fold=1.0, max_iter=50)
        inits = [numpy.array([0.5, 0.5])] * 2
        got = assign.finish_many(samples, results, haps, args, refine_inits=inits)
        for s, (view, w) in enumerate(samples):
            want = _per_sample(view, w, results[s], haps, args, inits[s])
            assert (want["margin"] == 0.0).all()                          # exact ties throughout
            later = [c[1] for c in want["contribs"]].index("h0090")
            assert (want["row_label"] == later).all()
            assert got[s]["route"] == "batch" and numpy.array_equal(got[s]["row_label"], want["row_label"]), (named, s)
            assert got[s]["refined"]["props"][0] == got[s]["refined"]["props"][1]


# ---- fall-backs and edges ------------------------------------------------------------------------------------------
def test_fall_backs_take_the_per_sample_route_with_the_same_result(small):
    from mixemt_amd import assign
    samples, results, haps = small["samples"], small["results"], small["haps"]
    rows = [cm.n_rows for cm, _ in samples]
    rng = numpy.random.default_rng(5)
    cols = rng.choice(len(haps), size=3, replace=False)
    args = finish_args(contributors=",".join(haps[int(c)] for c in cols), max_iter=300)
    inits = [rng.dirichlet([1.0] * 3) for _ in samples]
    batch = assign.finish_many(samples, results, haps, args, refine_inits=inits)
    capped = assign.finish_many(samples, results, haps, args, refine_inits=inits, max_rows=64)
    single = assign.finish_many(samples, results, haps, args, refine_inits=inits, max_rows=0)
    assert [r["route"] for r in capped] == ["batch" if n <= 64 else "single" for n in rows]
    assert capped[rows.index(64)]["route"] == "batch" and capped[rows.index(65)]["route"] == "single"
    assert [r["route"] for r in single] == ["single"] * len(samples)
    for s, (cm, w) in enumerate(samples):
        want = _per_sample(cm, w, results[s], haps, args, inits[s])
        for got in (batch[s], capped[s], single[s]):
            assert set(got) == set(batch[0])
            _same_as_per_sample(got, want, args.min_fold, "sample %d (%s)" % (s, got["route"]))
    # 17 contributors: the per-sample route, the same keys
    cols17 = rng.choice(len(haps), size=17, replace=False)
    args17 = finish_args(contributors=",".join(haps[int(c)] for c in cols17), max_iter=300)
    inits17 = [rng.dirichlet([1.0] * 17) for _ in samples]
    got = assign.finish_many(samples[2:4], results[2:4], haps, args17, refine_inits=inits17[2:4])
    assert [r["route"] for r in got] == ["single", "single"] and set(got[0]) == set(batch[0])
    for j, s in enumerate((2, 3)):
        _same_as_per_sample(got[j], _per_sample(samples[s][0], samples[s][1], results[s], haps, args17, inits17[s]),
                            args17.min_fold, "17 contributors")
    # max_iter: done == 2 on exactly that iteration
    short = assign.finish_many(samples, results, haps, finish_args(contributors=args.contributors, max_iter=7), refine_inits=inits)
    for s, r in enumerate(short):
        want = _per_sample(samples[s][0], samples[s][1], results[s], haps, finish_args(contributors=args.contributors, max_iter=7),
                           inits[s])
        assert r["refined"]["iters"] == want["run"]["iters"] and r["refined"]["done"] == want["run"]["done"]
    assert any(r["refined"]["done"] == [2] and r["refined"]["iters"] == [7] for r in short)


def test_several_runs_stay_with_the_per_sample_route(small):
    from mixemt_amd import assign, em
    samples, haps = small["samples"][1:4], small["haps"]
    numpy.random.seed(21)
    results = em.run_em_many(samples, em_args(max_iter=20, n_multi=2))
    numpy.random.seed(22)
    got = assign.finish_many(samples, results, haps, finish_args(contributors="%s,%s" % (haps[3], haps[40]), n_multi=2, max_iter=50))
    assert [r["route"] for r in got] == ["single"] * 3
    assert all(r["refined"]["inits"].shape == (2, 2) and len(r["refined"]["iters"]) == 2 for r in got)


def test_a_sample_without_contributors_beside_a_normal_one(pins):
    from mixemt_amd import assign, em
    haps, g4 = pins["haps"], pins["g4"]
    few = (pins["cm"].rows(0, 5), numpy.ones(5))          # total weight 5 < min_reads
    res_few = em.run_em_many([few], em_args(max_iter=30), inits=[g4["inits"]])[0]
    numpy.random.seed(13)
    got = assign.finish_many([few, pins["samples"][0]], [res_few, pins["results"][0]], haps, finish_args())
    assert got[0]["contribs"] == [] and got[0]["refined"] is None and got[0]["route"] == "batch"
    assert len(got[0]["assigned"]) == 0 and got[0]["row_label"].shape == (0,) and len(got[0]["vote_order"]) >= 1
    numpy.random.seed(13)
    alone = assign.finish_many(pins["samples"][:1], pins["results"][:1], haps, finish_args())[0]
    assert len(got[1]["contribs"]) == 3 and got[1]["contribs"] == alone["contribs"]
    assert numpy.array_equal(got[1]["row_label"], alone["row_label"])
    assert numpy.array_equal(got[1]["refined"]["inits"], alone["refined"]["inits"])          # the empty sample drew nothing


def test_a_row_without_a_record_poisons_its_own_sample_only(small):
    import torch
    from mixemt_amd import assign, em
    samples, results, haps = small["samples"][2:5], small["results"][2:5], small["haps"]
    wts_d = [torch.from_numpy(w).cuda() for _, w in samples]
    ln_props = numpy.stack([r["ln_theta_k"][0] for r in results])
    good = assign._finish_batch(samples, wts_d, [0, 1, 2])
    best, votes, counts, first, _, errors = good.votes(ln_props)
    assert errors == [False, False, False]
    ndist = good.ndist.clone()
    ndist[int(good.row0[1]) + 7] = 0                      # forged in a copy: the row is never dereferenced
    bad = em.SampleFinish(good.rec, good.rec_off, ndist, good.wts, good.rowmax, good.row0, good.n_haps)
    best2, votes2, counts2, first2, _, errors2 = bad.votes(ln_props)
    assert errors2 == [False, True, False] and numpy.isnan(votes2[1]).all()
    assert int(best2[int(good.row0[1]) + 7]) == -1
    for s in (0, 2):
        lo, hi = int(good.row0[s]), int(good.row0[s + 1])
        assert numpy.array_equal(best2[lo:hi].cpu().numpy(), best[lo:hi].cpu().numpy())
        assert numpy.array_equal(votes2[s].view(numpy.int64), votes[s].view(numpy.int64))
        assert numpy.array_equal(first2[s], first[s]) and numpy.array_equal(counts2[s], counts[s])
    # finish_many raises that sample's error
    from mixemt_amd import preprocess
    cm1 = samples[1][0]
    forged = preprocess.CodedMatrix(cm1.n_rows, cm1.n_haps, cm1.rec, cm1.rec_off, ndist[int(good.row0[1]):int(good.row0[2])],
                                    cm1.rowmax, cm1.used, cm1.rest_rows, cm1.m_rest)
    with pytest.raises(ValueError, match="sample 1 has a row without a record"):
        assign.finish_many([samples[0], (forged, samples[1][1]), samples[2]], results, haps,
                           finish_args(contributors="%s,%s" % (haps[1], haps[2])))


def test_refused_calls_launch_nothing_and_good_ones_run(small):
    """(the messages of every refusal: tests/test_samples_finish_host.py)"""
    import torch
    from mixemt_amd import assign
    from mixemt_amd._dev import current_stream
    samples, results = small["samples"][2:4], small["results"][2:4]
    low = assign._finish_batch(samples, [torch.from_numpy(w).cuda() for _, w in samples], [0, 1])
    lib, n_haps = low.lib, low.n_haps
    cols = numpy.array([[1, 5, 0, 0], [2, 3, 9, 0]], dtype=numpy.int32)
    ncol = numpy.array([2, 3], dtype=numpy.int32)
    out = torch.full((low.n_rows, 4), -7.0, dtype=torch.float64, device=low.dev)

    def gather(row0, ld, cols, ncol):
        row0 = numpy.ascontiguousarray(row0, dtype=numpy.int64)
        return lib.mxm_gather_columns_samples(ctypes.byref(low.coded), row0.ctypes.data_as(ctypes.c_void_p), len(row0) - 1, n_haps,
                                              cols.ctypes.data_as(ctypes.c_void_p), ncol.ctypes.data_as(ctypes.c_void_p), ld,
                                              out.data_ptr(), low.ws.data_ptr(), low.ws_bytes, current_stream())
    good_row0 = list(low.row0)
    assert gather([0, 70, 60, low.n_rows], 4, numpy.zeros((3, 4), dtype=numpy.int32), numpy.ones(3, dtype=numpy.int32)) == -1
    assert gather(good_row0[:-1] + [low.n_rows - 1], 4, cols, ncol) == -1
    assert gather(good_row0, 5, cols, ncol) == -1
    assert gather(good_row0, 4, cols, numpy.array([2, 5], dtype=numpy.int32)) == -1
    bad_cols = cols.copy()
    bad_cols[1, 2] = n_haps
    assert gather(good_row0, 4, bad_cols, ncol) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()                            # nothing ran
    assert gather(good_row0, 4, cols, ncol) == 0
    torch.cuda.synchronize()
    dense = torch.cat([cm.dense() for cm, _ in samples]).cpu().numpy()
    got = out.cpu().numpy()
    for s in range(2):
        lo, hi = good_row0[s], good_row0[s + 1]
        k = int(ncol[s])
        assert numpy.array_equal(got[lo:hi, :k], dense[lo:hi][:, cols[s, :k]]) and numpy.isneginf(got[lo:hi, k:]).all()
