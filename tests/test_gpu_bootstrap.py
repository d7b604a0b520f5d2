"""
Bootstrap intervals for the refined proportions (include/mixemt_hip_bootstrap.h; assign.bootstrap_many) on the device:
  weights   mxm_bootstrap_weights bit for bit against the draw rule restated in tests/_bootstrap_ref.py, in ragged batches
            with ids of the samples' own, on both sides of MXM_BOOTSTRAP_LDS_ROWS;
  loop      every replicate of mxm_em_loop_samples_narrow_boot bit for bit against mxm_em_loop_samples_narrow on that
            sample alone under the replicate's weights;
  summary   mxm_bootstrap_summary against the restated quantile formula, numpy.quantile, math.fsum and numpy.exp;
  end to end   the golden samples of tests/test_gpu_samples_finish.py through run_em_many -> finish_many -> bootstrap_many.
The weights and the loop read no record, so their tests hand em.SampleFinish a record buffer of zeros.
"""
import ctypes
import io
import math

import numpy
import pytest

import _bootstrap_ref as ref
from conftest import em_args, golden
from test_samples_finish_host import finish_args

pytestmark = pytest.mark.gpu

LDS_ROWS = 8192                 # MXM_BOOTSTRAP_LDS_ROWS (tests/test_bootstrap_host.py holds the header to it)
SEED = 20261020


def _finish(weights, n_haps=66):
    """em.SampleFinish over samples given by their weight vectors alone (no entry under test reads a record)."""
    import torch
    from mixemt_amd import em
    row0 = numpy.concatenate([[0], numpy.cumsum([len(w) for w in weights])]).astype(numpy.int64)
    n_rows = int(row0[-1])
    wts = torch.from_numpy(numpy.concatenate([numpy.asarray(w, dtype=numpy.float64) for w in weights])).cuda()
    return em.SampleFinish(torch.zeros(64, dtype=torch.uint8, device="cuda"), torch.zeros(n_rows, dtype=torch.int64, device="cuda"),
                           torch.ones(n_rows, dtype=torch.int32, device="cuda"), wts, None, row0, n_haps)


def _slices(fin, wb, n_boot):
    """wb -> one [B][R_s] numpy array per sample."""
    host = wb.cpu().numpy()
    return [host[n_boot * int(lo):n_boot * int(hi)].reshape(n_boot, int(hi - lo)) for lo, hi in zip(fin.row0[:-1], fin.row0[1:])]


def _same_bits(a, b):
    a, b = numpy.ascontiguousarray(a, dtype=numpy.float64), numpy.ascontiguousarray(b, dtype=numpy.float64)
    return a.shape == b.shape and numpy.array_equal(a.view(numpy.int64), b.view(numpy.int64))


# ---- weights ---------------------------------------------------------------------------------------------------------
def _weight_cases():
    rng = numpy.random.default_rng(5)
    one_draw = numpy.zeros(257)
    one_draw[200] = 1
    five = numpy.zeros(257)
    five[[3, 100, 256]] = (2, 2, 1)
    ends = rng.integers(0, 4, size=257).astype(numpy.float64)
    ends[:5], ends[-7:], ends[130] = 0, 0, 0
    return {"one row": numpy.array([7.0]), "(1, 2^20)": numpy.array([1.0, 2.0 ** 20]), "N = 1": one_draw, "N = 5": five,
            "zero ends": ends, "at the limit": rng.integers(0, 3, size=LDS_ROWS).astype(numpy.float64),
            "one past the limit": rng.integers(0, 3, size=LDS_ROWS + 1).astype(numpy.float64)}


BATCHES = [(("one row", "(1, 2^20)", "N = 1"), (4000000000, 0, 17)),
           (("N = 5", "at the limit", "zero ends"), (3, 2 ** 32 - 1, 9)),
           (("one past the limit", "one row", "N = 5"), (70000, 5, 6))]


@pytest.mark.parametrize("names,ids", BATCHES, ids=["small", "limit", "past"])
def test_weights_equal_the_restated_draw_rule_bit_for_bit(names, ids):
    cases = _weight_cases()
    n_boot = 4
    fin = _finish([cases[n] for n in names])
    wb, errors = fin.boot_weights(n_boot, SEED, ids)
    assert errors == [0, 0, 0]
    for name, s_id, got in zip(names, ids, _slices(fin, wb, n_boot)):
        w = cases[name]
        want = ref.resample_all(w, SEED, s_id, n_boot)
        assert (got.sum(axis=1) == w.sum()).all(), name                     # every replicate's counts sum to N_s exactly
        assert not got[:, w == 0].any(), name
        assert _same_bits(got, want), name
    if "(1, 2^20)" in names:                                                # (the replicates are not all alike: rows were drawn)
        assert len({tuple(r) for r in _slices(fin, wb, n_boot)[1]}) > 1


def test_a_sample_keeps_its_draws_alone_last_in_a_batch_and_under_another_b():
    cases = _weight_cases()
    me = cases["zero ends"]
    alone = _finish([me])
    wb, _ = alone.boot_weights(8, SEED, [77])
    first = _slices(alone, wb, 8)[0]
    assert _same_bits(first, ref.resample_all(me, SEED, 77, 8))
    batch = _finish([cases["N = 5"], cases["one past the limit"], me])
    wb, _ = batch.boot_weights(64, SEED, [1, 2, 77])
    last = _slices(batch, wb, 64)[2]
    assert _same_bits(last[:8], first)
    assert len({tuple(r) for r in last}) == 64                              # 64 different replicates
    wb, _ = alone.boot_weights(8, SEED + 1, [77])
    assert not _same_bits(_slices(alone, wb, 8)[0], first)                  # the seed is in the key
    wb, _ = alone.boot_weights(8, SEED, [78])
    assert not _same_bits(_slices(alone, wb, 8)[0], first)                  # the id is in the counter


@pytest.mark.parametrize("n_boot", [65, 130])
def test_global_counters_in_a_later_chunk_of_replicates(n_boot):
    """A sample beyond MXM_BOOTSTRAP_LDS_ROWS draws its replicates in launches of BOOT_CHUNK = 64 (bootstrap_kernels.hpp),
    from the second launch on with b0 > 0: 65 replicates = a second launch of one, 130 = two full launches and one of two.
    The batch holds a sample one past the limit, one at it and a small one; every replicate of every sample bit for bit."""
    cases = _weight_cases()
    names, ids = ("one past the limit", "at the limit", "zero ends"), (70000, 2 ** 32 - 1, 9)
    assert [len(cases[n]) for n in names] == [LDS_ROWS + 1, LDS_ROWS, 257]
    fin = _finish([cases[n] for n in names])
    wb, errors = fin.boot_weights(n_boot, SEED, ids)
    assert errors == [0, 0, 0]
    got_all = _slices(fin, wb, n_boot)
    wb64, errors = fin.boot_weights(64, SEED, ids)
    assert errors == [0, 0, 0]
    for name, s_id, got, first in zip(names, ids, got_all, _slices(fin, wb64, 64)):
        w = cases[name]
        assert got.shape == (n_boot, len(w))
        assert (got.sum(axis=1) == w.sum()).all(), name                     # every replicate's counts sum to N_s exactly
        assert not got[:, w == 0].any(), name
        assert _same_bits(got, ref.resample_all(w, SEED, s_id, n_boot)), name
        assert _same_bits(got[:64], first), name                            # the first chunk is the B = 64 call's
        assert len({tuple(r) for r in got}) == n_boot, name                 # no replicate of a later chunk repeats an earlier one


def test_a_refused_sample_is_flagged_and_leaves_its_neighbours_intact():
    cases = _weight_cases()
    for bad, code in ((numpy.array([1.0, 2.5, 3.0]), 1), (numpy.array([1.0, -2.0, 3.0]), 1), (numpy.array([1.0, numpy.nan]), 1),
                      (numpy.zeros(4), 2), (numpy.full(3, 2.0 ** 30), 2), (numpy.array([1.0, 2.0 ** 40]), 2)):
        fin = _finish([cases["N = 5"], bad, cases["zero ends"]])
        wb, errors = fin.boot_weights(3, SEED, [4, 5, 6])
        got = _slices(fin, wb, 3)
        assert errors == [0, code, 0], bad
        assert numpy.isnan(got[1]).all(), bad
        assert _same_bits(got[0], ref.resample_all(cases["N = 5"], SEED, 4, 3)), bad
        assert _same_bits(got[2], ref.resample_all(cases["zero ends"], SEED, 6, 3)), bad


# ---- loop ------------------------------------------------------------------------------------------------------------
def _loop_batch(ld):
    """S = 3 samples at stride ld: one column; 600 x 3 (linearised in LDS); 9600 cells > 9216, so through E -- 1200 x 8, or
    2400 x 4 at ld = 4, which has no eighth column.  -> (weights, ncol, reduced matrix [R][ld] with -inf pad columns)."""
    rng = numpy.random.default_rng(40 + ld)
    shapes = [(300, 1), (600, 3), (2400, 4) if ld == 4 else (1200, 8)]
    weights = [rng.integers(0, 4, size=r).astype(numpy.float64) for r, _ in shapes]
    mat = numpy.full((sum(r for r, _ in shapes), ld), -numpy.inf)
    at = 0
    for r, k in shapes:
        # weakly informative rows: the loop takes 24 .. 51 iterations to 1e-9 (restated in numpy), several launches of 16
        mat[at:at + r, :k] = rng.normal(-30.0, 1.0, size=(r, k)) + 4.0 * (rng.random((r, k)) < 0.4)
        at += r
    return weights, numpy.array([k for _, k in shapes], dtype=numpy.int32), mat


def _one_run(lib, mat_s, ld, k, w, start, tol, max_iter, check_every):
    """mxm_em_loop_samples_narrow on ONE sample under the weights w, called directly: every table it leaves."""
    import torch
    from mixemt_amd import _lib, em
    fin = _finish([w])
    p0 = numpy.zeros((1, ld))
    p0[0, :k] = start
    ln0, p0 = em.log_inits(p0)
    props, ln_cur = torch.from_numpy(p0).cuda(), torch.from_numpy(ln0).cuda()
    ln_new, state = ln_cur.clone(), em.new_state(1, "cuda")
    lin = torch.empty((len(w), ld), dtype=torch.float64, device="cuda")
    host = (_lib.EmState * 1)()
    ncol = numpy.array([k], dtype=numpy.int32)
    dev = torch.from_numpy(numpy.ascontiguousarray(mat_s)).cuda()
    rc = lib.mxm_em_loop_samples_narrow(ctypes.byref(fin.coded), fin.row0_ptr, 1, fin.n_haps, dev.data_ptr(), ld, ncol.ctypes.data,
                                        fin.wts.data_ptr(), props.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(), state.data_ptr(),
                                        tol, max_iter, check_every, lin.data_ptr(), fin.ws.data_ptr(), fin.ws_bytes,
                                        torch.cuda.current_stream().cuda_stream, host)
    assert rc == 0, lib.mxm_last_error()
    return {"ln_cur": ln_cur.cpu().numpy()[0], "ln_new": ln_new.cpu().numpy()[0], "props_cur": props.cpu().numpy()[0],
            "state": (host[0].done, host[0].iters, host[0].l1)}


@pytest.fixture(scope="module")
def loops():
    """Per ld, made once: the batch, its replicates' weights and the batched loop's tables at check_every = 16."""
    import torch
    made = {}

    def get(ld):
        if ld not in made:
            weights, ncol, mat = _loop_batch(ld)
            fin = _finish(weights)
            n_boot = 5
            wb, errors = fin.boot_weights(n_boot, SEED, [11, 12, 13])
            assert errors == [0, 0, 0]
            starts = [numpy.random.default_rng(ld + s).dirichlet([2.0] * int(k)) for s, k in enumerate(ncol)]
            mat_d = torch.from_numpy(mat).cuda()
            tables = fin.em_loop_boot(mat_d, ld, ncol, wb, n_boot, starts, 1e-9, 300, check_every=16)
            made[ld] = (fin, mat, mat_d, ncol, wb, n_boot, starts, tables)
        return made[ld]
    return get


@pytest.mark.parametrize("ld", [4, 8, 16])
def test_every_replicate_equals_the_one_run_loop_on_that_sample_alone(loops, ld):
    fin, mat, mat_d, ncol, wb, n_boot, starts, (ln_cur, ln_new, props_cur, _, states) = loops(ld)
    got = {"ln_cur": ln_cur.cpu().numpy(), "ln_new": ln_new.cpu().numpy(), "props_cur": props_cur.cpu().numpy()}
    slices = _slices(fin, wb, n_boot)
    iters = set()
    for s in range(3):
        lo, hi, k = int(fin.row0[s]), int(fin.row0[s + 1]), int(ncol[s])
        for b in range(n_boot):
            want = _one_run(fin.lib, mat[lo:hi], ld, k, slices[s][b], starts[s], 1e-9, 300, 16)
            for key in got:
                assert _same_bits(got[key][s * n_boot + b, :k], want[key][:k]), (ld, s, b, key)
            done, n_iter, l1 = states[s][b]
            assert (done, n_iter) == want["state"][:2] and _same_bits([l1], [want["state"][2]]), (ld, s, b)
            assert done == 1 and (n_iter == 1 if k == 1 else 16 < n_iter < 300), (ld, s, b, done, n_iter)
            iters.add((s, n_iter))
    print("ld", ld, "iterations per (sample, count):", sorted(iters))
    assert len({n for s, n in iters if s > 0}) > 1                        # the replicates do not all stop together


@pytest.mark.parametrize("ld", [4, 8, 16])
def test_check_every_changes_no_bit_and_max_iter_stops_with_done_2(loops, ld):
    fin, mat, mat_d, ncol, wb, n_boot, starts, (ln_cur, ln_new, props_cur, _, states) = loops(ld)
    one = fin.em_loop_boot(mat_d, ld, ncol, wb, n_boot, starts, 1e-9, 300, check_every=1)
    for a, b in zip((ln_cur, ln_new, props_cur), one[:3]):
        assert _same_bits(a.cpu().numpy(), b.cpu().numpy()), ld
    assert [[st[:2] for st in sample] for sample in one[4]] == [[st[:2] for st in sample] for sample in states]
    short = fin.em_loop_boot(mat_d, ld, ncol, wb, n_boot, starts, 0.0, 2, check_every=16)
    assert all(st[:2] == (2, 2) for sample in short[4][1:] for st in sample), short[4]
    # (one column: the first step already moves nothing, but 0 < 0.0 is false, so it too runs into max_iter)
    assert all(st[:2] == (2, 2) for st in short[4][0]), short[4][0]


def test_the_loop_refuses_a_large_sample_without_e_and_launches_nothing(loops):
    import torch
    from mixemt_amd import _lib, em
    fin, mat, mat_d, ncol, wb, n_boot, starts, _ = loops(8)
    ws_bytes = fin._boot_ws(n_boot, 8)
    tabs = [torch.full((3 * n_boot, 8), 0.25, dtype=torch.float64, device="cuda") for _ in range(3)]
    state = em.new_state(3 * n_boot, "cuda")
    host = (_lib.EmState * (3 * n_boot))()
    rc = fin.lib.mxm_em_loop_samples_narrow_boot(ctypes.byref(fin.coded), fin.row0_ptr, 3, fin.n_haps, n_boot, mat_d.data_ptr(), 8,
                                                 ncol.ctypes.data, wb.data_ptr(), tabs[0].data_ptr(), tabs[1].data_ptr(),
                                                 tabs[2].data_ptr(), state.data_ptr(), 1e-9, 300, 16, None, fin.ws.data_ptr(), ws_bytes,
                                                 torch.cuda.current_stream().cuda_stream, host)
    assert rc == -1 and b"more than 9216 cells needs the global copy E" in fin.lib.mxm_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == 0.25).all()) for t in tabs) and not bool(state.any())


# ---- summary ---------------------------------------------------------------------------------------------------------
def _summary_inputs(n_boot, ld=4):
    """S = 2 samples of 3 and 1 columns: log proportions of B replicates each, every replicate done."""
    import torch
    rng = numpy.random.default_rng(n_boot)
    ncol = numpy.array([3, 1], dtype=numpy.int32)
    ln_new = numpy.full((2, n_boot, ld), -numpy.inf)
    ln_new[0, :, :3] = numpy.log(rng.dirichlet([5.0, 2.0, 0.3], size=n_boot))
    ln_new[1, :, 0] = numpy.log(rng.random(n_boot))
    raw = numpy.zeros((2 * n_boot, 6), dtype=numpy.int32)
    raw[:, 0] = 1                                                          # done = 1
    return ncol, ln_new, raw, torch


def _summary(fin, n_boot, ld, ncol, ln_new, raw, q_lo=0.025, q_hi=0.975):
    import torch
    state = torch.from_numpy(raw.reshape(-1).view(numpy.int64).copy()).cuda()
    return fin.boot_summary(n_boot, ld, ncol, torch.from_numpy(ln_new.reshape(2 * n_boot, ld)).cuda(), state, q_lo, q_hi)


@pytest.mark.parametrize("n_boot", [2, 3, 64, 1000, 4096])
def test_summary_against_the_restated_formula_numpy_and_fsum(n_boot):
    ld = 4
    ncol, ln_new, raw, _ = _summary_inputs(n_boot, ld)
    fin = _finish([numpy.ones(3), numpy.ones(2)])
    for q_lo, q_hi in ((0.025, 0.975), (0.0, 1.0), (0.5, 0.05)):
        x, lo, hi, mean, sd, flag = _summary(fin, n_boot, ld, ncol, ln_new, raw, q_lo, q_hi)
        assert flag.tolist() == [0, 0]
        for s in range(2):
            k = int(ncol[s])
            want_x = numpy.exp(ln_new[s, :, :k])
            assert (numpy.abs(x[s, :, :k] - want_x) <= 2 * numpy.spacing(want_x)).all(), (n_boot, s)      # 1 ulp each: ocml, numpy
            assert not x[s, :, k:].any() and numpy.isnan(lo[s, k:]).all()                                  # pad columns: untouched
            for c in range(k):
                col = numpy.sort(x[s, :, c])
                for got, q in ((lo[s, c], q_lo), (hi[s, c], q_hi)):
                    assert got == ref.quantile(col, q), (n_boot, s, c, q)                                  # the header's formula, exactly
                    want = numpy.quantile(x[s, :, c], q, method="linear")
                    assert abs(got - want) <= 2 * numpy.spacing(want), (n_boot, s, c, q)
                # values in [0, 1]: B additions of at most 2^-53 * B each, over B -- the bound holds for any order of summation
                bound = 4 * n_boot * 2.0 ** -53
                exact = math.fsum(x[s, :, c]) / n_boot
                assert abs(mean[s, c] - exact) <= bound, (n_boot, s, c, mean[s, c] - exact)
                want_sd = math.sqrt(math.fsum((x[s, :, c] - exact) ** 2) / (n_boot - 1))
                assert abs(sd[s, c] - want_sd) <= bound, (n_boot, s, c, sd[s, c] - want_sd)
                assert abs(sd[s, c] - numpy.std(x[s, :, c], ddof=1)) <= bound


def test_a_replicate_that_is_not_usable_poisons_its_column_only():
    n_boot, ld = 64, 4
    ncol, ln_new, raw, _ = _summary_inputs(n_boot, ld)
    fin = _finish([numpy.ones(3), numpy.ones(2)])
    clean = _summary(fin, n_boot, ld, ncol, ln_new, raw)
    bad = ln_new.copy()
    bad[0, 5, 1] = numpy.nan
    x, lo, hi, mean, sd, flag = _summary(fin, n_boot, ld, ncol, bad, raw)
    assert flag.tolist() == [1, 0]
    for table, want in zip((lo, hi, mean, sd), clean[1:5]):
        assert numpy.isnan(table[0, 1]) and _same_bits(table[0, [0, 2]], want[0, [0, 2]]) and _same_bits(table[1, :1], want[1, :1])
    assert numpy.isnan(x[0, 5, 1]) and _same_bits(numpy.delete(x[0, :, 1], 5), numpy.delete(clean[0][0, :, 1], 5))
    inf = ln_new.copy()
    inf[1, 63, 0] = numpy.inf                                               # not finite either
    assert _summary(fin, n_boot, ld, ncol, inf, raw)[5].tolist() == [0, 1]
    # a replicate that is not done, or whose state carries an error: every column of its sample
    for field in (0, 5):
        marked = raw.copy()
        marked[n_boot + 7, field] = 0 if field == 0 else 1
        x, lo, hi, mean, sd, flag = _summary(fin, n_boot, ld, ncol, ln_new, marked)
        assert flag.tolist() == [0, 1] and numpy.isnan([lo[1, 0], hi[1, 0], mean[1, 0], sd[1, 0]]).all()
        assert _same_bits(lo[0, :3], clean[1][0, :3]) and _same_bits(x[:, :, :], clean[0])


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cohort(b17):
    """g4's 600 rows and g9's 2400 rows as ONE records matrix, their first EM and their refined second half (made once)."""
    from mixemt_amd import assign, em, preprocess
    refseq, phy, haps, tables = b17
    g4, g9 = golden("g4_run_em"), golden("g9_run_em_2400")
    cm, row0 = preprocess.build_em_records_many(tables, [(g["row_ptr"], g["site"], g["obs"]) for g in (g4, g9)])
    samples = [(cm.rows(0, 600), g4["wts"]), (cm.rows(600, 3000), g9["wts"])]
    results = em.run_em_many(samples, em_args(), inits=[g4["inits"], g9["inits"]])
    numpy.random.seed(8)
    finished = assign.finish_many(samples, results, haps, finish_args())
    assert [f["route"] for f in finished] == ["batch", "batch"] and all(f["refined"] is not None for f in finished)
    return {"cm": cm, "samples": samples, "results": results, "finished": finished, "haps": haps, "g4": g4}


def test_golden_samples_end_to_end(cohort):
    """The g8 sample (g4's rows refined over its contributors) beside g9's 2400 rows."""
    from mixemt_amd import assign, stats
    samples, finished, haps = cohort["samples"], cohort["finished"], cohort["haps"]
    args = finish_args()
    boots, skipped = assign.bootstrap_many(samples, finished, haps, args, n_boot=200, seed=3)
    assert skipped == [] and all(b is not None for b in boots)
    for s, (boot, fin) in enumerate(zip(boots, finished)):
        k = len(fin["contribs"])
        assert boot["columns"] == fin["sub_haps"] and boot["props_boot"].shape == (200, k)
        assert boot["iters"].shape == (200,) and (boot["done"] == 1).all()
        assert (boot["seed"], boot["level"], boot["n_boot"]) == (3, 0.95, 200)
        assert numpy.abs(boot["props_boot"].sum(axis=1) - 1.0).max() < 1e-12
        assert (boot["lo"] <= boot["hi"]).all()
        assert [row[:3] for row in boot["intervals"]] == fin["contribs"]
        for row in boot["intervals"]:
            c = boot["columns"].index(row[1])
            assert row[3:] == [boot["lo"][c], boot["hi"][c], boot["sd"][c]]
            print("sample", s, row)
            if k > 1:                                                       # resampled reads: the replicates differ
                assert row[3] < row[4] and row[5] > 0
            if s == 0:
                # the golden g4 sample (1198 reads, three contributors): each point estimate lies inside the 95 % percentile
                # interval of 200 resamples of its own reads warm-started at it -- which also ties every interval to ITS
                # contributor: in another column order 0.52 / 0.43 / 0.05 would not sit in one another's intervals
                assert row[3] <= row[2] <= row[4], row
        for c in range(k):
            col = numpy.sort(boot["props_boot"][:, c])
            # (the documented quantiles: (1 - level) / 2 is not the double 0.025)
            assert boot["lo"][c] == ref.quantile(col, (1.0 - 0.95) / 2.0) and boot["hi"][c] == ref.quantile(col, (1.0 + 0.95) / 2.0)
    # the same seed: the same result; another seed: other replicates; the one-sample form: the same call on a list of one
    again, _ = assign.bootstrap_many(samples, finished, haps, args, n_boot=200, seed=3)
    other, _ = assign.bootstrap_many(samples, finished, haps, args, n_boot=200, seed=4)
    for s in range(2):
        assert _same_bits(again[s]["props_boot"], boots[s]["props_boot"]) and _same_bits(again[s]["lo"], boots[s]["lo"])
        if len(finished[s]["contribs"]) > 1:
            assert not _same_bits(other[s]["props_boot"], boots[s]["props_boot"])
    one, why = assign.bootstrap(samples[1][0], samples[1][1], finished[1], haps, args, n_boot=200, seed=3, sample_ids=[1])
    assert why is None and _same_bits(one["props_boot"], boots[1]["props_boot"])         # (its id, not its place, is in the counter)
    # a sample without `refined` beside one with: skipped with a reason, reported with NA
    plain = assign.finish_many(samples, cohort["results"], haps, finish_args(refine_ests=False))
    mixed, skipped = assign.bootstrap_many(samples, [finished[0], plain[1]], haps, args, n_boot=200, seed=3)
    assert mixed[1] is None and [s for s, _ in skipped] == [1] and "no refined result" in skipped[0][1]
    assert _same_bits(mixed[0]["props_boot"], boots[0]["props_boot"])
    out = io.StringIO()
    stats.report_intervals_many(out, [finished[0], plain[1]], mixed, titles=["g4", "g9"])
    want = "# g4\n" + "".join("%s\t%s\t%.4f\t%.4f\t%.4f\t%.4f\n" % tuple(row) for row in mixed[0]["intervals"])
    want += "# g9\n" + "".join("%s\t%s\t%.4f\tNA\tNA\tNA\n" % tuple(con) for con in plain[1]["contribs"])
    assert out.getvalue() == want and out.getvalue().count("\n") == 2 + len(finished[0]["contribs"]) + len(plain[1]["contribs"])


def test_one_contributor_and_one_row(cohort):
    from mixemt_amd import assign
    samples, results, haps, g14 = cohort["samples"], cohort["results"], cohort["haps"], golden("g14_single_contributor")
    # g14: the unmixed sample -- one contributor, refined on 600 x 1
    numpy.random.seed(13)
    name = haps[int(g14["col"][0])]
    done = assign.finish_many(samples[:1], results[:1], haps, finish_args(contributors=name))
    boot, why = assign.bootstrap(samples[0][0], samples[0][1], done[0], haps, finish_args(), n_boot=64, seed=1)
    assert why is None and boot["lo"].tolist() == [1.0] and boot["hi"].tolist() == [1.0] and boot["sd"].tolist() == [0.0]
    assert boot["intervals"] == [["hap1", name, 1.0, 1.0, 1.0, 0.0]]
    # g6's five columns on ONE row of weight 40: every replicate draws that row 40 times, so all replicates are one and
    # lo = hi; with one contributor the proportion is 1 and lo = hi = prop to the bit
    g6 = golden("g6_refine")
    names = [haps[int(c)] for c in g6["cols"]]
    row = [(cohort["cm"].rows(0, 1), numpy.array([40.0]))]
    for fixed in (names[:1], names):
        numpy.random.seed(14)
        done = assign.finish_many(row, results[:1], haps, finish_args(contributors=",".join(fixed)))
        boot, why = assign.bootstrap(row[0][0], row[0][1], done[0], haps, finish_args(), n_boot=16, seed=2)
        assert why is None and _same_bits(boot["lo"], boot["hi"]) and not boot["sd"].any(), fixed
        assert all(_same_bits(boot["props_boot"][b], boot["props_boot"][0]) for b in range(16))
        prop = numpy.asarray(done[0]["refined"]["props"])
        moved = numpy.abs(boot["lo"] - prop).sum()
        print("one row,", len(fixed), "columns: sum |lo - prop|", moved, "iterations", sorted(set(boot["iters"].tolist())))
        # lo = hi = prop, to the loop's tolerance and no further: a replicate's weights ARE the sample's (40 draws of the one
        # row), so its first step is the step the refinement would have taken next from theta_{k+1} = prop, and it stops
        # there when that step's l1 = sum |p' - prop| is below args.tolerance -- the very sum bounded here.  (Exact equality
        # cannot hold for K > 1: the warm-started loop takes at least that one more step.)  Column by column, so a
        # replicate started or reported in another column order would show.
        assert (boot["iters"] == 1).all() and moved < finish_args().tolerance, (fixed, moved, boot["iters"])
        assert [r[1] for r in boot["intervals"]] == [c[1] for c in done[0]["contribs"]]
        for r in boot["intervals"]:
            assert abs(r[3] - r[2]) < finish_args().tolerance and r[3] == r[4], r
        if len(fixed) == 1:
            assert boot["lo"].tolist() == [1.0] and [r[2] for r in boot["intervals"]] == [1.0]


def test_device_weights_are_checked_where_they_are(cohort):
    """Weights handed over as device tensors are not read back: a sample the weights entry refuses is skipped with the
    entry's reason, and its neighbour comes out with the bits it has in a batch of its own."""
    import torch
    from mixemt_amd import assign
    samples, finished, haps = cohort["samples"], cohort["finished"], cohort["haps"]
    good = torch.from_numpy(numpy.asarray(samples[0][1], dtype=numpy.float64)).cuda()
    bad = torch.from_numpy(numpy.asarray(samples[1][1], dtype=numpy.float64)).cuda()
    bad[5] = 0.5
    boots, skipped = assign.bootstrap_many([(samples[0][0], good), (samples[1][0], bad)], finished, haps, finish_args(), n_boot=32, seed=3)
    assert boots[1] is None and skipped == [(1, assign.BOOTSTRAP_REFUSED[1])]
    alone, _ = assign.bootstrap_many(samples[:1], finished[:1], haps, finish_args(), n_boot=32, seed=3)
    assert _same_bits(boots[0]["props_boot"], alone[0]["props_boot"]) and _same_bits(boots[0]["lo"], alone[0]["lo"])
    zero = torch.zeros_like(good)
    boots, skipped = assign.bootstrap_many([(samples[0][0], zero), (samples[1][0], bad)], finished, haps, finish_args(), n_boot=32)
    assert boots == [None, None] and skipped == [(0, assign.BOOTSTRAP_REFUSED[2]), (1, assign.BOOTSTRAP_REFUSED[1])]
