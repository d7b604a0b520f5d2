"""
The EM loops of many samples in one batched device pass (mxm_em_iter_samples / mxm_em_loop_samples; em.run_em_many):
every sample must come out as if it had run alone -- the reference's goldens per sample, the oracle on small shapes,
and the same BITS whatever else shares the batch.
"""
import ctypes

import numpy
import pytest

from conftest import em_args, golden
from oracle import em_oracle

pytestmark = pytest.mark.gpu

PROPS_ATOL = 1e-9


@pytest.fixture(scope="module")
def pins(b17):
    """g4's 600 rows and g9's 2400 rows as ONE records matrix (built once, shared, never written to)."""
    from mixemt_amd import preprocess
    refseq, phy, haps, tables = b17
    g4, g5, g9, g15 = (golden(n) for n in ("g4_run_em", "g5_run_em_multi", "g9_run_em_2400", "g15_run_em_max_iter"))
    cm, row0 = preprocess.build_em_records_many(tables, [(g["row_ptr"], g["site"], g["obs"]) for g in (g4, g9)])
    assert list(row0) == [0, 600, 3000] and cm.rest_rows.numel() == 0
    return {"g4": g4, "g5": g5, "g9": g9, "g15": g15, "rows4": cm.rows(0, 600), "rows9": cm.rows(600, 3000), "cm": cm}


def test_reference_pins_in_one_batch(pins):
    """g4, the three restarts of g5 as three samples over g4's rows, g9 (1209 iterations): each its own golden -- a sample
    that converges early freezes while the others run on."""
    from mixemt_amd import em
    g4, g5, g9 = pins["g4"], pins["g5"], pins["g9"]
    samples = [(pins["rows4"], g4["wts"])] + [(pins["rows4"], g5["wts"])] * 3 + [(pins["rows9"], g9["wts"])]
    inits = [g4["inits"]] + [g5["inits"][r][None, :] for r in range(3)] + [g9["inits"]]
    res = em.run_em_many(samples, em_args(), inits=inits)
    assert [r["route"] for r in res] == ["batch"] * 5
    want_iters = [int(g4["iters"][0])] + [int(v) for v in g5["iters"]] + [int(g9["iters"][0])]
    print("iterations", [r["iters"] for r in res], "golden", want_iters)
    assert [r["iters"] for r in res] == [[n] for n in want_iters]
    assert all(r["done"] == [1] for r in res)
    assert len(set(want_iters)) == 5 and max(want_iters) == want_iters[-1] == 1209      # they do stop on different steps
    for r, g in ((res[0], g4), (res[4], g9)):
        print("max |props - golden|", numpy.abs(r["props"] - g["props"]).max())
        assert numpy.abs(r["props"] - g["props"]).max() < PROPS_ATOL
        assert int(r["props"].argmax()) == int(g["props"].argmax())
    # g5's golden is the reference's fold of its three restarts (em.py:155-163)
    ln_sum = numpy.log(res[1]["run_props"][0]) + numpy.log(res[2]["run_props"][0]) + numpy.log(res[3]["run_props"][0])
    folded = numpy.exp(ln_sum / 3)
    print("g5 max |props - golden|", numpy.abs(folded - g5["props"]).max())
    assert numpy.abs(folded - g5["props"]).max() < PROPS_ATOL
    assert int(folded.argmax()) == int(g5["props"].argmax())
    # ... and the same through n_multi = 3 on ONE sample (entries over the same records, folded by run_em_many)
    multi = em.run_em_many([(pins["rows4"], g5["wts"])], em_args(n_multi=3), inits=[g5["inits"]])[0]
    assert multi["iters"] == [int(v) for v in g5["iters"]] and multi["done"] == [1, 1, 1]
    assert numpy.abs(multi["props"] - g5["props"]).max() < PROPS_ATOL
    for run in range(3):                                  # the very bits of the three-samples form
        assert numpy.array_equal(multi["run_props"][run], res[1 + run]["run_props"][0])


def test_max_iter_pin_beside_a_second_sample(pins):
    """g15: g4's sample stopped by max_iter = 25 (em.py:140-142), in a batch with g9."""
    from mixemt_amd import em
    g4, g9, g15 = pins["g4"], pins["g9"], pins["g15"]
    res = em.run_em_many([(pins["rows4"], g4["wts"]), (pins["rows9"], g9["wts"])], em_args(max_iter=25),
                         inits=[g4["inits"], g9["inits"]])
    assert res[0]["done"] == [2] and res[0]["iters"] == [25]
    print("max |props - g15.props_25|", numpy.abs(res[0]["props"] - g15["props_25"]).max())
    assert numpy.abs(res[0]["props"] - g15["props_25"]).max() < PROPS_ATOL
    assert res[1]["done"] == [2] and res[1]["iters"] == [25]


def test_a_sample_is_the_same_bits_alone_first_or_last(pins):
    from mixemt_amd import em
    g4, g5, g9 = pins["g4"], pins["g5"], pins["g9"]
    me = (pins["rows4"], g4["wts"])
    others = [(pins["rows9"], g9["wts"])] + [(pins["rows4"], g5["wts"])] * 3
    other_inits = [g9["inits"]] + [g5["inits"][r][None, :] for r in range(3)]
    args = em_args(max_iter=120)                          # (bits, not convergence: a short loop)
    alone = em.run_em_many([me], args, inits=[g4["inits"]])[0]
    first = em.run_em_many([me] + others, args, inits=[g4["inits"]] + other_inits)
    last = em.run_em_many(others + [me], args, inits=other_inits + [g4["inits"]])
    again = em.run_em_many(others + [me], args, inits=other_inits + [g4["inits"]])
    for got in (first[0], last[4]):
        assert got["iters"] == alone["iters"] == [120]
        assert numpy.array_equal(got["ln_theta_k"].view(numpy.int64), alone["ln_theta_k"].view(numpy.int64))          # ln_cur
        assert numpy.array_equal(got["ln_theta_next"].view(numpy.int64), alone["ln_theta_next"].view(numpy.int64))    # ln_new
    for a, b in zip(last, again):                         # two runs of the same batch
        assert a["iters"] == b["iters"]
        assert numpy.array_equal(a["ln_theta_k"].view(numpy.int64), b["ln_theta_k"].view(numpy.int64))
        assert numpy.array_equal(a["ln_theta_next"].view(numpy.int64), b["ln_theta_next"].view(numpy.int64))


def _few_values(rng, rows, n_haps, n_vals):
    """A matrix whose rows hold at most n_vals distinct values (so that they code)."""
    vals = rng.normal(-25.0, 8.0, size=(rows, n_vals))
    return numpy.take_along_axis(vals, rng.integers(0, n_vals, size=(rows, n_haps)), axis=1)


@pytest.mark.parametrize("n_haps", [66, 128, 5408])
def test_small_shapes_against_the_oracle(n_haps):
    """Samples of 1, 2, K - 1, K, K + 1 and 2K + 1 rows in one batch; weights with 0 and > 1; at the width that has room
    for them, a sample with rows of 257 .. 1024 distinct values (wide records) between byte-coded ones."""
    from mixemt_amd import _lib, em
    k = _lib.load().mxm_samples_tile_rows()
    rng = numpy.random.default_rng(100 + n_haps)
    mats = [_few_values(rng, rows, n_haps, 9) for rows in (1, 2, k - 1, k, k + 1, 2 * k + 1)]
    if n_haps >= 1024:
        wide = _few_values(rng, k + 3, n_haps, 9)
        wide[0::2] = _few_values(rng, len(wide[0::2]), n_haps, 600)
        wide[1] = _few_values(rng, 1, n_haps, 300)[0]
        assert all(256 < len(numpy.unique(row)) <= 1024 for row in wide[0::2])
        mats.insert(3, wide)
    wts = [rng.integers(0, 5, size=len(m)).astype(numpy.float64) for m in mats]
    for w in wts:
        w[0] = max(w[0], 2.0)                             # (a sample of weight 0 has no proportions at all)
    assert any((w == 0).any() for w in wts) and any((w > 1).any() for w in wts)
    inits = [rng.dirichlet([1.0] * n_haps)[None, :] for _ in mats]
    args = em_args(max_iter=40)
    res = em.run_em_many(list(zip(mats, wts)), args, inits=inits)
    if n_haps >= 1024:                                    # the wide rows did get 16-bit codes
        plan = em.EmPlan(mats[3], wts[3], storage="coded")
        assert plan.coded_wide == len(mats[3][0::2]) + 1 and plan.coded_rest == 0
    for m, w, init, r in zip(mats, wts, inits, res):
        theta, _, n_iter = em_oracle._one_run(m, w, numpy.log(init[0]), numpy.empty_like(m), args.max_iter, args.tolerance, False)
        err = numpy.abs(r["props"] - numpy.exp(theta)).max()
        print("rows %d: iterations %s (oracle %d), max |props - oracle| %.3g" % (len(m), r["iters"], n_iter, err))
        assert r["route"] == "batch" and r["iters"] == [n_iter]
        assert err < PROPS_ATOL


def test_a_row_of_minus_infinity_poisons_its_own_sample_only():
    """em.py:81-87: -inf - (-inf) = NaN in that sample's proportions; its neighbours are bit for bit what they are without it."""
    from mixemt_amd import _lib, em
    k = _lib.load().mxm_samples_tile_rows()
    rng = numpy.random.default_rng(9)
    n_haps = 128
    mats = [_few_values(rng, rows, n_haps, 7) for rows in (k + 5, 2 * k + 2, 3)]
    mats[1][k + 1, :] = -numpy.inf
    wts = [rng.integers(1, 4, size=len(m)).astype(numpy.float64) for m in mats]
    inits = [rng.dirichlet([1.0] * n_haps)[None, :] for _ in mats]
    args = em_args(max_iter=8, tolerance=0.0)
    with_it = em.run_em_many(list(zip(mats, wts)), args, inits=inits)
    without = em.run_em_many([(mats[0], wts[0]), (mats[2], wts[2])], args, inits=[inits[0], inits[2]])
    assert with_it[1]["done"] == [2] and with_it[1]["iters"] == [8] and numpy.isnan(with_it[1]["props"]).all()
    for a, b in ((with_it[0], without[0]), (with_it[2], without[1])):
        assert a["iters"] == b["iters"] == [8] and numpy.isfinite(a["props"]).all()
        assert numpy.array_equal(a["ln_theta_k"].view(numpy.int64), b["ln_theta_k"].view(numpy.int64))
        assert numpy.array_equal(a["ln_theta_next"].view(numpy.int64), b["ln_theta_next"].view(numpy.int64))
    # weight 0 drops the row, as scipy drops it
    wts[1][k + 1] = 0.0
    dropped = em.run_em_many(list(zip(mats, wts)), args, inits=inits)
    assert numpy.isfinite(dropped[1]["props"]).all()


def test_bad_arguments_are_refused_before_anything_is_launched():
    import torch
    from mixemt_amd import _lib, em
    from mixemt_amd._dev import current_stream
    lib = _lib.load()
    rng = numpy.random.default_rng(2)
    n_haps = 128
    mat = _few_values(rng, 50, n_haps, 5)
    plan = em.EmPlan(mat, numpy.ones(50), storage="coded", keep_log_matrix=False)
    rec, rec_off, ndist = plan._coded_keep[:3]
    batch = em.SampleBatch(rec, rec_off, ndist, plan.wts, [0, 20, 50], n_haps)
    props = torch.full((2, n_haps), 1.0 / n_haps, dtype=torch.float64, device=batch.dev)
    ln, ln_next = torch.log(props), torch.log(props)
    colsum = torch.full_like(props, -7.0)
    state = em.new_state(2, batch.dev)
    host_state = (_lib.EmState * 2)()

    def calls(coded, row0, n_samples, width):
        row0 = numpy.ascontiguousarray(row0, dtype=numpy.int64)
        r0 = row0.ctypes.data_as(ctypes.c_void_p)
        yield lib.mxm_em_iter_samples(ctypes.byref(coded), r0, n_samples, batch.wts.data_ptr(), props.data_ptr(), width,
                                      state.data_ptr(), colsum.data_ptr(), batch.ws.data_ptr(), batch.ws_bytes, current_stream())
        yield lib.mxm_em_loop_samples(ctypes.byref(coded), r0, n_samples, batch.wts.data_ptr(), width, props.data_ptr(),
                                      ln.data_ptr(), ln_next.data_ptr(), colsum.data_ptr(), state.data_ptr(), 1e-4, 10, 4,
                                      batch.ws.data_ptr(), batch.ws_bytes, current_stream(), host_state)

    def copy_of(coded, **fields):
        out = _lib.Coded()
        ctypes.memmove(ctypes.byref(out), ctypes.byref(coded), ctypes.sizeof(_lib.Coded))
        for name, value in fields.items():
            setattr(out, name, value)
        return out

    quads = copy_of(batch.coded, qrec=rec.data_ptr(), qoff=rec_off.data_ptr(), nquad=ndist.data_ptr())
    rest = copy_of(batch.coded, R_rest=1)
    cases = {"an empty sample": (batch.coded, [0, 20, 20, 50], 3, n_haps),
             "row0 not ascending": (batch.coded, [0, 30, 20, 50], 3, n_haps),
             "row0[S] != R": (batch.coded, [0, 20, 49], 2, n_haps),
             "odd H": (batch.coded, [0, 20, 50], 2, n_haps - 1),
             "H below 66": (batch.coded, [0, 20, 50], 2, 64),
             "H above 8192": (batch.coded, [0, 20, 50], 2, 8194),
             "a quad dictionary": (quads, [0, 20, 50], 2, n_haps),
             "a dense rest": (rest, [0, 20, 50], 2, n_haps)}
    for what, (coded, row0, n_samples, width) in cases.items():
        for rc in calls(coded, row0, n_samples, width):
            assert rc == -1, what
            assert lib.mxm_last_error().decode() != "", what
    torch.cuda.synchronize()
    assert (colsum == -7.0).all() and int(state.abs().sum()) == 0          # nothing ran
    # the binding raises
    with pytest.raises(ValueError, match="mxm_samples_plan"):
        em.SampleBatch(rec, rec_off, ndist, plan.wts, [0, 50, 50], n_haps)
    # and the same arguments, left alone, do run
    for rc in calls(batch.coded, [0, 20, 50], 2, n_haps):
        assert rc == 0
    torch.cuda.synchronize()
    assert torch.isfinite(colsum).all() and (colsum != -7.0).all()
