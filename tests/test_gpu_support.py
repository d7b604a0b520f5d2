"""
Contributor support (include/mixemt_hip_support.h; assign.support_many) on the device:
  loop      every fit of mxm_em_loop_samples_narrow_masks bit for bit against mxm_em_loop_samples_narrow on that sample alone
            with its matrix gathered at just the masked-in columns (the "compacted" loop), from the same uniform start: every
            ld, column counts around the strides, masks at both ends, rows around the workgroup's 256 threads, ragged batches,
            the LDS / E boundary, a masked-out column that dominates, unused slots and finished fits across a resume;
  loglik    mxm_loglik_samples_masks against the long-double reference of tests/_support_ref.py on the bits the kernel reads;
  end to end   the golden samples of tests/test_gpu_samples_finish.py (g8, g14, g6 as one batch) through run_em_many ->
            finish_many -> support_many -> report_support_many.
The two entries read no record, so their tests hand em.SampleFinish a record buffer of zeros.
"""
import ctypes
import io
import math

import numpy
import pytest

import _exact as ex
import _support_ref as ref
from conftest import em_args, golden
from test_gpu_bootstrap import _finish, _one_run, _same_bits
from test_samples_finish_host import finish_args

pytestmark = pytest.mark.gpu

THREADS = 256                   # SFIN_THREADS: the loop's and the log-likelihood's workgroup
LDS_CELLS = 9216                # SFIN_LDS_DOUBLES
TOL, MAX_ITER = 1e-9, 300
WORST = {"ratio": 0.0}          # the largest rel(ll_gpu) / bound seen by the accuracy tests (printed by each)


def _ld_for(k):
    return 4 if k <= 4 else (8 if k <= 8 else 16)


def _bits(masks, ld):
    return ((numpy.asarray(masks, dtype=numpy.uint32)[..., None] >> numpy.arange(ld, dtype=numpy.uint32)) & 1).astype(numpy.float64)


def _start_tables(masks, ld, fill=None):
    """Uniform starts over every mask as the device tables of a direct call: {props_cur, ln_cur, ln_new} [S * B][ld] and the
    zeroed states.  fill: the value of every entry outside a mask (default: 0 / -inf as em_loop_masks uploads them)."""
    import torch
    from mixemt_amd import em
    n, n_fits = masks.shape
    bits = _bits(masks, ld)
    p0 = (bits / numpy.maximum(bits.sum(axis=2, keepdims=True), 1)).reshape(n * n_fits, ld)
    ln0, p0 = em.log_inits(p0)
    if fill is not None:
        off = bits.reshape(n * n_fits, ld) == 0
        ln0[off], p0[off] = fill, fill
    return {"props_cur": torch.from_numpy(p0).cuda(), "ln_cur": torch.from_numpy(ln0).cuda(), "ln_new": torch.from_numpy(ln0.copy()).cuda(),
            "state": em.new_state(n * n_fits, "cuda")}


def _run_masks(fin, mat_d, ld, ncol, masks, tol=TOL, max_iter=MAX_ITER, check_every=16, tables=None, lin="own"):
    """mxm_em_loop_samples_narrow_masks called directly -> (rc, tables as numpy [S][B][ld], [(done, iters, l1)] [S][B], tables)."""
    import torch
    from mixemt_amd import _lib
    masks = numpy.ascontiguousarray(masks, dtype=numpy.uint32)
    ncol = numpy.ascontiguousarray(ncol, dtype=numpy.int32)
    n, n_fits = masks.shape
    tables = _start_tables(masks, ld) if tables is None else tables
    ws_bytes = fin._support_ws(n_fits, ld)
    if isinstance(lin, str):
        lin = torch.empty((n_fits * fin.n_rows, ld), dtype=torch.float64, device="cuda")
    host = (_lib.EmState * (n * n_fits))()
    rc = fin.lib.mxm_em_loop_samples_narrow_masks(ctypes.byref(fin.coded), fin.row0_ptr, n, fin.n_haps, n_fits, mat_d.data_ptr(), ld,
                                                  ncol.ctypes.data, masks.ctypes.data, fin.wts.data_ptr(), tables["props_cur"].data_ptr(),
                                                  tables["ln_cur"].data_ptr(), tables["ln_new"].data_ptr(), tables["state"].data_ptr(),
                                                  tol, max_iter, check_every, None if lin is None else lin.data_ptr(),
                                                  fin.ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream, host)
    torch.cuda.synchronize()
    got = {key: tables[key].cpu().numpy().reshape(n, n_fits, ld) for key in ("props_cur", "ln_cur", "ln_new")}
    states = [[(host[s * n_fits + b].done, host[s * n_fits + b].iters, host[s * n_fits + b].l1) for b in range(n_fits)] for s in range(n)]
    return rc, got, states, tables


def _compacted(lib, mat_s, w, mask, tol=TOL, max_iter=MAX_ITER, check_every=16):
    """The one-run loop on the sample alone with its matrix gathered at the masked-in columns, in ascending order, at the
    narrowest stride that holds them, from the uniform start."""
    cols = ref.mask_columns(mask)
    ld = _ld_for(len(cols))
    sub = numpy.full((mat_s.shape[0], ld), -numpy.inf)
    sub[:, :len(cols)] = mat_s[:, cols]
    return _one_run(lib, sub, ld, len(cols), w, numpy.full(len(cols), 1.0 / len(cols)), tol, max_iter, check_every)


def _check_fit(got, states, s, b, mask, k, want, what):
    """Fit (s, b) against the compacted loop's tables: the masked-in columns bit for bit, the masked-out ones -inf / 0."""
    cols = ref.mask_columns(mask)
    out = [c for c in range(k) if c not in cols]
    for key in ("ln_cur", "ln_new", "props_cur"):
        assert _same_bits(got[key][s, b, cols], want[key][:len(cols)]), (what, s, b, key)
    assert numpy.isneginf(got["ln_cur"][s, b, out]).all() and numpy.isneginf(got["ln_new"][s, b, out]).all(), (what, s, b)
    assert not got["props_cur"][s, b, out].any(), (what, s, b)
    done, n_iter, l1 = states[s][b]
    assert (done, n_iter) == want["state"][:2] and _same_bits([l1], [want["state"][2]]), (what, s, b, states[s][b], want["state"])


def _matrix(rng, rows, k, ld):
    mat = numpy.full((rows, ld), -numpy.inf)
    # weakly informative rows, as tests/test_gpu_bootstrap.py's: the loop takes tens of iterations to 1e-9, several launches
    mat[:, :k] = rng.normal(-30.0, 1.0, size=(rows, k)) + 4.0 * (rng.random((rows, k)) < 0.4)
    return mat


def _mask_set(k):
    """lowest bit, alternating bits, AN UNUSED SLOT, highest bit, all bits."""
    return [1, sum(1 << c for c in range(0, k, 2)), 0, 1 << (k - 1), (1 << k) - 1]


ROWS = (1, THREADS - 1, THREADS, THREADS + 1)
LOOP_CASES = [(ld, k) for ld in (4, 8, 16) for k in (1, 3, 4, 5, 8, 9, 16) if k <= ld]


@pytest.mark.parametrize("ld,k", LOOP_CASES, ids=["ld%d-K%d" % c for c in LOOP_CASES])
def test_every_fit_equals_the_compacted_one_run_loop(ld, k):
    import torch
    case = LOOP_CASES.index((ld, k))
    rng = numpy.random.default_rng(100 * ld + k)
    rows = [ROWS[(case + j) % 4] for j in range(3)]                         # ragged; over the cases every count stands everywhere
    ks = [k, max(1, k - 1), k]                                              # ... and the column counts are ragged too
    mats = [_matrix(rng, r, kk, ld) for r, kk in zip(rows, ks)]
    weights = [rng.integers(0, 4, size=r).astype(numpy.float64) for r in rows]
    for w in weights:
        w[0] = 2.0                                                          # (no sample without a weighted row)
    masks = numpy.array([_mask_set(kk) for kk in ks], dtype=numpy.uint32)
    fin = _finish(weights)
    rc, got, states, _ = _run_masks(fin, torch.from_numpy(numpy.concatenate(mats)).cuda(), ld, ks, masks)
    assert rc == 0, fin.lib.mxm_last_error()
    iters = set()
    for s in range(3):
        for b, mask in enumerate(masks[s]):
            if mask == 0:                                                   # the unused slot: nothing ran, nothing written
                assert states[s][b] == (0, 0, 0.0) and numpy.isneginf(got["ln_new"][s, b]).all() and not got["props_cur"][s, b].any()
                continue
            want = _compacted(fin.lib, mats[s], weights[s], int(mask))
            _check_fit(got, states, s, b, int(mask), ks[s], want, (ld, k))
            assert states[s][b][0] in (1, 2), (ld, k, s, b, states[s][b])   # (16 columns on 256 weak rows run into max_iter)
            iters.add(states[s][b][1])
    print("ld", ld, "K", k, "rows", rows, "iterations:", sorted(iters))
    assert k == 1 or max(iters) > 16                                        # more than one launch of check_every = 16
    # sample 1 alone, first and last: the same bits each time
    for order in ([1], [1, 0, 2], [2, 0, 1]):
        sub = _finish([weights[i] for i in order])
        rc, alone, st, _ = _run_masks(sub, torch.from_numpy(numpy.concatenate([mats[i] for i in order])).cuda(), ld,
                                      [ks[i] for i in order], masks[order])
        assert rc == 0
        at = order.index(1)
        for key in got:
            assert _same_bits(alone[key][at], got[key][1]), (ld, k, order, key)
        assert [x[:2] for x in st[at]] == [x[:2] for x in states[1]] and _same_bits([x[2] for x in st[at]], [x[2] for x in states[1]])


def test_the_lds_and_e_boundary_each_fit_in_its_own_slice():
    """K = 4: 2304 rows are 9216 cells (in LDS), 2305 rows go through E -- B x R x ld doubles, fit (s, b) in its own slice."""
    import torch
    rng = numpy.random.default_rng(2304)
    rows, ld, k = [LDS_CELLS // 4, LDS_CELLS // 4 + 1], 4, 4
    mats = [_matrix(rng, r, k, ld) for r in rows]
    weights = [rng.integers(0, 4, size=r).astype(numpy.float64) for r in rows]
    masks = numpy.array([[0b1111, 0b0111, 0b1011, 0b1101, 0b1110]] * 2, dtype=numpy.uint32)
    fin = _finish(weights)
    mat_d = torch.from_numpy(numpy.concatenate(mats)).cuda()
    # E = NULL: refused for the batch with the second sample, before anything is launched; accepted for the first alone
    tables = _start_tables(masks, ld)
    before = {key: tables[key].clone() for key in tables}
    rc, _, _, _ = _run_masks(fin, mat_d, ld, [k, k], masks, tables=tables, lin=None)
    assert rc == -1 and b"more than 9216 cells needs the global copy E" in fin.lib.mxm_last_error()
    assert all(torch.equal(tables[key], before[key]) for key in tables) and not bool(tables["state"].any())
    first = _finish(weights[:1])
    rc, alone, alone_states, _ = _run_masks(first, torch.from_numpy(mats[0]).cuda(), ld, [k], masks[:1], lin=None)
    assert rc == 0, first.lib.mxm_last_error()
    # with E at exactly B x R x ld doubles: every fit against the compacted loop (three columns: 6915 cells, in ITS LDS)
    lin = torch.full((5 * fin.n_rows, ld), float("nan"), dtype=torch.float64, device="cuda")
    rc, got, states, _ = _run_masks(fin, mat_d, ld, [k, k], masks, lin=lin)
    assert rc == 0, fin.lib.mxm_last_error()
    for s in range(2):
        for b, mask in enumerate(masks[s]):
            want = _compacted(fin.lib, mats[s], weights[s], int(mask))
            _check_fit(got, states, s, b, int(mask), k, want, "boundary")
            assert states[s][b][0] == 1 and states[s][b][1] > 16
    for key in got:
        assert _same_bits(alone[key][0], got[key][0]), key
    # the sample in LDS wrote nothing into E; the other's five slices hold e under each MASK's own shift
    lin_h = lin.cpu().numpy()
    assert numpy.isnan(lin_h[:5 * rows[0]]).all()
    for b, mask in enumerate(masks[1]):
        cols = ref.mask_columns(int(mask))
        part = lin_h[5 * rows[0] + b * rows[1]:5 * rows[0] + (b + 1) * rows[1]]
        want = numpy.exp(mats[1][:, cols] - mats[1][:, cols].max(axis=1, keepdims=True))
        assert numpy.abs(part[:, cols] - want).max() < 1e-15 and (part[:, cols].max(axis=1) == 1.0).all(), b
        assert not part[:, [c for c in range(4) if c not in cols]].any(), b


def test_a_masked_out_column_that_dominates_does_not_change_the_fit():
    """The masked-out cell exceeds every masked-in cell of its row by 800 nats: under a shift over ALL columns every
    masked-in e would underflow to 0 (z = 0, NaN); under the mask's own shift the fit is the compacted loop's."""
    import torch
    rng = numpy.random.default_rng(800)
    rows, ld, k = 300, 4, 3
    mat = _matrix(rng, rows, k, ld)
    mat[::2, 1] = mat[::2, [0, 2]].max(axis=1) + 800.0
    w = rng.integers(1, 4, size=rows).astype(numpy.float64)
    fin = _finish([w])
    masks = numpy.array([[0b101, 0b111]], dtype=numpy.uint32)
    rc, got, states, _ = _run_masks(fin, torch.from_numpy(mat).cuda(), ld, [k], masks)
    assert rc == 0, fin.lib.mxm_last_error()
    want = _compacted(fin.lib, mat, w, 0b101)
    _check_fit(got, states, 0, 0, 0b101, k, want, "dominated")
    assert states[0][0][0] == 1 and states[0][0][1] > 3 and numpy.isfinite(got["ln_new"][0, 0, [0, 2]]).all()
    assert abs(numpy.exp(got["ln_new"][0, 0, [0, 2]]).sum() - 1.0) < 1e-12
    # the full fit is another fit: the dominating column takes (nearly) all of it
    assert states[0][1][0] == 1 and numpy.exp(got["ln_new"][0, 1, 1]) > 0.4


def test_unused_slots_and_finished_fits_are_left_alone_across_a_resume():
    """check_every = 2, max_iter = 7: the one-column fits stop converged after their first step, the others at max_iter; one
    of those is then resumed (done <- 0, max_iter = 20) and nothing else may move -- the unused slot keeps the caller's bytes.
    A fit stopped at max_iter keeps theta_k in ln_cur / props_cur (ln_new holds the step it did not take over), as the one-run
    loop does: resumed, it takes that step again, so its 20th counted iteration ends where a straight run's 19th does."""
    import torch
    rng = numpy.random.default_rng(7)
    ld, ks, rows = 8, [5, 3], [THREADS + 1, 40]
    mats = [_matrix(rng, r, kk, ld) for r, kk in zip(rows, ks)]
    weights = [rng.integers(1, 4, size=r).astype(numpy.float64) for r in rows]
    masks = numpy.array([[0b00001, 0, 0b11111, 0b10101], [0b111, 0b010, 0, 0b011]], dtype=numpy.uint32)
    fin = _finish(weights)
    mat_d = torch.from_numpy(numpy.concatenate(mats)).cuda()
    tables = _start_tables(masks, ld, fill=0.25)                            # 0.25 wherever no mask bit is
    rc, got, states, tables = _run_masks(fin, mat_d, ld, ks, masks, max_iter=7, check_every=2, tables=tables)
    assert rc == 0, fin.lib.mxm_last_error()
    assert [[st[:2] for st in sample] for sample in states] == [[(1, 1), (0, 0), (2, 7), (2, 7)], [(2, 7), (1, 1), (0, 0), (2, 7)]]
    for s in range(2):
        for b, mask in enumerate(masks[s]):
            for key in got:
                if mask == 0:
                    assert (got[key][s, b] == 0.25).all(), (s, b, key)       # the unused slot
                else:
                    assert (got[key][s, b, ks[s]:] == 0.25).all(), (s, b, key)           # past the sample's columns
    raw0 = tables["state"].cpu().numpy().view(numpy.int32).reshape(8, 6).copy()
    assert not raw0[[1, 6]].any()                                           # the unused slots' states: never written
    # resume fit (0, 3) alone
    raw = raw0.copy()
    raw[3, 0] = 0
    tables["state"].copy_(torch.from_numpy(raw.reshape(-1).view(numpy.int64)).cuda())
    rc, again, states2, _ = _run_masks(fin, mat_d, ld, ks, masks, max_iter=20, check_every=2, tables=tables)
    assert rc == 0, fin.lib.mxm_last_error()
    assert states2[0][3][:2] == (2, 20)
    raw2 = tables["state"].cpu().numpy().view(numpy.int32).reshape(8, 6)
    for e in range(8):
        if e != 3:
            assert numpy.array_equal(raw2[e], raw0[e]), e
            for key in got:
                assert _same_bits(again[key][e // 4, e % 4], got[key][e // 4, e % 4]), (e, key)
    # ... and the resumed fit is where a straight run ends that takes every step once (19 of them), bit for bit
    want = _compacted(fin.lib, mats[0], weights[0], 0b10101, max_iter=19, check_every=2)
    want["state"] = (2, 20, want["state"][2])
    _check_fit(again, states2, 0, 3, 0b10101, 5, want, "resumed")


# ---- the log-likelihood ----------------------------------------------------------------------------------------------
def _loglik(fin, mat_d, ld, ncol, masks, ln_props, weighted=True):
    """mxm_loglik_samples_masks called directly -> (ll [S][B], n_eff [S]); ll starts as NaN."""
    import torch
    masks = numpy.ascontiguousarray(masks, dtype=numpy.uint32)
    ncol = numpy.ascontiguousarray(ncol, dtype=numpy.int32)
    n, n_fits = masks.shape
    lnp = torch.from_numpy(numpy.ascontiguousarray(ln_props, dtype=numpy.float64)).cuda()
    ll = torch.full((n, n_fits), float("nan"), dtype=torch.float64, device="cuda")
    n_eff = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    ws_bytes = fin._support_ws(n_fits, ld)
    rc = fin.lib.mxm_loglik_samples_masks(ctypes.byref(fin.coded), fin.row0_ptr, n, fin.n_haps, n_fits, mat_d.data_ptr(), ld,
                                          ncol.ctypes.data, masks.ctypes.data, fin.wts.data_ptr() if weighted else None, lnp.data_ptr(),
                                          ll.data_ptr(), n_eff.data_ptr(), fin.ws.data_ptr(), ws_bytes,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, fin.lib.mxm_last_error()
    return ll.cpu().numpy(), n_eff.cpu().numpy()


def _check_ll(got, mat, lnp, w, mask, what):
    """The tight rule of tests/_exact.py applied to ll: rel(ll_gpu) <= 8 max(rel(ll_seq), 4u); every term is <= 0 here (the
    cells are log-likelihoods below 0 and the proportions sum to at most 1), so the sum is perfectly conditioned."""
    exact = ref.exact_loglik(mat, lnp, w, mask)
    assert numpy.isfinite(float(exact)) and exact < 0, what
    rel_seq = ref.rel_ll(ref.seq_loglik(mat, lnp, w, mask), exact)
    bound = ex.tight_bound(rel_seq)
    rel = ref.rel_ll(got, exact)
    WORST["ratio"] = max(WORST["ratio"], rel / bound)
    print("%s: rel(ll_gpu) %.3g, rel(ll_seq) %.3g, bound %.3g, ratio %.3f (worst so far %.3f)" % (what, rel, rel_seq, bound, rel / bound,
                                                                                                 WORST["ratio"]))
    assert rel <= bound, (what, rel, bound)


@pytest.fixture(scope="module")
def ll_batch():
    """S = 3 samples at ld = 8 (made once): 700 x 5 with weights 2^0 .. 2^20 and a row of weight 0 that holds -inf cells;
    257 x 3; 1 x 2.  Four fits each (one slot unused in the last), refined on the device: ln_props is the loop's ln_new."""
    import torch
    rng = numpy.random.default_rng(96)
    ld, ks, rows = 8, [5, 3, 2], [700, THREADS + 1, 1]
    mats = [_matrix(rng, r, kk, ld) for r, kk in zip(rows, ks)]
    weights = [2.0 ** rng.integers(0, 21, size=rows[0]), rng.integers(0, 4, size=rows[1]).astype(numpy.float64), numpy.array([3.0])]
    weights[0][13] = 0.0
    mats[0][13, :5] = -numpy.inf
    masks = numpy.array([[0b11111, 0b10101, 0b00010, 0b01111], [0b111, 0b011, 0b100, 0b110], [0b11, 0b01, 0, 0b10]], dtype=numpy.uint32)
    fin = _finish(weights)
    mat_d = torch.from_numpy(numpy.concatenate(mats)).cuda()
    rc, got, states, _ = _run_masks(fin, mat_d, ld, ks, masks)
    assert rc == 0 and all(st[0] == 1 for s in range(3) for b, st in enumerate(states[s]) if masks[s, b])
    return {"ld": ld, "ks": ks, "rows": rows, "mats": mats, "weights": weights, "masks": masks, "fin": fin, "mat_d": mat_d,
            "ln_props": got["ln_new"]}


def test_loglik_against_the_long_double_reference(ll_batch):
    b = ll_batch
    ll, n_eff = _loglik(b["fin"], b["mat_d"], b["ld"], b["ks"], b["masks"], b["ln_props"])
    for s in range(3):
        for f, mask in enumerate(b["masks"][s]):
            if mask == 0:
                assert numpy.isnan(ll[s, f])                                 # the unused slot: left alone
                continue
            _check_ll(ll[s, f], b["mats"][s], b["ln_props"][s, f], b["weights"][s], int(mask), "weighted s%d f%d" % (s, f))
        exact = math.fsum(b["weights"][s])
        assert abs(n_eff[s] - exact) <= (b["rows"][s] + 8) * ex.U * exact, (s, n_eff[s], exact)
    # a nested fit is never better than the full one at the maximum (to the loop's tolerance)
    assert ll[0, 1] < ll[0, 0] and ll[0, 2] < ll[0, 0] and ll[1, 1] < ll[1, 0]
    # w = NULL: every weight 1 -- the row of weight 0 above now counts, and its cells are -inf: that sample's fits are -inf
    ll1, n1 = _loglik(b["fin"], b["mat_d"], b["ld"], b["ks"], b["masks"], b["ln_props"], weighted=False)
    assert n1.tolist() == [float(r) for r in b["rows"]]
    assert numpy.isneginf(ll1[0]).all()
    for f, mask in enumerate(b["masks"][1]):
        _check_ll(ll1[1, f], b["mats"][1], b["ln_props"][1, f], None, int(mask), "w = NULL f%d" % f)


def test_loglik_redoes_an_underflowing_row_in_log_space_and_gives_minus_inf_without_a_finite_cell(ll_batch):
    import torch
    b = ll_batch
    mat, w = b["mats"][1].copy(), b["weights"][1].copy()
    w[7] = w[9] = 2.0
    mat[7, :3] = (-1300.0, 0.0, -1305.0)                                    # under the mask 0b101: ln p + M near -2000
    mat[9, :3] = (-numpy.inf, -31.0, -numpy.inf)                            # no finite cell under 0b101; one under 0b111
    lnp = numpy.full((1, 3, 8), -numpy.inf)
    lnp[0, :, :3] = numpy.log(numpy.array([1e-300, 1.0 - 2e-300, 1e-300]))
    masks = numpy.array([[0b101, 0b111, 0b101]], dtype=numpy.uint32)
    fin = _finish([w])
    easy = mat.copy()
    easy[9, :3] = (-31.0, -31.0, -32.0)
    for name, m, finite in (("redo", easy, (True, True, True)), ("no finite cell", mat, (False, True, False))):
        ll, _ = _loglik(fin, torch.from_numpy(m).cuda(), 8, [3], masks, lnp)
        for f in range(3):
            if finite[f]:
                _check_ll(ll[0, f], m, lnp[0, f], w, int(masks[0, f]), "%s f%d" % (name, f))
            else:
                assert numpy.isneginf(ll[0, f]), (name, f, ll[0, f])
    # the redo was needed: the linear sum of row 7 under 0b101 is below 2^-960
    assert 1e-300 * (1.0 + math.exp(-5.0)) < ref.LINEAR_MIN


def test_loglik_has_the_same_bits_alone_first_and_last(ll_batch):
    import torch
    b = ll_batch
    ll, n_eff = _loglik(b["fin"], b["mat_d"], b["ld"], b["ks"], b["masks"], b["ln_props"])
    for order in ([1], [1, 0, 2], [2, 0, 1]):
        fin = _finish([b["weights"][i] for i in order])
        got, n_got = _loglik(fin, torch.from_numpy(numpy.concatenate([b["mats"][i] for i in order])).cuda(), b["ld"],
                             [b["ks"][i] for i in order], b["masks"][order], b["ln_props"][order])
        at = order.index(1)
        assert _same_bits(got[at], ll[1]) and _same_bits(n_got[at:at + 1], n_eff[1:2]), order
    # ... and whatever other fits share the batch: fit 3 alone in slot 0 (n_eff is written whether or not slot 0 is used)
    fin = _finish([b["weights"][1]])
    for masks, lnp, at in (([[b["masks"][1, 3]]], b["ln_props"][1:2, 3:4], 0), ([[0, b["masks"][1, 3]]], b["ln_props"][1:2, 2:4], 1)):
        got, n_got = _loglik(fin, torch.from_numpy(b["mats"][1]).cuda(), b["ld"], [b["ks"][1]], numpy.array(masks, dtype=numpy.uint32), lnp)
        assert _same_bits(got[0, at:at + 1], ll[1, 3:4]) and _same_bits(n_got, n_eff[1:2])


# ---- end to end ------------------------------------------------------------------------------------------------------
E2E_TOLERANCES = (1e-4, 1e-8)           # args.tolerance; the tolerance the test runs at when the reference finds a negative drop-one lrt there


@pytest.fixture(scope="module")
def cohort(b17):
    """The g4 rows three times in one batch, finished as the goldens g8 (its voted contributors), g14 (one contributor) and g6
    (five fixed columns) finish them -- the samples of tests/test_gpu_samples_finish.py; finished once per tolerance."""
    from mixemt_amd import assign, em, preprocess
    refseq, phy, haps, tables = b17
    g4 = golden("g4_run_em")
    cm, row0 = preprocess.build_em_records_many(tables, [(g4["row_ptr"], g4["site"], g4["obs"])])
    sample = (cm.rows(0, 600), g4["wts"])
    results = em.run_em_many([sample], em_args(), inits=[g4["inits"]])
    g14, g6 = golden("g14_single_contributor"), golden("g6_refine")
    fixed = [None, haps[int(g14["col"][0])], ",".join(haps[int(c)] for c in g6["cols"])]
    made = {}

    def finish(tolerance):
        if tolerance not in made:
            numpy.random.seed(8)
            made[tolerance] = [assign.finish_many([sample], results, haps, finish_args(contributors=con, tolerance=tolerance))[0]
                               for con in fixed]
            assert all(f["route"] == "batch" and f["refined"] is not None for f in made[tolerance])
            assert [len(f["contribs"]) for f in made[tolerance]] == [3, 1, 5]
        return made[tolerance]
    return {"samples": [sample] * 3, "finish": finish, "haps": haps, "cm": cm, "wts": g4["wts"]}


def _full_fit_gap(one, fin):
    """max |the full fit's proportion - the refinement's| over the contributors, matched by name."""
    by_name = dict(zip(one["models"][0]["names"], one["models"][0]["props"]))
    want = dict(zip(fin["sub_haps"], numpy.asarray(fin["refined"]["props"]).reshape(-1)))
    return max(abs(by_name[h] - want[h]) for h in want)


def _reference_drop_one(cohort, finished_one, tolerance, max_iter):
    """{haplogroup: drop-one lrt} of one sample from the CPU reference alone (tests/_support_ref.py: subset_em from the
    uniform start to `tolerance`, exact_loglik), on the sample's columns as the device gathers them."""
    import torch
    from mixemt_amd import assign
    index = {h: i for i, h in enumerate(cohort["haps"])}
    names = sorted((c[1] for c in finished_one["contribs"]), key=index.get)
    wts_d = {0: torch.from_numpy(numpy.asarray(cohort["wts"], dtype=numpy.float64)).cuda()}
    batch = assign._finish_batch(cohort["samples"][:1], wts_d, [0])
    ld = _ld_for(len(names))
    cols = numpy.zeros((1, ld), dtype=numpy.int32)
    cols[0, :len(names)] = [index[h] for h in names]
    mat = batch.gather(cols, [len(names)], ld).cpu().numpy()
    full = (1 << len(names)) - 1

    def ref_ll(mask):
        k = bin(mask).count("1")
        _, ln_new, _, done = ref.subset_em(mat, cohort["wts"], mask, numpy.full(k, 1.0 / k), tolerance, max_iter)
        lnp = numpy.full(ld, -numpy.inf)
        lnp[ref.mask_columns(mask)] = ln_new
        assert done == 1
        return float(ref.exact_loglik(mat, lnp, cohort["wts"], mask))
    top = ref_ll(full)
    return {hap: 2.0 * (top - ref_ll(full & ~(1 << c))) for c, hap in enumerate(names)}


def test_golden_samples_end_to_end(cohort):
    """g8, g14 and g6 as one batch through support_many(models="add-one", n_extra=2).  The CPU reference is asked first whether
    g8 and g6 give non-negative drop-one lrts at args.tolerance = 1e-4.  THEY DO NOT: g8's three and g6's three true
    contributors are far above 0 (700 / 331 / 20.5 and 327 / 271 / 19.9), but g6's two columns that nothing supports come out
    at -0.11 (A13) and -0.0025 (L2a1[2][1]) -- both fits stop 1e-4 short of their maxima, and the full fit of five columns
    stops further from its own than the fit of four.  So this test runs at tolerance 1e-8, finish_many and support_many
    alike.  (At 1e-4 the full fit also stands 8.3e-5 (g8) and 5.6e-4 (g6) from refined["props"]: each loop stops short of
    the common maximum from its own start.)"""
    from mixemt_amd import assign, stats
    samples, haps = cohort["samples"], cohort["haps"]
    index = {h: i for i, h in enumerate(haps)}
    loose = finish_args(tolerance=E2E_TOLERANCES[0])
    at_loose = cohort["finish"](loose.tolerance)
    true = [c[1] for c in at_loose[0]["contribs"]]
    lowest = []
    for s in (0, 2):
        lrts = _reference_drop_one(cohort, at_loose[s], loose.tolerance, loose.max_iter)
        print("reference at tolerance", loose.tolerance, "sample", s, "drop-one lrt", lrts)
        assert all(lrts[hap] > 0 for hap in lrts if hap in true or hap == "M9a'b"), (s, lrts)
        lowest.append(min(lrts.values()))
    args = finish_args(tolerance=E2E_TOLERANCES[0] if min(lowest) >= 0 else E2E_TOLERANCES[1])
    print("lowest reference drop-one lrt at", loose.tolerance, ":", min(lowest), "-> the test runs at tolerance", args.tolerance)
    finished = cohort["finish"](args.tolerance)
    assert [c[1] for c in finished[0]["contribs"]] == true

    numpy.random.seed(21)
    mark = numpy.random.random()
    numpy.random.seed(21)
    sup, skipped = assign.support_many(samples, finished, haps, args, models="add-one", n_extra=2)
    assert numpy.random.random() == mark                                    # the global stream was not advanced
    assert skipped == [] and all(x is not None for x in sup)
    for s, (one, fin) in enumerate(zip(sup, finished)):
        k = len(fin["contribs"])
        extras = [haps[int(h)] for h in fin["vote_order"] if haps[int(h)] not in [c[1] for c in fin["contribs"]]][:2]
        assert sorted(one["columns"], key=index.get) == one["columns"] and set(one["columns"]) == set(c[1] for c in fin["contribs"]) | set(extras)
        assert one["truncated_extras"] == [] and one["n_eff"] == float(numpy.sum(cohort["wts"]))
        assert len(one["models"]) == 1 + (k if k > 1 else 0) + len(extras)
        full = one["models"][0]
        assert set(full["names"]) == set(c[1] for c in fin["contribs"])
        print("sample", s, "max |full fit - refined|", _full_fit_gap(one, fin), "iterations", [fit["iters"] for fit in one["models"]],
              "refinement", fin["refined"]["iters"])
        # the full fit is the refinement from another start: the same proportions to 1e-6 (not the same bits)
        assert _full_fit_gap(one, fin) < 1e-6, (s, _full_fit_gap(one, fin))
        for fit in one["models"]:
            assert fit["done"] == 1 and abs(fit["props"].sum() - 1.0) < 1e-12 and numpy.isfinite(fit["loglik"]) and fit["loglik"] < 0
            assert fit["bic"] == ref.bic(fit["loglik"], len(fit["names"]), one["n_eff"]) and fit["aic"] == ref.aic(fit["loglik"], len(fit["names"]))
        assert one["best_bic"] == min(range(len(one["models"])), key=lambda i: one["models"][i]["bic"])
        if k == 1:                                                          # g14: the full fit only, nothing to leave out
            assert one["drop"] == [] and full["props"].tolist() == [1.0] and full["iters"] == 1
        else:
            assert [row[:3] for row in one["drop"]] == fin["contribs"]
            for j, row in enumerate(one["drop"]):
                left = one["models"][1 + j]
                assert set(left["names"]) == set(full["names"]) - {row[1]}
                assert row[3] == 2.0 * (full["loglik"] - left["loglik"]) and row[4] == ref.lrt_p(row[3])
                print("sample", s, "drop", row)
                if row[1] in true or row[1] == "M9a'b":                   # (g6 names g8's M9b by its parent M9a'b)
                    assert row[3] > 0, row
        assert [row[0] for row in one["add"]] == extras
        for j, row in enumerate(one["add"]):
            more = one["models"][len(one["models"]) - len(extras) + j]
            assert row[2] == 2.0 * (more["loglik"] - full["loglik"]) and row[3] == ref.lrt_p(row[2])
            assert row[1] == more["props"][more["names"].index(row[0])]
            print("sample", s, "add", row)
    # the best model by BIC of g8 holds every true contributor (the smallest drop-one lrt, M9b's, is above log n_eff = 7.1)
    assert set(true) <= set(sup[0]["models"][sup[0]["best_bic"]]["names"])
    # the report, line for line against the format restated
    out = io.StringIO()
    stats.report_support_many(out, finished, sup, titles=["g8", "g14", "g6"])
    text = ""
    for s, title in enumerate(("g8", "g14", "g6")):
        text += "# %s\n" % title
        rows = {row[0]: row for row in sup[s]["drop"]}
        for con in finished[s]["contribs"]:
            text += ("%s\t%s\t%.4f\t%.4f\t%.3g\n" % tuple(rows[con[0]])) if con[0] in rows else ("%s\t%s\t%.4f\tNA\tNA\n" % tuple(con))
        text += "".join("add\t%s\t%.4f\t%.4f\t%.3g\n" % tuple(row) for row in sup[s]["add"])
        best = sup[s]["models"][sup[s]["best_bic"]]
        text += "best_bic\t%s\t%.4f\n" % (",".join(best["names"]), best["bic"])
    assert out.getvalue() == text and text.count("\n") == 3 + 9 + 6 + 3
    print(text)
    # the one-sample form is the same call on a list of one; a sample without `refined` is skipped and reported with NA
    one, why = assign.support(samples[2][0], samples[2][1], finished[2], haps, args, models="add-one", n_extra=2)
    assert why is None and [m["loglik"] for m in one["models"]] == [m["loglik"] for m in sup[2]["models"]]
    mixed, skipped = assign.support_many(samples[:2], [dict(finished[0], refined=None), finished[1]], haps, args)
    assert mixed[0] is None and [s for s, _ in skipped] == [0] and mixed[1]["models"][0]["loglik"] == sup[1]["models"][0]["loglik"]
