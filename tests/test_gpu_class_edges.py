"""
The four producers of what the EM loop iterates over, at their exact class limits, with rows made to order
(tests/_class_rows.py; tests/test_class_rows.py proves on the CPU that "exactly 256" is exactly 256):

  A  mxm_encode_rows     D = 1, 2, 255, 256 | 257, 258, 1023, 1024 | 1025 distinct bit patterns, the longest probe chains,
                         both zeros, NaN payloads, -inf, the all-ones pattern -- and every record consumer over them
  B  mxm_build_quads     Q = 1, 255, 256 | 257, H / 4 distinct aligned quads, both encoders
  C  the marker build    n = 10, 63, 64 | 65, 127, 128 | 129 sites; K = 254 .. 256, 351, 352 | 353 and 255, 256, 703, 704 |
                         705, 1023, 1024 masks; E = 1024 | 1025 and 4096 | 4097, 5120 | 5121 marker entries -- dense and
                         records variants, and the records they make through the quad encoders and the consumers

References: the row's own bits (records, decode, gather), numpy.argmax (votes), the C oracle (matrix build, posterior)
and the long-double pass of tests/_exact.py under the accuracy module's rule (EM sums).  A record is read only through
tests/_guarded_abi.records.
"""
import ctypes

import numpy
import pytest

import _class_rows as cr
import _exact
import _guarded_abi as ga
from conftest import em_args
from oracle import c_oracle, em_oracle

pytestmark = pytest.mark.gpu

U = _exact.U


# ---------------------------------------------------------------- plumbing shared by the three parts
def _weights(n_rows):
    """1 .. 4 and one zero."""
    wts = numpy.random.default_rng(500 + n_rows).integers(1, 5, size=n_rows).astype(numpy.float64)
    if n_rows > 2:
        wts[n_rows // 3] = 0.0
    return wts


def _same_bits(a, b):
    return numpy.array_equal(cr.bits(a), cr.bits(b))


def _plan_records(plan, what):
    """{row: (codes, P table, log table)} of a coded plan, through the one reader of the layout."""
    rec, rec_off, ndist = (x.cpu().numpy() for x in plan._coded_keep[:3])
    recs, _ = ga.records(rec, rec_off, ndist, plan.n_haps, len(rec), what)
    return {r: (codes, ptab, mtab) for r, codes, ptab, mtab in recs}, ndist


def _decode(plan):
    """The coded rows' P (mxm_decode_rows); rows without a record stay NaN."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream
    out = torch.full((plan.n_rows, plan.n_haps), float("nan"), dtype=torch.float64, device=plan.dev)
    _lib.check(plan.lib.mxm_decode_rows(ctypes.byref(plan.coded), plan.n_haps, out.data_ptr(), out.stride(0), current_stream()),
               "mxm_decode_rows")
    return out.cpu().numpy()


def _iterated_matrix(plan):
    """The linearised matrix the plan's iteration reads, as the device holds it: decoded records + the dense rest."""
    import torch
    lin = _decode(plan)
    if plan.coded_rest:
        idx = torch.nonzero(plan.coded_ndist == 0).flatten().cpu().numpy()
        lin[idx] = plan._coded_keep[3][:, :plan.n_haps].cpu().numpy()
    assert numpy.isfinite(lin).all()
    return lin


def _em_iter(plan, props):
    """One pass for the restarts props[B][H]; colsum starts as NaN (every entry must be written)."""
    import torch
    from mixemt_amd import em
    p = torch.from_numpy(numpy.ascontiguousarray(props)).to(plan.dev)
    colsum = torch.full_like(p, float("nan"))
    state = em.new_state(p.shape[0], plan.dev)
    plan.em_iter(p, p.log(), state, colsum)
    torch.cuda.synchronize()
    em.read_state(state)
    return colsum.cpu().numpy()


def _prop_vectors(n_haps, n):
    rng = numpy.random.default_rng(77 + n_haps)
    return numpy.ascontiguousarray(rng.dirichlet([1.0] * n_haps, size=n))


def _check_exact(what, plan, wts, props, got):
    """tests/test_gpu_accuracy.py's rule, on the bits the kernel read: rel(T_gpu) <= 8 max(rel(T_seq), 4u) and
    <= (R + H + 8) u."""
    lin = _iterated_matrix(plan)
    for b in range(props.shape[0]):
        _exact.check_products(lin, props[b])
        exact = _exact.exact_colsum(lin, props[b], wts)
        rel_seq = _exact.rel_err(_exact.seq_colsum(lin, props[b], wts), exact)
        rel = _exact.rel_err(got[b], exact)
        print("%s restart %d: rel(T_gpu) = %.1f u, rel(T_seq) = %.1f u" % (what, b, rel / U, rel_seq / U))
        assert rel <= _exact.tight_bound(rel_seq), (what, b, rel / U, rel_seq / U)
        assert rel <= _exact.derived_bound(lin.shape[0], lin.shape[1]), (what, b, rel / U)


def _oracle_steps(mat, wts, init, n):
    theta = numpy.log(init)
    buf = numpy.empty_like(mat)
    last = theta
    with numpy.errstate(invalid="ignore", divide="ignore"):
        for _ in range(n):
            last = theta
            buf, theta = em_oracle.em_step(mat, wts, theta, buf)
    return last, buf, theta


# ================================================================ A. the dense encoder and every record consumer
def _encoder_input(n_haps, layout, order):
    mat, labels = cr.encoder_matrix(n_haps, layout)
    mat, labels = numpy.array(mat), list(labels)
    if order == "permuted":
        perm = numpy.random.default_rng(n_haps).permutation(len(mat))
        mat, labels = numpy.ascontiguousarray(mat[perm]), [labels[i] for i in perm]
    return mat, labels


ENCODER_CASES = [(h, layout, order) for h in cr.ENCODER_WIDTHS + (cr.ENCODER_ODD_WIDTH,) for layout in ("runs", "shuffled")
                 for order in ("as built", "permuted")]


@pytest.mark.parametrize("n_haps,layout,order", ENCODER_CASES)
def test_encoder_classes_records_and_tables(n_haps, layout, order):
    """ndist = D up to 1024 and 0 beyond, byte codes up to 256 and 16-bit codes beyond, stats[1] = the rows without a
    record, the log table = the row's own bit patterns each once, the P table = mxm_linearize's bits, rowmax = the dense
    plan's -- every device buffer at its documented size between guard bands."""
    from mixemt_amd import em
    mat, labels = _encoder_input(n_haps, layout, order)
    n_rows = len(mat)
    lib = ga.load_lib()
    what = "H=%d %s %s" % (n_haps, layout, order)
    limit = lib.mxm_coded_bytes(n_rows, n_haps)
    out, stats = ga.encode_rows(lib, mat, n_haps + 3, limit, what)
    ndist = out["ndist"].get(numpy.int32)
    want = numpy.array([cr.expected_ndist(row) for row in mat])
    by_label = numpy.array([0 if v in ("allones",) else (cr.n_distinct(row) if isinstance(v, str) else (v if v <= 1024 else 0))
                            for v, row in zip(labels, mat)])
    assert numpy.array_equal(want, by_label)
    print(what, "ndist", ndist.tolist())
    assert numpy.array_equal(ndist, want), (what, ndist.tolist(), want.tolist())
    n_over = sum(1 for v in labels if not isinstance(v, str) and v >= 1025)
    assert stats[1] == n_over + labels.count("allones") == int((want == 0).sum()), (what, stats)
    recs, _ = ga.records(out["rec"].get(numpy.uint8), out["rec_off"].get(numpy.int64), ndist, n_haps, limit, what)
    assert [r for r, _, _, _ in recs] == list(numpy.flatnonzero(want > 0))
    dense = em.EmPlan(mat, numpy.ones(n_rows))
    lin = dense.lin[:, :n_haps].cpu().numpy()
    assert _same_bits(out["rowmax"].get(numpy.float64), dense.rowmax.cpu().numpy()), what
    for r, codes, ptab, mtab in recs:
        assert codes.dtype == (numpy.uint8 if want[r] <= 256 else numpy.uint16), (what, r)
        assert len(mtab) == len(ptab) == want[r]
        assert numpy.array_equal(numpy.sort(cr.bits(mtab)), numpy.unique(cr.bits(mat[r]))), (what, r, labels[r])
        assert _same_bits(mtab[codes], mat[r]), (what, r, labels[r])          # -0.0 stays -0.0, NaN payloads are kept
        p_row = ptab[codes]
        nan = numpy.isnan(lin[r])
        assert numpy.array_equal(numpy.isnan(p_row), nan) and _same_bits(p_row[~nan], lin[r][~nan]), (what, r, labels[r])


def _coded_matrix(plan, mat_d):
    import torch
    from mixemt_amd import preprocess
    rest = torch.nonzero(plan.coded_ndist == 0).flatten()
    return preprocess.CodedMatrix(plan.n_rows, plan.n_haps, *plan._coded_keep[:3], plan.rowmax, 0, rest,
                                  mat_d[rest].contiguous())


def _tie_partner(ln, row, first, later, top):
    """ln[first], ln[later] such that ln[c] + row[c] == top in fp64 for both.  top = 300 and |row| < 80: the terms and the
    sums lie in [256, 512), one spacing of 2^-44 throughout, so stepping the term by one spacing moves the sum's exact
    value through every rounding interval -- one of a few steps of nextafter lands on top."""
    for c in (first, later):
        guess = top - row[c]
        for step in range(-8, 9):
            cand = guess
            for _ in range(abs(step)):
                cand = numpy.nextafter(cand, numpy.inf if step > 0 else -numpy.inf)
            if cand + row[c] == top:
                ln[c] = cand
                break
        else:
            raise AssertionError("no fp64 term makes the tie exact")


@pytest.mark.parametrize("n_haps,layout,order", ENCODER_CASES)
def test_record_consumers_over_the_limit_rows(n_haps, layout, order):
    """decode, gather, argmax + votes + first-seen order over the whole matrix (NaN rows included: numpy's semantics are
    defined there); the limit rows' LAST table entry wins, their FIRST one wins, and a tie between the last entry's
    column and a later one goes to the first."""
    import torch
    from mixemt_amd import assign, em, preprocess
    mat, labels = _encoder_input(n_haps, layout, order)
    n_rows = len(mat)
    what = "H=%d %s %s" % (n_haps, layout, order)
    wts = _weights(n_rows)
    plan = em.EmPlan(mat, wts, storage="coded")
    assert plan.storage == "coded" and plan.coded is not None
    recs, ndist = _plan_records(plan, what)
    want_nd = numpy.array([cr.expected_ndist(row) for row in mat])
    assert numpy.array_equal(ndist, want_nd)
    assert plan.coded_wide == int((want_nd > 256).sum()) and plan.coded_rest == int((want_nd == 0).sum())
    dense = em.EmPlan(mat, wts)
    lin = dense.lin[:, :n_haps].cpu().numpy()
    # mxm_decode_rows
    dec = _decode(plan)
    for r in numpy.flatnonzero(want_nd > 0):
        nan = numpy.isnan(lin[r])
        assert numpy.array_equal(numpy.isnan(dec[r]), nan) and _same_bits(dec[r][~nan], lin[r][~nan]), (what, r, labels[r])
    assert _same_bits(plan.rowmax.cpu().numpy(), dense.rowmax.cpu().numpy())
    cm = _coded_matrix(plan, dense.mat)
    limit_labels = cr.ENCODER_LIMIT_D + ("collide256", "collide1024", "zeros")
    limit_rows = [labels.index(v) for v in limit_labels if v in labels]              # (the first row of each kind)
    assert len(limit_rows) == (len(limit_labels) if n_haps != cr.ENCODER_ODD_WIDTH else 2)
    # mxm_gather_columns_coded: the columns that hold code nd - 1 and code 0 of every limit row, the row's ends
    cols = {0, n_haps - 1}
    where = {}
    for r in limit_rows:
        codes = recs[r][0]
        last_col, first_col = int(numpy.argmax(codes == want_nd[r] - 1)), int(numpy.argmax(codes == 0))
        assert codes[last_col] == want_nd[r] - 1 and codes[first_col] == 0
        where[r] = (last_col, first_col)
        cols.update((last_col, first_col))
    cols = sorted(cols)
    haps = ["h%d" % i for i in range(n_haps)]
    sub, _ = preprocess.reduce_em_records(cm, haps, [["x", haps[c], 0.0] for c in cols])
    assert _same_bits(sub.cpu().numpy(), mat[:, cols]), what
    # mxm_row_argmax_votes_coded + mxm_first_seen
    def votes(ln, label):
        with numpy.errstate(invalid="ignore"):
            want_best = (ln[None, :] + mat).argmax(axis=1)
        best, got_votes = assign.row_argmax_votes_records(cm, ln, wts)
        assert numpy.array_equal(best, want_best), (what, label, numpy.flatnonzero(best != want_best).tolist(),
                                                    [labels[i] for i in numpy.flatnonzero(best != want_best)])
        assert numpy.array_equal(got_votes, numpy.bincount(want_best, weights=wts, minlength=n_haps)), (what, label)
        order_got, votes_tab = assign.vote_table_from_records(cm, ln, wts)
        assert numpy.array_equal(order_got, assign._first_seen_order(want_best)), (what, label)
        assert numpy.array_equal(votes_tab, got_votes)
        return want_best
    rng = numpy.random.default_rng(n_haps + 5)
    background = rng.uniform(-3.0, 0.0, size=n_haps)
    votes(background, "background")
    for r in limit_rows:
        last_col, first_col = where[r]
        for col, label in ((last_col, "last entry"), (first_col, "first entry")):
            ln = background.copy()
            ln[col] = 200.0                                           # |M| < 80: a clear margin
            assert votes(ln, (labels[r], label))[r] == col
        # a tie between the last entry's column and a later one: the first wins.  Where that column IS the row's last
        # (the 256 colliding keys at H = 1028: the entry's one run ends the row) the partner is an earlier column, and wins.
        partner = (last_col + n_haps) // 2 if last_col < n_haps - 1 else n_haps // 2
        assert partner != last_col and (partner > last_col) == (last_col < n_haps - 1)
        ln = background.copy()
        _tie_partner(ln, mat[r], last_col, partner, 300.0)
        sums = ln + mat[r]
        assert sums[last_col] == sums[partner] == sums.max() == 300.0 and (sums == 300.0).sum() == 2
        assert votes(ln, (labels[r], "tie"))[r] == min(last_col, partner)


@pytest.mark.parametrize("n_haps,layout,order", ENCODER_CASES)
def test_em_forms_over_the_limit_rows(n_haps, layout, order):
    """mxm_em_iter_coded with one restart and three, the one-launch records loop (even widths), mxm_em_step_coded -- over
    the matrix without its two NaN rows."""
    import torch
    from mixemt_amd import em
    mat, labels = _encoder_input(n_haps, layout, order)
    keep = [r for r, v in enumerate(labels) if v not in cr.ENCODER_NAN_ROWS]
    mat = numpy.ascontiguousarray(mat[keep])
    n_rows = len(mat)
    assert not numpy.isnan(mat).any() and n_rows == len(labels) - (2 if n_haps != cr.ENCODER_ODD_WIDTH else 0)
    what = "H=%d %s %s" % (n_haps, layout, order)
    wts = _weights(n_rows)
    plan = em.EmPlan(mat, wts, storage="coded")
    assert plan.coded is not None and plan.coded_rest == sum(1 for r in keep if labels[r] == 1025)
    props = _prop_vectors(n_haps, 3)
    one = _em_iter(plan, props[:1])
    three = _em_iter(plan, props)
    assert plan.restart_tile() == plan.lib.mxm_restart_tile_coded(ctypes.byref(plan.coded), n_haps)
    assert numpy.array_equal(one[0], three[0])                        # a restart's sums do not depend on its neighbours
    _check_exact(what, plan, wts, props, three)
    # the posterior from the records' log tables: the oracle's em_step, test_gpu_coded.py's bound
    dense = em.EmPlan(mat, wts)
    rec_plan = em.EmPlan(None, wts, records=_coded_matrix(plan, dense.mat))
    ln = numpy.log(props[0])
    last, post_want, _ = _oracle_steps(mat, wts, props[0], 1)
    post = em.posterior(rec_plan, ln).cpu().numpy()
    finite = numpy.isfinite(post_want)
    assert numpy.array_equal(numpy.isfinite(post), finite) and numpy.abs(post[finite] - post_want[finite]).max() < 1e-10
    # The whole loop in one launch.  It takes records only (the rows of 1025 values stay out), and a shape it does not take
    # goes to the per-iteration kernels WITHOUT a word, mxm_set_loop_fused(1) or not: its grid is min(R, 5.2 sqrt(R) in
    # whole eights) workgroups, and a workgroup's slice of the H / 2 column pairs must not exceed 64 -- at H = 5408 that
    # asks for 43 workgroups, i.e. 63 rows and more.  So the loop gets the record rows three times over (as they are,
    # permuted, reversed: 84 rows, 48 workgroups), and the test PROVES the route: with the test hook that makes a
    # one-launch loop give up at its first grid barrier, mode 1 must return -3 -- the per-iteration kernels would not.
    if n_haps % 2 == 0:
        coded_rows = numpy.array([r for r in range(n_rows) if cr.expected_ndist(mat[r]) > 0])
        assert len(coded_rows) == 28
        stack = numpy.concatenate([coded_rows, numpy.random.default_rng(n_haps + 9).permutation(coded_rows), coded_rows[::-1]])
        loop_mat, loop_wts = numpy.ascontiguousarray(mat[stack]), numpy.ascontiguousarray(wts[stack])
        lib = plan.lib
        try:
            lib.mxm_set_loop_fused(1, 0)
            lib.mxm_diag_fused_force_abort(1)
            loop_plan = em.EmPlan(loop_mat, loop_wts, storage="coded")
            assert loop_plan.coded is not None and loop_plan.coded_rest == 0
            with pytest.raises(ValueError, match="one-launch loop"):
                em.em_loop(loop_plan, props[:1], 0.0, 3)
            lib.mxm_diag_fused_force_abort(0)
            res = em.run_em_ex(loop_mat, loop_wts, em_args(max_iter=3, tolerance=0.0), inits=props[:1], storage="coded",
                               want_read_mix=False)
        finally:
            lib.mxm_diag_fused_force_abort(0)
            lib.mxm_set_loop_fused(-1, 0)
        _, _, theta = _oracle_steps(loop_mat, loop_wts, props[0], 3)
        assert res["storage"] == "coded" and res["iters"] == [3]
        assert numpy.abs(res["props"] - numpy.exp(theta)).max() < 1e-12


# ================================================================ B. the quad encoders
def _code_dwords(codes, n_haps):
    """A byte-coded record's code array as the quad encoders see it: ldc / 4 dwords, pad bytes 0."""
    ldc = (n_haps + 7) // 8 * 8
    padded = numpy.zeros(ldc, dtype=numpy.uint8)
    padded[:n_haps] = codes
    return padded.view("<u4")


def _build_quads(plan, kind):
    """mxm_build_quads + mxm_quad_lists with encoder `kind`, straight through the C ABI -> (qrec, qoff, nquad, stats,
    quad_rows, byte_rows) on the host."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream
    lib, dev, n_rows, n_haps = plan.lib, plan.dev, plan.n_rows, plan.n_haps
    _lib.check(lib.mxm_set_quad_encoder(kind), "mxm_set_quad_encoder")
    cap = lib.mxm_quad_bytes(n_rows, n_haps)
    qrec = torch.zeros(cap, dtype=torch.uint8, device=dev)
    qoff = torch.full((n_rows,), -7, dtype=torch.int64, device=dev)
    nquad = torch.full((n_rows,), -7, dtype=torch.int32, device=dev)
    stats = torch.full((2,), -7, dtype=torch.int64, device=dev)
    _lib.check(lib.mxm_build_quads(ctypes.byref(plan.coded), n_haps, qrec.data_ptr(), cap, qoff.data_ptr(), nquad.data_ptr(),
                                   stats.data_ptr(), current_stream()), "mxm_build_quads")
    quad_rows = torch.full((n_rows,), -1, dtype=torch.int64, device=dev)
    byte_rows = torch.full((n_rows,), -1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    sbytes = lib.mxm_quad_lists_scratch_bytes(n_rows)
    scratch = torch.empty(max(1, (sbytes + 7) // 8), dtype=torch.int64, device=dev)
    _lib.check(lib.mxm_quad_lists(plan._coded_keep[2].data_ptr(), nquad.data_ptr(), n_rows, quad_rows.data_ptr(),
                                  byte_rows.data_ptr(), counts.data_ptr(), scratch.data_ptr(), scratch.numel() * 8,
                                  current_stream()), "mxm_quad_lists")
    torch.cuda.synchronize()
    n_q, n_b = (int(v) for v in counts.cpu())
    used, n_left = (int(v) for v in stats.cpu())
    assert used <= cap
    nquad_h, qoff_h = nquad.cpu().numpy(), qoff.cpu().numpy()
    blobs = {}
    for r in numpy.flatnonzero(nquad_h > 0):
        o, n = int(qoff_h[r]), int(nquad_h[r])
        assert o % 32 == 0 and 0 <= o and o + 2048 + 32 * n <= cap
        blobs[int(r)] = qrec[o:o + 2048 + 32 * n].cpu().numpy()
    return blobs, nquad_h, n_left, quad_rows.cpu().numpy()[:n_q], byte_rows.cpu().numpy()[:n_b]


def _check_quads(plan, recs, ndist, what, generator_q=None):
    """Both encoders over the plan's records.  Expected counts are formed in CODE space from the read-back records (pad
    bytes 0): Q distinct code dwords -> nquad = Q up to 256, else 0.  -> {row: Q} of the byte-coded rows."""
    n_rows, n_haps = plan.n_rows, plan.n_haps
    nqc = ((n_haps + 7) // 8 * 8) // 4
    byte_coded = numpy.flatnonzero((ndist > 0) & (ndist <= 256))
    q_of = {}
    for r in byte_coded:
        q_of[int(r)] = len(numpy.unique(_code_dwords(recs[r][0], n_haps)))
    want_nquad = numpy.zeros(n_rows, dtype=numpy.int32)
    for r, q in q_of.items():
        want_nquad[r] = q if q <= 256 else 0
    if generator_q is not None:
        # value space against code space: equal where the codes fill whole quads; with pad columns inside the last 8
        # (H = 1028: ldc = 1032) the all-pad quad (0, 0, 0, 0) is one more unless the row holds it anyway
        for r, q in generator_q.items():
            pad_quad = nqc * 4 - n_haps >= 4
            assert q_of[r] in ((q, q + 1) if pad_quad else (q,)), (what, r, q, q_of[r])
    dec = _decode(plan)
    got = {}
    try:
        for kind in (0, 1):
            blobs, nquad, n_left, quad_rows, byte_rows = _build_quads(plan, kind)
            label = "%s encoder %d" % (what, kind)
            print(label, "nquad", nquad.tolist()[:24], "Q", [q_of.get(r, -1) for r in range(min(24, n_rows))])
            assert numpy.array_equal(nquad, want_nquad), (label, numpy.flatnonzero(nquad != want_nquad).tolist())
            assert numpy.array_equal(quad_rows, numpy.flatnonzero(want_nquad > 0)), label
            assert numpy.array_equal(byte_rows, numpy.array([r for r in byte_coded if want_nquad[r] == 0], dtype=numpy.int64)), label
            assert n_left == len(byte_rows), label
            for r, blob in blobs.items():
                codes, ptab, _ = recs[r]
                dwords = _code_dwords(codes, n_haps)
                uniq = numpy.unique(dwords)                                    # ascending order of the code dword
                n = len(uniq)
                qcodes = blob[:2048].reshape(256, 8)                           # [thread][j]: quad t + 256 j
                quad_code = numpy.zeros(nqc, dtype=numpy.int64)
                for j in range(8):
                    idx = numpy.arange(256) + 256 * j
                    ok = idx < nqc
                    quad_code[idx[ok]] = qcodes[ok, j]
                    assert (qcodes[~ok, j] == 0).all(), (label, r)
                assert numpy.array_equal(quad_code, numpy.searchsorted(uniq, dwords)), (label, r)
                table = blob[2048:].view(numpy.float64).reshape(n, 4)
                want_table = numpy.stack([ptab[(uniq >> (8 * e)) & 255] for e in range(4)], axis=1)
                assert _same_bits(table, want_table), (label, r)
                assert _same_bits(table[quad_code].reshape(-1)[:n_haps], dec[r]), (label, r)
            got[kind] = blobs
    finally:
        plan.lib.mxm_set_quad_encoder(1)
    assert got[0].keys() == got[1].keys()
    for r, blob in got[0].items():
        assert numpy.array_equal(blob, got[1][r]), (what, r)
    return q_of


def _check_quad_iteration(plan_factory, wts, what):
    """One restart and three with the dictionary attached against the iteration without it (3e-15 relative to the largest
    sum, the quad modules' bound) and against the long-double pass under the accuracy rule."""
    plain = plan_factory()
    props = _prop_vectors(plain.n_haps, 3)
    base = _em_iter(plain, props)
    quad = plan_factory()
    attached = quad.attach_quads(True)
    assert attached, what                                 # every matrix here has rows of at most 256 quads
    assert quad.coded.n_quad_rows > 0
    one = _em_iter(quad, props[:1])
    three = _em_iter(quad, props)
    for b in range(3):
        assert (numpy.abs(three[b] - base[b]) / numpy.abs(base[b]).max()).max() < 3e-15, (what, b)
    assert (numpy.abs(one[0] - base[0]) / numpy.abs(base[0]).max()).max() < 3e-15, what
    _check_exact(what + " quads x1", quad, wts, props[:1], one)
    _check_exact(what + " quads x3", quad, wts, props, three)
    return True


@pytest.mark.parametrize("n_rows", cr.QUAD_ROW_COUNTS)
@pytest.mark.parametrize("n_haps", cr.QUAD_WIDTHS)
def test_quad_encoders_at_256_and_257_quads(n_haps, n_rows):
    from mixemt_amd import em
    mat, kinds = cr.quad_matrix(n_haps, n_rows)
    mat = numpy.array(mat)
    what = "H=%d R=%d" % (n_haps, n_rows)
    wts = _weights(n_rows)
    plan = em.EmPlan(mat, wts, storage="coded")
    recs, ndist = _plan_records(plan, what)
    want_nd = numpy.array([0 if k == "none" else (300 if k == "wide" else k[0]) for k in kinds])
    assert numpy.array_equal(ndist, want_nd)
    generator_q = {r: k[1] for r, k in enumerate(kinds) if not isinstance(k, str)}
    q_of = _check_quads(plan, recs, ndist, what, generator_q)
    if n_rows == 130:                                    # whichever way the pad quad falls (H = 1028), rows of exactly 256
        assert 256 in q_of.values() and 257 in q_of.values()          # and of exactly 257 code-space quads occur
        if n_haps % 8 == 0:
            assert {1, 255, 256, 257, n_haps // 4} <= set(q_of.values())
    assert _check_quad_iteration(lambda: em.EmPlan(mat, wts, storage="coded"), wts, what)


def test_quad_count_with_a_partial_last_quad():
    """H = 2050: the last quad holds two columns and two pad bytes; what the encoders must count is taken from the
    records' read-back codes, not from the generator."""
    from mixemt_amd import em
    n_haps = 2050
    rng = numpy.random.default_rng(2050)
    rows = []
    for d, q in ((4, 200), (16, 255), (16, 256), (16, 257), (64, 256), (200, 300), (3, 40)):
        head = cr.rows_with_quads(2048, d, [q], 2050 + q)[0]
        tail = head[rng.integers(0, 2048, size=2)]                   # two more columns of the row's own values
        rows.append(numpy.concatenate([head, tail]))
    rows.append(cr.rows_with_values(n_haps, [300], 1)[0])
    mat = numpy.ascontiguousarray(numpy.stack(rows))
    wts = _weights(len(mat))
    plan = em.EmPlan(mat, wts, storage="coded")
    recs, ndist = _plan_records(plan, "H=2050")
    q_of = _check_quads(plan, recs, ndist, "H=2050")
    assert min(q_of.values()) <= 256 < max(q_of.values())
    assert _check_quad_iteration(lambda: em.EmPlan(mat, wts, storage="coded"), wts, "H=2050")


# ================================================================ C. the marker build, dense and records
MARKER_CASES = [(h, part, dyadic) for h in cr.MARKER_WIDTHS for part in ("short", "long") for dyadic in (False, True)]
_marker = {}


def _marker_input(n_haps, part, dyadic):
    """tables, CSR, the C oracle's matrix, the facts of every row -- made once per case, never written to."""
    key = (n_haps, part, dyadic)
    if key not in _marker:
        tables, (row_ptr, site, obs), case_of_row = cr.marker_input(n_haps, part, dyadic)
        want = c_oracle.build_em_matrix(tables.expected, tables.lhit, tables.lmiss, row_ptr, site, obs, n_haps)
        want.setflags(write=False)
        cases = cr.marker_case_list(n_haps, part)
        facts = []
        for r, c in enumerate(case_of_row):
            sl = slice(row_ptr[r], row_ptr[r + 1])
            if r > 0 and case_of_row[r - 1] == c and c >= 0:
                facts.append(facts[-1])
                continue
            n, k, e, n_values = cr.row_facts(tables, site[sl], obs[sl])
            if c >= 0:                                                # the facts are the intended ones
                assert (n, k) == cases[c][:2] and (cases[c][2] is None or e == cases[c][2]), (cases[c], n, k, e)
                assert cases[c][2] is not None or not 64 < n <= 128 or e <= cr.LONG_MAX_ENTRIES     # (the masks decide)
            assert n_values == cr.n_distinct(want[r])
            facts.append((n, k, e, n_values))
        _marker[key] = (tables, (row_ptr, site, obs), want, facts)
    return _marker[key]


@pytest.fixture(scope="module", autouse=True)
def _release_inputs():
    yield
    _marker.clear()


@pytest.mark.parametrize("n_haps,part,dyadic", MARKER_CASES)
def test_dense_marker_build_at_the_site_mask_and_entry_limits(n_haps, part, dyadic):
    """Every kernel gives the C oracle's bits; the fallback list holds exactly the rows past a documented limit."""
    from mixemt_amd import preprocess
    tables, (row_ptr, site, obs), want, facts = _marker_input(n_haps, part, dyadic)
    what = "H=%d %s %s" % (n_haps, part, "dyadic" if dyadic else "generic")
    lib = ga.load_lib()
    for long_rows in (1, 0):
        assert lib.mxm_set_sparse_long_rows(long_rows) == 0
        got = preprocess.build_em_matrix_device(tables, row_ptr, site, obs, kernel="sparse").cpu().numpy()
        left = preprocess.build_em_matrix_device.last_fallback
        classes = [cr.marker_class(n, k, e, long_rows=bool(long_rows)) for n, k, e, _ in facts]
        print(what, "long rows", long_rows, "fallback", left, "of", len(facts), "expected", classes.count("fallback"))
        bad = numpy.flatnonzero((cr.bits(got) != cr.bits(want)).any(axis=1))
        assert len(bad) == 0, (what, long_rows, bad.tolist(), [facts[r] for r in bad])
        assert left == classes.count("fallback"), (what, long_rows, left, classes.count("fallback"))
    lib.mxm_set_sparse_long_rows(1)
    for kernel in ("lut", "bytes"):
        got = preprocess.build_em_matrix_device(tables, row_ptr, site, obs, kernel=kernel).cpu().numpy()
        assert _same_bits(got, want), (what, kernel)


def _decode_cm(cm):
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream
    out = torch.full((cm.n_rows, cm.n_haps), float("nan"), dtype=torch.float64, device=cm.rec.device)
    coded = cm.struct()
    _lib.check(_lib.load().mxm_decode_rows(ctypes.byref(coded), cm.n_haps, out.data_ptr(), out.stride(0), current_stream()),
               "mxm_decode_rows")
    return out.cpu().numpy()


@pytest.mark.parametrize("with_dense", [True, False])
@pytest.mark.parametrize("n_haps,part,dyadic", MARKER_CASES)
def test_records_marker_build_at_the_limits(n_haps, part, dyadic, with_dense):
    """Kernel-made records hold one entry per mask (byte codes up to 256 entries, 16-bit codes up to 353 / 705); a row
    past a limit gets the ENCODER's record, one entry per distinct value; a row of more than 1024 values stays dense."""
    from mixemt_amd import em, preprocess
    tables, (row_ptr, site, obs), want, facts = _marker_input(n_haps, part, dyadic)
    what = "H=%d %s %s dense=%s" % (n_haps, part, "dyadic" if dyadic else "generic", with_dense)
    n_rows = len(want)
    if with_dense:
        cm, mat = preprocess.build_em_records_device(tables, row_ptr, site, obs, dense=True)
        assert _same_bits(mat.cpu().numpy(), want), what
    else:
        cm = preprocess.build_em_records_device(tables, row_ptr, site, obs)
    classes = [cr.marker_class(n, k, e) for n, k, e, _ in facts]
    assert preprocess.build_em_matrix_device.last_fallback == classes.count("fallback"), what
    nd = cm.ndist_host()
    want_nd = numpy.array([k + 1 if cls != "fallback" else (v if v <= 1024 else 0) for (n, k, e, v), cls in zip(facts, classes)])
    print(what, "ndist", nd.tolist())
    assert numpy.array_equal(nd, want_nd), (what, numpy.flatnonzero(nd != want_nd).tolist())
    rest = cm.rest_rows.cpu().numpy()
    assert numpy.array_equal(rest, numpy.flatnonzero(want_nd == 0))
    assert _same_bits(cm.m_rest.cpu().numpy(), want[rest]), what
    if not dyadic:
        assert len(rest) == sum(1 for n, k, e, v in facts if v > 1024)
        assert (len(rest) > 0) == (part == "long")                    # the generic rows of 1025 values
    else:
        assert len(rest) == 0                                         # 1025 masks, three values: a byte record
    rec = cm.rec.cpu().numpy()
    recs, _ = ga.records(rec, cm.rec_off.cpu().numpy(), nd, n_haps, int(cm.capacity), what)
    dense_plan = em.EmPlan(numpy.array(want), numpy.ones(n_rows))
    lin = dense_plan.lin[:, :n_haps].cpu().numpy()                    # mxm_linearize's bits
    rowmax = cm.rowmax.cpu().numpy()
    kernel_wide = 0
    for r, codes, ptab, mtab in recs:
        assert codes.dtype == (numpy.uint8 if want_nd[r] <= 256 else numpy.uint16), (what, r, facts[r])
        assert _same_bits(mtab[codes], want[r]) and _same_bits(ptab[codes], lin[r]), (what, r, facts[r])
        assert rowmax[r] == want[r].max(), (what, r)
        sl = slice(row_ptr[r], row_ptr[r + 1])
        if classes[r] != "fallback":                                  # one entry per mask, equal sums repeated
            assert numpy.array_equal(numpy.sort(cr.bits(mtab)), cr.mask_values(tables, site[sl], obs[sl], want[r])), (what, r)
            kernel_wide += int(want_nd[r] > 256)
        else:                                                         # the encoder: each value once
            assert numpy.array_equal(numpy.sort(cr.bits(mtab)), numpy.unique(cr.bits(want[r]))), (what, r)
    assert kernel_wide > 0
    dec = _decode_cm(cm)
    coded = want_nd > 0
    assert _same_bits(dec[coded], lin[coded]), what


@pytest.mark.parametrize("n_haps,part", [(h, part) for h in cr.MARKER_WIDTHS for part in ("short", "long")])
def test_build_made_records_with_repeated_entries_through_the_consumers(n_haps, part):
    """Dyadic tables: records of 256 entries that hold three to five distinct values -- the only place where a table with
    repeated entries meets the quad encoders (which de-duplicate by CODE), the iteration and the argmax."""
    from mixemt_amd import assign, em, preprocess
    tables, (row_ptr, site, obs), want, facts = _marker_input(n_haps, part, True)
    what = "H=%d %s build-made" % (n_haps, part)
    n_rows = len(want)
    cm = preprocess.build_em_records_device(tables, row_ptr, site, obs)
    nd = cm.ndist_host()
    wts = _weights(n_rows)
    plan = em.EmPlan(None, wts, records=cm)
    recs, ndist = _plan_records(plan, what)
    full = [r for r in recs if ndist[r] == 256]
    assert full and all(len(numpy.unique(cr.bits(recs[r][2]))) <= 5 for r in full)       # 256 entries, a handful of values
    q_of = _check_quads(plan, recs, ndist, what)
    for r in full:                                       # counted by code, not by value: far more quads than value quads
        assert q_of[r] >= cr.n_quads(want[r][:n_haps // 4 * 4])
    assert _check_quad_iteration(lambda: em.EmPlan(None, wts, records=cm), wts, what)
    # one iteration against the dense matrix's, test_gpu_coded.py's bound; the argmax against numpy's on the oracle's matrix
    props = _prop_vectors(n_haps, 1)
    a = _em_iter(em.EmPlan(numpy.array(want), wts), props)
    b = _em_iter(plan, props)
    assert float((numpy.abs(a - b) / numpy.abs(a)).max()) < 1e-12
    rng = numpy.random.default_rng(n_haps)
    for _ in range(2):
        ln = rng.uniform(-30.0, 0.0, size=n_haps)
        best, votes = assign.row_argmax_votes_records(cm, ln, wts)
        want_best = (ln[None, :] + want).argmax(axis=1)
        assert numpy.array_equal(best, want_best), what
        assert numpy.array_equal(votes, numpy.bincount(want_best, weights=wts, minlength=n_haps))
