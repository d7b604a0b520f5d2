"""
Every EM LOOP over many iterations against the trajectory reference (tests/_exact_traj.py), into underflow.

tests/test_gpu_accuracy.py holds one pass of every form to ulp level; the loops it runs at max_iter = 1.  Here each loop
form runs K = 2, 3, 10 and 40 iterations (tol = 0: done == 2 and iters == K are asserted) -- K = 2 takes the carry from
iteration k to k + 1 once, K = 3 with state that was itself carried -- and its state is held to the long-double trajectory
on the bits the kernel reads (u = 2^-53, the maximum over the entries whose exact value is finite):

    max_h |ln_new - ln_exact,K|      <= 8 * max(err_seq(K), K u max(1, max |ln_exact,K|))   (ln_cur alike, at K - 1)
    |state.l1 - l1_exact,K|          <= 8 * max(the comparison pass's own l1 error, K u max |ln| + H u)
    colsum (where the form leaves it): test_gpu_accuracy's rule on T, against T_K; (R + H + 8) u, a bound for one pass from
                                     identical inputs, plus the ln bound at K - 1 by which pass K's inputs have moved
    props_cur against exp(ln_exact,K-1): relative error <= the ln bound at K - 1 plus 4 u wherever the exact proportion
                                     is a normal number, and at most the smallest normal number elsewhere.  The one-launch
                                     loops carry p as p T / tot (never re-derived from the log state): their proportions
                                     are held to this where they were normal numbers at every step, and measured where
                                     they had been subnormal (up to 100 % off: the LIMIT in mixemt_hip_tuning.h)

err_seq: the same recurrence in plain fp64 (sequential sums; oracle.em_oracle.em_step for the log-space widths).  Proportion
vectors: "dirichlet", "skewed" and "deep" (ln p ~ U(-760, -690): subnormal and zero in linear space, with more crossing
-745 while the loop runs); the precondition that replaces check_products for "deep" is asserted on the device's bits.
The stop decision is taken from the reference: K* and tol from _exact_traj.stop_point on the exact l1, and every form must
report done == 1 and iters == K* (the pairs whose l1 leaves no usable stop are pinned in tests/test_exact_traj.py).
Restarts that share passes start from different vectors and one tol under the three schedules; many samples each follow
their own trajectory.  The last test makes the header's documented limit of the EM pass a test.

MXM_ACCURACY_REPORT=<file> makes the module write its figures to <file>.loops (tools/accuracy_report.py).
"""
import ctypes
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy
import pytest

import _accuracy_inputs as inputs
import _exact
import _exact_traj as traj
import test_gpu_accuracy as one_pass

pytestmark = pytest.mark.gpu

U = _exact.U
STEPS = inputs.LOOP_STEPS
K_MAX = max(STEPS)
TINY = float(numpy.finfo(numpy.float64).tiny)
_refs = {}
_rows = {}                                              # (form, H, vector) -> {K: (error, err_seq, floor)}
_drift = {}                                             # (form, H, vector, K) -> props_cur's relative error (held, once subnormal)


# ---------------------------------------------------------------- references, made once per (bits of the matrix, vector)
def _digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = numpy.ascontiguousarray(a)
        h.update(str((a.shape, a.dtype)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


_pool = ThreadPoolExecutor(max_workers=8)              # references side by side: numpy's loops release the GIL


def _ref_start(X, props, ln, wts, log_space=False, steps=K_MAX):
    """Start the exact trajectory and the comparison pass from (X, ln) -- X = the device's linearised matrix, or the log
    matrix -- unless they are there already; _ref collects them."""
    key = (_digest(X, props, ln, wts), log_space, steps)
    if key not in _refs:
        if log_space:
            exact = _pool.submit(traj.exact_trajectory, X, ln, wts, steps, log_space=True)
            seq = _pool.submit(traj.oracle_trajectory, X, ln, wts, steps)
        else:
            if (props == 0).any() or (props[props > 0] < TINY).any():
                traj.deep_precondition(X, ln)
            else:
                _exact.check_products(X, props)
            exact = _pool.submit(traj.exact_trajectory, X, ln, wts, steps, props0=props)
            seq = _pool.submit(traj.seq_trajectory, X, ln, wts, steps, props0=props)
        _refs[key] = {"exact": exact, "seq": seq, "shape": X.shape, "props0": numpy.asarray(props)}
    return key


def _ref(X, props, ln, wts, log_space=False, steps=K_MAX):
    hit = _refs[_ref_start(X, props, ln, wts, log_space, steps)]
    for name in ("exact", "seq"):
        if not isinstance(hit[name], traj.Trajectory):
            hit[name] = hit[name].result()
    return hit


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    _refs.clear()
    path = os.environ.get("MXM_ACCURACY_REPORT")
    if not path:
        return
    with open(path + ".loops", "w") as out:
        out.write("| form | H | proportions | " + " | ".join("K = %d: loop / comparison pass" % k for k in STEPS) + " |\n")
        out.write("|---|---|---|" + "---|" * len(STEPS) + "\n")
        for (form, n_haps, vec), per_k in _rows.items():
            cells = []
            for k in STEPS:
                if k in per_k:
                    err, err_seq, floor = per_k[k]
                    cells.append("%.2f / %.2f" % (err / floor, err_seq / floor) if floor else "0 / 0")
                else:
                    cells.append("-")
            out.write("| %s | %d | %s | %s |\n" % (form, n_haps, vec, " | ".join(cells)))
        out.write("\nThe linear proportions a one-launch loop carries, `props_cur` against `exp(ln_exact)` at K = 40, \"deep\" vector "
                  "(largest relative error):\n\n| form | H | never subnormal on the way | subnormal or zero on the way |\n|---|---|---|---|\n")
        for (form, n_haps, vec, k), (held, rest) in _drift.items():
            if k == K_MAX and vec == "deep":
                out.write("| %s | %d | %.2g | %.2g |\n" % (form, n_haps, held, rest))


# ---------------------------------------------------------------- running a loop
class Run(object):
    pass


def _loop(who, props, ln, tol, max_iter, narrow=None, check_every=16):
    """mxm_em_loop / _f32 / _coded / _samples (/ _samples_narrow: narrow = (M device, ld, ncol)) from the given arrays."""
    import torch
    from mixemt_amd import _lib, em
    from mixemt_amd._dev import current_stream
    lib, dev = who.lib, who.dev
    n_runs, n_haps = props.shape
    props_cur, ln_cur = torch.from_numpy(props.copy()).to(dev), torch.from_numpy(ln.copy()).to(dev)
    ln_new = ln_cur.clone()
    colsum = torch.full_like(props_cur, float("nan"))
    state = em.new_state(n_runs, dev)
    host_state = (_lib.EmState * n_runs)()
    loop = (float(tol), int(max_iter), int(check_every))
    tail = (who.ws.data_ptr(), who.ws_bytes, current_stream(), host_state)
    head = (props_cur.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(), colsum.data_ptr(), state.data_ptr())
    if narrow is not None:
        m_d, ld, ncol = narrow
        e_buf = torch.empty((who.n_rows, ld), dtype=torch.float64, device=dev)
        _lib.check(lib.mxm_em_loop_samples_narrow(ctypes.byref(who.coded), who.row0_ptr, n_runs, who.n_haps, m_d.data_ptr(), ld,
                                                  ncol.ctypes.data_as(ctypes.c_void_p), who.wts.data_ptr(), props_cur.data_ptr(),
                                                  ln_cur.data_ptr(), ln_new.data_ptr(), state.data_ptr(), *loop, e_buf.data_ptr(),
                                                  *tail), "mxm_em_loop_samples_narrow")
    elif isinstance(who, em.SampleBatch):
        _lib.check(lib.mxm_em_loop_samples(ctypes.byref(who.coded), who.row0_ptr, who.n_entries, who.wts.data_ptr(), n_haps, *head,
                                           *loop, *tail), "mxm_em_loop_samples")
    elif who.coded is not None:
        _lib.check(lib.mxm_em_loop_coded(ctypes.byref(who.coded), who.wts.data_ptr(), n_haps, n_runs, *head, *loop, *tail),
                   "mxm_em_loop_coded")
    elif who.storage == "f32":
        p_ptr, ldp = who.lin_args()
        _lib.check(lib.mxm_em_loop_f32(p_ptr, ldp, who.wts.data_ptr(), who.n_rows, n_haps, n_runs, *head, *loop, *tail),
                   "mxm_em_loop_f32")
    else:
        m_ptr, ldm = who.mat_args()
        p_ptr, ldp = who.lin_args()
        _lib.check(lib.mxm_em_loop(m_ptr, ldm, p_ptr, ldp, who.wts.data_ptr(), who.n_rows, n_haps, n_runs, *head, *loop, *tail),
                   "mxm_em_loop")
    torch.cuda.synchronize()
    run = Run()
    run.ln_cur, run.ln_new, run.props_cur, run.colsum = (t.cpu().numpy() for t in (ln_cur, ln_new, props_cur, colsum))
    run.states = [(s.done, s.iters, s.l1) for s in host_state]
    assert [s[:2] for s in run.states] == [s[:2] for s in em.read_state(state)]
    return run


def _by_hand(plan, props, ln, tol, max_iter):
    """max_iter hand-made {mxm_em_iter; mxm_m_finalize} steps."""
    import torch
    from mixemt_amd import em
    p, lnc = torch.from_numpy(props.copy()).to(plan.dev), torch.from_numpy(ln.copy()).to(plan.dev)
    ln_new = lnc.clone()
    colsum = torch.full_like(p, float("nan"))
    state = em.new_state(p.shape[0], plan.dev)
    for _ in range(max_iter):
        plan.em_iter(p, lnc, state, colsum)
        plan.finalize(colsum, lnc, ln_new, p, state, tol, max_iter)
    torch.cuda.synchronize()
    run = Run()
    run.ln_cur, run.ln_new, run.props_cur, run.colsum = (t.cpu().numpy() for t in (lnc, ln_new, p, colsum))
    run.states = em.read_state(state)
    return run


def _same_bits(a, b, colsum=True):
    eq = lambda x, y: numpy.array_equal(one_pass._bits(x), one_pass._bits(y))
    return (eq(a.ln_cur, b.ln_cur) and eq(a.ln_new, b.ln_new) and eq(a.props_cur, b.props_cur)
            and (not colsum or eq(a.colsum, b.colsum))
            and [(d, i, numpy.float64(l).view(numpy.int64)) for d, i, l in a.states]
            == [(d, i, numpy.float64(l).view(numpy.int64)) for d, i, l in b.states])


# ---------------------------------------------------------------- the rule
def _check(form, run, b, ref, k, done, vec, colsum, ncol=None, record=True, carried=None):
    """Restart / sample b of `run` against its trajectory at step k (its first ncol columns).  carried: the form keeps its
    linear proportions as p T / tot from iteration to iteration (the one-launch loops; default: the forms without colsum)."""
    carried = (not colsum) if carried is None else carried
    exact, seq = ref["exact"], ref["seq"]
    n_rows, n_haps = ref["shape"]
    cut = slice(0, n_haps if ncol is None else ncol)
    assert run.states[b][:2] == (done, k), (form, vec, k, run.states[b])
    err_seq, l1_seq = traj.seq_errors(exact, seq, k)
    err = traj.ln_error(run.ln_new[b][cut], exact.ln[k])
    floor, bound = traj.ln_floor(exact.ln[k], k), traj.ln_bound(err_seq, exact.ln[k], k)
    l1_err = abs(float(_exact.LD(run.states[b][2]) - exact.l1[k]))
    l1_bound = traj.l1_bound(l1_seq, exact.ln[k], k)
    print("%-52s H=%-5d %-10s K=%-2d ln_new error %.3g (%.2f floors; comparison pass %.3g, bound %.3g) | l1 %.3g: error %.3g (bound %.3g)"
          % (form, n_haps, vec, k, err, err / floor if floor else 0.0, err_seq, bound, run.states[b][2], l1_err, l1_bound))
    if record and done == 2:
        _rows.setdefault((form, n_haps, vec), {})[k] = (err, err_seq, floor)
    assert err <= bound, (form, n_haps, vec, k, err, err_seq, bound)
    assert l1_err <= l1_bound, (form, n_haps, vec, k, l1_err, l1_seq, l1_bound)
    if k >= 2:                                         # ln_cur = log theta_{K-1}, props_cur its linear copy
        prev_bound = traj.ln_bound(traj.seq_errors(exact, seq, k - 1)[0], exact.ln[k - 1], k - 1)
        err_cur = traj.ln_error(run.ln_cur[b][cut], exact.ln[k - 1])
        assert err_cur <= prev_bound, (form, n_haps, vec, k, "ln_cur", err_cur, prev_bound)
        p_exact = numpy.exp(exact.ln[k - 1])
        normal = p_exact >= TINY
        got = run.props_cur[b][cut].astype(_exact.LD)
        rel_p = numpy.abs(got / numpy.where(normal, p_exact, 1) - 1)
        # a carried proportion is held to the rule only if it was a normal number at every step so far: one that has been
        # subnormal has lost bits the product p T / tot never gets back, one that reached 0 stays there (the documented
        # limit of the one-launch loops, mixemt_hip_tuning.h) -- those are measured, and must stay within [0, 2 p_exact]
        held = normal.copy()
        if carried:
            held &= (numpy.exp(exact.ln[:k]) >= TINY).all(axis=0) & (ref["props0"] >= TINY)
        drift = float(rel_p[held].max()) if held.any() else 0.0
        rest = float(rel_p[normal & ~held].max()) if (normal & ~held).any() else 0.0
        print("   props_cur against exp(ln_exact): relative error %.3g (bound %.3g)%s"
              % (drift, prev_bound + 4 * U, "; %.3g where the carried proportion had been subnormal" % rest if carried else ""))
        assert drift <= prev_bound + 4 * U, (form, n_haps, vec, k, "props_cur", drift, prev_bound)
        assert rest <= 1.0, (form, n_haps, vec, k, "props_cur", rest)
        assert (run.props_cur[b][cut][~normal] <= TINY).all() and (run.props_cur[b][cut] >= 0).all()
        if carried and done == 2 and record:
            _drift[(form, n_haps, vec, k)] = (drift, rest)
    if colsum:
        T = {"exact": exact.T[k], "rel_seq": _exact.rel_err(seq.T[k], exact.T[k])}
        rel = _exact.rel_err(run.colsum[b][cut], T["exact"])
        print("   colsum: rel(T_gpu) = %.1f u, rel(T_seq) = %.1f u" % (rel / U, T["rel_seq"] / U))
        assert rel <= _exact.tight_bound(T["rel_seq"]), (form, n_haps, vec, k, rel / U, T["rel_seq"] / U)
        # derived_bound is one pass from IDENTICAL inputs; pass K reads proportions that K - 1 steps have moved by up to the
        # ln bound d (a relative error d of p_h): Z_r moves by at most d relatively, and so does every term of T (first order)
        before = traj.ln_bound(traj.seq_errors(exact, seq, k - 1)[0], exact.ln[k - 1], k - 1) if k >= 2 else 0.0
        assert rel <= _exact.derived_bound(n_rows, n_haps) + before, (form, n_haps, vec, k, rel / U, before / U)


# the (width, vector) pairs whose reference l1 has no usable stop within 40 iterations (_exact_traj.stop_point), on the loop
# matrices and on the first 96 reads alike (tests/test_exact_traj.py pins the same for the host-linearised loop matrices):
# everywhere else a form MUST take its stop test -- at K* = 2 on the real rows, at K* = 3, 6 or 7 on the log-space widths
NO_USABLE_STOP = {66: ("dirichlet",), 1025: ("dirichlet",), 5408: ("dirichlet", "skewed"), 8200: ("dirichlet",)}


def _one_restart_form(form, who, X, vecs, wts, colsum, log_space=False, steps=STEPS, stop=True):
    """Every vector as a run of its own: K in `steps` with tol = 0, then the stop decision from the reference.
    -> {(vector, K): Run}."""
    out = {}
    for props, ln in vecs.values():
        _ref_start(X, props, ln, wts, log_space)
    for vec, (props, ln) in vecs.items():
        ref = _ref(X, props, ln, wts, log_space)
        for k in steps:
            run = out[(vec, k)] = _loop(who, props[None, :], ln[None, :], 0.0, k)
            _check(form, run, 0, ref, k, 2, vec, colsum)
        k_stop, tol = traj.stop_point(ref["exact"].l1)
        assert (k_stop is None) == (vec in NO_USABLE_STOP.get(X.shape[1], ())), (form, X.shape[1], vec, k_stop)
        if stop and k_stop is not None:
            run = _loop(who, props[None, :], ln[None, :], tol, K_MAX)
            _check(form + " (stop)", run, 0, ref, k_stop, 1, vec, colsum, record=False)
    return out


def _takes_one_launch(plan, props, ln):
    """Whether mxm_set_loop_fused(1 / 2) really sends this plan through a one-launch loop (an ineligible shape goes to the
    per-iteration kernels without a word): with the library's test hook raised, such a launch gives up, which mode 1 / 2
    reports as error -3."""
    plan.lib.mxm_diag_fused_force_abort(1)
    try:
        _loop(plan, props[None, :], ln[None, :], 0.0, 2)
    except ValueError as exc:
        assert "(-3)" in str(exc), exc
        return True
    finally:
        plan.lib.mxm_diag_fused_force_abort(0)
    return False


def _lin_of(plan):
    return numpy.ascontiguousarray(plan.lin[:, :plan.n_haps].cpu().numpy())


# ---------------------------------------------------------------- mxm_em_loop over the dense fp64 matrix
@pytest.mark.parametrize("n_haps", inputs.LOOP_WIDTHS_REAL)
def test_dense_loops(b17, n_haps):
    """Per-iteration kernels (mode 0: K steps by hand, to the bit), the one-launch loop with the columns split (mode 1) and
    with the rows split (mode 2); the latter two cut into launches of 1 and 3 iterations continue bit for bit."""
    from mixemt_amd import em
    label, mat, wts = inputs.loop_matrix(b17, n_haps)
    plan = em.EmPlan(mat, wts)
    assert plan.storage == "f64" and plan.lin is not None and plan.coded is None
    lin, vecs = _lin_of(plan), inputs.loop_vectors(n_haps)
    plan.lib.mxm_set_loop_fused(0, 0)
    runs = _one_restart_form("mxm_em_loop, per-iteration kernels", plan, lin, vecs, wts, True)
    for (vec, k), run in runs.items():
        props, ln = vecs[vec]
        assert _same_bits(run, _by_hand(plan, props[None, :], ln[None, :], 0.0, k)), (vec, k)
    for mode, form in ((1, "mxm_em_loop, one launch, columns split"), (2, "mxm_em_loop, one launch, rows split")):
        plan.lib.mxm_set_loop_fused(mode, 0)
        assert _takes_one_launch(plan, *vecs["skewed"])
        runs = _one_restart_form(form, plan, lin, vecs, wts, False)
        for chunk in (1, 3):
            plan.lib.mxm_set_loop_fused(mode, chunk)
            for (vec, k), run in runs.items():
                props, ln = vecs[vec]
                again = _loop(plan, props[None, :], ln[None, :], 0.0, k)
                assert _same_bits(run, again, colsum=False), (mode, chunk, vec, k)


@pytest.mark.parametrize("n_haps", [66, 5408])
def test_fp32_storage_loop(b17, n_haps):
    """mxm_em_loop_f32, referenced on the FLOAT matrix's bits."""
    import torch
    from mixemt_amd import em
    label, mat, wts = inputs.loop_matrix(b17, n_haps)
    plan = em.EmPlan(mat, wts, storage="f32")
    assert plan.storage == "f32" and plan.lin.dtype == torch.float32
    lin = _lin_of(plan)
    assert lin.dtype == numpy.float32
    _one_restart_form("mxm_em_loop_f32", plan, lin, inputs.loop_vectors(n_haps), wts, True)


@pytest.mark.parametrize("n_haps", inputs.LOOP_WIDTHS_LOG)
def test_log_space_loops(b17, n_haps):
    """Matrices without a linear copy: the narrow one-launch loop (its instances end at 16 columns: H = 3 and 16; wider
    matrices take the per-iteration kernels under every mode, which mode 1 is run to show) and the per-iteration log-space
    kernels (the narrow one up to 64 columns, the generic one beyond 8192)."""
    from mixemt_amd import em
    label, mat, wts = inputs.loop_matrix(b17, n_haps)
    plan = em.EmPlan(mat, wts)
    assert plan.lin is None and plan.coded is None and not plan.lib.mxm_linear_supported(n_haps)
    vecs = inputs.loop_vectors(n_haps)
    plan.lib.mxm_set_loop_fused(0, 0)
    per_iter = _one_restart_form("mxm_em_loop, log space, per-iteration kernels", plan, mat, vecs, wts, True, log_space=True)
    plan.lib.mxm_set_loop_fused(1, 0)
    assert _takes_one_launch(plan, *vecs["skewed"]) == (n_haps <= 16)
    if n_haps <= 16:
        fused = _one_restart_form("mxm_em_loop, narrow one-launch loop", plan, mat, vecs, wts, False, log_space=True)
        plan.lib.mxm_set_loop_fused(1, 3)
        for (vec, k), run in fused.items():
            props, ln = vecs[vec]
            assert _same_bits(run, _loop(plan, props[None, :], ln[None, :], 0.0, k), colsum=False), (vec, k)
    else:
        for (vec, k), run in per_iter.items():
            props, ln = vecs[vec]
            assert _same_bits(run, _loop(plan, props[None, :], ln[None, :], 0.0, k)), (vec, k)


# ---------------------------------------------------------------- mxm_em_loop_coded
@pytest.mark.parametrize("quads", [False, True])
@pytest.mark.parametrize("n_haps", [1025, 5408])
def test_records_loops(b17, n_haps, quads):
    """Records alone and beside a quad dictionary.  Per-iteration kernels on the loop matrix (at 5408 its 4000-bp rows are a
    dense rest); the one-launch loop -- even widths, no dense rest -- on the first 96 reads at 5408 with the default grid and
    at 66 under both grid settings of test_gpu_coded.py.  An odd width has no one-launch loop over records.  Every route is
    proven (_takes_one_launch)."""
    label, mat, wts = inputs.loop_matrix(b17, n_haps)
    vecs = inputs.loop_vectors(n_haps)
    plan = one_pass._coded_plan(mat, wts)
    if quads:
        assert plan.attach_quads(True) and plan.coded.n_quad_rows > 0
    else:
        assert plan.coded.n_quad_rows == 0
    plan.lib.mxm_set_loop_fused(0, 0)
    tag = ", quads" if quads else ""
    _one_restart_form("mxm_em_loop_coded, per-iteration kernels" + tag, plan, one_pass._decoded(plan), vecs, wts, True)
    if n_haps & 1:
        plan.lib.mxm_set_loop_fused(1, 0)
        assert not _takes_one_launch(plan, *vecs["skewed"])
        return
    # (96 rows get min(96, 5.2 sqrt(96)) = 56 workgroups at most, and a workgroup's slice holds 64 column pairs: 5408
    # columns need 43 workgroups -- the grid settings 8 and 40 have a one-launch loop at H = 66 only)
    for width, grid in ((n_haps, 0), (66, 8), (66, 40)):
        mat = numpy.array(inputs.real_rows(b17, width, "reads")[:inputs.LOOP_ROWS])
        plan = one_pass._coded_plan(mat, wts)
        assert plan.coded_rest == 0
        if quads:
            assert plan.attach_quads(True) and plan.coded.n_quad_rows > 0
        lin, vecs = one_pass._decoded(plan), inputs.loop_vectors(width)
        plan.lib.mxm_set_loop_fused(1, 0)
        plan.lib.mxm_set_fused_coded_grid(grid)
        assert _takes_one_launch(plan, *vecs["skewed"]), (width, grid)
        form = "mxm_em_loop_coded, one launch%s%s" % (tag, ", %d workgroups" % grid if grid else "")
        runs = _one_restart_form(form, plan, lin, vecs, wts, False, stop=grid == 0)
        plan.lib.mxm_set_loop_fused(1, 3)
        for (vec, k), run in runs.items():
            props, ln = vecs[vec]
            assert _same_bits(run, _loop(plan, props[None, :], ln[None, :], 0.0, k), colsum=False), (width, grid, vec, k)


# ---------------------------------------------------------------- several restarts, three schedules
RESTART_MAX_ITER = 12


def _restarts(form, plan, X, wts, vecs, names, tile=None):
    """B = 4 from different vectors under one tol (from the reference: _exact_traj.common_tol), schedules 0 / 1 / 2, the
    states read back every 2 iterations (check_every = 2: below every stop, so schedule 2 deals its full tile of three
    round-robin chunk by chunk, and a restart is resumed after its tile-mates had their turn, a stopped one staying frozen
    across them): each restart against its own trajectory at its own end; a stopped restart's state bit-identical across
    the schedules."""
    props, ln = one_pass._stack(vecs, names)
    refs = [_ref(X, props[b], ln[b], wts) for b in range(4)]
    tol, ends = traj.common_tol([r["exact"].l1[:RESTART_MAX_ITER + 1] for r in refs])
    print("%s: tol = %.3g, (iterations, done) = %s" % (form, tol, ends))
    assert len(set(ends[:3])) >= 2 and any(d == 1 for _, d in ends[:3])          # the tile of three loses a member on the way
    first = None
    for sched in (0, 1, 2):
        plan.lib.mxm_set_loop_fused(0, 0)
        plan.lib.mxm_set_compact_restarts(sched)
        if tile is not None:
            plan.lib.mxm_set_batch_tile(tile)
            assert plan.restart_tile() == tile
        run = _loop(plan, props, ln, tol, RESTART_MAX_ITER, check_every=2)
        for b, vec in enumerate(names):
            _check("%s, schedule %d" % (form, sched), run, b, refs[b], ends[b][0], ends[b][1], vec, False, record=False,
                   carried=False)
        if first is None:
            first = run
        for b in [b for b, (_, done) in enumerate(ends) if done == 1]:       # a stopped restart: the same bits under every schedule
            assert run.states[b] == first.states[b], (sched, b)          # (the others may meet other tile-mates, i.e. another
            for name in ("ln_cur", "ln_new", "props_cur"):               # kernel instance and summation order, on their way)
                assert numpy.array_equal(one_pass._bits(getattr(run, name)[b]), one_pass._bits(getattr(first, name)[b])), (sched, b, name)
    return ends


def test_four_dense_restarts_under_every_schedule(b17):
    """Four restarts with the tile held to three (mxm_set_batch_tile: at this width four would share one pass) -- schedules
    0 and 1 spread them evenly, 2 + 2, schedule 2 deals ONE tile of three round-robin over the four -- on a few-values
    matrix: its l1 moves enough for restarts to stop apart (iterations 3, 7 and max_iter; on the real rows l1 falls by a
    few per cent per iteration after the second one, and no later iteration is a usable stop)."""
    from mixemt_amd import em
    n_haps = 1025
    mat, wts = numpy.array(inputs.few_values(inputs.LOOP_ROWS, n_haps)), inputs.weights(inputs.LOOP_ROWS)
    plan = em.EmPlan(mat, wts, n_runs=4)
    assert plan.lin is not None and plan.restart_tile() == 4
    vecs = inputs.loop_vectors(n_haps)
    vecs["deep2"] = inputs.deep_vector(n_haps, seed=1, head=(0.05, 0.9))
    ends = _restarts("mxm_em_loop, B = 4", plan, _lin_of(plan), wts, vecs, ("deep", "dirichlet", "deep2", "skewed"), tile=3)
    assert len(set(ends)) >= 3 and min(k for k, _ in ends) > 2


def test_four_restarts_over_records_and_quads_under_every_schedule(b17):
    """A tile of three through em_iter_quad_batched_kernel and a single restart, on the real rows: two members of the
    tile stop at the second iteration (the only usable stop these rows offer), the third runs on alone."""
    n_haps = 5408
    label, mat, wts = inputs.loop_matrix(b17, n_haps)
    plan = one_pass._coded_plan(mat, wts, n_runs=4)
    assert plan.attach_quads(True) and plan.coded.n_quad_rows > 0 and plan.restart_tile() == 3
    vecs = inputs.loop_vectors(n_haps)
    vecs["deep, head 0.01"] = inputs.deep_vector(n_haps, seed=2, head=(0.01, 0.01))
    vecs["dirichlet2"] = inputs.prop_vectors(n_haps, seed=1)["dirichlet"]
    _restarts("mxm_em_loop_coded, quads, B = 4", plan, one_pass._decoded(plan), wts, vecs,
              ("deep, head 0.01", "dirichlet", "deep", "dirichlet2"))


# ---------------------------------------------------------------- many samples
LOOP_SAMPLE_VECTORS = ("skewed", "deep", "dirichlet", "deep", "skewed")


@pytest.mark.parametrize("n_haps", [66, 5408])
def test_many_samples_loop(b17, n_haps):
    """mxm_em_loop_samples on test_gpu_accuracy's ragged batch: every sample against its own trajectory, and each stops
    where its own reference does under the batch's one tol."""
    batch, _, samples, keep = one_pass._ragged_batch(b17, n_haps)
    vecs = inputs.loop_vectors(n_haps)
    props, ln = one_pass._stack(vecs, LOOP_SAMPLE_VECTORS)
    for s, (label, mat, wts, lin) in reversed(list(enumerate(samples))):           # (the tallest first)
        _ref_start(lin, props[s], ln[s], wts)
    refs = [_ref(lin, props[s], ln[s], wts) for s, (label, mat, wts, lin) in enumerate(samples)]
    for k in STEPS:
        run = _loop(batch, props, ln, 0.0, k)
        for s, vec in enumerate(LOOP_SAMPLE_VECTORS):
            _check("mxm_em_loop_samples, sample of %d rows" % samples[s][3].shape[0], run, s, refs[s], k, 2, vec, True)
    tol, ends = traj.common_tol([r["exact"].l1[:RESTART_MAX_ITER + 1] for r in refs])
    print("samples: tol = %.3g, (iterations, done) = %s" % (tol, ends))
    assert {d for _, d in ends} == {1, 2}                 # some sample stops on the way, the others run on beside it
    run = _loop(batch, props, ln, tol, RESTART_MAX_ITER, check_every=2)
    for s, vec in enumerate(LOOP_SAMPLE_VECTORS):
        _check("mxm_em_loop_samples (stop)", run, s, refs[s], ends[s][0], ends[s][1], vec, True, record=False)


def test_many_samples_narrow_loop(b17):
    """mxm_em_loop_samples_narrow: one workgroup per sample over 1 .. 8 of its columns (ld = 8); the "deep" samples have 5
    and 8 columns, so that deep_vector leaves 2 and 5 entries deep beside the three it sets; the stop under one tol."""
    import torch
    n_haps, ld = 5408, 8
    _, finish, samples, keep = one_pass._ragged_batch(b17, n_haps)
    ncol = numpy.array([1, 5, 2, 8, 3], dtype=numpy.int32)
    cols = [0, n_haps // 2, n_haps - 1, 1, 2, 3, 4, 5]
    n_rows = sum(len(s[1]) for s in samples)
    red = numpy.full((n_rows, ld), -numpy.inf)
    props, ln = numpy.zeros((len(samples), ld)), numpy.full((len(samples), ld), -numpy.inf)
    subs, at = [], 0
    for s, (label, mat, wts, _) in enumerate(samples):
        n = int(ncol[s])
        subs.append(numpy.ascontiguousarray(mat[:, cols[:n]]))
        red[at:at + len(mat), :n] = subs[-1]
        vec = LOOP_SAMPLE_VECTORS[s]
        if vec == "deep":                              # (the first draw that leaves a subnormal or zero proportion among so few)
            props[s, :n], ln[s, :n] = next(v for v in (inputs.deep_vector(n, seed=i) for i in range(16)) if (v[0] < TINY).any())
        else:
            props[s, :n], ln[s, :n] = inputs.prop_vectors(n)[vec]
        at += len(mat)
    refs = [_ref(subs[s], props[s, :ncol[s]], ln[s, :ncol[s]], samples[s][2], log_space=True) for s in range(len(samples))]
    m_d = torch.from_numpy(red).to(finish.dev)
    for k in STEPS:
        run = _loop(finish, props, ln, 0.0, k, narrow=(m_d, ld, ncol))
        for s, vec in enumerate(LOOP_SAMPLE_VECTORS):
            _check("mxm_em_loop_samples_narrow, %d columns" % ncol[s], run, s, refs[s], k, 2, vec, False, ncol=int(ncol[s]))
    tol, ends = traj.common_tol([r["exact"].l1[:RESTART_MAX_ITER + 1] for r in refs[1:]])     # (one column: l1 = 0 from step 2)
    print("narrow samples: tol = %.3g, (iterations, done) = %s" % (tol, ends))
    assert any(d == 1 for _, d in ends)
    run = _loop(finish, props, ln, tol, RESTART_MAX_ITER, narrow=(m_d, ld, ncol), check_every=2)
    assert run.states[0][0] == 1
    for s, vec in list(enumerate(LOOP_SAMPLE_VECTORS))[1:]:
        _check("mxm_em_loop_samples_narrow (stop)", run, s, refs[s], ends[s - 1][0], ends[s - 1][1], vec, False, ncol=int(ncol[s]),
               record=False)


# ---------------------------------------------------------------- the documented limit of the linear form
def _limit_problem(b17):
    """96 x 66: row 5 is -inf outside columns 7 and 40, whose ln p is -800 -- every supporter of a non-empty row has
    underflowed in linear space."""
    label, mat, wts = inputs.loop_matrix(b17, 66)
    props, ln = inputs.prop_vectors(66)["skewed"]
    ln = ln.copy()
    keep = mat[5, [7, 40]].copy()
    mat[5, :] = -numpy.inf
    mat[5, [7, 40]] = keep
    ln[[7, 40]] = -800.0
    wts = wts.copy()
    wts[5] = 2.0
    return mat, wts, numpy.exp(ln), ln


def test_documented_limit_of_the_em_pass(b17):
    """include/mixemt_hip.h, mxm_em_iter: "LIMIT of every form of this pass".  Every loop form is loud -- NaN proportions,
    done == 2, iters == max_iter -- never a silently dropped row; with weight 0 the row is dropped and the run is inside
    the rule; in a batch the row poisons its own sample and no other."""
    from mixemt_amd import em
    mat, wts, props, ln = _limit_problem(b17)
    assert (props[[7, 40]] == 0).all()
    dropped = wts.copy()
    dropped[5] = 0.0
    forms = []
    for mode in (0, 1, 2):
        forms.append(("mxm_em_loop, mode %d" % mode, mode, lambda w: em.EmPlan(mat, w)))
    forms.append(("mxm_em_loop_f32", 0, lambda w: em.EmPlan(mat, w, storage="f32")))
    forms.append(("mxm_em_loop_coded, per-iteration", 0, lambda w: one_pass._coded_plan(mat, w)))
    forms.append(("mxm_em_loop_coded, one launch", 1, lambda w: one_pass._coded_plan(mat, w)))
    for form, mode, make in forms:
        plan = make(wts)
        plan.lib.mxm_set_loop_fused(mode, 0)
        assert _takes_one_launch(plan, props, ln) == (mode != 0), form     # (no silent fall-back to the per-iteration kernels)
        run = _loop(plan, props[None, :], ln[None, :], 0.0, 3)
        print("%-36s weight 2: state %s, NaN in ln_new: %d of %d" % (form, run.states[0], numpy.isnan(run.ln_new).sum(), run.ln_new.size))
        assert run.states[0][:2] == (2, 3) and numpy.isnan(run.ln_new).all() and numpy.isnan(run.props_cur).all(), form
        plan = make(dropped)
        plan.lib.mxm_set_loop_fused(mode, 0)
        X = _lin_of(plan) if plan.lin is not None else one_pass._decoded(plan)
        ref = _ref(numpy.delete(X, 5, axis=0), props, ln, numpy.delete(dropped, 5))      # (dropped: the problem without it)
        run = _loop(plan, props[None, :], ln[None, :], 0.0, 3)
        _check(form + ", the row's weight 0", run, 0, ref, 3, 2, "limit", False, record=False)
    # many samples: the row poisons its own sample, no other
    rows = [0, 40, 96]
    plan = one_pass._coded_plan(mat, wts)
    assert plan.coded_rest == 0
    rec, rec_off, ndist = plan._coded_keep[:3]
    batch = em.SampleBatch(rec, rec_off, ndist, plan.wts, numpy.array(rows, dtype=numpy.int64), 66)
    both = numpy.ascontiguousarray(numpy.stack([props, props])), numpy.ascontiguousarray(numpy.stack([ln, ln]))
    run = _loop(batch, both[0], both[1], 0.0, 3)
    assert [s[:2] for s in run.states] == [(2, 3), (2, 3)]
    assert numpy.isnan(run.ln_new[0]).all() and numpy.isfinite(run.ln_new[1]).all()
    lin = one_pass._decoded(plan)
    _check("mxm_em_loop_samples, the clean sample", run, 1, _ref(lin[40:], props, ln, wts[40:]), 3, 2, "limit", True, record=False)
    # the kernels that stream M (here H = 64: the problem without two bystander columns) shift a row by max M, not by
    # max (ln p + M): the same limit, as loud -- the header said "of the linear form" and was corrected.  The reference's
    # log-space E-step itself, mxm_em_step, stays finite on that row and inside test_gpu_accuracy's rule.
    cols = [c for c in range(66) if c not in (1, 2)]      # (0, 33 and 65 -- the skewed vector's entries -- 7 and 40 all kept)
    sub, sub_ln = numpy.ascontiguousarray(mat[:, cols]), numpy.ascontiguousarray(ln[cols])
    assert sub.shape[1] == 64
    plan = em.EmPlan(sub, wts)
    assert plan.lin is None
    plan.lib.mxm_set_loop_fused(0, 0)
    run = _loop(plan, numpy.exp(sub_ln)[None, :], sub_ln[None, :], 0.0, 3)
    assert run.states[0][:2] == (2, 3) and numpy.isnan(run.ln_new).all() and numpy.isnan(run.props_cur).all()
    plan = em.EmPlan(sub, dropped)
    plan.lib.mxm_set_loop_fused(0, 0)
    ref = _ref(numpy.delete(sub, 5, axis=0), numpy.exp(sub_ln), sub_ln, numpy.delete(dropped, 5), log_space=True, steps=3)
    run = _loop(plan, numpy.exp(sub_ln)[None, :], sub_ln[None, :], 0.0, 3)
    _check("mxm_em_loop, H = 64, the row's weight 0", run, 0, ref, 3, 2, "limit", True, record=False)
    # ... and the narrow one-launch loop, on 16 of the columns
    cols16 = [0, 3, 4, 5, 6, 7, 8, 9, 10, 33, 40, 41, 42, 43, 44, 65]
    sub16, ln16 = numpy.ascontiguousarray(mat[:, cols16]), numpy.ascontiguousarray(ln[cols16])
    narrow = em.EmPlan(sub16, wts)
    narrow.lib.mxm_set_loop_fused(1, 0)
    assert narrow.lin is None and _takes_one_launch(narrow, numpy.exp(ln16), ln16)
    run = _loop(narrow, numpy.exp(ln16)[None, :], ln16[None, :], 0.0, 3)
    assert run.states[0][:2] == (2, 3) and numpy.isnan(run.ln_new).all() and numpy.isnan(run.props_cur).all()
    narrow = em.EmPlan(sub16, dropped)
    narrow.lib.mxm_set_loop_fused(1, 0)
    ref = _ref(numpy.delete(sub16, 5, axis=0), numpy.exp(ln16), ln16, numpy.delete(dropped, 5), log_space=True, steps=3)
    run = _loop(narrow, numpy.exp(ln16)[None, :], ln16[None, :], 0.0, 3)
    _check("mxm_em_loop, narrow one-launch loop, the row's weight 0", run, 0, ref, 3, 2, "limit", False, record=False)
    post = em.posterior(plan, sub_ln).cpu().numpy()
    exact_post = _exact.exact_posterior(sub, sub_ln)
    assert numpy.isfinite(post[5, [cols.index(7), cols.index(40)]]).all() and numpy.isneginf(numpy.delete(post[5], [cols.index(7), cols.index(40)])).all()
    with numpy.errstate(all="ignore"):                    # (-inf - -inf off the row's two supporters, in the oracle too)
        one_pass._check_posterior("mxm_em_step, the same problem", post, exact_post, one_pass._oracle_step(sub, wts, sub_ln)[0], 96, 64,
                                  "limit")
