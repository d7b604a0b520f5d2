"""
Every EM pass against the extended-precision reference (tests/_exact.py), at ulp level.

The rest of the suite compares proportions with an absolute 1e-9 / 1e-12: a relative error eps in T_h moves ln_new[h] by eps
whatever p_h is, but props[h] by p_h * eps only -- invisible for the thousands of haplogroups below 1e-9, although
ln_props[h] + M[r][h] is what the votes, the read assignment and the refinement EM consume.  Here ONE pass per form is run,
`colsum` (T, the M-step sums without their factor p_h) read back and compared under one rule for every form
(u = 2^-53, rel(X) = max_h |X_h - T_exact,h| / T_exact,h):

    rel(T_gpu) <= 8 * max(rel(T_seq), 4u)      T_seq: a plain fp64 pass in sequential order on the same inputs
    rel(T_gpu) <= (R + H + 8) * u              the first-order worst case of any summation order

The reference reads the bits the kernel reads: the linearised matrix comes back from the device (mxm_linearize's output,
mxm_decode_rows' output, the float matrix of the fp32 variant), proportions and weights are the arrays handed in.  For the
log-space forms (H <= 64, H > 8192) the comparison pass is oracle.em_oracle.em_step; both bounds hold for them as written.
The one-launch loops take no `colsum`; of them ln_new is checked, under mxm_set_loop_fused(1 / 2), which turns a launch
that cannot run into error -3 instead of a silent fall-back to the per-iteration kernels.  ln_new and the posterior are
compared absolutely: 8 x max(the fp64 oracle's own largest error, u x max |value|).

Inputs: tests/_accuracy_inputs.py.  MXM_ACCURACY_REPORT=<file> makes the module write its measured figures there as a
table (tools/accuracy_report.py -> profiles/accuracy/README.md).
"""
import ctypes
import os

import numpy
import pytest

import _accuracy_inputs as inputs
import _exact
from oracle import em_oracle

pytestmark = pytest.mark.gpu

U = _exact.U
_refs = {}
_rows = []
_exp_rows = []


# ---------------------------------------------------------------- the reference, made once per (matrix, vector)
def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and numpy.array_equal(a, b)


def _linear_ref(key, lin, props, wts):
    hit = _refs.get(key)
    if hit is None or not (_same(hit["P"], lin) and _same(hit["props"], props) and _same(hit["w"], wts)):
        _exact.check_products(lin, props)
        exact = _exact.exact_colsum(lin, props, wts)
        hit = {"P": lin, "props": props, "w": wts, "exact": exact,
               "rel_seq": _exact.rel_err(_exact.seq_colsum(lin, props, wts), exact)}
        _refs[key] = hit
    return hit


def _oracle_step(mat, wts, ln):
    """em_oracle.em_step: (posterior, ln_new, T recovered as sum_r w_r exp(post_rh - ln p_h))."""
    post, theta = em_oracle.em_step(numpy.asarray(mat), wts, ln, numpy.empty_like(mat))
    return post, theta, (numpy.exp(post - ln[None, :]) * wts[:, None]).sum(axis=0)


def _log_ref(key, mat, ln, wts):
    hit = _refs.get(key)
    if hit is None or not (_same(hit["M"], mat) and _same(hit["ln"], ln) and _same(hit["w"], wts)):
        _exact.check_products(inputs.linearise(mat), numpy.exp(ln))
        exact = _exact.exact_colsum_log(mat, ln, wts)
        _, theta, t_oracle = _oracle_step(mat, wts, ln)
        hit = {"M": mat, "ln": ln, "w": wts, "exact": exact, "theta": theta, "rel_seq": _exact.rel_err(t_oracle, exact)}
        _refs[key] = hit
    return hit


def _record(form, n_haps, n_rows, vec, rel, rel_seq, ln_err=None):
    _rows.append((form, n_haps, n_rows, vec, rel, rel_seq, ln_err))
    print("%-44s H=%-5d R=%-4d %-10s rel(T_gpu) = %s u, rel(T_seq) = %s u%s"
          % (form, n_haps, n_rows, vec, "-" if rel is None else "%.1f" % (rel / U), "-" if rel_seq is None else "%.1f" % (rel_seq / U),
             "" if ln_err is None else ", ln_new error %.3g" % ln_err))


def _check_T(form, ref, got, n_rows, n_haps, vec, ln_err=None):
    rel = _exact.rel_err(got, ref["exact"])
    _record(form, n_haps, n_rows, vec, rel, ref["rel_seq"], ln_err)
    assert rel <= _exact.tight_bound(ref["rel_seq"]), (form, n_haps, n_rows, vec, rel / U, ref["rel_seq"] / U)
    assert rel <= _exact.derived_bound(n_rows, n_haps), (form, n_haps, n_rows, vec, rel / U)


def _check_ln(form, got, exact_ln, oracle_ln, n_rows, n_haps, vec, record=True):
    """ln_new against exact_finalize, absolutely, wherever the exact value is finite (T > 0)."""
    exact_ln = numpy.asarray(exact_ln)
    ok = numpy.isfinite(exact_ln.astype(numpy.float64))
    assert ok.any() and numpy.isfinite(got[ok]).all()
    err = float(numpy.abs(got.astype(_exact.LD) - exact_ln)[ok].max())
    own = float(numpy.abs(oracle_ln.astype(_exact.LD) - exact_ln)[ok].max())
    bound = _exact.abs_bound(own, exact_ln[ok].astype(numpy.float64))
    if record:
        _record(form, n_haps, n_rows, vec, None, None, err)
    print("   ln_new: error %.3g, the fp64 oracle's %.3g, bound %.3g" % (err, own, bound))
    assert err <= bound, (form, n_haps, n_rows, vec, err, own, bound)
    return err


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    _refs.clear()                                      # (tens of MB per matrix: not for the rest of the session)
    path = os.environ.get("MXM_ACCURACY_REPORT")
    if not path:
        return
    with open(path, "w") as out:
        out.write("| form | H | R | proportions | rel(T_gpu) / u | rel(T_seq) / u | ratio | ln_new / posterior error |\n"
                  "|---|---|---|---|---|---|---|---|\n")
        for form, n_haps, n_rows, vec, rel, rel_seq, ln_err in _rows:
            cells = ["-" if rel is None else "%.1f" % (rel / U), "-" if rel_seq is None else "%.1f" % (rel_seq / U),
                     "-" if rel is None or not rel_seq else "%.2f" % (rel / rel_seq), "-" if ln_err is None else "%.2g" % ln_err]
            out.write("| %s | %d | %d | %s | %s |\n" % (form, n_haps, n_rows, vec, " | ".join(cells)))
        out.write("\nLargest error of `exp` in ulp, on the fp64 arguments `M - rowmax`:\n\n"
                  "| H | R | mxm_linearize | records' P tables | numpy.exp |\n|---|---|---|---|---|\n")
        for row in _exp_rows:
            out.write("| %d | %d | %.2f | %.2f | %.2f |\n" % row)


# ---------------------------------------------------------------- inputs and device plumbing
def _matrix(b17, n_haps, kind="reads", n_rows=None):
    """(label, log matrix, weights): real rows up to Build 17's width, few-values rows beside it."""
    if kind == "few" or n_haps < 65 or n_haps > 5408:
        mat, label = inputs.few_values(700, n_haps), "few values"
    else:
        mat, label = inputs.real_rows(b17, n_haps, kind), kind
    if n_rows is not None:
        mat, label = mat[:n_rows], "%s[:%d]" % (label, n_rows)
    return "%s %d" % (label, n_haps), numpy.array(mat), inputs.weights(len(mat))     # (a writable copy: it goes to torch)


def _vectors(n_haps):
    vecs = dict(inputs.prop_vectors(n_haps))
    second = inputs.prop_vectors(n_haps, seed=1)
    vecs["dirichlet2"], vecs["skewed2"] = second["dirichlet"], second["skewed"]
    return vecs


def _stack(vecs, names):
    return (numpy.ascontiguousarray(numpy.stack([vecs[n][0] for n in names])),
            numpy.ascontiguousarray(numpy.stack([vecs[n][1] for n in names])))


def _em_iter(plan, props, ln):
    """One pass for the restarts props / ln [B][H]; colsum starts as NaN (every entry must be written)."""
    import torch
    from mixemt_amd import em
    p = torch.from_numpy(props).to(plan.dev)
    lnp = torch.from_numpy(ln).to(plan.dev)
    colsum = torch.full_like(p, float("nan"))
    state = em.new_state(p.shape[0], plan.dev)
    plan.em_iter(p, lnp, state, colsum)
    torch.cuda.synchronize()
    em.read_state(state)
    return colsum.cpu().numpy()


def _decoded(plan):
    """The linearised matrix a records plan iterates: the coded rows decoded (mxm_decode_rows), the dense rest as
    mxm_linearize left it."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream
    out = torch.full((plan.n_rows, plan.n_haps), float("nan"), dtype=torch.float64, device=plan.dev)
    _lib.check(plan.lib.mxm_decode_rows(ctypes.byref(plan.coded), plan.n_haps, out.data_ptr(), out.stride(0), current_stream()),
               "mxm_decode_rows")
    if plan.coded_rest:
        idx = torch.nonzero(plan.coded_ndist == 0).flatten()
        out[idx] = plan._coded_keep[3][:, :plan.n_haps]
    lin = out.cpu().numpy()
    assert numpy.isfinite(lin).all()
    return lin


def _coded_plan(mat, wts, **kw):
    """Records plan + the classes of its rows counted on the host (one table entry per distinct value)."""
    from mixemt_amd import em
    plan = em.EmPlan(mat, wts, storage="coded", **kw)
    assert plan.storage == "coded" and plan.coded is not None
    uniq = numpy.array([len(numpy.unique(row)) for row in mat])
    assert plan.coded_wide == ((uniq > 256) & (uniq <= 1024)).sum() and plan.coded_rest == (uniq > 1024).sum()
    return plan


def _loop(plan, props, ln, batch=None):
    """mxm_em_loop / mxm_em_loop_coded / mxm_em_loop_samples with max_iter = 1, tol = 0 from the given arrays (not through
    log_inits: reference and kernel must start from the same bits).  -> colsum, ln_new (numpy) after the checks every loop
    form shares: done == 2, iters == 1, ln_cur untouched."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream
    who = batch if batch is not None else plan
    lib, dev = who.lib, who.dev
    n_runs, n_haps = props.shape
    props_cur, ln_cur = torch.from_numpy(props).to(dev), torch.from_numpy(ln).to(dev)
    ln_new = ln_cur.clone()
    colsum = torch.full_like(props_cur, float("nan"))
    state = torch.zeros(n_runs * (ctypes.sizeof(_lib.EmState) // 8), dtype=torch.int64, device=dev)
    host_state = (_lib.EmState * n_runs)()
    tail = (props_cur.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(), colsum.data_ptr(), state.data_ptr(), 0.0, 1, 16,
            who.ws.data_ptr(), who.ws_bytes, current_stream(), host_state)
    if batch is not None:
        _lib.check(lib.mxm_em_loop_samples(ctypes.byref(batch.coded), batch.row0_ptr, batch.n_entries, batch.wts.data_ptr(), n_haps,
                                           *tail), "mxm_em_loop_samples")
    elif plan.coded is not None:
        _lib.check(lib.mxm_em_loop_coded(ctypes.byref(plan.coded), plan.wts.data_ptr(), n_haps, n_runs, *tail), "mxm_em_loop_coded")
    else:
        m_ptr, ldm = plan.mat_args()
        p_ptr, ldp = plan.lin_args()
        _lib.check(lib.mxm_em_loop(m_ptr, ldm, p_ptr, ldp, plan.wts.data_ptr(), plan.n_rows, n_haps, n_runs, *tail), "mxm_em_loop")
    torch.cuda.synchronize()
    assert [(s.done, s.iters) for s in host_state] == [(2, 1)] * n_runs
    assert numpy.array_equal(ln_cur.cpu().numpy().view(numpy.int64), ln.view(numpy.int64))
    return colsum.cpu().numpy(), ln_new.cpu().numpy()


def _iter_then_finalize(plan, props, ln):
    """{em_iter; mxm_m_finalize} with max_iter = 1, tol = 0 -> colsum, ln_new."""
    import torch
    from mixemt_amd import em
    p, lnc = torch.from_numpy(props).to(plan.dev), torch.from_numpy(ln).to(plan.dev)
    ln_new = lnc.clone()
    colsum = torch.full_like(p, float("nan"))
    state = em.new_state(p.shape[0], plan.dev)
    plan.em_iter(p, lnc, state, colsum)
    plan.finalize(colsum, lnc, ln_new, p, state, 0.0, 1)
    torch.cuda.synchronize()
    assert [(s[0], s[1]) for s in em.read_state(state)] == [(2, 1)] * p.shape[0]
    return colsum.cpu().numpy(), ln_new.cpu().numpy()


def _check_loop_ln(form, ref, ln_new, mat, wts, props, ln, vec, record):
    """A loop's ln_new against exact_finalize over the exact T; the oracle's own ln_new for the scale of the bound.
    record = False: the caller puts the error into the row of its colsum check."""
    exact_ln = _exact.exact_finalize(ref["exact"], ln, props)
    theta = ref["theta"] if "theta" in ref else _oracle_step(mat, wts, ln)[1]
    return _check_ln(form, ln_new, exact_ln, theta, mat.shape[0], mat.shape[1], vec, record=record)


# ---------------------------------------------------------------- the per-iteration forms
@pytest.mark.parametrize("n_rows", [700, 37])
@pytest.mark.parametrize("n_haps", [65, 1023, 5408, 8192])
def test_dense_linear_pass(b17, n_haps, n_rows):
    """mxm_em_iter with P (the wide kernel): one restart, and a full restart tile sharing the pass."""
    from mixemt_amd import em
    label, mat, wts = _matrix(b17, n_haps, n_rows=n_rows)
    plan = em.EmPlan(mat, wts, n_runs=4)
    assert plan.storage == "f64" and plan.lin is not None and plan.coded is None
    lin = numpy.ascontiguousarray(plan.lin[:, :n_haps].cpu().numpy())
    vecs = _vectors(n_haps)
    tile = plan.restart_tile()
    assert tile == plan.lib.mxm_restart_tile(n_haps) and 1 <= tile <= 4
    for names in (["skewed"], ["dirichlet"], ["dirichlet", "skewed", "dirichlet2", "skewed2"][:tile]):
        props, ln = _stack(vecs, names)
        got = _em_iter(plan, props, ln)
        for b, vec in enumerate(names):
            ref = _linear_ref((label, vec), lin, props[b], wts)
            _check_T("mxm_em_iter, dense fp64, B = %d" % len(names), ref, got[b], n_rows, n_haps, vec)


@pytest.mark.parametrize("n_haps", [1, 2, 17, 64, 8200])
def test_log_space_pass(b17, n_haps):
    """mxm_em_iter without P: the narrow (H <= 64) and the generic (H > 8192) log-space kernels."""
    from mixemt_amd import em
    label, mat, wts = _matrix(b17, n_haps)
    plan = em.EmPlan(mat, wts)
    assert plan.lin is None and plan.coded is None and not plan.lib.mxm_linear_supported(n_haps)
    vecs = _vectors(n_haps)
    for vec in ("dirichlet", "skewed"):
        props, ln = _stack(vecs, [vec])
        got = _em_iter(plan, props, ln)
        ref = _log_ref((label, vec, "log"), mat, ln[0], wts)
        _check_T("mxm_em_iter, log space", ref, got[0], len(mat), n_haps, vec)


@pytest.mark.parametrize("n_haps", [66, 5408])
def test_fp32_storage_pass(b17, n_haps):
    """mxm_em_iter_f32: the reference reads the FLOAT matrix, so only the fp64 arithmetic over it is judged."""
    import torch
    from mixemt_amd import em
    label, mat, wts = _matrix(b17, n_haps, n_rows=700)
    plan = em.EmPlan(mat, wts, storage="f32")
    assert plan.storage == "f32" and plan.lin.dtype == torch.float32
    lin = numpy.ascontiguousarray(plan.lin[:, :n_haps].cpu().numpy())
    assert lin.dtype == numpy.float32
    vecs = _vectors(n_haps)
    for vec in ("dirichlet", "skewed"):
        props, ln = _stack(vecs, [vec])
        got = _em_iter(plan, props, ln)
        ref = _linear_ref((label, vec, "f32"), lin, props[0], wts)
        _check_T("mxm_em_iter_f32", ref, got[0], len(mat), n_haps, vec)


@pytest.mark.parametrize("kind", ["reads", "pairs"])
@pytest.mark.parametrize("n_haps", [66, 1025, 2050, 5408])
def test_records_pass(b17, n_haps, kind):
    """mxm_em_iter_coded: byte-coded rows, wide records and (full width, the 4000-bp rows) a dense rest in one matrix."""
    label, mat, wts = _matrix(b17, n_haps, kind)
    plan = _coded_plan(mat, wts, n_runs=2)
    assert plan.coded.n_quad_rows == 0 and plan.restart_tile() == 1
    if n_haps == 5408:
        assert plan.coded_wide > 0 and (kind == "pairs" or plan.coded_rest > 0)
    print("rows %d: wide %d, dense rest %d" % (len(mat), plan.coded_wide, plan.coded_rest))
    lin = _decoded(plan)
    vecs = _vectors(n_haps)
    props, ln = _stack(vecs, ["dirichlet", "skewed"])
    got = _em_iter(plan, props, ln)
    for b, vec in enumerate(("dirichlet", "skewed")):
        ref = _linear_ref((label, vec), lin, props[b], wts)
        _check_T("mxm_em_iter_coded, records", ref, got[b], len(mat), n_haps, vec)


@pytest.mark.parametrize("n_haps", [1024, 2050, 5408])
def test_records_with_quads_pass(b17, n_haps):
    """The quad dictionary: one restart (em_iter_quad_coded_kernel), three restarts sharing the quad pass
    (em_iter_quad_batched_kernel) and four = a tile of three + one."""
    label, mat, wts = _matrix(b17, n_haps)
    plan = _coded_plan(mat, wts, n_runs=4)
    assert plan.attach_quads(True) and plan.coded.n_quad_rows > 0
    c = plan.coded
    assert c.n_quad_rows + c.n_byte_rows + c.n_wide + c.R_rest == len(mat)
    lin = _decoded(plan)
    vecs = _vectors(n_haps)
    batches = [["skewed"], ["dirichlet"]]
    if n_haps >= 2050:
        assert plan.restart_tile() == 3 == plan.lib.mxm_restart_tile_coded(ctypes.byref(plan.coded), n_haps)
        batches += [["dirichlet", "skewed", "dirichlet2"], ["skewed2", "dirichlet2", "dirichlet", "skewed"]]
    for names in batches:
        props, ln = _stack(vecs, names)
        got = _em_iter(plan, props, ln)
        for b, vec in enumerate(names):
            ref = _linear_ref((label, vec), lin, props[b], wts)
            _check_T("mxm_em_iter_coded, quads, B = %d" % len(names), ref, got[b], len(mat), n_haps, vec)


def _ragged_batch(b17, n_haps):
    """Samples of 1, 37, 257, 700 and tile + 1 rows back to back in one records matrix -> (batch, finish, per-sample
    (label, log matrix, weights, decoded P))."""
    import torch
    from mixemt_amd import _lib, em
    k = _lib.load().mxm_samples_tile_rows()
    reads = inputs.real_rows(b17, n_haps, "reads")[:inputs.N_READS]
    pairs = inputs.real_rows(b17, n_haps, "pairs")
    mats = [reads[0:1], reads[1:38], pairs, reads, reads[100:100 + k + 1]]
    assert [len(m) for m in mats] == [1, 37, 257, 700, k + 1]
    wts = [inputs.weights(len(m), seed=s) for s, m in enumerate(mats)]
    row0 = numpy.concatenate([[0], numpy.cumsum([len(m) for m in mats])]).astype(numpy.int64)
    cat = numpy.ascontiguousarray(numpy.concatenate(mats))
    plan = _coded_plan(cat, numpy.concatenate(wts), keep_log_matrix=False)
    assert plan.coded_rest == 0 and (n_haps < 5408 or plan.coded_wide > 0)
    lin = _decoded(plan)
    rec, rec_off, ndist = plan._coded_keep[:3]
    batch = em.SampleBatch(rec, rec_off, ndist, plan.wts, row0, n_haps)
    finish = em.SampleFinish(rec, rec_off, ndist, plan.wts, None, row0, n_haps)
    assert batch.n_tiles == sum((len(m) + k - 1) // k for m in mats)
    samples = [("sample %d of %d rows, %d" % (s, len(m), n_haps), numpy.ascontiguousarray(m), wts[s],
                numpy.ascontiguousarray(lin[row0[s]:row0[s + 1]])) for s, m in enumerate(mats)]
    keep = (plan, torch)                               # (the batch points into the plan's tensors)
    return batch, finish, samples, keep


SAMPLE_VECTORS = ("skewed", "dirichlet", "skewed", "dirichlet", "skewed")


@pytest.mark.parametrize("n_haps", [66, 5408])
def test_many_samples_pass_and_loop(b17, n_haps):
    """mxm_em_iter_samples and mxm_em_loop_samples on the ragged batch: every sample against its own reference."""
    import torch
    from mixemt_amd import em
    batch, _, samples, keep = _ragged_batch(b17, n_haps)
    vecs = _vectors(n_haps)
    props, ln = _stack(vecs, SAMPLE_VECTORS)
    p = torch.from_numpy(props).to(batch.dev)
    colsum = torch.full_like(p, float("nan"))
    state = em.new_state(len(samples), batch.dev)
    batch.em_iter(p, state, colsum)
    torch.cuda.synchronize()
    em.read_state(state)
    got = colsum.cpu().numpy()
    loop_T, loop_ln = _loop(None, props, ln, batch=batch)
    assert numpy.isfinite(loop_T).all()                # plain launches: the loop leaves its last sums in colsum
    for s, (label, mat, wts, lin) in enumerate(samples):
        vec = SAMPLE_VECTORS[s]
        ref = _linear_ref((label, vec), lin, props[s], wts)
        _check_T("mxm_em_iter_samples", ref, got[s], len(mat), n_haps, vec)
        err = _check_loop_ln("mxm_em_loop_samples", ref, loop_ln[s], mat, wts, props[s], ln[s], vec, False)
        _check_T("mxm_em_loop_samples", ref, loop_T[s], len(mat), n_haps, vec, ln_err=err)


# ---------------------------------------------------------------- the loop forms: max_iter = 1, tol = 0
def _loop_form(form, plan, label, mat, wts, lin, vecs, mode, one_launch):
    """Each vector as a run of its own (one restart per call); colsum is checked where the form writes it, ln_new always."""
    plan.lib.mxm_set_loop_fused(mode, 0)
    out = {}
    for vec in ("dirichlet", "skewed"):
        props, ln = _stack(vecs, [vec])
        colsum, ln_new = _loop(plan, props, ln)
        if lin is not None:
            ref = _linear_ref((label, vec), lin, props[0], wts)
        else:
            ref = _log_ref((label, vec, "log"), mat, ln[0], wts)
        err = _check_loop_ln(form, ref, ln_new[0], mat, wts, props[0], ln[0], vec, one_launch)
        if not one_launch:                             # (the one-launch loops take no colsum)
            _check_T(form, ref, colsum[0], mat.shape[0], mat.shape[1], vec, ln_err=err)
        out[vec] = (props, ln, colsum, ln_new)
    return out


def _bits(a):
    return numpy.ascontiguousarray(a).view(numpy.int64)


def test_dense_loops_600_by_5408(b17):
    """mxm_em_loop: the one-launch loop (mode 1: columns split, the matrix in registers; mode 2: rows split) and the
    per-iteration kernels (mode 0), whose ln_new is {em_iter; m_finalize}'s to the bit."""
    from mixemt_amd import em
    label, mat, wts = _matrix(b17, 5408, n_rows=600)
    plan = em.EmPlan(mat, wts)
    lin = numpy.ascontiguousarray(plan.lin[:, :5408].cpu().numpy())
    vecs = _vectors(5408)
    _loop_form("mxm_em_loop, one launch, columns split", plan, label, mat, wts, lin, vecs, 1, True)
    _loop_form("mxm_em_loop, one launch, rows split", plan, label, mat, wts, lin, vecs, 2, True)
    runs = _loop_form("mxm_em_loop, per-iteration kernels", plan, label, mat, wts, lin, vecs, 0, False)
    for vec, (props, ln, colsum, ln_new) in runs.items():
        t2, ln2 = _iter_then_finalize(plan, props, ln)
        assert numpy.array_equal(_bits(colsum), _bits(t2)) and numpy.array_equal(_bits(ln_new), _bits(ln2)), vec


def test_narrow_one_launch_loop_700_by_3(b17):
    """The refinement EM's shape: the contributors' three columns of the full-width rows, in log space."""
    from mixemt_amd import em
    full = inputs.real_rows(b17, 5408, "reads")[:700]
    mat = numpy.ascontiguousarray(full[:, [0, 2704, 5407]])
    wts = inputs.weights(700)
    plan = em.EmPlan(mat, wts)
    assert plan.lin is None
    vecs = _vectors(3)
    _loop_form("mxm_em_loop, narrow one-launch loop", plan, "contributors' columns 3", mat, wts, None, vecs, 1, True)
    runs = _loop_form("mxm_em_loop, narrow, per-iteration kernels", plan, "contributors' columns 3", mat, wts, None, vecs, 0, False)
    for vec, (props, ln, colsum, ln_new) in runs.items():
        t2, ln2 = _iter_then_finalize(plan, props, ln)
        assert numpy.array_equal(_bits(colsum), _bits(t2)) and numpy.array_equal(_bits(ln_new), _bits(ln2)), vec


def test_records_loops_700_by_5408(b17):
    """mxm_em_loop_coded in one launch (records without a dense rest), and through the per-iteration kernels."""
    label, mat, wts = _matrix(b17, 5408, n_rows=700)
    plan = _coded_plan(mat, wts)
    assert plan.coded_rest == 0 and plan.coded_wide > 0 and plan.coded.n_quad_rows == 0
    lin = _decoded(plan)
    vecs = _vectors(5408)
    _loop_form("mxm_em_loop_coded, one launch", plan, label, mat, wts, lin, vecs, 1, True)
    runs = _loop_form("mxm_em_loop_coded, per-iteration kernels", plan, label, mat, wts, lin, vecs, 0, False)
    for vec, (props, ln, colsum, ln_new) in runs.items():
        t2, ln2 = _iter_then_finalize(plan, props, ln)
        assert numpy.array_equal(_bits(colsum), _bits(t2)) and numpy.array_equal(_bits(ln_new), _bits(ln2)), vec


def test_many_samples_narrow_loop(b17):
    """mxm_em_loop_samples_narrow: one workgroup per sample over its contributors' columns (1 .. 3 of them, ld = 4)."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream
    n_haps, ld = 5408, 4
    _, finish, samples, keep = _ragged_batch(b17, n_haps)
    ncol = numpy.array([1, 3, 2, 3, 3], dtype=numpy.int32)
    cols = [0, n_haps // 2, n_haps - 1]
    n_rows = sum(len(s[1]) for s in samples)
    red = numpy.full((n_rows, ld), -numpy.inf)
    props = numpy.zeros((len(samples), ld))
    ln = numpy.full((len(samples), ld), -numpy.inf)
    at = 0
    for s, (label, mat, wts, _) in enumerate(samples):
        red[at:at + len(mat), :ncol[s]] = mat[:, cols[:ncol[s]]]
        props[s, :ncol[s]], ln[s, :ncol[s]] = _vectors(int(ncol[s]))[SAMPLE_VECTORS[s]]
        at += len(mat)
    dev = finish.dev
    m_d, props_cur, ln_cur = (torch.from_numpy(a).to(dev) for a in (red, props, ln))
    ln_new = ln_cur.clone()
    state = torch.zeros(len(samples) * (ctypes.sizeof(_lib.EmState) // 8), dtype=torch.int64, device=dev)
    host_state = (_lib.EmState * len(samples))()
    e_buf = torch.empty((n_rows, ld), dtype=torch.float64, device=dev)
    _lib.check(finish.lib.mxm_em_loop_samples_narrow(ctypes.byref(finish.coded), finish.row0_ptr, len(samples), n_haps, m_d.data_ptr(),
                                                     ld, ncol.ctypes.data_as(ctypes.c_void_p), finish.wts.data_ptr(), props_cur.data_ptr(),
                                                     ln_cur.data_ptr(), ln_new.data_ptr(), state.data_ptr(), 0.0, 1, 16, e_buf.data_ptr(),
                                                     finish.ws.data_ptr(), finish.ws_bytes, current_stream(), host_state),
               "mxm_em_loop_samples_narrow")
    torch.cuda.synchronize()
    assert [(s.done, s.iters) for s in host_state] == [(2, 1)] * len(samples)
    got = ln_new.cpu().numpy()
    for s, (label, mat, wts, _) in enumerate(samples):
        n = int(ncol[s])
        sub = numpy.ascontiguousarray(mat[:, cols[:n]])
        ref = _log_ref((label, "narrow"), sub, numpy.ascontiguousarray(ln[s, :n]), wts)
        _check_loop_ln("mxm_em_loop_samples_narrow", ref, got[s, :n], sub, wts, props[s, :n], ln[s, :n], SAMPLE_VECTORS[s], True)


# ---------------------------------------------------------------- mxm_m_finalize alone, the posteriors, the linearisation
@pytest.mark.parametrize("n_haps", [3, 66, 5408, 8200])
def test_m_finalize_alone(b17, n_haps):
    """T from the reference (rounded to fp64); ln_cur includes entries at -800, whose props_cur is 0."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream, require_gpu
    if n_haps == 3:
        mat, wts = numpy.ascontiguousarray(inputs.real_rows(b17, 5408, "reads")[:700][:, [0, 2704, 5407]]), inputs.weights(700)
    else:
        _, mat, wts = _matrix(b17, n_haps, n_rows=700)
    vecs = _vectors(n_haps)
    names = ["skewed", "dirichlet"]
    props, ln = _stack(vecs, names)
    ln[0, 1:min(n_haps - 1, 9):2] = -800.0
    props = numpy.exp(ln)
    assert (props[0] == 0).any()
    T = numpy.stack([_exact.exact_colsum(inputs.linearise(mat), vecs[n][0], wts).astype(numpy.float64) for n in names])
    lib, dev = _lib.load(), require_gpu()
    colsum, ln_cur, props_cur = (torch.from_numpy(a).to(dev) for a in (T, ln, props))
    ln_new = ln_cur.clone()
    state = torch.zeros(2 * (ctypes.sizeof(_lib.EmState) // 8), dtype=torch.int64, device=dev)
    _lib.check(lib.mxm_m_finalize(colsum.data_ptr(), ln_cur.data_ptr(), ln_new.data_ptr(), props_cur.data_ptr(), n_haps, 2, 0.0, 1,
                                  state.data_ptr(), current_stream()), "mxm_m_finalize")
    torch.cuda.synchronize()
    got = ln_new.cpu().numpy()
    for b, vec in enumerate(names):
        assert (T[b] > 0).all()
        exact_ln = _exact.exact_finalize(T[b], ln[b], props[b])
        plain = ln[b] + numpy.log(T[b]) - numpy.log((props[b] * T[b]).sum())
        _check_ln("mxm_m_finalize", got[b], exact_ln, plain, len(mat), n_haps, vec)


def _check_posterior(form, got, exact, oracle, n_rows, n_haps, vec):
    finite = numpy.isfinite(exact.astype(numpy.float64))
    assert numpy.array_equal(numpy.isfinite(got), finite) and numpy.array_equal(numpy.isfinite(oracle), finite)
    err = float(numpy.abs(got.astype(_exact.LD) - exact)[finite].max())
    own = float(numpy.abs(oracle.astype(_exact.LD) - exact)[finite].max())
    bound = _exact.abs_bound(own, exact[finite].astype(numpy.float64))
    print("%-30s H=%-5d %-10s posterior error %.3g, the fp64 oracle's %.3g, bound %.3g" % (form, n_haps, vec, err, own, bound))
    _rows.append((form + " (posterior)", n_haps, n_rows, vec, None, None, err))
    assert err <= bound, (form, n_haps, vec, err, own, bound)


@pytest.mark.parametrize("n_haps", [3, 64, 65, 5408])
def test_posterior_dense(b17, n_haps):
    """mxm_em_step against exact_posterior."""
    from mixemt_amd import em
    if n_haps == 3:
        mat, wts = numpy.ascontiguousarray(inputs.real_rows(b17, 5408, "reads")[:700][:, [0, 2704, 5407]]), inputs.weights(700)
    else:
        _, mat, wts = _matrix(b17, n_haps, n_rows=700)
    plan = em.EmPlan(mat, wts)
    for vec in ("dirichlet", "skewed"):
        ln = _vectors(n_haps)[vec][1]
        got = em.posterior(plan, ln).cpu().numpy()
        _check_posterior("mxm_em_step", got, _exact.exact_posterior(mat, ln), _oracle_step(mat, wts, ln)[0], len(mat), n_haps, vec)


@pytest.mark.parametrize("n_haps", [66, 5408])
def test_posterior_from_records(b17, n_haps):
    """mxm_em_step_coded: mode 0 (store) and mode 1 (logaddexp fold of a second vector into the first's posterior)."""
    import torch
    from mixemt_amd import em, preprocess
    label, mat, wts = _matrix(b17, n_haps)
    plan = _coded_plan(mat, wts)
    rest = torch.nonzero(plan.coded_ndist == 0).flatten()
    cm = preprocess.CodedMatrix(len(mat), n_haps, *plan._coded_keep[:3], plan.rowmax, 0, rest, plan.mat[rest].contiguous())
    rec_plan = em.EmPlan(None, wts, records=cm)
    assert rec_plan.mat is None and (n_haps < 5408 or (int(rest.numel()) > 0 and plan.coded_wide > 0))
    vecs = _vectors(n_haps)
    ln_a, ln_b = vecs["skewed"][1], vecs["dirichlet"][1]
    exact_a, exact_b = _exact.exact_posterior(mat, ln_a), _exact.exact_posterior(mat, ln_b)
    own_a, own_b = _oracle_step(mat, wts, ln_a)[0], _oracle_step(mat, wts, ln_b)[0]
    out = em.posterior(rec_plan, ln_a)
    _check_posterior("mxm_em_step_coded, mode 0", out.cpu().numpy(), exact_a, own_a, len(mat), n_haps, "skewed")
    out = em.posterior(rec_plan, ln_b, out=out, fold=True)
    hi, lo = numpy.maximum(exact_a, exact_b), numpy.minimum(exact_a, exact_b)
    fold = hi + numpy.log1p(numpy.exp(lo - hi))
    _check_posterior("mxm_em_step_coded, mode 1", out.cpu().numpy(), fold, numpy.logaddexp(own_a, own_b), len(mat), n_haps,
                     "skewed + dirichlet")


@pytest.mark.parametrize("n_haps", [66, 5408])
def test_linearisation_in_ulp(b17, n_haps):
    """mxm_linearize and the records' P tables against exp(M - rowmax) in long double, on the fp64 argument M - rowmax:
    the device's exp is no worse than numpy's by more than one ulp (both libraries document <= 1 ulp); decoded records
    equal mxm_linearize's rows bit for bit."""
    import torch
    from mixemt_amd import em
    label, mat, wts = _matrix(b17, n_haps)
    dense = em.EmPlan(mat, wts)
    coded = _coded_plan(mat, wts)
    rowmax = dense.rowmax.cpu().numpy()
    assert numpy.array_equal(rowmax, mat.max(axis=1)) and torch.equal(coded.rowmax, dense.rowmax)
    arg = mat - rowmax[:, None]
    exact = numpy.exp(arg.astype(_exact.LD))
    lin = dense.lin[:, :n_haps].cpu().numpy()
    host_ulp = _exact.ulp_err(numpy.exp(arg), exact)
    dev_ulp = _exact.ulp_err(lin, exact)
    dec = _decoded(coded)
    rec_ulp = _exact.ulp_err(dec, exact)
    print("H=%d: exp in ulp -- mxm_linearize %.3f, records %.3f, numpy.exp %.3f" % (n_haps, dev_ulp, rec_ulp, host_ulp))
    _exp_rows.append((n_haps, len(mat), dev_ulp, rec_ulp, host_ulp))
    assert dev_ulp <= host_ulp + 1.0 and rec_ulp <= host_ulp + 1.0
    assert numpy.array_equal(_bits(dec), _bits(lin))
