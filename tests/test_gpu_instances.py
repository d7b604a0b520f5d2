"""
Every kernel instance the width dispatchers compile, at the first and the last width that reach it.

tests/_instances.py restates, per dispatch_width site of mixemt_hip.hip, the host's formula from the width to the template
instance; this module runs site x instance x {first, last width of the class}.  A case is ONE call of the entry on 3, 37
or 64 rows (picked by the instance number), under the reference and the rule the entry's own tests already use -- nothing
new is introduced here:
  * the passes that return `colsum` (dense tiles of 1 .. 4 restarts, fp32 storage, records, records with a dense rest, the
    quad passes, the batched quad pass, many samples): T against _exact.exact_colsum on the bits the kernel read, both bounds of
    tests/test_gpu_accuracy.py (_exact.tight_bound, _exact.derived_bound) behind _exact.check_products;
  * mxm_linearize and mxm_linearize_f32: the long-double exp, at test_gpu_accuracy.py::test_linearisation_in_ulp's figure;
  * mxm_em_step: posterior and ln_new under _exact.abs_bound;
  * both argmax entries: EVERY row's label against the long-double values of tests/_exact_consumers.py on continuous
    inputs whose exact top-two margin is asserted (from the reference alone) to be far above rounding; integer weights,
    so the votes are exact;
  * mxm_encode_rows / mxm_decode_rows: the round trip equals mxm_linearize's rows bit for bit; the builders: the C oracle's
    bits (rows of 65 .. 128 observations for the long-row marker instances), and for mxm_build_em_records the decoded
    records against mxm_linearize's rows as well;
  * the one-launch loops: three iterations under mxm_set_loop_fused(1) / (2), ln_new against _exact_traj.exact_trajectory
    under the rule of tests/test_gpu_accuracy_loops.py; the library's force-abort hook shows first that the shape really
    takes the one-launch loop (an ineligible shape would go to the per-iteration kernels without a word).
Where an entry picks its kernel by more than the width, the case builds inputs that meet the condition the table states and
asserts it (and that the call returned 0: _lib.check raises otherwise).
Inputs: _accuracy_inputs.edge_rows (column slices of the real full-width rows up to 5408 columns, few_values beyond).
MXM_ACCURACY_REPORT=<prefix> makes the module write <prefix>.instances (tools/accuracy_report.py).
"""
import ctypes
import os

import numpy
import pytest

import _accuracy_inputs as inputs
import _exact
import _exact_consumers as xc
import _instances as inst
import test_gpu_accuracy as one_pass
import test_gpu_accuracy_loops as loops
from oracle import c_oracle, em_oracle

pytestmark = pytest.mark.gpu

U = _exact.U
MARGIN = 1e-6                                        # the argmax cases' smallest exact top-two margin: 10^7 x the rounding of
                                                     # values of size 100 (u * 100 = 1.1e-14)
_refs = {}
_rows = []                                           # (site, form, instance, H, R, vector, rel, rel_seq, other error)
_kept = {}


def _cases(name):
    return [pytest.param(i, h, id="%s<%d>-H%d" % (name, i, h)) for i, h in inst.edge_cases(name)]


def _record(site, form, instance, n_haps, n_rows, vec, rel, rel_seq, other=None):
    _rows.append((site, form, instance, n_haps, n_rows, vec, rel, rel_seq, other))
    print("%-44s H=%-5d R=%-4d %-10s rel(T_gpu) = %s u, rel(T_seq) = %s u%s"
          % ("%s <%d>" % (form, instance), n_haps, n_rows, vec, "-" if rel is None else "%.1f" % (rel / U),
             "-" if rel_seq is None else "%.1f" % (rel_seq / U), "" if other is None else ", %s" % other))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    _refs.clear()
    _kept.clear()
    path = os.environ.get("MXM_ACCURACY_REPORT")
    if not path:
        return
    with open(path + ".instances", "w") as out:
        out.write("Largest `rel(T_gpu) / rel(T_seq)` per site:\n\n| site | entry | kernel | cases | largest ratio | at |\n|---|---|---|---|---|---|\n")
        for name, site in inst.SITES.items():
            mine = [r for r in _rows if r[0] == name]
            ratios = [(r[6] / r[7], r) for r in mine if r[6] is not None and r[7]]
            if not mine:
                continue
            if ratios:
                top, r = max(ratios, key=lambda t: t[0])
                out.write("| %s | %s | `%s` | %d | %.2f | <%d>, H = %d, %s |\n" % (name, site.entry, site.kernel, len(mine), top, r[2], r[3], r[5]))
            else:
                out.write("| %s | %s | `%s` | %d | - | - |\n" % (name, site.entry, site.kernel, len(mine)))
        out.write("\n| site | instance | H | R | proportions | rel(T_gpu) / u | rel(T_seq) / u | ratio | other |\n|---|---|---|---|---|---|---|---|---|\n")
        for name, form, instance, n_haps, n_rows, vec, rel, rel_seq, other in _rows:
            out.write("| %s | %d | %d | %d | %s | %s | %s | %s | %s |\n"
                      % (name, instance, n_haps, n_rows, vec, "-" if rel is None else "%.1f" % (rel / U),
                         "-" if rel_seq is None else "%.1f" % (rel_seq / U), "-" if rel is None or not rel_seq else "%.2f" % (rel / rel_seq),
                         other or "-"))


# ---------------------------------------------------------------- inputs and references, made once
def _quad_reads(b17, n_haps, n_rows):
    """The first n_rows 150-bp reads (their first n_haps columns) that get a quad record for certain: at most 200 distinct
    aligned groups of four columns, counted here on the log values (the dictionary holds 256; a few reads pass that)."""
    import _class_rows
    reads = inputs.real_rows(b17, 5408, "reads")[:inputs.N_READS, :n_haps]
    pad = numpy.zeros((len(reads), inst.coded_ld(n_haps)))
    pad[:, :n_haps] = reads
    keep = []
    for r in range(len(reads)):
        if len(keep) < n_rows and _class_rows.n_quads(pad[r]) <= 200:
            keep.append(r)
    assert len(keep) == n_rows
    return reads[keep]


def _rows_of(b17, n_haps, instance, extra_wide=False, quads_only=False):
    """(label, log matrix, weights) of a case.  quads_only: every row must get a quad record (150-bp reads alone; beyond
    Build 17's width few_quads); extra_wide: one more row of min(H, 600) distinct values in random order -- a wide record
    from 257 columns on, which no quad pass takes (the leftover pass beside it)."""
    n_rows = inst.rows_for(instance)
    key = (n_haps, n_rows, extra_wide, quads_only)
    if key not in _kept:
        if quads_only or extra_wide:
            body = n_rows - (1 if extra_wide else 0)
            if n_haps > 5408:
                mat, label = inputs.few_quads(64, n_haps)[:body], "few quads[:%d] %d" % (body, n_haps)
            else:
                mat, label = _quad_reads(b17, n_haps, body), "%d reads with quads %d" % (body, n_haps)
            if extra_wide:
                import _class_rows
                wide = _class_rows.rows_with_values(n_haps, [min(n_haps, 600)], seed=n_haps, layout="shuffled")
                mat, label = numpy.concatenate([mat, wide]), label + " + a wide row"
        else:
            label, mat = inputs.edge_rows(b17, n_haps, n_rows)
        mat = numpy.array(mat)
        assert mat.shape == (n_rows, n_haps) and n_rows <= 64
        _kept[key] = (label, mat, inputs.weights(n_rows))
    return _kept[key]


VECTORS = ("dirichlet", "skewed", "dirichlet2", "skewed2")


def _names(instance, nb=1):
    """The proportion vectors of a case: one restart alternates between the two regimes, a tile takes the first nb."""
    return [VECTORS[instance % 2]] if nb == 1 else list(VECTORS[:nb])


def _linear_ref(label, vec, lin, props, wts):
    key = (label, vec, lin.dtype.str, _digest(lin))
    if key not in _refs:
        _exact.check_products(lin, props)
        exact = _exact.exact_colsum(lin, props, wts)
        _refs[key] = {"exact": exact, "rel_seq": _exact.rel_err(_exact.seq_colsum(lin, props, wts), exact)}
    return _refs[key]


def _digest(a):
    return loops._digest(a)


def _check_T(site, form, instance, ref, got, n_rows, n_haps, vec):
    rel = _exact.rel_err(got, ref["exact"])
    _record(site, form, instance, n_haps, n_rows, vec, rel, ref["rel_seq"])
    assert rel <= _exact.tight_bound(ref["rel_seq"]), (form, instance, n_haps, n_rows, vec, rel / U, ref["rel_seq"] / U)
    assert rel <= _exact.derived_bound(n_rows, n_haps), (form, instance, n_haps, n_rows, vec, rel / U)


def _aligned(t, by=16):
    return t.data_ptr() % by == 0 and t.stride(0) % 2 == 0


def _pass(site, form, instance, plan, lin, label, wts, n_haps, names):
    """One call of plan.em_iter for the restarts `names`; every restart against its reference."""
    props, ln = one_pass._stack(one_pass._vectors(n_haps), names)
    got = one_pass._em_iter(plan, props, ln)
    for b, vec in enumerate(names):
        _check_T(site, form, instance, _linear_ref(label, vec, lin, props[b], wts), got[b], len(wts), n_haps, vec)


# ---------------------------------------------------------------- the passes over the dense matrix
def _dense_cases():
    return [pytest.param(nb, i, h, id="em_iter_b%d<%d>-H%d" % (nb, i, h)) for nb in (1, 2, 3, 4) for i, h in inst.edge_cases("em_iter_b%d" % nb)]


@pytest.mark.parametrize("nb,instance,n_haps", _dense_cases())
def test_dense_pass(b17, nb, instance, n_haps):
    """mxm_em_iter over the linearised fp64 matrix, B = nb restarts in one tile: em_iter_wide_kernel<threads, NCH, nb, ...>."""
    from mixemt_amd import em
    label, mat, wts = _rows_of(b17, n_haps, instance)
    plan = em.EmPlan(mat, wts, n_runs=nb)
    assert plan.storage == "f64" and plan.lin is not None and plan.coded is None and plan.lin.stride(0) % 2 == 0
    assert plan.lib.mxm_restart_tile(n_haps) >= nb            # batch_fits(H, nb): the nb restarts share ONE pass
    buf = ctypes.create_string_buffer(128)
    assert plan.lib.mxm_describe_stream_kernel(n_haps, nb, buf, len(buf)) == 0
    assert buf.value.decode() == inst.stream_kernel_name(n_haps, nb) and ", %d, %d," % (instance, nb) in buf.value.decode()
    lin = numpy.ascontiguousarray(plan.lin[:, :n_haps].cpu().numpy())
    _pass("em_iter_b%d" % nb, "mxm_em_iter, dense fp64, B = %d" % nb, instance, plan, lin, label, wts, n_haps, _names(instance, nb))


@pytest.mark.parametrize("instance,n_haps", _cases("em_iter_f32"))
def test_fp32_storage_pass(b17, instance, n_haps):
    import torch
    from mixemt_amd import em
    label, mat, wts = _rows_of(b17, n_haps, instance)
    plan = em.EmPlan(mat, wts, storage="f32")
    assert plan.storage == "f32" and plan.lin.dtype == torch.float32 and plan.lin.stride(0) % 4 == 0
    lin = numpy.ascontiguousarray(plan.lin[:, :n_haps].cpu().numpy())
    _pass("em_iter_f32", "mxm_em_iter_f32", instance, plan, lin, label, wts, n_haps, _names(instance))


@pytest.mark.parametrize("instance,n_haps", _cases("linearize"))
def test_linearize(b17, instance, n_haps):
    """linearize_wide_kernel<NCH, double>: exp in ulp against the long double, rowmax exact, the pad columns [H, ldp)
    zero as the header promises."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream, require_gpu
    label, mat, wts = _rows_of(b17, n_haps, instance)
    lib, dev = _lib.load(), require_gpu()
    n_rows = len(mat)
    m_d = torch.from_numpy(mat).to(dev)
    out = torch.full((n_rows, n_haps + 2), -7.0, dtype=torch.float64, device=dev)
    rowmax = torch.full((n_rows,), float("nan"), dtype=torch.float64, device=dev)
    assert n_haps % 2 == 0 and _aligned(m_d) and _aligned(out)           # the wide route's condition
    _lib.check(lib.mxm_linearize(m_d.data_ptr(), m_d.stride(0), n_rows, n_haps, out.data_ptr(), out.stride(0), rowmax.data_ptr(),
                                 current_stream()), "mxm_linearize")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[:, n_haps:] == 0.0).all() and numpy.isfinite(host).all()
    assert numpy.array_equal(rowmax.cpu().numpy(), mat.max(axis=1))
    arg = mat - mat.max(axis=1)[:, None]
    exact = numpy.exp(arg.astype(_exact.LD))
    host_ulp = _exact.ulp_err(numpy.exp(arg), exact)
    dev_ulp = _exact.ulp_err(host[:, :n_haps], exact)
    _record("linearize", "mxm_linearize", instance, n_haps, n_rows, "-", None, None, "exp %.3f ulp (numpy.exp %.3f)" % (dev_ulp, host_ulp))
    assert dev_ulp <= host_ulp + 1.0


@pytest.mark.parametrize("instance,n_haps", _cases("linearize_f32"))
def test_linearize_f32(b17, instance, n_haps):
    """linearize_wide_kernel<NCH, float>: exp in float ulp against the long double (the figure of test_linearize, beside
    numpy.exp rounded to float), rowmax exact, the pad columns zero."""
    import torch
    from mixemt_amd import _lib
    from mixemt_amd._dev import current_stream, require_gpu
    label, mat, wts = _rows_of(b17, n_haps, instance)
    lib, dev = _lib.load(), require_gpu()
    n_rows = len(mat)
    m_d = torch.from_numpy(mat).to(dev)
    ldp = (n_haps + 3) // 4 * 4 + 4
    out = torch.full((n_rows, ldp), -7.0, dtype=torch.float32, device=dev)
    rowmax = torch.full((n_rows,), float("nan"), dtype=torch.float64, device=dev)
    assert n_haps % 2 == 0 and _aligned(m_d) and out.data_ptr() % 8 == 0 and ldp % 4 == 0      # the wide route's condition
    _lib.check(lib.mxm_linearize_f32(m_d.data_ptr(), m_d.stride(0), n_rows, n_haps, out.data_ptr(), out.stride(0), rowmax.data_ptr(),
                                     current_stream()), "mxm_linearize_f32")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert host.dtype == numpy.float32 and (host[:, n_haps:] == 0.0).all() and numpy.isfinite(host).all()
    assert numpy.array_equal(rowmax.cpu().numpy(), mat.max(axis=1))
    arg = mat - mat.max(axis=1)[:, None]
    exact = numpy.exp(arg.astype(_exact.LD))
    host_ulp = _exact.ulp_err(numpy.exp(arg).astype(numpy.float32), exact)
    dev_ulp = _exact.ulp_err(host[:, :n_haps], exact)
    _record("linearize_f32", "mxm_linearize_f32", instance, n_haps, n_rows, "-", None, None,
            "exp %.3f float ulp (numpy.exp rounded to float %.3f)" % (dev_ulp, host_ulp))
    assert dev_ulp <= host_ulp + 1.0


def _exact_ln_new(exact_post, wts):
    """ln_new of mxm_em_step + mxm_log_normalize in long double: log sum_r w_r exp(post_rh), normalised over h."""
    t = _exact._pairwise_sum(numpy.exp(exact_post) * numpy.asarray(wts).astype(_exact.LD)[:, None], axis=0)
    with numpy.errstate(divide="ignore"):
        return numpy.log(t) - numpy.log(_exact._pairwise_sum(t, axis=0))


def _check_abs(site, form, instance, what, got, exact, oracle, n_rows, n_haps, vec):
    finite = numpy.isfinite(numpy.asarray(exact).astype(numpy.float64))
    assert finite.any() and numpy.array_equal(numpy.isfinite(got), finite)
    err = float(numpy.abs(got.astype(_exact.LD) - exact)[finite].max())
    own = float(numpy.abs(oracle.astype(_exact.LD) - exact)[finite].max())
    bound = _exact.abs_bound(own, numpy.asarray(exact)[finite].astype(numpy.float64))
    _record(site, form, instance, n_haps, n_rows, vec, None, None, "%s error %.3g (the fp64 oracle's %.3g, bound %.3g)" % (what, err, own, bound))
    assert err <= bound, (form, instance, n_haps, vec, what, err, own, bound)


@pytest.mark.parametrize("with_colsum,instance,n_haps",
                         [pytest.param(c, i, h, id="%s<%d>-H%d" % (s, i, h)) for s, c in (("em_step", False), ("em_step_colsum", True))
                          for i, h in inst.edge_cases(s)])
def test_em_step(b17, with_colsum, instance, n_haps):
    """estep_wide_kernel<NCH, colsum>: the posterior (and, with colsum, ln_new through mxm_log_normalize)."""
    import torch
    from mixemt_amd import em
    site = "em_step_colsum" if with_colsum else "em_step"
    label, mat, wts = _rows_of(b17, n_haps, instance)
    vec = _names(instance)[0]
    ln = one_pass._vectors(n_haps)[vec][1]
    oracle_post, oracle_ln = em_oracle.em_step(numpy.array(mat), wts, ln, numpy.empty_like(mat))
    exact = _exact.exact_posterior(mat, ln)
    if with_colsum:
        m_d = torch.from_numpy(mat).cuda()
        out = torch.full_like(m_d, float("nan"))
        assert n_haps % 2 == 0 and _aligned(m_d) and _aligned(out)
        post, ln_new = em.em_step(m_d, torch.from_numpy(wts).cuda(), torch.from_numpy(ln).cuda(), out)
        torch.cuda.synchronize()
        _check_abs(site, "mxm_em_step, colsum", instance, "ln_new", ln_new.cpu().numpy(), _exact_ln_new(exact, wts), oracle_ln, len(mat), n_haps, vec)
        got = post.cpu().numpy()
    else:
        plan = em.EmPlan(mat, wts)
        assert n_haps % 2 == 0 and _aligned(plan.mat)
        out = em.posterior(plan, ln)
        assert _aligned(out)
        got = out.cpu().numpy()
    _check_abs(site, "mxm_em_step", instance, "posterior", got, exact, oracle_post, len(mat), n_haps, vec)


# ---------------------------------------------------------------- the argmax entries
def _assert_margin(V):
    """From the reference alone: every row's exact maximum is MARGIN above the runner-up."""
    best, v1, v2 = xc.top_two(V)
    margin = (v1 - v2).astype(numpy.float64)
    assert numpy.isfinite(v1.astype(numpy.float64)).all() and margin.min() >= MARGIN, margin.min()
    assert margin.min() > 1e6 * U * float(numpy.abs(V).max())
    return best, float(margin.min())


def _check_labels(site, form, instance, best, votes, V, wts, n_haps):
    want, margin = _assert_margin(V)
    _record(site, form, instance, n_haps, len(want), "-", None, None, "smallest exact margin %.3g" % margin)
    assert numpy.array_equal(numpy.asarray(best).astype(numpy.int64), want), (form, instance, n_haps)      # every row
    assert numpy.array_equal(votes, xc.exact_votes(want, wts, n_haps)[0].astype(numpy.float64))


@pytest.mark.parametrize("instance,n_haps", _cases("argmax"))
def test_dense_argmax(instance, n_haps):
    """row_argmax_wide_kernel<NCH> on continuous values: the label of every row, the votes exactly."""
    import torch
    from mixemt_amd import assign
    n_rows = inst.rows_for(instance)
    rng = numpy.random.default_rng(9000 + n_haps)
    X = rng.normal(-20.0, 6.0, size=(n_rows, n_haps))
    # (a row whose maximum is its LAST column, one whose maximum is its first: the two ends of the class's tail)
    X[0, n_haps - 1] = X[0].max() + 3.0
    X[n_rows - 1, 0] = X[n_rows - 1].max() + 3.0
    wts = inputs.weights(n_rows)
    x_d = torch.from_numpy(X).cuda()
    assert n_haps % 2 == 0 and _aligned(x_d)
    best, votes = assign.row_argmax_votes(x_d, wts)
    _check_labels("argmax", "mxm_row_argmax_votes", instance, best, votes, X.astype(_exact.LD), wts, n_haps)
    assert best[0] == n_haps - 1 and best[n_rows - 1] == 0


def _coded_matrix(plan, mat):
    import torch
    from mixemt_amd import preprocess
    rest = torch.nonzero(plan.coded_ndist == 0).flatten()
    assert int(rest.numel()) == 0
    return preprocess.CodedMatrix(len(mat), mat.shape[1], *plan._coded_keep[:3], plan.rowmax, 0, rest, plan.mat[rest].contiguous())


@pytest.mark.parametrize("instance,n_haps", _cases("argmax_coded"))
def test_records_argmax(b17, instance, n_haps):
    """records_argmax_narrow_kernel<NCH> (+ records_argmax_kernel<NCH, true> for the wide records), one run: argmax_h of
    ln_p[h] + M[r][h] with a continuous ln_p."""
    from mixemt_amd import assign
    label, mat, wts = _rows_of(b17, n_haps, instance, extra_wide=n_haps >= 257)
    plan = one_pass._coded_plan(mat, wts)
    assert plan.coded_rest == 0 and (n_haps < 257 or plan.coded_wide >= 1)
    cm = _coded_matrix(plan, mat)
    ln = numpy.random.default_rng(9100 + n_haps).normal(-20.0, 6.0, size=n_haps)
    # (the last column of the class wins row 0 outright, by 3: the tail of the last chunk decides a label)
    ln[n_haps - 1] = float((ln[:-1] + mat[0, :-1]).max() - mat[0, n_haps - 1]) + 3.0
    V = xc.exact_vote_values(mat, ln)
    best, votes = assign.row_argmax_votes_records(cm, ln, wts)
    _check_labels("argmax_coded", "mxm_row_argmax_votes_coded", instance, best, votes, V, wts, n_haps)
    assert best[0] == n_haps - 1


# ---------------------------------------------------------------- records: encoder, passes, quads, samples
@pytest.mark.parametrize("instance,n_haps", _cases("encode_rows"))
def test_encode_decode_round_trip(b17, instance, n_haps):
    """encode_rows_kernel<NCH> + encode_wide_rows_kernel<NCH>: the decoded records are mxm_linearize's rows bit for bit."""
    import torch
    from mixemt_amd import em
    label, mat, wts = _rows_of(b17, n_haps, instance, extra_wide=n_haps >= 257)
    dense = em.EmPlan(mat, wts)
    plan = one_pass._coded_plan(mat, wts)
    assert plan.coded_rest == 0 and plan.mat.data_ptr() % 8 == 0 and (n_haps < 257 or plan.coded_wide >= 1)
    dec = one_pass._decoded(plan)
    lin = dense.lin[:, :n_haps].cpu().numpy()
    _record("encode_rows", "mxm_encode_rows / mxm_decode_rows", instance, n_haps, len(mat), "-", None, None, "%d wide records" % plan.coded_wide)
    assert numpy.array_equal(one_pass._bits(dec), one_pass._bits(lin))
    assert torch.equal(plan.rowmax, dense.rowmax)


@pytest.mark.parametrize("instance,n_haps", _cases("em_iter_coded"))
def test_records_pass(b17, instance, n_haps):
    """em_iter_coded_kernel<256, NCH, 4, 2>: byte-coded rows and (from 257 columns) a wide record, no quad dictionary."""
    label, mat, wts = _rows_of(b17, n_haps, instance, extra_wide=n_haps >= 257)
    plan = one_pass._coded_plan(mat, wts)
    assert plan.coded_rest == 0 and plan.coded.n_quad_rows == 0 and not plan.coded.qrec
    _pass("em_iter_coded", "mxm_em_iter_coded, records", instance, plan, one_pass._decoded(plan), label, wts, n_haps, _names(instance))


@pytest.mark.parametrize("instance,n_haps", _cases("em_iter_rest"))
def test_records_pass_with_a_dense_rest(b17, instance, n_haps):
    """em_iter_wide_kernel<256, NCH, 1, 2, 1>: the rows of a records plan that get no record -- here one row of 1025
    distinct values beside the coded ones -- go through the 256-thread shape of the streaming kernel, behind the records pass."""
    import _class_rows
    label, mat, wts = _rows_of(b17, n_haps, instance)
    mat = numpy.array(mat)
    mat[0] = _class_rows.rows_with_values(n_haps, [1025], seed=n_haps, layout="shuffled")[0]
    label += " + a row of 1025 values"
    assert wts[0] > 0
    plan = one_pass._coded_plan(mat, wts)
    c = plan.coded
    assert plan.coded_rest == 1 == c.R_rest and c.ldp_rest % 2 == 0 and c.P_rest % 16 == 0 and c.n_quad_rows == 0
    _pass("em_iter_rest", "mxm_em_iter_coded, records + dense rest", instance, plan, one_pass._decoded(plan), label, wts, n_haps, _names(instance))


def _quad_plan(b17, n_haps, instance, leftover, n_runs=1):
    label, mat, wts = _rows_of(b17, n_haps, instance, extra_wide=leftover, quads_only=True)
    plan = one_pass._coded_plan(mat, wts, n_runs=n_runs)
    assert plan.attach_quads(True) and plan.coded.qrec
    c = plan.coded
    assert plan.coded_rest == 0 and c.n_quad_rows + c.n_byte_rows + c.n_wide == len(mat) and c.n_quad_rows > 0
    if leftover:
        assert c.n_byte_rows + c.n_wide >= 1
    else:
        assert c.n_byte_rows == 0 and c.n_wide == 0
    return label, mat, wts, plan


@pytest.mark.parametrize("instance,n_haps", _cases("quad"))
def test_quad_pass(b17, instance, n_haps):
    """em_iter_quad_kernel<NCH, 4>: every row a quad row."""
    label, mat, wts, plan = _quad_plan(b17, n_haps, instance, False)
    _pass("quad", "mxm_em_iter_coded, quads alone", instance, plan, one_pass._decoded(plan), label, wts, n_haps, _names(instance))


@pytest.mark.parametrize("instance,n_haps", _cases("quad_coded"))
def test_quad_pass_beside_leftover_rows(b17, instance, n_haps):
    """em_iter_quad_coded_kernel<NCH, 4>: the quad rows and a wide record in one grid (the table starts the first class at
    257 columns: a narrower row is byte-coded with at most 64 quads -- always a quad row)."""
    label, mat, wts, plan = _quad_plan(b17, n_haps, instance, True)
    _pass("quad_coded", "mxm_em_iter_coded, quads + leftover", instance, plan, one_pass._decoded(plan), label, wts, n_haps, _names(instance))


@pytest.mark.parametrize("instance,n_haps", _cases("quad_batched"))
def test_batched_quad_pass(b17, instance, n_haps):
    """em_iter_quad_batched_kernel<3, NCH, 1> and, from 257 columns (a leftover row), <3, NCH, 6>: three restarts per pass."""
    label, mat, wts, plan = _quad_plan(b17, n_haps, instance, n_haps >= 257, n_runs=3)
    assert plan.restart_tile() == 3 == plan.lib.mxm_restart_tile_coded(ctypes.byref(plan.coded), n_haps)
    _pass("quad_batched", "mxm_em_iter_coded, quads, B = 3", instance, plan, one_pass._decoded(plan), label, wts, n_haps, _names(instance, 3))


@pytest.mark.parametrize("instance,n_haps", _cases("samples"))
def test_many_samples_pass(b17, instance, n_haps):
    """em_iter_samples_kernel<NCH, 4>: the rows as two samples (one row; the rest), each against its own reference."""
    import torch
    from mixemt_amd import em
    label, mat, wts = _rows_of(b17, n_haps, instance, extra_wide=n_haps >= 257)
    plan = one_pass._coded_plan(mat, wts, keep_log_matrix=False)
    assert plan.coded_rest == 0 and not plan.coded.qrec
    lin = one_pass._decoded(plan)
    row0 = numpy.array([0, 1, len(mat)], dtype=numpy.int64)
    rec, rec_off, ndist = plan._coded_keep[:3]
    batch = em.SampleBatch(rec, rec_off, ndist, plan.wts, row0, n_haps)
    names = [VECTORS[instance % 2], VECTORS[(instance + 1) % 2]]
    props, ln = one_pass._stack(one_pass._vectors(n_haps), names)
    p = torch.from_numpy(props).to(batch.dev)
    colsum = torch.full_like(p, float("nan"))
    state = em.new_state(2, batch.dev)
    batch.em_iter(p, state, colsum)
    torch.cuda.synchronize()
    em.read_state(state)
    got = colsum.cpu().numpy()
    for s, vec in enumerate(names):
        lo, hi = int(row0[s]), int(row0[s + 1])
        sub = numpy.ascontiguousarray(lin[lo:hi])
        ref = _linear_ref("%s, rows %d:%d" % (label, lo, hi), vec, sub, props[s], wts[lo:hi])
        _check_T("samples", "mxm_em_iter_samples", instance, ref, got[s], hi - lo, n_haps, vec)


# ---------------------------------------------------------------- the builders: the C oracle's bits
def _tables(b17, n_haps):
    """HapVarTables of the first n_haps haplogroups (beyond Build 17's 5408: the list taken twice -- columns repeat, which
    no kernel can tell)."""
    from mixemt_amd import preprocess
    refseq, phy, haps, tables = b17
    if n_haps == len(haps):
        return tables
    if n_haps not in _tab:
        _tab.clear()                                    # (one table at a time: 30 MB each)
        _tab[n_haps] = preprocess.HapVarTables.build(refseq, phy, (haps + haps)[:n_haps])
    return _tab[n_haps]


_csr = {}
_tab = {}


def _observations(b17, n_rows, long_rows):
    """CSR rows over the whole tree's variant sites (every sub-tree's tables share them): 150-bp reads (at most 64
    observations each), or merged pairs of 65 .. 128 observations."""
    from mixemt_amd import synth
    refseq, phy, haps, tables = b17
    if long_rows not in _csr:
        if long_rows:
            row_ptr, site, obs, _ = synth.synth_pairs(tables, len(refseq), 400, seed=71)
        else:
            row_ptr, site, obs, _ = synth.synth_reads(tables, len(refseq), 200, seed=72)
        n = numpy.diff(row_ptr)
        keep = numpy.flatnonzero((n >= 65) & (n <= 128)) if long_rows else numpy.flatnonzero((n >= 1) & (n <= 64))
        assert len(keep) >= 64
        _csr[long_rows] = (row_ptr, site, obs, keep[:64])
    row_ptr, site, obs, keep = _csr[long_rows]
    keep = keep[:n_rows]
    parts = [(site[row_ptr[r]:row_ptr[r + 1]], obs[row_ptr[r]:row_ptr[r + 1]]) for r in keep]
    ptr = numpy.zeros(n_rows + 1, dtype=numpy.int64)
    numpy.cumsum([len(p[0]) for p in parts], out=ptr[1:])
    return ptr, numpy.concatenate([p[0] for p in parts]), numpy.concatenate([p[1] for p in parts])


def _build_case(b17, site_name, kernel, instance, n_haps, long_rows):
    from mixemt_amd import preprocess
    tables = _tables(b17, n_haps)
    assert tables.n_haps == n_haps and tables.lut() is not None
    n_rows = inst.rows_for(instance)
    row_ptr, site, obs = _observations(b17, n_rows, long_rows)
    want = c_oracle.build_em_matrix(tables.expected, tables.lhit, tables.lmiss, row_ptr, site, obs, n_haps)
    got = preprocess.build_em_matrix_device(tables, row_ptr, site, obs, kernel=kernel, sort_rows=False).cpu().numpy()
    left = preprocess.build_em_matrix_device.last_fallback if kernel == "sparse" else 0
    _record(site_name, "build, kernel = %s%s" % (kernel, ", long rows" if long_rows else ""), instance, n_haps, n_rows, "-", None, None,
            "%d rows left to the fallback list" % left)
    assert got.shape == want.shape and numpy.array_equal(one_pass._bits(got), one_pass._bits(want))
    return left


@pytest.mark.parametrize("instance,n_haps", _cases("build_lut"))
def test_lut_build(b17, instance, n_haps):
    """build_lut_kernel<NT, LUT_CPL>."""
    _build_case(b17, "build_lut", "lut", instance, n_haps, False)


@pytest.mark.parametrize("instance,n_haps", _cases("build_sparse"))
def test_marker_build(b17, instance, n_haps):
    """build_sparse_kernel<N, P, false, 1>: rows of up to 64 observations, none of them left to the fallback list."""
    assert _build_case(b17, "build_sparse", "sparse", instance, n_haps, False) == 0


@pytest.mark.parametrize("instance,n_haps", _cases("build_sparse_long"))
def test_marker_build_long_rows(b17, instance, n_haps):
    """build_sparse_kernel<N, ceil(N / 2), false, 2>: rows of 65 .. 128 observations.  The fallback list takes only rows
    beyond the long instance's own limits (704 masks, 5120 marker entries): at most a few of the widest tables' rows."""
    n_rows = inst.rows_for(instance)
    assert _build_case(b17, "build_sparse_long", "sparse", instance, n_haps, True) < max(2, n_rows // 2)


def _records_build_case(b17, site_name, instance, n_haps, long_rows):
    """mxm_build_em_records with the dense matrix beside the records: M the C oracle's bits; every record decodes to
    mxm_linearize's row of that matrix bit for bit, its rowmax the row's maximum."""
    import torch
    from mixemt_amd import _lib, em, preprocess
    from mixemt_amd._dev import current_stream
    tables = _tables(b17, n_haps)
    assert tables.n_haps == n_haps and tables.lut() is not None
    n_rows = inst.rows_for(instance)
    row_ptr, site, obs = _observations(b17, n_rows, long_rows)
    want = c_oracle.build_em_matrix(tables.expected, tables.lhit, tables.lmiss, row_ptr, site, obs, n_haps)
    cm, mat = preprocess.build_em_records_device(tables, row_ptr, site, obs, dense=True)
    left = preprocess.build_em_matrix_device.last_fallback
    nd = cm.ndist_host()
    _record(site_name, "records build%s" % (", long rows" if long_rows else ""), instance, n_haps, n_rows, "-", None, None,
            "%d rows left to the fallback list, %d wide records" % (left, int((nd > 256).sum())))
    assert numpy.array_equal(one_pass._bits(mat.cpu().numpy()), one_pass._bits(want))
    assert (nd > 0).all() and int(cm.rest_rows.numel()) == 0          # (no row of these has more than 1024 values)
    out = torch.full((n_rows, n_haps), float("nan"), dtype=torch.float64, device=cm.rec.device)
    coded = cm.struct()
    _lib.check(_lib.load().mxm_decode_rows(ctypes.byref(coded), n_haps, out.data_ptr(), out.stride(0), current_stream()), "mxm_decode_rows")
    lin = em.EmPlan(numpy.array(want), numpy.ones(n_rows)).lin[:, :n_haps].cpu().numpy()
    assert numpy.array_equal(one_pass._bits(out.cpu().numpy()), one_pass._bits(lin))
    assert numpy.array_equal(cm.rowmax.cpu().numpy(), want.max(axis=1))
    return left


@pytest.mark.parametrize("instance,n_haps", _cases("build_records"))
def test_records_build(b17, instance, n_haps):
    """build_sparse_kernel<N, P, true, 1>: rows of up to 64 observations, none of them left to the fallback list."""
    assert _records_build_case(b17, "build_records", instance, n_haps, False) == 0


@pytest.mark.parametrize("instance,n_haps", _cases("build_records_long"))
def test_records_build_long_rows(b17, instance, n_haps):
    """build_sparse_kernel<N, ceil(N / 2), true, 2>: rows of 65 .. 128 observations (the fallback list as in
    test_marker_build_long_rows)."""
    n_rows = inst.rows_for(instance)
    assert _records_build_case(b17, "build_records_long", instance, n_haps, True) < max(2, n_rows // 2)


# ---------------------------------------------------------------- the one-launch loops: three iterations
K_LOOP = 3


def _loop_case(site, form, instance, plan, X, label, wts, n_haps, mode, log_space=False):
    vec = _names(instance)[0]
    props, ln = one_pass._vectors(n_haps)[vec]
    plan.lib.mxm_set_loop_fused(mode, 0)
    assert loops._takes_one_launch(plan, props, ln), (form, n_haps)
    ref = loops._ref(X, props, ln, wts, log_space, steps=K_LOOP)
    run = loops._loop(plan, props[None, :], ln[None, :], 0.0, K_LOOP)
    err = loops.traj.ln_error(run.ln_new[0], ref["exact"].ln[K_LOOP])
    _record(site, form, instance, n_haps, len(wts), vec, None, None, "ln_new error %.3g after %d iterations" % (err, K_LOOP))
    loops._check(form, run, 0, ref, K_LOOP, 2, vec, False, record=False)


@pytest.mark.parametrize("instance,n_haps", _cases("fused_rows"))
def test_one_launch_loop_rows_split(b17, instance, n_haps):
    """em_fused_loop_kernel<NCH, FUSED_NBUF> (mxm_set_loop_fused(2))."""
    from mixemt_amd import em
    label, mat, wts = _rows_of(b17, n_haps, instance)
    plan = em.EmPlan(mat, wts)
    assert plan.lin is not None and _aligned(plan.lin)
    _loop_case("fused_rows", "mxm_em_loop, one launch, rows split", instance, plan, loops._lin_of(plan), label, wts, n_haps, 2)


@pytest.mark.parametrize("instance,n_haps", _cases("fused_cols"))
def test_one_launch_loop_columns_split(b17, instance, n_haps):
    """em_fused_cols_kernel<12 / 22 / 24, 1> (mxm_set_loop_fused(1)) on a device of 256 CUs."""
    import torch
    from mixemt_amd import em
    if torch.cuda.get_device_properties(0).multi_processor_count != inst.CUS:
        pytest.skip("the columns-split loop needs a grid of exactly 256 workgroups")
    label, mat, wts = _rows_of(b17, n_haps, instance)
    plan = em.EmPlan(mat, wts)
    assert plan.lin is not None and _aligned(plan.lin)
    _loop_case("fused_cols", "mxm_em_loop, one launch, columns split", instance, plan, loops._lin_of(plan), label, wts, n_haps, 1)


@pytest.mark.parametrize("instance,n_haps", _cases("fused_coded"))
def test_one_launch_loop_over_records(b17, instance, n_haps):
    """em_fused_coded_kernel<CNCH, 4, true> (mxm_set_loop_fused(1)) on 64 rows: the widest width a grid of 48 workgroups takes."""
    label, mat, wts = _rows_of(b17, n_haps, 2, extra_wide=n_haps >= 257)         # (rows_for(2) = 64 for every instance: see the table)
    assert len(mat) == 64
    plan = one_pass._coded_plan(mat, wts)
    assert plan.coded_rest == 0 and n_haps % 2 == 0
    _loop_case("fused_coded", "mxm_em_loop_coded, one launch", instance, plan, one_pass._decoded(plan), label, wts, n_haps, 1)


@pytest.mark.parametrize("instance,n_haps", _cases("fused_narrow"))
def test_narrow_one_launch_loop(b17, instance, n_haps):
    """em_fused_narrow_kernel<4 / 8 / 16, 1> in log space."""
    from mixemt_amd import em
    n_rows = inst.rows_for(instance)
    mat, wts = numpy.array(inputs.few_values(64, n_haps)[:n_rows]), inputs.weights(n_rows)
    plan = em.EmPlan(mat, wts)
    assert plan.lin is None
    _loop_case("fused_narrow", "mxm_em_loop, narrow one-launch loop", instance, plan, mat, "few values %d" % n_haps, wts, n_haps, 1, log_space=True)
