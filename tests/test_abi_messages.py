"""
What the C ABI says when it refuses a call: the exact return code and the exact bytes of mxm_last_error(), entry point
by entry point.  Every row is refused by the host code before its first HIP call (shape and pointer checks), so the
table needs no device; the pointers that are not NULL are never followed.
"""
import ctypes

import pytest

from mixemt_amd import _lib

PTR = 0x1000                 # "some pointer": 32-byte aligned, never dereferenced by a row below
ODD = 0x1004                 # ... one that is only 4-byte aligned


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import build
    build.build()
    return _lib.load()


def _coded(**kw):
    """A mxm_coded that passes coded_check unless a field says otherwise."""
    c = _lib.Coded()
    c.rec, c.rec_off, c.ndist, c.R = PTR, PTR, PTR, 10
    for key, val in kw.items():
        setattr(c, key, val)
    return ctypes.byref(c)


def _quads(**kw):
    """... with a quad dictionary whose lists cover the ten rows."""
    fields = dict(qrec=PTR, qoff=PTR, nquad=PTR, quad_rows=PTR, n_quad_rows=6, byte_rows=PTR, n_byte_rows=4)
    fields.update(kw)
    return _coded(**fields)


def _i64(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _i32(*vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _cols(n_aln=0, n_frag=0, **kw):
    c = _lib.AlnColumns()
    c.n_aln, c.n_frag = n_aln, n_frag
    for key, val in kw.items():
        setattr(c, key, val)
    return ctypes.byref(c)


STATES = (_lib.EmState * 4)()
ROW0_ONE = _i64(0, 10)                                   # one sample of ten rows
NULL_INPUTS = (ctypes.c_void_p * 1)(None)
LD_INPUTS = _i64(100)
OUT_HANDLE = ctypes.c_void_p()

# (entry point, arguments, return code, message)
TABLE = [
    # ---- the builds ------------------------------------------------------------------------------------------------
    ("mxm_build_em_matrix", (PTR, 8, PTR, PTR, PTR, PTR, PTR, -1, 5, 1, PTR, 8, None), -1,
     "mxm_build_em_matrix: bad shape R=-1 H=5"),
    ("mxm_build_em_matrix", (ODD, 8, PTR, PTR, PTR, PTR, PTR, 4, 5, 1, PTR, 8, None), -1,
     "mxm_build_em_matrix: E must be 8-byte aligned with lde a multiple of 8 and >= H rounded up to 8 (lde=8)"),
    ("mxm_build_em_matrix", (PTR, 8, PTR, PTR, PTR, PTR, PTR, 4, 5, 1, PTR, 4, None), -1, "mxm_build_em_matrix: ldm < H"),
    ("mxm_build_em_matrix", (PTR, 8, PTR, PTR, PTR, PTR, PTR, 4, 5, 65537, PTR, 8, None), -1,
     "mxm_build_em_matrix: more than 65536 variant sites"),
    ("mxm_build_em_matrix_lut", (PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, None, 4, 0, 1, PTR, 8, None), -1,
     "mxm_build_em_matrix_lut: bad shape R=4 H=0"),
    ("mxm_build_em_matrix_lut", (PTR, 9008, PTR, PTR, PTR, PTR, PTR, PTR, None, 4, 9000, 1, PTR, 9000, None), -1,
     "mxm_build_em_matrix_lut: more than 8192 haplogroups (H=9000): use mxm_build_em_matrix"),
    ("mxm_build_em_matrix_lut", (PTR, 12, PTR, PTR, PTR, PTR, PTR, PTR, None, 4, 5, 1, PTR, 8, None), -1,
     "mxm_build_em_matrix_lut: Ecode must be 8-byte aligned with lde a multiple of 8 and >= H rounded up to 8 (lde=12)"),
    ("mxm_build_em_matrix_lut", (PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, None, 4, 5, 1, PTR, 4, None), -1,
     "mxm_build_em_matrix_lut: ldm < H"),
    ("mxm_build_em_matrix_lut", (PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, None, 4, 5, 65537, PTR, 8, None), -1,
     "mxm_build_em_matrix_lut: table of 65537 x 8 bytes exceeds one buffer descriptor"),
    ("mxm_build_em_matrix_lut_rows", (PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, None, 4, 5, 1, PTR, 8, None), -1,
     "mxm_build_em_matrix_lut_rows: bad arguments"),
    ("mxm_build_em_matrix_lut_rows", (PTR, 9008, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 4, 9000, 1, PTR, 9000, None), -1,
     "mxm_build_em_matrix_lut_rows: more than 8192 haplogroups (H=9000)"),
    ("mxm_build_em_matrix_lut_rows", (PTR, 4, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 4, 5, 1, PTR, 8, None), -1,
     "mxm_build_em_matrix_lut_rows: Ecode must be 8-byte aligned with lde a multiple of 8 and >= H rounded up to 8 (lde=4)"),
    ("mxm_build_em_matrix_lut_rows", (PTR, 8, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 4, 5, 1, PTR, 4, None), -1,
     "mxm_build_em_matrix_lut_rows: ldm < H"),
    ("mxm_build_em_matrix_lut_rows", (PTR, 40000, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 4, 5, 60000, PTR, 8, None), -1,
     "mxm_build_em_matrix_lut_rows: table of 60000 x 40000 bytes exceeds one buffer descriptor"),
    ("mxm_scatter_records", (None, 3, PTR, PTR, PTR, 0, PTR, PTR, PTR, None), -1, "mxm_scatter_records: bad arguments"),
    # build_sparse_impl (who) through its two callers
    ("mxm_build_em_matrix_sparse", (PTR,) * 10 + (4, 5, 1, None, 8, PTR, PTR, None), -1, "mxm_build_em_matrix_sparse: M required"),
    ("mxm_build_em_matrix_sparse", (PTR,) * 10 + (-4, 5, 1, PTR, 8, PTR, PTR, None), -1,
     "mxm_build_em_matrix_sparse: bad shape R=-4 H=5"),
    ("mxm_build_em_matrix_sparse", (PTR,) * 10 + (4, 8193, 1, PTR, 8193, PTR, PTR, None), -1,
     "mxm_build_em_matrix_sparse: more than 8192 haplogroups (H=8193): use mxm_build_em_matrix"),
    ("mxm_build_em_matrix_sparse", (PTR,) * 10 + (4, 5, 1, PTR, 4, PTR, PTR, None), -1, "mxm_build_em_matrix_sparse: ldm < H"),
    ("mxm_build_em_matrix_sparse", (None,) + (PTR,) * 9 + (4, 5, 1, PTR, 8, PTR, PTR, None), -1,
     "mxm_build_em_matrix_sparse: marker tables and the fallback list are required"),
    ("mxm_build_em_records", (PTR,) * 10 + (4, 10, 1, None, 0, PTR, 1 << 20, PTR, PTR, PTR, PTR, PTR, PTR, None), -1,
     "mxm_build_em_records: records need H in [65, 8192] (H=10)"),
    ("mxm_build_em_records", (PTR,) * 10 + (4, 100, 1, None, 0, ODD, 1 << 20, PTR, PTR, PTR, PTR, PTR, PTR, None), -1,
     "mxm_build_em_records: record buffer (16-byte aligned, >= one record) and output arrays required"),
    ("mxm_build_em_records", (PTR,) * 10 + (-1, 100, 1, None, 0, PTR, 1 << 20, PTR, PTR, PTR, PTR, PTR, PTR, None), -1,
     "mxm_build_em_records: bad shape R=-1 H=100"),
    ("mxm_build_em_records", (PTR,) * 10 + (4, 100, 1, PTR, 99, PTR, 1 << 20, PTR, PTR, PTR, PTR, PTR, PTR, None), -1,
     "mxm_build_em_records: ldm < H"),
    ("mxm_build_em_records", (PTR,) * 10 + (4, 100, 1, None, 0, PTR, 1 << 20, PTR, PTR, PTR, PTR, None, PTR, None), -1,
     "mxm_build_em_records: marker tables and the fallback list are required"),
    ("mxm_expand_tables", (PTR, PTR, PTR, PTR, PTR, 4, 10, 9, PTR, None), -1, "mxm_expand_tables: bad arguments"),
    # ---- dense EM -----------------------------------------------------------------------------------------------------
    ("mxm_linearize", (PTR, 8, -1, 5, PTR, 8, PTR, None), -1, "mxm_linearize: bad shape"),
    ("mxm_linearize", (PTR, 8, 4, 5, PTR, 7, PTR, None), -1, "mxm_linearize: ldp must be even and >= H (ldp=7)"),
    ("mxm_linearize_f32", (PTR, 8, 4, 0, PTR, 8, PTR, None), -1, "mxm_linearize_f32: bad shape"),
    ("mxm_linearize_f32", (PTR, 8, 4, 5, PTR, 6, PTR, None), -1, "mxm_linearize_f32: ldp must be a multiple of 4 and >= H (ldp=6)"),
    ("mxm_em_iter", (PTR, 8, None, 0, PTR, PTR, PTR, 0, 5, 1, PTR, PTR, PTR, 1 << 30, None), -1, "mxm_em_iter: bad shape R=0 H=5"),
    ("mxm_em_iter", (PTR, 8, None, 0, PTR, PTR, PTR, 4, 5, 1, PTR, PTR, None, 1 << 30, None), -1, "mxm_em_iter: workspace too small"),
    ("mxm_em_iter", (PTR, 8, PTR, 7, PTR, PTR, PTR, 4, 5, 1, PTR, PTR, PTR, 1 << 30, None), -1, "mxm_em_iter: ldp must be even and >= H"),
    ("mxm_em_iter", (PTR, 4, None, 0, PTR, PTR, PTR, 4, 5, 1, PTR, PTR, PTR, 1 << 30, None), -1, "mxm_em_iter: ldm < H"),
    ("mxm_em_iter_f32", (PTR, 100, PTR, PTR, 4, 100, 0, PTR, PTR, PTR, 1 << 30, None), -1, "mxm_em_iter_f32: bad shape R=4 H=100"),
    ("mxm_em_iter_f32", (PTR, 12, PTR, PTR, 4, 10, 1, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_f32: H=10 outside the linear kernel's range"),
    ("mxm_em_iter_f32", (PTR, 102, PTR, PTR, 4, 100, 1, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_f32: ldp must be a multiple of 4 and >= H"),
    ("mxm_em_iter_f32", (PTR, 100, PTR, PTR, 4, 100, 1, PTR, PTR, PTR, 16, None), -1, "mxm_em_iter_f32: workspace too small"),
    ("mxm_m_finalize", (PTR, PTR, PTR, PTR, 5, 1, 1e-4, 10, None, None), -1, "mxm_m_finalize: bad arguments"),
    ("mxm_em_loop", (PTR, 8, None, 0, PTR, 4, 5, 1, PTR, PTR, PTR, PTR, None, 1e-4, 10, 5, PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop: state pointers required"),
    ("mxm_em_loop", (PTR, 8, None, 0, PTR, 4, -5, 1, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop: bad shape R=4 H=-5"),
    ("mxm_em_loop", (PTR, 8, None, 0, PTR, 4, 5, 1, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 16, None, STATES), -1,
     "mxm_em_loop: workspace too small"),
    ("mxm_em_loop_f32", (PTR, 100, PTR, 4, 100, 1, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, None), -1,
     "mxm_em_loop: state pointers required"),
    ("mxm_em_loop_f32", (PTR, 100, PTR, 0, 100, 1, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop: bad shape R=0 H=100"),
    ("mxm_em_step", (PTR, 4, PTR, PTR, 4, 5, PTR, 8, 0, None, None, 0, None), -1, "mxm_em_step: bad shape"),
    ("mxm_em_step", (PTR, 8, PTR, PTR, 4, 5, PTR, 4, 0, None, None, 0, None), -1, "mxm_em_step: ldo < H"),
    ("mxm_em_step", (PTR, 8, PTR, PTR, 4, 5, PTR, 8, 0, PTR, None, 0, None), -1, "mxm_em_step: workspace too small"),
    ("mxm_log_normalize", (PTR, 0, PTR, None), -1, "mxm_log_normalize: H <= 0"),
    ("mxm_l1_exp_diff", (PTR, PTR, -1, PTR, None), -1, "mxm_l1_exp_diff: H <= 0"),
    ("mxm_add_scalar", (PTR, 4, 4, 5, 1.0, None), -1, "mxm_add_scalar: bad shape"),
    ("mxm_assign_reads", (PTR, 8, PTR, PTR, 0, 4, 5, -1.0, PTR, None), -1, "mxm_assign_reads: bad shape"),
    ("mxm_row_argmax_votes", (PTR, 4, PTR, 4, 5, PTR, None, None, 0, None), -1, "mxm_row_argmax_votes: bad shape"),
    ("mxm_row_argmax_votes", (PTR, 8, PTR, 4, 5, PTR, PTR, None, 0, None), -1, "mxm_row_argmax_votes: workspace too small"),
    ("mxm_first_seen", (None, 4, 5, PTR, None), -1, "mxm_first_seen: bad arguments"),
    ("mxm_gather_columns", (PTR, 8, 4, 5, PTR, 3, PTR, 2, None), -1, "mxm_gather_columns: bad shape"),
    ("mxm_fold_logaddexp", (PTR, 100, NULL_INPUTS, LD_INPUTS, 9, 4, 100, 0.0, None), -1,
     "mxm_fold_logaddexp: bad shape (at most 8 inputs per call)"),
    ("mxm_fold_logaddexp", (PTR, 100, NULL_INPUTS, LD_INPUTS, 1, 4, 100, 0.0, None), -1, "mxm_fold_logaddexp: bad input 0"),
    # ---- records: coded_check (who) through its callers, then each caller's own refusals ---------------------------------
    ("mxm_decode_rows", (None, 100, PTR, 100, None), -1, "mxm_decode_rows: bad coded matrix (rows 0, H 100)"),
    ("mxm_decode_rows", (_coded(), 64, PTR, 100, None), -1, "mxm_decode_rows: bad coded matrix (rows 10, H 64)"),
    ("mxm_decode_rows", (_coded(rec_off=None), 100, PTR, 100, None), -1, "mxm_decode_rows: coded matrix arrays missing"),
    ("mxm_decode_rows", (_coded(R_rest=2, P_rest=PTR, ldp_rest=101), 100, PTR, 100, None), -1,
     "mxm_decode_rows: the dense rest needs 16-byte aligned rows with an even ld >= H"),
    ("mxm_decode_rows", (_coded(n_wide=1), 100, PTR, 100, None), -1, "mxm_decode_rows: n_wide > 0 needs wide_rows"),
    ("mxm_decode_rows", (_quads(nquad=None), 100, PTR, 100, None), -1,
     "mxm_decode_rows: quad dictionary arrays missing (or qrec not 32-byte aligned)"),
    ("mxm_decode_rows", (_quads(n_byte_rows=3), 100, PTR, 100, None), -1,
     "mxm_decode_rows: quad_rows + byte_rows + wide_rows + the dense rest must be all 10 rows"),
    ("mxm_decode_rows", (_coded(), 100, PTR, 99, None), -1, "mxm_decode_rows: ldp < H"),
    ("mxm_em_iter_coded", (_quads(n_quad_rows=7), PTR, PTR, 100, 1, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_coded: quad_rows + byte_rows + wide_rows + the dense rest must be all 10 rows"),
    ("mxm_em_iter_coded", (_coded(), PTR, PTR, 100, 0, PTR, PTR, PTR, 1 << 30, None), -1, "mxm_em_iter_coded: bad arguments"),
    ("mxm_em_iter_coded", (_coded(), PTR, PTR, 100, 1, PTR, PTR, PTR, 16, None), -1, "mxm_em_iter_coded: workspace too small"),
    ("mxm_em_loop_coded", (None, PTR, 8193, 1, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop_coded: bad coded matrix (rows 0, H 8193)"),
    ("mxm_em_loop_coded", (_coded(), PTR, 100, 1, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, None, 1 << 30, None, STATES), -1,
     "mxm_em_loop_coded: workspace too small"),
    ("mxm_build_quads", (None, 100, PTR, 1 << 20, PTR, PTR, PTR, None), -1, "mxm_build_quads: bad coded matrix (rows 0, H 100)"),
    ("mxm_build_quads", (_coded(), 10, PTR, 1 << 20, PTR, PTR, PTR, None), -1, "mxm_build_quads: bad coded matrix (rows 10, H 10)"),
    ("mxm_build_quads", (_coded(), 100, ODD, 1 << 20, PTR, PTR, PTR, None), -1,
     "mxm_build_quads: qoff, nquad, stats and a 32-byte aligned qrec required"),
    ("mxm_quad_lists", (PTR, PTR, 0, PTR, PTR, PTR, PTR, 1 << 20, None), -1, "mxm_quad_lists: bad arguments"),
    ("mxm_quad_lists", (PTR, PTR, 100, PTR, PTR, PTR, PTR, 0, None), -1, "mxm_quad_lists: scratch too small"),
    ("mxm_encode_rows", (PTR, 99, 4, 100, PTR, 1 << 20, PTR, PTR, PTR, PTR, None), -1, "mxm_encode_rows: bad shape R=4 H=100"),
    ("mxm_encode_rows", (PTR, 10, 4, 10, PTR, 1 << 20, PTR, PTR, PTR, PTR, None), -1,
     "mxm_encode_rows: needs H in [65, 8192] (H=10 ldm=10)"),
    ("mxm_encode_rows", (PTR, 100, 4, 100, PTR, 100, PTR, PTR, PTR, PTR, None), -1,
     "mxm_encode_rows: record buffer missing, unaligned or smaller than one record"),
    ("mxm_encode_rows", (PTR, 100, 4, 100, PTR, 1 << 20, PTR, PTR, PTR, None, None), -1, "mxm_encode_rows: output arrays required"),
    ("mxm_row_argmax_votes_coded", (_coded(n_wide=-1), 100, 1, PTR, None, None, None, 0, None, 0, None, PTR, None, None, 0, None), -1,
     "mxm_row_argmax_votes_coded: n_wide > 0 needs wide_rows"),
    ("mxm_row_argmax_votes_coded", (_coded(), 100, 0, PTR, None, None, None, 0, None, 0, None, PTR, None, None, 0, None), -1,
     "mxm_row_argmax_votes_coded: ln_props, best and 1..4096 runs required"),
    ("mxm_row_argmax_votes_coded", (_coded(), 100, 2, PTR, None, None, None, 0, None, 0, None, PTR, None, None, 0, None), -1,
     "mxm_row_argmax_votes_coded: several runs need props and rowmax (each run's row normaliser)"),
    ("mxm_row_argmax_votes_coded", (_coded(), 100, 1, PTR, None, None, None, 0, None, 2, None, PTR, None, None, 0, None), -1,
     "mxm_row_argmax_votes_coded: the rows without a record need M_rest, rest_rows and ldm_rest >= H"),
    ("mxm_row_argmax_votes_coded", (_coded(), 100, 1, PTR, None, None, None, 0, None, 0, None, PTR, PTR, None, 0, None), -1,
     "mxm_row_argmax_votes_coded: workspace too small"),
    ("mxm_em_step_coded", (_coded(R=0), 100, PTR, PTR, PTR, None, 0, None, 0, PTR, 100, 0, None), -1,
     "mxm_em_step_coded: bad coded matrix (rows 0, H 100)"),
    ("mxm_em_step_coded", (_coded(), 100, PTR, PTR, PTR, None, 0, None, 0, PTR, 99, 0, None), -1, "mxm_em_step_coded: bad arguments"),
    ("mxm_em_step_coded", (_coded(), 100, PTR, PTR, PTR, PTR, 99, PTR, 2, PTR, 100, 0, None), -1,
     "mxm_em_step_coded: the rows without a record need M_rest, rest_rows and ldm_rest >= H"),
    ("mxm_gather_columns_coded", (_coded(ndist=None), 100, PTR, 3, None, 0, None, 0, PTR, 3, None), -1,
     "mxm_gather_columns_coded: coded matrix arrays missing"),
    ("mxm_gather_columns_coded", (_coded(), 100, PTR, 3, None, 0, None, 0, PTR, 2, None), -1, "mxm_gather_columns_coded: bad arguments"),
    ("mxm_gather_columns_coded", (_coded(), 100, PTR, 3, None, 0, None, -1, PTR, 3, None), -1,
     "mxm_gather_columns_coded: the rows without a record need M_rest, rest_rows and ldm_rest >= H"),
    ("mxm_diag_stream_coded", (_coded(), 8200, 1, PTR, None), -1, "mxm_diag_stream_coded: bad coded matrix (rows 10, H 8200)"),
    ("mxm_diag_stream_coded", (_coded(), 5408, 0, PTR, None), -1, "mxm_diag_stream_coded: bad arguments"),
    ("mxm_diag_stream_coded", (_coded(), 100, 1, PTR, None), -1, "mxm_diag_stream_coded: built for H in (5120, 6144]"),
    ("mxm_diag_stream_quads", (_coded(rec=None), 100, 1, PTR, None), -1, "mxm_diag_stream_quads: coded matrix arrays missing"),
    ("mxm_diag_stream_quads", (_coded(), 100, 1, PTR, None), -1, "mxm_diag_stream_quads: a coded matrix with a quad dictionary required"),
    ("mxm_diag_stream_read", (None, 1 << 20, 1, 0, PTR, None), -1, "mxm_diag_stream_read: bad arguments"),
    ("mxm_diag_stream_read", (PTR, 100, 1, 3, PTR, None), -1, "mxm_diag_stream_read: buffer smaller than one record"),
    ("mxm_diag_stream_read", (PTR, 100, 1, 2, PTR, None), -1, "mxm_diag_stream_read: buffer smaller than one row"),
    ("mxm_diag_fused_stamps", (None, None), -1, "mxm_diag_fused_stamps: bad arguments"),
    # ---- many samples: the plan, then samples_check (who) through its two callers ---------------------------------------
    ("mxm_samples_plan", (None, 0, None, 0, None), -1, "mxm_samples_plan: bad arguments (S=0)"),
    ("mxm_samples_plan", (_i64(5, 10), 1, None, 0, None), -1, "mxm_samples_plan: row0[0] must be 0 (it is 5)"),
    ("mxm_samples_plan", (_i64(0, 10, 10), 2, None, 0, None), -1,
     "mxm_samples_plan: row0 must ascend and no sample may be empty (sample 1 has 0 rows)"),
    ("mxm_samples_plan", (_i64(0, 40, 140), 2, (_lib.SampleTile * 3)(), 3, None), -1,
     "mxm_samples_plan: room for 3 tiles, sample 1 needs more"),
    ("mxm_em_iter_samples", (_coded(), ROW0_ONE, 70000, PTR, PTR, 100, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_samples: bad arguments (S = 70000; 1 .. 65535 samples)"),
    ("mxm_em_iter_samples", (_coded(rec=None), ROW0_ONE, 1, PTR, PTR, 100, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_samples: coded matrix arrays missing (rows 10)"),
    ("mxm_em_iter_samples", (_coded(), ROW0_ONE, 1, PTR, PTR, 101, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_samples: H = 101: an even width in [66, 8192] is required"),
    ("mxm_em_iter_samples", (_quads(), ROW0_ONE, 1, PTR, PTR, 100, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_samples: a quad dictionary is attached; the batched pass reads the records only"),
    ("mxm_em_iter_samples", (_coded(), _i64(3, 10), 1, PTR, PTR, 100, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_samples_plan: row0[0] must be 0 (it is 3)"),
    ("mxm_em_iter_samples", (_coded(), _i64(0, 9), 1, PTR, PTR, 100, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_samples: row0[S] = 9, the matrix has 10 rows"),
    ("mxm_em_iter_samples", (_coded(), ROW0_ONE, 1, PTR, None, 100, PTR, PTR, PTR, 1 << 30, None), -1,
     "mxm_em_iter_samples: bad arguments"),
    ("mxm_em_iter_samples", (_coded(), ROW0_ONE, 1, PTR, PTR, 100, PTR, PTR, PTR, 16, None), -1,
     "mxm_em_iter_samples: workspace too small (or not 16-byte aligned)"),
    ("mxm_em_loop_samples", (_coded(), ROW0_ONE, 1, PTR, 67, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop_samples: H = 67: an even width in [66, 8192] is required"),
    ("mxm_em_loop_samples", (_coded(R_rest=2, P_rest=PTR, ldp_rest=100), ROW0_ONE, 1, PTR, 100, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5,
                             PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop_samples: 2 rows without a record (the dense rest): such a sample runs on its own"),
    ("mxm_em_loop_samples", (_coded(n_wide=2), ROW0_ONE, 1, PTR, 100, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop_samples: n_wide > 0 needs wide_rows"),
    ("mxm_em_loop_samples", (_coded(), _i64(0, 4, 12), 2, PTR, 100, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, STATES), -1,
     "mxm_em_loop_samples: row0[S] = 12, the matrix has 10 rows"),
    ("mxm_em_loop_samples", (_coded(), ROW0_ONE, 1, PTR, 100, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, PTR, 1 << 30, None, None), -1,
     "mxm_em_loop_samples: bad arguments"),
    ("mxm_em_loop_samples", (_coded(), ROW0_ONE, 1, PTR, 100, PTR, PTR, PTR, PTR, PTR, 1e-4, 10, 5, ODD, 1 << 30, None, STATES), -1,
     "mxm_em_loop_samples: workspace too small (or not 16-byte aligned)"),
    # ---- the knobs ----------------------------------------------------------------------------------------------------
    ("mxm_set_min_rows_per_wg", (0,), -1, "mxm_set_min_rows_per_wg: n < 1"),
    ("mxm_set_batch_tile", (5,), -1, "mxm_set_batch_tile: tile must be 1..4"),
    ("mxm_set_coded_batch_tile", (2,), -1, "mxm_set_coded_batch_tile: 1 or 3, got 2"),
    ("mxm_set_quad_encoder", (-7,), -1, "mxm_set_quad_encoder: 0 or 1, got -7"),
    ("mxm_describe_stream_kernel", (5408, 5, None, 0), -1, "mxm_describe_stream_kernel: bad arguments"),
    # ---- the exchange ---------------------------------------------------------------------------------------------------
    ("mxm_exchange_create", (17, 0, 100, ctypes.byref(OUT_HANDLE), PTR), -1,
     "mxm_exchange_create: 1..16 ranks, a rank among them and a slot size required"),
    ("mxm_exchange_connect", (None, PTR), -1, "mxm_exchange_connect: NULL argument"),
    ("mxm_exchange_push", (None, PTR, 10, None), -1, "mxm_exchange_push: bad arguments"),
    ("mxm_exchange_pull", (None, PTR, 10, None, 0, None), -1, "mxm_exchange_pull: bad arguments"),
    ("mxm_exchange_reduce", (None, PTR, 10, None, 0, None), -1, "mxm_exchange_reduce: bad arguments"),
    ("mxm_exchange_info", (None, None, None), -1, "mxm_exchange_info: NULL handle"),
    # ---- alignments: the encoder and the BAM reader (host code) ------------------------------------------------------------
    ("mxm_aln_encode", (_cols(), PTR, 100, PTR, 1, 20, 20, 1, None), -1, "mxm_aln_encode: out is NULL"),
    ("mxm_aln_encode", (_cols(), PTR, 0, PTR, 1, 20, 20, 1, ctypes.byref(OUT_HANDLE)), -1, "mxm_aln_encode: bad arguments"),
    ("mxm_aln_encode", (_cols(n_aln=3), PTR, 100, PTR, 1, 20, 20, 1, ctypes.byref(OUT_HANDLE)), -1,
     "mxm_aln_encode: alignment columns missing"),
    ("mxm_aln_sizes_of", (None, None), -1, "mxm_aln_sizes_of: NULL argument"),
    ("mxm_aln_fetch", (None,) * 10, -1, "mxm_aln_fetch: NULL handle"),
    ("mxm_aln_fetch_fragments", (None,) * 5, -1, "mxm_aln_fetch_fragments: NULL handle"),
    ("mxm_bam_read", (None, 1, ctypes.byref(OUT_HANDLE)), -1, "mxm_bam_read: NULL argument"),
    ("mxm_bam_read", (b"/no/such/dir/reads.bam", 1, None), -1, "mxm_bam_read: NULL argument"),
    ("mxm_bam_read", (b"/no/such/dir/reads.bam", 1, ctypes.byref(OUT_HANDLE)), -6, "mxm_bam_read: cannot open /no/such/dir/reads.bam"),
    ("mxm_bam_sizes_of", (None, None), -1, "mxm_bam_sizes_of: NULL argument"),
    ("mxm_bam_columns", (None, None), -1, "mxm_bam_columns: NULL argument"),
    ("mxm_bam_fetch_names", (None,) * 5, -1, "mxm_bam_fetch_names: NULL handle"),
    # ---- pileup and assembly: aln_columns_ok and asm_rows_from (who) through their callers ----------------------------------
    ("mxm_observe_bases", (None, None, 20, 20, 100, PTR, None), -1, "mxm_observe_bases: bad arguments"),
    ("mxm_observe_bases", (_cols(n_aln=1 << 31), None, 20, 20, 100, PTR, None), -1,
     "mxm_observe_bases: more than 2^31 - 1 alignments (2147483648)"),
    ("mxm_observe_bases", (_cols(n_aln=3), None, 20, 20, 100, PTR, None), -1,
     "mxm_observe_bases: ref_start, mapq, cig_ptr, cigar, seq_ptr and seq are required"),
    ("mxm_observe_bases_labelled", (_cols(n_aln=3), None, PTR, -2, 20, 20, 100, PTR, None), -1,
     "mxm_observe_bases_labelled: n_labels < 0 (-2)"),
    ("mxm_observe_bases_labelled", (_cols(n_aln=3, ref_start=PTR, mapq=PTR, cig_ptr=PTR, cigar=PTR, seq_ptr=PTR, seq=PTR), None, None, 2,
                                    20, 20, 100, PTR, None), -1, "mxm_observe_bases_labelled: label is required"),
    ("mxm_consensus", (PTR, -1, 100, 100, 1, 0, PTR, PTR, PTR, None), -1, "mxm_consensus: bad shape"),
    ("mxm_consensus", (PTR, 2, 100, 100, 1, 0, None, PTR, PTR, None), -1, "mxm_consensus: counts and cons are required"),
    ("mxm_consensus", (ODD, 2, 100, 100, 1, 0, PTR, PTR, PTR, None), -1, "mxm_consensus: counts must be 16-byte aligned"),
    ("mxm_new_variants", (PTR, 99, 4, _i32(0), 1, 100, PTR, PTR, None), -1, "mxm_new_variants: bad shape"),
    ("mxm_new_variants", (PTR, 100, 4, None, 1, 100, PTR, PTR, None), -1, "mxm_new_variants: bad participating rows"),
    ("mxm_new_variants", (PTR, 100, 4, _i32(0), 128, 100, PTR, PTR, None), -1,
     "mxm_new_variants: 128 participating contributors, at most 127 (an owner is an int8)"),
    ("mxm_new_variants", (PTR, 100, 4, _i32(1, 9), 2, 100, PTR, PTR, None), -1, "mxm_new_variants: participating row 9 is no row"),
    ("mxm_new_variants", (PTR, 100, 4, _i32(1), 1, 100, None, PTR, None), -1, "mxm_new_variants: cons, newvar and n_new are required"),
    ("mxm_first_observed", (None, PTR, PTR, 2, 20, 20, 100, PTR, PTR, None), -1, "mxm_first_observed: bad arguments"),
    ("mxm_first_observed", (_cols(n_aln=1 << 32), PTR, PTR, 2, 20, 20, 100, PTR, PTR, None), -1,
     "mxm_first_observed: more than 2^31 - 1 alignments (4294967296)"),
    ("mxm_first_observed", (_cols(), PTR, PTR, -1, 20, 20, 100, PTR, PTR, None), -1, "mxm_first_observed: bad shape"),
    ("mxm_first_observed", (_cols(n_aln=3, ref_start=PTR, mapq=PTR, cig_ptr=PTR, cigar=PTR, seq_ptr=PTR, seq=PTR), None, PTR, 2, 20, 20,
                            100, PTR, PTR, None), -1, "mxm_first_observed: label, tied and cons are required"),
    ("mxm_extend_assign", (_cols(n_aln=-1), PTR, PTR, 9, 4, _i32(0), 1, 0, 20, 20, PTR, 100, PTR, PTR, PTR, None), -1,
     "mxm_extend_assign: bad arguments"),
    ("mxm_extend_assign", (_cols(), PTR, PTR, 9, 4, _i32(0), -1, 0, 20, 20, PTR, 100, PTR, PTR, PTR, None), -1,
     "mxm_extend_assign: bad participating rows"),
    ("mxm_extend_assign", (_cols(), PTR, PTR, 9, 4, _i32(4), 1, 0, 20, 20, PTR, 100, PTR, PTR, PTR, None), -1,
     "mxm_extend_assign: participating row 4 is no row"),
    ("mxm_extend_assign", (_cols(), PTR, PTR, 9, 4, _i32(0), 1, -1, 20, 20, PTR, 100, PTR, PTR, PTR, None), -1,
     "mxm_extend_assign: bad shape"),
    ("mxm_extend_assign", (_cols(n_aln=3, ref_start=PTR, mapq=PTR, cig_ptr=PTR, cigar=PTR, seq_ptr=PTR, seq=PTR), None, PTR, 9, 4,
                           _i32(0), 1, 0, 20, 20, PTR, 100, PTR, PTR, PTR, None), -1,
     "mxm_extend_assign: label, joined, frag, frag_state, newvar and n_moved are required"),
]


def _row_id(row):
    return "%s-%s" % (row[0], row[3].split(": ", 1)[1][:40].replace(" ", "_"))


@pytest.mark.parametrize("name,args,code,message", TABLE, ids=[_row_id(row) for row in TABLE])
def test_refusal_code_and_message(lib, name, args, code, message):
    rc = getattr(lib, name)(*args)
    assert rc == code
    assert lib.mxm_last_error() == message.encode()


def test_table_covers_every_entry_point_that_refuses_before_the_device():
    """Every export that can fail appears, except those whose only failures come from the device or from a handle that
    has to exist first."""
    covered = {row[0] for row in TABLE}
    cannot_fail_on_the_host = {
        # sizes, queries and setters that take every value
        "mxm_version", "mxm_last_error", "mxm_linear_supported", "mxm_workspace_bytes", "mxm_restart_tile", "mxm_restart_tile_coded",
        "mxm_quad_loop_min_rows", "mxm_record_bytes", "mxm_coded_bytes", "mxm_exchange_handle_bytes", "mxm_quad_bytes",
        "mxm_quad_lists_scratch_bytes", "mxm_samples_tile_rows", "mxm_samples_workspace_bytes", "mxm_diag_fused_force_abort",
        "mxm_set_fused_coded_grid", "mxm_set_quad_left_grid", "mxm_set_sparse_long_rows", "mxm_set_sparse_long_entries",
        "mxm_set_timing_events", "mxm_set_compact_restarts", "mxm_set_loop_graph", "mxm_set_loop_fused",
        "mxm_set_progress_callback", "mxm_reset_tuning", "mxm_set_sparse_max_distinct",
        # void
        "mxm_exchange_destroy", "mxm_aln_free", "mxm_bam_free",
        # a negative row number is its only refusal, and it has no message
        "mxm_encode_signatures",
        # launches at once: its only failure is the device's
        "mxm_preload",
    }
    assert covered | cannot_fail_on_the_host == set(_lib.SIGNATURES)
    assert not covered & cannot_fail_on_the_host
