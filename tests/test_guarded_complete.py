"""
Every entry of the C ABI is either called by a guarded test (tests/test_gpu_guarded_*.py on the device,
tests/test_guarded_host.py on the host: every buffer at its exact documented size between red zones, tests/_guarded.py) or
listed below with the reason why it needs none.  A new entry in one of the headers fails this test until it is guarded
or excused.  No GPU.
"""
import glob
import os
import re

from conftest import ROOT

HEADERS = ["mixemt_hip.h", "mixemt_hip_samples_finish.h", "mixemt_hip_var_check.h", "mixemt_hip_tuning.h"]

HOST_GETTER = "pure host getter or size function: no caller-sized buffer"
SETTER = "tuning setter / reset: takes values, no buffer"
DIAG = "mxm_diag_*: measurement hooks outside the boundary"
FREES = "releases a handle"
OWNS = "owns the memory it fills; the caller sizes nothing"
EXCHANGE = "mxm_exchange_*: the IPC-mapped buffers are the library's own"

EXCLUDED = {
    "mxm_version": HOST_GETTER, "mxm_last_error": HOST_GETTER, "mxm_linear_supported": HOST_GETTER,
    "mxm_restart_tile": HOST_GETTER, "mxm_restart_tile_coded": HOST_GETTER, "mxm_quad_loop_min_rows": HOST_GETTER,
    "mxm_workspace_bytes": HOST_GETTER, "mxm_record_bytes": HOST_GETTER, "mxm_coded_bytes": HOST_GETTER,
    "mxm_quad_bytes": HOST_GETTER, "mxm_quad_lists_scratch_bytes": HOST_GETTER, "mxm_samples_workspace_bytes": HOST_GETTER,
    "mxm_samples_finish_workspace_bytes": HOST_GETTER, "mxm_samples_tile_rows": HOST_GETTER,
    "mxm_describe_stream_kernel": HOST_GETTER + " beyond the text buffer whose length it is told",
    "mxm_preload": HOST_GETTER + " (loads the code object; takes no argument)",
    "mxm_reset_tuning": SETTER, "mxm_set_loop_graph": SETTER, "mxm_set_loop_fused": SETTER, "mxm_set_fused_coded_grid": SETTER,
    "mxm_set_quad_left_grid": SETTER, "mxm_set_sparse_long_rows": SETTER, "mxm_set_sparse_long_entries": SETTER,
    "mxm_set_quad_encoder": SETTER, "mxm_set_coded_batch_tile": SETTER, "mxm_set_batch_tile": SETTER,
    "mxm_set_compact_restarts": SETTER, "mxm_set_min_rows_per_wg": SETTER, "mxm_set_sparse_max_distinct": SETTER,
    "mxm_set_progress_callback": "host callback hook: no buffer", "mxm_set_timing_events": "event handles: no buffer",
    "mxm_diag_stream_read": DIAG, "mxm_diag_stream_coded": DIAG, "mxm_diag_stream_quads": DIAG,
    "mxm_diag_fused_force_abort": DIAG, "mxm_diag_fused_stamps": DIAG,
    "mxm_aln_free": FREES, "mxm_bam_free": FREES, "mxm_exchange_destroy": FREES,
    "mxm_bam_read": OWNS, "mxm_bam_sizes_of": OWNS, "mxm_bam_columns": OWNS, "mxm_aln_encode": OWNS, "mxm_aln_sizes_of": OWNS,
    "mxm_exchange_handle_bytes": EXCHANGE, "mxm_exchange_create": EXCHANGE, "mxm_exchange_connect": EXCHANGE,
    "mxm_exchange_push": EXCHANGE, "mxm_exchange_pull": EXCHANGE, "mxm_exchange_reduce": EXCHANGE, "mxm_exchange_info": EXCHANGE,
}

# an excluded name may still be CALLED by a guarded test (a size function is how the exact size is asked for): what counts
# for the others is a call through the library handle with buffers the test sized itself
CALL = re.compile(r"\blib\.(mxm_\w+)\s*\(")
ALIAS = re.compile(r"\blib\.(mxm_\w+)\b(?!\s*\()")         # `entry = lib.mxm_linearize if ... else lib.mxm_linearize_f32`


def declared_entries():
    names = set()
    for header in HEADERS:
        with open(os.path.join(ROOT, "include", header)) as fin:
            text = fin.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
        for decl in text.split(";"):
            # a declaration `type mxm_name(arguments)`: the first mxm_ name directly followed by its parameter list
            found = re.search(r"\b(mxm_\w+)\s*\(", decl)
            if found and "typedef" not in decl.split(found.group(1))[0]:
                names.add(found.group(1))
    return names


def guarded_calls():
    names = set()
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_guarded_*.py"))) + [
        os.path.join(ROOT, "tests", "test_guarded_host.py"), os.path.join(ROOT, "tests", "_guarded_abi.py")]
    for path in paths:
        with open(path) as fin:
            text = fin.read()
        names.update(CALL.findall(text))
        names.update(ALIAS.findall(text))
    return names


def test_the_parser_sees_the_abi():
    names = declared_entries()
    assert len(names) > 90
    for known in ("mxm_em_iter", "mxm_check_variants_samples", "mxm_votes_samples", "mxm_set_progress_callback", "mxm_bam_free",
                  "mxm_last_error", "mxm_exchange_reduce", "mxm_samples_plan", "mxm_diag_fused_stamps"):
        assert known in names, known
    for no_entry in ("mxm_em_state", "mxm_coded", "mxm_aln_columns", "mxm_sample_tile", "mxm_bam", "mxm_exchange"):
        assert no_entry not in names, no_entry
    # the binding lists the same symbols: a header the parser missed would show here
    from mixemt_amd import _lib
    bound = set(_lib.SIGNATURES) | set(_lib.FINISH_SIGNATURES) | set(_lib.VARCHECK_SIGNATURES)
    assert names == bound, (sorted(names - bound), sorted(bound - names))


def test_every_entry_is_guarded_or_excused():
    names = declared_entries()
    guarded = guarded_calls()
    assert not (set(EXCLUDED) - names), "excused names that are no entry: %r" % sorted(set(EXCLUDED) - names)
    missing = sorted(n for n in names if n not in guarded and n not in EXCLUDED)
    assert not missing, "entries neither called by a guarded test nor excused: %r" % missing
    # an excuse is for entries without a caller-sized buffer only: nothing that a guarded module covers hides behind one
    assert all(EXCLUDED[n] for n in EXCLUDED)
    for name in names - set(EXCLUDED):
        assert name in guarded, name
