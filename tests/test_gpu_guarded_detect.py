"""
The entries of include/mixemt_hip_detect.h called through ctypes with every buffer guard-banded at its exact documented size
(tests/_guarded.py): mxm_detect_candidates (votes, first, props [E][H], state [E], cand / cprop [E][ld], ncand [E]; rows_host
[E] guarded ON THE HOST) and mxm_check_variants_entries (counts [T][L][16] at the 16 bytes the entry asks for, the tree's
tables, cand [E][ld], ncand [E], keep / n_uniq / n_found [E][ld], flag [E]; table_of_host [E] guarded on the host).  H = 66 and
5408, every ld; entries past a list's end and the rows of refused entries must keep their sentinel.  Values are compared with
tests/_detect_ref.py and with the host check of tests/test_gpu_var_check.py, not only the guards.
"""
import numpy
import pytest

import _detect_ref as ref
from _guarded import guarded, guarded_from
from _guarded_abi import DEV, check_all, is_sentinel, load_lib, stream, sync
from test_gpu_detect import entries_for
from test_gpu_var_check import TOY, host_check, table
from test_observe import asm_args
from test_var_check_host import toy_tree

pytestmark = pytest.mark.gpu

F8, I8, I4 = numpy.float64, numpy.int64, numpy.int32
A, C, G, T = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    return load_lib()


@pytest.mark.parametrize("ld", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("n_haps", [66, 5408])
def test_candidates(lib, n_haps, ld):
    """mixemt_hip_detect.h: "votes [E][H] double, first [E][H] int64", "rows_host [E] int64 HOST", "props [E][H] double", "state
    [E]", "cand [E][ld] int32, ncand [E] int32, cprop [E][ld] double"; "slots at and past ncand[e] are not written"."""
    from mixemt_amd import _lib
    kinds, entries = entries_for(n_haps, ld, 31 * ld + n_haps)
    n = len(entries)
    state = (_lib.EmState * n)()
    for i, e in enumerate(entries):
        state[i].done, state[i].error = e[4]
    rows = numpy.array([e[2] for e in entries], dtype=I8)
    rows_host = guarded_from(rows, I8, 8, None)
    run = {"votes": guarded_from(numpy.stack([e[0] for e in entries]), F8, 8, DEV),
           "first": guarded_from(numpy.stack([e[1] for e in entries]), I8, 8, DEV),
           "props": guarded_from(numpy.stack([e[3] for e in entries]), F8, 8, DEV),
           "state": guarded_from(numpy.frombuffer(bytes(state), dtype=numpy.uint8), numpy.uint8, 8, DEV),
           "cand": guarded(4 * n * ld, 4, DEV), "ncand": guarded(4 * n, 4, DEV), "cprop": guarded(8 * n * ld, 8, DEV),
           "rows_host": rows_host}
    what = "H=%d ld=%d" % (n_haps, ld)
    assert lib.mxm_detect_candidates(run["votes"].ptr, run["first"].ptr, rows_host.ptr, run["props"].ptr, run["state"].ptr, n, n_haps,
                                     3.0, ld, run["cand"].ptr, run["ncand"].ptr, run["cprop"].ptr, stream()) == 0, lib.mxm_last_error()
    sync()
    check_all(run, what)
    assert numpy.array_equal(rows_host.get(I8), rows)
    for key, i in (("votes", 0), ("first", 1), ("props", 3)):                   # inputs are inputs
        assert run[key].get(entries[0][i].dtype).tobytes() == numpy.stack([e[i] for e in entries]).tobytes(), key
    ncand, cand, cprop = run["ncand"].get(I4), run["cand"].get(I4, (n, ld)), run["cprop"].get(F8, (n, ld))
    for i, (votes, first, n_rows, props, st) in enumerate(entries):
        want_n, want_c, want_p = ref.candidates(votes, first, n_rows, props, 3.0, ld, st)
        assert ncand[i] == want_n, (what, kinds[i])
        if 0 <= want_n <= ld:
            assert cand[i, :want_n].tolist() == want_c and cprop[i, :want_n].tobytes() == numpy.array(want_p, dtype=F8).tobytes(), (what, kinds[i])
            assert is_sentinel(cand[i, want_n:]) and is_sentinel(cprop[i, want_n:]), (what, kinds[i])
        elif want_n < 0:
            assert is_sentinel(cand[i]) and is_sentinel(cprop[i]), "a refused entry's row was written (%s, %s)" % (what, kinds[i])


@pytest.mark.parametrize("ld", [4, 8, 16, 32, 64])
@pytest.mark.parametrize("L", [9, 64])
def test_check_entries(lib, L, ld):
    """"counts [T][L][16] (device, 16-byte aligned)", "table_of_host [E] int32 HOST", "cand [E][ld], ncand [E] device int32", "keep
    [E][ld] uint8, n_uniq / n_found [E][ld] int32 (both nullable), flag [E] int32"; "An entry flagged 1 or 2 is left alone"."""
    from mixemt_amd import assign
    phy = toy_tree()
    tab = assign.VarCheckTables.build(phy, TOY)                                  # (host arrays: the device copies are guarded here)
    index = {h: i for i, h in enumerate(TOY)}
    args = asm_args()
    tables = numpy.stack([table(L, {(0, G): 5, (1, T): 5}), table(L, {(0, G): 5, (2, T): 5, (4, T): 5}), table(L, {(0, G): 9})])
    lists = [["I", "A", "H", "F"][:min(ld, 4)], ["H", "I"], [], ["H"], ["I", "A"], ["F", "I", "A"]]
    table_of = numpy.array([0, 1, 2, 1, 0, 0], dtype=I4)
    n = len(lists)
    cand = numpy.frombuffer(b"\xff" * (4 * n * ld), dtype=I4).reshape(n, ld).copy()      # past a list's end: -1, never read
    for e, names in enumerate(lists):
        cand[e, :len(names)] = [index[x] for x in names]
    ncand = numpy.array([len(x) for x in lists], dtype=I4)
    ncand[4] = -1                                                                # flag 1: left alone
    cand[5, 1] = len(TOY)                                                        # flag 2: left alone
    table_host = guarded_from(table_of, I4, 4, None)
    run = {"counts": guarded_from(tables, I4, 16, DEV), "key_ptr": guarded_from(tab.key_ptr_h, I4, 4, DEV),
           "key": guarded_from(tab.key_h, I4, 4, DEV), "site": guarded_from(tab.site_h, I4, 4, DEV),
           "site_key": guarded_from(tab.site_key_h, I4, 4, DEV), "cand": guarded_from(cand, I4, 4, DEV),
           "ncand": guarded_from(ncand, I4, 4, DEV), "keep": guarded(n * ld, 1, DEV), "n_uniq": guarded(4 * n * ld, 4, DEV),
           "n_found": guarded(4 * n * ld, 4, DEV), "flag": guarded(4 * n, 4, DEV), "table_of_host": table_host}
    what = "L=%d ld=%d" % (L, ld)
    for with_counts in (True, False):
        assert lib.mxm_check_variants_entries(run["counts"].ptr, 3, L, run["key_ptr"].ptr, run["key"].ptr, len(TOY), run["site"].ptr,
                                              run["site_key"].ptr, len(tab.site_h), tab.max_pos, table_host.ptr, n, run["cand"].ptr,
                                              run["ncand"].ptr, ld, float(args.min_var_reads), float(args.frac_var_reads),
                                              float(args.var_fraction), 0, 0, run["keep"].ptr,
                                              run["n_uniq"].ptr if with_counts else None, run["n_found"].ptr if with_counts else None,
                                              run["flag"].ptr, stream()) == 0, lib.mxm_last_error()
        sync()
        check_all(run, what)
        assert numpy.array_equal(table_host.get(I4), table_of)
        assert numpy.array_equal(run["cand"].get(I4, (n, ld)), cand) and numpy.array_equal(run["ncand"].get(I4), ncand)
        keep, uniq, found = run["keep"].get(numpy.uint8, (n, ld)), run["n_uniq"].get(I4, (n, ld)), run["n_found"].get(I4, (n, ld))
        assert run["flag"].get(I4).tolist() == [0, 0, 0, 0, 1, 2], what
        for e, names in enumerate(lists):
            if e >= 4:
                assert is_sentinel(keep[e]) and is_sentinel(uniq[e]) and is_sentinel(found[e]), "a flagged entry was written (%s, %d)" % (what, e)
                continue
            want = host_check(phy, tables[table_of[e]], names, args)
            k = len(names)
            assert [(bool(keep[e, i]), int(uniq[e, i]), int(found[e, i])) for i in range(k)] == want, (what, e)
            assert is_sentinel(keep[e, k:]) and is_sentinel(uniq[e, k:]) and is_sentinel(found[e, k:]), (what, e)
