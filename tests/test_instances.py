"""
The instance table (tests/_instances.py) against the host source it restates -- CPU only, nothing is launched:
  * every dispatch_width call of mixemt_hip.hip belongs to a site of the table, and every site to a call;
  * per site the classes partition the widths the entry takes with no gap and no overlap, one class per instance;
  * the number of instances is the dispatch's own MAX, or the named constant / narrowing the site states;
  * mxm_describe_stream_kernel names the instance the table predicts at every edge width, for tiles of 1 .. 4 restarts.
"""
import ctypes
import re

import pytest

import _instances as inst


def test_every_dispatch_site_is_in_the_table():
    found = inst.dispatch_sites()
    assert len(found) == len(set((f, n) for f, n, _ in found))
    wheres = set(site.where for site in inst.SITES.values())
    missing = [(f, n) for f, n, _ in found if (f, n) not in wheres]
    assert not missing, "dispatch_width sites without a row in tests/_instances.py: %s" % missing
    gone = sorted(wheres - set((f, n) for f, n, _ in found))
    assert not gone, "rows of tests/_instances.py whose dispatch_width call is gone: %s" % gone


@pytest.mark.parametrize("name", list(inst.SITES))
def test_classes_partition_the_supported_widths(name):
    site = inst.SITES[name]
    cls = inst.classes(name)
    supported = [h for h in range(site.lo, site.hi + 1) if site.supported(h)]
    assert supported and not site.supported(site.lo - 1) and not site.supported(site.hi + 1)
    # no overlap, no gap: the classes' widths, concatenated, are the supported widths in order
    covered = [h for c in cls for h in range(c.first, c.last + 1) if site.supported(h)]
    assert covered == supported
    assert all(a.last < b.first for a, b in zip(cls, cls[1:]))
    # one class per instance, instances ascending from the first; both edges map to the class's instance
    assert [c.instance for c in cls] == sorted(set(c.instance for c in cls))
    for c in cls:
        assert site.instance(c.first) == site.instance(c.last) == c.instance
        assert all(site.instance(h) == c.instance for h in range(c.first, c.last + 1) if site.supported(h))
    if site.by_width:
        assert [c.instance for c in cls] == list(range(site.first, site.first + len(cls))), name
    # the rows of the sweep: every row count occurs where the site has three instances or more
    if site.by_width and len(cls) >= 3:
        assert set(inst.rows_for(c.instance) for c in cls) == {3, 37, 64}


@pytest.mark.parametrize("name", list(inst.SITES))
def test_instance_count_is_the_maximum_the_source_names(name):
    site = inst.SITES[name]
    written = {(f, n): m for f, n, m in inst.dispatch_sites()}[site.where]
    if written == "MAX_RPT":                             # (the columns-split loop dispatches on RPT inside a lambda per CP)
        hit = re.search(r"if \(cp <= (\d+)\) columns\(.*?\n\s*else if \(cp <= (\d+)\) columns\(.*?\n\s*else columns\(std::integral_constant<int, (\d+)>",
                        inst.source())
        assert hit and [int(g) for g in hit.groups()] == [12, 22, inst.const("FCOLS_MAX_CP")]
        assert len(inst.classes(name)) == site.count == 3
        return
    compiled = int(written) if written.isdigit() else inst.const(written)
    n_classes = len(inst.classes(name))
    assert n_classes == site.count, (name, n_classes, site.count)
    if site.count_from == "MAX":
        assert site.count == compiled, (name, site.count, compiled)
    else:
        assert site.count <= compiled, (name, site.count, compiled, site.count_from)


def test_named_narrowings_are_what_the_source_says():
    """The constants behind every count that is not the dispatch's MAX."""
    src = inst.source()
    assert inst.SITES["quad"].count == inst.SITES["quad_coded"].count == inst.const("QUAD_MAX_NCH")
    assert inst.SITES["fused_rows"].count == inst.const("FUSED_MAX_NCH")
    assert (inst.SITES["em_step_colsum"].count, inst.SITES["em_step"].count) == inst.estep_wide_caps()
    assert [inst.SITES["em_iter_b%d" % nb].count for nb in (2, 3, 4)] == inst.max_nch_list()[2:]
    assert re.search(r"if constexpr \(NCH \* THREADS > MXM_MAX_COL2\)", src)
    assert re.search(r"if constexpr \(NCH \* MXM_F32_THREADS > 2048\)", src)
    assert re.search(r"if constexpr \(NCH \* THREADS <= 2048\)", src)
    assert re.search(r"if constexpr \(NCH \* FCODED_THREADS > 2048\)", src)
    assert re.search(r"const int nch = \(\(ldc / 4 \+ QUAD_THREADS - 1\) / QUAD_THREADS \+ 1\) / 2;", src)
    assert re.search(r"const int nch_a = \(ldc_a / 4 \+ 255\) / 256;", src)
    assert len(re.findall(r"const int nch = \(H / 2 \+ 255\) / 256;", src)) == 3       # linearize_wide, mxm_em_step, mxm_row_argmax_votes
    assert re.search(r"const int nt = \(H \+ LUT_THREADS \* LUT_CPL - 1\) / \(LUT_THREADS \* LUT_CPL\);", src)
    assert re.search(r"const int nch = \(hpad / 2 \+ SPB_THREADS - 1\) / SPB_THREADS;", src)
    assert re.search(r"const int nch = \(\(H \+ 3\) / 4 \+ MXM_F32_THREADS - 1\) / MXM_F32_THREADS;", src)
    assert re.search(r"const int nch = \(ldc / 4 \+ ENC_THREADS - 1\) / ENC_THREADS;", src)
    assert re.search(r"const int nch = \(ldc / 4 \+ SAMPLES_THREADS - 1\) / SAMPLES_THREADS;", src)
    assert re.search(r"const int cnch = \(ldc / 4 \+ FCODED_THREADS - 1\) / FCODED_THREADS;", src)
    assert re.search(r"const int nch = \(\(H \+ 1\) / 2 \+ FUSED_THREADS - 1\) / FUSED_THREADS;", src)


@pytest.fixture(scope="module")
def lib():
    from mixemt_amd import _lib, build
    build.build()
    return _lib.load()


def test_describe_stream_kernel_names_the_predicted_instance(lib):
    """Launches nothing: the name is formed on the host from the same arithmetic stream_linear_tile uses."""
    buf = ctypes.create_string_buffer(128)
    seen = set()
    for nb in (1, 2, 3, 4):
        for instance, n_haps in inst.edge_cases("em_iter_b%d" % nb):
            assert lib.mxm_describe_stream_kernel(n_haps, nb, buf, len(buf)) == 0
            name = buf.value.decode()
            assert name == inst.stream_kernel_name(n_haps, nb), (n_haps, nb)
            assert re.match(r"em_iter_wide_kernel<\d+, %d, %d, \d+, \d+>$" % (instance, nb), name), (name, instance)
            seen.add(name)
    assert len(seen) == sum(inst.SITES["em_iter_b%d" % nb].count for nb in (1, 2, 3, 4))
