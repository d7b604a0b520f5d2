"""
mixemt's report of a run and its `-t PREFIX` tables (the reference's mixemt/stats.py), same text byte for byte:

    report_contributors(out, contribs, contrib_reads)              stats.py:48-69   the contributor table
    write_variants(out, phylo, contribs, obs_tab, args)             stats.py:96-135  PREFIX.pos.tab
    write_statistics(phylo, all_obs, contribs, contrib_reads, args) stats.py:138-171 PREFIX.pos.tab + PREFIX.obs.tab

and, opt-in, the same for ALL samples of a cohort (assign.CohortContribReads + observe.CohortPileup), the tables' text
formatted on the device (include/mixemt_hip_stats_samples.h):

    report_contributors_many(out, contribs_list, cohort, titles=None)
    write_statistics_many(phylo, pileup, contribs_list, cohort, args, prefixes)

contrib_reads is assign.assign_reads' ContribReads (one label per alignment, on the device): every contributor's table
of PREFIX.obs.tab comes out of ONE labelled pileup (observe.count_bases_labelled -> mxm_observe_bases_labelled) and is
written by io.write_base_obs.  A plain mapping name -> alignment objects (the reference's shape) is accepted too; its
alignments are turned into columns and labelled on the host first.

The reference's quirks are kept, because its files have them:
  - write_variants' threshold is max(min_var_reads, total_obs(pos) * frac_var_reads) with `pos` the LAST variant position
    of the variant loop above it, not the row's position: one threshold for every row (and UnboundLocalError when the
    contributors have no variants at all);
  - obs.tab iterates sorted(contrib_reads) as strings (hap1, hap10, hap2, ..., unassigned); a key that is no
    contributor is labelled 'unassigned'; the 'all<TAB>mix' block only follows when there is more than one key;
  - pos.tab positions are 1-based, obs.tab positions 0-based, both over range(len(phylo.refseq)).
"""

import collections
import ctypes

import numpy

from . import io as _io
from . import observe
from .phylotree import pos_from_var


def report_contributors(out, contribs, contrib_reads):
    """
    stats.report_contributors (stats.py:48-69): hap#, haplogroup, proportion and alignment count of each contributor, as
    a padded table when `out` is a TTY, tab-separated otherwise.  Looks every contributor up in contrib_reads (which,
    a defaultdict in the reference, makes it a key).
    """
    if out.isatty():
        out.write("hap#   Haplogroup      Contribution   Reads\n")
        out.write("-------------------------------------------\n")
    for hap_id, haplogroup, prop in contribs:
        total_reads = len(contrib_reads[hap_id])
        if out.isatty():
            prop_str = "%.4f" % (prop)
            read_str = "%d" % (total_reads)
            out.write("%s %s %s %s\n" % (hap_id.ljust(6), haplogroup.ljust(15), prop_str.rjust(12), read_str.rjust(7)))
        else:
            out.write("%s\t%s\t%.4f\t%d\n" % (hap_id, haplogroup, prop, total_reads))


def _acgt(obs_tab, n):
    """[n][4] int64: obs_tab.obs_at(pos)[base] for base in ACGT, both strands (from the counted table when there is one)."""
    counts = getattr(obs_tab, "counts", None)
    if counts is None:
        return numpy.array([[obs_tab.obs_at(pos)[b] for b in "ACGT"] for pos in range(n)], dtype=numpy.int64) \
            .reshape(n, 4)
    tab = numpy.zeros((n, 16), dtype=numpy.int64)
    m = min(n, counts.shape[0])
    tab[:m] = counts[:m]
    return tab[:, 0:4] + tab[:, 7:11]


def write_variants(out, phylo, contribs, obs_tab, args):
    """
    stats.write_variants (stats.py:96-135), PREFIX.pos.tab: per reference position (1-based) the sample's A C G T counts,
    'polymorphic' / 'fixed' by phylo.polymorphic_sites of the contributors, 'variant' when more than one base reaches the
    threshold ('sample_fixed' otherwise), and the contributors' variants there ('hap:var', comma-separated).
    """
    haplogroups = [con[1] for con in contribs]
    variants = collections.defaultdict(list)
    for hap in haplogroups:
        for var in phylo.hap_var[hap]:
            pos = pos_from_var(var)
            variants[pos].append("%s:%s" % (hap, var))

    polymorphic = set(phylo.polymorphic_sites(haplogroups))
    n = len(phylo.refseq)
    if n == 0:
        return
    # (the reference's threshold: `pos` is the last variant position above, for every row)
    threshold = max(args.min_var_reads, obs_tab.total_obs(pos) * args.frac_var_reads)
    acgt = _acgt(obs_tab, n)
    variant = (acgt >= threshold).sum(axis=1) > 1
    out.write("".join("%d\t%d\t%d\t%d\t%d\t%s\t%s\t%s\n"
                      % (ref_pos + 1, a, c, g, t, "polymorphic" if ref_pos in polymorphic else "fixed",
                         "variant" if var else "sample_fixed", ",".join(variants.get(ref_pos, ())))
                      for ref_pos, (a, c, g, t), var in zip(range(n), acgt.tolist(), variant.tolist())))


def _labelled_columns(contrib_reads, keys):
    """A mapping name -> alignment objects as (AlignmentColumns, int32 label per alignment: the key's index in keys)."""
    from .alignments import AlignmentColumns
    alns, label = [], []
    for k, key in enumerate(keys):
        group = list(contrib_reads[key])
        alns.extend(group)
        label.extend([k] * len(group))
    if not alns:
        return None, None
    return AlignmentColumns.from_alignments(alns), numpy.array(label, dtype=numpy.int32)


def contrib_tables(contrib_reads, keys, min_mq, min_bq, ref_len):
    """
    The pileup of each key's alignments -- ObservedBases(contrib_reads[key], min_mq, min_bq) of the reference --, every
    table from ONE mxm_observe_bases_labelled call.  Returns {key: uint32 [L][16]} with L = observe.pileup_length of the
    alignments (>= ref_len); a key without alignments (or without a label) gets zeros.
    """
    from ._dev import require_gpu, torch
    dev = require_gpu()
    if hasattr(contrib_reads, "labels"):                      # assign.ContribReads
        cols, dcols, labels = contrib_reads.cols, None, contrib_reads.labels
        names = contrib_reads.names
        index = {key: contrib_reads.label_of(key) for key in keys}
    else:
        cols, host_labels = _labelled_columns(contrib_reads, keys)
        dcols, names = None, list(keys)
        index = {key: k for k, key in enumerate(keys)}
        labels = None if cols is None else torch.from_numpy(host_labels).to(dev)
    L = ref_len if cols is None else observe.pileup_length(cols, min_mq, ref_len)
    counts = torch.zeros((max(len(names), 1), L, 16), dtype=torch.int32, device=dev)
    if cols is not None and len(cols):
        if dcols is None:
            dcols = contrib_reads.device_columns() if hasattr(contrib_reads, "device_columns") \
                else observe.DeviceColumns(cols, dev)
        observe.count_bases_labelled(dcols, labels, counts, min_mq, min_bq)
    host = counts.cpu().numpy().view(numpy.uint32)
    zeros = numpy.zeros((L, 16), dtype=numpy.uint32)
    return {key: (zeros if index[key] is None else host[index[key]]) for key in keys}


def write_statistics(phylo, all_obs, contribs, contrib_reads, args):
    """
    stats.write_statistics (stats.py:138-171): args.stats_prefix + '.pos.tab' (write_variants over all_obs) and
    '.obs.tab' (io.write_base_obs of each key of contrib_reads, in sorted order, prefixed 'hap#<TAB>haplogroup', then of
    all_obs as 'all<TAB>mix' when there is more than one key).  Reads args.min_mq / min_bq (the contributors' pileups),
    min_var_reads / frac_var_reads (write_variants).
    """
    haplogroups = {con[0]: con[1] for con in contribs}
    with open("%s.pos.tab" % (args.stats_prefix), "w") as var_out:
        write_variants(var_out, phylo, contribs, all_obs, args)
    keys = sorted(contrib_reads)
    tables = contrib_tables(contrib_reads, keys, args.min_mq, args.min_bq, len(phylo.refseq))
    with open("%s.obs.tab" % (args.stats_prefix), "w") as obs_out:
        for con in keys:
            obs_tab = observe.ObservedBases(tables[con], args.min_mq, args.min_bq)
            _io.write_base_obs(obs_out, obs_tab, phylo.refseq, "%s\t%s" % (con, haplogroups.get(con, "unassigned")))
        if len(contrib_reads) > 1:
            _io.write_base_obs(obs_out, all_obs, phylo.refseq, "all\tmix")


# ---- the -t tables of a cohort: ALL samples' files from one labelled pileup and two formatter passes on the device ----------
MAX_TEXT_BYTES = 2 << 30            # default cap for each of the two texts of a cohort (all pos.tab, all obs.tab): a cap, not
                                    # a measurement


def report_contributors_many(out, contribs_list, cohort, titles=None):
    """
    report_contributors for every sample of an assign.CohortContribReads, table after table on `out` (padded on a TTY,
    tab-separated otherwise), the alignment counts from ONE cohort.counts().  As the reference's lookup does -- and
    assemble.write_consensus_seqs_many already does --, every contributor becomes a key of cohort.keys[s]: .sample(s)
    copies its keys, so nothing else would carry them to write_statistics_many.  titles: one per sample, written as
    '# title' ahead of the sample's table.
    """
    n = cohort.n_samples
    if len(contribs_list) != n or (titles is not None and len(titles) != n):
        raise ValueError("report_contributors_many: one contributor table (and one title) per sample is needed")
    for s, contribs in enumerate(contribs_list):
        for con in contribs:
            if con[0] not in cohort.keys[s]:
                cohort.keys[s].append(con[0])
    count = cohort.counts()
    tty = out.isatty()
    for s, contribs in enumerate(contribs_list):
        if titles is not None:
            out.write("# %s\n" % (titles[s],))
        if tty:
            out.write("hap#   Haplogroup      Contribution   Reads\n")
            out.write("-------------------------------------------\n")
        for hap_id, haplogroup, prop in contribs:
            lab = cohort.label_of(s, hap_id)
            total_reads = 0 if lab is None else int(count[lab])
            if tty:
                out.write("%s %s %s %s\n" % (hap_id.ljust(6), haplogroup.ljust(15), ("%.4f" % prop).rjust(12),
                                             ("%d" % total_reads).rjust(7)))
            else:
                out.write("%s\t%s\t%.4f\t%d\n" % (hap_id, haplogroup, prop, total_reads))


def report_intervals_many(out, finished, boots, titles=None):
    """
    The bootstrap intervals of a cohort (assign.bootstrap_many's list `boots` beside finish_many's `finished`), sample
    after sample: one tab-separated line 'hapNN<TAB>haplogroup<TAB>proportion<TAB>lo<TAB>hi<TAB>sd' per contributor, the
    numbers as report_contributors writes a proportion ('%.4f'; 'nan' for a column whose replicates were not all usable).
    A sample without intervals (boots[s] is None) gets its contributors' lines with NA in the last three fields.
    titles: one per sample, written as '# title' ahead of the sample's lines.
    """
    n = len(finished)
    if len(boots) != n or (titles is not None and len(titles) != n):
        raise ValueError("report_intervals_many: one bootstrap result (and one title) per sample is needed")
    for s in range(n):
        if titles is not None:
            out.write("# %s\n" % (titles[s],))
        if boots[s] is None:
            for hap_id, haplogroup, prop in finished[s]["contribs"]:
                out.write("%s\t%s\t%.4f\tNA\tNA\tNA\n" % (hap_id, haplogroup, prop))
        else:
            for hap_id, haplogroup, prop, lo, hi, sd in boots[s]["intervals"]:
                out.write("%s\t%s\t%.4f\t%.4f\t%.4f\t%.4f\n" % (hap_id, haplogroup, prop, lo, hi, sd))


def report_support_many(out, finished, support, titles=None):
    """
    The contributor support of a cohort (assign.support_many's list `support` beside finish_many's `finished`), sample
    after sample: one tab-separated line 'hapNN<TAB>haplogroup<TAB>proportion<TAB>lrt<TAB>p' per contributor (proportion
    and lrt as '%.4f', p as '%.3g'; NA NA where the contributor has no drop-one fit -- a sample of one contributor -- or the
    sample has no support result), then 'add<TAB>haplogroup<TAB>proportion<TAB>lrt<TAB>p' per extra that was added to the
    full set, then 'best_bic<TAB>name,name,...<TAB>bic' ('%.4f') for the model with the smallest BIC.
    titles: one per sample, written as '# title' ahead of the sample's lines.
    """
    n = len(finished)
    if len(support) != n or (titles is not None and len(titles) != n):
        raise ValueError("report_support_many: one support result (and one title) per sample is needed")
    for s in range(n):
        if titles is not None:
            out.write("# %s\n" % (titles[s],))
        rows = {} if support[s] is None else {row[0]: row for row in support[s]["drop"]}
        for hap_id, haplogroup, prop in finished[s]["contribs"]:
            if hap_id in rows:
                out.write("%s\t%s\t%.4f\t%.4f\t%.3g\n" % (hap_id, haplogroup, prop, rows[hap_id][3], rows[hap_id][4]))
            else:
                out.write("%s\t%s\t%.4f\tNA\tNA\n" % (hap_id, haplogroup, prop))
        if support[s] is not None:
            for haplogroup, prop, lrt, p_value in support[s]["add"]:
                out.write("add\t%s\t%.4f\t%.4f\t%.3g\n" % (haplogroup, prop, lrt, p_value))
            best = support[s]["models"][support[s]["best_bic"]]
            out.write("best_bic\t%s\t%.4f\n" % (",".join(best["names"]), best["bic"]))


DETECTION_HEADER = ("# detection bootstrap: call frequencies under resampled reads, conditional on the OBSERVED pileup (the variant "
                    "check is not resampled) and on the EM's stop rule; not the frequencies of the full pipeline\n")


def report_detection_many(out, finished, detect, titles=None):
    """
    The detection bootstrap of a cohort (assign.detect_many's list `detect` beside finish_many's `finished`).  The first
    line says what the frequencies are conditional on; then one block per sample: '# title' (with titles), a line
    '# n_used / n_boot replicates used; variant check: ...', a table with the columns haplogroup, candidate, kept, freq
    (kept / n_used, '%.4f'; NA without a usable replicate), estimate (the point estimate's proportion, '%.4f', or '-'),
    every column right-aligned to its widest cell, then 'same_set<TAB>count', 'set_size<TAB>size<TAB>count' lines and
    'set<TAB>name,name,...<TAB>count' for the most frequent kept sets ('-' for the empty set), then
    'failed<TAB>reason<TAB>count' lines.  A skipped sample (detect[s] is None) gets '# skipped: no detection bootstrap'.
    """
    n = len(finished)
    if len(detect) != n or (titles is not None and len(titles) != n):
        raise ValueError("report_detection_many: one detection result (and one title) per sample is needed")
    out.write(DETECTION_HEADER)
    for s in range(n):
        if titles is not None:
            out.write("# %s\n" % (titles[s],))
        res = detect[s]
        if res is None:
            out.write("# skipped: no detection bootstrap\n")
            continue
        n_used = res["n_used"]
        out.write("# %d / %d replicates used; variant check: %s\n" % (n_used, res["n_boot"], res["var_check"]))
        cells = [["haplogroup", "candidate", "kept", "freq", "estimate"]]
        for name, n_cand, n_kept, _, prop in res["detection"]:
            cells.append([str(name), "%d" % n_cand, "%d" % n_kept, "%.4f" % (n_kept / float(n_used)) if n_used else "NA",
                          "-" if prop is None else "%.4f" % prop])
        widths = [max(len(row[i]) for row in cells) for i in range(5)]
        for row in cells:
            out.write("  ".join(cell.rjust(w) for cell, w in zip(row, widths)) + "\n")
        out.write("same_set\t%d\n" % res["same_set"])
        for size, count in res["set_sizes"].items():
            out.write("set_size\t%d\t%d\n" % (size, count))
        for names, count in res["sets"]:
            out.write("set\t%s\t%d\n" % (",".join(names) if names else "-", count))
        for why, count in res["n_failed"].items():
            out.write("failed\t%s\t%d\n" % (why, count))


def _stats_block_plan(contribs_list, cohort):
    """
    The obs.tab blocks of every sample, host only: per sample None (no contributors: the reference has no threshold and
    writes nothing) or its blocks in file order as (prefix bytes, table) -- the sample's keys sorted as strings, each
    prefixed 'key<TAB>haplogroup<TAB>' ('unassigned' for a key that is no contributor), then 'all<TAB>mix<TAB>' when there
    is more than one key.  table: ("label", global label), ("all", sample), or None for a key without a label (a table of
    zeros).
    """
    plan = []
    for s, contribs in enumerate(contribs_list):
        if not contribs:
            plan.append(None)
            continue
        haplogroups = {con[0]: con[1] for con in contribs}
        keys = sorted(cohort.keys[s])
        blocks = []
        for key in keys:
            lab = cohort.label_of(s, key)
            prefix = "%s\t%s\t" % (key, haplogroups.get(key, "unassigned"))
            blocks.append((prefix.encode("utf-8"), None if lab is None else ("label", lab)))
        if len(keys) > 1:
            blocks.append((b"all\tmix\t", ("all", s)))
        plan.append(blocks)
    return plan


def _stats_pos_plan(phylo, contribs, n_pos):
    """
    What write_variants derives from the contributors, host only: (polymorphic uint8 [n_pos], {pos: tail bytes} for the
    positions inside [0, n_pos), the LAST variant position of its loop -- the one its threshold is taken at -- or None
    when no contributor has a variant).
    """
    haplogroups = [con[1] for con in contribs]
    variants = collections.defaultdict(list)
    pos_last = None
    for hap in haplogroups:
        for var in phylo.hap_var[hap]:
            pos = pos_from_var(var)
            variants[pos].append("%s:%s" % (hap, var))
            pos_last = pos
    poly = numpy.zeros(n_pos, dtype=numpy.uint8)
    sites = numpy.array([p for p in phylo.polymorphic_sites(haplogroups) if 0 <= p < n_pos], dtype=numpy.int64)
    poly[sites] = 1
    tails = {pos: ",".join(names).encode("utf-8") for pos, names in variants.items() if 0 <= pos < n_pos}
    return poly, tails, pos_last


def _stats_text(lib, kind, n_pos, tables, prefixes=None, poly=None, thr=None, tail=None, tail_ptr=None):
    """An _lib.StatsText and the host arrays it points to (to be kept alive while it is used)."""
    from . import _lib
    n_blocks = len(tables)
    table_host = (ctypes.c_void_p * max(n_blocks, 1))(*tables)
    keep = [table_host]
    st = _lib.StatsText(kind, n_blocks, n_pos, ctypes.cast(table_host, ctypes.c_void_p), None, None, None, None, None, None)
    if kind == 0:
        ptr = numpy.zeros(n_blocks + 1, dtype=numpy.int64)
        numpy.cumsum([len(p) for p in prefixes], out=ptr[1:])
        raw = numpy.frombuffer(b"".join(prefixes) or b"\0", dtype=numpy.uint8)
        keep += [ptr, raw]
        st.prefix_host, st.prefix_ptr_host = raw.ctypes.data, ptr.ctypes.data
    else:
        keep += [poly, thr, tail, tail_ptr]
        st.poly, st.thr, st.tail, st.tail_ptr = poly.data_ptr(), thr.data_ptr(), tail.data_ptr(), tail_ptr.data_ptr()
    n_tiles = lib.mxm_stats_text_tiles(n_blocks, n_pos)
    if n_tiles < 0:
        raise ValueError("write_statistics_many: %d blocks of %d lines are more than the formatter's tile index holds: split "
                         "the cohort" % (n_blocks, n_pos))
    return st, keep, n_tiles


def write_statistics_many(phylo, pileup, contribs_list, cohort, args, prefixes, max_text_bytes=MAX_TEXT_BYTES, timings=None):
    """
    write_statistics for every sample of an assign.CohortContribReads: prefixes[s] + '.pos.tab' and '.obs.tab' hold byte
    for byte what write_statistics(phylo, pileup.host(s), contribs_list[s], cohort.sample(s), args) writes under that
    prefix (cohort.keys[s] being the sample's keys: report_contributors_many makes the contributors keys).  Opt-in;
    write_statistics, write_variants and io.write_base_obs are unchanged and remain the definition of the bytes.
    pileup: the observe.CohortPileup of the same samples (counts [S][L][16] on the device).  args: min_mq, min_bq,
    min_var_reads and frac_var_reads are read; stats_prefix is not.
    The reference's quirks are kept: keys sorted as strings; 'unassigned' for a key that is no contributor; 'all<TAB>mix'
    only with more than one key; pos.tab 1-based, obs.tab 0-based; ONE threshold per sample, taken at the last variant
    position of write_variants' loop (computed on the device from pileup.counts: the same two IEEE operations).
    Device steps: one labelled pileup over the cohort's global labels; two mxm_stats_text_sizes calls; ONE read-back (the
    two texts' sizes and where each block starts); two mxm_stats_text_write calls; ONE download per text into pinned host
    memory (the formatter's error word rides behind the text); every file written from its contiguous slice in binary
    mode.  Per sample the host only makes phylo.polymorphic_sites, the 'hap:var' annotations and the prefixes: nothing
    on the host runs per line.
    Raises before any file is created: ValueError for a wrong number of tables or prefixes, for a text above
    max_text_bytes (default 2 GiB for each of the two texts, a cap and not a measurement: "... split the cohort"), and for
    a sample whose contributors have no variant at all (the reference has no threshold there and fails).
    A sample without contributors gets no files and None in the returned list; the others (pos_bytes, obs_bytes).
    timings: a dict that receives the seconds of the phases (plan: the per-sample host work; pileup; tables: the blocks'
    tables, flags, annotations and thresholds made and uploaded; sizes; write; download; files); asking for it adds a
    synchronise per phase.
    """
    import time
    from . import _lib
    from ._dev import current_stream, require_gpu, torch
    from .assemble import _cohort_tables
    t0 = time.perf_counter()
    n = cohort.n_samples
    if len(contribs_list) != n or len(prefixes) != n or pileup.n_samples != n:
        raise ValueError("write_statistics_many: one pileup table, one contributor table and one prefix per sample are needed "
                         "(%d samples, %d tables, %d contributor tables, %d prefixes)"
                         % (n, pileup.n_samples, len(contribs_list), len(prefixes)))
    n_pos = len(phylo.refseq)
    if pileup.L < n_pos:
        raise ValueError("write_statistics_many: the pileup has %d positions, the reference %d" % (pileup.L, n_pos))
    plan = _stats_block_plan(contribs_list, cohort)
    with_files = [s for s in range(n) if plan[s] is not None]
    pos_plans = []
    for s in with_files:
        pos_plans.append(_stats_pos_plan(phylo, contribs_list[s], n_pos))
        if pos_plans[-1][2] is None:
            raise ValueError("write_statistics_many: sample %d: its contributors have no variant at all, so the reference has "
                             "no threshold for its pos.tab" % s)
    dev = require_gpu()
    lib = _lib.load()

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
        return time.perf_counter()

    t0 = lap("plan", t0)
    # 1. the contributors' tables: one labelled pileup over the global labels
    L, tables = _cohort_tables(cohort, args, n_pos, "write_statistics_many")
    if len(cohort.cols) and n_pos and with_files:
        observe.count_bases_labelled(cohort.device_columns(), cohort.labels, tables, args.min_mq, args.min_bq)
    counts = pileup.counts
    if counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("write_statistics_many: pileup.counts must be a contiguous int32 device tensor")
    t0 = lap("pileup", t0)
    # the blocks: obs.tab by sample and then file order, pos.tab one per sample
    obs_tables, obs_prefixes, obs_first = [], [], [0]
    for s in with_files:
        for prefix, table in plan[s]:
            obs_prefixes.append(prefix)
            obs_tables.append(None if table is None else
                              tables.data_ptr() + table[1] * L * 64 if table[0] == "label" else
                              counts.data_ptr() + table[1] * pileup.L * 64)
        obs_first.append(len(obs_tables))
    n_files = len(with_files)
    pos_tables = [counts.data_ptr() + s * pileup.L * 64 for s in with_files]
    poly = numpy.zeros((max(n_files, 1), max(n_pos, 1)), dtype=numpy.uint8)
    tail_len = numpy.zeros(n_files * n_pos + 1, dtype=numpy.int64)
    tail_bytes, last, valid = [], [], []
    for b, (poly_b, tails, pos_last) in enumerate(pos_plans):
        poly[b, :n_pos] = poly_b
        for pos in sorted(tails):
            tail_len[b * n_pos + pos + 1] = len(tails[pos])
            tail_bytes.append(tails[pos])
        valid.append(0 <= pos_last < pileup.L)
        last.append(pos_last if valid[-1] else 0)
    tail_ptr = torch.from_numpy(numpy.cumsum(tail_len)).to(dev)
    tail = torch.from_numpy(numpy.frombuffer(b"".join(tail_bytes) or b"\0", dtype=numpy.uint8).copy()).to(dev)
    poly_d = torch.from_numpy(poly).to(dev)
    # the reference's threshold, max(min_var_reads, total_obs(pos_last) * frac_var_reads), per sample on the device
    if n_files:
        rows = counts[torch.tensor(with_files, device=dev), torch.tensor(last, device=dev)].to(torch.int64) & 0xFFFFFFFF
        total = (rows[:, 0:4].sum(dim=1) + rows[:, 7:11].sum(dim=1)) * torch.tensor(valid, device=dev).to(torch.int64)
        thr = torch.maximum(torch.full((n_files,), float(args.min_var_reads), dtype=torch.float64, device=dev),
                            total.to(torch.float64) * float(args.frac_var_reads))
    else:
        thr = torch.zeros(1, dtype=torch.float64, device=dev)
    texts = [_stats_text(lib, 1, n_pos, pos_tables, poly=poly_d, thr=thr, tail=tail, tail_ptr=tail_ptr),
             _stats_text(lib, 0, n_pos, obs_tables, prefixes=obs_prefixes)]
    t0 = lap("tables", t0)
    # 2. the sizes; 3. ONE read-back: where each block starts in its text, and the texts' sizes
    tpb = (n_pos + 255) // 256
    offs, starts = [], []
    for st, _, n_tiles in texts:
        off = torch.empty(n_tiles + 1, dtype=torch.int64, device=dev)
        _lib.check(lib.mxm_stats_text_sizes(ctypes.byref(st), off.data_ptr(), current_stream()), "mxm_stats_text_sizes")
        offs.append(off)
        starts.append(off[::tpb] if n_tiles else off.new_zeros(st.n_blocks + 1))
    got = torch.cat(starts).cpu().numpy()
    start = [got[:n_files + 1], got[n_files + 1:]]
    t0 = lap("sizes", t0)
    for k, what in enumerate(("pos.tab", "obs.tab")):
        if int(start[k][-1]) > int(max_text_bytes):
            raise ValueError("write_statistics_many: the %s text of %d samples takes %d bytes, above the cap of %d bytes "
                             "(max_text_bytes): split the cohort" % (what, n_files, int(start[k][-1]), int(max_text_bytes)))
    # 4. the texts, each with the formatter's error word behind it
    outs = []
    for k, (st, _, _) in enumerate(texts):
        size = int(start[k][-1])
        pad = (size + 3) // 4 * 4
        out = torch.empty(pad + 4, dtype=torch.uint8, device=dev)
        out[pad:].zero_()
        _lib.check(lib.mxm_stats_text_write(ctypes.byref(st), offs[k].data_ptr(), out.data_ptr(), size, out.data_ptr() + pad,
                                            current_stream()), "mxm_stats_text_write")
        outs.append((out, size, pad))
    t0 = lap("write", t0)
    # 5. ONE download per text into pinned memory
    hosts = []
    for out, size, pad in outs:
        host = torch.empty(pad + 4, dtype=torch.uint8, pin_memory=True)
        host.copy_(out, non_blocking=True)
        hosts.append(host)
    torch.cuda.current_stream().synchronize()
    t0 = lap("download", t0)
    for k, (out, size, pad) in enumerate(outs):
        if int(hosts[k][pad:].view(torch.int32)[0]) != 0:
            raise RuntimeError("write_statistics_many: the formatter skipped a tile of the %s text (sizes and text disagree)"
                               % ("pos.tab", "obs.tab")[k])
    # 6. the files: each one slice of its text
    result = [None] * n
    pos_text, obs_text = hosts[0].numpy(), hosts[1].numpy()
    for b, s in enumerate(with_files):
        lo, hi = int(start[0][b]), int(start[0][b + 1])
        with open("%s.pos.tab" % (prefixes[s]), "wb") as fout:
            fout.write(pos_text[lo:hi])
        olo, ohi = int(start[1][obs_first[b]]), int(start[1][obs_first[b + 1]])
        with open("%s.obs.tab" % (prefixes[s]), "wb") as fout:
            fout.write(obs_text[olo:ohi])
        result[s] = (hi - lo, ohi - olo)
    lap("files", t0)
    return result
