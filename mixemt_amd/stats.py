"""
mixemt's report of a run and its `-t PREFIX` tables (the reference's mixemt/stats.py), same text byte for byte:

    report_contributors(out, contribs, contrib_reads)              stats.py:48-69   the contributor table
    write_variants(out, phylo, contribs, obs_tab, args)             stats.py:96-135  PREFIX.pos.tab
    write_statistics(phylo, all_obs, contribs, contrib_reads, args) stats.py:138-171 PREFIX.pos.tab + PREFIX.obs.tab

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
