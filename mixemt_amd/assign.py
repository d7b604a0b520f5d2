"""
Consumers of the EM result that reduce the [R][H] posterior matrix to one small
value per read -- the "next" rows f-1..f-3 of SURVEY.md section 8.  On the
device they are single streaming / gather passes over a matrix that is already
resident, and they remove the 43 GB device->host copy of `read_mix` the
reference's NumPy versions would need:

    find_contribs_from_reads   <- assemble._find_contribs_from_reads  assemble.py:103-123
    get_contributors (+ _records) <- assemble.get_contributors        assemble.py:31-100
    check_contrib_phy_vars     <- assemble._check_contrib_phy_vars    assemble.py:126-208 (host logic over the pileup of
                                  observe.observe_bases)
    check_variants_samples     <- the same for the samples of a cohort in one launch, over pileups on the device
                                  (VarCheckTables: the tree's variants as arrays; finish_many(obs=CohortPileup))
    read_votes / report_read_votes <- stats.report_read_votes          stats.py:34-45
    update_contribs            <- assemble.update_contribs             assemble.py:211-230
    assign_read_indexes        <- assemble.assign_read_indexes         assemble.py:284-334
                                  (with _find_best_n_for_read :267-281)
    assign_reads (ContribReads) <- assemble.assign_reads               assemble.py:233-264 (one label per alignment)
                                  (consensus and extension over the labels: mixemt_amd/assemble.py)

Matrices may be numpy arrays (uploaded) or ROCm tensors.
"""

import collections
import collections.abc
import sys

import numpy

from . import _lib
from ._dev import as_device, current_stream, ptr, require_gpu, torch


def _contributors_on_device(best_d, votes_d, n_haps, min_reads):
    """
    Columns with at least min_reads votes in the order their haplogroup first won a row (assemble.py:115-123): the
    first-seen row of every haplogroup is formed on the device (mxm_first_seen), so 2 x H values come back instead of
    best[R] (4 MB and a numpy.unique over R at 10^6 rows: 23 ms for a 1.5 ms pass).
    """
    lib = _lib.load()
    n_rows = best_d.numel()
    first = torch.empty(n_haps, dtype=torch.int64, device=best_d.device)
    _lib.check(lib.mxm_first_seen(best_d.data_ptr(), n_rows, n_haps, first.data_ptr(), current_stream()), "mxm_first_seen")
    first_h, votes_h = first.cpu().numpy(), votes_d.cpu().numpy()
    seen = numpy.flatnonzero(first_h < n_rows)
    order = seen[numpy.argsort(first_h[seen], kind="stable")]
    return [int(h) for h in order if votes_h[h] >= min_reads], order, votes_h


def _row_argmax_votes_device(read_hap_mat, wts):
    lib = _lib.load()
    dev = require_gpu()
    mat = as_device(read_hap_mat, torch.float64, dev)
    n_rows, n_haps = mat.shape
    w_d = None if wts is None else as_device(wts, torch.float64, dev)
    best = torch.empty(n_rows, dtype=torch.int32, device=dev)
    votes = torch.zeros(n_haps, dtype=torch.float64, device=dev)
    if n_rows:
        nbytes = lib.mxm_workspace_bytes(n_rows, n_haps, 1)       # per-workgroup vote rows (no float atomics)
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
        _lib.check(lib.mxm_row_argmax_votes(mat.data_ptr(), mat.stride(0), ptr(w_d), n_rows, n_haps,
                                            best.data_ptr(), votes.data_ptr(), ws.data_ptr(), nbytes,
                                            current_stream()), "mxm_row_argmax_votes")
    return best, votes


def row_argmax_votes(read_hap_mat, wts=None):
    """
    best[r] = first index of the row maximum (numpy.argmax semantics) and
    votes[h] = sum of wts over the rows that picked h (mxm_row_argmax_votes).
    Returns (best int32[R], votes float64[H]) as numpy arrays.
    """
    best, votes = _row_argmax_votes_device(read_hap_mat, wts)
    return best.cpu().numpy(), votes.cpu().numpy()


def row_argmax_votes_records(cm, ln_theta_k, wts=None):
    """
    row_argmax_votes of run_em's returned posterior for a matrix that exists only as records
    (preprocess.CodedMatrix) -- neither the dense matrix nor the posterior matrix is made
    (mxm_row_argmax_votes_coded).  ln_theta_k: the log theta_k of the run ([H]) or of every run of a multi-run
    ([n_multi][H], em.run_em_ex's "ln_theta_k"): the reference votes on the logaddexp fold of the runs' posteriors
    (em.py:156 -> assemble.py:115-123), in which each run's row normaliser weighs that run's columns -- with one
    run it drops out and best = argmax_h (ln_theta[h] + M[r][h]).  Rows without a record are read from their
    dense copies by the same entry point; votes are summed without float atomics.
    Returns (best int32[R], votes float64[H]) as numpy arrays.
    """
    best, votes = _row_argmax_votes_records_device(cm, ln_theta_k, wts)
    return best.cpu().numpy(), votes.cpu().numpy()


def _row_argmax_votes_records_device(cm, ln_theta_k, wts=None):
    import ctypes
    lib = _lib.load()
    dev = cm.rec.device
    if isinstance(ln_theta_k, torch.Tensor):
        lnp = as_device(ln_theta_k, torch.float64, dev)
        lnp = (lnp.reshape(1, -1) if lnp.dim() == 1 else lnp).contiguous()
        props = torch.exp(lnp)
    else:
        # H values per run: exponentiated on the host (the process's first torch.exp on the device loads torch's
        # elementwise kernels -- 18 ms that landed in this 3 ms stage)
        host = numpy.atleast_2d(numpy.ascontiguousarray(ln_theta_k, dtype=numpy.float64))
        lnp = torch.from_numpy(host).to(dev)
        props = torch.from_numpy(numpy.exp(host)).to(dev)
    n_runs = lnp.shape[0]
    if lnp.dim() != 2 or lnp.shape[1] != cm.n_haps:
        raise ValueError("ln_theta_k does not match the matrix width")
    best = torch.zeros(cm.n_rows, dtype=torch.int32, device=dev)
    votes = torch.zeros(cm.n_haps, dtype=torch.float64, device=dev)
    w_d = None if wts is None else as_device(wts, torch.float64, dev)
    nbytes = lib.mxm_workspace_bytes(cm.n_rows, cm.n_haps, 1)
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)
    coded = cm.struct()
    n_rest = int(cm.rest_rows.numel())
    _lib.check(lib.mxm_row_argmax_votes_coded(
        ctypes.byref(coded), cm.n_haps, n_runs, lnp.data_ptr(), props.data_ptr(), cm.rowmax.data_ptr(),
        cm.m_rest.data_ptr() if n_rest else 0, cm.m_rest.stride(0) if n_rest else 0,
        cm.rest_rows.data_ptr() if n_rest else 0, n_rest, ptr(w_d), best.data_ptr(), votes.data_ptr(),
        ws.data_ptr(), nbytes, current_stream()), "mxm_row_argmax_votes_coded")
    return best, votes


def find_contribs_from_records(cm, ln_theta_k, wts, args):
    """find_contribs_from_reads (assemble.py:103-123) from records and the EM's log theta_k ([H], or [n_multi][H]
    for a multi-run: see row_argmax_votes_records)."""
    best, votes = _row_argmax_votes_records_device(cm, ln_theta_k, wts)
    return _contributors_on_device(best, votes, cm.n_haps, args.min_reads)[0]


def vote_table_from_records(cm, ln_theta_k, wts=None):
    """(columns in first-seen order, votes[H]) of the records' vote (stats.py:34-45 / assemble.py:115-123); H-sized
    arrays only leave the device."""
    best, votes = _row_argmax_votes_records_device(cm, ln_theta_k, wts)
    _, order, votes_h = _contributors_on_device(best, votes, cm.n_haps, 0)
    return order, votes_h


def _first_seen_order(best):
    """Column indexes in the order they first appear in `best` (dict insertion order
    of the reference's vote table, assemble.py:116-119)."""
    uniq, first = numpy.unique(best, return_index=True)
    return uniq[numpy.argsort(first, kind="stable")]


def find_contribs_from_reads(read_hap_mat, wts, args):
    """
    Haplogroup columns that are the most probable source of at least
    args.min_reads fragments (assemble.py:103-123), in the reference's order
    (first appearance among the rows).
    """
    best, votes = _row_argmax_votes_device(read_hap_mat, wts)
    return _contributors_on_device(best, votes, votes.numel(), args.min_reads)[0]


def check_contrib_phy_vars(phylo, obs, contrib_prop, args):
    """
    assemble._check_contrib_phy_vars (assemble.py:126-208): from the largest proportion down, a candidate is kept when
    enough of its variants that no kept candidate has already claimed are seen in the sample -- a (pos, derived base)
    is seen when obs.obs_at(pos, der) >= max(args.min_var_reads, obs.total_obs(pos) * args.frac_var_reads); kept when
    it has no such variants, or args.var_count is set and met, or the seen fraction is >= args.var_fraction.  A kept
    candidate's seen variants and its ancestral bases (phylo.get_ancestral) are claimed.  `obs`: an
    observe.ObservedBases (or the reference's).  contrib_prop: [[haplogroup, proportion], ...] by descending proportion.
    Verbose lines go to stderr, as the reference writes them.
    """
    from .phylotree import der_allele, pos_from_var
    used_vars = set()
    ignore_haps = set()
    threshold = 0                                  # (the reference's "Keeping" line prints the last site's threshold)
    if args.verbose:
        sys.stderr.write("Checking diagnostic variants:\n")
    for hap, _ in contrib_prop:
        uniq_vars = set((pos_from_var(var), der_allele(var)) for var in phylo.hap_var[hap])
        uniq_vars -= used_vars
        if args.verbose:
            sys.stderr.write("%s (%d unique variants)\n" % (hap, len(uniq_vars)))
        found_vars = set()
        for pos, der in sorted(uniq_vars):
            seen, total = obs.obs_at(pos, der), obs.total_obs(pos)
            if args.verbose:
                var = "%d%s" % (pos + 1, der)
                sys.stderr.write("  %s: %d/%d\n" % (var.rjust(6), seen, total))
            threshold = max(args.min_var_reads, total * args.frac_var_reads)
            if seen >= threshold:
                found_vars.add((pos, der))
        if (len(uniq_vars) == 0
                or (args.var_count is not None and len(found_vars) >= args.var_count)
                or (float(len(found_vars)) / len(uniq_vars) >= args.var_fraction)):
            if args.verbose:
                sys.stderr.write("Keeping '%s': %d/%d unique variant bases observed at least %d times.\n"
                                 % (hap, len(found_vars), len(uniq_vars), threshold))
            used_vars.update(found_vars)
            used_vars.update(phylo.get_ancestral(hap))
        else:
            if args.verbose:
                sys.stderr.write("Ignoring '%s': only %d/%d unique variant bases observed.\n"
                                 % (hap, len(found_vars), len(uniq_vars)))
            ignore_haps.add(hap)
    return [con for con in contrib_prop if con[0] not in ignore_haps]


def _contributor_table(phylo, obs, haplogroups, props, find, args):
    """assemble.get_contributors (assemble.py:31-100) around a candidate finder `find()` -> column indexes."""
    if not getattr(args, "contributors", None):
        contributors = find()
    else:
        contributors = []
        for con in args.contributors.split(","):
            try:
                contributors.append(haplogroups.index(con))
            except ValueError:
                raise ValueError("Unknown haplogroup '%s'" % (con))
    contrib_prop = [[haplogroups[con], props[con]] for con in contributors]
    contrib_prop.sort(key=lambda con: con[1], reverse=True)
    if args.var_check and not getattr(args, "contributors", None):
        contrib_prop = check_contrib_phy_vars(phylo, obs, contrib_prop, args)
    return _name_contributors(contrib_prop)


def _name_contributors(contrib_prop):
    """[[haplogroup, proportion], ...] -> [[hapNN, haplogroup, proportion], ...] (assemble.py:93-99)."""
    name_fmt = "hap%%0%dd" % (len(str(len(contrib_prop) + 1)))
    for num, con in enumerate(contrib_prop):
        con.insert(0, name_fmt % (num + 1))
    return contrib_prop


def get_contributors(phylo, obs, haplogroups, wts, em_results, args):
    """
    assemble.get_contributors (assemble.py:31-100): [[hapNN, haplogroup, proportion], ...] by descending proportion --
    the candidates with at least args.min_reads votes (or args.contributors, comma-separated: ValueError for an unknown
    one), filtered by check_contrib_phy_vars when args.var_check and no args.contributors.  em_results = (props,
    read_hap_mat) with the posterior matrix dense (numpy or device).
    """
    props, read_hap_mat = em_results
    return _contributor_table(phylo, obs, haplogroups, props,
                              lambda: find_contribs_from_reads(read_hap_mat, wts, args), args)


def get_contributors_records(phylo, obs, haplogroups, wts, props, cm, ln_theta_k, args):
    """get_contributors for a matrix held as records (no posterior matrix): the candidates of find_contribs_from_records."""
    return _contributor_table(phylo, obs, haplogroups, props,
                              lambda: find_contribs_from_records(cm, ln_theta_k, wts, args), args)


def read_votes(read_hap_mat):
    """Counter {column: number of rows voting for it}, unweighted (stats.py:39-40),
    with the reference's insertion order so that most_common() breaks ties alike."""
    best, votes = _row_argmax_votes_device(read_hap_mat, None)
    _, order, votes_h = _contributors_on_device(best, votes, votes.numel(), 0)
    counter = collections.Counter()
    for h in order:
        counter[int(h)] = int(votes_h[h])
    return counter


def report_read_votes(haplogroups, read_hap_mat, top_n=10):
    """stats.report_read_votes (stats.py:34-45), same text on stderr."""
    sys.stderr.write("\nTop 10 haplogroups by read probabilities...\n")
    for hap_i, count in read_votes(read_hap_mat).most_common(top_n):
        sys.stderr.write("%s\t%d\n" % (haplogroups[hap_i], count))
    sys.stderr.write("\n")


def update_contribs(contribs, em_results, haps):
    """assemble.update_contribs (assemble.py:211-230): refined proportions by name."""
    props, _ = em_results
    by_hap = {haps[i]: props[i] for i in range(len(haps))}
    for con in contribs:
        con[2] = by_hap[con[1]]
    return contribs


class AssignedReads(collections.abc.Mapping):
    """
    assign_read_indexes' result -- contributor name -> set of row indexes, plus 'unassigned' (assemble.py:284-334) -- held
    as ONE small integer per row: the sets are only formed when someone looks at them (a 10^6-row table of Python
    integers costs 40 ms to build and nothing downstream of the EM needs it before a writer asks).  Behaves like the
    reference's defaultdict(set) for reading: keys are the names that got at least one row (contributors in their
    order, then 'unassigned'), table[name] is a set (empty for a name without rows), dict(table) the reference's dict.
        count(name)   rows of `name` without forming the set
        rows(name)    their indexes as a numpy array (ascending)
    """

    def __init__(self, assigned, names):
        self._assigned = numpy.asarray(assigned)             # ordinal of the contributor, -1 = unassigned
        self._names = list(names)
        counts = numpy.bincount(self._assigned[self._assigned >= 0], minlength=len(self._names)) if self._assigned.size \
            else numpy.zeros(len(self._names), dtype=numpy.int64)
        self._counts = {name: int(counts[i]) for i, name in enumerate(self._names)}
        n_un = int((self._assigned < 0).sum())
        self._keys = [name for name in self._names if self._counts[name] > 0]
        if n_un:
            self._counts["unassigned"] = n_un
            self._keys.append("unassigned")
        self._sets = {}

    def rows(self, name):
        if name == "unassigned" and "unassigned" not in self._names:
            return numpy.flatnonzero(self._assigned < 0)
        if name not in self._names:
            return numpy.zeros(0, dtype=numpy.int64)
        return numpy.flatnonzero(self._assigned == self._names.index(name))

    def count(self, name):
        return self._counts.get(name, 0)

    def __getitem__(self, name):
        got = self._sets.get(name)
        if got is None:
            got = set(self.rows(name).tolist())
            if name in self._keys:
                self._sets[name] = got
        return got

    def __iter__(self):
        return iter(self._keys)

    def __len__(self):
        return len(self._keys)

    def __contains__(self, name):
        return name in self._keys

    def __eq__(self, other):
        try:
            return dict(self) == dict(other)
        except (TypeError, ValueError):
            return NotImplemented

    def __repr__(self):
        return "AssignedReads(%s)" % ", ".join("%s: %d" % (k, self._counts[k]) for k in self._keys)


def assign_read_indexes(contribs, em_results, haps, reads, min_fold):
    """
    assemble.assign_read_indexes (assemble.py:284-334): contributor name -> set
    of row indexes, plus 'unassigned'; a row goes to its best contributor when,
    after dividing out the mixture proportions, it beats the runner-up by
    min_fold.  One gather kernel (mxm_assign_reads) instead of an argsort of
    all H columns per row; the result is an AssignedReads (one integer per row, sets formed on demand).
    """
    return _assign_rows(contribs, em_results, haps, len(reads), min_fold)[0]


def _assign_rows(contribs, em_results, haps, n_rows, min_fold):
    """assign_read_indexes' AssignedReads and the per-row ordinals it was made from, still on the device (None with one
    contributor or fewer: every row is the first's)."""
    props, read_hap_mat = em_results
    names = [hap_n for hap_n, _, _ in contribs]
    if len(contribs) <= 1:
        return AssignedReads(numpy.zeros(n_rows, dtype=numpy.int32), names[:1]), None
    lib = _lib.load()
    dev = require_gpu()
    mat = as_device(read_hap_mat, torch.float64, dev)
    with numpy.errstate(divide="ignore"):
        log_props = numpy.log(numpy.asarray(props, dtype=numpy.float64))
    cols = numpy.array([haps.index(group) for _, group, _ in contribs], dtype=numpy.int32)
    lp_d = torch.from_numpy(log_props).to(dev)
    cols_d = torch.from_numpy(cols).to(dev)
    assigned = torch.empty(n_rows, dtype=torch.int32, device=dev)
    if n_rows:
        _lib.check(lib.mxm_assign_reads(mat.data_ptr(), mat.stride(0), lp_d.data_ptr(), cols_d.data_ptr(),
                                        len(cols), n_rows, mat.shape[1], float(numpy.log(min_fold)),
                                        assigned.data_ptr(), current_stream()), "mxm_assign_reads")
    return AssignedReads(assigned.cpu().numpy(), names), assigned


class ContribReads(collections.abc.Mapping):
    """
    assemble.assign_reads' result -- contributor name -> that contributor's alignments (assemble.py:233-264) -- held as
    ONE int32 label per alignment on the device: label k < n_contribs is contribs[k], label n_contribs 'unassigned'
    (two contributors or more), -1 an alignment whose fragment is in no row (it is in no table, as in the reference,
    where its read id is in no row's list).
        labels        int32 device tensor [n_aln]; names: the label -> name list
        joined        int32 device tensor [n_aln]: the extension round in which the alignment entered its list (0 =
                      assign_reads; assemble.extend_assemblies writes it) -- the order of a list is (joined, index)
        relabel(labels, joined=None)   take new labels (assemble's extension): counts and host copies are refreshed
        len(cr[name]) that contributor's alignment count (the "Reads" column of report_contributors)
        rows(name)    its alignment indexes (ascending: the file order the reference's lists keep), numpy int64
        as_dict(alns) the reference's dict: name -> [alns[i] for i in rows(name)] (indexes when alns is None)
    Behaves like the reference's defaultdict(list): the keys are the names that got alignments (in the order the
    AssignedReads lists them), and looking up another name adds it as a key with no alignments -- bin/mixemt's
    report_contributors does that for every contributor before write_statistics iterates the keys.
    """

    def __init__(self, cols, labels, names, keys, dcols=None, frag=None):
        self.cols = cols                                     # alignments.AlignmentColumns the labels index
        self.names = list(names)
        self._keys = list(keys)
        self._dcols = dcols
        self._frag = frag                                    # cols.frag on the device (made on demand)
        self.rounds = 0                                      # extension rounds these labels have been through
        self.relabel(labels, torch.zeros(labels.numel(), dtype=torch.int32, device=labels.device))

    def relabel(self, labels, joined=None):
        """Take new labels (and, when given, the rounds the alignments joined their lists in); the names and the keys
        stay what they are."""
        self.labels = labels
        if joined is not None:
            self.joined = joined
        n_labels = len(self.names)
        lab = labels[labels >= 0]
        self._counts = torch.bincount(lab.to(torch.int64), minlength=n_labels).cpu().numpy() if lab.numel() \
            else numpy.zeros(n_labels, dtype=numpy.int64)
        self._host = None

    def device_frag(self):
        """cols.frag (the alignments' fragment = query name) on the device, made once."""
        if self._frag is None:
            self._frag = torch.from_numpy(numpy.ascontiguousarray(self.cols.frag, dtype=numpy.int64)).to(self.labels.device)
        return self._frag

    def device_columns(self):
        """The alignments uploaded for the labelled pileup (observe.DeviceColumns), made once."""
        if self._dcols is None:
            from .observe import DeviceColumns
            self._dcols = DeviceColumns(self.cols, self.labels.device)
        return self._dcols

    def label_of(self, name):
        """The label of `name`, or None for a name without one (a key looked up that is no contributor)."""
        try:
            return self.names.index(name)
        except ValueError:
            return None

    def count(self, name):
        k = self.label_of(name)
        return 0 if k is None else int(self._counts[k])

    def rows(self, name):
        k = self.label_of(name)
        if k is None or not self._counts[k]:
            return numpy.zeros(0, dtype=numpy.int64)
        if self._host is None:
            self._host = self.labels.cpu().numpy()
        return numpy.flatnonzero(self._host == k)

    def as_dict(self, alns=None):
        if alns is None:
            return {name: self.rows(name).tolist() for name in self._keys}
        return {name: [alns[i] for i in self.rows(name)] for name in self._keys}

    def __getitem__(self, name):
        if name not in self._keys:
            self._keys.append(name)                          # (defaultdict(list): the lookup makes the key)
        return self.rows(name)

    def __iter__(self):
        return iter(list(self._keys))

    def __len__(self):
        return len(self._keys)

    def __contains__(self, name):
        return name in self._keys

    def __repr__(self):
        return "ContribReads(%s)" % ", ".join("%s: %d" % (k, self.count(k)) for k in self._keys)


def _row_groups(cols, reads):
    """(ptr, frag) of the rows' fragments: a ReadIdGroups' own arrays, or the reference's list of read-id lists mapped
    to fragment indexes of cols.names."""
    if hasattr(reads, "ptr") and hasattr(reads, "frag"):
        return numpy.asarray(reads.ptr, dtype=numpy.int64), numpy.asarray(reads.frag, dtype=numpy.int64)
    index = {name: f for f, name in enumerate(cols.names)}
    lens = [len(ids) for ids in reads]
    ptr = numpy.zeros(len(lens) + 1, dtype=numpy.int64)
    numpy.cumsum(lens, out=ptr[1:])
    frag = numpy.array([index[name] for ids in reads for name in ids], dtype=numpy.int64)
    return ptr, frag


def alignment_labels(frag, ptr, group_frag, row_label, n_frag, no_row=-1):
    """
    One int32 label per alignment (device): row_label[row of the alignment's fragment], or `no_row` when its fragment is
    in no row.  frag: the alignments' fragment indexes; ptr / group_frag: the rows' fragments (ReadIdGroups); row_label:
    int32 per row.  All device tensors (frag / group_frag int64, ptr int64).
    """
    dev = row_label.device
    frag_label = torch.full((max(int(n_frag), 1),), int(no_row), dtype=torch.int32, device=dev)
    if group_frag.numel():
        frag_label[group_frag] = torch.repeat_interleave(row_label, ptr[1:] - ptr[:-1],
                                                         output_size=int(group_frag.numel()))
    return frag_label[frag].contiguous() if frag.numel() else torch.zeros(0, dtype=torch.int32, device=dev)


def assign_reads(cols, contribs, em_results, haps, reads, args, dcols=None):
    """
    assemble.assign_reads (assemble.py:233-264) over alignments held as columns (alignments.AlignmentColumns; the
    reference re-reads the BAM file and matches query names): assign_read_indexes' rows, then every alignment of a
    row's fragments goes to that row's contributor (or 'unassigned').  reads: the rows' fragments (the encoder's
    ReadIdGroups, or the reference's list of read-id lists).  Returns a ContribReads, one label per alignment, made on
    the device.  dcols: the columns already uploaded (observe.DeviceColumns), reused by write_statistics.
    """
    dev = require_gpu()
    table, assigned = _assign_rows(contribs, em_results, haps, len(reads), args.min_fold)
    names = [hap_n for hap_n, _, _ in contribs]
    if len(contribs) > 1:
        names.append("unassigned")
        row_label = torch.where(assigned >= 0, assigned, torch.full_like(assigned, len(contribs)))
    else:
        row_label = torch.zeros(len(reads), dtype=torch.int32, device=dev)
    ptr, group_frag = _row_groups(cols, reads)
    n_frag = max(len(cols.names), int(cols.frag.max()) + 1 if len(cols) else 0)
    frag_d = torch.from_numpy(cols.frag).to(dev)
    labels = alignment_labels(frag_d, torch.from_numpy(ptr).to(dev), torch.from_numpy(group_frag).to(dev), row_label,
                              n_frag)
    return ContribReads(cols, labels, names, list(table), dcols, frag_d)


# ---- the variant check of many samples on the device (mxm_check_variants_samples) ------------------------------------------
VAR_CHECK_MAX_CANDS = 64            # candidates a sample may have on the device route (the widest table stride of the entry)
VAR_CHECK_MAX_L = 131072            # MXM_VAR_CHECK_MAX_L of include/mixemt_hip_var_check.h: the kernel's bitsets live in LDS


class VarCheckTables(object):
    """
    What check_contrib_phy_vars reads from the tree, as int32 arrays in the column order of `haplogroups` (numpy: the
    attributes ending in _h; device tensors without the suffix when a device was given):
        key_ptr [H + 1], key [nnz]   the keys of haplogroup h are the distinct pos * 4 + code of (pos_from_var(v),
                                     der_allele(v)) for v in phylo.hap_var[h], code = index in "ACGT", ascending
        site [n_sites]               phylo.get_variant_pos(), ascending
        site_key [n_sites]           site * 4 + code of refseq[site], or -1 where the reference base is not one of ACGT
        max_pos                      the largest position in key / site (-1: none); n_haps; phylo: the tree it was built from
    The tables are built from hap_var / variants as they stand when build() is called, so custom haplogroups
    (add_custom_hap) and ignored sites (ignore_sites) are covered -- and a tree edited afterwards needs a new build.
    """
    CODES = {base: code for code, base in enumerate("ACGT")}

    def __init__(self, phylo, key_ptr, key, site, site_key, dev=None):
        self.phylo = phylo
        self.key_ptr_h, self.key_h, self.site_h, self.site_key_h = key_ptr, key, site, site_key
        self.n_haps = len(key_ptr) - 1
        self.max_pos = max(int(key.max()) >> 2 if len(key) else -1, int(site.max()) if len(site) else -1)
        self.device = dev
        self.key_ptr = self.key = self.site = self.site_key = None
        if dev is not None:
            def up(arr):
                return torch.from_numpy(arr if arr.size else numpy.zeros(1, dtype=numpy.int32)).to(dev)
            self.key_ptr, self.key, self.site, self.site_key = up(key_ptr), up(key), up(site), up(site_key)

    @classmethod
    def build(cls, phylo, haplogroups, dev=None):
        """The tables of `phylo` for the columns `haplogroups` (uploaded to `dev` when given), or None when a derived
        allele is not one of ACGT: the caller then takes the host route."""
        from .phylotree import der_allele, pos_from_var
        codes = cls.CODES
        seen = {}                                             # variant string -> key (the haplogroups share most of them)
        key_ptr = numpy.zeros(len(haplogroups) + 1, dtype=numpy.int64)
        keys = []
        for h, hap in enumerate(haplogroups):
            own = set()
            for var in phylo.hap_var[hap]:
                k = seen.get(var)
                if k is None:
                    code = codes.get(der_allele(var))
                    if code is None:
                        return None
                    k = seen[var] = pos_from_var(var) * 4 + code
                own.add(k)
            keys.extend(sorted(own))
            key_ptr[h + 1] = len(keys)
        site = numpy.asarray(phylo.get_variant_pos(), dtype=numpy.int64)
        # A reference base outside ACGT (say 'N') gives -1 and is never claimed: the claimed pairs are only ever compared
        # with (position, derived base) pairs, whose base IS one of ACGT, so a claimed (pos, 'N') can never equal one and
        # dropping it changes no decision.
        ref_code = [codes.get(phylo.refseq[p]) for p in site.tolist()]
        site_key = numpy.array([-1 if code is None else p * 4 + code for p, code in zip(site.tolist(), ref_code)],
                               dtype=numpy.int64)
        if (len(keys) and max(keys) >= 2 ** 31) or len(keys) >= 2 ** 31:
            return None
        return cls(phylo, key_ptr.astype(numpy.int32), numpy.asarray(keys, dtype=numpy.int32).reshape(-1),
                   site.astype(numpy.int32), site_key.astype(numpy.int32), dev)


def _var_check_ld(widest):
    for ld in (4, 8, 16, 32, 64):
        if widest <= ld:
            return ld
    raise ValueError("the device variant check takes at most %d candidates per sample" % VAR_CHECK_MAX_CANDS)


def check_variants_samples(counts, tables, cands, args, want_counts=False):
    """
    check_contrib_phy_vars for many samples in ONE launch (mxm_check_variants_samples) over pileups on the device.
    counts: int32 device tensor [S][L][16] (observe.CohortPileup.counts); tables: a VarCheckTables built with a device;
    cands: per sample the candidates' haplogroup indexes in checking order (descending proportion); args: min_var_reads,
    frac_var_reads, var_fraction, var_count.  Returns keep (numpy bool [S][ld]: keep[s][:len(cands[s])] is the sample's)
    and, with want_counts, also n_uniq and n_found (int32 [S][ld]): the two numbers the reference prints per candidate.
    """
    if counts.dim() != 3 or counts.shape[2] != 16 or counts.dtype != torch.int32 or not counts.is_contiguous():
        raise ValueError("counts must be a contiguous int32 [S][L][16] device tensor")
    if tables.key_ptr is None:
        raise ValueError("check_variants_samples: the tables were built without a device")
    n = len(cands)
    if counts.shape[0] != n:
        raise ValueError("check_variants_samples: %d pileups for %d candidate lists" % (counts.shape[0], n))
    ld = _var_check_ld(max([len(c) for c in cands] + [1]))
    cand = numpy.zeros((n, ld), dtype=numpy.int32)
    ncand = numpy.zeros(n, dtype=numpy.int32)
    for s, c in enumerate(cands):
        ncand[s] = len(c)
        cand[s, :len(c)] = c
    dev = counts.device
    keep = torch.zeros((n, ld), dtype=torch.uint8, device=dev)
    n_uniq = torch.zeros((n, ld), dtype=torch.int32, device=dev) if want_counts else None
    n_found = torch.zeros((n, ld), dtype=torch.int32, device=dev) if want_counts else None
    var_count = getattr(args, "var_count", None)
    _lib.check(_lib.load().mxm_check_variants_samples(
        counts.data_ptr(), n, int(counts.shape[1]), tables.key_ptr.data_ptr(), tables.key.data_ptr(), tables.n_haps,
        tables.site.data_ptr(), tables.site_key.data_ptr(), len(tables.site_h), tables.max_pos, cand.ctypes.data,
        ncand.ctypes.data, ld, float(args.min_var_reads), float(args.frac_var_reads), float(args.var_fraction),
        0 if var_count is None else 1, 0 if var_count is None else int(var_count), keep.data_ptr(), ptr(n_uniq), ptr(n_found),
        current_stream()), "mxm_check_variants_samples")
    keep_h = keep.cpu().numpy().astype(bool)
    if want_counts:
        return keep_h, n_uniq.cpu().numpy(), n_found.cpu().numpy()
    return keep_h


# ---- the second half of a cohort run, batched (em.run_em_many's counterpart) ------------------------------------------
FINISH_KMAX = 16                    # contributors a batched sample may have (the reduced matrix's widest row stride)
FINISH_MAX_ROWS = 100000            # rows up to which one workgroup per sample was measured not slower than the per-sample
                                    # refinement (S = 64: 0.10 / 0.15 / 0.44 / 1.00 of the per-sample loop's wall time at 600 /
                                    # 4 600 / 3 * 10^4 / 10^5 rows, profiles/samples/finish.md); nothing larger was measured.
                                    # Measured for ONE run per sample only: finish_many(runs="batch") shares the limit
                                    # (profiles/samples/runs.md)
FINISH_RUNS_MAX = 64                # runs per sample the batch route takes with runs="batch" (MXM_SAMPLES_RUNS_MAX: a cap)


def _finish_route(n_rows, first_route, n_multi, max_rows, n_contribs=None, n_columns=None, runs="single"):
    """'batch' or 'single' for one sample of finish_many: the per-sample functions take a sample whose first EM ran on
    its own, every sample of a multi-run (the fold of the runs' posteriors, em.py:156, is theirs) unless runs="batch"
    and there are at most FINISH_RUNS_MAX runs, one of more than max_rows rows, and -- once its contributors are known --
    one with more than FINISH_KMAX of them (or with a haplogroup named twice, whose reduced matrix has fewer columns than
    contributors)."""
    if runs not in ("single", "batch"):
        raise ValueError("finish_many: runs must be 'single' or 'batch', not %r" % (runs,))
    if first_route == "single" or n_rows > max_rows or (n_multi > 1 and (runs == "single" or n_multi > FINISH_RUNS_MAX)):
        return "single"
    if n_contribs is not None and (n_contribs > FINISH_KMAX or (n_columns is not None and n_columns != n_contribs)):
        return "single"
    return "batch"


def _finish_columns(contribs, hap_index):
    """One sample's column plan: (cols, perm, sub_haps).  The reduced matrix keeps the contributors' columns in ASCENDING
    haplogroup index (preprocess.py:247-251), the contributor table is by descending proportion: cols[i] is the
    haplogroup index of reduced column i, perm[i] the ordinal of that haplogroup's contributor."""
    idx = [hap_index[con[1]] for con in contribs]
    order = sorted(range(len(idx)), key=lambda k: idx[k])
    return [idx[k] for k in order], order, [contribs[k][1] for k in order]


def _finish_tables(plans):
    """The batch's [S][ld] tables from the batched samples' column plans: (ld, cols, ncol, perm) with ld = 4, 8 or 16 by
    the largest number of columns among THESE samples; pad entries are 0."""
    widest = max([len(cols) for cols, _, _ in plans] + [1])
    if widest > FINISH_KMAX:
        raise ValueError("finish_many: a batched sample may have at most %d contributors" % FINISH_KMAX)
    ld = 4 if widest <= 4 else (8 if widest <= 8 else 16)
    cols = numpy.zeros((len(plans), ld), dtype=numpy.int32)
    perm = numpy.zeros((len(plans), ld), dtype=numpy.int32)
    ncol = numpy.zeros(len(plans), dtype=numpy.int32)
    for s, (c, p, _) in enumerate(plans):
        ncol[s] = len(c)
        cols[s, :len(c)] = c
        perm[s, :len(c)] = p
    return ld, cols, ncol, perm


def _finish_inits(n_cols, refine_inits, alpha, n_multi=1):
    """The refinements' initial proportions: n_cols[s] = columns of sample s's reduced matrix, None for a sample that is
    not refined.  refine_inits None: init_props(K_s) from numpy's global legacy stream, sample after sample, refined
    samples only (n_multi draws each).  A list of [n_multi][K_s] arrays (None where not refined)."""
    from .em import init_props
    if refine_inits is not None and len(refine_inits) != len(n_cols):
        raise ValueError("finish_many: refine_inits needs one entry per sample")
    out = []
    for s, k in enumerate(n_cols):
        if k is None:
            out.append(None)
        elif refine_inits is None:
            out.append(numpy.stack([init_props(k, alpha=alpha) for _ in range(n_multi)]))
        else:
            init = numpy.atleast_2d(numpy.ascontiguousarray(refine_inits[s], dtype=numpy.float64))
            if init.shape != (n_multi, k):
                raise ValueError("finish_many: refine_inits[%d] must hold %d proportions, in the reduced matrix's column "
                                 "order (ascending haplogroup index)" % (s, k))
            out.append(init)
    return out


def _fixed_contributors(args, hap_index):
    """args.contributors as haplogroup indexes (None when it is empty): ValueError for an unknown one, as
    get_contributors raises it."""
    fixed = getattr(args, "contributors", None)
    if not fixed:
        return None
    cols = []
    for con in fixed.split(","):
        if con not in hap_index:
            raise ValueError("Unknown haplogroup '%s'" % (con))
        cols.append(hap_index[con])
    return cols


def _finish_check(samples, results, haplogroups, args, obs, phylo=None, var_tables=None):
    """finish_many's argument checks (host only); returns the haplogroup -> index table."""
    from .preprocess import CodedMatrix
    if not samples or len(results) != len(samples):
        raise ValueError("finish_many: one result of run_em_many per sample is needed (%d samples, %d results)"
                         % (len(samples), len(results)))
    mats = [pair[0] for pair in samples]
    if any(not isinstance(m, CodedMatrix) for m in mats) or any(m.rec.data_ptr() != mats[0].rec.data_ptr() for m in mats):
        raise ValueError("finish_many: the samples must be views of ONE record buffer (preprocess.build_em_records_many's "
                         "matrix and cm.rows(lo, hi) of it)")
    hap_index = {}
    for i, hap in enumerate(haplogroups):
        hap_index.setdefault(hap, i)
    if mats[0].n_haps != len(haplogroups):
        raise ValueError("finish_many: %d haplogroups for matrices of %d columns" % (len(haplogroups), mats[0].n_haps))
    fixed = _fixed_contributors(args, hap_index)
    if args.var_check and fixed is None:
        if obs is None:
            raise ValueError("finish_many: args.var_check without args.contributors needs obs= (one observe.ObservedBases "
                             "per sample) and phylo=")
        if len(obs) != len(samples):
            raise ValueError("finish_many: obs needs one entry per sample (%d samples, %d entries)" % (len(samples), len(obs)))
        if _is_cohort_pileup(obs):
            if phylo is None:
                raise ValueError("finish_many: the variant check needs phylo=")
            if var_tables is not None and var_tables.n_haps != len(haplogroups):
                raise ValueError("finish_many: var_tables was built for %d haplogroups, the samples have %d"
                                 % (var_tables.n_haps, len(haplogroups)))
    return hap_index, fixed


def _is_cohort_pileup(obs):
    from .observe import CohortPileup
    return isinstance(obs, CohortPileup)


def _empty_finish(route, order, votes):
    return {"contribs": [], "vote_order": order, "votes": votes, "sub_haps": [], "refined": None,
            "assigned": AssignedReads(numpy.zeros(0, dtype=numpy.int32), []), "row_label": numpy.zeros(0, dtype=numpy.int32),
            "route": route, "posterior": None, "var_check": None}


def _finish_single(cm, wts, res, contribs, order, votes, haplogroups, hap_index, args, init, want_posterior):
    """One sample through the existing per-sample functions (reduce_em_records -> run_em_ex -> update_contribs ->
    _assign_rows; unrefined: the full-width posterior of the first EM), with finish_many's result dict."""
    from . import em, preprocess
    if not contribs:
        return _empty_finish("single", order, votes)
    _, _, sub_haps = _finish_columns(contribs, hap_index)
    refined = posterior = None
    if args.refine_ests:
        sub, sub_haps = preprocess.reduce_em_records(cm, haplogroups, contribs)
        run = em.run_em_ex(sub, wts, args, inits=init)
        contribs = update_contribs(contribs, (run["props"], run["read_mix"]), sub_haps)
        table, assigned = _assign_rows(contribs, (run["props"], run["read_mix"]), sub_haps, cm.n_rows, args.min_fold)
        refined = {key: run[key] for key in ("props", "iters", "done", "l1", "inits")}
        posterior = run["read_mix"] if want_posterior else None
    else:
        read_mix = em.RecordsPosterior(cm, res["ln_theta_k"]).dense()
        table, assigned = _assign_rows(contribs, (res["props"], read_mix), haplogroups, cm.n_rows, args.min_fold)
    label = numpy.zeros(cm.n_rows, dtype=numpy.int32) if assigned is None else assigned.cpu().numpy()
    return {"contribs": contribs, "vote_order": order, "votes": votes, "sub_haps": sub_haps, "refined": refined,
            "assigned": table, "row_label": label, "route": "single", "posterior": posterior, "var_check": None}


def _finish_batch(samples, wts_d, ids):
    """em.SampleFinish over the samples `ids` (their record offsets back to back; nothing of the records is copied)."""
    from . import em
    mats = [samples[i][0] for i in ids]
    row0 = numpy.concatenate([[0], numpy.cumsum([m.n_rows for m in mats])]).astype(numpy.int64)
    return em.SampleFinish(mats[0].rec, torch.cat([m.rec_off for m in mats]), torch.cat([m.ndist for m in mats]),
                           torch.cat([wts_d[i] for i in ids]), torch.cat([m.rowmax for m in mats]), row0, mats[0].n_haps)


def finish_many(samples, results, haplogroups, args, phylo=None, obs=None, refine_inits=None, max_rows=None,
                want_posterior=False, var_tables=None, runs="single"):
    """
    What mixemt reports for a sample after its EM (bin/mixemt:298-323: get_contributors, the refinement run_em on the
    contributors' columns with update_contribs, assign_read_indexes) for ALL samples of one em.run_em_many call in
    batched device passes, instead of a Python loop of get_contributors_records / reduce_em_records / run_em /
    _assign_rows over them.  Opt-in; the per-sample functions are unchanged.
    samples: run_em_many's list of (preprocess.CodedMatrix, weights), views of ONE record buffer
        (preprocess.build_em_records_many's matrix and cm.rows(lo, hi) of it); anything else is a ValueError.
    results: run_em_many's list (props and ln_theta_k are read).
    args: the reference's namespace -- min_reads, contributors, var_check (with min_var_reads, frac_var_reads, var_count,
        var_fraction, verbose), refine_ests, min_fold, tolerance, max_iter, init_alpha, n_multi.
    phylo / obs: for the variant check, required when args.var_check is set and args.contributors is empty.  obs is a list
        with one observe.ObservedBases per sample (check_contrib_phy_vars, run per sample on the host as it is), or an
        observe.CohortPileup (observe.observe_bases_many): the pileups stay on the device and ONE
        mxm_check_variants_samples call checks every sample with at most 64 candidates (a sample on the "single" route
        after its own vote); what that call cannot take goes through check_contrib_phy_vars over obs.host(s), unchanged --
        args.verbose (the stderr lines are the reference's), a sample with more candidates, a tree with a derived allele
        outside ACGT, a pileup shorter than the tree's last variant or longer than 131 072 positions.
    var_tables: a VarCheckTables.build(phylo, haplogroups, device) to reuse between calls (CohortPileup only); built once per
        call otherwise.  A tree edited since needs a new build.
    refine_inits: None draws init_props(K_s) from numpy's global legacy stream, sample after sample, only for the samples
        that are refined -- NOT the stream position a Python loop over whole samples would reach (there the first EM's
        draw of sample s + 1 follows the refinement draw of sample s); or a list with [K_s] proportions per sample (None
        where nothing is refined), in the REDUCED matrix's column order: ascending haplogroup index (preprocess.py:247-251),
        not contributor order.
        With args.n_multi = B > 1: [B][K_s] per sample; None draws B vectors per refined sample, still sample after sample
        (sample s's B draws, then sample s + 1's), whichever route a sample takes.
    max_rows: a sample of more rows takes the per-sample route (default FINISH_MAX_ROWS).
    runs: what happens to the samples when args.n_multi > 1 (mixemt's -M).  "single", the default: every sample takes the
        per-sample route.  "batch": a sample stays on the batch route whenever everything else allows it -- its first EM
        was batched, at most max_rows rows, at most 16 contributors, no haplogroup named twice -- and args.n_multi <= 64;
        the vote and the read assignment then work on the runs' posteriors folded in run order as run_em folds them
        (mxm_votes_samples_runs, mxm_assign_reads_samples_runs) and the refinement runs one workgroup per (sample, run)
        (mxm_em_loop_samples_narrow_runs).  `refined` then holds props = the runs' geometric mean (em._fold_runs), iters /
        done / l1 as lists of B, inits / ln_theta_k / ln_theta_next as [B][K_s]; `posterior` is the folded reduced
        posterior; unrefined, the rows are assigned from the first EM's folded posterior and folded props.  Anything else
        is a ValueError.  With args.n_multi == 1 the keyword changes nothing.
    Returns one dict per sample:
        contribs    [[hapNN, haplogroup, proportion], ...] as get_contributors and update_contribs leave it
        vote_order, votes   what vote_table_from_records returns (haplogroups in first-seen order, unweighted votes [H])
        sub_haps    the reduced matrix's column names
        refined     {props, iters, done, l1, inits} of the refinement run (batch route: also ln_theta_k and ln_theta_next,
                    the loop's own log vectors); None when args.refine_ests is false (the rows are then assigned from
                    the first EM's posterior, contributors' columns only) or nothing contributes
        assigned    an AssignedReads (contributor order); row_label: its int32 [R_s] ordinals, -1 = unassigned
        route       "batch", or "single": the sample went through the per-sample functions -- its first EM ran on its
                    own, args.n_multi > 1 without runs="batch" (or more than 64 runs), more than max_rows rows, or more
                    than 16 contributors
        var_check   "device" or "host": where the sample's candidates were checked; None when the check is off
                    (args.var_check false, or args.contributors given)
        posterior   always present; None unless want_posterior is set (an addition to mixemt's own outputs, for tests and
                    for `-s`-like dumps): then the reduced posterior under theta_k ([R_s][K_s], device), refined samples only
    A sample without a contributor returns contribs == [], refined None and an empty AssignedReads; nothing is launched
    for it.  A sample with ONE contributor is still refined on R x 1, as bin/mixemt:311-320 does.
    """
    from . import em
    hap_index, fixed = _finish_check(samples, results, haplogroups, args, obs, phylo, var_tables)
    n = len(samples)
    n_multi = int(getattr(args, "n_multi", 1))
    if runs not in ("single", "batch"):
        raise ValueError("finish_many: runs must be 'single' or 'batch', not %r" % (runs,))
    max_rows = FINISH_MAX_ROWS if max_rows is None else int(max_rows)
    dev = require_gpu()
    wts_d = [as_device(w, torch.float64, dev).reshape(-1) for _, w in samples]
    if any(int(w.numel()) != m.n_rows for w, (m, _) in zip(wts_d, samples)):
        raise ValueError("finish_many: weights do not match the samples' rows")
    route = [_finish_route(samples[s][0].n_rows, results[s].get("route"), n_multi, max_rows, runs=runs) for s in range(n)]
    contribs, orders, counts = [None] * n, [None] * n, [None] * n
    checked = bool(args.var_check) and fixed is None
    cohort = checked and _is_cohort_pileup(obs)
    if cohort:
        obs_of = obs.host                                   # (downloads the sample's table: host-route samples only)
    else:
        obs_of = (lambda s: obs[s]) if obs is not None else (lambda s: None)
    var_route = ["host" if checked else None] * n
    on_device = False
    if cohort and not args.verbose and obs.L <= VAR_CHECK_MAX_L:
        if var_tables is None:
            var_tables = VarCheckTables.build(phylo, haplogroups, dev)
        on_device = var_tables is not None and var_tables.key_ptr is not None and var_tables.max_pos < obs.L
    pending = {}                                            # sample -> its candidates in checking order (device route)

    # ---- votes and contributor tables ----
    voted = [s for s in range(n) if route[s] == "batch"]
    first_batch = lse_all = None
    if voted:
        first_batch = _finish_batch(samples, wts_d, voted)
        if n_multi > 1:                                      # (runs="batch": the vote over the runs' folded posterior)
            ln_props = numpy.stack([numpy.atleast_2d(results[s]["ln_theta_k"]) for s in voted])
            if ln_props.shape[1] != n_multi:
                raise ValueError("finish_many: args.n_multi = %d, the results hold %d runs" % (n_multi, ln_props.shape[1]))
            _, votes_w, counts_h, first_h, lse_all, errors = first_batch.votes_runs(ln_props, want_lse=not args.refine_ests)
        else:
            ln_props = numpy.stack([numpy.atleast_2d(results[s]["ln_theta_k"])[0] for s in voted])
            _, votes_w, counts_h, first_h, lse_all, errors = first_batch.votes(ln_props, want_lse=not args.refine_ests)
        for j, s in enumerate(voted):
            if errors[j]:
                raise ValueError("finish_many: sample %d has a row without a record (ndist outside 1 .. 1024)" % s)
            n_rows = samples[s][0].n_rows
            seen = numpy.flatnonzero(first_h[j] < n_rows)
            order = seen[numpy.argsort(first_h[j][seen], kind="stable")]
            orders[s], counts[s] = order, counts_h[j].astype(numpy.float64)
            found = [int(h) for h in order if votes_w[j][h] >= args.min_reads]
            if on_device and len(found) <= VAR_CHECK_MAX_CANDS:
                props = results[s]["props"]
                pending[s] = sorted(found, key=lambda con: props[con], reverse=True)    # (stable, as _contributor_table's sort)
            else:
                contribs[s] = _contributor_table(phylo, obs_of(s) if checked else None, haplogroups, results[s]["props"],
                                                 lambda: found, args)
    for s in range(n):
        if route[s] == "single":
            cm = samples[s][0]
            orders[s], counts[s] = vote_table_from_records(cm, results[s]["ln_theta_k"], None)
            if on_device:                                   # (its own vote, then the cohort's one check launch)
                found = find_contribs_from_records(cm, results[s]["ln_theta_k"], wts_d[s], args)
                if len(found) <= VAR_CHECK_MAX_CANDS:
                    props = results[s]["props"]
                    pending[s] = sorted(found, key=lambda con: props[con], reverse=True)
                    continue
            contribs[s] = get_contributors_records(phylo, obs_of(s) if checked else None, haplogroups, wts_d[s],
                                                   results[s]["props"], cm, results[s]["ln_theta_k"], args)
    if pending:
        # one launch for every sample that takes the device check; a sample that is not in it has no candidates there
        keep = check_variants_samples(obs.counts, var_tables, [pending.get(s, []) for s in range(n)], args)
        for s, cand in pending.items():
            props = results[s]["props"]
            contribs[s] = _name_contributors([[haplogroups[con], props[con]] for i, con in enumerate(cand) if keep[s, i]])
            var_route[s] = "device"

    # ---- column plans; the samples that leave the batch now that their contributors are known ----
    plans = [None] * n
    for s in range(n):
        if contribs[s]:
            plans[s] = _finish_columns(contribs[s], hap_index)
            if route[s] == "batch":
                route[s] = _finish_route(samples[s][0].n_rows, results[s].get("route"), n_multi, max_rows,
                                         len(contribs[s]), len(set(plans[s][0])), runs=runs)
    refine = bool(args.refine_ests)
    inits = _finish_inits([len(set(plans[s][0])) if (refine and plans[s] is not None) else None for s in range(n)],
                          refine_inits, args.init_alpha, n_multi)

    out = [None] * n
    for s in range(n):
        if not contribs[s]:
            out[s] = _empty_finish(route[s], orders[s], counts[s])
        elif route[s] == "single":
            out[s] = _finish_single(samples[s][0], wts_d[s], results[s], contribs[s], orders[s], counts[s], haplogroups,
                                    hap_index, args, inits[s], want_posterior)
    for s in range(n):
        if out[s] is not None:
            out[s]["var_check"] = var_route[s]
    ids = [s for s in range(n) if out[s] is None]
    if not ids:
        return out

    # ---- the batch: gather, refinement loop, assignment ----
    batch = first_batch if ids == voted else _finish_batch(samples, wts_d, ids)
    ld, cols, ncol, perm = _finish_tables([plans[s] for s in ids])
    mat = batch.gather(cols, ncol, ld)
    many = n_multi > 1
    ln_theta = numpy.full((len(ids), n_multi, ld) if many else (len(ids), ld), -numpy.inf)
    log_props = numpy.full((len(ids), ld), -numpy.inf)
    refined = [None] * len(ids)
    lse = None
    if refine and many:
        ln_cur, ln_new, states = batch.em_loop_runs(mat, ld, ncol, [inits[s] for s in ids], args.tolerance, args.max_iter)
        for j, s in enumerate(ids):
            k = int(ncol[j])
            props = em._fold_runs(ln_new[j, :, :k])                             # em.py:155, :163
            refined[j] = {"props": props, "iters": [st[1] for st in states[j]], "done": [st[0] for st in states[j]],
                          "l1": [st[2] for st in states[j]], "inits": inits[s], "ln_theta_k": ln_cur[j, :, :k].copy(),
                          "ln_theta_next": ln_new[j, :, :k].copy()}
            contribs[s] = update_contribs(contribs[s], (props, None), plans[s][2])
            ln_theta[j, :, :k] = ln_cur[j, :, :k]
            with numpy.errstate(divide="ignore"):
                log_props[j, :k] = numpy.log(props)
    elif refine:
        ln_cur, ln_new, states = batch.em_loop(mat, ld, ncol, [inits[s][0] for s in ids], args.tolerance, args.max_iter)
        for j, s in enumerate(ids):
            k = int(ncol[j])
            props = numpy.exp(ln_new[j, :k])                                    # em.py:163 with one run
            refined[j] = {"props": props, "iters": [states[j][1]], "done": [states[j][0]], "l1": [states[j][2]],
                          "inits": inits[s], "ln_theta_k": ln_cur[j, :k].copy(), "ln_theta_next": ln_new[j, :k].copy()}
            contribs[s] = update_contribs(contribs[s], (props, None), plans[s][2])
            ln_theta[j, :k] = ln_cur[j, :k]
            with numpy.errstate(divide="ignore"):
                log_props[j, :k] = numpy.log(props)
    else:
        # the first EM's posterior, contributors' columns only: its full-width row normaliser comes from the vote pass
        if ids == voted:
            lse = lse_all
        else:
            start = numpy.concatenate([[0], numpy.cumsum([samples[s][0].n_rows for s in voted])])
            at = {s: j for j, s in enumerate(voted)}
            lse = torch.cat([lse_all[int(start[at[s]]):int(start[at[s] + 1])] for s in ids])
        for j, s in enumerate(ids):
            k = int(ncol[j])
            if many:
                ln_theta[j, :, :k] = numpy.atleast_2d(results[s]["ln_theta_k"])[:, cols[j, :k]]
            else:
                ln_theta[j, :k] = numpy.atleast_2d(results[s]["ln_theta_k"])[0][cols[j, :k]]
            with numpy.errstate(divide="ignore"):
                log_props[j, :k] = numpy.log(numpy.asarray(results[s]["props"], dtype=numpy.float64)[cols[j, :k]])
    assigned, post = (batch.assign_runs if many else batch.assign)(mat, ld, ncol, perm, ln_theta, log_props, lse, args.min_fold,
                                                                   want_post=want_posterior and refine)
    labels = assigned.cpu().numpy()
    for j, s in enumerate(ids):
        lo, hi = int(batch.row0[j]), int(batch.row0[j + 1])
        names = [con[0] for con in contribs[s]]
        label = labels[lo:hi].copy()
        out[s] = {"contribs": contribs[s], "vote_order": orders[s], "votes": counts[s], "sub_haps": plans[s][2],
                  "refined": refined[j], "assigned": AssignedReads(label, names),
                  "row_label": label, "route": "batch", "var_check": var_route[s],
                  "posterior": post[lo:hi, :int(ncol[j])] if post is not None else None}
    return out


# ---- the third stage of a cohort run: one label per alignment for ALL samples (assign_reads' counterpart) --------------------
COHORT_TABLES_BYTES = 4 << 30       # default budget for the [n_labels][L][16] tables of the cohort's assembly stage: a cap,
                                    # not a measurement


def _cohort_budget(who, n_labels, L, max_bytes):
    need = int(n_labels) * int(L) * 64
    if need > int(max_bytes):
        raise ValueError("%s: %d labels x %d positions need %d bytes of pileup tables, above the budget of %d bytes "
                         "(max_bytes): split the cohort" % (who, n_labels, L, need, int(max_bytes)))


def _cohort_label_plan(finished, n_rows):
    """
    The global labels of a cohort from finish_many's list (host only): with K_s = len(contribs), sample s owns the labels
    lab0[s] .. lab0[s] + K_s -- its contributors in order, then its 'unassigned' (the slot is always reserved; no alignment
    carries it when K_s == 1, as assign_reads has no such label then).  n_rows[s]: the sample's rows.
    -> (lab0 int64 [S + 1], names per sample as assign_reads names its labels, keys per sample as it orders them, the rows'
    GLOBAL labels per sample: numpy int32 [R_s]).  A sample without contributors has no names, no keys and every row -1.
    """
    lab0 = numpy.zeros(len(finished) + 1, dtype=numpy.int64)
    names, keys, rows = [], [], []
    for s, fin in enumerate(finished):
        contribs = fin["contribs"]
        k = len(contribs)
        lab0[s + 1] = lab0[s] + k + 1
        names.append([con[0] for con in contribs] + (["unassigned"] if k > 1 else []))
        keys.append(list(fin["assigned"]) if k else [])
        if k == 0:
            row = numpy.full(int(n_rows[s]), -1, dtype=numpy.int64)
        elif k == 1:
            row = numpy.full(int(n_rows[s]), lab0[s], dtype=numpy.int64)
        else:
            local = numpy.asarray(fin["row_label"], dtype=numpy.int64)
            if local.shape != (int(n_rows[s]),):
                raise ValueError("assign_reads_many: sample %d has %d rows of fragments and %d row labels"
                                 % (s, int(n_rows[s]), local.size))
            if local.size and int(local.max()) >= k:
                raise ValueError("assign_reads_many: sample %d has a row label >= its %d contributors" % (s, k))
            row = numpy.where(local >= 0, lab0[s] + local, lab0[s] + k)
        rows.append(row.astype(numpy.int32))
    if int(lab0[-1]) >= 2 ** 31:
        raise ValueError("assign_reads_many: more than 2^31 - 1 labels")
    return lab0, names, keys, rows


class CohortContribReads(object):
    """
    assign_reads' result for ALL samples of a cohort (assign_reads_many): ONE int32 label per alignment over the
    concatenated columns, the labels GLOBAL -- sample s owns lab0[s] .. lab0[s] + K_s (its contributors, then 'unassigned');
    -1 stays -1.
        cols_list, cols, aln0    the samples' columns, their concatenation (alignments.concat_columns) and the samples' first
                                 alignments; device_columns() / device_frag(): the upload, made once
        lab0, n_labels, aln_sample   int64 [S + 1]; lab0[-1]; int32 device tensor [n_aln]: the sample of each alignment
        labels, joined           int32 device tensors [n_aln] (assemble.extend_assemblies_many updates them in place)
        rounds                   per sample the extension rounds its labels have been through; round_log: per sample one
                                 (moved, unassigned before, new variants) per round (assemble.extend_assemblies_many)
        names, keys              per sample what ContribReads.names and its keys would be
        max_bytes                the budget of the assembly stage's tables (assign_reads_many)
        sample(s)                an ordinary ContribReads over cols_list[s] with the sample's LOCAL labels, joined and rounds
                                 (copies: changing it does not change the cohort): stats.report_contributors,
                                 stats.write_statistics, assemble.write_consensus_seqs and as_dict work on it unchanged
        label_of(s, name)        the global label of a name of sample s, or None
        counts()                 alignments per global label, numpy int64 [n_labels]
    """

    def __init__(self, cols_list, cols, aln0, lab0, names, keys, labels, aln_sample, dcols=None, frag=None,
                 max_bytes=COHORT_TABLES_BYTES):
        self.cols_list, self.cols = list(cols_list), cols
        self.aln0 = numpy.asarray(aln0, dtype=numpy.int64)
        self.lab0 = numpy.asarray(lab0, dtype=numpy.int64)
        self.n_samples, self.n_labels = len(self.cols_list), int(self.lab0[-1])
        self.names = [list(n) for n in names]
        self.keys = [list(k) for k in keys]
        self.labels, self.aln_sample = labels, aln_sample
        self.joined = torch.zeros(labels.numel(), dtype=torch.int32, device=labels.device)
        self.rounds = [0] * self.n_samples
        self.round_log = [[] for _ in range(self.n_samples)]
        self.max_bytes = int(max_bytes)
        self._dcols, self._frag = dcols, frag
        self.n_frag = max(len(cols.names), int(cols.frag.max()) + 1 if len(cols) else 0)

    def __len__(self):
        return self.n_samples

    def n_contribs(self, s):
        return int(self.lab0[s + 1] - self.lab0[s]) - 1

    def device_columns(self):
        if self._dcols is None:
            from .observe import DeviceColumns
            self._dcols = DeviceColumns(self.cols, self.labels.device)
        return self._dcols

    def device_frag(self):
        if self._frag is None:
            self._frag = torch.from_numpy(numpy.ascontiguousarray(self.cols.frag, dtype=numpy.int64)).to(self.labels.device)
        return self._frag

    def label_of(self, s, name):
        try:
            return int(self.lab0[s]) + self.names[s].index(name)
        except ValueError:
            return None

    def counts(self):
        lab = self.labels[self.labels >= 0]
        if not lab.numel():
            return numpy.zeros(self.n_labels, dtype=numpy.int64)
        return torch.bincount(lab.to(torch.int64), minlength=self.n_labels).cpu().numpy()

    def sample(self, s):
        s = int(s)
        if not 0 <= s < self.n_samples:
            raise IndexError("sample index out of range")
        lo, hi = int(self.aln0[s]), int(self.aln0[s + 1])
        glob = self.labels[lo:hi]
        local = torch.where(glob >= 0, glob - int(self.lab0[s]), glob).to(torch.int32).contiguous()
        cr = ContribReads(self.cols_list[s], local, self.names[s], self.keys[s])
        cr.relabel(local, self.joined[lo:hi].clone())
        cr.rounds = self.rounds[s]
        return cr


def assign_reads_many(cols_list, finished, reads_list, args, pileup=None, max_bytes=COHORT_TABLES_BYTES):
    """
    assign_reads for ALL samples of a cohort in one pass over the concatenated columns -> CohortContribReads.  Opt-in;
    assign_reads is unchanged, and per sample the result is what assign_reads(cols_list[s], contribs, ...) gives: the same
    label per alignment (.sample(s).labels), names and keys.
    cols_list: the samples' alignments.AlignmentColumns; finished: assign.finish_many's list (contribs, assigned and
    row_label are read); reads_list: the samples' rows of fragments (ReadIdGroups, or the reference's lists of read ids);
    args: min_mq is read (the tables' length).
    pileup: an observe.CohortPileup made with keep_columns=True over the same cols_list: its concatenated columns and their
    upload are reused instead of uploading again.
    The labels come from alignment_labels over the concatenated arrays (alignments.concat_columns re-bases the fragments, so
    no two samples share one) and the global row labels of _cohort_label_plan: no kernel of its own.
    max_bytes: the assembly stage that follows (assemble.extend_assemblies_many, call_consensus_many,
    write_consensus_seqs_many) keeps one pileup table per global label, n_labels x L x 64 bytes (L: the longest pileup, at
    least the reference's length); the non-strict consensus' tie rule takes the same size again as scratch.  Above
    max_bytes -- default 4 GiB, a cap and not a measurement -- this function and those raise ValueError
    ("... split the cohort"): nothing is chunked silently.
    A sample without contributors has no names and no keys, and every alignment of it is labelled -1.
    """
    from .alignments import concat_columns
    from .observe import pileup_length
    cols_list = list(cols_list)
    if not cols_list or len(finished) != len(cols_list) or len(reads_list) != len(cols_list):
        raise ValueError("assign_reads_many: one finish_many result and one list of rows per sample are needed (%d samples, "
                         "%d results, %d lists)" % (len(cols_list), len(finished), len(reads_list)))
    n = len(cols_list)
    lab0, names, keys, rows = _cohort_label_plan(finished, [len(reads) for reads in reads_list])
    dcols = None
    if pileup is not None and pileup.cols is not None:
        joined, aln0, dcols = pileup.cols, pileup.aln0, pileup.dcols
        if len(aln0) != n + 1 or any(int(aln0[s + 1] - aln0[s]) != len(c) for s, c in enumerate(cols_list)):
            raise ValueError("assign_reads_many: the pileup's columns are not those of cols_list")
    else:
        joined, aln0 = concat_columns(cols_list)
    _cohort_budget("assign_reads_many", int(lab0[-1]), pileup_length(joined, args.min_mq), max_bytes)
    dev = require_gpu()
    ptrs, groups, base, row0 = [numpy.zeros(1, dtype=numpy.int64)], [], 0, 0
    for cols, reads in zip(cols_list, reads_list):
        ptr, group_frag = _row_groups(cols, reads)
        ptrs.append(ptr[1:] + row0)
        groups.append(group_frag + base)
        row0 += int(ptr[-1])
        base += max(len(cols.names), int(cols.frag.max()) + 1 if len(cols) else 0)      # (concat_columns' re-basing)
    frag_d = torch.from_numpy(numpy.ascontiguousarray(joined.frag, dtype=numpy.int64)).to(dev)
    row_label = torch.from_numpy(numpy.concatenate(rows)).to(dev)
    labels = alignment_labels(frag_d, torch.from_numpy(numpy.concatenate(ptrs)).to(dev),
                              torch.from_numpy(numpy.concatenate(groups).astype(numpy.int64)).to(dev), row_label,
                              max(base, 1))
    aln_sample = torch.from_numpy(numpy.repeat(numpy.arange(n, dtype=numpy.int32), numpy.diff(aln0))).to(dev)
    return CohortContribReads(cols_list, joined, aln0, lab0, names, keys, labels, aln_sample, dcols, frag_d, max_bytes)


# ---- bootstrap intervals for the refined proportions of a cohort (no counterpart in the reference) -----------------------------
BOOTSTRAP_MAX = 4096                # MXM_BOOTSTRAP_MAX of include/mixemt_hip_bootstrap.h: replicates per sample (a cap)
BOOTSTRAP_BYTES = 4 << 30           # default budget for the replicates' weights, linearised matrices and tables: a cap, not a
                                    # measurement


BOOTSTRAP_REFUSED = {1: "its weights are not non-negative integers",          # state[s].error of mxm_bootstrap_weights
                     2: "its weights sum to 0 or to 2^31 and more: a total in [1, 2^31) is needed"}


def _bootstrap_skip(sample, finished_one, max_rows):
    """Why bootstrap_many leaves a sample out (None: it takes part), decided on the host.  sample = (matrix, weights).
    Weights that are a device tensor are NOT read back here: mxm_bootstrap_weights checks them where they are, and
    bootstrap_many skips the sample on its error code."""
    refined = finished_one.get("refined")
    if refined is None:
        return "no refined result (args.refine_ests off, or nothing contributes)"
    n_con = len(finished_one["contribs"])
    if n_con < 1 or n_con > FINISH_KMAX or len(finished_one["sub_haps"]) != n_con:
        return "%d contributors over %d columns: 1 .. %d, each a column of its own, are taken" % (
            n_con, len(finished_one["sub_haps"]), FINISH_KMAX)
    if sample[0].n_rows > max_rows:
        return "%d rows, more than max_rows = %d" % (sample[0].n_rows, max_rows)
    wts = sample[1]
    on_device = hasattr(wts, "is_cuda") and wts.is_cuda
    if (int(wts.numel()) if on_device else numpy.asarray(wts).size) != sample[0].n_rows:
        raise ValueError("bootstrap_many: weights do not match the samples' rows")
    if on_device:
        return None
    wts = numpy.asarray(wts, dtype=numpy.float64).reshape(-1)
    if not (numpy.all(numpy.isfinite(wts)) and numpy.all(wts >= 0) and numpy.all(wts == numpy.floor(wts))):
        return BOOTSTRAP_REFUSED[1]
    if not 0 < wts.sum() < 2.0 ** 31:
        return BOOTSTRAP_REFUSED[2]
    return None


def _bootstrap_check(samples, haplogroups, who="bootstrap_many"):
    """bootstrap_many's (and support_many's) check of the matrices (host only), as finish_many makes it for its own."""
    from .preprocess import CodedMatrix
    mats = [pair[0] for pair in samples]
    if any(not isinstance(m, CodedMatrix) for m in mats) or any(m.rec.data_ptr() != mats[0].rec.data_ptr() for m in mats):
        raise ValueError("%s: the samples must be views of ONE record buffer (preprocess.build_em_records_many's "
                         "matrix and cm.rows(lo, hi) of it), as finish_many takes them" % who)
    if mats[0].n_haps != len(haplogroups):
        raise ValueError("%s: %d haplogroups for matrices of %d columns" % (who, len(haplogroups), mats[0].n_haps))


def bootstrap_many(samples, finished, haplogroups, args, n_boot=1000, seed=0, level=0.95, max_rows=None,
                   max_bytes=BOOTSTRAP_BYTES, sample_ids=None):
    """
    Percentile bootstrap intervals for the refined proportions of the samples of one finish_many call, all replicates of
    all samples in batched device passes (include/mixemt_hip_bootstrap.h) -- opt-in; the reference has no counterpart.
    A replicate resamples the sample's N_s reads with replacement (a multinomial draw over the de-duplicated rows by their
    weights: mxm_bootstrap_weights) and runs the refinement EM on the sample's reduced matrix under the resampled weights
    (mxm_em_loop_samples_narrow_boot), started at log(refined["props"]) -- the point estimate, NOT a fresh random start:
    the interval is CONDITIONAL on the detected contributor set and on the mode the point estimate sits in.
    samples, finished: finish_many's arguments and its result list; haplogroups as there.  args: tolerance, max_iter.
    n_boot: 2 .. 4096 replicates per sample.  level: the interval's coverage in (0, 1): lo / hi are the quantiles at
        (1 - level) / 2 and (1 + level) / 2 (numpy.quantile's "linear").
    seed, sample_ids: the draws of replicate b of sample s depend on (seed, sample_ids[s], b) alone; sample_ids defaults to
        the sample's index in this call, so pass ids of your own where a sample must keep its draws across calls.
    max_rows: as finish_many's (default FINISH_MAX_ROWS).  max_bytes: the call refuses up front when the replicates'
        weights, the linearised matrices and the tables need more.
    A sample takes part when it has a `refined` result, 1 .. 16 contributors (each a column of its own), at most max_rows
    rows and non-negative integer weights with a total in [1, 2^31) (weights on the host are checked there, a device tensor
    by mxm_bootstrap_weights where it is).  Everything that can be refused on the host is refused before a device is asked
    for.  Returns (boots, skipped): boots[s] is None for every other sample and skipped holds its (s, reason), in sample
    order; otherwise a dict:
        columns     the reduced matrix's column names (sub_haps)
        props_boot  [B][K] the replicates' proportions, in that column order
        lo, hi, mean, sd   [K] each (sd with ddof = 1); NaN in a column with a replicate that is not finite
        iters, done [B] each: the replicates' EM steps and stops.  done = 2 is a replicate that ran into args.max_iter: as
                    run_em reports such a run's proportions, it IS in props_boot and in the four summaries -- look at `done`
                    where only converged replicates should count
        intervals   rows [hapNN, haplogroup, proportion, lo, hi, sd] in the order of `contribs`
        seed, level, n_boot   the call's own values
    """
    n = len(samples) if samples else 0
    if not samples or len(finished) != n:
        raise ValueError("bootstrap_many: one result of finish_many per sample is needed (%d samples, %d results)"
                         % (n, len(finished)))
    if sample_ids is not None and len(sample_ids) != n:
        raise ValueError("bootstrap_many: sample_ids needs one id per sample (%d samples, %d ids)" % (n, len(sample_ids)))
    n_boot = int(n_boot)
    if n_boot < 2 or n_boot > BOOTSTRAP_MAX:
        raise ValueError("bootstrap_many: n_boot = %d: 2 .. %d replicates are taken" % (n_boot, BOOTSTRAP_MAX))
    if not 0.0 < float(level) < 1.0:
        raise ValueError("bootstrap_many: level = %r must lie in (0, 1)" % (level,))
    ids_all = list(range(n)) if sample_ids is None else [int(i) for i in sample_ids]
    if any(i < 0 or i >= 2 ** 32 for i in ids_all):
        raise ValueError("bootstrap_many: sample_ids must be 32-bit unsigned integers")
    max_rows = FINISH_MAX_ROWS if max_rows is None else int(max_rows)
    boots, skipped = [None] * n, []
    hap_index = {}
    for i, hap in enumerate(haplogroups):
        hap_index.setdefault(hap, i)
    ids, plans = [], []
    for s in range(n):
        why = _bootstrap_skip(samples[s], finished[s], max_rows)
        if why is None:
            plan = _finish_columns(finished[s]["contribs"], hap_index)
            if len(set(plan[0])) != len(plan[0]) or list(plan[2]) != list(finished[s]["sub_haps"]) \
                    or len(finished[s]["refined"]["props"]) != len(plan[0]):
                why = "a haplogroup named twice: its reduced matrix has fewer columns than contributors"
        if why is None:
            ids.append(s)
            plans.append(plan)
        else:
            skipped.append((s, why))
    if not ids:
        return boots, skipped
    _bootstrap_check([samples[s] for s in ids], haplogroups)
    ld, cols, ncol, _ = _finish_tables(plans)
    rows = [samples[s][0].n_rows for s in ids]
    total, tables = sum(rows), len(ids) * n_boot * ld
    spills = any(r * int(k) > 9216 for r, k in zip(rows, ncol))
    need = 8 * n_boot * total + (8 * total * ld if spills else 0) + (4 * 8 + 24) * tables + 8 * total * ld
    need += 4 * min(n_boot, 64) * (total + 32 * len(ids))     # (the workspace's counters: at most 32 spare rows per sample)
    if need > int(max_bytes):
        raise ValueError("bootstrap_many: %d replicates of %d samples (%d rows) need %d bytes of weights and tables, above the "
                         "budget of %d bytes (max_bytes): split the cohort or lower n_boot"
                         % (n_boot, len(ids), total, need, int(max_bytes)))

    dev = require_gpu()
    wts_d = {s: as_device(samples[s][1], torch.float64, dev).reshape(-1) for s in ids}
    while True:
        batch = _finish_batch(samples, wts_d, ids)
        wb, errors = batch.boot_weights(n_boot, seed, [ids_all[s] for s in ids])
        if not any(errors):
            break
        # device weights that the entry refused: those samples are skipped, the others drawn again without them (their
        # draws depend on their ids, not on the batch)
        skipped = sorted(skipped + [(s, BOOTSTRAP_REFUSED.get(e, "mxm_bootstrap_weights: error %d" % e))
                                    for s, e in zip(ids, errors) if e])
        keep = [j for j, e in enumerate(errors) if not e]
        ids, plans = [ids[j] for j in keep], [plans[j] for j in keep]
        if not ids:
            return boots, skipped
        ld, cols, ncol, _ = _finish_tables(plans)
    mat = batch.gather(cols, ncol, ld)
    starts = [numpy.asarray(finished[s]["refined"]["props"], dtype=numpy.float64).reshape(-1) for s in ids]
    _, ln_new, _, state, states = batch.em_loop_boot(mat, ld, ncol, wb, n_boot, starts, args.tolerance, args.max_iter)
    q_lo, q_hi = (1.0 - float(level)) / 2.0, (1.0 + float(level)) / 2.0
    x, lo, hi, mean, sd, _ = batch.boot_summary(n_boot, ld, ncol, ln_new, state, q_lo, q_hi)
    for j, s in enumerate(ids):
        k = int(ncol[j])
        column = {name: i for i, name in enumerate(plans[j][2])}
        rows_out = []
        for con in finished[s]["contribs"]:
            i = column[con[1]]
            rows_out.append([con[0], con[1], con[2], float(lo[j, i]), float(hi[j, i]), float(sd[j, i])])
        boots[s] = {"columns": list(plans[j][2]), "props_boot": x[j, :, :k].copy(), "lo": lo[j, :k].copy(), "hi": hi[j, :k].copy(),
                    "mean": mean[j, :k].copy(), "sd": sd[j, :k].copy(), "iters": numpy.array([st[1] for st in states[j]]),
                    "done": numpy.array([st[0] for st in states[j]]), "intervals": rows_out, "seed": seed, "level": level,
                    "n_boot": n_boot}
    return boots, skipped


def bootstrap(cm, wts, finished_one, haplogroups, args, **kwargs):
    """bootstrap_many for ONE sample: (its dict or None, the skip reason or None)."""
    boots, skipped = bootstrap_many([(cm, wts)], [finished_one], haplogroups, args, **kwargs)
    return boots[0], (skipped[0][1] if skipped else None)


# ---- detection bootstrap: how often each contributor is CALLED under resampled reads (no counterpart in the reference) --------
DETECT_BYTES = 4 << 30              # default budget for ONE chunk of (sample, replicate) entries: a cap, not a measurement
DETECT_LD = 64                      # row stride of the candidate tables (the widest the check takes): E x 64 tables leave the device
DETECT_SETS = 10                    # kept sets listed per sample


def _detect_skip(sample, result_one, args):
    """Why detect_many leaves a sample out (None: it takes part), decided on the host; device weights are left to
    mxm_bootstrap_weights, as _bootstrap_skip leaves them."""
    if result_one.get("route") != "batch":
        return "its first EM did not run in the batch (route %r)" % (result_one.get("route"),)
    if int(getattr(args, "n_multi", 1)) != 1:
        return "args.n_multi = %d: one EM run per sample is taken" % int(args.n_multi)
    if getattr(args, "contributors", None):
        return "args.contributors is given: there is nothing to detect"
    wts = sample[1]
    on_device = hasattr(wts, "is_cuda") and wts.is_cuda
    if (int(wts.numel()) if on_device else numpy.asarray(wts).size) != sample[0].n_rows:
        raise ValueError("detect_many: weights do not match the samples' rows")
    if on_device:
        return None
    wts = numpy.asarray(wts, dtype=numpy.float64).reshape(-1)
    if not (numpy.all(numpy.isfinite(wts)) and numpy.all(wts >= 0) and numpy.all(wts == numpy.floor(wts))):
        return BOOTSTRAP_REFUSED[1]
    if not 0 < wts.sum() < 2.0 ** 31:
        return BOOTSTRAP_REFUSED[2]
    return None


def _detect_entry_bytes(n_rows, n_haps, tile_rows, row_bytes=16):
    """What ONE (sample, replicate) entry of n_rows rows adds to a chunk: its tiles' partial sums, the vote's tables (24 H),
    the loop's four tables (32 H), the start's copy and the exponentiated proportions (16 H), `best` and the repeated
    rec_off / ndist (row_bytes per row together), and the 64-wide tables that leave the device."""
    n_tiles = (int(n_rows) + tile_rows - 1) // tile_rows
    return n_tiles * n_haps * 8 + (24 + 32 + 16) * n_haps + (4 + row_bytes) * int(n_rows) + DETECT_LD * 32 + 64


DETECT_CHUNK_ENTRIES = 65535        # entries one mxm_em_loop_samples call takes


def _detect_chunks(entry_bytes, max_bytes):
    """Contiguous chunks [e0, e1) of the entries, each within max_bytes (and within the batched loop's 65535 entries);
    ValueError when one entry does not fit."""
    chunks, e0, used = [], 0, 0
    for e, need in enumerate(entry_bytes):
        if need > max_bytes:
            raise ValueError("detect_many: one (sample, replicate) entry needs %d bytes, above the budget of %d bytes "
                             "(max_bytes): split the cohort or lower n_boot" % (need, max_bytes))
        if used + need > max_bytes or e - e0 >= DETECT_CHUNK_ENTRIES:
            chunks.append((e0, e))
            e0, used = e, 0
        used += need
    if e0 < len(entry_bytes):
        chunks.append((e0, len(entry_bytes)))
    return chunks


def _exp_as_run_em_many(ln):
    """numpy.exp over a CONTIGUOUS copy, as run_em_many exponentiates its log proportions: numpy takes another loop for a
    strided view, and the two loops need not round alike."""
    flat = numpy.ascontiguousarray(ln, dtype=numpy.float64)
    return numpy.exp(flat.reshape(-1)).reshape(flat.shape)


DETECT_FAILED = ("the EM loop did not finish", "poisoned: a NaN vote or proportion, or a loop error",
                 "more than 64 candidates", "the variant check left it alone (ncand)", "a candidate index outside the tree")


def _detect_failure(ncand, flag, done):
    """The reason a replicate is not usable (None: it is), in the order the result documents."""
    if done == 0:
        return DETECT_FAILED[0]
    if ncand < 0:
        return DETECT_FAILED[1]
    if ncand > DETECT_LD:
        return DETECT_FAILED[2]
    if flag == 1:
        return DETECT_FAILED[3]
    if flag != 0:
        return DETECT_FAILED[4]
    return None


def _detect_summary(cand, ncand, keep, flag, done, contribs, haplogroups, hap_index):
    """The host summary of ONE sample's replicates: cand [B][ld] / ncand [B] / keep [B][ld] (None: the check is off, every
    candidate is kept) / flag [B] / done [B] as they left the device; contribs: the point estimate's [[hapNN, haplogroup,
    proportion], ...].  Returns the dict of detection, n_used, n_failed, set_sizes, same_set, sets (see detect_many)."""
    n_boot = len(ncand)
    est = [hap_index[con[1]] for con in contribs]
    est_prop = {}
    for con in contribs:
        est_prop.setdefault(hap_index[con[1]], con[2])
    n_cand, n_kept = {h: 0 for h in est}, {h: 0 for h in est}
    failed, sizes, sets, n_used, same = {}, {}, {}, 0, 0
    for b in range(n_boot):
        why = _detect_failure(int(ncand[b]), int(flag[b]), int(done[b]))
        if why is not None:
            failed[why] = failed.get(why, 0) + 1
            continue
        n_used += 1
        kept = []
        for i in range(int(ncand[b])):
            h = int(cand[b][i])
            n_cand[h] = n_cand.get(h, 0) + 1
            n_kept.setdefault(h, 0)
            if keep is None or keep[b][i]:
                n_kept[h] += 1
                kept.append(h)
        key = tuple(sorted(kept))
        sizes[len(key)] = sizes.get(len(key), 0) + 1
        sets[key] = sets.get(key, 0) + 1                     # (dict order = first occurrence)
        same += 1 if set(key) == set(est) and len(key) == len(set(est)) else 0
    rows = [[haplogroups[h], n_cand[h], n_kept[h], h in est_prop, est_prop.get(h)]
            for h in sorted(n_cand, key=lambda h: (-n_kept[h], h))]
    top = sorted(sets.items(), key=lambda kv: -kv[1])[:DETECT_SETS]          # (stable: ties by first occurrence)
    return {"detection": rows, "n_used": n_used, "n_failed": failed, "set_sizes": dict(sorted(sizes.items())), "same_set": same,
            "sets": [([haplogroups[h] for h in key], count) for key, count in top]}


def detect_many(samples, results, finished, haplogroups, args, n_boot=200, seed=0, level=0.95, obs=None, phylo=None,
                var_tables=None, sample_ids=None, inits=None, max_bytes=DETECT_BYTES):
    """
    A bootstrap of the DETECTION: how often each haplogroup is called a contributor when the sample's reads are drawn
    again, for the samples of one run_em_many / finish_many call, all replicates in batched device passes -- opt-in; the
    reference has no counterpart.  Per replicate: the sample's N_s reads are resampled with replacement
    (mxm_bootstrap_weights), the WIDE EM over all haplogroups runs under the resampled weights (mxm_em_loop_samples; the
    entries of the batch are (sample, replicate) pairs over the sample's records, offsets repeated, nothing copied), the
    rows vote (mxm_votes_samples), the candidates are formed on the device (mxm_detect_candidates: args.min_reads, checking
    order) and, with args.var_check, checked there (mxm_check_variants_entries).  Only 64-wide tables leave the device.
    WHAT THE FREQUENCIES ARE CONDITIONAL ON: the variant check runs against the OBSERVED pileup -- pileup noise is not
    resampled -- and every replicate stops by the rule of args.tolerance / args.max_iter from a warm start.  They are NOT
    the call frequencies of the full pipeline under resampled alignments.
    samples, results: run_em_many's arguments and results; finished: finish_many's results (its contributors are the point
        estimate the replicates are compared with).  args: min_reads, var_check (min_var_reads, frac_var_reads, var_fraction,
        var_count), tolerance, max_iter, n_multi, contributors.
    n_boot: 2 .. 4096 replicates per sample.  seed, sample_ids: replicate b of sample s depends on (seed, sample_ids[s], b)
        alone (sample_ids defaults to the index in this call): n_boot = 8 reproduces the replicates of n_boot = 4.
    inits: None starts every replicate of s at results[s]["props"] renormalised to sum 1 -- for fixed components the wide
        likelihood is concave in the proportions, so its maximum does not depend on the start; the warm start only shortens
        the way -- or a list with [H] proportions per sample (None: the default).
    obs / phylo / var_tables: with args.var_check, obs must be an observe.CohortPileup (table s is sample s's; anything else
        is a ValueError) and phylo (or var_tables, a VarCheckTables built with a device) is required.
    level: coverage of lo / hi below.  max_bytes: entries (s, b) are taken in order in contiguous chunks of at most this many
        bytes (_detect_entry_bytes each); ValueError when one entry does not fit.  The chunking changes no result.
    A row of resampled weight 0 STAYS in the batch with weight 0: it still counts for `first`.  That differs from deleting
    the row only between candidates of exactly equal proportions, and for args.min_reads <= 0, where a haplogroup that won
    only weight-0 rows is a candidate.
    A sample takes part when results[s]["route"] == "batch", args.n_multi == 1, args.contributors is empty and its weights
    are non-negative integers with a total in [1, 2^31) (device weights are checked by mxm_bootstrap_weights).  Returns
    (detect, skipped): detect[s] is None for every other sample and skipped holds its (s, reason); otherwise a dict:
        detection   rows [haplogroup, n_candidate, n_kept, in_estimate, estimate_prop_or_None] for every haplogroup that is a
                    candidate in a usable replicate or among finished[s]["contribs"], by descending n_kept, then index;
                    with the check off n_kept == n_candidate
        n_used      usable replicates, the denominator: flag == 0, 0 <= ncand <= 64, done != 0; n_failed: {reason: count}
                    of the others, which appear in no count
        set_sizes   {size of the kept set: replicates};  same_set: replicates whose kept set is the point estimate's
        sets        the ten most frequent kept sets as ([haplogroups by index], count), ties by first occurrence
        columns, props_boot [B][K]   the point estimate's contributors and their WIDE-EM proportions per replicate,
                    unconditional on the set (NaN for a replicate whose loop did not finish)
        lo, hi, mean, sd [K]   mxm_bootstrap_summary over props_boot when 1 <= K <= 16; otherwise absent, and
                    `summary` says why (it is "mxm_bootstrap_summary" when they are there)
        cand [B][64], ncand [B], keep [B][64], flag [B], cand_props [B][64]   the replicates' own tables (cand_props: exp of
                    the loop's log theta_{k+1} formed on the host, as run_em_many forms props)
        iters, done [B]; seed, level, n_boot; var_check: "observed pileup" or "off"
    """
    from . import em
    from .observe import CohortPileup
    n = len(samples) if samples else 0
    if not samples or len(results) != n or len(finished) != n:
        raise ValueError("detect_many: one result of run_em_many and one of finish_many per sample are needed (%d samples, %d and "
                         "%d results)" % (n, len(results), len(finished) if finished is not None else 0))
    if sample_ids is not None and len(sample_ids) != n:
        raise ValueError("detect_many: sample_ids needs one id per sample (%d samples, %d ids)" % (n, len(sample_ids)))
    if inits is not None and len(inits) != n:
        raise ValueError("detect_many: inits needs one entry per sample (%d samples, %d entries)" % (n, len(inits)))
    n_boot = int(n_boot)
    if n_boot < 2 or n_boot > BOOTSTRAP_MAX:
        raise ValueError("detect_many: n_boot = %d: 2 .. %d replicates are taken" % (n_boot, BOOTSTRAP_MAX))
    if not 0.0 < float(level) < 1.0:
        raise ValueError("detect_many: level = %r must lie in (0, 1)" % (level,))
    ids_all = list(range(n)) if sample_ids is None else [int(i) for i in sample_ids]
    if any(i < 0 or i >= 2 ** 32 for i in ids_all):
        raise ValueError("detect_many: sample_ids must be 32-bit unsigned integers")
    max_bytes = int(max_bytes)
    checked = bool(args.var_check)
    if checked:
        if not isinstance(obs, CohortPileup):
            raise ValueError("detect_many: args.var_check needs obs= an observe.CohortPileup (the pileups stay on the device)")
        if len(obs) != n:
            raise ValueError("detect_many: obs needs one table per sample (%d samples, %d tables)" % (n, len(obs)))
        if phylo is None and var_tables is None:
            raise ValueError("detect_many: the variant check needs phylo= (or var_tables=)")
        if var_tables is not None and (var_tables.n_haps != len(haplogroups) or var_tables.key_ptr is None):
            raise ValueError("detect_many: var_tables must be built with a device for the samples' %d haplogroups" % len(haplogroups))
        if obs.L > VAR_CHECK_MAX_L:
            raise ValueError("detect_many: a pileup of %d positions: the check kernel takes at most %d" % (obs.L, VAR_CHECK_MAX_L))
    hap_index = {}
    for i, hap in enumerate(haplogroups):
        hap_index.setdefault(hap, i)
    n_haps = len(haplogroups)
    detect, skipped, ids = [None] * n, [], []
    for s in range(n):
        why = _detect_skip(samples[s], results[s], args)
        if why is None:
            ids.append(s)
        else:
            skipped.append((s, why))
    if not ids:
        return detect, skipped
    _bootstrap_check([samples[s] for s in ids], haplogroups, who="detect_many")
    starts = {}
    for s in ids:
        start = numpy.asarray(results[s]["props"] if inits is None or inits[s] is None else inits[s], dtype=numpy.float64).reshape(-1)
        if start.shape != (n_haps,) or not numpy.all(numpy.isfinite(start)) or numpy.any(start < 0) or not start.sum() > 0:
            raise ValueError("detect_many: the start of sample %d must be %d finite non-negative proportions with a positive sum"
                             % (s, n_haps))
        starts[s] = start / start.sum()
    lib = _lib.load()
    tile_rows = int(lib.mxm_samples_tile_rows())
    mat0 = samples[ids[0]][0]
    row_bytes = mat0.rec_off.element_size() + mat0.ndist.element_size()
    for s in ids:                                            # (the one-entry refusal needs no device either)
        need = _detect_entry_bytes(samples[s][0].n_rows, n_haps, tile_rows, row_bytes)
        if need > max_bytes:
            _detect_chunks([need], max_bytes)

    dev = require_gpu()
    if checked:
        if var_tables is None:
            var_tables = VarCheckTables.build(phylo, haplogroups, dev)
        if var_tables is None or var_tables.key_ptr is None:
            raise ValueError("detect_many: the tree has a derived allele outside ACGT: the device check cannot take it")
        if var_tables.max_pos >= obs.L:
            raise ValueError("detect_many: the tree's variants reach past the pileup (L = %d)" % obs.L)
    wts_d = {s: as_device(samples[s][1], torch.float64, dev).reshape(-1) for s in ids}
    while True:
        batch = _finish_batch(samples, wts_d, ids)
        wb, errors = batch.boot_weights(n_boot, seed, [ids_all[s] for s in ids])
        if not any(errors):
            break
        skipped = sorted(skipped + [(s, BOOTSTRAP_REFUSED.get(e, "mxm_bootstrap_weights: error %d" % e))
                                    for s, e in zip(ids, errors) if e])
        ids = [s for s, e in zip(ids, errors) if not e]
        if not ids:
            return detect, skipped
    del batch
    n_part = len(ids)
    rows = [samples[s][0].n_rows for s in ids]
    row0 = numpy.concatenate([[0], numpy.cumsum(rows)]).astype(numpy.int64)
    ln0_h, p0_h = em.log_inits(numpy.stack([starts[s] for s in ids]))
    ln0_d, p0_d = torch.from_numpy(ln0_h).to(dev), torch.from_numpy(p0_h).to(dev)
    # the point estimate's contributor columns, one width for all samples (pad: column 0, masked on the host)
    est = [[hap_index[con[1]] for con in finished[s]["contribs"]] for s in ids]
    width = max([len(cols) for cols in est] + [1])
    est_h = numpy.zeros((n_part, width), dtype=numpy.int64)
    for j, cols in enumerate(est):
        est_h[j, :len(cols)] = cols
    est_d = torch.from_numpy(est_h).to(dev)
    n_entries = n_part * n_boot
    entry_bytes = [_detect_entry_bytes(rows[e // n_boot], n_haps, tile_rows, row_bytes) for e in range(n_entries)]
    ld = DETECT_LD
    out = {"cand": [], "ncand": [], "keep": [], "flag": [], "ln_cand": [], "ln_est": [], "state": [], "states": []}
    var_count = getattr(args, "var_count", None)
    for e0, e1 in _detect_chunks(entry_bytes, max_bytes):
        count = e1 - e0
        sample_of = numpy.arange(e0, e1) // n_boot                      # (index among the participating samples)
        parts_off, parts_nd = [], []
        for j in range(int(sample_of[0]), int(sample_of[-1]) + 1):
            reps = int((sample_of == j).sum())
            parts_off.append(samples[ids[j]][0].rec_off.repeat(reps))
            parts_nd.append(samples[ids[j]][0].ndist.repeat(reps))
        rows_h = numpy.array([rows[j] for j in sample_of], dtype=numpy.int64)
        c_row0 = numpy.concatenate([[0], numpy.cumsum(rows_h)]).astype(numpy.int64)
        j0, b0 = int(sample_of[0]), e0 - int(sample_of[0]) * n_boot
        w0 = n_boot * int(row0[j0]) + b0 * rows[j0]                      # (wb's layout: the chunk's weights are one slice)
        wts_c = wb[w0:w0 + int(c_row0[-1])]
        off_c, nd_c = torch.cat(parts_off), torch.cat(parts_nd)
        of_d = torch.from_numpy(sample_of).to(dev)
        loop = em.SampleBatch(mat0.rec, off_c, nd_c, wts_c, c_row0, n_haps)
        ln_cur, ln_new, state, states = loop.em_loop_device(ln0_d[of_d], p0_d[of_d], args.tolerance, args.max_iter)
        vote = em.SampleFinish(mat0.rec, off_c, nd_c, wts_c, None, c_row0, n_haps)
        votes, first, _ = vote.votes_device(ln_cur)
        props = torch.exp(ln_new)
        cand = torch.zeros((count, ld), dtype=torch.int32, device=dev)
        ncand = torch.zeros(count, dtype=torch.int32, device=dev)
        cprop = torch.zeros((count, ld), dtype=torch.float64, device=dev)
        _lib.check(lib.mxm_detect_candidates(votes.data_ptr(), first.data_ptr(), rows_h.ctypes.data, props.data_ptr(),
                                             state.data_ptr(), count, n_haps, float(args.min_reads), ld, cand.data_ptr(),
                                             ncand.data_ptr(), cprop.data_ptr(), current_stream()), "mxm_detect_candidates")
        keep = flag = None
        if checked:
            keep = torch.zeros((count, ld), dtype=torch.uint8, device=dev)
            flag = torch.zeros(count, dtype=torch.int32, device=dev)
            table_of = numpy.array([ids[j] for j in sample_of], dtype=numpy.int32)
            _lib.check(lib.mxm_check_variants_entries(
                obs.counts.data_ptr(), int(obs.counts.shape[0]), int(obs.L), var_tables.key_ptr.data_ptr(), var_tables.key.data_ptr(),
                var_tables.n_haps, var_tables.site.data_ptr(), var_tables.site_key.data_ptr(), len(var_tables.site_h),
                var_tables.max_pos, table_of.ctypes.data, count, cand.data_ptr(), ncand.data_ptr(), ld, float(args.min_var_reads),
                float(args.frac_var_reads), float(args.var_fraction), 0 if var_count is None else 1,
                0 if var_count is None else int(var_count), keep.data_ptr(), None, None, flag.data_ptr(), current_stream()),
                "mxm_check_variants_entries")
        # only E x 64 tables leave the device: the lists, and log theta_{k+1} at the lists and at the estimate's columns
        slot_ok = torch.arange(ld, device=dev).reshape(1, ld) < ncand.clamp(0, ld).reshape(-1, 1)
        at = torch.where(slot_ok, cand.to(torch.int64), torch.zeros_like(cand, dtype=torch.int64)).clamp(0, n_haps - 1)
        out["ln_cand"].append(torch.gather(ln_new, 1, at).cpu().numpy())
        out["ln_est"].append(torch.gather(ln_new, 1, est_d[of_d]))
        out["state"].append(state)
        out["cand"].append(cand.cpu().numpy())
        out["ncand"].append(ncand.cpu().numpy())
        out["keep"].append(keep.cpu().numpy().astype(bool) if checked else None)
        out["flag"].append(flag.cpu().numpy() if checked else numpy.zeros(count, dtype=numpy.int32))
        out["states"].extend(states)
        del loop, vote, votes, first, props, ln_cur, ln_new

    cand_h, ncand_h = numpy.concatenate(out["cand"]), numpy.concatenate(out["ncand"])
    keep_h = numpy.concatenate(out["keep"]) if checked else None
    flag_h, ln_cand = numpy.concatenate(out["flag"]), numpy.concatenate(out["ln_cand"])
    ln_est_d = torch.cat(out["ln_est"])
    ln_est = ln_est_d.cpu().numpy()
    done_h = numpy.array([st[0] for st in out["states"]])
    iters_h = numpy.array([st[1] for st in out["states"]])
    # lo / hi / mean / sd through the bootstrap's summary entry, for the samples whose estimate has 1 .. 16 contributors
    summary = {}
    small = [j for j in range(n_part) if 1 <= len(est[j]) <= FINISH_KMAX]
    if small:
        s_ld = 4 if max(len(est[j]) for j in small) <= 4 else (8 if max(len(est[j]) for j in small) <= 8 else 16)
        table = torch.full((len(small), n_boot, s_ld), -float("inf"), dtype=torch.float64, device=dev)
        state_all = torch.cat(out["state"]).reshape(n_entries, -1)
        for i, j in enumerate(small):
            k = len(est[j])
            table[i, :, :k] = ln_est_d[j * n_boot:(j + 1) * n_boot, :k]
        st_small = torch.cat([state_all[j * n_boot:(j + 1) * n_boot] for j in small]).contiguous()
        ncol = numpy.array([len(est[j]) for j in small], dtype=numpy.int32)
        x = torch.zeros((len(small), n_boot, s_ld), dtype=torch.float64, device=dev)
        four = torch.full((4, len(small), s_ld), float("nan"), dtype=torch.float64, device=dev)
        sflag = torch.zeros(len(small), dtype=torch.int32, device=dev)
        q_lo, q_hi = (1.0 - float(level)) / 2.0, (1.0 + float(level)) / 2.0
        _lib.check(lib.mxm_bootstrap_summary(len(small), n_boot, s_ld, ncol.ctypes.data, table.data_ptr(), st_small.data_ptr(),
                                             q_lo, q_hi, x.data_ptr(), four[0].data_ptr(), four[1].data_ptr(), four[2].data_ptr(),
                                             four[3].data_ptr(), sflag.data_ptr(), current_stream()), "mxm_bootstrap_summary")
        four_h = four.cpu().numpy()
        for i, j in enumerate(small):
            summary[j] = four_h[:, i, :len(est[j])].copy()
    for j, s in enumerate(ids):
        sl = slice(j * n_boot, (j + 1) * n_boot)
        res = _detect_summary(cand_h[sl], ncand_h[sl], keep_h[sl] if checked else None, flag_h[sl], done_h[sl],
                              finished[s]["contribs"], haplogroups, hap_index)
        k = len(est[j])
        props_boot = _exp_as_run_em_many(ln_est[sl, :k])
        props_boot[done_h[sl] == 0] = numpy.nan
        width_ok = numpy.arange(ld).reshape(1, ld) < numpy.clip(ncand_h[sl], 0, ld).reshape(-1, 1)
        res.update({"columns": [con[1] for con in finished[s]["contribs"]], "props_boot": props_boot,
                    "cand": cand_h[sl].copy(), "ncand": ncand_h[sl].copy(), "flag": flag_h[sl].copy(),
                    "keep": keep_h[sl].copy() if checked else width_ok,
                    "cand_props": numpy.where(width_ok, _exp_as_run_em_many(ln_cand[sl]), numpy.nan),
                    "iters": iters_h[sl].copy(), "done": done_h[sl].copy(), "seed": seed, "level": level, "n_boot": n_boot,
                    "var_check": "observed pileup" if checked else "off"})
        if j in summary:
            res.update({"lo": summary[j][0], "hi": summary[j][1], "mean": summary[j][2], "sd": summary[j][3],
                        "summary": "mxm_bootstrap_summary"})
        else:
            res["summary"] = "omitted: %d contributors in the point estimate, the summary entry takes 1 .. %d" % (k, FINISH_KMAX)
        detect[s] = res
    return detect, skipped


def detect(cm, wts, result_one, finished_one, haplogroups, args, **kwargs):
    """detect_many for ONE sample: (its dict or None, the skip reason or None)."""
    for key in ("inits", "sample_ids"):
        if kwargs.get(key) is not None:
            kwargs[key] = [kwargs[key]]
    found, skipped = detect_many([(cm, wts)], [result_one], [finished_one], haplogroups, args, **kwargs)
    return found[0], (skipped[0][1] if skipped else None)


# ---- contributor support: nested-model fits over subsets of the reduced matrix (no counterpart in the reference) ---------------
SUPPORT_MAX_FITS = 256              # MXM_SUPPORT_MAX_FITS of include/mixemt_hip_support.h: fits per sample (a cap: 2^8 - 1 subsets)
SUPPORT_ALL_KMAX = 8                # models="all" enumerates 2^K - 1 subsets: refused above this many contributors
SUPPORT_BYTES = 4 << 30             # default budget for the masks, the tables, the gathered matrices and the fits' E: a cap
SUPPORT_MAX_ROWS = 100000           # FINISH_MAX_ROWS: one sample of 10^5 rows, every fit through its own slice of E, was measured at
                                    # 0.34 of the loop of gather / em_loop / logsumexp per (sample, model); nothing larger was
                                    # measured (profiles/samples/support.md)


def _support_skip(sample, finished_one, max_rows):
    """Why support_many leaves a sample out (None: it takes part), decided on the host: bootstrap_many's rule without the
    integer-weight condition.  Weights that are a device tensor are not read back."""
    refined = finished_one.get("refined")
    if refined is None:
        return "no refined result (args.refine_ests off, or nothing contributes)"
    n_con = len(finished_one["contribs"])
    if n_con < 1 or n_con > FINISH_KMAX or len(finished_one["sub_haps"]) != n_con:
        return "%d contributors over %d columns: 1 .. %d, each a column of its own, are taken" % (
            n_con, len(finished_one["sub_haps"]), FINISH_KMAX)
    if len(set(con[1] for con in finished_one["contribs"])) != n_con:
        return "a haplogroup named twice: its reduced matrix has fewer columns than contributors"
    if sample[0].n_rows > max_rows:
        return "%d rows, more than max_rows = %d" % (sample[0].n_rows, max_rows)
    wts = sample[1]
    on_device = hasattr(wts, "is_cuda") and wts.is_cuda
    if (int(wts.numel()) if on_device else numpy.asarray(wts).size) != sample[0].n_rows:
        raise ValueError("support_many: weights do not match the samples' rows")
    if not on_device:
        wts = numpy.asarray(wts, dtype=numpy.float64).reshape(-1)
        if not (numpy.all(numpy.isfinite(wts)) and numpy.all(wts >= 0)):
            return "its weights are not non-negative finite numbers"
    return None


def _support_plan(finished_one, hap_index, models, n_extra, extra, haplogroups=None):
    """One sample's fits, host only: (cols, names, masks, model_names, extras, truncated).  cols / names: the candidate
    columns (contributors, then extras) in ASCENDING haplogroup index, as the reduced matrix keeps them; masks[i]: fit i's
    bits over those columns; model_names[i]: its haplogroups in column order.  vote_order may hold haplogroup indexes (as
    finish_many returns it: `haplogroups` then names them) or names."""
    contribs = [con[1] for con in finished_one["contribs"]]
    explicit = not isinstance(models, str)
    if extra is not None:
        wanted = list(extra)
    elif n_extra and int(n_extra) > 0:
        voted = [hap if isinstance(hap, str) else haplogroups[int(hap)] for hap in finished_one["vote_order"]]
        wanted = [hap for hap in voted if hap not in contribs][:int(n_extra)]
    else:
        wanted = []
    if explicit:                                          # a model may name haplogroups beyond the extras: they become extras
        fits = [tuple(fit) for fit in models]
        for fit in fits:
            wanted += [hap for hap in fit if hap not in contribs and hap not in wanted]
    extras = []
    for hap in wanted:
        if hap not in hap_index:
            raise ValueError("support_many: Unknown haplogroup '%s'" % (hap,))
        if hap not in contribs and hap not in extras:
            extras.append(hap)
    room = FINISH_KMAX - len(contribs)
    extras, truncated = extras[:room], extras[room:]
    cand = contribs + extras
    order = sorted(range(len(cand)), key=lambda k: hap_index[cand[k]])
    names = [cand[k] for k in order]
    bit = {hap: i for i, hap in enumerate(names)}
    full = tuple(contribs)
    if explicit:
        for fit in fits:
            if not fit or len(set(fit)) != len(fit):
                raise ValueError("support_many: a model needs at least one haplogroup, each named once: %r" % (fit,))
            gone = [hap for hap in fit if hap not in bit]
            if gone:
                raise ValueError("support_many: the model %r needs more than %d candidate columns (%s left out)"
                                 % (fit, FINISH_KMAX, ", ".join(gone)))
    elif models == "all":
        if len(contribs) > SUPPORT_ALL_KMAX:
            raise ValueError("support_many: models='all' enumerates every subset: at most %d contributors, not %d"
                             % (SUPPORT_ALL_KMAX, len(contribs)))
        fits = [full] + [tuple(contribs[i] for i in range(len(contribs)) if (sub >> i) & 1)
                         for sub in range(1, (1 << len(contribs)) - 1)]
    elif models in ("drop-one", "add-one"):
        fits = [full]
        if len(contribs) > 1:
            fits += [tuple(hap for hap in contribs if hap != out) for out in contribs]
        if models == "add-one":
            fits += [full + (hap,) for hap in extras]
    else:
        raise ValueError("support_many: models must be 'drop-one', 'add-one', 'all' or a list of name tuples per sample, "
                         "not %r" % (models,))
    masks = [sum(1 << bit[hap] for hap in fit) for fit in fits]
    model_names = [tuple(hap for hap in names if hap in fit) for fit in fits]
    return [hap_index[hap] for hap in names], names, masks, model_names, extras, truncated


def support_lrt_p(lrt):
    """The p-value of a likelihood-ratio statistic for ONE proportion tested at the boundary p_k = 0: under the null the
    statistic follows the mixture 1/2 chi2_0 + 1/2 chi2_1 (Self & Liang 1987), so p = 1/2 P(chi2_1 > lrt) =
    1/2 erfc(sqrt(max(lrt, 0) / 2)); lrt <= 0 gives 0.5."""
    import math
    return 0.5 * math.erfc(math.sqrt(max(float(lrt), 0.0) / 2.0))


def support_many(samples, finished, haplogroups, args, models="drop-one", n_extra=0, extra=None, max_rows=None,
                 max_bytes=SUPPORT_BYTES):
    """
    Is a reported contributor supported by the data, and did the vote miss one?  For the samples of one finish_many call:
    refinement fits over SUBSETS of each sample's reduced matrix -- the full contributor set, each contributor left out,
    optionally each of a few runner-up haplogroups added -- with their maximised log-likelihoods, all fits of all samples
    in batched device passes (include/mixemt_hip_support.h) -- opt-in; the reference has no counterpart.
    samples, finished: finish_many's arguments and its result list; haplogroups as there.  args: tolerance, max_iter.
    models: "drop-one" (the full set and each contributor left out; one contributor: the full fit only), "add-one" (those
        and the full set with each extra added), "all" (every non-empty subset of the contributors; refused above 8
        contributors), or a list with, per sample, a list of tuples of haplogroup names.
    extra: per sample a list of haplogroup names; else the extras are the first n_extra haplogroups of
        finished[s]["vote_order"] that are not contributors.  Contributors plus extras are capped at 16 columns; what was
        cut is reported in `truncated_extras`.
    Every fit starts UNIFORM over its columns: for fixed components the mixture log-likelihood is concave in the proportions,
    so the maximum does not depend on the start; no random numbers are drawn and numpy's global stream is not advanced.
    max_rows: as finish_many's (default SUPPORT_MAX_ROWS).  max_bytes: the call refuses up front when the masks, the
    tables, the gathered matrices and -- when a sample exceeds the loop's LDS -- the fits' linearised copies need more.
    A sample takes part when it has a `refined` result, 1 .. 16 contributors (each a column of its own), at most max_rows
    rows and non-negative finite weights.  Everything that can be refused on the host is refused before a device is asked
    for.  Returns (support, skipped): support[s] is None for every other sample and skipped holds its (s, reason), in
    sample order; otherwise a dict:
        columns     the candidate columns' names, in the gathered matrix's order (ascending haplogroup index)
        n_eff       the sum of the sample's weights
        models      per fit a dict: names (in column order), props, loglik, iters, done, bic = -2 ll + (|m| - 1) log n_eff,
                    aic = -2 ll + 2 (|m| - 1)
        best_bic    the index in `models` of the smallest bic
        drop        rows [hapNN, haplogroup, proportion, lrt, p] in the order of `contribs`, lrt = 2 (ll_full - ll_drop),
                    for every contributor whose drop-one fit (and the full fit) is among the models
        add         rows [haplogroup, its proportion in the larger fit, lrt, p], lrt = 2 (ll_add - ll_full)
        truncated_extras   the extras that did not fit the 16 columns
    p = 1/2 erfc(sqrt(max(lrt, 0) / 2)): the null sits on the boundary p_k = 0, where the statistic follows
    1/2 chi2_0 + 1/2 chi2_1.  lrt is reported RAW: both fits stop at args.tolerance, not at their maxima, so at a loose
    tolerance it can come out slightly negative (p is then 0.5).
    WHAT THE NUMBERS ASSUME: the fragments are treated as independent draws from the mixture; reads that share an error
    process or a PCR ancestor are not, and lrt then overstates the evidence.  De-duplication does not change ll: a row of
    weight w counts exactly as w equal rows.
    """
    import math
    n = len(samples) if samples else 0
    if not samples or len(finished) != n:
        raise ValueError("support_many: one result of finish_many per sample is needed (%d samples, %d results)"
                         % (n, len(finished)))
    explicit = not isinstance(models, str)
    if explicit and len(models) != n:
        raise ValueError("support_many: models needs one list of name tuples per sample (%d samples, %d lists)" % (n, len(models)))
    if extra is not None and len(extra) != n:
        raise ValueError("support_many: extra needs one list of names per sample (%d samples, %d lists)" % (n, len(extra)))
    max_rows = SUPPORT_MAX_ROWS if max_rows is None else int(max_rows)
    support, skipped = [None] * n, []
    hap_index = {}
    for i, hap in enumerate(haplogroups):
        hap_index.setdefault(hap, i)
    ids, plans = [], []
    for s in range(n):
        why = _support_skip(samples[s], finished[s], max_rows)
        if why is None:
            ids.append(s)
            plans.append(_support_plan(finished[s], hap_index, models[s] if explicit else models, n_extra,
                                       None if extra is None else extra[s], haplogroups))
        else:
            skipped.append((s, why))
    if not ids:
        return support, skipped
    n_fits = max(len(plan[2]) for plan in plans)
    if n_fits > SUPPORT_MAX_FITS:
        raise ValueError("support_many: %d fits for one sample: 1 .. %d are taken" % (n_fits, SUPPORT_MAX_FITS))
    _bootstrap_check([samples[s] for s in ids], haplogroups, who="support_many")
    ld, cols, ncol, _ = _finish_tables([(plan[0], list(range(len(plan[0]))), plan[1]) for plan in plans])
    masks = numpy.zeros((len(ids), n_fits), dtype=numpy.uint32)
    for j, plan in enumerate(plans):
        masks[j, :len(plan[2])] = plan[2]
    rows = [samples[s][0].n_rows for s in ids]
    total, tables = sum(rows), len(ids) * n_fits * ld
    spills = any(r * int(k) > 9216 for r, k in zip(rows, ncol))
    need = 4 * len(ids) * n_fits + (3 * 8 + 24) * tables + 8 * len(ids) * n_fits + 8 * total * ld
    need += 8 * n_fits * total * ld if spills else 0
    if need > int(max_bytes):
        raise ValueError("support_many: %d fits of %d samples (%d rows) need %d bytes of masks, tables and matrices, above the "
                         "budget of %d bytes (max_bytes): split the cohort or ask for fewer models"
                         % (n_fits, len(ids), total, need, int(max_bytes)))

    dev = require_gpu()
    wts_d = {s: as_device(samples[s][1], torch.float64, dev).reshape(-1) for s in ids}
    batch = _finish_batch(samples, wts_d, ids)
    mat = batch.gather(cols, ncol, ld)
    bits = (masks[:, :, None] >> numpy.arange(ld, dtype=numpy.uint32)[None, None, :]) & 1
    size = numpy.maximum(bits.sum(axis=2, keepdims=True), 1)
    starts = [(bits[j] / size[j])[:, :int(ncol[j])] for j in range(len(ids))]
    _, ln_new, states = batch.em_loop_masks(mat, ld, ncol, masks, starts, args.tolerance, args.max_iter)
    ll, n_eff = batch.loglik_masks(mat, ld, ncol, masks, ln_new)
    for j, s in enumerate(ids):
        _, names, fit_masks, fit_names, extras, truncated = plans[j]
        column = {hap: i for i, hap in enumerate(names)}
        fits, index = [], {}
        for b, fit in enumerate(fit_names):
            free = len(fit) - 1
            at = [column[hap] for hap in fit]
            value = float(ll[j, b])
            fits.append({"names": fit, "props": numpy.exp(ln_new[j, b, at]), "loglik": value, "iters": int(states[j][b][1]),
                         "done": int(states[j][b][0]), "bic": -2.0 * value + (free * math.log(float(n_eff[j])) if free else 0.0),
                         "aic": -2.0 * value + 2.0 * free})
            index.setdefault(frozenset(fit), b)
        contribs = finished[s]["contribs"]
        full = index.get(frozenset(con[1] for con in contribs))
        drop, add = [], []
        if full is not None:
            everyone = frozenset(con[1] for con in contribs)
            for con in contribs:
                b = index.get(everyone - {con[1]}) if len(contribs) > 1 else None
                if b is not None:
                    lrt = 2.0 * (fits[full]["loglik"] - fits[b]["loglik"])
                    drop.append([con[0], con[1], con[2], lrt, support_lrt_p(lrt)])
            for hap in extras:
                b = index.get(everyone | {hap})
                if b is not None:
                    lrt = 2.0 * (fits[b]["loglik"] - fits[full]["loglik"])
                    add.append([hap, float(fits[b]["props"][fits[b]["names"].index(hap)]), lrt, support_lrt_p(lrt)])
        support[s] = {"columns": list(names), "n_eff": float(n_eff[j]), "models": fits,
                      "best_bic": min(range(len(fits)), key=lambda b: (fits[b]["bic"] != fits[b]["bic"], fits[b]["bic"])),
                      "drop": drop, "add": add, "truncated_extras": list(truncated)}
    return support, skipped


def support(cm, wts, finished_one, haplogroups, args, **kwargs):
    """support_many for ONE sample: (its dict or None, the skip reason or None).  models / extra, where given as lists, are
    this sample's own (a list of name tuples; a list of names)."""
    if "models" in kwargs and not isinstance(kwargs["models"], str):
        kwargs["models"] = [kwargs["models"]]
    if kwargs.get("extra") is not None:
        kwargs["extra"] = [kwargs["extra"]]
    out, skipped = support_many([(cm, wts)], [finished_one], haplogroups, args, **kwargs)
    return out[0], (skipped[0][1] if skipped else None)
